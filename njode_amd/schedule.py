"""
Host-side time grid of one NJ-ODE pass.

``NJODE.forward`` in the reference keeps a float64 Python clock
(``models.py:430-439, 497-505``): Euler steps of ``delta_t`` while the clock is
more than one step away from the next observation time, then one partial step
onto it; the loop guard is ``current_time < obs_time - 1e-10 * delta_t``.  The
kernels consume that clock as fp32 arrays, rounded exactly where ATen rounds
(python-float operands of fp32 tensor ops are cast to fp32):

    step_dt[k]  = fp32(delta_t_k)                 (h + delta_t_ * f(...))
    step_t[k]   = fp32(current_time before k)     (current_time - tau)
    time_f32[i] = fp32(times[i])                  (tau[i_obs] = obs_time)
    k_jump[i]   = number of Euler steps completed when jump i happens

``path_t`` is the reference's ``path_t`` output (float64, first entry 0).
"""
import collections

import numpy as np
import torch

from . import _lib

def _walk_clock(times, delta_t, T, until_T, strict=False):
    """The float64 clock of one pass: (step lengths, clock before each step, k_jump, path_t,
    row_of_jump) as Python lists.  ``strict``: ``ValueError`` for an observation time the clock
    has already reached (the reference's conditional-expectation walk skips those)."""
    dts, ts, k_jump, path_t, row_of_jump = [], [], [], [0.0], []
    now = 0.0

    def walk(now, target):
        guard = target - 1e-10 * delta_t
        while now < guard:
            step = delta_t if now < target - delta_t else target - now
            dts.append(step)
            ts.append(now)
            now = now + step
            path_t.append(now)
        return now

    for obs_time in times:
        if strict and not obs_time > now:
            raise ValueError('observation times must be strictly increasing and positive '
                             '({!r} after the clock reached {!r})'.format(float(obs_time), now))
        now = walk(now, obs_time)
        k_jump.append(len(dts))
        row_of_jump.append(len(path_t))
        path_t.append(obs_time)
    if until_T:
        now = walk(now, T)
    return dts, ts, k_jump, path_t, row_of_jump


class Schedule:
    __slots__ = ('step_dt', 'step_t', 'k_jump', 'time_f32', 'path_t', 'n_steps', 'n_times',
                 'row_of_jump')

    def __init__(self, times, delta_t, T, until_T):
        times = np.asarray(times, dtype=np.float64)
        dts, ts, k_jump, path_t, row_of_jump = _walk_clock(times, delta_t, T, until_T)
        self.step_dt = np.asarray(dts, dtype=np.float64).astype(np.float32)
        self.step_t = np.asarray(ts, dtype=np.float64).astype(np.float32)
        self.k_jump = np.asarray(k_jump, dtype=np.int32)
        self.time_f32 = times.astype(np.float32)
        self.path_t = np.asarray(path_t, dtype=np.float64)
        self.row_of_jump = np.asarray(row_of_jump, dtype=np.int64)
        self.n_steps = len(dts)
        self.n_times = len(times)

    @property
    def n_rows(self):
        return 1 + self.n_steps + self.n_times

    def has_tail(self):
        """Euler steps after the last jump (until_T) -- or no jump at all."""
        if self.n_times == 0:
            return self.n_steps > 0
        return int(self.k_jump[-1]) < self.n_steps

    def packed_nbytes(self):
        return 4 * (2 * self.n_steps + 3 * self.n_times + 1)

    def pack_into(self, buf, time_ptr):
        """Write [step_dt | step_t | k_jump | time_f32 | time_ptr] into the int32
        numpy view ``buf`` (the layout the library copies with one memcpy)."""
        K, nt = self.n_steps, self.n_times
        f = buf.view(np.float32)
        f[0:K] = self.step_dt
        f[K:2 * K] = self.step_t
        buf[2 * K:2 * K + nt] = self.k_jump
        f[2 * K + nt:2 * K + 2 * nt] = self.time_f32
        buf[2 * K + 2 * nt:2 * K + 3 * nt + 1] = time_ptr
        return K, nt

    def struct(self, base):
        """The ``NjodeSchedule`` over a buffer ``pack_into`` has filled, at address ``base``."""
        K, nt = self.n_steps, self.n_times
        return _lib.NjodeSchedule(K, nt, base, base + 4 * K, base + 8 * K, base + 8 * K + 4 * nt,
                                  base + 8 * K + 8 * nt)


CondExpClock = collections.namedtuple(
    'CondExpClock', 'step_dt step_t k_jump path_t row_of_jump n_steps n_times stage_first')


def _walk_clock_staged(times, delta_t, maturities):
    """The clock of ``stock_model.Combined.compute_cond_exp``: the single walk's lists plus the
    index of every stage's first Euler step.  Stage ``i`` walks to its accumulated ``T``; the next
    one starts at the last clock value written (``path_t[-1]``: that ``T`` through a partial step,
    or an observation time within 1e-10 of it) and passes over the times it has reached."""
    dts, ts, k_jump, path_t, row_of_jump, stage_first = [], [], [], [0.0], [], []
    now, T = 0.0, 0

    def walk(now, target):
        guard = target - 1e-10 * delta_t
        while now < guard:
            step = delta_t if now < target - delta_t else target - now
            dts.append(step)
            ts.append(now)
            now = now + step
            path_t.append(now)
        return now

    for si, maturity in enumerate(maturities):
        T = T + maturity
        if si:
            now = path_t[-1]
        stage_first.append(len(dts))
        for obs_time in times:
            if obs_time > T + 1e-10:
                break
            if obs_time <= now:
                continue
            now = walk(now, obs_time)
            k_jump.append(len(dts))
            row_of_jump.append(len(path_t))
            path_t.append(obs_time)
        now = walk(now, T)
    return dts, ts, k_jump, path_t, row_of_jump, stage_first


def cond_exp_clock(times, delta_t, T, stage_maturities=None):
    """The clock of ``stock_model.StockModel.compute_cond_exp`` (``start_time=None``) in float64:
    ``step_dt`` / ``step_t`` [K] (length of Euler step k, clock before it), ``k_jump`` [n_times]
    int32, and ``path_t`` -- the host walk's ``path_t``, entry for entry.  It is ``Schedule``'s
    clock up to ``T`` before the fp32 rounding: the analytic factors are
    ``exp(rate * periodic_coeff(step_t) * step_dt)`` in float64.

    ``stage_maturities`` (a list, one entry per stage of a regime-switch dataset): the clock of
    ``stock_model.Combined.compute_cond_exp`` instead, stage after stage; ``T`` is then the
    accumulated sum of the list, whatever is passed.  ``stage_first`` [n_stages] int32 is the
    index of each stage's first Euler step (``[0]`` for the single walk).

    ``ValueError`` unless ``times`` is strictly increasing with ``0 < times[i] <= T + 1e-10``
    (the host walk silently skips a time its clock has reached and stops at one beyond ``T``)."""
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    if stage_maturities is not None:
        stage_maturities = [float(m) for m in stage_maturities]
        if not stage_maturities or not all(np.isfinite(m) and m > 0 for m in stage_maturities):
            raise ValueError('stage maturities must be positive and finite, at least one')
        T = 0
        for m in stage_maturities:      # (accumulated as Combined.compute_cond_exp does)
            T = T + m
    delta_t, T = float(delta_t), float(T)
    if not (delta_t > 0 and np.isfinite(delta_t) and np.isfinite(T)):
        raise ValueError('delta_t must be positive and T finite')
    if not np.all(np.isfinite(times)):
        raise ValueError('observation times must be finite')
    if times.size and (np.any(np.diff(times) <= 0) or times[0] <= 0):
        raise ValueError('observation times must be strictly increasing and positive')
    if times.size and times[-1] > T + 1e-10:
        raise ValueError('observation time {!r} beyond T = {!r}'.format(float(times[-1]), T))
    if stage_maturities is None:
        dts, ts, k_jump, path_t, row_of_jump = _walk_clock(times, delta_t, T, True, strict=True)
        stage_first = [0]
    else:
        dts, ts, k_jump, path_t, row_of_jump, stage_first = _walk_clock_staged(
            times, delta_t, stage_maturities)
        if len(k_jump) != len(times):
            raise ValueError('an observation time falls between two stages of the clock')
    return CondExpClock(np.asarray(dts, dtype=np.float64), np.asarray(ts, dtype=np.float64),
                        np.asarray(k_jump, dtype=np.int32), np.asarray(path_t, dtype=np.float64),
                        np.asarray(row_of_jump, dtype=np.int64), len(dts), len(times),
                        np.asarray(stage_first, dtype=np.int32))


class ScheduleCache:
    """LRU of schedules keyed by (times, delta_t, T, until_T); ``make``: the schedule class."""

    def __init__(self, capacity=64, make=Schedule):
        self.capacity, self.make = capacity, make
        self._d = collections.OrderedDict()

    def get(self, times, delta_t, T, until_T):
        times = np.ascontiguousarray(times, dtype=np.float64)
        key = (times.tobytes(), float(delta_t), float(T), bool(until_T))
        s = self._d.get(key)
        if s is None:
            s = self.make(times, delta_t, T, until_T)
            self._d[key] = s
            if len(self._d) > self.capacity:
                self._d.popitem(last=False)
        else:
            self._d.move_to_end(key)
        return s


class PinnedRing:
    """Round-robin pinned host buffers for the asynchronous schedule upload.  A
    slot is reused only after the event recorded behind its last upload has
    completed."""

    def __init__(self, slots=16):
        self.slots = [None] * slots
        self.events = [None] * slots
        self.next = 0
        self.held = set()

    def acquire(self, nbytes):
        i = self.next
        while i in self.held and len(self.held) < len(self.slots):
            i = (i + 1) % len(self.slots)
        self.next = (i + 1) % len(self.slots)
        ev = self.events[i]
        if ev is not None:
            ev.synchronize()
        t = self.slots[i]
        n_int = (nbytes + 3) // 4 + 16
        if t is None or t.numel() < n_int:
            t = torch.empty(max(n_int, 1024), dtype=torch.int32).pin_memory()
            self.slots[i] = t
        return i, t

    def hold(self, i):
        """Slot ``i`` is read by work that is not enqueued yet (a deferred plan): ``acquire``
        passes it over until ``release_with`` / ``release_after`` frees it."""
        self.held.add(i)

    def release_with(self, i, j):
        """Slot ``i`` is free when slot ``j`` is: both were read by the same enqueued call (they
        share ``j``'s event; recording it again for either only moves the guard later)."""
        self.held.discard(i)
        self.events[i] = self.events[j]

    def release_after(self, i, stream):
        self.held.discard(i)
        ev = self.events[i]
        if ev is None:
            ev = torch.cuda.Event()
            self.events[i] = ev
        ev.record(stream)
