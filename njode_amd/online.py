"""
Online filtering with a trained NJ-ODE (C ABI: ``include/njode_online.h``).

``NJODE.forward`` is the batch form: it starts at ``t = 0`` and needs the whole record.  An
``OnlineState`` keeps ``(h, last_X, tau, now)`` of ``n_series`` series on the GPU; ``observe`` feeds
the listed series their next measurement, ``predict`` reads forecasts from a copy of the state, and
each call costs the Euler steps that are new; ``observe_many`` applies a run of events per series --
observations and empty slices, laid out by series -- in ONE launch, with the bits of the same events
fed one call at a time, and ``replay(fused=True)`` is the warm start from a collated history through
it.  Two kernel families serve it (``kernels=``):
``'wave'``, one wave per series, for build-table shapes with two hidden layers and sizes up to 64
without a GRU jump, and ``'generic'``, a tile of up to 16 series per workgroup on the matrix cores,
for every model the shape-generic kernels run (any widths and depths, ``nn_desc = None``,
per-network descriptions, ``use_rnn``); ``'auto'`` takes the first where it applies.  The state is
the same: a ``state_dict`` moves between the two.  The results of any sequence of calls on one series
are those of the reference forward on the batch that consists of that series alone, with ``times``
equal to the targets of the calls in order.

``ids`` and times are host arrays (numpy or lists): they are checked here, on the host, and
uploaded.  Values (``start_X``, ``X``, ``M``) are tensors or arrays; outputs are device tensors.
Eval mode only, no loss, no gradients.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib


KERNELS = ('wave', 'generic', 'auto')


def default_max_steps(t, delta_t):
    """``ceil(max(t) / delta_t) + 2``: since a clock is never negative, an upper bound of the Euler
    steps the walk to any one of the targets ``t`` takes."""
    t = np.asarray(t, dtype=np.float64)
    top = float(t.max()) if t.size else 0.0
    return max(int(math.ceil(top / float(delta_t))) + 2, 1)


def by_series(time_ptr, obs_idx):
    """The rows of a collated batch (``time_ptr``: the rows of each time slice, ``obs_idx``: the
    series of each row) laid out by series: ``(ids, ev_ptr, perm, inv)``.  ``ids`` are the series
    that have rows, ascending; series ``ids[r]`` owns the sorted rows ``ev_ptr[r] .. ev_ptr[r + 1] - 1``;
    sorted row ``k`` is row ``perm[k]`` of the batch and row ``i`` of the batch is sorted row
    ``inv[i]``.  The sort is stable, so a series keeps the order of its rows, which is that of the
    slices.  A pure host function."""
    ptr = np.asarray(time_ptr, dtype=np.int64)
    idx = np.asarray(obs_idx, dtype=np.int64)
    if ptr.ndim != 1 or ptr.size < 1 or idx.ndim != 1 or ptr[0] != 0 or ptr[-1] != idx.size or np.any(np.diff(ptr) < 0):
        raise ValueError('time_ptr does not describe {} slices of {} rows'.format(max(ptr.size - 1, 0), idx.size))
    perm = np.argsort(idx, kind='stable').astype(np.int64)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size, dtype=np.int64)
    ids, counts = np.unique(idx, return_counts=True)
    ev_ptr = np.zeros(ids.size + 1, dtype=np.int64)
    np.cumsum(counts, out=ev_ptr[1:])
    return ids.astype(np.int64), ev_ptr, perm, inv


class OnlineState:
    """The resident state of ``n_series`` series of ``model`` (``NJODE.online``)."""

    def __init__(self, model, n_series, delta_t, kernels='wave'):
        n_series, delta_t = int(n_series), float(delta_t)
        if n_series <= 0:
            raise ValueError('n_series must be positive, got {}'.format(n_series))
        if not (delta_t > 0 and math.isfinite(delta_t)):
            raise ValueError('delta_t must be positive and finite, got {!r}'.format(delta_t))
        if kernels not in KERNELS:
            raise ValueError('kernels must be one of {}, got {!r}'.format(KERNELS, kernels))
        self.model, self.n_series, self.delta_t = model, n_series, delta_t
        self.dims = model._get_dims()
        L = _lib.lib()
        wave_ok = bool(L.njode_online_supported(ctypes.byref(self.dims)))
        wave_why = L.njode_last_error().decode('utf-8', 'replace')
        if kernels == 'auto':
            kernels = 'wave' if wave_ok else 'generic'
        gen_ok = bool(L.njode_online_gen_supported(ctypes.byref(self.dims)))
        gen_why = L.njode_last_error().decode('utf-8', 'replace')
        if kernels == 'wave' and not wave_ok:
            hint = " (kernels='generic' runs this model on the shape-generic kernels)" if gen_ok else ''
            raise NotImplementedError('NJODE.online: ' + wave_why + hint)
        if kernels == 'generic' and not gen_ok:
            raise NotImplementedError('NJODE.online: ' + gen_why)
        self.kernels = kernels
        # generic family: series per tile of 16 chains (None: the library's rule; 1, 2, 4, 8, 16)
        self.series_per_tile = None
        self._tables, self._tables_stamp, self._tables_bytes = None, None, 0
        if kernels == 'generic':
            nbytes = ctypes.c_size_t(0)
            _lib.check(L.njode_online_tables_bytes(ctypes.byref(self.dims), ctypes.byref(nbytes)))
            self._tables_bytes = int(nbytes.value)
        self.d, self.H, self.d_out = model.input_size, model.hidden_size, model.output_size
        self.masked = bool(model.masked)
        dev = next(model.parameters()).device
        self.device = dev
        self.h = torch.zeros(n_series, self.H, dtype=torch.float32, device=dev)
        self.last_X = torch.zeros(n_series, self.d, dtype=torch.float32, device=dev)
        self.tau = torch.zeros(n_series, dtype=torch.float32, device=dev)
        self.now = torch.zeros(n_series, dtype=torch.float64, device=dev)
        self.status = None      # the status tensor of the last advance / observe / predict call
        self.n_done = None      # observe_many: the events applied per row of the last call
        self._pending = []      # (ids, status tensor) of the calls check() has not read yet

    # -- host-side checks ---------------------------------------------------------------
    def _eval_only(self):
        if self.model.training:
            raise ValueError('online filtering runs in eval mode only (no dropout): call model.eval()')

    def _ids(self, ids, n=None):
        """(host int32 ids or None, number of rows)."""
        if ids is None:
            if n is None or n > self.n_series:
                raise ValueError('{} rows without ids, the state has {} series'.format(n, self.n_series))
            return None, n
        raw = np.asarray(ids)
        if raw.ndim != 1 or (raw.size and not np.issubdtype(raw.dtype, np.integer)):
            raise ValueError('ids must be a flat list of integers')
        raw = raw.astype(np.int64)
        if raw.size and (raw.min() < 0 or raw.max() >= self.n_series):
            raise ValueError('ids out of range [0, {}): {}'.format(self.n_series, raw.tolist()))
        if np.unique(raw).size != raw.size:
            raise ValueError('duplicate ids in one call: {}'.format(raw.tolist()))
        if n is not None and raw.size != n:
            raise ValueError('{} ids for {} rows'.format(raw.size, n))
        return raw.astype(np.int32), int(raw.size)

    @staticmethod
    def _times(t, shape):
        t = np.asarray(t, dtype=np.float64)
        if t.shape != shape:
            raise ValueError('times of shape {}, expected {}'.format(t.shape, shape))
        if not np.all(np.isfinite(t)) or np.any(t < 0):
            raise ValueError('times must be finite and not negative')
        return np.ascontiguousarray(t)

    def _values(self, v, n, width, what):
        v = torch.as_tensor(v)
        if v.dim() != 2 or v.shape[0] != n or v.shape[1] != width:
            raise ValueError('{} of shape {}, expected ({}, {})'.format(what, tuple(v.shape), n, width))
        return v

    def _rows(self, first, ids):
        """Number of rows of a call: ``len(ids)``, else the leading size of its first array."""
        if ids is not None:
            return len(ids)
        return int(np.shape(first)[0]) if np.ndim(first) else 1

    # -- device side ----------------------------------------------------------------------
    def _on_device(self):
        if self.device.type != 'cuda':
            raise RuntimeError('njode_amd online filtering runs on an MI355X only (the model is on {}); '
                               'there is no CPU path.'.format(self.device))

    def _up(self, a):
        return None if a is None else torch.from_numpy(a).to(self.device)

    def _f32(self, v):
        return v.to(device=self.device, dtype=torch.float32).contiguous()

    def _struct(self):
        return _lib.NjodeOnlineState(self.h.data_ptr(), self.last_X.data_ptr(), self.tau.data_ptr(),
                                     self.now.data_ptr(), self.n_series)

    def _params(self):
        m = self.model
        m._ensure_flat(full=True)
        if m._flat.device != self.device:
            raise RuntimeError('model parameters moved to {}; the state is on {}'.format(m._flat.device, self.device))
        if self.kernels == 'generic':
            self._spt()             # (a bad series_per_tile stops the call before its status is queued)
            self._ensure_tables(m)
        return m._flat

    def _ensure_tables(self, m):
        """The generic family's fragment tables, packed from the flat vector at the first device
        call and again whenever the parameters may have changed: another flat vector (address), a
        write to it (its version counter; ``_param_writes`` for FusedAdam's raw-pointer step), or
        a write to a parameter (the parameters' own version counters: ``load_state_dict``,
        ``p.add_``).  A write through ``p.data`` bumps no counter and is not seen, as autograd does not
        see it: take a new state and ``load_state_dict`` this one's."""
        stamp = (m._flat.data_ptr(), m._flat._version, m._param_writes) + tuple(p._version for p in m._flat_params)
        if self._tables is not None and stamp == self._tables_stamp:
            return
        if self._tables is None:
            self._tables = torch.empty(self._tables_bytes, dtype=torch.uint8, device=self.device)
        _lib.check(_lib.lib().njode_online_tables_f32(
            ctypes.byref(self.dims), m._flat.data_ptr(), self._tables.data_ptr(), self._tables_bytes,
            _lib.stream_arg(self.device)))
        self._tables_stamp = stamp

    def _spt(self):
        spt = self.series_per_tile
        if spt is None:
            return 0
        if spt not in (1, 2, 4, 8, 16):
            raise ValueError('series_per_tile must be None, 1, 2, 4, 8 or 16, got {!r}'.format(spt))
        return int(spt)

    def _gen_head(self, P):
        return (ctypes.byref(self.dims), P.data_ptr(), self._tables.data_ptr(), self._tables_bytes)

    def _status(self, ids, n):
        st = torch.empty(n, dtype=torch.int32, device=self.device)
        self.status = st        # the last call's: one entry per row, 0 reached / 1 bound / 2 bad id / 3 bad range
        self._pending.append((np.arange(n) if ids is None else ids.copy(), st))
        if len(self._pending) > 256:
            self.check()
        return st

    # -- the calls --------------------------------------------------------------------------
    def reset(self, start_X, ids=None):
        """``h = encoder_map(start_X)`` (masked: mask 0), ``last_X = start_X``, ``tau = 0``, ``now = 0``."""
        self._eval_only()
        ids, n = self._ids(ids, None if ids is not None else self._rows(start_X, None))
        x = self._values(start_X, n, self.d, 'start_X')
        self._on_device()
        P, x, ids_d = self._params(), self._f32(x), self._up(ids)
        if self.kernels == 'generic':
            _lib.check(_lib.lib().njode_online_gen_reset_f32(
                *self._gen_head(P), ctypes.byref(self._struct()), _lib.ptr_arg(ids_d), n, x.data_ptr(),
                self._spt(), _lib.stream_arg(self.device)))
            return
        _lib.check(_lib.lib().njode_online_reset_f32(
            ctypes.byref(self.dims), P.data_ptr(), ctypes.byref(self._struct()), _lib.ptr_arg(ids_d), n,
            x.data_ptr(), _lib.stream_arg(self.device)))

    def advance(self, t, ids=None, max_steps=None):
        """An empty time slice at ``t`` (one time per listed series)."""
        self._eval_only()
        ids, n = self._ids(ids, None if ids is not None else self._rows(t, None))
        t = self._times(t, (n,))
        max_steps = default_max_steps(t, self.delta_t) if max_steps is None else int(max_steps)
        self._on_device()
        P, t_d, ids_d = self._params(), self._up(t), self._up(ids)
        st = self._status(ids, n)
        if self.kernels == 'generic':
            _lib.check(_lib.lib().njode_online_gen_advance_f32(
                *self._gen_head(P), ctypes.byref(self._struct()), _lib.ptr_arg(ids_d), n, t_d.data_ptr(),
                self.delta_t, max_steps, self._spt(), st.data_ptr(), _lib.stream_arg(self.device)))
            return
        _lib.check(_lib.lib().njode_online_advance_f32(
            ctypes.byref(self.dims), P.data_ptr(), ctypes.byref(self._struct()), _lib.ptr_arg(ids_d), n,
            t_d.data_ptr(), self.delta_t, max_steps, st.data_ptr(), _lib.stream_arg(self.device)))

    def observe(self, t, X, M=None, ids=None, max_steps=None, out=None):
        """``advance(t)``, then the jump with observation ``X`` (masked models: and mask ``M``).
        Returns ``(Y_before, Y)``, the readouts before and after the jump, ``[n, d_out]`` each
        (``out``: a pair of device tensors to write them into)."""
        self._eval_only()
        ids, n = self._ids(ids, None if ids is not None else self._rows(X, None))
        t = self._times(t, (n,))
        x = self._values(X, n, self.d, 'X')
        if self.masked and M is None:
            raise ValueError('a masked model needs M')
        if not self.masked and M is not None:
            raise ValueError('M given to an unmasked model')
        m = self._values(M, n, self.d, 'M') if self.masked else None
        max_steps = default_max_steps(t, self.delta_t) if max_steps is None else int(max_steps)
        self._on_device()
        P, t_d, ids_d, x = self._params(), self._up(t), self._up(ids), self._f32(x)
        m = self._f32(m) if m is not None else None
        if out is None:
            out = (torch.empty(n, self.d_out, dtype=torch.float32, device=self.device),
                   torch.empty(n, self.d_out, dtype=torch.float32, device=self.device))
        yb, y = out
        st = self._status(ids, n)
        if self.kernels == 'generic':
            _lib.check(_lib.lib().njode_online_gen_observe_f32(
                *self._gen_head(P), ctypes.byref(self._struct()), _lib.ptr_arg(ids_d), n, t_d.data_ptr(),
                x.data_ptr(), _lib.ptr_arg(m), self.delta_t, max_steps, self._spt(), yb.data_ptr(), y.data_ptr(),
                st.data_ptr(), _lib.stream_arg(self.device)))
            return yb, y
        _lib.check(_lib.lib().njode_online_observe_f32(
            ctypes.byref(self.dims), P.data_ptr(), ctypes.byref(self._struct()), _lib.ptr_arg(ids_d), n,
            t_d.data_ptr(), x.data_ptr(), _lib.ptr_arg(m), self.delta_t, max_steps, yb.data_ptr(),
            y.data_ptr(), st.data_ptr(), _lib.stream_arg(self.device)))
        return yb, y

    def predict(self, t_query, ids=None, max_steps=None):
        """Forecasts ``[n, Q, d_out]`` at the queries ``t_query [n, Q]`` (ascending per series) from a
        copy of the state; the stored state is untouched.  A later query goes on from where the
        earlier one stopped."""
        self._eval_only()
        ids, n = self._ids(ids, None if ids is not None else self._rows(t_query, None))
        tq = np.asarray(t_query, dtype=np.float64)
        if tq.ndim != 2 or tq.shape[0] != n or tq.shape[1] < 1:
            raise ValueError('t_query of shape {}, expected ({}, Q >= 1)'.format(tq.shape, n))
        tq = self._times(tq, tq.shape)
        if np.any(np.diff(tq, axis=1) < 0):
            raise ValueError('the queries of a series must ascend')
        Q = tq.shape[1]
        max_steps = default_max_steps(tq, self.delta_t) if max_steps is None else int(max_steps)
        self._on_device()
        P, t_d, ids_d = self._params(), self._up(tq), self._up(ids)
        y = torch.empty(n, Q, self.d_out, dtype=torch.float32, device=self.device)
        st = self._status(ids, n)
        if self.kernels == 'generic':
            _lib.check(_lib.lib().njode_online_gen_predict_f32(
                *self._gen_head(P), ctypes.byref(self._struct()), _lib.ptr_arg(ids_d), n, t_d.data_ptr(), Q,
                self.delta_t, max_steps, self._spt(), y.data_ptr(), st.data_ptr(), _lib.stream_arg(self.device)))
            return y
        _lib.check(_lib.lib().njode_online_predict_f32(
            ctypes.byref(self.dims), P.data_ptr(), ctypes.byref(self._struct()), _lib.ptr_arg(ids_d), n,
            t_d.data_ptr(), Q, self.delta_t, max_steps, y.data_ptr(), st.data_ptr(),
            _lib.stream_arg(self.device)))
        return y

    def observe_many(self, ev_ptr, t, X, M=None, kind=None, ids=None, max_steps=None, out=None):
        """A run of events per listed series in one launch.  Events are laid out by series: row
        ``r`` of the call owns events ``ev_ptr[r] .. ev_ptr[r + 1] - 1`` and applies them in that
        order.  ``kind[e] = 1`` (or ``kind=None``) is ``observe`` at ``t[e]`` with ``X[e]`` (``M[e]``);
        ``kind[e] = 0`` is ``advance`` to ``t[e]``, and both its output rows are the readout of the
        state it arrives at.  Returns ``(Y_before, Y)``, ``[n_events, d_out]`` each, and leaves the
        events applied per row in ``self.n_done`` beside ``self.status``.  The results are the bits
        of the same events fed one call at a time; ``max_steps`` bounds the steps in front of each
        event, and a series it stops skips its remaining events (their rows are NaN)."""
        self._eval_only()
        raw = np.asarray(ev_ptr)
        if raw.ndim != 1 or raw.size < 1 or not np.issubdtype(raw.dtype, np.integer):
            raise ValueError('ev_ptr must be a flat list of integers, one more than rows')
        ids, n = self._ids(ids, raw.size - 1)
        ptr = raw.astype(np.int64)
        n_events = int(np.shape(t)[0]) if np.ndim(t) else -1
        if ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != n_events:
            raise ValueError('ev_ptr does not describe {} ranges of {} events'.format(n, n_events))
        if n_events >= 2 ** 31:
            raise ValueError('{} events in one call'.format(n_events))
        t = self._times(t, (n_events,))
        x = self._values(X, n_events, self.d, 'X')
        if self.masked and M is None:
            raise ValueError('a masked model needs M')
        if not self.masked and M is not None:
            raise ValueError('M given to an unmasked model')
        m = self._values(M, n_events, self.d, 'M') if self.masked else None
        if kind is not None:
            kraw = np.asarray(kind)
            if kraw.shape != (n_events,) or (kraw.size and not (np.issubdtype(kraw.dtype, np.integer)
                                                                 or kraw.dtype == np.bool_)):
                raise ValueError('kind must be {} integers'.format(n_events))
            if kraw.size and not np.all((kraw == 0) | (kraw == 1)):
                raise ValueError('kind entries must be 0 (empty slice) or 1 (observation)')
            kind = np.ascontiguousarray(kraw.astype(np.int32))
        max_steps = default_max_steps(t, self.delta_t) if max_steps is None else int(max_steps)
        self._on_device()
        P, t_d, ids_d, x = self._params(), self._up(t), self._up(ids), self._f32(x)
        ptr_d, kind_d = self._up(ptr.astype(np.int32)), self._up(kind)
        m = self._f32(m) if m is not None else None
        if out is None:
            out = (torch.empty(n_events, self.d_out, dtype=torch.float32, device=self.device),
                   torch.empty(n_events, self.d_out, dtype=torch.float32, device=self.device))
        yb, y = out
        st = self._status(ids, n)
        self.n_done = torch.empty(n, dtype=torch.int32, device=self.device)
        if self.kernels == 'generic':
            _lib.check(_lib.lib().njode_online_gen_run_f32(
                *self._gen_head(P), ctypes.byref(self._struct()), _lib.ptr_arg(ids_d), n, ptr_d.data_ptr(), n_events,
                t_d.data_ptr(), x.data_ptr(), _lib.ptr_arg(m), _lib.ptr_arg(kind_d), self.delta_t, max_steps,
                self._spt(), yb.data_ptr(), y.data_ptr(), st.data_ptr(), self.n_done.data_ptr(),
                _lib.stream_arg(self.device)))
            return yb, y
        _lib.check(_lib.lib().njode_online_run_f32(
            ctypes.byref(self.dims), P.data_ptr(), ctypes.byref(self._struct()), _lib.ptr_arg(ids_d), n,
            ptr_d.data_ptr(), n_events, t_d.data_ptr(), x.data_ptr(), _lib.ptr_arg(m), _lib.ptr_arg(kind_d),
            self.delta_t, max_steps, yb.data_ptr(), y.data_ptr(), st.data_ptr(), self.n_done.data_ptr(),
            _lib.stream_arg(self.device)))
        return yb, y

    def replay(self, times, time_ptr, X, obs_idx, M=None, fused=False):
        """Feed a collated batch slice by slice (``obs_idx``: the series of each row): a warm start
        from history.  A slice without rows moves nobody.  Returns ``(Y_before, Y)``, one row per
        row of ``X``.  ``fused=True``: the rows are sorted by series on the host (stable: a series
        keeps its time order) and fed as ONE ``observe_many`` to the series that have rows; the
        results, in the original row order, are the bits of the loop's."""
        self._eval_only()
        times = np.asarray(times, dtype=np.float64)
        ptr = np.asarray(time_ptr, dtype=np.int64)
        idx = np.asarray(obs_idx.cpu() if torch.is_tensor(obs_idx) else obs_idx).astype(np.int64)
        if ptr.shape != (times.size + 1,) or ptr[0] != 0 or ptr[-1] != idx.size or np.any(np.diff(ptr) < 0):
            raise ValueError('time_ptr does not describe {} slices of {} rows'.format(times.size, idx.size))
        x = self._values(X, idx.size, self.d, 'X')
        if self.masked and M is None:
            raise ValueError('a masked model needs M')
        if not self.masked and M is not None:
            raise ValueError('M given to an unmasked model')
        m = self._values(M, idx.size, self.d, 'M') if self.masked else None
        if fused:
            ids, ev_ptr, perm, inv = by_series(ptr, idx)
            t_row = np.repeat(times, np.diff(ptr))[perm]
            sel = torch.from_numpy(perm).to(x.device)
            msel = None if m is None else m[torch.from_numpy(perm).to(m.device)]
            yb, y = self.observe_many(ev_ptr, t_row, x[sel], msel, ids=ids)
            back = torch.from_numpy(inv).to(self.device)
            return yb[back], y[back]
        self._on_device()
        x = self._f32(x)
        m = self._f32(m) if m is not None else None
        yb = torch.empty(idx.size, self.d_out, dtype=torch.float32, device=self.device)
        y = torch.empty_like(yb)
        for i, t in enumerate(times):
            lo, hi = int(ptr[i]), int(ptr[i + 1])
            if hi > lo:
                self.observe(np.full(hi - lo, t), x[lo:hi], None if m is None else m[lo:hi], ids=idx[lo:hi],
                             out=(yb[lo:hi], y[lo:hi]))
        return yb, y

    # -- bookkeeping ------------------------------------------------------------------------
    def check(self):
        """Read the status of every call since the last check (synchronises); ``RuntimeError`` naming
        the series that the step bound stopped."""
        pending, self._pending = self._pending, []
        stopped, bad, ranges = set(), set(), set()
        for ids, st in pending:
            s = st.cpu().numpy()
            stopped.update(int(i) for i in ids[s == 1])
            bad.update(int(i) for i in ids[s == 2])
            ranges.update(int(i) for i in ids[s == 3])
        if bad:
            raise RuntimeError('online: ids outside the state: {}'.format(sorted(bad)))
        if ranges:
            raise RuntimeError('online: series {} were given a range of events outside the call'.format(sorted(ranges)))
        if stopped:
            raise RuntimeError('online: series {} hit max_steps before their target; their state is where '
                               'the bound stopped them'.format(sorted(stopped)))

    def state_dict(self):
        return {'h': self.h.clone(), 'last_X': self.last_X.clone(), 'tau': self.tau.clone(),
                'now': self.now.clone(), 'delta_t': self.delta_t}

    def load_state_dict(self, sd):
        for k, t in (('h', self.h), ('last_X', self.last_X), ('tau', self.tau), ('now', self.now)):
            src = torch.as_tensor(sd[k])
            if src.shape != t.shape:
                raise ValueError('{} of shape {}, expected {}'.format(k, tuple(src.shape), tuple(t.shape)))
            t.copy_(src.to(device=t.device, dtype=t.dtype))
        self.delta_t = float(sd.get('delta_t', self.delta_t))
