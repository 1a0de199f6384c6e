"""Helpers of the tests of runs of events (``observe_many``; a helper module, not a conftest), for
both kernel families: event lists per series from a collated batch, the same events fed one call at
a time, and the raw C-ABI call with every buffer in a guard-band arena."""
import ctypes

import numpy as np
import pytest
import torch

import guarded
from online_gen_util import bits, eq_bits, same_bits
from njode_amd import _lib, schedule

# [series][call] in units of delta_t, off the grid: a t = 0 observation, the same time again, partial
# steps, exactly two full steps, target == now (the matrix of the single-call clock tests, restated)
CLOCK_TIMES = np.asarray([
    [0.0, 0.0, 0.5, 3.5],
    [0.4, 0.4, 3.1, 3.1],
    [2.0, 4.3, 4.3, 9.6],
    [0.0, 5.25, 5.25, 5.5]])


def event_lists(b, N, delta_t):
    """Per series ``[(t, kind, row of X or -1)]``.  The role of series s is s % 5:
    0  every slice of the batch in order, its own rows as observations and the other series' times as
       empty slices, plus an empty slice 0.3 delta_t behind each observation but one in the last slice (a
       partial step);
    1  no event;  2  one event, its first observation;  3  every slice of the batch as an empty slice;
    4  its own observations only."""
    ptr, idx = np.asarray(b['time_ptr']), np.asarray(b['obs_idx'])
    times = np.asarray(b['times'], dtype=np.float64)
    own = [{} for _ in range(N)]
    for i in range(times.size):
        for r in range(int(ptr[i]), int(ptr[i + 1])):
            assert i not in own[int(idx[r])]
            own[int(idx[r])][i] = r
    lists = []
    for s in range(N):
        role, ev = s % 5, []
        for i, t in enumerate(times):
            mine = i in own[s]
            if role == 0:
                ev.append((float(t), 1, own[s][i]) if mine else (float(t), 0, -1))
                if mine and i + 1 < times.size:
                    ev.append((float(t) + 0.3 * delta_t, 0, -1))
            elif role == 3:
                ev.append((float(t), 0, -1))
            elif mine and (role == 4 or (role == 2 and not ev)):
                ev.append((float(t), 1, own[s][i]))
        lists.append([] if role == 1 else ev)
    return lists


def pack(lists, X, M):
    """(ev_ptr, t, kind, X rows, M rows or None) of the lists; the value rows of an empty slice are
    NaN: whoever reads them shows."""
    ev_ptr = np.concatenate([[0], np.cumsum([len(ev) for ev in lists])]).astype(np.int64)
    flat = [e for ev in lists for e in ev]
    d = X.shape[1]
    t = np.asarray([e[0] for e in flat], dtype=np.float64)
    kind = np.asarray([e[1] for e in flat], dtype=np.int32)
    xs = torch.full((len(flat), d), float('nan'))
    ms = torch.full((len(flat), d), float('nan')) if M is not None else None
    for k, e in enumerate(flat):
        if e[1]:
            xs[k] = X[e[2]]
            if M is not None:
                ms[k] = M[e[2]]
    return ev_ptr, t, kind, xs, ms


def truth_events(ev, X, M):
    """The list of one series as ``online_util.truth`` takes it."""
    return [(t, X[r] if k else None, (M[r] if M is not None else None) if k else None) for t, k, r in ev]


def run(st, lists, ids, X, M, max_steps=None):
    """One observe_many with the lists -> (Y_before, Y)."""
    ev_ptr, t, kind, xs, ms = pack(lists, X, M)
    return st.observe_many(ev_ptr, t, xs, ms, kind=kind, ids=ids, max_steps=max_steps)


def single_calls(st, lists, ids, X, M, max_steps=None):
    """The same events one call at a time: call k of a series is its k-th event, ``observe`` for an
    observation, ``advance`` for an empty slice (whose two rows are ``predict`` with Q = 1 taken
    before it); the k-th events of the series travel together, which the distinct ids allow.  A
    series the bound stops gets no further call.  Returns (Y_before, Y, status per list, events
    applied per list); the rows of events that were not applied are NaN."""
    offs = np.concatenate([[0], np.cumsum([len(ev) for ev in lists])]).astype(np.int64)
    yb_all = torch.full((int(offs[-1]), st.d_out), float('nan'), device=st.device)
    y_all = yb_all.clone()
    status, done = [0] * len(lists), [0] * len(lists)
    for k in range(max((len(ev) for ev in lists), default=0)):
        for want in (1, 0):
            rows = [r for r, ev in enumerate(lists) if k < len(ev) and ev[k][1] == want and status[r] == 0]
            if not rows:
                continue
            tt = np.asarray([lists[r][k][0] for r in rows])
            sid = [int(ids[r]) for r in rows]
            at = torch.as_tensor([int(offs[r]) + k for r in rows], device=st.device)
            if want:
                src = [lists[r][k][2] for r in rows]
                yb, y = st.observe(tt, X[src], None if M is None else M[src], ids=sid, max_steps=max_steps)
            else:
                yb = y = st.predict(tt[:, None], ids=sid, max_steps=max_steps)[:, 0]
                st.advance(tt, ids=sid, max_steps=max_steps)
            got = st.status.cpu().tolist()
            yb_all[at], y_all[at] = yb, y
            for r, s in zip(rows, got):
                status[r] = s
                done[r] += s == 0
    return yb_all, y_all, status, done


def steps_per_event(times, delta_t):
    """Euler steps in front of each of a series' targets, from t = 0."""
    k_jump = schedule._walk_clock(times, delta_t, 0.0, False)[2]
    return [int(k_jump[j] - (k_jump[j - 1] if j else 0)) for j in range(len(times))]


def clock_after(times, delta_t):
    now = 0.0
    for x in schedule._walk_clock(times, delta_t, 0.0, False)[0]:
        now = now + x
    return now


# ---- the raw call in a guard-band arena -----------------------------------------------------------------
def random_state(S, d, H, delta_t, seed=13):
    g = torch.Generator().manual_seed(seed)
    h0 = 0.3 * torch.randn(S, H, generator=g)
    x0 = 0.3 * torch.randn(S, d, generator=g)
    tau0 = (torch.arange(S) % 4).float() * 0.5 * delta_t
    now0 = tau0.double() + 0.1 * delta_t
    return h0, x0, tau0, now0


def arena_run(m, state0, ids, ev_ptr, t, X, M, kind, delta_t, max_steps, phase, generic=False, spt=0,
              null=None):
    """One run through the C ABI with every buffer of the call -- parameters, tables, state, ids,
    ev_ptr, events, outputs, status, n_done -- at exactly its stated size in a guard-band arena
    (``null``: 'Yb' or 'Y' passed as NULL).  Returns (return code, {name: bytes after the call},
    guards that changed)."""
    h0, x0, tau0, now0 = state0
    S, H, d, DO = h0.shape[0], h0.shape[1], x0.shape[1], m.output_size
    n, E = len(ids), len(t)
    m._ensure_flat(full=True)
    P = m._flat.detach().clone()
    dims = m._get_dims()
    L = _lib.lib()
    ar = guarded.Arena('cuda', phase=phase)
    ar.add('P', 4 * P.numel(), 'nan32')
    if generic:
        tb = ctypes.c_size_t(0)
        _lib.check(L.njode_online_tables_bytes(ctypes.byref(dims), ctypes.byref(tb)))
        tb = int(tb.value)
        ar.add('tables', tb, 'nan32')
    ar.add('h', 4 * S * H, 'nan32').add('last_X', 4 * S * d, 'nan32').add('tau', 4 * S, 'nan32')
    ar.add('now', 8 * S, 'nan64').add('ids', 4 * n, 'index', modulo=S).add('ev_ptr', 4 * (n + 1), 'index', modulo=2)
    ar.add('t', 8 * E, 'nan64').add('X', 4 * E * d, 'nan32').add('M', 4 * E * d, 'nan32')
    ar.add('kind', 4 * E, 'index', modulo=2)
    ar.add('Yb', 4 * E * DO).add('Y', 4 * E * DO).add('status', 4 * n).add('n_done', 4 * n)
    ar.build()
    vals = dict(P=P, h=h0, last_X=x0, tau=tau0, now=now0, ids=torch.as_tensor(ids, dtype=torch.int32),
                ev_ptr=torch.as_tensor(ev_ptr, dtype=torch.int32), t=torch.as_tensor(t, dtype=torch.float64), X=X,
                kind=torch.as_tensor(kind, dtype=torch.int32))
    if M is not None:
        vals['M'] = M
    for key, v in vals.items():
        ar.put(key, v.cuda())
    state = _lib.NjodeOnlineState(ar.ptr('h'), ar.ptr('last_X'), ar.ptr('tau'), ar.ptr('now'), S)
    stream = _lib.stream_arg(torch.device('cuda'))
    yb = None if null == 'Yb' else ar.ptr('Yb')
    y = None if null == 'Y' else ar.ptr('Y')
    tail = (ar.ptr('ids'), n, ar.ptr('ev_ptr'), E, ar.ptr('t'), ar.ptr('X'), ar.ptr('M') if M is not None else None,
            ar.ptr('kind'), delta_t, max_steps)
    if generic:
        _lib.check(L.njode_online_tables_f32(ctypes.byref(dims), ar.ptr('P'), ar.ptr('tables'), tb, stream))
        rc = L.njode_online_gen_run_f32(ctypes.byref(dims), ar.ptr('P'), ar.ptr('tables'), tb, ctypes.byref(state), *tail,
                                        spt, yb, y, ar.ptr('status'), ar.ptr('n_done'), stream)
    else:
        rc = L.njode_online_run_f32(ctypes.byref(dims), ar.ptr('P'), ctypes.byref(state), *tail, yb, y,
                                    ar.ptr('status'), ar.ptr('n_done'), stream)
    guards = ar.check()
    out = {k: ar.view(k).clone() for k in ('h', 'last_X', 'tau', 'now', 'Yb', 'Y', 'status', 'n_done')}
    out['f32'] = {k: ar.view(k, torch.float32).clone() for k in ('h', 'last_X', 'tau', 'Yb', 'Y')}
    out['status'] = ar.view('status', torch.int32).tolist()
    out['n_done'] = ar.view('n_done', torch.int32).tolist()
    out['image'] = {k: ar.image[ar.where[k][0]:ar.where[k][0] + ar.where[k][1]].clone() for k in ('Yb', 'Y')}
    return rc, out, guards


# ---- checks both kernel families share -----------------------------------------------------------------
# (``shape``: (d, H, d_out, masked); ``new_state(N)``: a fresh state of N series)
BOUND_TIMES = [[1.5, 2.5, 4.0, 5.0], [0.5, 2.0, 7.5, 8.0], [1.0, 1.0, 3.5], [2.6, 3.0]]     # in units of delta_t
BOUND_KINDS = [[1, 0, 1, 1], [1, 0, 1, 1], [0, 1, 1], [1, 1]]


def bound_case(shape, delta_t, seed=9):
    d, N = shape[0], len(BOUND_TIMES)
    g = torch.Generator().manual_seed(seed)
    start = 0.2 * torch.randn(N, d, generator=g)
    n_ev = sum(len(x) for x in BOUND_TIMES)
    X = 0.5 * torch.randn(n_ev, d, generator=g)
    M = (torch.rand(n_ev, d, generator=g) < 0.3).float() if shape[3] else None
    lists, r = [], 0
    for ts, ks in zip(BOUND_TIMES, BOUND_KINDS):
        lists.append([(t * delta_t, k, r + j) for j, (t, k) in enumerate(zip(ts, ks))])
        r += len(ts)
    # max_steps from the host's walk: series 1 cannot reach its third event, every other walk fits
    steps = [steps_per_event([t for t, _, _ in ev], delta_t) for ev in lists]
    max_steps = 3
    assert steps[1][2] > max_steps and max(steps[1][:2]) <= max_steps
    assert all(max(x) <= max_steps for s, x in enumerate(steps) if s != 1)
    return start, X, M, lists, max_steps


def check_bound(new_state, shape, delta_t):
    start, X, M, lists, max_steps = bound_case(shape, delta_t)
    N = len(lists)
    st, one, free = new_state(N), new_state(N), new_state(N)
    for x in (st, one, free):
        x.reset(start)
    yb, y = run(st, lists, None, X, M, max_steps=max_steps)
    assert st.status.cpu().tolist() == [0, 1, 0, 0]
    assert st.n_done.cpu().tolist() == [4, 2, 3, 2]
    with pytest.raises(RuntimeError, match=r'\[1\]'):
        st.check()
    offs = np.concatenate([[0], np.cumsum([len(ev) for ev in lists])])
    lo, hi = int(offs[1]), int(offs[2])
    assert torch.isnan(y[lo + 2:hi]).all() and torch.isnan(yb[lo + 2:hi]).all()
    assert torch.isfinite(y[:lo + 2]).all() and torch.isfinite(y[hi:]).all() and torch.isfinite(yb[hi:]).all()
    # the same single calls with the same bound: the same states, rows and counts
    yb1, y1, status, done = single_calls(one, lists, list(range(N)), X, M, max_steps=max_steps)
    one._pending = []
    assert status == [0, 1, 0, 0] and done == [4, 2, 3, 2]
    assert same_bits(bits(st), bits(one))
    assert eq_bits(yb, yb1) and eq_bits(y, y1)
    assert float(st.now[1]) == clock_after([0.5 * delta_t, 2.0 * delta_t], delta_t) + delta_t + delta_t + delta_t
    assert float(st.tau[1]) == float(np.float32(0.5 * delta_t))
    # every other series: its unbounded run
    ybf, yf = run(free, lists, None, X, M)
    free.check()
    others = [0, 2, 3]
    assert all(eq_bits(p[others], q[others]) for p, q in zip(bits(st), bits(free)))
    keep = torch.ones(len(y), dtype=torch.bool, device=y.device)
    keep[lo:hi] = False
    assert eq_bits(y[keep], yf[keep]) and eq_bits(yb[keep], ybf[keep])
    assert eq_bits(y[lo:lo + 2], yf[lo:lo + 2])


def arena_case(shape, delta_t):
    """Seven series, six events: rows on series 6 (events 0, 1) and 2 (events 3, 4, 5) are good."""
    d = shape[0]
    g = torch.Generator().manual_seed(13)
    t = np.asarray([0.7, 2.9, 1.0, 1.6, 1.6, 4.2]) * delta_t
    kind = [1, 0, 1, 0, 1, 1]
    X = 0.5 * torch.randn(6, d, generator=g)
    M = (torch.rand(6, d, generator=g) < 0.3).float() if shape[3] else None
    return t, kind, X, M


def check_bad_rows(m, shape, new_state, generic=False, spt=0):
    """An id outside the state: status 2; a descending range and a range that ends at n_events + 1:
    status 3; n_done 0; their state rows, output rows and every guard band untouched; the good rows of
    the call are those of a call without the bad ones."""
    delta_t = 0.37 * 2.0 ** -10
    t, kind, X, M = arena_case(shape, delta_t)
    state0 = random_state(7, shape[0], shape[1], delta_t)
    names = ('h', 'last_X', 'tau', 'now')
    ids, ev_ptr = [6, 9, 2, 0, 3], [0, 2, 3, 6, 5, 7]
    ref = new_state(7)
    ref.load_state_dict(dict(zip(names, state0)))
    good = [0, 1, 3, 4, 5]
    ryb, ry = ref.observe_many([0, 2, 5], t[good], X[good], None if M is None else M[good],
                               kind=np.asarray(kind)[good], ids=[6, 2], max_steps=8)
    ref.check()
    DO = shape[2]
    for phase in (0, 1):
        rc, out, guards = arena_run(m, state0, ids, ev_ptr, t, X, M, kind, delta_t, 8, phase, generic, spt)
        assert rc == 0 and guards == []
        assert out['status'] == [0, 2, 0, 3, 3] and out['n_done'] == [2, 0, 3, 0, 0]
        for name, src in zip(names, state0):
            dtype = torch.float64 if name == 'now' else torch.float32
            got = out[name].view(dtype).view(7, -1)
            assert eq_bits(got, getattr(ref, name).view(7, -1)), (phase, name)     # (ref never moved series 0 and 3)
            src = src.view(7, -1).cuda()
            idle, moved = [0, 1, 3, 4, 5], [2, 6]
            assert eq_bits(got[idle], src[idle]) and (name == 'last_X' or not eq_bits(got[moved], src[moved]))
        for name, want in (('Yb', ryb), ('Y', ry)):
            rows = out[name].view(torch.float32).view(6, DO)
            assert eq_bits(rows[good], want), (phase, name)
            image = out['image'][name].view(torch.float32).view(6, DO)
            assert eq_bits(rows[2], image[2]), (phase, name)      # the event nobody owns: never written


def check_stated_sizes(m, shape, generic=False, spt=0):
    delta_t = 0.37 * 2.0 ** -10
    t, kind, X, M = arena_case(shape, delta_t)
    state0 = random_state(7, shape[0], shape[1], delta_t)
    ids, ev_ptr = [6, 2, 0, 3, 5], [0, 2, 2, 3, 5, 6]
    results = []
    for null in ('Yb', 'Y'):
        for phase in (0, 1):
            rc, out, guards = arena_run(m, state0, ids, ev_ptr, t, X, M, kind, delta_t, 8, phase, generic, spt,
                                        null=null)
            assert rc == 0 and guards == [], (null, phase, guards)
            assert out['status'] == [0] * 5 and out['n_done'] == [2, 0, 1, 2, 1]
            assert all(torch.isfinite(v).all() for k, v in out['f32'].items() if k[0] != 'Y')
            full, nothing = ('Y', 'Yb') if null == 'Yb' else ('Yb', 'Y')
            assert torch.isfinite(out['f32'][full]).all()
            assert torch.equal(out[nothing], out['image'][nothing])
            results.append(out)
    for k in ('h', 'last_X', 'tau', 'now'):
        assert all(torch.equal(results[0][k], r[k]) for r in results[1:]), k
    assert torch.equal(results[0]['Y'], results[1]['Y']) and torch.equal(results[2]['Yb'], results[3]['Yb'])
