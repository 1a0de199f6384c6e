"""Online filtering on the GPU against the float64 oracle.

The truth of a series is the oracle's forward on the batch that consists of that series alone, with
``times`` = the targets of the calls in order (``online_util.truth``); the yardstick is
``check_vs_oracle(predict=True)``'s rule, err(online, f64) <= max(2 err(oracle fp32, f64), 2e-6) and
never looser than ATOL / RTOL, on h, Y_before, Y and the predictions (``online_util.Worst``).

Worst measured err(online, f64) / err(o32, f64) (MI355X): masked shapes 1.63 (hT, 3.1e-7 against
1.9e-7), the 41-wide residual shape at most 1.41; unmasked shapes 6.9 (hT 3.1e-7 against 4.5e-8: both at
fp32 rounding, it passes on the 2e-6 floor).
"""
import ctypes

import numpy as np
import pytest
import torch

import guarded
import hip_util
import online_util
from njode_amd import _lib, schedule, synthetic_physionet
from njode_amd.build import CONFIGS
from online_util import Worst, model_cfg, params_of, series_events, truth

pytestmark = pytest.mark.gpu

DT = 2.0 ** -10


def make_model(i):
    cfg = model_cfg(CONFIGS[i])
    sd = params_of(cfg, seed=i)
    return cfg, sd, hip_util.hip_model(cfg, sd).eval()


def make_batch(c, N, seed=0):
    """(batch, delta_t, T): the smallest batches that take every branch of a shape."""
    if c[6]:
        b = synthetic_physionet.make_batch(batch_size=N, dim=c[0], n_grid=40, n_obs_range=(3, 6), seed=seed)
        b['start_X'] = 0.1 * torch.randn(N, c[0], generator=torch.Generator().manual_seed(seed))
        return b, b['delta_t'], b['T']
    return hip_util.exact_k_batch(N, 12, obs_per_path=3, seed=seed, d=c[0])


def slices(b):
    ptr = np.asarray(b['time_ptr'])
    for i, t in enumerate(np.asarray(b['times'], dtype=np.float64)):
        lo, hi = int(ptr[i]), int(ptr[i + 1])
        if hi > lo:
            yield float(t), lo, hi, b['obs_idx'][lo:hi].numpy()


def bits(st):
    return [t.clone() for t in (st.h, st.last_X, st.tau, st.now)]


def same_bits(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


# ---- 1. every accepted shape ---------------------------------------------------------------------
@pytest.mark.parametrize('N', [5, 1, 9])
@pytest.mark.parametrize('i', online_util.ACCEPTED)
def test_every_shape(i, N):
    """reset, the batch slice by slice, advance(T): Y_before, Y and h after every jump and the final
    h against the per-series oracle; replay gives the same bits as the slice-by-slice calls."""
    c = CONFIGS[i]
    cfg, sd, m = make_model(i)
    b, delta_t, T = make_batch(c, N, seed=i)
    M = b.get('M')
    st = m.online(N, delta_t)
    st.reset(b['start_X'])
    got = {}      # (series, event number) -> (Y_before, Y, h)
    n_ev = [0] * N
    for t, lo, hi, ids in slices(b):
        yb, y = st.observe(np.full(hi - lo, t), b['X'][lo:hi], None if M is None else M[lo:hi], ids=ids)
        h = st.h[torch.as_tensor(ids, device='cuda')].cpu().numpy()
        for k, s in enumerate(ids):
            got[(int(s), n_ev[s])] = (yb[k].cpu().numpy(), y[k].cpu().numpy(), h[k])
            n_ev[s] += 1
    st.advance(np.full(N, T))
    st.check()
    hT = st.h.cpu().numpy()
    assert np.array_equal(st.tau.cpu().numpy(),
                          np.asarray([(series_events(b, s) or [(0.0,)])[-1][0] for s in range(N)], dtype=np.float32))

    st2 = m.online(N, delta_t)
    st2.reset(b['start_X'])
    yb2, y2 = st2.replay(b['times'], b['time_ptr'], b['X'], b['obs_idx'], M)
    st2.advance(np.full(N, T))
    st2.check()
    assert same_bits(bits(st), bits(st2))
    assert torch.isfinite(yb2).all() and torch.isfinite(y2).all()
    r0 = int(np.asarray(b['time_ptr'])[1]) - 1      # (the first slice's last row)
    assert r0 >= 0
    s0 = int(b['obs_idx'][r0])
    assert np.array_equal(y2[r0].cpu().numpy(), got[(s0, 0)][1]) and np.array_equal(yb2[r0].cpu().numpy(), got[(s0, 0)][0])

    w = Worst()
    for s in range(N):
        ev = series_events(b, s)
        o32, o64, rows = truth(cfg, sd, ev, b['start_X'][s], delta_t, T)
        for k, r in enumerate(rows):
            yb, y, h = got[(s, k)]
            w.add('Y_before', yb, o32['path_y'][r - 1, 0], o64['path_y'][r - 1, 0])
            w.add('Y', y, o32['path_y'][r, 0], o64['path_y'][r, 0])
            w.add('h', h, o32['path_h'][r, 0], o64['path_h'][r, 0])
        w.add('hT', hT[s], o32['hT'][0], o64['hT'][0])
    w.check('cfg{} N={}'.format(i, N))


# ---- 2. the clock's branches ----------------------------------------------------------------------
CLOCK_TIMES = np.asarray([       # [series][call], in units of delta_t = 0.37 dt; off the grid
    [0.0, 0.0, 0.5, 3.5],        # t = 0 observation, the same time again, a partial step, 3 full steps
    [0.4, 0.4, 3.1, 3.1],        # a partial step, the same time again, 2 full + 1 partial, target == now
    [2.0, 4.3, 4.3, 9.6],        # exactly 2 full steps (2 delta_t - delta_t is exact)
    [0.0, 5.25, 5.25, 5.5]])


@pytest.mark.parametrize('i', [online_util.DEMO, online_util.PHYSIO])
def test_clock_branches(i):
    c = CONFIGS[i]
    cfg, sd, m = make_model(i)
    d, delta_t = c[0], 0.37 * DT
    times = CLOCK_TIMES * delta_t
    N, n_calls = times.shape
    g = torch.Generator().manual_seed(7)
    start = 0.2 * torch.randn(N, d, generator=g)
    X = 0.5 * torch.randn(n_calls, N, d, generator=g)
    M = (torch.rand(n_calls, N, d, generator=g) < 0.3).float() if c[6] else None
    # the branches the issue lists are really taken, and differ between the series of one call
    kinds = set()
    for s in range(N):
        dts, _, k_jump, _, _ = schedule._walk_clock(times[s], delta_t, 0.0, False)
        for j in range(n_calls):
            mine = dts[(k_jump[j - 1] if j else 0):k_jump[j]]
            full = sum(1 for x in mine if x == delta_t)
            kinds.add((min(full, 2), len(mine) - full))
    assert {(0, 0), (0, 1), (2, 0), (2, 1)} <= kinds, kinds

    st = m.online(N, delta_t)
    st.reset(start)
    w = Worst()
    outs = []
    for j in range(n_calls):
        yb, y = st.observe(times[:, j], X[j], None if M is None else M[j])
        outs.append((yb.cpu().numpy(), y.cpu().numpy(), st.h.cpu().numpy()))
    st.check()
    for s in range(N):
        ev = [(times[s, j], X[j, s], None if M is None else M[j, s]) for j in range(n_calls)]
        o32, o64, rows = truth(cfg, sd, ev, start[s], delta_t)
        for j, r in enumerate(rows):
            w.add('Y_before', outs[j][0][s], o32['path_y'][r - 1, 0], o64['path_y'][r - 1, 0])
            w.add('Y', outs[j][1][s], o32['path_y'][r, 0], o64['path_y'][r, 0])
            w.add('h', outs[j][2][s], o32['path_h'][r, 0], o64['path_h'][r, 0])
        # now moves through Euler steps only; tau is the fp32 time of the last jump
        dts = schedule._walk_clock(times[s], delta_t, 0.0, False)[0]
        now = 0.0
        for x in dts:
            now = now + x
        assert float(st.now[s]) == now and float(st.tau[s]) == float(np.float32(times[s, -1]))
    w.check('clock cfg{}'.format(i))


# ---- 3. predict, 4. advance then observe ----------------------------------------------------------
@pytest.fixture(scope='module')
def warm():
    """Demo-shaped and masked states after two observations each (shared, never modified: the
    tests below work on copies of the four tensors)."""
    out = {}
    for i in (online_util.DEMO, online_util.PHYSIO):
        c = CONFIGS[i]
        cfg, sd, m = make_model(i)
        d, delta_t, N = c[0], 0.37 * DT, 3
        g = torch.Generator().manual_seed(11 + i)
        start = 0.2 * torch.randn(N, d, generator=g)
        t_obs = np.asarray([[0.0, 2.2], [1.3, 1.3], [0.6, 4.9]]) * delta_t
        X = 0.5 * torch.randn(2, N, d, generator=g)
        M = (torch.rand(2, N, d, generator=g) < 0.3).float() if c[6] else None
        st = m.online(N, delta_t)
        st.reset(start)
        for j in range(2):
            st.observe(t_obs[:, j], X[j], None if M is None else M[j])
        st.check()
        ev = [[(t_obs[s, j], X[j, s], None if M is None else M[j, s]) for j in range(2)] for s in range(N)]
        out[i] = dict(cfg=cfg, sd=sd, m=m, st=st, sd0=st.state_dict(), ev=ev, start=start, delta_t=delta_t,
                      d=d, masked=bool(c[6]), N=N)
    return out


def fresh(wm):
    st = wm['m'].online(wm['N'], wm['delta_t'])
    st.load_state_dict(wm['sd0'])
    return st


@pytest.mark.parametrize('i', [online_util.DEMO, online_util.PHYSIO])
def test_predict(warm, i):
    wm = warm[i]
    st, dl = fresh(wm), wm['delta_t']
    before = bits(st)
    # off the grid, a repeated query, a query at the clock itself (series 1: no step at all)
    q3 = np.asarray([[2.2, 3.0, 3.0], [1.3, 1.3, 7.77], [5.0, 5.9, 12.45]]) * dl
    q1 = q3[:, 2:]
    w = Worst()
    for tag, q in (('Q1', q1), ('Q3', q3)):
        y = st.predict(q)
        assert same_bits(before, bits(st)), tag
        assert torch.equal(y.view(torch.int32), st.predict(q).view(torch.int32)), tag
        y = y.cpu().numpy()
        for s in range(wm['N']):
            ev = wm['ev'][s] + [(t, None, None) for t in q[s]]
            o32, o64, rows = truth(wm['cfg'], wm['sd'], ev, wm['start'][s], dl)
            for k, r in enumerate(rows[2:]):
                w.add('pred', y[s, k], o32['path_y'][r, 0], o64['path_y'][r, 0])
    st.check()
    assert same_bits(before, bits(st))
    # a subset, out of order: the rows of the full call
    ys = st.predict(q3[[2, 0]], ids=[2, 0])
    assert torch.equal(ys.view(torch.int32), st.predict(q3)[[2, 0]].view(torch.int32))
    w.check('predict cfg{}'.format(i))


@pytest.mark.parametrize('i', [online_util.DEMO, online_util.PHYSIO])
def test_advance_then_observe(warm, i):
    wm = warm[i]
    st, dl, N, d = fresh(wm), wm['delta_t'], wm['N'], wm['d']
    t1 = np.asarray([3.3, 1.3, 6.05]) * dl
    t2 = np.asarray([3.3, 4.4, 9.5]) * dl
    g = torch.Generator().manual_seed(5)
    X = 0.5 * torch.randn(N, d, generator=g)
    M = (torch.rand(N, d, generator=g) < 0.3).float() if wm['masked'] else None
    keep = bits(st)
    st.advance(t1)
    assert torch.equal(keep[1], st.last_X) and torch.equal(keep[2], st.tau)    # an empty slice: no jump
    yb, y = st.observe(t2, X, M)
    st.check()
    w = Worst()
    for s in range(N):
        ev = wm['ev'][s] + [(t1[s], None, None), (t2[s], X[s], None if M is None else M[s])]
        o32, o64, rows = truth(wm['cfg'], wm['sd'], ev, wm['start'][s], dl)
        r = rows[-1]
        w.add('Y_before', yb[s].cpu().numpy(), o32['path_y'][r - 1, 0], o64['path_y'][r - 1, 0])
        w.add('Y', y[s].cpu().numpy(), o32['path_y'][r, 0], o64['path_y'][r, 0])
        w.add('h', st.h[s].cpu().numpy(), o32['path_h'][r, 0], o64['path_h'][r, 0])
    w.check('advance+observe cfg{}'.format(i))


# ---- 5. subsets of series -----------------------------------------------------------------------
@pytest.mark.parametrize('i', [online_util.DEMO, online_util.PHYSIO])
def test_subsets(i):
    c = CONFIGS[i]
    cfg, sd, m = make_model(i)
    d, delta_t, N = c[0], 0.37 * DT, 5
    g = torch.Generator().manual_seed(3)
    start = 0.2 * torch.randn(N, d, generator=g)
    X = 0.5 * torch.randn(N, d, generator=g)
    M = (torch.rand(N, d, generator=g) < 0.3).float() if c[6] else None
    t = np.asarray([2.5, 0.0, 9.0, 4.2, 1.0]) * delta_t
    a, b = m.online(N, delta_t), m.online(N, delta_t)
    a.reset(start)
    b.reset(start)
    start_bits = bits(a)

    def rows(ids):
        return t[ids], X[ids], None if M is None else M[ids]

    ya = {}
    for ids in ([3, 0], [1]):
        tt, xx, mm = rows(ids)
        yb, y = a.observe(tt, xx, mm, ids=ids)
        for k, s in enumerate(ids):
            ya[s] = (yb[k], y[k])
    tt, xx, mm = rows([0, 1, 3])
    yb, y = b.observe(tt, xx, mm, ids=[0, 1, 3])
    a.check()
    b.check()
    assert same_bits(bits(a), bits(b))
    for k, s in enumerate([0, 1, 3]):
        assert torch.equal(ya[s][0].view(torch.int32), yb[k].view(torch.int32))
        assert torch.equal(ya[s][1].view(torch.int32), y[k].view(torch.int32))
    for x0, x1 in zip(start_bits, bits(a)):     # the series not named: bitwise unchanged
        assert torch.equal(x0[[2, 4]].contiguous().view(torch.uint8), x1[[2, 4]].contiguous().view(torch.uint8))
    assert not torch.equal(start_bits[0][[0, 1, 3]], a.h[[0, 1, 3]])


# ---- 6. the batch kernels, where the clocks coincide --------------------------------------------
def test_agrees_with_batch_route():
    b, meta = hip_util.bs_batch(7)
    delta_t, T = meta['dt'], meta['maturity']
    cfg = hip_util.demo_cfg()
    sd = params_of(cfg, seed=2)
    m = hip_util.hip_model(cfg, sd).eval()
    with torch.no_grad():
        hT, _, path_t, _, path_y = hip_util.hip_forward(m, b, delta_t, T, return_path=True, get_loss=False,
                                                        until_T=True)
    rows_b = schedule.Schedule(b['times'], delta_t, T, True).row_of_jump
    st = m.online(7, delta_t)
    st.reset(b['start_X'])
    _, y = st.replay(b['times'], b['time_ptr'], b['X'], b['obs_idx'])
    ptr = np.asarray(b['time_ptr'])
    for i in range(len(b['times'])):
        for r in range(int(ptr[i]), int(ptr[i + 1])):
            s = int(b['obs_idx'][r])
            np.testing.assert_allclose(y[r].cpu().numpy(), path_y[rows_b[i], s].cpu().numpy(), atol=hip_util.ATOL,
                                       rtol=hip_util.RTOL)
    st.advance(np.full(7, T))
    st.check()
    np.testing.assert_allclose(st.h.cpu().numpy(), hT.cpu().numpy(), atol=hip_util.ATOL, rtol=hip_util.RTOL)


# ---- 7. the bound -----------------------------------------------------------------------------------
@pytest.mark.parametrize('i', [online_util.DEMO, online_util.PHYSIO])
def test_bound(i):
    c = CONFIGS[i]
    cfg, sd, m = make_model(i)
    d, delta_t, N = c[0], 0.37 * DT, 4
    g = torch.Generator().manual_seed(9)
    start = 0.2 * torch.randn(N, d, generator=g)
    X = 0.5 * torch.randn(N, d, generator=g)
    M = (torch.rand(N, d, generator=g) < 0.3).float() if c[6] else None
    t = np.asarray([1.5, 5.5, 1.5, 2.5]) * delta_t      # series 1: 6 steps ahead (5 full, 1 partial)
    assert [len(schedule._walk_clock([x], delta_t, 0.0, False)[0]) for x in t] == [2, 6, 2, 3]
    st, free = m.online(N, delta_t), m.online(N, delta_t)
    st.reset(start)
    free.reset(start)
    yb, y = st.observe(t, X, M, max_steps=3)
    assert st.status.cpu().tolist() == [0, 1, 0, 0]
    with pytest.raises(RuntimeError, match=r'\[1\]'):
        st.check()
    assert torch.isnan(y[1]).all() and torch.isnan(yb[1]).all()
    # series 1: three steps, no jump -- path row 3 of its walk (row 0 the start, row k behind step k)
    w = Worst()
    o32, o64, rows = truth(cfg, sd, [(t[1], None, None)], start[1], delta_t)
    assert rows[0] == 7
    w.add('h', st.h[1].cpu().numpy(), o32['path_h'][3, 0], o64['path_h'][3, 0])
    assert float(st.tau[1]) == 0.0 and torch.equal(st.last_X[1].cpu(), start[1])
    assert float(st.now[1]) == delta_t + delta_t + delta_t
    for s in (0, 2, 3):
        o32, o64, rows = truth(cfg, sd, [(t[s], X[s], None if M is None else M[s])], start[s], delta_t)
        w.add('Y', y[s].cpu().numpy(), o32['path_y'][rows[0], 0], o64['path_y'][rows[0], 0])
        w.add('h', st.h[s].cpu().numpy(), o32['path_h'][rows[0], 0], o64['path_h'][rows[0], 0])
    w.check('bound cfg{}'.format(i))
    # a second call with a sufficient bound ends where an unbounded walk does
    one = [1]
    yb2, y2 = st.observe(t[one], X[one], None if M is None else M[one], ids=one)
    yf, yy = free.observe(t, X, M)
    st.check()
    free.check()
    assert same_bits(bits(st), bits(free))
    assert torch.equal(y2[0].view(torch.int32), yy[1].view(torch.int32))
    assert torch.equal(yb2[0].view(torch.int32), yf[1].view(torch.int32))


# ---- 8. stated sizes ------------------------------------------------------------------------------
@pytest.mark.parametrize('i', [online_util.DEMO, online_util.PHYSIO])
def test_stated_sizes(i):
    """One observe and one predict with every buffer carved from a guard-band arena at exactly the
    header's lengths: guards intact, the same bits under both arena phases."""
    c = CONFIGS[i]
    cfg, sd, m = make_model(i)
    d, H, DO = c[0], c[1], c[2]
    S, n, Q, delta_t = 7, 5, 3, 0.37 * DT
    g = torch.Generator().manual_seed(13)
    h0 = 0.3 * torch.randn(S, H, generator=g)
    x0 = 0.3 * torch.randn(S, d, generator=g)
    tau0 = torch.tensor([0.0, 1.0, 0.5, 2.0, 0.0, 0.25, 3.0]) * delta_t
    now0 = tau0.double() + 0.1 * delta_t
    ids = torch.tensor([6, 2, 0, 3, 5], dtype=torch.int32)
    t = now0[ids.long()] + torch.tensor([0.0, 0.4, 2.0, 3.7, 1.0], dtype=torch.float64) * delta_t
    tq = t[:, None] + torch.tensor([0.0, 0.5, 2.5], dtype=torch.float64)[None] * delta_t
    X = 0.5 * torch.randn(n, d, generator=g)
    M = (torch.rand(n, d, generator=g) < 0.3).float()
    m._ensure_flat(full=True)
    P = m._flat.detach().clone()
    dims = m._get_dims()
    L = _lib.lib()
    results = []
    for phase in (0, 1):
        ar = guarded.Arena('cuda', phase=phase)
        ar.add('P', 4 * P.numel(), 'nan32').add('h', 4 * S * H, 'nan32').add('last_X', 4 * S * d, 'nan32')
        ar.add('tau', 4 * S, 'nan32').add('now', 8 * S, 'nan64').add('ids', 4 * n, 'index', modulo=S)
        ar.add('t', 8 * n, 'nan64').add('tq', 8 * n * Q, 'nan64').add('X', 4 * n * d, 'nan32')
        ar.add('M', 4 * n * d, 'nan32')
        ar.add('Yb', 4 * n * DO).add('Y', 4 * n * DO).add('Yq', 4 * n * Q * DO).add('status', 4 * n)
        ar.add('status_q', 4 * n)
        ar.build()
        for name, v in (('P', P), ('h', h0), ('last_X', x0), ('tau', tau0), ('now', now0), ('ids', ids), ('t', t),
                        ('tq', tq), ('X', X), ('M', M)):
            ar.put(name, v.cuda())
        state = _lib.NjodeOnlineState(ar.ptr('h'), ar.ptr('last_X'), ar.ptr('tau'), ar.ptr('now'), S)
        stream = _lib.stream_arg(torch.device('cuda'))
        _lib.check(L.njode_online_predict_f32(ctypes.byref(dims), ar.ptr('P'), ctypes.byref(state), ar.ptr('ids'), n,
                                              ar.ptr('tq'), Q, delta_t, 8, ar.ptr('Yq'), ar.ptr('status_q'), stream))
        _lib.check(L.njode_online_observe_f32(ctypes.byref(dims), ar.ptr('P'), ctypes.byref(state), ar.ptr('ids'), n,
                                              ar.ptr('t'), ar.ptr('X'), ar.ptr('M') if c[6] else None, delta_t, 8,
                                              ar.ptr('Yb'), ar.ptr('Y'), ar.ptr('status'), stream))
        assert ar.check() == []
        assert ar.view('status', torch.int32).tolist() == [0] * n
        assert ar.view('status_q', torch.int32).tolist() == [0] * n
        out = {k: ar.view(k).clone() for k in ('h', 'last_X', 'tau', 'now', 'Yb', 'Y', 'Yq')}
        assert all(torch.isfinite(ar.view(k, torch.float32)).all() for k in ('h', 'last_X', 'tau', 'Yb', 'Y', 'Yq'))
        results.append(out)
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k
