"""Online filtering on the shape-generic matrix-core kernels (``kernels='generic'``) on the GPU.

The truth of a series is the oracle's forward on the batch that consists of that series alone, with
``times`` = the targets of the calls in order (``online_util.truth``); the yardstick is
``check_vs_oracle(predict=True)``'s rule, err(online, f64) <= max(2 err(oracle fp32, f64), 2e-6) and
never looser than ATOL / RTOL, on h, Y_before, Y and the predictions (``online_util.Worst``).  Where
the batch call of a shape runs the same kernel family, the online results are held to its rows in
bits.

Worst measured err(online, f64) / err(o32, f64) per shape class (MI355X): wide / deep unmasked shapes
2.58 (``Y_before`` of a state taken over from the wave family on the demo shape, 2.18e-7 against
8.45e-8), 2.44 within this family (``one_layer_easy`` N = 1, ``Y_before`` 2.41e-7 against 9.88e-8);
masked shapes 2.19 (``d8_h4`` N = 5, ``Y_before`` 6.34e-7 against 2.90e-7); GRU-jump shapes 1.99
(``gru_w80`` N = 19, ``Y_before`` 2.77e-7 against 1.39e-7).  Every figure above 2 is at fp32 rounding
and passes on the 2e-6 floor; the largest absolute error is 1.69e-6 (``hT`` of the 41-wide PhysioNet
shape, where the fp32 oracle has 1.84e-6).
"""
import ctypes

import numpy as np
import pytest
import torch

import guarded
import hip_util
import online_gen_util as ogu
import online_util
from njode_amd import _lib, schedule
from online_gen_util import bits, eq_bits, same_bits, slices
from online_util import Worst, series_events, truth
from test_hip_online import CLOCK_TIMES

pytestmark = pytest.mark.gpu

DT = 2.0 ** -10


@pytest.fixture(scope='module')
def model_of():
    """name -> (cfg, sd, model), built once per shape and never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ogu.make_model(name, seed=sorted(ogu.SHAPES).index(name))
        return cache[name]
    return get


def run_batch(m, b, N, delta_t, T, spt, replay=False):
    """reset, the batch (slice by slice, or through replay), advance(T).  Returns the state and
    {(series, event number): (Y_before, Y, h after the jump)}."""
    M = b.get('M')
    st = ogu.online(m, N, delta_t, spt)
    st.reset(b['start_X'])
    got, n_ev = {}, [0] * N
    if replay:
        yb, y = st.replay(b['times'], b['time_ptr'], b['X'], b['obs_idx'], M)
        for r, s in enumerate(b['obs_idx'].tolist()):
            got[(s, n_ev[s])] = (yb[r].cpu().numpy(), y[r].cpu().numpy(), None)
            n_ev[s] += 1
    else:
        for t, lo, hi, ids in slices(b):
            yb, y = st.observe(np.full(hi - lo, t), b['X'][lo:hi], None if M is None else M[lo:hi], ids=ids)
            h = st.h[torch.as_tensor(ids, device='cuda')].cpu().numpy()
            for k, s in enumerate(ids):
                got[(int(s), n_ev[s])] = (yb[k].cpu().numpy(), y[k].cpu().numpy(), h[k])
                n_ev[s] += 1
    st.advance(np.full(N, T))
    st.check()
    return st, got


# ---- 1. every branch of the kernel ------------------------------------------------------------------
# (N, series_per_tile): a lone series in a tile of 1; one ragged tile of 16; 19 series under the
# library's rule (tiles of 1), in a full tile of 16 plus a ragged one of 3, and in five tiles of 4 with
# a ragged last one; the climate shape at N = 5 only
CASES = [(name, N, spt) for name in sorted(ogu.SHAPES)
         for N, spt in ((1, None), (5, 16), (19, None), (19, 16), (19, 4))
         if name != 'climate_w400_h50' or N == 5]


@pytest.mark.parametrize('name,N,spt', CASES)
def test_every_shape(model_of, name, N, spt):
    cfg, sd, m = model_of(name)
    b, delta_t, T = ogu.make_batch(cfg, N, seed=3)
    st, got = run_batch(m, b, N, delta_t, T, spt)
    hT = st.h.cpu().numpy()
    last = np.asarray([(series_events(b, s) or [(0.0,)])[-1][0] for s in range(N)], dtype=np.float32)
    assert np.array_equal(st.tau.cpu().numpy(), last)
    st2, got2 = run_batch(m, b, N, delta_t, T, spt, replay=True)
    assert same_bits(bits(st), bits(st2))
    for key, (yb, y, _) in got2.items():
        assert np.array_equal(yb, got[key][0]) and np.array_equal(y, got[key][1]), key
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
    w.check('{} N={} spt={}'.format(name, N, spt))


# ---- 2. bit identities --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ogu.GENERIC_BATCH)
def test_bits_of_the_batch_kernel(model_of, name):
    """Y_before, Y, h after each jump and hT of every series = the rows of the batch call on the
    batch of that series alone (the same family's k_gen_fwd), in bits."""
    cfg, sd, m = model_of(name)
    N = 5
    b, delta_t, T = ogu.make_batch(cfg, N, seed=5)
    st, got = run_batch(m, b, N, delta_t, T, 16)
    hT = st.h.cpu()
    for s in range(N):
        ev = series_events(b, s)
        b1 = online_util.batch_of_one(ev, b['start_X'][s], cfg['input_size'], ogu.is_masked(cfg))
        with torch.no_grad():
            h1, _, _, path_h, path_y = hip_util.hip_forward(m, b1, delta_t, T, return_path=True, get_loss=False,
                                                            until_T=True)
        rows = schedule._walk_clock(b1['times'], delta_t, T, True)[4]
        path_h, path_y = path_h.cpu().numpy(), path_y.cpu().numpy()
        for k, r in enumerate(rows):
            yb, y, h = got[(s, k)]
            assert np.array_equal(yb.view(np.int32), path_y[r - 1, 0].view(np.int32)), (name, s, k, 'Y_before')
            assert np.array_equal(y.view(np.int32), path_y[r, 0].view(np.int32)), (name, s, k, 'Y')
            assert np.array_equal(h.view(np.int32), path_h[r, 0].view(np.int32)), (name, s, k, 'h')
        assert eq_bits(hT[s], h1.cpu()[0]), (name, s, 'hT')


@pytest.mark.parametrize('name', ['w80', 'gru_masked', 'w160'])
def test_bits_do_not_depend_on_the_tile(model_of, name):
    """A series alone in a tile of 1, alone in a tile of 16, and in column 5 of a tile beside 8
    series with other targets: the same bits.  The same call on the same state: the same bits."""
    cfg, sd, m = model_of(name)
    d, delta_t, S = cfg['input_size'], 0.37 * DT, 9
    masked = ogu.is_masked(cfg)
    g = torch.Generator().manual_seed(21)
    start = 0.2 * torch.randn(S, d, generator=g)
    X = 0.5 * torch.randn(S, d, generator=g)
    M = (torch.rand(S, d, generator=g) < 0.4).float() if masked else None
    t = np.asarray([0.0, 7.3, 1.0, 4.4, 2.0, 3.3, 9.9, 0.5, 6.0]) * delta_t
    tq = t[:, None] + np.asarray([0.0, 0.7, 2.5])[None] * delta_t
    k = 5
    outs = []
    for spt, ids in ((1, [k]), (16, [k]), (16, [3, 8, 0, 6, 1, k, 2, 7, 4]), (4, list(range(S)))):
        st = ogu.online(m, S, delta_t, spt)
        st.reset(start)
        pos = ids.index(k)
        yb, y = st.observe(t[ids], X[ids], None if M is None else M[ids], ids=ids)
        yq = st.predict(tq[ids], ids=ids)
        keep = bits(st)
        yq2 = st.predict(tq[ids], ids=ids)
        assert eq_bits(yq, yq2) and same_bits(keep, bits(st))
        st.check()
        outs.append([yb[pos], y[pos], yq[pos]] + [x[k] for x in bits(st)])
    for other in outs[1:]:
        assert same_bits(outs[0], other)
    assert torch.isfinite(outs[0][2]).all()


# ---- 3. the clock's branches, four series in ONE tile ---------------------------------------------------
@pytest.mark.parametrize('name', ['w80', 'gru_masked'])
def test_clock_branches(model_of, name):
    cfg, sd, m = model_of(name)
    d, delta_t = cfg['input_size'], 0.37 * DT
    masked = ogu.is_masked(cfg)
    times = CLOCK_TIMES * delta_t
    N, n_calls = times.shape
    g = torch.Generator().manual_seed(7)
    start = 0.2 * torch.randn(N, d, generator=g)
    X = 0.5 * torch.randn(n_calls, N, d, generator=g)
    M = (torch.rand(n_calls, N, d, generator=g) < 0.3).float() if masked else None
    kinds = set()       # the branches are really taken, and differ between the series of one call
    for s in range(N):
        dts, _, k_jump, _, _ = schedule._walk_clock(times[s], delta_t, 0.0, False)
        for j in range(n_calls):
            mine = dts[(k_jump[j - 1] if j else 0):k_jump[j]]
            full = sum(1 for x in mine if x == delta_t)
            kinds.add((min(full, 2), len(mine) - full))
    assert {(0, 0), (0, 1), (2, 0), (2, 1)} <= kinds, kinds

    st = ogu.online(m, N, delta_t, 16)
    st.reset(start)
    w, outs = Worst(), []
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
        now = 0.0
        for x in schedule._walk_clock(times[s], delta_t, 0.0, False)[0]:
            now = now + x
        assert float(st.now[s]) == now and float(st.tau[s]) == float(np.float32(times[s, -1]))
    w.check('clock {}'.format(name))


# ---- 4. predict ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def warm(model_of):
    """States after two observations per series (shared; the tests work on copies)."""
    out = {}
    for name in ('w80', 'gru_masked'):
        cfg, sd, m = model_of(name)
        d, delta_t, N = cfg['input_size'], 0.37 * DT, 3
        masked = ogu.is_masked(cfg)
        g = torch.Generator().manual_seed(11)
        start = 0.2 * torch.randn(N, d, generator=g)
        t_obs = np.asarray([[0.0, 2.2], [1.3, 1.3], [0.6, 4.9]]) * delta_t
        X = 0.5 * torch.randn(2, N, d, generator=g)
        M = (torch.rand(2, N, d, generator=g) < 0.3).float() if masked else None
        st = ogu.online(m, N, delta_t)
        st.reset(start)
        for j in range(2):
            st.observe(t_obs[:, j], X[j], None if M is None else M[j])
        st.check()
        ev = [[(t_obs[s, j], X[j, s], None if M is None else M[j, s]) for j in range(2)] for s in range(N)]
        out[name] = dict(cfg=cfg, sd=sd, m=m, sd0=st.state_dict(), ev=ev, start=start, delta_t=delta_t, d=d,
                         masked=masked, N=N)
    return out


def fresh(wm, spt=None):
    st = ogu.online(wm['m'], wm['N'], wm['delta_t'], spt)
    st.load_state_dict(wm['sd0'])
    return st


@pytest.mark.parametrize('name', ['w80', 'gru_masked'])
def test_predict(warm, name):
    wm = warm[name]
    st, dl, N, d = fresh(wm, 16), wm['delta_t'], wm['N'], wm['d']
    before = bits(st)
    # off the grid and different per series, a repeated query, a query at the clock itself
    q5 = np.asarray([[2.2, 3.0, 3.0, 4.6, 9.1], [1.3, 1.3, 7.77, 7.77, 8.0], [5.0, 5.9, 12.45, 12.45, 13.0]]) * dl
    q1 = q5[:, 2:3]
    w = Worst()
    for tag, q in (('Q1', q1), ('Q5', q5)):
        y = st.predict(q)
        assert same_bits(before, bits(st)), tag
        yn = y.cpu().numpy()
        for s in range(N):
            ev = wm['ev'][s] + [(t, None, None) for t in q[s]]
            o32, o64, rows = truth(wm['cfg'], wm['sd'], ev, wm['start'][s], dl)
            for k, r in enumerate(rows[2:]):
                w.add('pred', yn[s, k], o32['path_y'][r, 0], o64['path_y'][r, 0])
        # advance to each query in turn, then observe there: Y_before is the forecast
        for k in range(q.shape[1]):
            walk = fresh(wm, 16)
            for j in range(k):
                walk.advance(q[:, j])
            x = torch.zeros(N, d)
            yb, _ = walk.observe(q[:, k], x, torch.ones(N, d) if wm['masked'] else None)
            walk.check()
            assert eq_bits(y[:, k], yb), (tag, k)
    st.check()
    assert same_bits(before, bits(st))
    ys = st.predict(q5[[2, 0]], ids=[2, 0])
    assert eq_bits(ys, st.predict(q5)[[2, 0]])
    w.check('predict {}'.format(name))


# ---- 5. subsets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['w80', 'gru_masked'])
def test_subsets(model_of, name):
    cfg, sd, m = model_of(name)
    d, delta_t, N = cfg['input_size'], 0.37 * DT, 11
    masked = ogu.is_masked(cfg)
    g = torch.Generator().manual_seed(3)
    start = 0.2 * torch.randn(N, d, generator=g)
    X = 0.5 * torch.randn(N, d, generator=g)
    M = (torch.rand(N, d, generator=g) < 0.3).float() if masked else None
    t = np.asarray([2.5, 0.0, 9.0, 4.2, 1.0, 3.3, 0.4, 7.0, 2.0, 5.5, 6.1]) * delta_t
    a, b = ogu.online(m, N, delta_t, 4), ogu.online(m, N, delta_t, 4)
    a.reset(start)
    b.reset(start)
    start_bits = bits(a)
    listed = [9, 3, 0, 7, 1, 10, 5]             # permuted, 7 rows: one full tile of 4 and a ragged one
    rest = [2, 4, 6, 8]

    def rows(ids):
        return t[ids], X[ids], None if M is None else M[ids]

    ya = {}
    for ids in ([3, 0, 10], [1], [7, 9, 5]):
        yb, y = a.observe(*rows(ids), ids=ids)
        for k, s in enumerate(ids):
            ya[s] = (yb[k], y[k])
    yb, y = b.observe(*rows(listed), ids=listed)
    a.check()
    b.check()
    assert same_bits(bits(a), bits(b))
    for k, s in enumerate(listed):
        assert eq_bits(ya[s][0], yb[k]) and eq_bits(ya[s][1], y[k])
    for x0, x1 in zip(start_bits, bits(a)):     # the series not named: bitwise unchanged
        assert eq_bits(x0[rest], x1[rest])
    assert not torch.equal(start_bits[0][listed], a.h[listed])

    # a bad id through the C ABI: status 2, nothing touched; its neighbours in the tile run
    ids = torch.tensor([2, N, 4, -1, 6], dtype=torch.int32, device='cuda')
    tt = torch.as_tensor(t[[2, 0, 4, 0, 6]], device='cuda')
    xx = X[[2, 0, 4, 0, 6]].cuda().contiguous()
    mm = M[[2, 0, 4, 0, 6]].cuda().contiguous() if masked else None
    status = torch.full((5,), -7, dtype=torch.int32, device='cuda')
    yb = torch.full((5, cfg['output_size']), 123.0, device='cuda')
    y = yb.clone()
    keep = bits(a)
    P = a._params()
    _lib.check(_lib.lib().njode_online_gen_observe_f32(
        *a._gen_head(P), ctypes.byref(a._struct()), ids.data_ptr(), 5, tt.data_ptr(), xx.data_ptr(), _lib.ptr_arg(mm),
        delta_t, 64, 16, yb.data_ptr(), y.data_ptr(), status.data_ptr(), _lib.stream_arg(a.device)))
    assert status.tolist() == [0, 2, 0, 2, 0]
    assert (yb[[1, 3]] == 123.0).all() and (y[[1, 3]] == 123.0).all()
    for x0, x1 in zip(keep, bits(a)):
        assert eq_bits(x0[[8] + listed], x1[[8] + listed])
    ref_yb, ref_y = b.observe(*rows([2, 4, 6]), ids=[2, 4, 6])
    assert eq_bits(y[[0, 2, 4]], ref_y) and eq_bits(yb[[0, 2, 4]], ref_yb) and same_bits(bits(a), bits(b))


# ---- 6. the bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['w80', 'gru_masked'])
def test_bound(model_of, name):
    cfg, sd, m = model_of(name)
    d, delta_t, N = cfg['input_size'], 0.37 * DT, 4
    masked = ogu.is_masked(cfg)
    g = torch.Generator().manual_seed(9)
    start = 0.2 * torch.randn(N, d, generator=g)
    X = 0.5 * torch.randn(N, d, generator=g)
    M = (torch.rand(N, d, generator=g) < 0.3).float() if masked else None
    t = np.asarray([1.5, 5.5, 1.5, 2.5]) * delta_t      # series 1: 6 steps ahead (5 full, 1 partial)
    assert [len(schedule._walk_clock([x], delta_t, 0.0, False)[0]) for x in t] == [2, 6, 2, 3]
    st, free, adv = ogu.online(m, N, delta_t, 16), ogu.online(m, N, delta_t, 16), ogu.online(m, N, delta_t, 16)
    for x in (st, free, adv):
        x.reset(start)
    yb, y = st.observe(t, X, M, max_steps=3)
    assert st.status.cpu().tolist() == [0, 1, 0, 0]
    with pytest.raises(RuntimeError, match=r'\[1\]'):
        st.check()
    assert torch.isnan(y[1]).all() and torch.isnan(yb[1]).all()
    # the stopped series: the state advance reaches with that many steps, no jump
    adv.advance(t[[1]], ids=[1], max_steps=3)
    assert adv.status.cpu().tolist() == [1]
    assert all(eq_bits(p[1], q[1]) for p, q in zip(bits(st), bits(adv)))
    w = Worst()
    o32, o64, rows = truth(cfg, sd, [(t[1], None, None)], start[1], delta_t)
    assert rows[0] == 7
    w.add('h', st.h[1].cpu().numpy(), o32['path_h'][3, 0], o64['path_h'][3, 0])
    assert float(st.tau[1]) == 0.0 and torch.equal(st.last_X[1].cpu(), start[1])
    assert float(st.now[1]) == delta_t + delta_t + delta_t
    w.check('bound {}'.format(name))
    # the neighbours: the bits of a run without the stopped series
    others = [0, 2, 3]
    yfb, yf = free.observe(t[others], X[others], None if M is None else M[others], ids=others)
    assert eq_bits(y[others], yf) and eq_bits(yb[others], yfb)
    assert all(eq_bits(p[others], q[others]) for p, q in zip(bits(st), bits(free)))
    # predict: NaN from the query the series could not reach
    tq = np.stack([t, t + 4 * delta_t], axis=1)
    yq = free.predict(tq, max_steps=5)      # series 1 (still at 0): 6 steps to its first query
    assert free.status.cpu().tolist() == [0, 1, 0, 0]
    assert torch.isnan(yq[1]).all() and torch.isfinite(yq[others]).all()
    with pytest.raises(RuntimeError, match=r'\[1\]'):
        free.check()
    # a second call with a sufficient bound ends where an unbounded walk does
    yb2, y2 = st.observe(t[[1]], X[[1]], None if M is None else M[[1]], ids=[1])
    yfb, yf = free.observe(t[[1]], X[[1]], None if M is None else M[[1]], ids=[1])
    st.check()
    free.check()
    assert same_bits(bits(st), bits(free)) and eq_bits(y2, yf) and eq_bits(yb2, yfb)


# ---- 7. stated sizes ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['w160', 'gru_masked'])
def test_stated_sizes(model_of, name):
    """All four modes and the pack with every buffer -- the tables included -- carved from a
    guard-band arena at exactly the header's lengths, n = 5 rows in tiles of 4: guards intact, the
    same bits under both arena phases."""
    cfg, sd, m = model_of(name)
    d, H, DO = cfg['input_size'], cfg['hidden_size'], cfg['output_size']
    masked = ogu.is_masked(cfg)
    S, n, Q, delta_t, spt = 7, 5, 3, 0.37 * DT, 4
    g = torch.Generator().manual_seed(13)
    h0 = 0.3 * torch.randn(S, H, generator=g)
    x0 = 0.3 * torch.randn(S, d, generator=g)
    tau0 = torch.tensor([0.0, 1.0, 0.5, 2.0, 0.0, 0.25, 3.0]) * delta_t
    now0 = tau0.double() + 0.1 * delta_t
    ids = torch.tensor([6, 2, 0, 3, 5], dtype=torch.int32)
    t = now0[ids.long()] + torch.tensor([0.0, 0.4, 2.0, 3.7, 1.0], dtype=torch.float64) * delta_t
    t2 = t + 1.5 * delta_t
    tq = t2[:, None] + torch.tensor([0.0, 0.5, 2.5], dtype=torch.float64)[None] * delta_t
    X = 0.5 * torch.randn(n, d, generator=g)
    M = (torch.rand(n, d, generator=g) < 0.3).float()
    m._ensure_flat(full=True)
    P = m._flat.detach().clone()
    dims = m._get_dims()
    L = _lib.lib()
    tb = ctypes.c_size_t(0)
    _lib.check(L.njode_online_tables_bytes(ctypes.byref(dims), ctypes.byref(tb)))
    tb = int(tb.value)
    results = []
    for phase in (0, 1):
        ar = guarded.Arena('cuda', phase=phase)
        ar.add('P', 4 * P.numel(), 'nan32').add('tables', tb, 'nan32')
        ar.add('h', 4 * S * H, 'nan32').add('last_X', 4 * S * d, 'nan32')
        ar.add('tau', 4 * S, 'nan32').add('now', 8 * S, 'nan64').add('ids', 4 * n, 'index', modulo=S)
        ar.add('t', 8 * n, 'nan64').add('t2', 8 * n, 'nan64').add('tq', 8 * n * Q, 'nan64')
        ar.add('X', 4 * n * d, 'nan32').add('M', 4 * n * d, 'nan32').add('X0', 4 * n * d, 'nan32')
        ar.add('Yb', 4 * n * DO).add('Y', 4 * n * DO).add('Yq', 4 * n * Q * DO)
        ar.add('status', 4 * n).add('status_a', 4 * n).add('status_q', 4 * n)
        ar.build()
        for key, v in (('P', P), ('h', h0), ('last_X', x0), ('tau', tau0), ('now', now0), ('ids', ids), ('t', t),
                       ('t2', t2), ('tq', tq), ('X', X), ('M', M), ('X0', X)):
            ar.put(key, v.cuda())
        state = _lib.NjodeOnlineState(ar.ptr('h'), ar.ptr('last_X'), ar.ptr('tau'), ar.ptr('now'), S)
        stream = _lib.stream_arg(torch.device('cuda'))
        head = (ctypes.byref(dims), ar.ptr('P'), ar.ptr('tables'), tb)
        _lib.check(L.njode_online_tables_f32(ctypes.byref(dims), ar.ptr('P'), ar.ptr('tables'), tb, stream))
        _lib.check(L.njode_online_gen_observe_f32(*head, ctypes.byref(state), ar.ptr('ids'), n, ar.ptr('t'), ar.ptr('X'),
                                                  ar.ptr('M') if masked else None, delta_t, 8, spt, ar.ptr('Yb'),
                                                  ar.ptr('Y'), ar.ptr('status'), stream))
        _lib.check(L.njode_online_gen_advance_f32(*head, ctypes.byref(state), ar.ptr('ids'), n, ar.ptr('t2'), delta_t, 8,
                                                  spt, ar.ptr('status_a'), stream))
        _lib.check(L.njode_online_gen_predict_f32(*head, ctypes.byref(state), ar.ptr('ids'), n, ar.ptr('tq'), Q, delta_t,
                                                  8, spt, ar.ptr('Yq'), ar.ptr('status_q'), stream))
        assert ar.check() == []
        for key in ('status', 'status_a', 'status_q'):
            assert ar.view(key, torch.int32).tolist() == [0] * n, key
        out = {k: ar.view(k).clone() for k in ('h', 'last_X', 'tau', 'now', 'Yb', 'Y', 'Yq')}
        assert all(torch.isfinite(ar.view(k, torch.float32)).all() for k in ('h', 'last_X', 'tau', 'Yb', 'Y', 'Yq'))
        # reset last: it overwrites the listed series
        _lib.check(L.njode_online_gen_reset_f32(*head, ctypes.byref(state), ar.ptr('ids'), n, ar.ptr('X0'), spt, stream))
        assert ar.check() == []
        out['h_reset'] = ar.view('h').clone()
        assert torch.equal(ar.view('last_X', torch.float32).view(S, d)[ids.long()].cpu(), X)
        assert ar.view('now', torch.float64)[ids.long()].abs().max().item() == 0.0
        results.append(out)
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k


# ---- 8. parameters and interchange ------------------------------------------------------------------------
def _one_observe(m, start, t, X, M, delta_t):
    st = ogu.online(m, start.shape[0], delta_t)
    st.reset(start)
    yb, y = st.observe(t, X, M)
    yq = st.predict(t[:, None] + 2.5 * delta_t)
    st.check()
    return [yb, y, yq] + bits(st)


@pytest.mark.parametrize('name', ['w80', 'gru_masked'])
def test_results_follow_the_parameters(name):
    """After load_state_dict of other weights, and after an in-place p.add_, the next call's bits are
    those of a fresh state on the new weights (the fragment tables are packed again)."""
    cfg = ogu.SHAPES[name]
    sd_a, sd_b = online_util.params_of(cfg, seed=1), online_util.params_of(cfg, seed=2)
    m = hip_util.hip_model(cfg, sd_a).eval()
    d, delta_t, N = cfg['input_size'], 0.37 * DT, 3
    g = torch.Generator().manual_seed(4)
    start = 0.2 * torch.randn(N, d, generator=g)
    X = 0.5 * torch.randn(N, d, generator=g)
    M = (torch.rand(N, d, generator=g) < 0.3).float() if ogu.is_masked(cfg) else None
    t = np.asarray([1.5, 0.0, 3.2]) * delta_t
    st = ogu.online(m, N, delta_t)

    def through_st():
        st.reset(start)
        yb, y = st.observe(t, X, M)
        yq = st.predict(t[:, None] + 2.5 * delta_t)
        st.check()
        return [yb, y, yq] + bits(st)

    out_a = through_st()
    m.load_state_dict(sd_b)
    out_b = through_st()
    assert not eq_bits(out_a[1], out_b[1])
    assert same_bits(out_b, _one_observe(hip_util.hip_model(cfg, sd_b).eval(), start, t, X, M, delta_t))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.01)
    out_c = through_st()
    assert not eq_bits(out_b[1], out_c[1])
    sd_c = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert same_bits(out_c, _one_observe(hip_util.hip_model(cfg, sd_c).eval(), start, t, X, M, delta_t))


@pytest.mark.parametrize('i', [online_util.DEMO, online_util.PHYSIO])
def test_a_wave_state_continues_on_the_generic_family(model_of, i):
    name = 'cfg{}'.format(i)
    cfg, sd, m = model_of(name)
    d, delta_t, N = cfg['input_size'], 0.37 * DT, 3
    masked = ogu.is_masked(cfg)
    g = torch.Generator().manual_seed(17)
    start = 0.2 * torch.randn(N, d, generator=g)
    t_obs = np.asarray([[0.0, 2.2, 5.1, 8.3], [1.3, 1.3, 4.4, 6.0], [0.6, 4.9, 4.9, 11.2]]) * delta_t
    X = 0.5 * torch.randn(4, N, d, generator=g)
    M = (torch.rand(4, N, d, generator=g) < 0.3).float() if masked else None
    wave = m.online(N, delta_t)
    assert wave.kernels == 'wave'
    wave.reset(start)
    for j in range(2):
        wave.observe(t_obs[:, j], X[j], None if M is None else M[j])
    wave.check()
    st = ogu.online(m, N, delta_t)
    st.load_state_dict(wave.state_dict())
    outs = []
    for j in (2, 3):
        yb, y = st.observe(t_obs[:, j], X[j], None if M is None else M[j])
        outs.append((yb.cpu().numpy(), y.cpu().numpy(), st.h.cpu().numpy()))
    st.check()
    w = Worst()
    for s in range(N):
        ev = [(t_obs[s, j], X[j, s], None if M is None else M[j, s]) for j in range(4)]
        o32, o64, rows = truth(cfg, sd, ev, start[s], delta_t)
        for j, r in zip((0, 1), rows[2:]):
            w.add('Y_before', outs[j][0][s], o32['path_y'][r - 1, 0], o64['path_y'][r - 1, 0])
            w.add('Y', outs[j][1][s], o32['path_y'][r, 0], o64['path_y'][r, 0])
            w.add('h', outs[j][2][s], o32['path_h'][r, 0], o64['path_h'][r, 0])
    w.check('wave -> generic cfg{}'.format(i))
