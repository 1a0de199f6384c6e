"""A run of events per series in one launch on the wave family (``observe_many``,
``njode_online_run_f32``) on the GPU.

The contract is that of the header: the result of a run on a series -- the state after it and every
output row -- is, in bits, the result of the same events fed one call at a time
(``online_run_util.single_calls``).  Against float64 the yardstick is the one of the single calls,
``online_util.Worst``: err(online, f64) <= max(2 err(oracle fp32, f64), 2e-6).
"""
import numpy as np
import pytest
import torch

import hip_util
import online_run_util as oru
import online_util
from njode_amd import schedule, synthetic_physionet
from njode_amd.build import CONFIGS
from online_gen_util import bits, eq_bits, same_bits
from online_util import Worst, model_cfg, params_of, truth

pytestmark = pytest.mark.gpu

DT = 2.0 ** -10
BOTH = [online_util.DEMO, online_util.PHYSIO]


@pytest.fixture(scope='module')
def model_of():
    """config number -> (cfg, sd, model), built once and never modified."""
    cache = {}

    def get(i):
        if i not in cache:
            cfg = model_cfg(CONFIGS[i])
            sd = params_of(cfg, seed=i)
            cache[i] = (cfg, sd, hip_util.hip_model(cfg, sd).eval())
        return cache[i]
    return get


def shape_of(c):
    """(d, H, d_out, masked) of a row of the build table."""
    return c[0], c[1], c[2], bool(c[6])


def make_batch(c, N, seed=0):
    """tests/test_hip_online.py::make_batch's shapes: 12 - 40 grid steps, 3 - 6 observations per series."""
    if c[6]:
        b = synthetic_physionet.make_batch(batch_size=N, dim=c[0], n_grid=40, n_obs_range=(3, 6), seed=seed)
        b['start_X'] = 0.1 * torch.randn(N, c[0], generator=torch.Generator().manual_seed(seed))
        return b, b['delta_t'], b['T']
    return hip_util.exact_k_batch(N, 12, obs_per_path=3, seed=seed, d=c[0])


# ---- 1. the bits of the single calls --------------------------------------------------------------------
CASES = [(i, 5) for i in online_util.ACCEPTED] + [(i, N) for i in BOTH for N in (1, 9)]


@pytest.mark.parametrize('i,N', CASES)
def test_bits_of_the_single_calls(model_of, i, N):
    c = CONFIGS[i]
    cfg, sd, m = model_of(i)
    b, delta_t, T = make_batch(c, N, seed=i)
    X, M = b['X'], b.get('M')
    lists = oru.event_lists(b, N, delta_t)
    if N >= 5:      # no event, one event, empty slices only, both kinds: all in the one call
        assert [len(lists[1]), len(lists[2])] == [0, 1] and {k for _, k, _ in lists[3]} == {0}
        assert {k for _, k, _ in lists[0]} == {0, 1} and {k for _, k, _ in lists[4]} == {1}
    one, many = m.online(N, delta_t), m.online(N, delta_t)
    one.reset(b['start_X'])
    many.reset(b['start_X'])
    yb1, y1, status, done = oru.single_calls(one, lists, list(range(N)), X, M)
    yb, y = oru.run(many, lists, None, X, M)
    assert many.status.cpu().tolist() == [0] * N == status
    assert many.n_done.cpu().tolist() == [len(ev) for ev in lists] == done
    assert same_bits(bits(one), bits(many))
    assert eq_bits(yb, yb1) and eq_bits(y, y1)
    assert torch.isfinite(y).all() and torch.isfinite(yb).all()
    kind = torch.as_tensor([k for ev in lists for _, k, _ in ev], device='cuda')
    assert eq_bits(yb[kind == 0], y[kind == 0])
    one.advance(np.full(N, T))
    many.advance(np.full(N, T))
    one.check()
    many.check()
    assert same_bits(bits(one), bits(many))
    last = [[t for t, k, _ in ev if k] for ev in lists]
    assert np.array_equal(many.tau.cpu().numpy(), np.asarray([(x or [0.0])[-1] for x in last], dtype=np.float32))


@pytest.mark.parametrize('i', BOTH)
def test_the_same_call_gives_the_same_bits(model_of, i):
    c = CONFIGS[i]
    cfg, sd, m = model_of(i)
    N = 5
    b, delta_t, T = make_batch(c, N, seed=2)
    lists = oru.event_lists(b, N, delta_t)
    a = m.online(N, delta_t)
    a.reset(b['start_X'])
    a.observe(np.full(N, 0.5 * delta_t), torch.zeros(N, c[0]), torch.ones(N, c[0]) if c[6] else None)
    clone = m.online(N, delta_t)
    clone.load_state_dict(a.state_dict())
    out_a = oru.run(a, lists, None, b['X'], b.get('M'))
    out_b = oru.run(clone, lists, None, b['X'], b.get('M'))
    a.check()
    clone.check()
    assert same_bits(bits(a), bits(clone)) and eq_bits(out_a[0], out_b[0]) and eq_bits(out_a[1], out_b[1])
    # a subset of the series, out of order: the rows and the states of the full call
    sub = m.online(N, delta_t)
    sub.reset(b['start_X'])
    sub.observe(np.full(N, 0.5 * delta_t), torch.zeros(N, c[0]), torch.ones(N, c[0]) if c[6] else None)
    keep = bits(sub)
    ids = [4, 0, 3]
    yb, y = oru.run(sub, [lists[s] for s in ids], ids, b['X'], b.get('M'))
    sub.check()
    offs = np.concatenate([[0], np.cumsum([len(ev) for ev in lists])])
    rows = torch.as_tensor(np.concatenate([np.arange(offs[s], offs[s + 1]) for s in ids]), device='cuda')
    assert eq_bits(y, out_a[1][rows]) and eq_bits(yb, out_a[0][rows])
    for x0, x1, xa in zip(keep, bits(sub), bits(a)):
        assert eq_bits(x1[ids], xa[ids]) and eq_bits(x1[[1, 2]], x0[[1, 2]])


# ---- 2. against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize('i', BOTH)
def test_against_float64(model_of, i):
    c = CONFIGS[i]
    cfg, sd, m = model_of(i)
    N = 5
    b, delta_t, T = make_batch(c, N, seed=i)
    X, M = b['X'], b.get('M')
    lists = oru.event_lists(b, N, delta_t)
    st = m.online(N, delta_t)
    st.reset(b['start_X'])
    yb, y = oru.run(st, lists, None, X, M)
    h = st.h.cpu().numpy()
    st.advance(np.full(N, T))
    st.check()
    hT = st.h.cpu().numpy()
    yb, y = yb.cpu().numpy(), y.cpu().numpy()
    w, e = Worst(), 0
    for s in range(N):
        o32, o64, rows = truth(cfg, sd, oru.truth_events(lists[s], X, M), b['start_X'][s], delta_t, T)
        assert len(rows) >= len(lists[s])
        for (t, k, _), r in zip(lists[s], rows):
            before = r - 1 if k else r      # an empty slice: the readout of the state it arrives at, twice
            w.add('Y_before', yb[e], o32['path_y'][before, 0], o64['path_y'][before, 0])
            w.add('Y', y[e], o32['path_y'][r, 0], o64['path_y'][r, 0])
            e += 1
        if lists[s]:
            r = rows[len(lists[s]) - 1]
            w.add('h', h[s], o32['path_h'][r, 0], o64['path_h'][r, 0])
        w.add('hT', hT[s], o32['hT'][0], o64['hT'][0])
    assert e == len(y)
    w.check('run cfg{}'.format(i))


# ---- 3. the clock -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', BOTH)
def test_clock(model_of, i):
    """The four series of the clock matrix as four ranges of one call, the second call of each an
    empty slice."""
    c = CONFIGS[i]
    cfg, sd, m = model_of(i)
    d, delta_t = c[0], 0.37 * DT
    times = oru.CLOCK_TIMES * delta_t
    N, n_calls = times.shape
    g = torch.Generator().manual_seed(7)
    start = 0.2 * torch.randn(N, d, generator=g)
    X = 0.5 * torch.randn(N * n_calls, d, generator=g)
    M = (torch.rand(N * n_calls, d, generator=g) < 0.3).float() if c[6] else None
    lists = [[(float(times[s, j]), 0 if j == 1 else 1, s * n_calls + j) for j in range(n_calls)] for s in range(N)]
    st = m.online(N, delta_t)
    st.reset(start)
    yb, y = oru.run(st, lists, None, X, M)
    st.check()
    assert st.n_done.cpu().tolist() == [n_calls] * N
    w = Worst()
    for s in range(N):
        assert float(st.now[s]) == oru.clock_after(times[s], delta_t)
        assert float(st.tau[s]) == float(np.float32(times[s, -1]))
        o32, o64, rows = truth(cfg, sd, oru.truth_events(lists[s], X, M), start[s], delta_t)
        for j, r in enumerate(rows):
            w.add('Y', y[s * n_calls + j].cpu().numpy(), o32['path_y'][r, 0], o64['path_y'][r, 0])
        w.add('h', st.h[s].cpu().numpy(), o32['path_h'][rows[-1], 0], o64['path_h'][rows[-1], 0])
    w.check('run clock cfg{}'.format(i))
    # tau is the time of the last OBSERVATION: a range that ends in empty slices keeps the earlier one
    st.reset(start)
    lists2 = [[(t, k if j < 3 else 0, r) for j, (t, k, r) in enumerate(ev)] for ev in lists]
    oru.run(st, lists2, None, X, M)
    st.check()
    for s in range(N):
        assert float(st.tau[s]) == float(np.float32(times[s, 2])) and float(st.now[s]) == oru.clock_after(times[s], delta_t)


# ---- 4. the bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', BOTH)
def test_bound(model_of, i):
    m = model_of(i)[2]
    delta_t = 0.37 * DT
    oru.check_bound(lambda N: m.online(N, delta_t), shape_of(CONFIGS[i]), delta_t)


# ---- 5. bad rows, 6. stated sizes -------------------------------------------------------------------------
@pytest.mark.parametrize('i', BOTH)
def test_bad_rows(model_of, i):
    m = model_of(i)[2]
    oru.check_bad_rows(m, shape_of(CONFIGS[i]), lambda N: m.online(N, 0.37 * DT))


@pytest.mark.parametrize('i', BOTH)
def test_stated_sizes(model_of, i):
    oru.check_stated_sizes(model_of(i)[2], shape_of(CONFIGS[i]))


def test_bad_range_is_named_by_check(model_of):
    """Status 3 through the Python layer: only a caller who goes around observe_many's checks gets
    there, so the status tensor is set by hand."""
    m = model_of(online_util.DEMO)[2]
    st = m.online(4, 0.01)
    st._pending.append((np.asarray([2, 0, 3]), torch.tensor([0, 3, 3], dtype=torch.int32, device='cuda')))
    with pytest.raises(RuntimeError, match=r'\[0, 3\].*range'):
        st.check()


# ---- 7. the fused replay ------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', BOTH)
def test_fused_replay(model_of, i):
    c = CONFIGS[i]
    cfg, sd, m = model_of(i)
    N = 9
    b, delta_t, T = make_batch(c, N, seed=4)
    loop, fused = m.online(N, delta_t), m.online(N, delta_t)
    loop.reset(b['start_X'])
    fused.reset(b['start_X'])
    yb1, y1 = loop.replay(b['times'], b['time_ptr'], b['X'], b['obs_idx'], b.get('M'))
    yb2, y2 = fused.replay(b['times'], b['time_ptr'], b['X'], b['obs_idx'], b.get('M'), fused=True)
    loop.check()
    fused.check()
    assert same_bits(bits(loop), bits(fused)) and eq_bits(yb1, yb2) and eq_bits(y1, y2)
    assert int(fused.n_done.sum()) == len(b['obs_idx'])


def test_fused_replay_agrees_with_batch_route():
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
    _, y = st.replay(b['times'], b['time_ptr'], b['X'], b['obs_idx'], fused=True)
    ptr = np.asarray(b['time_ptr'])
    for i in range(len(b['times'])):
        for r in range(int(ptr[i]), int(ptr[i + 1])):
            s = int(b['obs_idx'][r])
            np.testing.assert_allclose(y[r].cpu().numpy(), path_y[rows_b[i], s].cpu().numpy(), atol=hip_util.ATOL,
                                       rtol=hip_util.RTOL)
    st.advance(np.full(7, T))
    st.check()
    np.testing.assert_allclose(st.h.cpu().numpy(), hT.cpu().numpy(), atol=hip_util.ATOL, rtol=hip_util.RTOL)
