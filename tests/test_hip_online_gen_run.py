"""A run of events per series in one launch on the shape-generic matrix-core kernels
(``observe_many`` with ``kernels='generic'``, ``njode_online_gen_run_f32``) on the GPU.

The contract is the wave family's (``tests/test_hip_online_run.py``): the bits of the same events
fed one call at a time, whatever the tile size, a series' column and its neighbours' events; against
float64 the yardstick of the single calls, ``online_util.Worst``.
"""
import numpy as np
import pytest
import torch

import online_gen_util as ogu
import online_run_util as oru
import online_util
from online_gen_util import bits, eq_bits, same_bits
from online_util import Worst, truth

pytestmark = pytest.mark.gpu

DT = 2.0 ** -10
PAIR = ['w80', 'gru_masked']      # one unmasked and one masked shape


@pytest.fixture(scope='module')
def model_of():
    """name -> (cfg, sd, model), built once per shape and never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ogu.make_model(name, seed=sorted(ogu.SHAPES).index(name))
        return cache[name]
    return get


def shape_of(cfg):
    return cfg['input_size'], cfg['hidden_size'], cfg['output_size'], ogu.is_masked(cfg)


# ---- 1. the bits of the single calls --------------------------------------------------------------------
# the masked GRU shape, d_out != d, nn_desc = None at width 100, the 400-wide climate shape; a lone
# series, one ragged tile of 16, 19 series under the library's rule, in tiles of 16 and of 4
CASES = [(name, N, spt) for name in ('gru_masked', 'out5', 'none_h100', 'climate_w400_h50')
         for N, spt in ((1, None), (5, 16), (19, None), (19, 16), (19, 4))]


@pytest.mark.parametrize('name,N,spt', CASES)
def test_bits_of_the_single_calls(model_of, name, N, spt):
    cfg, sd, m = model_of(name)
    b, delta_t, T = ogu.make_batch(cfg, N, seed=3)
    X, M = b['X'], b.get('M')
    lists = oru.event_lists(b, N, delta_t)
    one, many = ogu.online(m, N, delta_t, spt), ogu.online(m, N, delta_t, spt)
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


# ---- 2. against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', PAIR)
def test_against_float64(model_of, name):
    cfg, sd, m = model_of(name)
    N = 5
    b, delta_t, T = ogu.make_batch(cfg, N, seed=5)
    X, M = b['X'], b.get('M')
    lists = oru.event_lists(b, N, delta_t)
    st = ogu.online(m, N, delta_t, 16)
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
        for (t, k, _), r in zip(lists[s], rows):
            before = r - 1 if k else r
            w.add('Y_before', yb[e], o32['path_y'][before, 0], o64['path_y'][before, 0])
            w.add('Y', y[e], o32['path_y'][r, 0], o64['path_y'][r, 0])
            e += 1
        if lists[s]:
            r = rows[len(lists[s]) - 1]
            w.add('h', h[s], o32['path_h'][r, 0], o64['path_h'][r, 0])
        w.add('hT', hT[s], o32['hT'][0], o64['hT'][0])
    assert e == len(y)
    w.check('run {}'.format(name))


# ---- 4. the bound, 5. bad rows, stated sizes ------------------------------------------------------------
@pytest.mark.parametrize('name', PAIR)
def test_bound(model_of, name):
    cfg, sd, m = model_of(name)
    delta_t = 0.37 * DT
    oru.check_bound(lambda N: ogu.online(m, N, delta_t, 16), shape_of(cfg), delta_t)


@pytest.mark.parametrize('name', PAIR)
def test_bad_rows(model_of, name):
    """Five rows in tiles of 4: the bad rows sit beside good ones in a tile, and one is alone in the
    ragged tile."""
    cfg, sd, m = model_of(name)
    oru.check_bad_rows(m, shape_of(cfg), lambda N: ogu.online(m, N, 0.37 * DT, 16), generic=True, spt=4)


@pytest.mark.parametrize('name', PAIR)
def test_stated_sizes(model_of, name):
    cfg, sd, m = model_of(name)
    oru.check_stated_sizes(m, shape_of(cfg), generic=True, spt=4)


# ---- tile independence, and the same bits from the same call ----------------------------------------------
@pytest.mark.parametrize('name', ['w80', 'gru_masked', 'w160'])
def test_bits_do_not_depend_on_the_tile(model_of, name):
    """A series alone in a tile of 1, alone in a tile of 16, in column 5 of a tile beside 8 series
    whose ranges are longer, shorter, empty and of other kinds, and in tiles of 4: the same bits.  The
    same call on a clone of the state: the same bits."""
    cfg, sd, m = model_of(name)
    d, delta_t, S = cfg['input_size'], 0.37 * DT, 9
    masked = ogu.is_masked(cfg)
    g = torch.Generator().manual_seed(21)
    start = 0.2 * torch.randn(S, d, generator=g)
    n_max = 6
    X = 0.5 * torch.randn(S * n_max, d, generator=g)
    M = (torch.rand(S * n_max, d, generator=g) < 0.4).float() if masked else None
    k = 5
    length = [6, 1, 0, 2, 5, 3, 4, 6, 2]                   # series k: 3 events, longer and shorter beside it
    kinds = [[1, 0, 1, 1, 0, 1], [0], [], [0, 0], [1, 1, 1, 1, 1], [1, 0, 1], [0, 1, 0, 1], [0] * 6, [1, 1]]
    gaps = np.asarray([0.0, 2.3, 0.7, 1.0, 4.4, 0.0])     # in units of delta_t, off the grid
    lists = []
    for s in range(S):
        ts = np.cumsum(np.roll(gaps, s)[:length[s]]) * delta_t
        lists.append([(float(t), kinds[s][j], s * n_max + j) for j, t in enumerate(ts)])
    assert [len(ev) for ev in lists] == length and [kk for _, kk, _ in lists[k]] == [1, 0, 1]
    outs = []
    for spt, ids in ((1, [k]), (16, [k]), (16, [3, 8, 0, 6, 1, k, 2, 7, 4]), (4, list(range(S)))):
        st = ogu.online(m, S, delta_t, spt)
        st.reset(start)
        clone = ogu.online(m, S, delta_t, spt)
        clone.load_state_dict(st.state_dict())
        sub = [lists[s] for s in ids]
        yb, y = oru.run(st, sub, ids, X, M)
        yb2, y2 = oru.run(clone, sub, ids, X, M)
        st.check()
        clone.check()
        assert eq_bits(yb, yb2) and eq_bits(y, y2) and same_bits(bits(st), bits(clone))
        assert st.n_done.cpu().tolist() == [len(ev) for ev in sub]
        lo = sum(len(ev) for ev in sub[:ids.index(k)])
        outs.append([yb[lo:lo + 3], y[lo:lo + 3]] + [x[k] for x in bits(st)])
    for other in outs[1:]:
        assert same_bits(outs[0], other)
    assert torch.isfinite(outs[0][1]).all()


# ---- interchange --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', [online_util.DEMO, online_util.PHYSIO])
def test_a_wave_run_continues_on_the_generic_family(model_of, i):
    """Not bit equality: the families differ in summation order."""
    name = 'cfg{}'.format(i)
    cfg, sd, m = model_of(name)
    d, delta_t, N = cfg['input_size'], 0.37 * DT, 3
    masked = ogu.is_masked(cfg)
    g = torch.Generator().manual_seed(17)
    start = 0.2 * torch.randn(N, d, generator=g)
    t_obs = np.asarray([[0.0, 2.2, 5.1, 8.3], [1.3, 1.3, 4.4, 6.0], [0.6, 4.9, 4.9, 11.2]]) * delta_t
    kinds = [[1, 0, 1, 1], [1, 1, 0, 1], [0, 1, 1, 0]]
    X = 0.5 * torch.randn(4 * N, d, generator=g)
    M = (torch.rand(4 * N, d, generator=g) < 0.3).float() if masked else None
    lists = [[(float(t_obs[s, j]), kinds[s][j], 4 * s + j) for j in range(4)] for s in range(N)]
    wave = m.online(N, delta_t)
    assert wave.kernels == 'wave'
    wave.reset(start)
    oru.run(wave, [ev[:2] for ev in lists], None, X, M)
    wave.check()
    st = ogu.online(m, N, delta_t)
    st.load_state_dict(wave.state_dict())
    yb, y = oru.run(st, [ev[2:] for ev in lists], None, X, M)
    st.check()
    yb, y, h = yb.cpu().numpy(), y.cpu().numpy(), st.h.cpu().numpy()
    w = Worst()
    for s in range(N):
        o32, o64, rows = truth(cfg, sd, oru.truth_events(lists[s], X, M), start[s], delta_t)
        for j in (2, 3):
            r, e = rows[j], 2 * s + j - 2
            before = r - 1 if kinds[s][j] else r
            w.add('Y_before', yb[e], o32['path_y'][before, 0], o64['path_y'][before, 0])
            w.add('Y', y[e], o32['path_y'][r, 0], o64['path_y'][r, 0])
        w.add('h', h[s], o32['path_h'][rows[3], 0], o64['path_h'][rows[3], 0])
    w.check('wave run -> generic run cfg{}'.format(i))


# ---- the fused replay -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', PAIR)
def test_fused_replay(model_of, name):
    cfg, sd, m = model_of(name)
    N = 19
    b, delta_t, T = ogu.make_batch(cfg, N, seed=4)
    loop, fused = ogu.online(m, N, delta_t, 4), ogu.online(m, N, delta_t, 4)
    loop.reset(b['start_X'])
    fused.reset(b['start_X'])
    yb1, y1 = loop.replay(b['times'], b['time_ptr'], b['X'], b['obs_idx'], b.get('M'))
    yb2, y2 = fused.replay(b['times'], b['time_ptr'], b['X'], b['obs_idx'], b.get('M'), fused=True)
    loop.check()
    fused.check()
    assert same_bits(bits(loop), bits(fused)) and eq_bits(yb1, yb2) and eq_bits(y1, y2)
