"""The dropout keep-bit stream of the matrix-core kernels ("nothing tests
the per-unit keep rate or cross-unit independence of that stream").  oracle/dropout_oracle.py
restates the device code in numpy; here its statistics are tested on CPU, and (-m gpu) the
device's words are compared with the restatement bit for bit."""
import numpy as np
import pytest
import torch

from oracle import dropout_oracle as do

NET_ODE, NET_ENC = 0, 1
W, P = 50, 0.1


def _keep(n_paths, steps, net=NET_ODE, layer=0, seed=0x1234567890ABCDEF):
    gid = np.arange(n_paths, dtype=np.uint64)[:, None]
    tkey = np.arange(steps, dtype=np.uint64)[None, :]
    return do.keep_units(seed, np.broadcast_to(gid, (n_paths, steps)),
                         np.broadcast_to(tkey, (n_paths, steps)), net, W, P, layer)


def test_keep_rate_per_unit():
    k = _keep(4000, 100).reshape(-1, W).astype(np.float64)      # 400 000 draws per unit
    n = k.shape[0]
    rate = k.mean(axis=0)
    p_keep = 1.0 - int(P * 65536 + 0.5) / 65536.0
    se = np.sqrt(p_keep * (1 - p_keep) / n)
    assert np.all(np.abs(rate - p_keep) < 4.5 * se), (rate.min(), rate.max(), p_keep, se)
    assert abs(rate.mean() - p_keep) < 4.5 * se / np.sqrt(W)


def test_units_are_pairwise_uncorrelated():
    k = _keep(2000, 100).reshape(-1, W).astype(np.float64)
    n = k.shape[0]
    c = np.corrcoef(k.T)
    off = c[~np.eye(W, dtype=bool)]
    # 2 450 pairs, null s.d. 1 / sqrt(n): the largest |rho| of that many should stay below ~4.7 sd
    assert np.max(np.abs(off)) < 5.0 / np.sqrt(n), np.max(np.abs(off)) * np.sqrt(n)
    # joint drops of neighbouring units (same random word: low / high half) at the product rate
    both = ((1 - k[:, 0::2][:, :24]) * (1 - k[:, 1::2][:, :24])).mean()
    pd = int(P * 65536 + 0.5) / 65536.0
    assert abs(both - pd * pd) < 5.0 * np.sqrt(pd * pd * (1 - pd * pd) / (n * 24))


def test_independent_across_steps_paths_layers_networks():
    a = _keep(3000, 64).astype(np.float64)                         # [paths, steps, W]
    n = a.shape[0] * (a.shape[1] - 1) * W
    def corr(x, y):
        x, y = x.reshape(-1), y.reshape(-1)
        return float(np.corrcoef(x, y)[0, 1])
    tol = 5.0 / np.sqrt(n)
    assert abs(corr(a[:, :-1], a[:, 1:])) < tol                    # consecutive Euler steps
    assert abs(corr(a[:-1, :-1], a[1:, :-1])) < tol                # neighbouring paths
    b = _keep(3000, 64, layer=1).astype(np.float64)
    assert abs(corr(a, b)) < 5.0 / np.sqrt(a.size)                 # the two hidden layers
    e = _keep(3000, 64, net=NET_ENC).astype(np.float64)
    assert abs(corr(a, e)) < 5.0 / np.sqrt(a.size)                 # two networks, same key
    s2 = _keep(3000, 64, seed=0x1234567890ABCDF0).astype(np.float64)
    assert abs(corr(a, s2)) < 5.0 / np.sqrt(a.size)                # neighbouring seeds


def test_stream_does_not_depend_on_the_batch_a_path_is_in():
    """keyed by the GLOBAL path id: a path's masks are the same whatever shard holds it"""
    full = _keep(64, 10)
    gid = np.arange(40, 64, dtype=np.uint64)[:, None]
    tkey = np.arange(10, dtype=np.uint64)[None, :]
    part = do.keep_units(0x1234567890ABCDEF, np.broadcast_to(gid, (24, 10)),
                         np.broadcast_to(tkey, (24, 10)), NET_ODE, W, P)
    assert np.array_equal(full[40:], part)


# ---- the VALU and shape-generic streams (njode_kernels.h Masks::draw, njode_gen.h drop_word) ----------
def _keep_of(stream, n_paths, steps, net=NET_ODE, layer=0, width=W, p=P, seed=0x1234567890ABCDEF):
    gid = np.broadcast_to(np.arange(n_paths, dtype=np.uint64)[:, None], (n_paths, steps))
    tkey = np.broadcast_to(np.arange(steps, dtype=np.uint64)[None, :], (n_paths, steps))
    return do.keep_mask(stream, seed, gid, tkey, net, layer, width, p)


@pytest.mark.parametrize('stream', ['valu', 'gen'])
def test_other_streams_keep_rate_and_independence(stream):
    width = 51                                                    # (odd: the last pair is half used)
    a = _keep_of(stream, 2000, 100, width=width).astype(np.float64)   # [paths, steps, W]
    k = a.reshape(-1, width)
    n = k.shape[0]
    p_keep = 1.0 - do.thr16(P) / 65536.0
    se = np.sqrt(p_keep * (1 - p_keep) / n)
    rate = k.mean(axis=0)
    assert np.all(np.abs(rate - p_keep) < 4.5 * se), (rate.min(), rate.max(), p_keep, se)
    c = np.corrcoef(k.T)
    assert np.max(np.abs(c[~np.eye(width, dtype=bool)])) < 5.0 / np.sqrt(n)

    def corr(x, y):
        return float(np.corrcoef(x.reshape(-1), y.reshape(-1))[0, 1])
    tol = 5.0 / np.sqrt(a.size)
    assert abs(corr(a[:, :-1], a[:, 1:])) < tol                    # consecutive Euler steps
    assert abs(corr(a[:-1], a[1:])) < tol                          # neighbouring paths
    for other in (dict(layer=1), dict(net=do.NET_ENC), dict(net=do.NET_DEC_BJ), dict(net=do.NET_DEC),
                  dict(seed=0x1234567890ABCDF0)):
        b = _keep_of(stream, 2000, 100, width=width, **other).astype(np.float64)
        assert abs(corr(a, b)) < tol, (stream, other)              # layers, networks, seeds
        assert not np.array_equal(a[:20], b[:20]), (stream, other)


def test_generic_stream_draws_every_layer_of_a_deep_net():
    layers = [_keep_of('gen', 400, 20, layer=l, width=33).astype(np.float64) for l in range(8)]
    for i in range(8):
        for j in range(i):
            c = float(np.corrcoef(layers[i].reshape(-1), layers[j].reshape(-1))[0, 1])
            assert abs(c) < 5.0 / np.sqrt(layers[i].size), (i, j, c)


def test_streams_are_keyed_by_the_64_bit_global_path_id():
    for stream in do.STREAMS:
        lo = do.keep_mask(stream, 5, np.arange(8, dtype=np.uint64), 3, NET_ODE, 0, W, 0.5)
        hi = do.keep_mask(stream, 5, np.arange(8, dtype=np.uint64) + np.uint64(2 ** 32), 3, NET_ODE, 0, W, 0.5)
        assert not np.array_equal(lo, hi), stream
        # the seed's high word moves the stream too
        s2 = do.keep_mask(stream, 5 + 2 ** 32, np.arange(8, dtype=np.uint64), 3, NET_ODE, 0, W, 0.5)
        assert not np.array_equal(lo, s2), stream


def test_valu_stream_continues_the_state_into_layer_two():
    """Masks::draw: layer 2's words follow layer 1's on the same xorshift32 state"""
    st = do.path_state(77, np.uint64(9), 4, NET_ODE)
    words = do.xorshift32_words(st, 25).astype(np.uint64)          # ceil(49 / 2) = 25 words for two layers
    thr = do.thr16(0.3)
    ref = np.array([((words[u >> 1] >> np.uint64(16 * (u & 1))) & np.uint64(0xFFFF)) >= thr for u in range(49)])
    got = np.concatenate([do.valu_keep(77, np.uint64(9), 4, NET_ODE, 24, 0.3, 0)[:24],
                          do.valu_keep(77, np.uint64(9), 4, NET_ODE, 24, 0.3, 1)])
    # (layer 1: units 0..23 = words 0..11; layer 2: words 12..23)
    assert np.array_equal(got, ref[:48].astype(np.uint8))


def test_threshold_and_scale_are_the_kernels():
    assert do.thr16(0.1) == 6554 and do.thr16(0.5) == 32768 and do.thr16(0.9) == 58982
    assert do.thr16(0.999999) == 65535                               # clamped
    assert do.thr16(5e-6) == 0                                       # p > 0, nothing dropped
    # fp32 rounding of p decides: in float64 p 65536 + 0.5 = 6553.9999999, in fp32 6554.0
    p = (6553.5 - 1e-7) / 65536.0
    assert int(p * 65536.0 + 0.5) == 6553 and do.thr16(p) == 6554
    assert do.inv_keep(0.9) == float(np.float32(1) / np.float32(1 - 58982 / 65536.0))
    assert abs(do.inv_keep(0.9) / (1 / (1 - 0.9)) - 1) > 5e-5        # not torch's 1 / (1 - p)
    assert do.inv_keep(5e-6) == 1.0


class _Ones:
    scale = 1.0

    def __call__(self, net, tkey, rows, layer, width):
        return np.ones((len(np.asarray(rows)), width), dtype=np.uint8)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('shape', ['demo', 'masked', 'rnn'])
def test_masked_oracle_with_all_ones_is_the_plain_oracle(dtype, shape):
    """The mask source with all-ones masks and unit scale: bit for bit the oracle without dropout
    (loss, hT, path_h, path_y and every gradient)"""
    import hip_util
    from njode_amd import models, synthetic_physionet
    if shape == 'masked':
        cfg = dict(hip_util.demo_cfg(d=3, H=3, masked=True))
        b = synthetic_physionet.make_batch(batch_size=5, dim=3, n_grid=12, n_obs_range=(2, 4), seed=1)
        dt, T = b['delta_t'], b['T']
    else:
        cfg = hip_util.demo_cfg()
        cfg['use_rnn'] = shape == 'rnn'
        b, meta = hip_util.bs_batch(6, seed=2, nb_steps=20, obs_perc=0.3)
        dt, T = meta['dt'], meta['maturity']
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in models.NJODE(**cfg).state_dict().items()}
    cfg = dict(cfg, dropout_rate=0.0)
    outs = []
    for masks in (None, _Ones()):
        out, g = hip_util.oracle_truth(cfg, sd, b, dt, T, dtype, masks=masks, return_path=True, until_T=True)
        outs.append((out, g))
    (o1, g1), (o2, g2) = outs
    assert torch.equal(o1[0], o2[0]) and torch.equal(o1[1], o2[1])
    assert torch.equal(o1[3], o2[3]) and torch.equal(o1[4], o2[4])
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k


def test_masked_oracle_uses_the_kernels_keys():
    """the oracle asks the mask source for every evaluation with the kernels' (net, time key, rows)"""
    import hip_util
    from njode_amd import models
    from oracle import njode_oracle as no
    cfg = hip_util.demo_cfg(dropout=0.1)
    b, meta = hip_util.bs_batch(4, seed=3, nb_steps=10, obs_perc=0.3)
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in models.NJODE(**cfg).state_dict().items()}
    seen = []

    class Spy(_Ones):
        def __call__(self, net, tkey, rows, layer, width):
            seen.append((net, tkey, tuple(int(r) for r in np.asarray(rows)), layer))
            return super().__call__(net, tkey, rows, layer, width)
    hip_util.oracle_truth(cfg, sd, b, meta['dt'], meta['maturity'], torch.float64, masks=Spy(), return_path=True)
    from njode_amd.schedule import Schedule
    s = Schedule(b['times'], meta['dt'], meta['maturity'], False)
    every = tuple(range(4))
    assert seen[0][:3] == (no.NET_ENC, no.TKEY_START, every)
    assert seen[2][:3] == (no.NET_DEC_ROW, no.TKEY_START - 1, every)
    odes = [k for k in seen if k[0] == no.NET_ODE and k[3] == 0]
    assert [k[1] for k in odes] == list(range(s.n_steps))
    rows = [k for k in seen if k[0] == no.NET_DEC_ROW and k[3] == 0][1:]
    assert [k[1] for k in rows] == [0x80000000 + k for k in range(s.n_steps)]
    for i, kj in enumerate(s.k_jump):
        lo, hi = int(b['time_ptr'][i]), int(b['time_ptr'][i + 1])
        obs = tuple(int(r) for r in b['obs_idx'][lo:hi])
        assert (no.NET_DEC_BJ, int(kj), every, 0) in seen
        assert (no.NET_ENC, int(kj), obs, 1) in seen
        assert (no.NET_DEC, int(kj), every, 1) in seen


@pytest.mark.gpu
def test_device_words_equal_the_restatement():
    import ctypes
    import torch
    from njode_amd import _lib
    L = _lib.lib()
    seed, n_words = 0x9E3779B97F4A7C15, 14
    keys = [(0, 0, 0), (1, 0, 0), (12345, 7, 0), (2 ** 33 + 5, 99, 1), (19999, 100, 0),
            (3, 0xFFFFFFFF, 1), (77, 0x80000005, 4)]
    out = torch.zeros(4 * n_words, dtype=torch.int32, device='cuda')
    for gid, tkey, net in keys:
        _lib.check(L.njode_selftest_dropout_words(
            ctypes.c_uint64(seed), ctypes.c_uint64(gid), ctypes.c_uint32(tkey), ctypes.c_uint32(net),
            n_words, ctypes.c_void_p(out.data_ptr()), None))
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32).reshape(4, n_words)
        for g in range(4):
            st = do.mfma_group_state(seed, np.uint64(gid), g, tkey, net)
            ref = do.xorshift32_words(st, n_words).astype(np.uint32)
            assert np.array_equal(got[g], ref), (gid, tkey, net, g)
