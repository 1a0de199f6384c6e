"""A run of events per series in one launch (``njode_online_run_f32``, ``njode_online_gen_run_f32``,
``OnlineState.observe_many``, ``replay(fused=True)``), the part that needs no GPU: the symbols, what
the entry points refuse before any launch, the host-side argument checks, and the by-series layout of
a collated batch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gen_envelope
import online_gen_util as ogu
import online_util
from njode_amd import _lib, models, online
from njode_amd.build import CONFIGS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('njode_online_run_f32', 'njode_online_gen_run_f32')
BAD, UNSUP, OK = _lib.E_BADARG, _lib.E_UNSUPPORTED, _lib.NJODE_OK


def dims_of(c):
    d, H, DO, nh, W, act, masked, curt, res, rnn = c
    flags = ((_lib.F_MASKED if masked else 0) | (_lib.F_INPUT_CURRENT_T if curt else 0)
             | (_lib.F_RESIDUAL if res else 0) | (_lib.F_USE_RNN if rnn else 0))
    return _lib.NjodeDims(d, H, DO, nh, W, act, flags)


def test_symbols_declared_listed_and_exported():
    header = open(os.path.join(REPO, 'include', 'njode_online.h')).read()
    declared = set(re.findall(r'\b(njode_[a-z0-9_]+)\s*\(', header))
    L = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS
        assert getattr(L, name) is not None and getattr(L, name).restype is ctypes.c_int


# ---- the C ABI: every pointer below is a value that must not be followed (no device here) ------------
def wave(L, dims, st, n=2, ev_ptr=256, n_events=3, t=256, X=256, M=None, kind=None, delta_t=0.1, max_steps=5,
         status=256, n_done=256, params=256, ids=None):
    return L.njode_online_run_f32(ctypes.byref(dims) if dims is not None else None, params, ctypes.byref(st), ids, n,
                                  ev_ptr, n_events, t, X, M, kind, delta_t, max_steps, None, None, status, n_done, None)


def gen(L, dims, st, tables=256, tb=1 << 30, spt=0, n=2, ev_ptr=256, n_events=3, t=256, X=256, M=None, kind=None,
        delta_t=0.1, max_steps=5, status=256, n_done=256, params=256, ids=None):
    return L.njode_online_gen_run_f32(ctypes.byref(dims) if dims is not None else None, params, tables, tb,
                                      ctypes.byref(st), ids, n, ev_ptr, n_events, t, X, M, kind, delta_t, max_steps, spt,
                                      None, None, status, n_done, None)


def _tables_bytes(d):
    out = ctypes.c_size_t(0)
    assert _lib.lib().njode_online_tables_bytes(ctypes.byref(d), ctypes.byref(out)) == OK
    return int(out.value)


def families():
    """(call, unmasked dims, masked dims, keywords of a good call per dims) of both families."""
    L = _lib.lib()
    du, dm = dims_of(CONFIGS[online_util.DEMO]), dims_of(CONFIGS[online_util.PHYSIO])
    gu = gen_envelope.dims_of(*ogu.raw_of_cfg(ogu.SHAPES['w80']))
    gm = gen_envelope.dims_of(*ogu.raw_of_cfg(ogu.SHAPES['climate_w400_h50']))
    return [(lambda d, st, **kw: wave(L, d, st, **kw), du, dm, {}, {}),
            (lambda d, st, **kw: gen(L, d, st, **kw), gu, gm, {'tb': _tables_bytes(gu)}, {'tb': _tables_bytes(gm)})]


@pytest.mark.parametrize('fam', [0, 1])
def test_entry_points_refuse_before_any_launch(fam):
    call, du, dm, ku, km = families()[fam]
    st = _lib.NjodeOnlineState(256, 512, 768, 1024, 4)
    why = _lib.lib().njode_last_error
    # every bad clock of test_entry_points_refuse_bad_clock_before_any_launch
    for delta_t, max_steps in ((0.0, 5), (-1.0, 5), (float('inf'), 5), (float('nan'), 5), (0.1, 0), (0.1, -3)):
        assert call(du, st, delta_t=delta_t, max_steps=max_steps, **ku) == BAD, (delta_t, max_steps)
    # null ev_ptr / n_done / status
    for name in ('ev_ptr', 'n_done', 'status'):
        assert call(du, st, **dict(ku, **{name: None})) == BAD, name
        assert name in why().decode()
    # n_events < 0; null t or X with n_events > 0
    assert call(du, st, n_events=-1, **ku) == BAD and 'n_events' in why().decode()
    assert call(du, st, t=None, **ku) == BAD
    assert call(du, st, X=None, **ku) == BAD
    # M on an unmasked model, missing on a masked one
    assert call(du, st, M=256, **ku) == BAD and 'unmasked' in why().decode()
    assert call(dm, st, **km) == BAD and 'needs M' in why().decode()
    # more rows than series without ids; a negative n; a null state array, params, dims
    assert call(du, st, n=5, **ku) == BAD
    assert call(du, st, n=-1, **ku) == BAD
    assert call(du, _lib.NjodeOnlineState(256, None, 768, 1024, 4), **ku) == BAD
    assert call(du, st, params=None, **ku) == BAD
    assert call(None, st, **ku) == BAD
    # what is legal: n = 0 launches nothing, whatever the events say
    assert call(du, st, n=0, **ku) == OK
    assert call(du, st, n=0, n_events=0, t=None, X=None, **ku) == OK
    assert call(dm, st, n=0, M=256, **km) == OK


def test_generic_entry_refuses_bad_tables_and_tile():
    call, du, _, ku, _ = families()[1]
    st = _lib.NjodeOnlineState(256, 512, 768, 1024, 4)
    why = _lib.lib().njode_last_error
    assert call(du, st, tables=None, tb=ku['tb']) == BAD and 'tables' in why().decode()
    assert call(du, st, tb=ku['tb'] - 1) == BAD and 'tables_bytes' in why().decode()
    for spt in (-1, 3, 5, 12, 32, 17):
        assert call(du, st, spt=spt, **ku) == BAD, spt
        assert 'series_per_tile' in why().decode()
    for spt in (1, 2, 4, 8, 16):
        assert call(du, st, spt=spt, n=0, **ku) == OK


def test_unsupported_follows_each_family():
    L = _lib.lib()
    st = _lib.NjodeOnlineState(256, 512, 768, 1024, 4)
    refused = dims_of(CONFIGS[online_util.REFUSED[0]])
    assert L.njode_online_supported(ctypes.byref(refused)) == 0
    msg = L.njode_last_error().decode()
    assert wave(L, refused, st) == UNSUP and L.njode_last_error().decode() == msg
    raw = ogu.REFUSED['rnn_4h_above_1024']
    d = gen_envelope.dims_of(*raw)
    assert L.njode_online_gen_supported(ctypes.byref(d)) == 0
    msg = L.njode_last_error().decode()
    assert gen(L, d, st) == UNSUP and L.njode_last_error().decode() == msg
    # the shape whose per-chain clocks do not fit: still refused, the run adds no LDS of its own ...
    assert gen(L, gen_envelope.dims_of(*ogu.LDS_WINDOW), st) == UNSUP
    # ... and one unit of hidden size less is still accepted
    smaller = (ogu.LDS_WINDOW[0], ogu.LDS_WINDOW[1] - 1) + ogu.LDS_WINDOW[2:]
    ds = gen_envelope.dims_of(*smaller)
    assert gen(L, ds, st, tb=_tables_bytes(ds), n=0) == OK


# ---- observe_many on CPU-resident states: ValueError before the RuntimeError that names the device ---
@pytest.fixture(scope='module')
def states():
    out = {}
    for key, d in (('demo', 2), ('masked', 41)):
        c = CONFIGS[3] if key == 'demo' else CONFIGS[online_util.PHYSIO]
        out[key] = (models.NJODE(**online_util.model_cfg(c)).eval().online(5, 0.01), d)
    out['generic'] = (models.NJODE(**ogu.SHAPES['one_layer_easy']).eval().online(5, 0.01, kernels='generic'), 2)
    return out


@pytest.mark.parametrize('key', ['demo', 'generic'])
def test_observe_many_value_errors(states, key):
    st, d = states[key]
    x, t, ptr = torch.zeros(3, d), [0.1, 0.2, 0.1], [0, 2, 3]
    # a well-formed call gets as far as the device
    with pytest.raises(RuntimeError, match='MI355X'):
        st.observe_many(ptr, t, x, kind=[1, 0, 1], ids=[4, 1])
    with pytest.raises(RuntimeError, match='MI355X'):
        st.observe_many([0, 0, 3, 3], t, x)
    # ev_ptr: wrong length for the ids, not starting at 0, decreasing, not ending at len(t), not integer, not flat
    for bad in ([0, 3], [0, 1, 2, 3], [1, 2, 3], [0, 3, 2], [0, 2, 2], [0, 2, 4], [0.0, 2.0, 3.0], [[0, 2, 3]], [], 3):
        with pytest.raises(ValueError):
            st.observe_many(bad, t, x, ids=[0, 1])
    with pytest.raises(ValueError):
        st.observe_many([0, 1, 1, 2, 2, 3, 3], t, x)      # six rows, five series, no ids
    # kind
    for bad in ([1, 2, 0], [1, -1, 0], [1, 0], [0.0, 1.0, 1.0], [[1, 0, 1]]):
        with pytest.raises(ValueError):
            st.observe_many(ptr, t, x, kind=bad, ids=[0, 1])
    # times
    for bad in ([0.1, float('nan'), 0.1], [0.1, float('inf'), 0.2], [-0.1, 0.2, 0.3], [[0.1, 0.2, 0.3]], 0.1):
        with pytest.raises(ValueError):
            st.observe_many(ptr, bad, x, ids=[0, 1])
    # shapes
    for bad in (torch.zeros(3, d + 1), torch.zeros(2, d), torch.zeros(3)):
        with pytest.raises(ValueError):
            st.observe_many(ptr, t, bad, ids=[0, 1])
    # ids
    for bad in ([1, 1], [0, 5], [-1, 2], [[0, 1]], [0.5, 1.0]):
        with pytest.raises(ValueError):
            st.observe_many(ptr, t, x, ids=bad)
    with pytest.raises(ValueError, match='unmasked'):
        st.observe_many(ptr, t, x, M=torch.ones(3, d), ids=[0, 1])


def test_observe_many_mask_rules(states):
    stm, dm = states['masked']
    xm = torch.zeros(3, dm)
    with pytest.raises(ValueError, match='needs M'):
        stm.observe_many([0, 2, 3], [0.1, 0.2, 0.1], xm, ids=[0, 1])
    with pytest.raises(ValueError):
        stm.observe_many([0, 2, 3], [0.1, 0.2, 0.1], xm, M=torch.ones(3, dm - 1), ids=[0, 1])
    with pytest.raises(ValueError):
        stm.observe_many([0, 2, 3], [0.1, 0.2, 0.1], xm, M=torch.ones(2, dm), ids=[0, 1])
    with pytest.raises(RuntimeError, match='MI355X'):
        stm.observe_many([0, 2, 3], [0.1, 0.2, 0.1], xm, M=torch.ones(3, dm), ids=[0, 1])


def test_eval_mode_only(states):
    st, d = states['demo']
    st.model.train()
    try:
        with pytest.raises(ValueError, match='eval'):
            st.observe_many([0, 1], [0.1], torch.zeros(1, d), ids=[0])
        with pytest.raises(ValueError, match='eval'):
            st.replay([0.1], [0, 1], torch.zeros(1, d), [0], fused=True)
    finally:
        st.model.eval()


def test_fused_replay_makes_the_checks_of_replay(states):
    st, d = states['demo']
    stm, dm = states['masked']
    for fused in (False, True):
        with pytest.raises(ValueError):
            st.replay([0.1, 0.2], [0, 1, 3], torch.zeros(2, d), [0, 1], fused=fused)       # time_ptr
        with pytest.raises(ValueError):
            st.replay([0.1, 0.2], [0, 1, 2], torch.zeros(3, d), [0, 1], fused=fused)       # rows of X
        with pytest.raises(ValueError, match='unmasked'):
            st.replay([0.1, 0.2], [0, 1, 2], torch.zeros(2, d), [0, 1], M=torch.ones(2, d), fused=fused)
        with pytest.raises(ValueError, match='needs M'):
            stm.replay([0.1], [0, 2], torch.zeros(2, dm), [0, 1], fused=fused)
        with pytest.raises(RuntimeError, match='MI355X'):
            st.replay([0.1, 0.2], [0, 1, 2], torch.zeros(2, d), [0, 1], fused=fused)
    # the fused form feeds one observe_many, whose checks come before the device as well
    with pytest.raises(ValueError, match='out of range'):
        st.replay([0.1, 0.2], [0, 1, 2], torch.zeros(2, d), [0, 7], fused=True)
    with pytest.raises(ValueError):
        st.replay([0.1, float('nan')], [0, 1, 2], torch.zeros(2, d), [0, 1], fused=True)


def test_default_of_replay_is_the_loop():
    import inspect
    assert inspect.signature(online.OnlineState.replay).parameters['fused'].default is False


# ---- the by-series layout ----------------------------------------------------------------------------
def restate(time_ptr, obs_idx):
    """by_series in plain loops: the rows of each series in slice order."""
    rows = {}
    for i in range(len(time_ptr) - 1):
        for r in range(time_ptr[i], time_ptr[i + 1]):
            rows.setdefault(int(obs_idx[r]), []).append(r)
    ids = sorted(rows)
    perm = [r for s in ids for r in rows[s]]
    ev_ptr = np.concatenate([[0], np.cumsum([len(rows[s]) for s in ids])]).astype(np.int64)
    inv = np.zeros(len(perm), dtype=np.int64)
    for k, r in enumerate(perm):
        inv[r] = k
    return np.asarray(ids, dtype=np.int64), ev_ptr, np.asarray(perm, dtype=np.int64), inv


LAYOUTS = {
    'an empty slice': ([0, 2, 2, 5, 6], [1, 0, 2, 0, 1, 2]),
    'a series without rows': ([0, 2, 3, 5], [3, 0, 0, 4, 3]),                 # series 1 and 2 have none
    'first and last row of the batch': ([0, 3, 5, 7], [2, 0, 1, 1, 0, 0, 2]),
    'no rows at all': ([0, 0, 0], []),
    'one series': ([0, 1, 2, 3], [4, 4, 4]),
}


@pytest.mark.parametrize('name', sorted(LAYOUTS))
def test_by_series(name):
    ptr, idx = LAYOUTS[name]
    got = online.by_series(ptr, idx)
    want = restate(ptr, idx)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w), (name, g, w)
    ids, ev_ptr, perm, inv = got
    idx = np.asarray(idx, dtype=np.int64)
    assert np.array_equal(perm[inv], np.arange(idx.size)) and np.array_equal(inv[perm], np.arange(idx.size))
    for r, s in enumerate(ids):
        mine = perm[ev_ptr[r]:ev_ptr[r + 1]]
        assert mine.size > 0 and np.all(idx[mine] == s) and np.all(np.diff(mine) > 0)
    # the same arrays, whatever they arrive as
    again = online.by_series(np.asarray(ptr, dtype=np.int32), torch.as_tensor(idx))
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_by_series_refuses_a_bad_time_ptr():
    for ptr, idx in (([0, 1, 3], [0, 1]), ([1, 2], [0, 1]), ([0, 2, 1, 2], [0, 1]), ([], [])):
        with pytest.raises(ValueError):
            online.by_series(ptr, idx)
