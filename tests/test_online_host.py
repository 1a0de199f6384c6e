"""Online filtering, the part that needs no GPU: exported symbols, the verdict on every compiled
shape, the host-side argument checks, the default step bound, and the yardstick itself -- that the
batch-of-one truth the GPU tests use and the oracle's batch call describe the same thing where the
clocks coincide."""
import ctypes

import numpy as np
import pytest
import torch

import hip_util
import online_util
from njode_amd import _lib, models, online, schedule
from njode_amd.build import CONFIGS

NEW = ('njode_online_supported', 'njode_online_reset_f32', 'njode_online_advance_f32',
       'njode_online_observe_f32', 'njode_online_predict_f32')


def dims_of(c):
    d, H, DO, nh, W, act, masked, curt, res, rnn = c
    flags = ((_lib.F_MASKED if masked else 0) | (_lib.F_INPUT_CURRENT_T if curt else 0)
             | (_lib.F_RESIDUAL if res else 0) | (_lib.F_USE_RNN if rnn else 0))
    return _lib.NjodeDims(d, H, DO, nh, W, act, flags)


def test_symbols_exported():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert getattr(L, name) is not None


@pytest.mark.parametrize('i', range(len(CONFIGS)))
def test_supported_verdict(i):
    L = _lib.lib()
    c = CONFIGS[i]
    ok = L.njode_online_supported(ctypes.byref(dims_of(c)))
    why = L.njode_last_error().decode()
    assert ok == (1 if i in online_util.ACCEPTED else 0), (c, why)
    assert why.startswith('online: ') and len(why) > 12, why
    if c[3] == 0:
        assert 'nn_desc = None' in why
    if c[9]:
        assert 'use_rnn' in why


def test_verdict_counts_and_wide_models():
    assert len(online_util.ACCEPTED) == 10 and len(online_util.REFUSED) == 2
    L = _lib.lib()
    wide = dims_of((1, 10, 1, 2, 80, 0, 0, 0, 1, 0))
    assert L.njode_online_supported(ctypes.byref(wide)) == 0
    assert '<= 64' in L.njode_last_error().decode()
    absent = dims_of((3, 9, 3, 2, 30, 0, 0, 0, 1, 0))
    assert L.njode_online_supported(ctypes.byref(absent)) == 0
    assert 'build table' in L.njode_last_error().decode()


@pytest.mark.parametrize('i', online_util.REFUSED)
def test_factory_refuses_with_the_reason(i):
    m = models.NJODE(**online_util.model_cfg(CONFIGS[i])).eval()
    with pytest.raises(NotImplementedError) as e:
        m.online(4, 0.01)
    _lib.lib().njode_online_supported(ctypes.byref(dims_of(CONFIGS[i])))
    assert _lib.lib().njode_last_error().decode() in str(e.value)


def test_entry_points_refuse_bad_clock_before_any_launch():
    """delta_t <= 0 or non-finite and max_steps <= 0: NJODE_E_BADARG from pointer values that are
    never followed (no device here)."""
    L = _lib.lib()
    dims = dims_of(CONFIGS[online_util.DEMO])
    st = _lib.NjodeOnlineState(256, 512, 768, 1024, 4)
    for delta_t, max_steps in ((0.0, 5), (-1.0, 5), (float('inf'), 5), (float('nan'), 5), (0.1, 0), (0.1, -3)):
        rc = L.njode_online_advance_f32(ctypes.byref(dims), 256, ctypes.byref(st), None, 2, 256, delta_t,
                                        max_steps, 256, None)
        assert rc == _lib.E_BADARG, (delta_t, max_steps, L.njode_last_error())
        rc = L.njode_online_observe_f32(ctypes.byref(dims), 256, ctypes.byref(st), None, 2, 256, 256, None,
                                        delta_t, max_steps, None, None, 256, None)
        assert rc == _lib.E_BADARG
        rc = L.njode_online_predict_f32(ctypes.byref(dims), 256, ctypes.byref(st), None, 2, 256, 3, delta_t,
                                        max_steps, 256, 256, None)
        assert rc == _lib.E_BADARG
    # M on an unmasked model, a missing M on a masked one, more rows than series without ids
    assert L.njode_online_observe_f32(ctypes.byref(dims), 256, ctypes.byref(st), None, 2, 256, 256, 256, 0.1, 5,
                                      None, None, 256, None) == _lib.E_BADARG
    masked = dims_of(CONFIGS[online_util.PHYSIO])
    assert L.njode_online_observe_f32(ctypes.byref(masked), 256, ctypes.byref(st), None, 2, 256, 256, None, 0.1, 5,
                                      None, None, 256, None) == _lib.E_BADARG
    assert L.njode_online_reset_f32(ctypes.byref(dims), 256, ctypes.byref(st), None, 5, 256, None) == _lib.E_BADARG
    refused = dims_of(CONFIGS[online_util.REFUSED[0]])
    assert L.njode_online_reset_f32(ctypes.byref(refused), 256, ctypes.byref(st), None, 2, 256,
                                    None) == _lib.E_UNSUPPORTED


@pytest.fixture(scope='module')
def states():
    """A demo-shaped and a masked state on the CPU: every check below fires before the device is
    asked for."""
    out = {}
    for key, d in (('demo', 2), ('masked', 41)):
        c = CONFIGS[3] if key == 'demo' else CONFIGS[online_util.PHYSIO]
        out[key] = (models.NJODE(**online_util.model_cfg(c)).eval().online(5, 0.01), d)
    return out


def test_value_errors(states):
    st, d = states['demo']
    x = torch.zeros(2, d)
    for bad_ids in ([1, 1], [0, 5], [-1, 2], [[0, 1]], [0.5, 1.0]):
        with pytest.raises(ValueError):
            st.observe([0.1, 0.1], x, ids=bad_ids)
        with pytest.raises(ValueError):
            st.advance([0.1, 0.1], ids=bad_ids)
        with pytest.raises(ValueError):
            st.predict([[0.1], [0.1]], ids=bad_ids)
        with pytest.raises(ValueError):
            st.reset(x, ids=bad_ids)
    for bad_t in ([0.1, float('nan')], [0.1, float('inf')], [-0.1, 0.2], [0.1], [[0.1, 0.2]]):
        with pytest.raises(ValueError):
            st.observe(bad_t, x, ids=[0, 1])
        with pytest.raises(ValueError):
            st.advance(bad_t, ids=[0, 1])
    with pytest.raises(ValueError):
        st.predict([[0.1, float('nan')], [0.1, 0.2]], ids=[0, 1])
    with pytest.raises(ValueError, match='ascend'):
        st.predict([[0.2, 0.1], [0.1, 0.2]], ids=[0, 1])
    with pytest.raises(ValueError):
        st.predict([0.1, 0.2], ids=[0, 1])            # not [n, Q]
    with pytest.raises(ValueError, match='unmasked'):
        st.observe([0.1, 0.1], x, M=torch.ones(2, d), ids=[0, 1])
    for bad_x in (torch.zeros(2, d + 1), torch.zeros(3, d), torch.zeros(2)):
        with pytest.raises(ValueError):
            st.observe([0.1, 0.1], bad_x, ids=[0, 1])
        with pytest.raises(ValueError):
            st.reset(bad_x, ids=[0, 1])
    with pytest.raises(ValueError):
        st.reset(torch.zeros(6, d))                    # more rows than series, no ids
    with pytest.raises(ValueError):
        st.replay([0.1, 0.2], [0, 1, 3], torch.zeros(2, d), [0, 1])
    stm, dm = states['masked']
    xm = torch.zeros(2, dm)
    with pytest.raises(ValueError, match='needs M'):
        stm.observe([0.1, 0.1], xm, ids=[0, 1])
    with pytest.raises(ValueError):
        stm.observe([0.1, 0.1], xm, M=torch.ones(2, dm - 1), ids=[0, 1])
    with pytest.raises(ValueError, match='needs M'):
        stm.replay([0.1], [0, 2], xm, [0, 1])


def test_eval_mode_only(states):
    st, d = states['demo']
    st.model.train()
    try:
        with pytest.raises(ValueError, match='eval'):
            st.advance([0.1], ids=[0])
        with pytest.raises(ValueError, match='eval'):
            st.reset(torch.zeros(1, d), ids=[0])
    finally:
        st.model.eval()


def test_constructor_checks():
    m = models.NJODE(**online_util.model_cfg(CONFIGS[0])).eval()
    for n, dt in ((0, 0.1), (3, 0.0), (3, -1.0), (3, float('inf')), (3, float('nan'))):
        with pytest.raises(ValueError):
            m.online(n, dt)


def test_default_max_steps_is_an_upper_bound():
    b, dt, T = hip_util.exact_k_batch(5, 12, obs_per_path=3)
    cases = [(np.asarray(b['times']), dt), (np.asarray(b['times']), 0.37 * dt),
             (np.asarray([0.0, 0.0, 0.3 * dt, 5.77 * dt, T]), 0.37 * dt), (np.asarray([1e-13, 7.0]), 0.5)]
    for times, delta_t in cases:
        for t in times:
            for now in [0.0] + [float(x) for x in times if x <= t]:
                # one call: from the clock a series has after the target `now` to the target t
                dts, _, k_jump, _, _ = schedule._walk_clock([now, t], delta_t, 0.0, False)
                n = len(dts) - k_jump[0]
                assert n <= online.default_max_steps([t], delta_t), (t, now, delta_t, n)
        assert online.default_max_steps(times, delta_t) == max(online.default_max_steps([t], delta_t) for t in times)


def test_yardstick_batch_of_one_is_the_batch():
    """On the exact grid (2**-10, every step a full one, all arithmetic of the clock exact) the
    oracle's batch call and its five batch-of-one calls agree on each series' path_y rows and hT:
    1e-6 in fp32, a few ulps in float64."""
    b, dt, T = hip_util.exact_k_batch(5, 12)
    cfg = hip_util.demo_cfg()
    sd = online_util.params_of(cfg)
    o32, o64 = hip_util.oracle_pair(cfg, sd, b, dt, T, predict=True, get_loss=False, until_T=True)
    rows_b = schedule._walk_clock(b['times'], dt, T, True)[4]
    times = list(np.asarray(b['times']))
    for s in range(5):
        ev = online_util.series_events(b, s)
        assert ev
        s32, s64, rows = online_util.truth(cfg, sd, ev, b['start_X'][s], dt, T)
        for one, batch, tol in ((s32, o32, 1e-6), (s64, o64, 1e-14)):
            assert np.abs(one['hT'][0] - batch['hT'][s]).max() <= tol
            for (t, _, _), r in zip(ev, rows):
                rb = rows_b[times.index(t)]
                assert np.abs(one['path_y'][r, 0] - batch['path_y'][rb, s]).max() <= tol, (s, t)
                assert np.abs(one['path_y'][r - 1, 0] - batch['path_y'][rb - 1, s]).max() <= tol, (s, t)
