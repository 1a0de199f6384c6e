"""GRU-ODE-Bayes baseline without a GPU: the torch restatement (tests/gob_oracle.py) against the
goldens the reference's own class wrote, the surface of ``njode_amd.gru_ode_bayes.NNFOwithBayesianJumps``
(state_dict, initialisation, refusals), the harness keyword, and the pure-host entry points of
include/njode_gob.h.

Tolerances against the goldens are SURVEY 8c's numbers for "same ATen ops": loss relative <= 1e-6,
arrays <= 1e-6 absolute (gradients: relative to the tensor's largest entry, the same bound on a
scale-free number -- the KL term multiplies its inputs by 5 000)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gob_util
from gob_util import CASES, golden, golden_batch, golden_cfg, part
from njode_amd import _lib

HAVE_LIB = os.path.exists(_lib.LIB_PATH)
needs_lib = pytest.mark.skipif(not HAVE_LIB, reason='libnjode_hip.so not built in this checkout')


@pytest.mark.parametrize('name', CASES)
def test_restatement_equals_the_reference_goldens(name):
    g = golden(name)
    b, cfg = golden_batch(g), golden_cfg(g)
    sd = part(g, 'sd.')
    r = gob_util.restate(sd, b, cfg['mixing'], torch.float32, grads=True, return_path=True)
    for key in ('loss', 'loss_1'):
        assert abs(r[key] - float(g[key])) <= 1e-6 * abs(float(g[key])), (key, r[key], float(g[key]))
    for key in ('hT', 'path_p', 'path_h'):
        assert r[key].shape == g[key].shape
        assert np.abs(r[key] - g[key]).max() <= 1e-6, (key, np.abs(r[key] - g[key]).max())
    np.testing.assert_allclose(r['path_t'], g['path_t'], rtol=0, atol=1e-12)
    grads = part(g, 'g.')
    assert set(grads) == set(r['g'])
    for k, ref in grads.items():
        scale = max(np.abs(ref).max(), 1e-30)
        assert np.abs(r['g'][k] - ref).max() <= 1e-6 * max(scale, 1.0), (k, np.abs(r['g'][k] - ref).max(), scale)


def test_restatement_float64_is_close_to_its_float32_run():
    g = golden('gob_d1_impute')
    b, cfg = golden_batch(g), golden_cfg(g)
    r32 = gob_util.restate(part(g, 'sd.'), b, cfg['mixing'], torch.float32)
    r64 = gob_util.restate(part(g, 'sd.'), b, cfg['mixing'], torch.float64)
    assert abs(r32['loss'] - r64['loss']) <= 2e-6 * abs(r64['loss'])
    for k in r64['g']:
        assert gob_util.rel_l2(r32['g'][k], r64['g'][k]) < 1e-5, k


# ---- the class ------------------------------------------------------------------------------------

@needs_lib
@pytest.mark.parametrize('name', CASES)
def test_state_dict_keys_shapes_and_loading(name):
    from njode_amd import gru_ode_bayes
    g = golden(name)
    cfg, sd = golden_cfg(g), part(g, 'sd.')
    torch.manual_seed(0)
    m = gru_ode_bayes.NNFOwithBayesianJumps(**gob_util.model_kwargs(cfg))
    own = m.state_dict()
    assert list(own) == list(sd)
    for k in sd:
        assert tuple(own[k].shape) == sd[k].shape, k
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    for k, v in m.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), sd[k])
    # the kernels' parameters are views of one flat vector in state_dict order, the rest is outside it
    flat = m.flat_parameters()
    keys = [k for k in sd if not k.startswith(gob_util.SKIP)]
    assert flat.numel() == sum(sd[k].size for k in keys)
    np.testing.assert_array_equal(flat.numpy(), np.concatenate([sd[k].ravel() for k in keys]))
    assert m.epoch == 1 and m.weight == cfg['mixing'] and m.weight_decay_step() == cfg['mixing']


@needs_lib
def test_initialisation_statistics():
    from njode_amd import gru_ode_bayes
    cfg = dict(input_size=2, hidden_size=40, p_hidden=30, prep_hidden=8, cov_hidden=20, mixing=1e-4, impute=True)
    torch.manual_seed(5)
    m = gru_ode_bayes.NNFOwithBayesianJumps(**gob_util.model_kwargs(cfg))
    for name, mod in m.named_modules():
        if type(mod) == torch.nn.Linear:
            bound = np.sqrt(6.0 / (mod.in_features + mod.out_features))     # Xavier uniform
            w = mod.weight.detach().numpy()
            assert np.abs(w).max() <= bound * (1 + 1e-6), name
            if w.size >= 400:
                assert abs(w.std() - bound / np.sqrt(3.0)) < 0.15 * bound, name
            if mod.bias is not None:
                assert torch.all(mod.bias == 0.05), name
    assert torch.all(m.gru_obs.bias_prep == 0.1)
    assert abs(float(m.gru_obs.w_prep.detach().std()) - np.sqrt(2.0 / (4 + 8))) < 0.1
    k = 1.0 / np.sqrt(40)                                                    # GRUCell: untouched
    assert float(m.gru_obs.gru_d.weight_hh.abs().max()) <= k
    # bias=False: bias slots exist in the flat vector and are zero
    nb = gru_ode_bayes.NNFOwithBayesianJumps(**gob_util.model_kwargs(cfg, bias=False))
    assert nb.p_model[0].bias is None and not hasattr(nb.gru_c.lin_hh, 'bias_ih')
    assert nb.flat_parameters().numel() == m.flat_parameters().numel()


@needs_lib
@pytest.mark.parametrize('kw, word', [
    (dict(full_gru_ode=False), 'full_gru_ode'), (dict(logvar=False), 'logvar'),
    (dict(solver='midpoint'), 'solver'), (dict(solver='dopri5'), 'solver'),
    (dict(smoother=True), 'smoother'), (dict(store_hist=True), 'store_hist'),
    (dict(hidden_size=65), 'hidden_size'), (dict(prep_hidden=257), 'prep_hidden')])
def test_refusals_name_the_option(kw, word):
    from njode_amd import gru_ode_bayes
    args = gob_util.model_kwargs(dict(input_size=1, hidden_size=10, p_hidden=10, prep_hidden=10, cov_hidden=10,
                                      mixing=1e-4, impute=False))
    args.update(kw)
    with pytest.raises(NotImplementedError, match=word):
        gru_ode_bayes.NNFOwithBayesianJumps(**args)


@needs_lib
def test_cpu_inputs_raise_no_cpu_path():
    g = golden('gob_d1_plain')
    m = gob_util.hip_model(golden_cfg(g), part(g, 'sd.'), device='cpu')
    with pytest.raises(RuntimeError, match='no CPU path'):
        gob_util.hip_call(m, golden_batch(g))


def test_other_model_with_a_wrong_value_raises():
    from njode_amd import train
    for value in ('GRU_ODE', 'ODE_RNN', None):
        with pytest.raises(ValueError, match='other_model'):
            train.train((None, None, None), {}, other_model=value)


@needs_lib
def test_device_eval_does_not_apply_to_the_baseline():
    from njode_amd import train
    with pytest.raises(ValueError, match='device_eval'):
        train.train((None, None, None), {}, other_model='GRU_ODE_Bayes', device_eval=True)


# ---- pure-host entry points -------------------------------------------------------------------------

def _dims(d=1, H=10, PH=10, PR=10, CH=10, flags=_lib.GOB_F_BIAS):
    return _lib.NjodeGobDims(d, H, PH, PR, CH, flags)


def _count(d, H, PH, PR, CH, impute):
    n = PH * H + PH + 2 * d * PH + 2 * d + 3 * H * H + d * 4 * PR + d * PR
    n += 3 * H * PR * d + 3 * H * H + 6 * H + CH * d + CH + H * CH + H
    return n + (3 * H * 2 * d + 3 * H if impute else 0)


@needs_lib
def test_supported_param_count_and_the_envelope():
    L = _lib.lib()
    for d, H, PH, PR, CH in ((1, 10, 10, 10, 10), (5, 50, 25, 10, 50), (32, 64, 64, 8, 64), (1, 3, 1, 1, 1),
                             (1, 64, 64, 256, 64), (2, 50, 50, 50, 50)):
        for impute in (0, 1):
            dims = _dims(d, H, PH, PR, CH, _lib.GOB_F_BIAS | (_lib.GOB_F_IMPUTE if impute else 0))
            assert L.njode_gob_supported(ctypes.byref(dims)) == 1, (d, H, PH, PR, CH)
            assert L.njode_gob_param_count(ctypes.byref(dims)) == _count(d, H, PH, PR, CH, impute)
    for bad, word in ((_dims(H=65), 'hidden_size'), (_dims(PH=65), 'p_hidden'), (_dims(CH=65), 'cov_hidden'),
                      (_dims(d=33, PR=1), 'input_size'), (_dims(d=2, PR=129), 'prep_hidden'),
                      (_dims(H=0), 'positive'), (_dims(flags=4), 'flag')):
        assert L.njode_gob_supported(ctypes.byref(bad)) == 0
        assert word in L.njode_last_error().decode(), (word, L.njode_last_error())
        assert L.njode_gob_param_count(ctypes.byref(bad)) == 0


@needs_lib
def test_workspace_bytes_accepts_and_refuses():
    L = _lib.lib()
    need = ctypes.c_size_t(0)
    dims = _dims(5, 50, 25, 10, 50)
    sizes = {}
    for flags in (0, _lib.C_TRAIN, _lib.C_RETURN_PATH, _lib.C_SAVE_BWD, _lib.C_TRAIN | _lib.C_SAVE_BWD):
        assert L.njode_gob_workspace_bytes(ctypes.byref(dims), 9, 54, 30, 40, flags, ctypes.byref(need)) == 0
        sizes[flags] = need.value
        assert need.value % 256 == 0 and need.value > 0
    P = L.njode_gob_param_count(ctypes.byref(dims))
    # SAVE_BWD adds the stored states and nine slabs of P floats (a slab per path at this size)
    assert sizes[_lib.C_SAVE_BWD] - sizes[0] >= 4 * (40 * 9 * 50 + 54 * 50 + 9 * 50 + 9 * P)
    assert sizes[_lib.C_TRAIN] == sizes[0] == sizes[_lib.C_RETURN_PATH]
    # n_obs = 0 and no times at all are sizes like any other
    assert L.njode_gob_workspace_bytes(ctypes.byref(dims), 1, 0, 0, 0, _lib.C_SAVE_BWD, ctypes.byref(need)) == 0
    for args in ((0, 0, 0, 0, 0), (4, -1, 0, 0, 0), (4, 0, -1, 0, 0), (4, 0, 0, -1, 0),
                 (4, 0, 0, 0, _lib.C_GET_LOSS), (4, 0, 0, 0, 0x1000)):
        assert L.njode_gob_workspace_bytes(ctypes.byref(dims), *args, ctypes.byref(need)) == _lib.E_BADARG
    assert L.njode_gob_workspace_bytes(ctypes.byref(dims), 4, 0, 0, 0, 0, None) == _lib.E_BADARG
    assert L.njode_gob_workspace_bytes(ctypes.byref(_dims(H=65)), 4, 0, 0, 0, 0,
                                       ctypes.byref(need)) == _lib.E_UNSUPPORTED


@needs_lib
def test_exports_list_names_the_new_entry_points():
    L = _lib.lib()
    for name in ('njode_gob_supported', 'njode_gob_param_count', 'njode_gob_workspace_bytes',
                 'njode_gob_forward_f32', 'njode_gob_backward_f32'):
        assert name in _lib.EXPORTS and hasattr(L, name)
