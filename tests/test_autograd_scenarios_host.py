"""The scenario table of tests/autograd_scenarios.py on the CPU oracle alone, in fp32 and float64: what
plain ``torch.autograd`` really does under each scenario's statements.  The GPU half
(tests/test_hip_autograd_contract.py) takes its expectations from the same runs; this module states,
where there is no GPU, the outcomes that contract relies on:

* a parameter step between a forward and its backward raises (``param_step_*``, ``param_flat_copy``);
* an in-place change of ``M`` (masked model) or ``obs_idx`` raises; one of ``X``, ``start_X`` or
  ``n_obs_ot`` goes ahead and leaves the gradient of the forward-time batch, bit for bit;
* every other scenario runs, fp32 and float64 agree, frozen tensors keep ``.grad is None``, a frozen
  model builds no graph, in-place arithmetic on the outputs back-propagates.
"""
import numpy as np
import pytest
import torch

import autograd_scenarios as S
from hip_util import rel_l2

RAISES = {'param_step_torch', 'param_step_fused', 'param_flat_copy', 'input_inplace_obs_idx'}
RAISES_MASKED = RAISES | {'input_inplace_M'}

_ROWS = {}
_RUNS = {}


def rows():
    if not _ROWS:
        _ROWS.update(S.model_rows(small=True))
    return _ROWS


def outcome(model, name):
    if (model, name) not in _RUNS:
        r = rows()[model]
        _RUNS[model, name] = S.run_on_oracle(name, r['cfg'], r['sd'], r['A'], r['B'], r['stream'])
    return _RUNS[model, name]


def plain_step(model):
    """the gradient of one untouched forward + backward on batch A (float64)"""
    if (model, None) not in _RUNS:
        r = rows()[model]
        with S.one_thread():
            m = S.OracleModel(r['cfg'], r['sd'], torch.float64, r['stream'])
            h, l = m(S.oracle_batch(r['A'], torch.float64))
            l.backward()
            _RUNS[model, None] = m.observe(l, h)
    return _RUNS[model, None]


@pytest.mark.parametrize('name', list(S.SCENARIOS))
@pytest.mark.parametrize('model', ['demo', 'masked'])
def test_scenario_on_the_oracle(model, name):
    (k32, o32), (k64, o64) = outcome(model, name)
    want = 'raises' if name in (RAISES_MASKED if model == 'masked' else RAISES) else 'ok'
    assert k32 == k64 == want, (model, name, k32, k64, o32 if k32 == 'raises' else '', o64 if k64 == 'raises' else '')
    if want == 'raises':
        assert 'modified by an inplace operation' in o64, o64
        return
    assert o32.keys() == o64.keys() and 'final' in o64
    for tag in o64:
        a, b = o32[tag], o64[tag]
        assert a['flags'] == b['flags']
        assert a['loss'] == pytest.approx(b['loss'], rel=1e-4, abs=1e-9)
        for k, g in b['g'].items():
            assert (g is None) == (a['g'][k] is None), (tag, k)
            if g is not None and np.any(g):
                assert rel_l2(a['g'][k], g) < 1e-3, (tag, k, rel_l2(a['g'][k], g))
            elif g is not None:
                assert not np.any(a['g'][k]), (tag, k)


@pytest.mark.parametrize('model', ['demo', 'masked'])
@pytest.mark.parametrize('which', ['X', 'start_X', 'n_obs_ot'])
def test_a_changed_batch_value_does_not_move_the_gradient(model, which):
    _, (kind, obs) = outcome(model, 'input_inplace_' + which)
    assert kind == 'ok'
    ref = plain_step(model)
    assert obs['final']['loss'] == ref['loss']
    for k, g in ref['g'].items():
        assert np.array_equal(obs['final']['g'][k], g), k


@pytest.mark.parametrize('model', ['demo', 'masked'])
def test_frozen_tensors_keep_no_grad(model):
    for name, frozen in (('frozen_readout', lambda k: k.startswith('readout_map.')),
                         ('frozen_all_but_ode', lambda k: not k.startswith('ode_f.')),
                         ('frozen_all', lambda k: True)):
        _, (kind, obs) = outcome(model, name)
        assert kind == 'ok'
        f = obs['final']
        assert f['flags']['no_graph'] == (name == 'frozen_all')
        for k, g in f['g'].items():
            assert (g is None) == frozen(k), (name, k)
        if name != 'frozen_all':
            ref = plain_step(model)
            for k, g in f['g'].items():
                if g is not None:      # (the trainable tensors: the gradient they always had)
                    assert rel_l2(g, ref['g'][k]) < 1e-12, (name, k)


@pytest.mark.parametrize('model', ['demo', 'masked'])
def test_outputs_and_sums_follow_the_chain_rule(model):
    """sanity of the table itself: the scenarios' objectives are what their names say"""
    ref = plain_step(model)
    _, (_, up) = outcome(model, 'upstream')
    for k, g in up['zero']['g'].items():
        assert g is not None and not np.any(g), k
    _, (_, acc) = outcome(model, 'accumulate')
    for k, g in ref['g'].items():
        assert rel_l2(acc['final']['g'][k], g) < 1e-12, k
        assert rel_l2(acc['two']['g'][k], g) > 1e-3, k        # (two batches were summed)
    _, (_, sub) = outcome(model, 'grad_subset')
    got = {k: g for k, g in sub['final']['g'].items() if g is not None}
    assert len(got) == 2
    for k, g in got.items():
        assert rel_l2(g, ref['g'][k]) < 1e-12, k
    _, (_, st) = outcome(model, 'state_change')
    assert abs(st['final']['loss'] - ref['loss']) > 1e-4 * abs(ref['loss'])   # (weight 0.7, dropout: another loss)
