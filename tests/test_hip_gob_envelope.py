"""The GRU-ODE-Bayes baseline (``njode_gob.hip``, ``njode_amd/gru_ode_bayes.py``) across its stated
envelope, at both clamps of its slab count and with dropout off the regular grid, against the float64
run of the torch restatement under the rule and floors of ``test_hip_gob`` (its ``check``, ``pair``,
``hip_run`` and ``FLOOR_*``, imported, not copied):

    err(HIP, f64) <= max(2 err(fp32 restatement, f64), floor)

``k_gob_fwd`` and ``k_gob_bwd`` take every size at run time, so their risks sit in run-time branches the
golden shapes do not enter: prep units that straddle the 64-lane chunks (``from_options``' default
``prep_hidden = hidden_size`` on five climate features gives 250 units), layers wider than
``hidden_size`` (lanes are clamped by a different bound per layer), upstream gradients of both losses at
once, a workgroup of the sweep that takes several paths of a model that does real work, the byte budget
as the binding slab clamp, and the mask key of a lazily evaluated ``p`` where the schedule is irregular.
The cases are defined and labelled by ``tests/gob_envelope.py``, the restatement
``test_gob_envelope_host`` pins to the library; every test here asserts the labels it is about.

Cases (``random_batch`` walks on steps of 0.05, both ``impute`` settings unless the case is a golden
one): the lane layouts ``straddle250`` (d 5, all widths 50: features straddle lanes 64, 128 and 192, the
last chunk is partial), ``straddle255`` (d 3, H 9, p_hidden = cov_hidden = 64, prep 85), ``d32_small``
(d 32, H 5, p_hidden 3, prep 7, cov_hidden 2: 2 d = 64 > H, d > cov_hidden), ``ng65``, ``ng150`` (three
chunks; added to the issue's table, which has none) and ``straddle250`` without bias, training call with
``c_hT`` and path call each; a batch nobody is observed in at d 2, H 11; the objectives 0.7 loss + 0.4
loss_1 + <c, hT>, the same without c at mixing = 0, <c, hT> alone and loss + loss_1 on the d = 1 impute
golden batch and on ``straddle250``; d 2, H 11, p_hidden 9, prep 5, cov_hidden 6 at B = 1 030 and 2 050
(S = 1 024; a workgroup takes two and three paths), at 1 030 again with dropout 0.1, and four of its paths
alone, bit for bit; d 32 with 64-wide layers at B = 760 (S = 745 / 654 by the 256 MiB budget);
``hip_util.irregular_batch`` of two golden batches under dropout 0.1 on two consecutive steps, the same
with a second slice on one Euler step, with and without dropout, training-mode path calls on both, and
``straddle255`` at p = 0.5; the C ABI between guard bands on ``straddle250``, B = 1 030 and B = 760.

Measured on an MI355X.  No case is outside the rule and no defect was found.  Worst err(HIP) /
err(fp32) per family, on arrays and on a loss, and the worst err / bound: lane layouts 2.29 (a gradient
at 3.9e-7 relative L2) and 31.0 on a loss (2.5e-4 of 2 543, 9.9e-8 relative, where the fp32 restatement
landed 3.2e-9 from float64), err / bound 0.105; objectives 2.44 (a gradient at 1.8e-7), 0.079; slabs 2.04
and 14.8 on a loss (1.1e-7 relative), 0.111; B = 1 030 with dropout 1.22 and 103.9 on a loss (1.2e-7
relative next to the restatement's 1.1e-9), 0.116; dropout off the grid 2.54 (a gradient at 1.2e-7),
0.231 (``path_h`` at 4.6e-7, the fp32 restatement at 4.0e-7).  Wherever the ratio exceeds 2 the error is
below the floor; no floor was raised.  Wall time: 5.5 s for the 53 tests (the slowest 0.85 s, the first
one, which loads the library; every other one below 0.25 s, the two 0.6 GB guard-band arenas of B = 760
included, so ``min_guard`` stays at its default), next to 7.1 s for ``test_hip_gob.py`` in the same run.

Mutations of ``njode_gob.hip`` (scratch copies, numerically wrong, every access in range, never
committed; each built and run once), the tests of this module that fail, and ``test_hip_gob.py``:

  (a) the prep adjoint credits a feature only in the chunk where it starts: all 12 ``test_lane_layouts``,
      the 8 ``test_objectives`` on ``straddle250``, both ``test_dropout_at_width_64``; the existing module
      fails ``prep256_d1`` (one feature over four chunks) and passes the other 48.
  (b) ``c2 = (grad_loss + grad_loss_1) * mixing``: the 6 ``test_objectives`` with (0.7, 0.4) + c and
      (1, 1) (mixing = 0 and <c, hT> alone cannot see it); the existing module fails its four ``loss_1``
      gradient cases.
  (c) rows j >= H of ``p_model.0``'s weight gradient skipped in ``pm_bwd``: both ``straddle255`` rows of
      ``test_lane_layouts``, both ``test_dropout_at_width_64``; the existing module passes (50 of 50).
  (d) ``keep_unit`` returns true under ``RETURN_PATH``: the four ``test_training_mode_path_calls``; the
      existing module passes.
  (e) the slice consumer's ``prev_key`` called with ``i + 1``: both ``test_max_slabs_with_dropout``, both
      ``test_dropout_on_irregular_batches``, both ``test_two_slices_on_one_euler_step`` with p = 0.1, both
      ``test_dropout_at_width_64``; the existing module fails its four dropout cases.
  (f) ``lam`` seeded from ``grad_hT`` for a workgroup's first path only: all 8 slab tests; the existing
      module fails ``B1030_shared_slabs``.
  (g) ``prev_key`` with ``>`` for ``>=`` (a slice directly after a slice, or a step directly after one,
      takes the key of the Euler step before): ``test_two_slices_on_one_euler_step`` with p = 0.1 on both
      batches and the impute rows of three more dropout tests; without ``impute`` nothing but the
      two-slices case sees it (the existing module fails its two impute dropout cases).
  (h) ``p_model.3``'s bias gradient skipped for lanes >= H: both ``d32_small`` rows; the existing module
      fails ``tiny_h3_prep1``.
"""
import functools

import numpy as np
import pytest
import torch

import gob_envelope as ge
import gob_util
from gob_util import golden, part
from njode_amd import _lib, schedule
from oracle import dropout_oracle
from test_hip_gob import abi_call, c_of, check, hip_run, pair, random_model

pytestmark = pytest.mark.gpu

CASES = ge.case_table()
BOTH = pytest.mark.parametrize('impute', [False, True], ids=['plain', 'impute'])
SEED = 0x1234567 * 2 ** 32 + 0x89ABCDE        # dropout seed of test_hip_gob's mask test


@functools.lru_cache(maxsize=None)
def batch(name):
    """A case's batch: made once, shared, never modified."""
    return CASES[name][1]()


def case(name, impute):
    cfg, _, bias = CASES[name]
    cfg = dict(cfg, impute=impute)
    b = batch(name)
    return cfg, b, bias, ge.labels(cfg, *ge.call_sizes(b), bias=bias)


def model_of(name, impute, **kw):
    """The case's HIP model (one seeded initialisation per model family) and its state dict; a golden
    case's own parameters."""
    cfg, _, bias = CASES[name]
    cfg = dict(cfg, impute=impute)
    family = name.split('/')[0]
    if family in ge.GOLDEN:
        sd = part(golden(family), 'sd.')
        return gob_util.hip_model(cfg, sd, **kw), sd
    return random_model(cfg, 40 + sorted({n.split('/')[0] for n in CASES}).index(family), bias=bias, **kw)


def all_live(r64):
    """Every gradient tensor of the float64 truth is non-zero: no tensor is checked against zeros."""
    dead = [k for k, g in r64['g'].items() if not np.abs(g).max() > 0]
    assert not dead, dead


def masks_of(step, p):
    return dropout_oracle.KernelMasks('gen', dropout_oracle.call_seed(SEED, step), p)


# ---- 1. lane layouts ------------------------------------------------------------------------------------
LANE_LABELS = {
    'straddle250': {'chunks4', 'last_chunk_partial', 'feature_straddles_chunk'},
    'straddle255': {'chunks4', 'last_chunk_partial', 'feature_straddles_chunk', 'PH_gt_H', 'CH_gt_H'},
    'd32_small': {'chunks4', 'last_chunk_partial', 'feature_straddles_chunk', 'D2_gt_H', 'D_gt_CH'},
    'ng65': {'chunks2', 'last_chunk_partial', 'feature_straddles_chunk'},
    'ng150': {'chunks3', 'last_chunk_partial', 'feature_straddles_chunk'},
    'straddle250_nobias': {'chunks4', 'feature_straddles_chunk', 'no_bias'},
}


@BOTH
@pytest.mark.parametrize('name', ge.LANES)
def test_lane_layouts(name, impute):
    """Training call (loss + <c, hT>: loss, loss_1, hT, every gradient tensor) and path call."""
    cfg, b, bias, lab = case(name, impute)
    assert LANE_LABELS[name] <= lab and 'S_eq_B' in lab, lab
    m, sd = model_of(name, impute)
    c = c_of(b, cfg)
    r32, r64 = pair(sd, b, cfg['mixing'], c_hT=c)
    all_live(r64)
    tag = '{} impute={:d}'.format(name, impute)
    res = hip_run(m.train(), b, c_hT=c)
    check(tag, res, r32, r64)
    if not bias:
        assert 'p_model.0.bias' not in res['g'] and 'gru_obs.gru_d.bias_ih' not in res['g']
    p32, p64 = pair(sd, b, cfg['mixing'], grads=False, return_path=True)
    check(tag + ' path', hip_run(m.eval(), b, return_path=True), p32, p64)


def test_no_rows_at_a_real_size():
    """Nobody is observed: both losses exactly 0, hT and the gradients of <c, hT> against the truth."""
    cfg, b, bias, lab = case('shared_real/no_rows', True)
    assert {'no_rows', 'impute', 'S_eq_B'} <= lab
    m, sd = model_of('shared_real/no_rows', True)
    c = c_of(b, cfg)
    r32, r64 = pair(sd, b, cfg['mixing'], c_hT=c)
    res = hip_run(m.train(), b, c_hT=c)
    check('shared_real/no_rows', res, r32, r64)
    assert res['loss'] == 0.0 and res['loss_1'] == 0.0 and not res['g']['gru_obs.w_prep'].any()


# ---- 2. objectives ----------------------------------------------------------------------------------------
OBJECTIVES = [
    # id, (a, b) of a * loss + b * loss_1, with <c, hT>, mixing (None: the case's)
    ('0.7loss+0.4loss_1+c.hT', (0.7, 0.4), True, None),
    ('0.7loss+0.4loss_1_mixing0', (0.7, 0.4), False, 0.0),
    ('c.hT_alone', (0, 0), True, None),
    ('loss+loss_1', (1, 1), False, None),
]


@pytest.mark.parametrize('tag, ab, with_c, mixing', OBJECTIVES, ids=[o[0] for o in OBJECTIVES])
@pytest.mark.parametrize('name, impute', [('gob_d1_impute', True), ('straddle250', False), ('straddle250', True)])
def test_objectives(name, impute, tag, ab, with_c, mixing):
    """Both upstream gradients at once: c1 = grad_loss + grad_loss_1 on the terms of loss_1,
    c2 = grad_loss * mixing on those of loss_2."""
    cfg, b, bias, lab = case(name, impute)
    assert ('feature_straddles_chunk' in lab) == (name == 'straddle250') and int(b['time_ptr'][-1]) > 0
    if mixing is not None:
        cfg = dict(cfg, mixing=mixing)
    m, sd = model_of(name, impute)
    m.mixing = cfg['mixing']
    c = c_of(b, cfg) if with_c else None
    r32, r64 = pair(sd, b, cfg['mixing'], objective=ab, c_hT=c)
    all_live(r64)
    check('{} impute={:d} {}'.format(name, impute, tag), hip_run(m.train(), b, ab, c), r32, r64)


# ---- 3. slabs ---------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize('B', [1030, 2050])
def test_max_slabs_at_a_model_that_does_real_work(B, impute):
    """S = 1 024 < B: workgroups 0 - 5 of the sweep take two paths (B = 2 050: two take three), three
    masked rows per path on ten Euler steps."""
    name = 'shared_real/b{}'.format(B)
    cfg, b, bias, lab = case(name, impute)
    assert {'S_max_slabs', 'B_gt_256'} <= lab and ('slab_takes_3' in lab) == (B == 2050)
    m, sd = model_of(name, impute)
    c = c_of(b, cfg)
    r32, r64 = pair(sd, b, cfg['mixing'], c_hT=c)
    all_live(r64)
    check('{} impute={:d}'.format(name, impute), hip_run(m.train(), b, c_hT=c), r32, r64)


@BOTH
def test_max_slabs_with_dropout(impute):
    """... with dropout 0.1 and the kernels' masks: path ids >= 1 024 enter the mask keys."""
    cfg, b, bias, lab = case('shared_real/b1030', impute)
    assert 'S_max_slabs' in lab
    m, sd = model_of('shared_real/b1030', impute, dropout_rate=0.1, dropout_seed=SEED)
    c = c_of(b, cfg)
    r32, r64 = pair(sd, b, cfg['mixing'], c_hT=c, masks=masks_of(0, 0.1))
    check('shared_real/b1030 p=0.1 impute={:d}'.format(impute), hip_run(m.train(), b, c_hT=c), r32, r64)


@BOTH
def test_paths_alone_and_inside_1030_are_bit_equal(impute):
    """The forward is per path: hT of paths 0, 1 023, 1 024 and 1 029 of the eval call, in bits, alone
    (B = 1, the same rows on the same times) and inside the batch."""
    cfg, b, bias, lab = case('shared_real/b1030', impute)
    assert 'S_max_slabs' in lab
    m, sd = model_of('shared_real/b1030', impute)
    big = hip_run(m.eval(), b, grads=False)
    for p in ge.ALONE:
        name = 'shared_real/alone{}'.format(p)
        one = batch(name)
        assert {'b1', 'S_eq_B'} <= case(name, impute)[3]
        assert int(one['time_ptr'][-1]) == int((b['obs_idx'] == p).sum()) == 3
        alone = hip_run(m, one, grads=False)
        assert np.array_equal(alone['hT'][0], big['hT'][p]), p


@BOTH
def test_slab_byte_budget(impute):
    """d = 32 next to three 64-wide layers: 745 (654 with impute) slabs fit 256 MiB, 760 paths share them."""
    cfg, b, bias, lab = case('budget/b760', impute)
    assert {'S_byte_budget', 'chunks4', 'B_gt_256'} <= lab
    assert ge.slab_count(ge.param_count(cfg), 760) == (654 if impute else 745)
    m, sd = model_of('budget/b760', impute)
    c = c_of(b, cfg)
    r32, r64 = pair(sd, b, cfg['mixing'], c_hT=c)
    all_live(r64)
    check('budget/b760 impute={:d}'.format(impute), hip_run(m.train(), b, c_hT=c), r32, r64)


# ---- 4. dropout off the regular grid -----------------------------------------------------------------------
def irregular(name, kind='irregular'):
    """The irregular batch of a golden case, with the properties the tests are about."""
    cfg, b, bias, lab = case('{}/{}'.format(name, kind), ge.golden_cfg(name)[1])
    s = schedule.Schedule(b['times'], b['delta_t'], b['T'], True)
    assert b['times'][0] == 0.0 and s.k_jump[0] == 0 and int(b['obs_idx'][0]) == 0      # TKEY_START feeds a slice
    assert (np.diff(b['time_ptr']) == 0).any()                                          # a slice without rows
    assert (s.step_dt < np.float32(0.999 * b['delta_t'])).any()                         # partial Euler steps
    return cfg, b, s


@pytest.mark.parametrize('name', ge.GOLDEN)
def test_dropout_on_irregular_batches(name):
    """p = 0.1, two consecutive steps with the kernels' masks: a jump at t = 0, partial Euler steps, a
    slice without rows."""
    cfg, b, s = irregular(name)
    m, sd = model_of(name, cfg['impute'], dropout_rate=0.1, dropout_seed=SEED)
    m.train()
    first = None
    for step in range(2):
        r32, r64 = pair(sd, b, cfg['mixing'], masks=masks_of(step, 0.1))
        res = hip_run(m, b)
        check('{} irregular p=0.1 step {}'.format(name, step), res, r32, r64)
        first = first or res
    assert first['loss'] != res['loss']


@pytest.mark.parametrize('p_drop', [0.0, 0.1])
@pytest.mark.parametrize('name', ge.GOLDEN)
def test_two_slices_on_one_euler_step(name, p_drop):
    """A time 1e-11 delta_t after an observed one: both slices have the same ``k_jump``, the second
    one's ``p`` is the first one's (net 7, the same time key), and one path has a row in both."""
    cfg, b, s = irregular(name, 'two_slices')
    assert (s.k_jump[1:] == s.k_jump[:-1]).sum() == 1, s.k_jump
    m, sd = model_of(name, cfg['impute'], dropout_rate=p_drop, dropout_seed=SEED)
    c = c_of(b, cfg)
    masks = masks_of(0, p_drop) if p_drop else None
    r32, r64 = pair(sd, b, cfg['mixing'], c_hT=c, masks=masks)
    check('{} two slices p={}'.format(name, p_drop), hip_run(m.train(), b, c_hT=c), r32, r64)
    if not p_drop:
        p32, p64 = pair(sd, b, cfg['mixing'], grads=False, return_path=True)
        check('{} two slices path'.format(name), hip_run(m.eval(), b, return_path=True), p32, p64)


@pytest.mark.parametrize('kind', ['irregular', 'two_slices'])
@pytest.mark.parametrize('name', ge.GOLDEN)
def test_training_mode_path_calls(name, kind):
    """``model.train(); model(..., return_path=True)``: TRAIN | RETURN_PATH.  path_p, path_h, hT and
    the loss against the restatement with the masks of that step; hT and loss bit-equal to a plain
    training call of a second model with the same seed at the same step."""
    cfg, b, s = irregular(name, kind)
    m, sd = model_of(name, cfg['impute'], dropout_rate=0.1, dropout_seed=SEED)
    twin, _ = model_of(name, cfg['impute'], dropout_rate=0.1, dropout_seed=SEED)
    m.train(), twin.train()
    for step in range(2):
        p32, p64 = pair(sd, b, cfg['mixing'], grads=False, return_path=True, masks=masks_of(step, 0.1))
        pa = hip_run(m, b, return_path=True)
        check('{} {} train-mode path step {}'.format(name, kind, step), pa, p32, p64)
        np.testing.assert_allclose(pa['path_t'], p64['path_t'], rtol=0, atol=1e-12)
        plain = hip_run(twin, b)
        assert pa['loss'] == plain['loss'] and np.array_equal(pa['hT'], plain['hT']), step
    # (the masks are drawn: the eval path differs)
    assert not np.array_equal(hip_run(m.eval(), b, return_path=True)['path_p'], pa['path_p'])


@BOTH
def test_dropout_at_width_64(impute):
    """``straddle255`` at p = 0.5: p_hidden = cov_hidden = 64 units draw 32 mask words each."""
    cfg, b, bias, lab = case('straddle255', impute)
    assert {'PH_gt_H', 'CH_gt_H', 'chunks4'} <= lab and cfg['p_hidden'] == cfg['cov_hidden'] == 64
    m, sd = model_of('straddle255', impute, dropout_rate=0.5, dropout_seed=SEED)
    c = c_of(b, cfg)
    r32, r64 = pair(sd, b, cfg['mixing'], c_hT=c, masks=masks_of(0, 0.5))
    check('straddle255 p=0.5 impute={:d}'.format(impute), hip_run(m.train(), b, c_hT=c), r32, r64)


# ---- 5. exact sizes between guard bands ----------------------------------------------------------------------
ABI = [('straddle250', False), ('straddle250', True), ('shared_real/b1030', False), ('shared_real/b1030', True),
       ('budget/b760', False), ('budget/b760', True)]


@pytest.mark.parametrize('name, impute', ABI, ids=['{}-{}'.format(n, 'impute' if i else 'plain') for n, i in ABI])
def test_abi_stays_inside_buffers_of_exactly_the_stated_size(name, impute):
    """TRAIN | RETURN_PATH | SAVE_BWD with dropout 0.1 through the C ABI, both pattern phases: return
    codes 0, no guard byte changed, outputs finite and bit-equal across the phases."""
    cfg, b, bias, lab = case(name, impute)
    assert {'straddle250': 'feature_straddles_chunk', 'shared_real/b1030': 'S_max_slabs',
            'budget/b760': 'S_byte_budget'}[name] in lab
    _, sd = model_of(name, impute)
    outs = []
    for phase in (0, 1):
        A, fwd, bwd, need, (B, H, D, n_rows, P) = abi_call(cfg, sd, b, phase)
        assert need == ge.workspace_bytes(cfg, *ge.call_sizes(b), _lib.C_TRAIN | _lib.C_SAVE_BWD) and P == ge.param_count(cfg)
        assert fwd() == 0, _lib.lib().njode_last_error()
        assert bwd() == 0, _lib.lib().njode_last_error()
        assert A.check() == []
        outs.append([A.view(n, torch.float32).clone() for n in ('hT', 'loss', 'path_h', 'path_p', 'grad_params')])
        del A, fwd, bwd
    for a, z in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, z)     # nothing read from in or around the buffers
