"""The float64 route (``njode_amd.float64.NJODE64``, ``njode_f64.hip``) across its stated envelope and at
both clamps of its slab count, against the float64 CPU oracle under the bound of
``test_hip_f64_route`` (its ``Checker``, ``REL`` and ``FLOOR``, imported, not copied):

    err(HIP f64, f64 oracle) <= max(1e-6 x e32, 256 x 2^-52 x max|truth|)

The route takes every shape at run time, so its risks sit in run-time branches: the lanes the slab
update deals to a weight row, the path loop of a workgroup of the adjoint sweep (S < B slabs: the
per-path re-seeding of lam, lamx, last_X and tau, a slab that takes several paths), the strided loops of
the loss tree and the row table, depth 0 and 8, the residual cases with real chunks.  The cases are
defined and labelled by ``tests/f64_envelope.py``, the restatement ``test_f64_envelope_host`` pins to the
library; every test here asserts the labels it is about.

Cases: the 19 rows of ``test_hip_generic_envelope.ROWS`` without ``use_rnn`` (training call with a fixed
``c_hT`` and path call each; ``d3_do7`` the path call and the refusal of its loss), that module's edges
``b1`` / ``empty`` / ``longK``, the demo and a masked model at B = 2 100 (S = 2 048), an ODE network of
eight 1 024-wide layers at B = 20 (S = 18 by the byte budget), 250 x 2 100 row-table entries, a batch
without observations, bit-equal paths alone and inside 2 100, and the Python surface (``get_pred``,
``device_outputs=False``, ``float64()`` of a device model, deep copies).  Two rows the envelope table
does not have were added after the first run: ``deep8_live`` (the ODE network of ``deep_mixed`` is dead
behind its width-1 relu, so its nine gradients are exactly zero there) and ``masked_res12`` /
``masked_res21`` (the adjoint of the encoder's residual runs in masked models only, and the table's
masked rows have D = H).

Measured (one MI355X, ``profiles/f64_route.jsonl``): every row is inside the shared bound, no row has a
``REL`` of its own.  Worst err / e32 per branch family: widths and lane layouts 1.2e-7 (``w1``, an ODE
bias gradient), depth 3.5e-8, large D and masked 3.9e-9, residual chunks 1.1e-8, the b1 / empty / longK
edges 2.3e-8, S = 2 048 < B 2.3e-8, the byte budget (S = 18) 4.2e-7 (the loss; 0.0045 of its bound, which
is the floor there), the strided row table 5.7e-9, no observations 2.9e-9.  The largest err / bound of
the module is 0.027.  Wall time: 14.3 s for the 59 tests (the slowest, the 250 x 2 100 row table, 3.3 s,
the CPU oracle's), next to 7.2 s for ``test_hip_f64_route.py`` on the same machine.

Mutations of ``njode_f64.hip`` (numerically wrong, no access out of range; never committed), the tests of
this module that fail, and whether ``test_hip_f64_route.py`` notices:

  (a) ``lam`` seeded from ``grad_hT`` for a workgroup's first path only: ``test_max_slabs_unmasked``,
      ``test_max_slabs_masked``, ``test_slab_byte_budget``, ``test_row_table_beyond_the_clear_grid``;
      the existing module passes (51 of 51).
  (b) ``lamx`` reset for a workgroup's first path only: ``test_max_slabs_masked``; the existing module
      passes.
  (c) ``tree_sum_256`` (under ``k_f64_loss``) reads the first 256 partials only: ``test_max_slabs_unmasked``,
      ``test_max_slabs_masked``, ``test_row_table_beyond_the_clear_grid``; the existing module passes.
  (d) ``res_bwd`` case 2 without the division by ``mult``: 19 tests (every training row with the
      readout's case 2, trivial chunks included, both ``masked_res`` rows); the existing module fails
      too (20 tests: the goldens have the readout's case 2 with mult = 10).
  (e) ``res_bwd`` case 1 sums chunk 0 only: ``test_envelope_row_loss_and_gradients[d8_res21]``, both
      ``test_masked_models_with_chunked_residuals`` rows; the existing module passes.
  (f) the bias line of the slab update skipped for j >= nth: the training rows ``w400``, ``w1024``,
      ``w1024_h228``, ``none_h628``, ``empty-w400`` and ``test_slab_byte_budget``; the existing module
      fails ``test_widths_the_goldens_do_not_have[w1024]``.
"""
import copy

import numpy as np
import pytest
import torch

import f64_envelope as fe
import hip_util
import test_hip_generic_envelope as env
from njode_amd import _lib
from test_hip_f64_route import _bits, _init_sd, check_predict, check_train, fwd64, model64

pytestmark = pytest.mark.gpu

ENV_ROWS = [r for r in env.ROWS if r not in fe.REFUSED_ROWS]
CASES = fe.case_table()


def c_hT_of(B, H, scale=0.05):
    """A fixed, non-trivial upstream gradient of hT."""
    return scale * torch.cos(torch.arange(B * H, dtype=torch.float32)).view(B, H)


def _case(name):
    cfg, make = CASES[name]
    b, dt, T, until = make()
    lab = fe.case_labels(cfg, fe.call_sizes(b, dt, T, until))
    return cfg, b, dt, T, until, lab


def _train(name, cfg, sd, b, dt, T, until):
    kw = {'until_T': True} if until else {}
    check_train(name + '/train', cfg, sd, b, dt, T, c_hT=c_hT_of(b['start_X'].shape[0], cfg['hidden_size']), **kw)


# ---- the envelope's rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize('row', ENV_ROWS)
def test_envelope_row_loss_and_gradients(row):
    """Loss, hT and every gradient tensor of loss + (c_hT hT).sum().  ``deep_mixed`` has ``bias=False``:
    only the slots that hold a parameter are compared (the gradients are taken per named parameter)."""
    cfg, b, dt, T, until, lab = _case('env/' + row)
    if 'do_ne_d' in lab:       # no loss to train on: the library says so
        m = model64(cfg, env.state_dict(row))
        with pytest.raises(_lib.NjodeError, match='get_loss needs input_size == output_size'):
            fwd64(m, b, dt, T)
        return
    _train('env/' + row, cfg, env.state_dict(row), b, dt, T, until)


@pytest.mark.parametrize('row', ENV_ROWS)
def test_envelope_row_paths(row):
    cfg, b, dt, T, until, lab = _case('env/' + row)
    check_predict('env/{}/path'.format(row), cfg, env.state_dict(row), b, dt, T, get_loss='do_ne_d' not in lab)


@pytest.mark.parametrize('edge,row', fe.EDGES)
def test_envelope_edges(edge, row):
    """One path; a path without observations and an ``until_T`` tail; K = 4 097."""
    name = 'env/{}/{}'.format(row, edge)
    cfg, b, dt, T, until, lab = _case(name)
    B, _, _, K = fe.call_sizes(b, dt, T, until)
    assert {'b1': B == 1 and 'b1' in lab, 'empty': until and int((b['n_obs_ot'] == 0).sum()) == 1,
            'longK': K == 4097}[edge]
    _train(name, cfg, env.state_dict(row), b, dt, T, until)
    if edge != 'longK':
        check_predict(name + '/path', cfg, env.state_dict(row), b, dt, T)


@pytest.mark.parametrize('row', fe.REFUSED_ROWS)
def test_use_rnn_rows_are_refused_at_construction(row):
    from njode_amd.float64 import NJODE64
    with pytest.raises(NotImplementedError, match='use_rnn: the GRU jump has no float64 kernels'):
        NJODE64(**env.ROWS[row][0])


def test_absent_bias_slots_stay_zero():
    """``bias=False``: the flat vector keeps a slot per bias; nothing writes them -- not the backward,
    not an optimizer step -- while every present parameter moves."""
    cfg, b, dt, T, until, lab = _case('env/deep_mixed')
    assert 'no_bias' in lab
    m = model64(cfg, env.state_dict('deep_mixed'))
    flat = m.flat_parameters()
    present = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
    for off, n, _ in m._param_slices:
        present[off:off + n] = True
    n_absent = int((~present).sum())
    assert n_absent == fe.restate_cfg(cfg)[1]['P'] - sum(p.numel() for p in m.parameters()) > 0
    assert torch.count_nonzero(flat[~present]) == 0
    before = flat.clone()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    hT, loss = fwd64(m, b, dt, T)
    (loss + hT.sum()).backward()
    opt.step()
    assert m.flat_parameters() is flat and m._views_in_place()
    assert torch.count_nonzero(flat[~present]) == 0
    # (the width-1 relu of this row's ODE network is dead at these weights and nothing behind it has a
    # bias: that network's gradients are exactly zero -- ``deep8_live`` is the row with a live one)
    moved = {k: bool((p.grad != 0).any()) for k, p in m.named_parameters()}
    assert all(v for k, v in moved.items() if not k.startswith('ode_f')), moved
    assert bool((flat[present] != before[present]).any())


def test_depth_8_0_3_without_bias_and_a_live_ode_network():
    """Nine ODE layers of mixed widths whose gradients are all non-zero, next to depth 0 and depth 3."""
    cfg, b, dt, T, until, lab = _case('deep8_live')
    assert {'no_bias', 'depth_0', 'depth_8', 'depth_mixed', 'input_current_t', 'loss_easy', 'row_exact',
            'idle_row_groups'} <= lab
    sd = _init_sd(cfg, 6)
    o64 = hip_util.oracle_truth(cfg, sd, b, dt, T, torch.float64)[1]
    assert len(o64) == 14 and all(np.abs(g).max() > 0 for g in o64.values())
    _train('deep8_live', cfg, sd, b, dt, T, until)
    check_predict('deep8_live/path', cfg, sd, b, dt, T)


@pytest.mark.parametrize('name', ['masked_res12', 'masked_res21'])
def test_masked_models_with_chunked_residuals(name):
    """The adjoint of the ENCODER's residual reaches a parameter only in a masked model (through
    ``Y_bj``); the masked rows of the envelope table have D = H.  Here D = 6 / H = 12 and D = 12 / H = 6:
    both residual cases with two chunks of six units, in the encoder and in the readout."""
    cfg, b, dt, T, until, lab = _case(name)
    assert ({'masked_enc_case_1_mult2+', 'dec_case_2_mult2+'} <= lab if name == 'masked_res12' else
            {'masked_enc_case_2_mult2+', 'dec_case_1_mult2+'} <= lab)
    assert float((1 - b['M']).sum()) > 0          # (some coordinate is not observed: Y_bj feeds the encoder)
    sd = _init_sd(cfg, 8)
    _train(name, cfg, sd, b, dt, T, until)
    check_predict(name + '/path', cfg, sd, b, dt, T)


# ---- slab count at both clamps, strided batch and table loops ----------------------------------------------
def test_max_slabs_unmasked():
    """B = 2 100 > 2 048 slabs: workgroups 0 - 51 of the sweep take two paths, the others one."""
    cfg, b, dt, T, until, lab = _case('slab/demo_b2100')
    assert {'S_max_slabs', 'S_uneven', 'loss_tree_strided'} <= lab
    sd = _init_sd(cfg, 1)
    c_hT = torch.randn(fe.BIG_B, cfg['hidden_size'], generator=torch.Generator().manual_seed(5))
    check_train('slab/demo_b2100/train', cfg, sd, b, dt, T, c_hT=c_hT)
    check_predict('slab/demo_b2100/path', cfg, sd, b, dt, T)


def test_max_slabs_masked():
    """... on a masked model: lamx, last_X and tau are re-seeded between the paths of one workgroup."""
    cfg, b, dt, T, until, lab = _case('slab/masked_b2100')
    assert {'S_max_slabs', 'S_uneven', 'loss_tree_strided', 'masked'} <= lab
    sd = env.state_dict(fe.MASKED_BIG[0])
    _train('slab/masked_b2100', cfg, sd, b, dt, T, until)
    check_predict('slab/masked_b2100/path', cfg, sd, b, dt, T)


def test_slab_byte_budget():
    """P = 7 373 333: 18 slabs of 59 MB for 20 paths, workgroups 0 and 1 take two paths."""
    cfg, b, dt, T, until, lab = _case('slab/budget')
    assert {'S_budget', 'S_uneven', 'units_loop', 'depth_8', 'row_strided'} <= lab
    model = fe.restate_cfg(cfg)[1]
    assert model['P'] == 7373333 and fe.slab_count(model, b['start_X'].shape[0]) == 18
    sd = _init_sd(cfg, 4)
    _train('slab/budget', cfg, sd, b, dt, T, until)
    check_predict('slab/budget/path', cfg, sd, b, dt, T)


def test_row_table_beyond_the_clear_grid():
    """250 observation times x 2 100 paths: ``k_rows_clear`` strides.  Loss, hT, gradients."""
    cfg, b, dt, T, until, lab = _case('slab/rows_clear')
    assert {'rows_clear_strided', 'S_max_slabs', 'loss_tree_strided'} <= lab
    _train('slab/rows_clear', cfg, _init_sd(cfg, 1), b, dt, T, until)


def test_no_observations_at_all():
    """n_obs = 0, n_times = 0: the loss is exactly 0; hT and the gradients of (c_hT hT).sum() through the
    until_T tail go against the oracle; a path call."""
    cfg, b, dt, T, until, lab = _case('no_rows')
    assert 'no_rows' in lab and until and fe.call_sizes(b, dt, T, until) == (6, 0, 0, 4)
    sd = _init_sd(cfg, 1)
    m = model64(cfg, sd)
    hT, loss = fwd64(m, b, dt, T, until_T=True)
    assert float(loss.detach()) == 0.0
    _train('no_rows', cfg, sd, b, dt, T, until)
    check_predict('no_rows/path', cfg, sd, b, dt, T)


# ---- independence from the batch at S < B ------------------------------------------------------------
@pytest.mark.parametrize('name', ['slab/rows_clear', 'slab/masked_b2100'])
def test_paths_do_not_depend_on_a_large_batch(name):
    """Paths 0 - 3 alone (same times, slices left empty) and inside the 2 100-path batch: bit-equal hT and
    path rows, where the loss tree and (demo shape) the row table stride."""
    cfg, b, dt, T, until, lab = _case(name)
    assert 'loss_tree_strided' in lab and ('masked' in lab or 'rows_clear_strided' in lab)
    keep = b['obs_idx'] < 4
    slice_of = np.repeat(np.arange(len(b['times'])), np.diff(b['time_ptr']))
    counts = np.bincount(slice_of[keep.numpy()], minlength=len(b['times']))
    small = dict(b, X=b['X'][keep], obs_idx=b['obs_idx'][keep], start_X=b['start_X'][:4],
                 n_obs_ot=b['n_obs_ot'][:4], time_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    if 'M' in b:
        small['M'] = b['M'][keep]
    m = model64(cfg, _init_sd(cfg, 1), train=False)
    with torch.no_grad():
        big = fwd64(m, b, dt, T, return_path=True, until_T=True, get_loss=True)
        sml = fwd64(m, small, dt, T, return_path=True, until_T=True, get_loss=True)
    assert big[3].shape[1] == fe.BIG_B and sml[3].shape[1] == 4
    assert torch.equal(_bits(big[0][:4]), _bits(sml[0]))
    assert torch.equal(_bits(big[3][:, :4]), _bits(sml[3]))
    assert torch.equal(_bits(big[4][:, :4]), _bits(sml[4]))


# ---- the Python surface ------------------------------------------------------------------------------
def _small():
    cfg = hip_util.demo_cfg()
    b, meta = hip_util.bs_batch(12, seed=4, obs_perc=0.2, nb_steps=30)
    return cfg, _init_sd(cfg, 1), b, meta['dt'], meta['maturity']


def _args(b, dt, T):
    d = hip_util.to_dev(b)
    return (d['times'], d['time_ptr'], d['X'], d['obs_idx'], dt, T, d['start_X'])


def test_get_pred_is_the_path_call():
    cfg, sd, b, dt, T = _small()
    m = model64(cfg, sd)
    pred = m.get_pred(*_args(b, dt, T))
    assert not m.training
    with torch.no_grad():
        _, _, path_t, _, path_y = fwd64(m, b, dt, T, return_path=True, get_loss=False, until_T=True)
    assert pred['pred'].is_cuda and torch.equal(_bits(pred['pred']), _bits(path_y))
    assert np.array_equal(pred['pred_t'], path_t)


def test_host_outputs_carry_the_same_bits():
    """``device_outputs=False``: loss and pred arrive on the CPU, the bits of the device ones."""
    from njode_amd.float64 import NJODE64
    cfg, sd, b, dt, T = _small()
    dev = model64(cfg, sd, train=False)
    host = NJODE64(**dict(cfg, options=dict(cfg['options'], device_outputs=False)))
    host.load_state_dict({k: v.double() for k, v in sd.items()})
    host = host.cuda().eval()
    with torch.no_grad():
        hT_d, loss_d = fwd64(dev, b, dt, T)
        hT_h, loss_h = fwd64(host, b, dt, T)
    assert loss_d.is_cuda and not loss_h.is_cuda and hT_h.is_cuda
    assert torch.equal(_bits(loss_h), _bits(loss_d.cpu())) and torch.equal(_bits(hT_h), _bits(hT_d))
    p_d, p_h = dev.get_pred(*_args(b, dt, T)), host.get_pred(*_args(b, dt, T))
    assert p_d['pred'].is_cuda and not p_h['pred'].is_cuda
    assert torch.equal(_bits(p_h['pred']), _bits(p_d['pred'].cpu())) and np.array_equal(p_h['pred_t'], p_d['pred_t'])


@pytest.mark.parametrize('train', [True, False])
def test_float64_of_a_device_model(train):
    """``hip_model(...).float64()``: on the model's device, in its mode, the fp32 parameters widened."""
    from njode_amd.float64 import NJODE64
    cfg, sd, b, dt, T = _small()
    ref = hip_util.hip_model(cfg, sd).train(train)
    twin = ref.float64()
    assert isinstance(twin, NJODE64) and twin.training == train and twin.device_outputs
    assert twin.flat_parameters().device == next(ref.parameters()).device and twin.flat_parameters().is_cuda
    assert twin._views_in_place()
    for (k, p), (k2, q) in zip(ref.named_parameters(), twin.named_parameters()):
        assert k == k2 and q.dtype == torch.float64 and q.device == p.device
        assert torch.equal(q, p.detach().double())
    want = model64(cfg, sd, train=train)
    with torch.no_grad():
        a, c = fwd64(twin, b, dt, T), fwd64(want, b, dt, T)
    assert torch.equal(_bits(a[0]), _bits(c[0])) and torch.equal(_bits(a[1]), _bits(c[1]))


def test_deep_copy_gives_the_same_bits_and_trains_alone():
    cfg, sd, b, dt, T = _small()
    twin = hip_util.hip_model(cfg, sd).train().float64()
    other = copy.deepcopy(twin)
    assert other._views_in_place() and other.flat_parameters().data_ptr() != twin.flat_parameters().data_ptr()
    res = []
    for m in (twin, other):
        hT, loss = fwd64(m, b, dt, T)
        (loss + hT.sum()).backward()
        res.append([hT, loss] + [p.grad for p in m.parameters()])
    for a, c in zip(*res):
        assert torch.equal(_bits(a), _bits(c))
    before = twin.flat_parameters().clone()
    opt = torch.optim.SGD(other.parameters(), lr=0.05)
    opt.step()
    assert torch.equal(_bits(twin.flat_parameters()), _bits(before))
    assert other._views_in_place() and bool((other.flat_parameters() != before).any())
    # the copy trains: the step along its own gradient lowers its loss, the original's stays
    with torch.no_grad():
        _, l_copy = fwd64(other, b, dt, T)
        _, l_orig = fwd64(twin, b, dt, T)
    assert torch.equal(_bits(l_orig), _bits(res[0][1])) and float(l_copy) != float(l_orig)
