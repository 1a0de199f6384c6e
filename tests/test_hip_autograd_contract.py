"""The ``model(...)`` / ``loss.backward()`` / ``torch.optim`` route held to plain autograd's contract.

Every scenario of tests/autograd_scenarios.py runs, statement for statement, on the CPU oracle under
ordinary ``torch.autograd`` (fp32 and float64) and on the HIP model, on four models that take distinct
kernel routes (confirmed by kernel names, ``test_rows_take_their_routes``):

    demo      CONFIGS[0]: segment plan, wave per item      A = exact_k_batch(24, 100, 4), B = (17, 100, 4)
    masked    first HAS_CHAIN shape: lockstep, wave/path   A, B = synthetic_physionet batches of 19 / 11 paths
    gru       the compiled use_rnn shape                   A = exact_k_batch(17, 60)
    generic   width 100 three times: shape-generic kernels A = exact_k_batch(17, 50)

the demo and masked rows also through the ``torch.library`` operator (``options['torch_library_op']``).

Where the oracle returns observations (loss, hT, the ``.grad`` of every tensor at some moment), the HIP
model's are held to ``hip_util.check_vs_oracle``: err(HIP, f64) <= max(2 err(oracle fp32, f64), floor)
with the default floors, never looser than GRAD_REL_L2 / LOSS_RTOL; a ``.grad`` that is None on the oracle
is None here.  Where the oracle raises ``RuntimeError`` the HIP route raises ``RuntimeError``, the raising
backward creates or changes no ``.grad``, no workspace slot stays taken, and an ordinary step on the same
model afterwards passes the gradient rule against the oracle at the model's current parameters.

``input_inplace_*``: the HIP route RAISES for all five tensors whenever the call kept the caller's own
tensor (fp32 / int32, contiguous, on the device -- as every batch of this module is): its backward reads
the batch again, and a version counter is the only host-side evidence there is.  (Plain autograd raises
for ``M`` and ``obs_idx`` only and uses the forward-time values of the others; a batch the call had to
convert is a private copy, and the backward then returns the forward-time gradient.)

On the parent commit (first GPU run of this module; the readings were made from the code): a parameter
step between forward and backward -- torch.optim.Adam, FusedAdam, flat_parameters().copy_() -- was
silently accepted on all six rows (gradient of old activations and new weights); a changed batch reached
the backward kernels (X on every specialised route, start_X on demo and gru, n_obs_ot on masked, gru and
demo_op, M on masked; the shape-generic kernels read none of them again); ``loss += 1`` / ``hT += 1``
raised on the autograd.Function route and worked through the operator; ``copy.deepcopy(model)`` failed
("cannot pickle 'Event' object"); every other scenario already passed (93 of 135 cases).

Worst measured err(HIP, f64) / err(o32, f64) per scenario and row (MI355X; every case passes on the
default floors, a ratio above 2 passes on the floor where both errors are at fp32 rounding; "+step" is
the ordinary step after a raise; the raising scenarios have no other number):

    scenario                     demo  demo_op  masked  masked_op   gru  generic
    sum2                         1.00     1.00    1.28       1.28  2.04     1.61
    interleave_fifo              2.19     2.19    1.74       1.74  2.02     1.40
    interleave_lifo              1.47     1.47    1.74       1.74  3.80     1.40
    accumulate                   1.87     1.87    1.18       1.18  2.04     1.61
    frozen_readout               1.87     1.87    1.18       1.18  2.04     1.61
    frozen_all_but_ode           1.87     1.87    1.16       1.16  2.04     1.61
    frozen_all                   1.00     1.00    0.90       0.90  2.04     1.00
    grad_subset                  1.00     1.00    1.07       1.07  2.04     1.00
    upstream                     3.13     3.13    1.41       1.41  2.04     1.12
    out_inplace                  2.33     2.33    1.48       1.48  1.72     1.65
    state_change                 1.31     1.31    1.38       1.38  3.14     1.30
    param_step_torch +step       7.59     7.59    0.93       0.93  2.43     1.74
    param_step_fused +step       1.87     1.87    1.18       1.18  2.04     1.61
    param_flat_copy +step        2.28     2.28    2.23       2.23  1.77     2.47
    input_inplace_X +step        1.87     1.87    1.18       1.18  2.04     1.61
    input_inplace_start_X +step  1.87     1.87    1.18       1.18  2.04     1.61
    input_inplace_M (+step)      1.87     1.87    1.18       1.18  2.04     1.61
    input_inplace_obs_idx +step  1.87     1.87    1.18       1.18  2.04     1.61
    input_inplace_n_obs_ot +step 1.87     1.87    1.18       1.18  2.04     1.61
    dropped_graph                1.87     1.87    1.18       1.18  2.04     1.61
    side_stream                  1.87     1.87    1.18       1.18  2.04     1.61
    deepcopy                     1.41     1.41    1.37       1.37  2.65     1.00
    worker_thread_deferred       2.51     2.51    1.48       1.48  2.04     1.60

(7.59: readout_map.ffnn.6.bias of the step after the Adam update, 3.75e-07 against 4.94e-08 relative
L2, both far under the 1e-5 floor.)  The module takes about 26 s, of which the oracle about 20.
"""
import contextlib
import copy

import numpy as np
import pytest
import torch

import autograd_scenarios as S
import hip_util
import test_hip_generic_envelope as GE
import test_hip_route_matrix as RM
from hip_util import hip_model, kernel_names, oracle_pair

pytestmark = pytest.mark.gpu

# row -> (model of autograd_scenarios.model_rows, through the torch.library operator?)
ROWS = {'demo': ('demo', False), 'demo_op': ('demo', True), 'masked': ('masked', False),
        'masked_op': ('masked', True), 'gru': ('gru', False), 'generic': ('generic', False)}

_MODELS = {}
_EXPECTED = {}
RATIOS = {}


def models():
    if not _MODELS:
        _MODELS.update(S.model_rows())
    return _MODELS


def expected(model, name):
    """the oracle's outcome of a scenario, (fp32, float64): computed once per model"""
    if (model, name) not in _EXPECTED:
        r = models()[model]
        _EXPECTED[model, name] = S.run_on_oracle(name, r['cfg'], r['sd'], r['A'], r['B'], r['stream'])
    return _EXPECTED[model, name]


def dev_batch(b):
    """A fresh device copy of CPU batch ``b`` in the types the library reads, so that the call keeps these
    very tensors (``times`` / ``time_ptr`` stay the batch's own objects: a prefetched plan is found by them)."""
    out = dict(b)
    for k in ('X', 'start_X', 'M'):
        if k in b:
            out[k] = b[k].to('cuda', torch.float32).clone()
    for k in ('obs_idx', 'n_obs_ot'):
        out[k] = b[k].to('cuda', torch.int32).clone()
    return out


class HipModel(S.Backend):
    SETTINGS = {'weight': 'weight', 'dropout_rate': 'dropout_rate', 'dp_global_batch': 'dp_global_batch',
                'dp_path_offset': 'dp_path_offset', 'step_counter': '_step_counter'}

    def __init__(self, m):
        self.m = m
        self.params = dict(m.named_parameters())
        self.marked = None

    @classmethod
    def make(cls, cfg, sd, use_op):
        cfg = copy.deepcopy(cfg)
        cfg['options'] = dict(cfg.get('options', {}), torch_library_op=use_op)
        return cls(hip_model(cfg, sd).train())

    def set(self, **kw):
        for k, v in kw.items():
            if k == 'training':
                self.m.train(v)
            else:
                setattr(self.m, self.SETTINGS[k], v)

    def get(self, key):
        return self.m.training if key == 'training' else getattr(self.m, self.SETTINGS[key])

    def const(self, array):
        return torch.as_tensor(np.asarray(array), dtype=torch.float32).cuda()

    def __call__(self, b):
        return self.m(b['times'], b['time_ptr'], b['X'], b['obs_idx'], b['delta_t'], b['T'], b['start_X'],
                      b['n_obs_ot'], M=b.get('M'))

    def write_params(self, kind):
        from njode_amd import models as nm
        if kind == 'torch':
            self.adam().step()
        elif kind == 'fused':
            nm.FusedAdam(self.m, lr=1e-3).step()
        else:
            flat = self.m.flat_parameters()
            with torch.no_grad():
                flat.copy_(flat * 1.01)

    @contextlib.contextmanager
    def stream(self):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            yield
        torch.cuda.current_stream().wait_stream(s)

    def prefetch(self, b):
        self.m.prefetch_plan(b['times'], b['time_ptr'], b['X'], b['obs_idx'], b['delta_t'], b['T'], b['start_X'],
                             b['n_obs_ot'], M=b.get('M'))

    def pool_state(self):
        torch.cuda.synchronize()
        return (len(self.m._ws_pool), torch.cuda.memory_allocated(), sum(1 for s in self.m._ws_pool if s[1]))

    def grads(self):
        return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in self.params.items()}

    def mark(self):
        self.marked = self.grads()

    def clone(self):
        return HipModel(copy.deepcopy(self.m))


def check_obs(tag, family, got, o32, o64):
    """one observation of the HIP model against the oracle's: None-ness exactly, numbers by the rule"""
    assert got['flags'].get('no_graph') == o64['flags'].get('no_graph'), (tag, got['flags'], o64['flags'])
    if got['flags'].get('no_graph'):
        assert got['flags']['ws_in_use'] == 0, (tag, 'a call without a graph kept its workspace')
    for k, g in o64['g'].items():
        assert (got['g'][k] is None) == (g is None), (tag, k, 'grad is None:', got['g'][k] is None, 'oracle:', g is None)
    live = [k for k, g in o64['g'].items() if g is not None]
    res = {'loss_auto': got['loss'], 'hT': got['hT']}
    res.update({'g.' + k: got['g'][k] for k in live})
    a = dict(o32, g={k: o32['g'][k] for k in live})
    b = dict(o64, g={k: o64['g'][k] for k in live})
    _ruled(tag, family, a, b, res)


def _ruled(tag, family, o32, o64, res):
    """hip_util.check_vs_oracle, its worst ratio recorded per (row, scenario)"""
    one = {}
    hip_util.check_vs_oracle(tag, o32, o64, res, one, 'x')
    key = (tag.split(' ')[0], family)
    RATIOS[key] = max(RATIOS.get(key, 0.0), one['x'])


def check_after_raise(tag, row, hm, msg):
    """the raising backward left nothing behind, and the model still steps correctly"""
    r = models()[ROWS[row][0]]
    assert hm.marked is not None, (tag, 'raised before the statement that was expected to', msg)
    assert 'modified by an inplace operation' in msg, (tag, msg)
    now = hm.grads()
    for k, g in hm.marked.items():
        assert (g is None) == (now[k] is None), (tag, k, 'the raising backward created or dropped a .grad')
        assert g is None or torch.equal(g, now[k]), (tag, k, 'the raising backward changed a .grad')
    assert not any(s[1] for s in hm.m._ws_pool), (tag, 'a workspace slot stayed taken after the raise')
    hm.zero_grad()
    h, l = hm(dev_batch(r['A']))
    l.backward()
    got = hm.observe(l, h)
    sd = {k: v.detach().cpu().clone() for k, v in hm.m.state_dict().items()}
    b = r['A']
    o32, o64 = oracle_pair(r['cfg'], sd, {k: v for k, v in b.items() if k not in ('delta_t', 'T')}, b['delta_t'],
                           b['T'])
    res = {'loss_auto': got['loss'], 'hT': got['hT']}
    res.update({'g.' + k: g for k, g in got['g'].items()})
    _ruled(tag + ' (next step)', tag.split(' ')[1] + ' +step', o32, o64, res)


@pytest.mark.parametrize('name', list(S.SCENARIOS))
@pytest.mark.parametrize('row', list(ROWS))
def test_scenario(row, name):
    model, use_op = ROWS[row]
    r = models()[model]
    (k32, o32), (k64, o64) = expected(model, name)
    assert k32 == k64, (row, name, 'the oracle disagrees with itself', k32, k64)
    hm = HipModel.make(r['cfg'], r['sd'], use_op)
    kind, got = S.run(S.SCENARIOS[name], hm, dev_batch(r['A']), dev_batch(r['B']))
    torch.cuda.synchronize()
    tag = '{} {}'.format(row, name)
    if k64 == 'raises':
        assert kind == 'raises', (tag, 'plain autograd raises here:', o64[:120])
        check_after_raise(tag, row, hm, got)
    elif kind == 'raises':
        # only a changed batch tensor may raise where plain autograd goes ahead (module docstring)
        assert name.startswith('input_inplace_'), (tag, got)
        check_after_raise(tag, row, hm, got)
    else:
        assert got.keys() == o64.keys(), (tag, sorted(got), sorted(o64))
        for obs in o64:
            check_obs('{} [{}]'.format(tag, obs), name, got[obs], o32[obs], o64[obs])


def test_rows_take_their_routes():
    want = {'demo': (RM.ITEMS, RM.MIXED + RM.ONE_WAVE),
            'masked': (['k_paths_fwd_chain', 'k_paths_bwd_adj_chain'], ['k_paths_fwd_mfma']),
            'gru': (RM.GRU, RM.ITEMS + RM.MIXED)}
    for row, (model, use_op) in ROWS.items():
        r = models()[model]
        hm = HipModel.make(r['cfg'], r['sd'], use_op)
        A = dev_batch(r['A'])

        def step():
            h, l = hm(A)
            l.backward()
        _, names = kernel_names(step)
        if model == 'generic':
            GE._check_names(row, names, 'seg')
        else:
            RM.check_names(row, names, *want[model])


def test_changed_batch_that_the_call_had_to_copy_gives_the_forward_time_gradient():
    """A batch the call converts (float64 values, int64 indices on the host: the reference's own
    collate output) is a private copy: writing into the caller's tensors between forward and backward
    neither raises nor moves the gradient."""
    r = models()['demo']
    b = S.oracle_batch(r['A'], torch.float64)
    grads = []
    for touch in (False, True):
        hm = HipModel.make(r['cfg'], r['sd'], False)
        h, l = hm(dict(b, start_X=b['start_X'].cuda()))
        if touch:
            b['X'].mul_(2)
            b['obs_idx'].add_(1).remainder_(len(b['start_X']))
            b['n_obs_ot'].add_(1)
        l.backward()
        grads.append(hm.grads())
    for k, g in grads[0].items():
        assert torch.equal(g, grads[1][k]), k


def test_zz_report_worst_ratios():
    """prints the table of the module docstring (run with -s)"""
    names = sorted({k[1] for k in RATIOS})
    print('worst err(HIP, f64) / err(o32, f64)  ' + ' '.join('{:>9s}'.format(r) for r in ROWS))
    for n in names:
        print('RATIO {:30s} '.format(n) + ' '.join('{:9.2f}'.format(RATIOS.get((r, n), float('nan'))) for r in ROWS))
