"""Usage patterns of the ``model(...)`` / ``loss.backward()`` / ``torch.optim`` route, written ONCE and
run on two backends: the CPU oracle under ordinary ``torch.autograd`` (fp32 and float64) and the HIP
model.  A plain module: no fixtures, no pytest settings.

A scenario is a short function ``fn(m, A, B)`` over an abstract model ``m`` and two batches (dicts of
tensors; every run receives fresh clones, so a scenario may write into them).  ``m(batch)`` returns
``(hT, loss)``; ``m.params`` maps the state_dict names to the leaf tensors; everything else a scenario
may touch is a method of ``Backend`` below.  The statements of a scenario are the same on both backends;
the expected outcome is never written down: it is whatever the oracle does under those statements --
the observations it returns (``Backend.observe``: loss, hT and the ``.grad`` of every tensor at that
moment), or that it raises ``RuntimeError``.

Operations that only exist in this project (a non-default stream, a prefetched plan, the workspace
pool, ``FusedAdam``, the flat parameter vector) are methods whose oracle version is the nearest plain
statement: no-ops, or, for the raw parameter writes, the ``torch.optim.Adam`` step they stand for.

``tests/test_autograd_scenarios_host.py`` runs the table on the oracle alone (no GPU),
``tests/test_hip_autograd_contract.py`` runs it on the HIP model against the oracle.
"""
import contextlib
import threading

import numpy as np
import torch

from oracle import dropout_oracle as do
from oracle import njode_oracle

P_DROP = 0.1


def _np(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def c_hT(B, H):
    """the weight of hT in an objective that reaches it: no power of two, both signs"""
    return (0.37 * np.cos(np.arange(B * H, dtype=np.float64) * 0.7)).reshape(B, H).astype(np.float32)


class Backend:
    """What a scenario may do to a model besides calling it.  The defaults are the oracle's."""
    params = None

    # -- settings a call captures (train/eval, loss weight, dropout rate, data-parallel shard, step counter)
    def set(self, **kw):
        raise NotImplementedError

    def get(self, key):
        raise NotImplementedError

    def zero_grad(self, set_to_none=True):
        for p in self.params.values():
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def const(self, array):
        """``array`` as a tensor of the backend's dtype and device"""
        raise NotImplementedError

    def observe(self, loss=None, hT=None, flags=None):
        return {'loss': None if loss is None else float(loss.detach()), 'hT': _np(hT),
                'g': {k: _np(p.grad) for k, p in self.params.items()}, 'flags': dict(flags or {})}

    def values(self):
        return {k: p.detach().clone() for k, p in self.params.items()}

    # -- optimizers
    def adam(self):
        return torch.optim.Adam([p for p in self.params.values() if p.requires_grad], lr=1e-3)

    def sgd(self, lr=0.05):
        return torch.optim.SGD([p for p in self.params.values() if p.requires_grad], lr=lr)

    def write_params(self, kind):
        """'torch': a torch.optim.Adam step; 'fused' / 'flat_copy': the project's own parameter writers
        (FusedAdam.step, flat_parameters().copy_()), which the oracle stands in for with the Adam step."""
        self.adam().step()

    # -- project-only operations: nothing on the oracle
    def stream(self):
        return contextlib.nullcontext()

    def prefetch(self, batch):
        pass

    def pool_state(self):
        return None

    def mark(self):
        """called right before the statement that may raise"""

    def clone(self):
        raise NotImplementedError

    def in_thread(self, fn):
        err = []

        def run():
            try:
                fn()
            except BaseException as e:    # (re-raised in the caller's thread)
                err.append(e)
        t = threading.Thread(target=run)
        t.start()
        t.join()
        if err:
            raise err[0]


class OracleModel(Backend):
    """The CPU oracle as a stateful model: the settings are read at call time, as the HIP model's call
    object captures them.  ``stream``: the dropout word stream of the kernel family the HIP row runs
    (oracle/dropout_oracle.py), so that a dropout call draws the kernels' own masks."""

    def __init__(self, cfg, sd, dtype, stream='mc'):
        self.cfg, self.dtype, self.mask_stream = cfg, dtype, stream
        self.o = njode_oracle.make_oracle(cfg)
        self.params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
        self.s = dict(training=True, weight=float(cfg.get('weight', 0.5)),
                      dropout_rate=float(cfg.get('dropout_rate', 0.0)), dp_global_batch=None,
                      dp_path_offset=0, step_counter=0)
        self.dseed = int(cfg.get('options', {}).get('dropout_seed', 0))

    def set(self, **kw):
        assert set(kw) <= set(self.s), kw
        self.s.update(kw)

    def get(self, key):
        return self.s[key]

    def const(self, array):
        return torch.as_tensor(np.asarray(array)).to(self.dtype)

    def clone(self):
        new = OracleModel(self.cfg, {k: p.detach() for k, p in self.params.items()}, self.dtype, self.mask_stream)
        new.s = dict(self.s)
        return new

    def __call__(self, b):
        o, s = self.o, self.s
        o.training, o.weight, o.p_drop = s['training'], s['weight'], s['dropout_rate']
        o.masks = None
        if s['training'] and s['dropout_rate'] > 0:
            o.masks = do.KernelMasks(self.mask_stream, do.call_seed(self.dseed, s['step_counter']),
                                     s['dropout_rate'], gid0=s['dp_path_offset'])
        if s['training']:
            s['step_counter'] += 1
        hT, loss = o.forward(self.params, b['times'], b['time_ptr'], b['X'], b['obs_idx'], b['delta_t'], b['T'],
                             b['start_X'], b['n_obs_ot'], M=b.get('M'))
        if s['dp_global_batch']:
            loss = loss * (float(len(b['start_X'])) / float(s['dp_global_batch']))
        return hT, loss


def oracle_batch(b, dtype):
    """A fresh copy of CPU batch ``b`` for the oracle in ``dtype`` (the fp32 values, widened)."""
    out = {}
    for k, v in b.items():
        if torch.is_tensor(v):
            out[k] = v.to(dtype).clone() if v.is_floating_point() else v.clone()
        else:
            out[k] = v
    return out


# =====================================================================================================
# the scenarios
# =====================================================================================================
def sum2(m, A, B):
    hA, lA = m(A)
    hB, lB = m(B)
    (lA + 0.5 * lB).backward()
    return {'final': m.observe(lA, hA)}


def _interleave(m, A, B, fifo):
    m.set(dropout_rate=P_DROP, step_counter=7)
    hA, lA = m(A)
    hB, lB = m(B)
    first, second = (lA, lB) if fifo else (lB, lA)
    first.backward()
    o1 = m.observe(lA, hA)
    second.backward()
    return {'first': o1, 'final': m.observe(lB, hB)}


def interleave_fifo(m, A, B):
    return _interleave(m, A, B, True)


def interleave_lifo(m, A, B):
    return _interleave(m, A, B, False)


def accumulate(m, A, B):
    for b in (A, B):
        h, l = m(b)
        l.backward()
    two = m.observe(l, h)
    m.zero_grad(set_to_none=False)
    h, l = m(A)
    l.backward()
    return {'two': two, 'final': m.observe(l, h)}


def _frozen(m, A, frozen):
    for k, p in m.params.items():
        if frozen(k):
            p.requires_grad_(False)
    h, l = m(A)
    no_graph = l.grad_fn is None
    state = m.pool_state()
    if not no_graph:
        l.backward()
    return {'final': m.observe(l, h, flags={'no_graph': no_graph, 'ws_in_use': None if state is None else state[2]})}


def frozen_readout(m, A, B):
    return _frozen(m, A, lambda k: k.startswith('readout_map.'))


def frozen_all_but_ode(m, A, B):
    return _frozen(m, A, lambda k: not k.startswith('ode_f.'))


def frozen_all(m, A, B):
    return _frozen(m, A, lambda k: True)


def grad_subset(m, A, B):
    names = sorted(m.params)
    names = [names[0], names[-1]]
    h, l = m(A)
    gs = torch.autograd.grad(l, [m.params[n] for n in names])
    obs = m.observe(l, h)
    assert all(g is None for g in obs['g'].values()), 'torch.autograd.grad must not write .grad'
    obs['g'].update({n: _np(g) for n, g in zip(names, gs)})
    return {'final': obs}


def upstream(m, A, B):
    h, l = m(A)
    c = m.const(c_hT(*h.shape))
    (l ** 2 + (c * h).sum()).backward()
    o = m.observe(l, h)
    m.zero_grad()
    h, l = m(A)
    (l * 0).backward()
    return {'zero': m.observe(l, h), 'final': o}


def out_inplace(m, A, B):
    h, l = m(A)
    c = m.const(c_hT(*h.shape))
    l += 1
    l *= 2
    h += 1
    (l + (c * h).sum()).backward()
    return {'final': m.observe(l, h)}


def state_change(m, A, B):
    m.set(training=True, weight=0.7, dropout_rate=P_DROP, dp_path_offset=3, step_counter=11)
    h, l = m(A)
    m.set(training=False, weight=0.9, dropout_rate=0.4, dp_global_batch=1000, dp_path_offset=77,
          step_counter=m.get('step_counter') + 5)
    l.backward()
    return {'final': m.observe(l, h)}


def _param_step(m, A, B, kind):
    hA, lA = m(A)
    hB, lB = m(B)
    lA.backward()
    m.write_params(kind)
    m.mark()
    lB.backward()
    return {'final': m.observe(lB, hB)}


def param_step_torch(m, A, B):
    return _param_step(m, A, B, 'torch')


def param_step_fused(m, A, B):
    return _param_step(m, A, B, 'fused')


def param_flat_copy(m, A, B):
    return _param_step(m, A, B, 'flat_copy')


def _input_inplace(m, A, name):
    h, l = m(A)
    t = A[name]
    if name == 'n_obs_ot':
        t.add_(1)
    elif name == 'obs_idx':
        # (+ 1, folded back into [0, B): no backend is ever handed an index outside the batch)
        t.add_(1).remainder_(len(A['start_X']))
    else:
        t.mul_(2)
    m.mark()
    l.backward()
    return {'final': m.observe(l, h)}


def input_inplace_X(m, A, B):
    return _input_inplace(m, A, 'X')


def input_inplace_start_X(m, A, B):
    return _input_inplace(m, A, 'start_X')


def input_inplace_M(m, A, B):
    if 'M' not in A:      # an unmasked model takes no M: the scenario is the plain step
        A = dict(A, M=m.const(np.zeros(1, dtype=np.float32)))
    return _input_inplace(m, A, 'M')


def input_inplace_obs_idx(m, A, B):
    return _input_inplace(m, A, 'obs_idx')


def input_inplace_n_obs_ot(m, A, B):
    return _input_inplace(m, A, 'n_obs_ot')


N_DROPPED = 40


def dropped_graph(m, A, B):
    out = s2 = None
    for i in range(N_DROPPED):
        out = m(A)       # under grad, never back-propagated
        if i == 1:
            s2 = m.pool_state()
    s40 = m.pool_state()
    assert s40 == s2, ('the workspace pool or the device memory in use grew', s2, s40)
    del out
    h, l = m(A)
    l.backward()
    return {'final': m.observe(l, h)}


def side_stream(m, A, B):
    h, l = m(A)
    l.backward()
    o0 = m.observe(l, h)
    m.zero_grad()
    with m.stream():
        h, l = m(A)
        l.backward()
    o1 = m.observe(l, h)
    assert o0['loss'] == o1['loss'] and np.array_equal(o0['hT'], o1['hT'])
    for k in o0['g']:
        assert np.array_equal(o0['g'][k], o1['g'][k]), ('side stream: other bits', k)
    return {'final': o1}


def deepcopy(m, A, B):
    h, l = m(A)
    l.backward()
    m.sgd().step()
    m.zero_grad()
    m2 = m.clone()
    h, l = m(A)
    l.backward()
    o = m.observe(l, h)
    h2, l2 = m2(A)
    l2.backward()
    o2 = m2.observe(l2, h2)
    before, before2 = m.values(), m2.values()
    m2.sgd().step()
    after, after2 = m.values(), m2.values()
    for k in before:
        assert torch.equal(before[k], after[k]), ('stepping the copy moved the original', k)
    assert any(not torch.equal(before2[k], after2[k]) for k in before2), 'the copy did not step'
    return {'copy': o2, 'final': o}


def worker_thread_deferred(m, A, B):
    hA, lA = m(A)
    c = m.const(c_hT(*hA.shape))
    m.prefetch(B)        # (pending: the next forward call carries it)
    m.in_thread(lambda: (lA + (c * hA).sum()).backward())
    o1 = m.observe(lA, hA)
    hB, lB = m(B)
    lB.backward()
    return {'first': o1, 'final': m.observe(lB, hB)}


SCENARIOS = {fn.__name__: fn for fn in (
    sum2, interleave_fifo, interleave_lifo, accumulate, frozen_readout, frozen_all_but_ode, frozen_all,
    grad_subset, upstream, out_inplace, state_change, param_step_torch, param_step_fused, param_flat_copy,
    input_inplace_X, input_inplace_start_X, input_inplace_M, input_inplace_obs_idx, input_inplace_n_obs_ot,
    dropped_graph, side_stream, deepcopy, worker_thread_deferred)}


def run(fn, m, A, B):
    """('ok', observations) or ('raises', message): the outcome of a scenario on one backend."""
    try:
        return 'ok', fn(m, A, B)
    except RuntimeError as e:
        return 'raises', str(e)


@contextlib.contextmanager
def one_thread():
    """the oracle's tensors are a few paths wide: a pool of threads only synchronises (and its
    reductions give other bits than one thread's); restored afterwards"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


def run_on_oracle(name, cfg, sd, A, B, stream='mc'):
    """((outcome, observations) in fp32, the same in float64) of scenario ``name`` on the oracle."""
    with one_thread():
        return tuple(run(SCENARIOS[name], OracleModel(cfg, sd, dt, stream), oracle_batch(A, dt), oracle_batch(B, dt))
                     for dt in (torch.float32, torch.float64))


# =====================================================================================================
# the model rows: the smallest batches that still take distinct kernel routes
# =====================================================================================================
def _w(n, act='tanh', layers=2):
    return tuple((n, act) for _ in range(layers))


def _with_grid(b, dt, T):
    out = {k: v for k, v in b.items() if k not in ('true_paths', 'observed_dates')}
    out.update(delta_t=dt, T=T)
    return out


def _state_dict(cfg, seed=0):
    from njode_amd import models
    torch.manual_seed(seed)
    return {k: v.detach().clone() for k, v in models.NJODE(**cfg).state_dict().items()}


def model_rows(small=False):
    """name -> dict(cfg, sd, A, B, stream): the four models of the GPU half and their batches (CPU
    tensors).  ``small``: the host half's sizes (same shapes, fewer paths and steps)."""
    import test_hip_generic_envelope as GE
    import test_hip_route_matrix as RM
    from hip_util import exact_k_batch
    from njode_amd import synthetic_physionet
    from njode_amd.build import CONFIGS

    def physio(B, seed):
        b = synthetic_physionet.make_batch(batch_size=B, n_grid=20 if small else 60,
                                           n_obs_range=(2, 4) if small else (3, 9), seed=seed)
        return _with_grid(b, b['delta_t'], b['T'])

    rows = {}
    cfg = RM.model_cfg(CONFIGS[0])
    rows['demo'] = dict(cfg=cfg, stream='mc',
                        A=_with_grid(*(exact_k_batch(6, 20, 3) if small else exact_k_batch(24, 100, 4))),
                        B=_with_grid(*(exact_k_batch(5, 20, 3, seed=5) if small else exact_k_batch(17, 100, 4, seed=5))))
    chain = next(c for c in CONFIGS if RM.caps(c)['HAS_CHAIN'])
    rows['masked'] = dict(cfg=RM.model_cfg(chain), stream='mc', A=physio(5 if small else 19, 3),
                          B=physio(4 if small else 11, 4))
    if not small:
        gru = next(c for c in CONFIGS if c[9])
        A = _with_grid(*exact_k_batch(17, 60))
        rows['gru'] = dict(cfg=RM.model_cfg(gru), stream='valu', A=A, B=A)
        A = _with_grid(*exact_k_batch(17, 50))
        rows['generic'] = dict(cfg=GE._cfg(1, 10, _w(100), _w(100), _w(100)), stream='gen', A=A, B=A)
    for r in rows.values():
        r['sd'] = _state_dict(r['cfg'])
    return rows
