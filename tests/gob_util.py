"""Shared helpers of the GRU-ODE-Bayes tests: the golden cases (tests/golden/gob_*.npz, written by
tests/golden/make_golden_gob.py from the reference's own class), the restatement's results in a
given dtype (computed once per case and dtype, shared, never modified), and the HIP model."""
import functools
import os

import numpy as np
import torch

import gob_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ('gob_d1_plain', 'gob_d1_impute', 'gob_clim_plain', 'gob_clim_impute')
SKIP = ('classification_model.', 'gru_obs.gru_debug.')


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
        return {k: z[k] for k in z.files}


def part(g, prefix):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def golden_batch(g):
    i = part(g, 'in.')
    return dict(times=i['times'].astype(np.float64), time_ptr=i['time_ptr'].astype(np.int64),
                X=torch.from_numpy(i['X']), M=torch.from_numpy(i['M']),
                obs_idx=torch.from_numpy(i['obs_idx']).long(), start_X=torch.from_numpy(i['start_X']),
                delta_t=float(i['delta_t']), T=float(i['T']))


def golden_cfg(g):
    c = {k: v.item() for k, v in part(g, 'cfg.').items()}
    return dict(input_size=int(c['input_size']), hidden_size=int(c['hidden_size']), p_hidden=int(c['p_hidden']),
                prep_hidden=int(c['prep_hidden']), cov_hidden=int(c['cov_hidden']), mixing=float(c['mixing']),
                impute=bool(c['impute']))


def model_kwargs(cfg, dropout_rate=0.0, bias=True, **options):
    """Constructor arguments of NNFOwithBayesianJumps (either implementation) for ``cfg``."""
    return dict(input_size=cfg['input_size'], hidden_size=cfg['hidden_size'], p_hidden=cfg['p_hidden'],
                prep_hidden=cfg['prep_hidden'], bias=bias, cov_size=cfg['input_size'],
                cov_hidden=cfg['cov_hidden'], logvar=True, mixing=cfg['mixing'], dropout_rate=dropout_rate,
                full_gru_ode=True, solver='euler', impute=cfg['impute'], **options)


def objective_of(objective, loss, loss_1, hT, c_hT):
    """The scalar a test differentiates: ``objective`` is 'loss', 'loss_1' or a pair (a, b) for
    a * loss + b * loss_1 (a term whose weight is 0 is left out of the graph); ``c_hT`` (a tensor like
    ``hT`` or None) adds <c_hT, hT>."""
    if isinstance(objective, str):
        terms = [{'loss': loss, 'loss_1': loss_1}[objective]]
    else:
        a, b = objective
        terms = ([a * loss] if a else []) + ([b * loss_1] if b else [])
    if c_hT is not None:
        terms.append((c_hT * hT).sum())
    assert terms, 'an objective of no terms'
    return sum(terms[1:], terms[0])


def restate(sd, b, mixing, dtype, grads=True, masks=None, c_hT=None, objective='loss', return_path=False,
            device=None):
    """The restatement in ``dtype``: dict of float64 numpy arrays hT, loss, loss_1[, path_p, path_h]
    and g (gradients of ``objective`` [+ <c_hT, hT>] per loss parameter; ``objective``: see
    ``objective_of``)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        p = gob_oracle.cast(sd, dtype, device=device, requires_grad=grads)
        cast = lambda t: t.to(dtype=dtype, device=device)
        with torch.set_grad_enabled(grads):
            out = gob_oracle.forward(p, b['times'], b['time_ptr'], cast(b['X']), cast(b['M']), b['obs_idx'],
                                     b['delta_t'], b['T'], cast(b['start_X']), mixing, masks=masks,
                                     return_path=return_path)
        res = {k: out[k].detach().cpu().numpy().astype(np.float64) for k in out if k != 'path_t'}
        if return_path:
            res['path_t'] = out['path_t']
        if grads:
            c = None if c_hT is None else torch.as_tensor(c_hT).to(dtype=dtype, device=device)
            obj = objective_of(objective, out['loss'], out['loss_1'], out['hT'], c)
            keys = gob_oracle.loss_keys(p)
            gs = torch.autograd.grad(obj, [p[k] for k in keys], allow_unused=True)
            res['g'] = {k: (np.zeros(tuple(p[k].shape)) if g is None else g.cpu().numpy().astype(np.float64))
                        for k, g in zip(keys, gs)}
    finally:
        torch.set_num_threads(threads)
    return res


def rel_l2(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-12))


def hip_model(cfg, sd=None, dropout_rate=0.0, bias=True, device='cuda', **options):
    from njode_amd import gru_ode_bayes
    options.setdefault('device_outputs', True)
    m = gru_ode_bayes.NNFOwithBayesianJumps(**model_kwargs(cfg, dropout_rate, bias, options=options))
    if sd is not None:
        m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    return m.to(device)


def hip_call(m, b, **kw):
    dev = next(m.parameters()).device
    return m(b['times'], b['time_ptr'], b['X'].to(dev), b['M'].to(dev), b['obs_idx'], b['delta_t'], b['T'],
             b['start_X'].to(dev), **kw)
