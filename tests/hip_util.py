"""Shared helpers of the GPU parity tests: build the HIP-backed model and the CPU
oracle from the same config / parameters and run both on the same batch."""
import copy

import numpy as np
import torch

from njode_amd import data_utils, models
from oracle import njode_oracle

NN50 = ((50, 'tanh'), (50, 'tanh'))
# fp32 tolerances of the HIP path vs the reference/oracle:
ATOL, RTOL = 1e-5, 1e-4        # hT, path_h, path_y at S = 100
RTOL_LONG = 1e-3               # ... at S = 3 000 (PhysioNet-shaped, masked)
LOSS_RTOL = 1e-4
GRAD_REL_L2 = 1e-3             # per-tensor relative L2 error of gradients


def demo_cfg(d=1, H=10, dropout=0.0, **options):
    return dict(input_size=d, hidden_size=H, output_size=d, ode_nn=NN50, readout_nn=NN50,
                enc_nn=NN50, use_rnn=False, bias=True, dropout_rate=dropout, options=options)


def hip_model(cfg, state_dict=None, device='cuda', device_outputs=True):
    cfg = copy.deepcopy(cfg)
    cfg.setdefault('options', {})
    cfg['options'] = dict(cfg['options'], device_outputs=device_outputs)
    m = models.NJODE(**cfg)
    if state_dict is not None:
        m.load_state_dict(state_dict)
    return m.to(device)


def to_dev(b, device='cuda'):
    out = dict(b)
    for k in ('X', 'start_X', 'n_obs_ot', 'M'):
        if k in out and out[k] is not None:
            out[k] = out[k].to(device)
    return out


def hip_forward(m, b, delta_t, T, **kw):
    d = to_dev(b)
    return m(d['times'], d['time_ptr'], d['X'], d['obs_idx'], delta_t, T, d['start_X'],
             d.get('n_obs_ot'), M=d.get('M'), **kw)


def oracle_forward(cfg, sd, b, delta_t, T, training=False, weight=None, grads=False, masks=None, **kw):
    o = njode_oracle.make_oracle(cfg)
    o.training = training
    o.masks = masks
    if weight is not None:
        o.weight = weight
    params = {k: v.clone().requires_grad_(grads) for k, v in sd.items()}
    out = o.forward(params, b['times'], b['time_ptr'], b['X'], b['obs_idx'], delta_t, T,
                    b['start_X'], b.get('n_obs_ot'), M=b.get('M'), **kw)
    return out, params


def rel_l2(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-12))


def bs_batch(n_paths, seed=0, name='BlackScholes', obs_perc=0.1, nb_steps=100):
    hp = copy.deepcopy(data_utils.hyperparam_default)
    hp.update(nb_paths=n_paths, obs_perc=obs_perc, nb_steps=nb_steps)
    paths, obs, nb_obs, meta = data_utils.create_dataset(name, hp, seed=seed)
    b = data_utils.collate_arrays(paths, obs, nb_obs, meta['dt'])
    return b, meta


def grads_by_name(m):
    return {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}


def exact_k_batch(n_paths, n_steps, obs_per_path=4, seed=0, d=1):
    """Demo-shaped unmasked batch whose segment-plan call takes EXACTLY ``n_steps`` Euler steps: the
    grid step is 2**-10, so every observation time k * dt is exact in float64 and the schedule walks
    full steps onto it; path 0 is observed at the last grid point (no tail).  Returns (batch, dt, T)."""
    rng = np.random.RandomState(seed)
    dt = 2.0 ** -10
    obs = np.zeros((n_paths, n_steps + 1), dtype=np.int64)
    for p in range(n_paths):
        obs[p, 1 + rng.choice(n_steps, size=min(obs_per_path, n_steps), replace=False)] = 1
    obs[0, n_steps] = 1
    paths = np.cumsum(rng.normal(0.0, 0.05, size=(n_paths, d, n_steps + 1)), axis=2) + 1.0
    b = data_utils.collate_arrays(paths, obs, obs[:, 1:].sum(axis=1), dt)
    return b, dt, n_steps * dt


def irregular_batch(b, dt, dt_factor=0.37):
    """(batch, delta_t): ``b`` (a collated batch of grid step ``dt``) made irregular, a pure function of
    its arguments.  Every row of one path -- not path 0, not a path of the last observed slice -- is
    removed (``n_obs_ot`` recounted, slices it leaves empty stay); a jump at t = 0.0 with one row for
    path 0 is put in front (no Euler step before it; kept if the batch already has it); a time without
    rows is inserted midway between two inner times; delta_t = dt_factor dt does not divide the grid,
    so every grid interval ends in a partial Euler step."""
    times = np.asarray(b['times'], dtype=np.float64)
    ptr = np.asarray(b['time_ptr'], dtype=np.int64)
    idx = b['obs_idx'].numpy()
    B, d = b['start_X'].shape[0], b['X'].shape[1]
    assert len(times) >= 3 and ptr[-1] == len(idx) > 0
    slice_of = np.repeat(np.arange(len(times)), np.diff(ptr))
    last = set(idx[slice_of == slice_of[-1]].tolist())
    seen = set(idx.tolist())
    victim = next(p for p in range(1, B) if p in seen and p not in last)
    keep = idx != victim
    idx2, sl2 = idx[keep], slice_of[keep]
    kt = torch.from_numpy(keep)
    X, M = b['X'][kt], (b['M'][kt] if 'M' in b else None)
    counts = np.bincount(sl2, minlength=len(times))
    # the t = 0 jump of path 0 (rows are sorted by time, then path: it is row 0)
    if times[0] != 0.0 or not (counts[0] and idx2[0] == 0):
        m0 = (torch.arange(d) % 3 == 0).to(X.dtype)
        x0 = 0.5 + 0.01 * torch.arange(d, dtype=X.dtype)
        if M is not None:
            x0, M = x0 * m0, torch.cat([m0[None], M])
        X, idx2 = torch.cat([x0[None], X]), np.concatenate([[0], idx2])
        if times[0] != 0.0:
            times, counts = np.concatenate([[0.0], times]), np.concatenate([[1], counts])
        else:
            counts[0] += 1
    # a time without rows, strictly inside the range and off the grid
    j = len(times) // 2
    times = np.insert(times, j + 1, 0.5 * (times[j] + times[j + 1]))
    counts = np.insert(counts, j + 1, 0)
    out = {k: v for k, v in b.items() if k not in ('true_paths', 'observed_dates')}
    out.update(times=times, time_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), X=X,
               obs_idx=torch.tensor(idx2, dtype=torch.long),
               n_obs_ot=torch.tensor(np.bincount(idx2, minlength=B).astype(np.int64)))
    if M is not None:
        out['M'] = M
    return out, dt_factor * dt


def oracle_truth(cfg, sd, b, delta_t, T, dtype, grads=True, masks=None, c_hT=None, **kw):
    """The oracle's hT, loss and per-parameter gradients in ``dtype``; inputs and parameters are the
    fp32 values the kernels see, widened (times stay the fp32 clock's).  Dropout is off, or, with
    ``masks`` (a mask source, oracle/dropout_oracle.KernelMasks), the kernels' masks in a training
    call.  ``c_hT``: the gradients are those of loss + (c_hT hT).sum()."""
    cast = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b.items()}
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    if not grads:
        with torch.no_grad():
            out, _ = oracle_forward(cfg, sdd, cast, delta_t, T, training=masks is not None, masks=masks, **kw)
        return out, None
    out, params = oracle_forward(cfg, sdd, cast, delta_t, T, training=True, grads=True, masks=masks, **kw)
    obj = out[1] if c_hT is None else out[1] + (torch.as_tensor(c_hT).to(dtype) * out[0]).sum()
    obj.backward()
    # (a parameter the objective does not depend on -- the readout of a batch nobody is observed in -- has
    # no .grad: its gradient is zero)
    return out, {k: (np.zeros(tuple(p.shape)) if p.grad is None else p.grad.detach().numpy().astype(np.float64))
                 for k, p in params.items()}


def kernel_names(fn):
    """Run ``fn()`` with the library's kernel profile on; returns (fn's result, sorted kernel names)."""
    from njode_amd import _lib
    torch.cuda.synchronize()
    _lib.profile_enable(1)
    _lib.profile_read()
    try:
        res = fn()
        torch.cuda.synchronize()
        names = sorted(_lib.profile_read())
    finally:
        _lib.profile_enable(0)
    return res, names


def oracle_pair(cfg, sd, b, delta_t, T, predict=False, masks=None, grads=None, **kw):
    """(f32, f64) oracle results of one batch: dicts of loss, hT, g (per-parameter gradients)[,
    path_h, path_y].  ``kw['get_loss'] = False``: a prediction call (no loss, no gradients);
    ``grads=False``: an eval-mode call that keeps its loss (no gradients).
    ``masks``: a mask source (oracle/dropout_oracle.KernelMasks): a training call with the
    kernels' own dropout masks, the same masks in fp32 and float64 (``check_vs_oracle``'s
    yardstick stays the fp32 oracle's distance from float64)."""
    # (one thread: the oracle's tensors are a few paths wide, and a pool of threads only
    # synchronises -- 0.3 s against 20 s for a 24-path batch of 100 steps on a busy host)
    # (restored below: later tests of the session keep their own setting)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    get_loss = kw.get('get_loss', True)
    grads = get_loss if grads is None else grads
    try:
        res = []
        for dtype in (torch.float32, torch.float64):
            out, g = oracle_truth(cfg, sd, b, delta_t, T, dtype, grads=grads, masks=masks, return_path=predict,
                                  **kw)
            r = {'hT': out[0].detach().numpy().astype(np.float64), 'g': g}
            if get_loss:
                # (a batch without observations: the oracle's loss is the reference's Python 0)
                r['loss'] = float(out[1].detach()) if torch.is_tensor(out[1]) else float(out[1])
            if predict:
                r['path_h'] = out[3].detach().numpy().astype(np.float64)
                r['path_y'] = out[4].detach().numpy().astype(np.float64)
            res.append(r)
    finally:
        torch.set_num_threads(threads)
    return tuple(res)


def check_vs_oracle(tag, o32, o64, res, ratios, family, floor_h=2e-6, floor_g=1e-5, predict=False):
    """HIP results ``res`` (loss_fused, loss_auto, hT, g.<name>, grad_fused, grad_auto[, path_h, path_y]) against
    the float64 oracle, with the fp32 oracle's own distance from it as the yardstick:
    err(HIP, f64) <= max(2 err(o32, f64), floor), and never looser than ATOL / RTOL / GRAD_REL_L2.  A
    prediction call's ``res`` has no loss keys, or ``loss_predict`` alone (``get_loss=True``: no
    gradients); a step the fused call cannot make (``until_T``) has no ``loss_fused`` / ``grad_fused``.
    Records the worst ratio of ``family`` in ``ratios``."""
    worst, worst_of = 0.0, ('', 0.0, 0.0)

    def ratio(e, e32, what=''):
        nonlocal worst, worst_of
        r = e / max(e32, 1e-300)
        if r > worst:
            worst, worst_of = r, (what, e, e32)
        return r

    loss_keys = [k for k in ('loss_fused', 'loss_auto', 'loss_predict') if k in res]
    if loss_keys:
        l64 = o64['loss']
        e32 = abs(o32['loss'] - l64)
        for key in loss_keys:
            e = abs(res[key] - l64)
            assert e <= max(2 * e32, 1e-6 * abs(l64)), (tag, key, res[key], l64, e, e32)
            assert e <= 1e-4 * abs(l64), (tag, key)
    eh, eh32 = np.abs(res['hT'] - o64['hT']).max(), np.abs(o32['hT'] - o64['hT']).max()
    assert eh <= max(2 * eh32, floor_h), (tag, 'hT', eh, eh32)
    np.testing.assert_allclose(res['hT'], o64['hT'], atol=ATOL, rtol=RTOL, err_msg=tag)
    ratio(eh, eh32, 'hT')
    if 'loss_auto' in res:
        for k in o64['g']:
            e, e32g = rel_l2(res['g.' + k], o64['g'][k]), rel_l2(o32['g'][k], o64['g'][k])
            assert e <= max(2 * e32g, floor_g), (tag, k, e, e32g)
            assert e <= GRAD_REL_L2, (tag, k, e)
            ratio(e, e32g, k)
    if 'grad_fused' in res:
        # the fused step: the same kernels, the same numbers (flat, in the model's parameter order)
        assert rel_l2(res['grad_fused'], res['grad_auto']) < 1e-5, (tag, rel_l2(res['grad_fused'], res['grad_auto']))
    if predict:
        ep, ep32 = np.abs(res['path_h'] - o64['path_h']).max(), np.abs(o32['path_h'] - o64['path_h']).max()
        assert ep <= max(2 * ep32, floor_h), (tag, 'path_h', ep, ep32)
        ratio(ep, ep32, 'path_h')
        if 'path_y' in res:
            ey, ey32 = np.abs(res['path_y'] - o64['path_y']).max(), np.abs(o32['path_y'] - o64['path_y']).max()
            assert ey <= max(2 * ey32, floor_h), (tag, 'path_y', ey, ey32)
            ratio(ey, ey32, 'path_y')
    ratios[family] = max(ratios.get(family, 0.0), worst)
    print('{:40s} worst err(HIP, f64) / err(o32, f64) = {:.2f}  ({}: {:.2e} / {:.2e})'.format(tag, worst, *worst_of))
