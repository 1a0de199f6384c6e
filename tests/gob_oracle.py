"""
TEST INFRASTRUCTURE: a functional, dtype-generic torch restatement of the GRU-ODE-Bayes baseline
(reference ``GRU_ODE_Bayes/models_gru_ode_bayes.py``, class ``NNFOwithBayesianJumps`` as
``NJODE/train.py:383-392`` constructs it: full GRU-ODE cell, log-variance, Euler), written from its
semantics.  It runs on whatever dtype and device the ``state_dict`` it is given has, so the same
code is the fp32 run and the float64 truth of the GPU tests.

Reference lines restated:
  start           ``:384-386``   h = covariates_map(cov), p = p_model(h)
  clock           ``:409-422, 457-467``
  Euler step      ``:155-174`` (autonomous), ``:116-135`` (impute), ``:335-363``
  jump            ``:192-218``, ``:430-449``
  KL term         ``:561-575``
  loss, returns   ``:477-494``

``masks``: an optional mask source with the call convention of
``oracle/dropout_oracle.py::KernelMasks('gen', seed, p)``: ``masks(net, tkey, rows, layer, width)``
gives the [len(rows), width] keep indicators, ``masks.scale`` the factor of a kept unit.  Keys are
the kernels': net 5 = covariates_map (start), 6 = p_model at the start and after Euler step k
(time key k), 7 = p_model after time slice i (time key = Euler steps completed by then).
"""
import math

import numpy as np
import torch

NET_COV, NET_P, NET_P_JUMP = 5, 6, 7
TKEY_START = 0xFFFFFFFF


def _linear(sd, name, x):
    y = x @ sd[name + '.weight'].t()
    b = sd.get(name + '.bias')
    return y if b is None else y + b


def _hidden(sd, name, x, masks, net, tkey):
    """Linear -> ReLU -> Dropout of a two-layer net's first half."""
    a = torch.relu(_linear(sd, name, x))
    if masks is not None:
        keep = masks(net, tkey, np.arange(x.shape[0]), 0, a.shape[1])
        a = a * torch.as_tensor(np.asarray(keep, dtype=np.float64), dtype=a.dtype, device=a.device) \
            * torch.tensor(masks.scale, dtype=a.dtype, device=a.device)
    return a


def p_model(sd, h, masks, net, tkey):
    return _linear(sd, 'p_model.3', _hidden(sd, 'p_model.0', h, masks, net, tkey))


def covariates_map(sd, cov, masks):
    return torch.tanh(_linear(sd, 'covariates_map.3',
                              _hidden(sd, 'covariates_map.0', cov, masks, NET_COV, TKEY_START)))


def cell_dh(sd, p, h, impute):
    """(1 - z)(u - h) of the full GRU-ODE cell; x = lin_x(p) with impute, else 0."""
    H = h.shape[1]
    if impute:
        x = _linear(sd, 'gru_c.lin_x', p)
        xr, xz, xh = x[:, :H], x[:, H:2 * H], x[:, 2 * H:]
    else:
        xr = xz = xh = torch.zeros_like(h)
    r = torch.sigmoid(xr + h @ sd['gru_c.lin_hr.weight'].t())
    z = torch.sigmoid(xz + h @ sd['gru_c.lin_hz.weight'].t())
    u = torch.tanh(xh + (r * h) @ sd['gru_c.lin_hh.weight'].t())
    return (1 - z) * (u - h)


def gru_cell(sd, prefix, x, h):
    """torch.nn.GRUCell: gates r, z, n; n = tanh(W_in x + b_in + r (W_hn h + b_hn))."""
    H = h.shape[1]
    gi = x @ sd[prefix + '.weight_ih'].t()
    gh = h @ sd[prefix + '.weight_hh'].t()
    if prefix + '.bias_ih' in sd:
        gi = gi + sd[prefix + '.bias_ih']
        gh = gh + sd[prefix + '.bias_hh']
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return n + z * (h - n)


def observe(sd, h, p, X_obs, M_obs, i_obs):
    """The observation cell on the rows ``i_obs``: new h and the loss_1 terms."""
    d = X_obs.shape[1]
    p_obs = p[i_obs]
    mean, logvar = p_obs[:, :d], p_obs[:, d:]
    err = (X_obs - mean) / torch.exp(0.5 * logvar)
    losses = 0.5 * ((err ** 2 + logvar + math.log(2 * math.pi)) * M_obs)
    w, bp = sd['gru_obs.w_prep'], sd['gru_obs.bias_prep']                  # [d, 4, PR], [d, PR]
    inp = torch.stack([X_obs, mean, logvar, err], dim=2)                   # [n, d, 4]
    g = torch.relu(torch.einsum('nfc,fcj->nfj', inp, w) + bp) * M_obs[:, :, None]
    g = g.reshape(g.shape[0], d * w.shape[2])                                         # index f * PR + j
    h_new = h.clone()
    h_new[i_obs] = gru_cell(sd, 'gru_obs.gru_d', g, h[i_obs])
    return h_new, losses


def kl_term(p_obs, X_obs, M_obs, noise_std=1e-2):
    d = X_obs.shape[1]
    mean, logvar = p_obs[:, :d], p_obs[:, d:]
    std = torch.exp(0.5 * logvar)
    kl = (math.log(noise_std) - torch.log(std) + (std ** 2 + (mean - X_obs) ** 2) / (2 * noise_std ** 2) - 0.5)
    return (kl * M_obs).sum()


def forward(sd, times, time_ptr, X, M, obs_idx, delta_t, T, cov, mixing, masks=None, return_path=False):
    """``NNFOwithBayesianJumps.forward``: a dict with ``hT``, ``loss``, ``loss_1`` and, with
    ``return_path``, ``path_t`` (numpy), ``path_p``, ``path_h``."""
    impute = 'gru_c.lin_x.weight' in sd
    obs_idx = torch.as_tensor(obs_idx).long().to(cov.device)
    h = covariates_map(sd, cov, masks)
    p = p_model(sd, h, masks, NET_P, TKEY_START)
    now, k = 0.0, 0
    loss_1 = torch.zeros((), dtype=cov.dtype, device=cov.device)
    loss_2 = torch.zeros((), dtype=cov.dtype, device=cov.device)
    path_t, path_p, path_h = [0.0], [p], [h]

    def evolve(now, k, h, p, target):
        while now < target - 1e-10 * delta_t:
            dt = delta_t if now < target - delta_t else target - now
            h = h + dt * cell_dh(sd, p, h, impute)
            p = p_model(sd, h, masks, NET_P, k)
            now, k = now + dt, k + 1
            if return_path:
                path_t.append(now); path_p.append(p); path_h.append(h)
        return now, k, h, p

    for i, obs_time in enumerate(times):
        now, k, h, p = evolve(now, k, h, p, obs_time)
        lo, hi = int(time_ptr[i]), int(time_ptr[i + 1])
        X_obs, M_obs, i_obs = X[lo:hi], M[lo:hi], obs_idx[lo:hi]
        h, losses = observe(sd, h, p, X_obs, M_obs, i_obs)
        loss_1 = loss_1 + losses.sum()
        p = p_model(sd, h, masks, NET_P_JUMP, k)
        loss_2 = loss_2 + kl_term(p[i_obs], X_obs, M_obs)
        if return_path:
            path_t.append(float(obs_time)); path_p.append(p); path_h.append(h)
    now, k, h, p = evolve(now, k, h, p, T)

    out = {'hT': h, 'loss': loss_1 + mixing * loss_2, 'loss_1': loss_1}
    if return_path:
        out.update(path_t=np.array(path_t), path_p=torch.stack(path_p), path_h=torch.stack(path_h))
    return out


# the parameters the loss depends on, in state_dict order (the C ABI's flat order)
def loss_keys(sd):
    return [k for k in sd if not k.startswith(('classification_model.', 'gru_obs.gru_debug.'))]


def cast(sd, dtype, device=None, requires_grad=False):
    """A copy of a state_dict (tensors or numpy arrays) in ``dtype``; ``requires_grad``: leaves for
    autograd on the keys the loss depends on."""
    out = {}
    for k, v in sd.items():
        t = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v.detach().cpu().numpy())
        t = t.to(dtype=dtype, device=device).clone()
        out[k] = t
    if requires_grad:
        for k in loss_keys(out):
            out[k].requires_grad_(True)
    return out
