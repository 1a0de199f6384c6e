"""
Golden fixtures of the GRU-ODE-Bayes baseline: tests/golden/gob_*.npz.

Runs only where the reference checkout is (CPU; its root is /root/reference, or the directory named
by the environment variable NJODE_REFERENCE).  It imports the reference's own class
``GRU_ODE_Bayes.models_gru_ode_bayes.NNFOwithBayesianJumps`` and records, per case: the inputs, the
``state_dict`` (``sd.*``), the eval-mode ``hT`` / ``loss`` / ``loss_1`` / ``path_t`` / ``path_p`` /
``path_h``, the train-mode (dropout 0) gradients of ``loss`` (``g.*``), and the parameters the loss
depends on after 1 and 5 steps of ``torch.optim.Adam(lr=1e-3, weight_decay=5e-4)`` (``adam1.*``,
``adam5.*``).  Data only.  Usage:  python tests/golden/make_golden_gob.py

Cases (all with mixing 1e-4, bias):
  gob_d1_plain / gob_d1_impute      d = 1, hidden sizes 10: a Black-Scholes batch of 17 paths on 50
                                    grid steps (seed 3, 20 % observed), M = 1
  gob_clim_plain / gob_clim_impute  the climate shape d = 5, H = 50, p_hidden 25, prep_hidden 10,
                                    cov_hidden 50: 9 paths on 40 grid steps of 0.1, about six
                                    observation times per path, each feature observed with
                                    probability 0.6 (at least one per row)
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ.get('NJODE_REFERENCE', '/root/reference'))

from njode_amd import data_utils                                   # noqa: E402
from GRU_ODE_Bayes import models_gru_ode_bayes as ref               # noqa: E402

SKIP = ('classification_model.', 'gru_obs.gru_debug.')


def d1_batch():
    hp = copy.deepcopy(data_utils.hyperparam_default)
    hp.update(nb_paths=17, nb_steps=50, obs_perc=0.2)
    paths, obs, nb_obs, meta = data_utils.create_dataset('BlackScholes', hp, seed=3)
    b = data_utils.collate_arrays(paths, obs, nb_obs, meta['dt'])
    return dict(times=np.asarray(b['times'], dtype=np.float64), time_ptr=np.asarray(b['time_ptr'], dtype=np.int64),
                X=b['X'].float(), M=torch.ones_like(b['X']).float(), obs_idx=b['obs_idx'].long(),
                start_X=b['start_X'].float(), delta_t=float(meta['dt']), T=float(meta['maturity']))


def climate_batch(B=9, steps=40, d=5, dt=0.1, seed=11):
    rng = np.random.RandomState(seed)
    walk = np.cumsum(rng.normal(0.0, 0.3, size=(B, steps + 1, d)), axis=1)
    rows = []                                                       # (grid step, path, values, mask)
    for p in range(B):
        for s in sorted(rng.choice(np.arange(1, steps + 1), size=6, replace=False)):
            m = (rng.uniform(size=d) < 0.6).astype(np.float32)
            if m.sum() == 0:
                m[rng.randint(d)] = 1.0
            rows.append((int(s), p, walk[p, s] * m, m))
    rows.sort(key=lambda r: (r[0], r[1]))
    grid = sorted({r[0] for r in rows})
    counts = [sum(1 for r in rows if r[0] == s) for s in grid]
    return dict(times=np.array(grid, dtype=np.float64) * dt,
                time_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                X=torch.tensor(np.stack([r[2] for r in rows]), dtype=torch.float32),
                M=torch.tensor(np.stack([r[3] for r in rows]), dtype=torch.float32),
                obs_idx=torch.tensor([r[1] for r in rows], dtype=torch.long),
                start_X=torch.tensor(walk[:, 0], dtype=torch.float32), delta_t=dt, T=steps * dt)


def run_case(name, batch, cfg, seed):
    torch.manual_seed(seed)
    model = ref.NNFOwithBayesianJumps(
        input_size=cfg['input_size'], hidden_size=cfg['hidden_size'], p_hidden=cfg['p_hidden'],
        prep_hidden=cfg['prep_hidden'], bias=True, cov_size=cfg['input_size'], cov_hidden=cfg['cov_hidden'],
        logvar=True, mixing=cfg['mixing'], dropout_rate=0.0, full_gru_ode=True, solver='euler',
        impute=bool(cfg['impute']))
    b = batch
    args = (b['times'], b['time_ptr'], b['X'], b['M'], b['obs_idx'], b['delta_t'], b['T'], b['start_X'])
    out = {'in.' + k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in b.items()}
    out.update({'cfg.' + k: np.asarray(v) for k, v in cfg.items()})
    out.update({'sd.' + k: v.detach().numpy().copy() for k, v in model.state_dict().items()})
    model.eval()
    with torch.no_grad():
        hT, loss, _, loss_1 = model(*args)
        _, loss_p, _, path_t, path_p, path_h, _, _ = model(*args, return_path=True)
    assert float(loss_p) == float(loss)
    out.update(hT=hT.numpy(), loss=np.float64(loss), loss_1=np.float64(loss_1), path_t=np.asarray(path_t),
               path_p=path_p.numpy(), path_h=path_h.numpy())
    model.train()
    model.zero_grad()
    model(*args)[1].backward()
    for k, p in model.named_parameters():
        if k.startswith(SKIP):
            assert p.grad is None, k
        else:
            out['g.' + k] = p.grad.numpy().copy()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
    for step in range(1, 6):
        opt.zero_grad()
        model(*args)[1].backward()
        opt.step()
        if step in (1, 5):
            out.update({'adam{}.{}'.format(step, k): v.detach().numpy().copy()
                        for k, v in model.state_dict().items() if not k.startswith(SKIP)})
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print(name, 'loss', float(loss), 'loss_1', float(loss_1), 'rows', path_p.shape[0],
          os.path.getsize(path) // 1024, 'KB')


def main():
    torch.set_num_threads(1)
    d1, clim = d1_batch(), climate_batch()
    small = dict(input_size=1, hidden_size=10, p_hidden=10, prep_hidden=10, cov_hidden=10, mixing=1e-4)
    big = dict(input_size=5, hidden_size=50, p_hidden=25, prep_hidden=10, cov_hidden=50, mixing=1e-4)
    run_case('gob_d1_plain', d1, dict(small, impute=0), 1)
    run_case('gob_d1_impute', d1, dict(small, impute=1), 2)
    run_case('gob_clim_plain', clim, dict(big, impute=0), 3)
    run_case('gob_clim_impute', clim, dict(big, impute=1), 4)


if __name__ == '__main__':
    main()
