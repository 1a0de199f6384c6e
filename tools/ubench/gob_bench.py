"""
Training-step time of the GRU-ODE-Bayes baseline (njode_amd/gru_ode_bayes.py): forward + backward +
torch.optim.Adam, in ms per step, and the kernels' time per Euler step.

Shapes: d = 1, hidden sizes 10 at B = 100, 200 and 1 000 paths on 100 grid steps (Black-Scholes data,
10 % observed), impute False and True; the climate shape (d = 5, H = 50, p_hidden 25, prep_hidden 10,
cov_hidden 50) at B = 100 on 2 000 Euler steps (T = 200, delta_t = 0.1, about 20 masked rows per
path).  For context, in the same process and on the same batch: the test restatement
(tests/gob_oracle.py) moved to the GPU as plain torch ops with autograd and Adam, and NJ-ODE's own
fused step (NJODE.loss_and_grad + FusedAdam).

Method: every variant is warmed up, then timed between two device events over a window of at least
0.3 s (the torch restatement of the long shapes: at least 2 steps); the kernels' own times come from
the library's per-kernel event profile in a separate, untimed pass.  One JSON line per shape goes
to profiles/gob_bench.jsonl.

Usage:  python tools/ubench/gob_bench.py [--out profiles/gob_bench.jsonl] [--quick]
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import gob_oracle                                                       # noqa: E402
from njode_amd import _lib, data_utils, gru_ode_bayes, models           # noqa: E402

NN50 = ((50, 'tanh'), (50, 'tanh'))


def bs_batch(B, n_steps):
    hp = copy.deepcopy(data_utils.hyperparam_default)
    hp.update(nb_paths=B, nb_steps=n_steps, obs_perc=0.1)
    paths, obs, nb_obs, meta = data_utils.create_dataset('BlackScholes', hp, seed=0)
    b = data_utils.collate_arrays(paths, obs, nb_obs, meta['dt'])
    b['M'] = torch.ones_like(b['X'])
    return b, float(meta['dt']), float(meta['maturity'])


def climate_batch(B, n_steps, d=5, dt=0.1, rows_per_path=20, seed=0):
    rng = np.random.RandomState(seed)
    walk = np.cumsum(rng.normal(0.0, 0.05, size=(B, n_steps + 1, d)), axis=1).astype(np.float32)
    when = np.stack([np.sort(rng.choice(np.arange(1, n_steps + 1), size=rows_per_path, replace=False))
                     for _ in range(B)])
    order = np.lexsort((np.repeat(np.arange(B), rows_per_path), when.ravel()))
    step, path = when.ravel()[order], np.repeat(np.arange(B), rows_per_path)[order]
    M = (rng.uniform(size=(len(step), d)) < 0.6).astype(np.float32)
    M[M.sum(axis=1) == 0, 0] = 1.0
    grid, counts = np.unique(step, return_counts=True)
    b = dict(times=grid.astype(np.float64) * dt, time_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
             X=torch.from_numpy(walk[path, step] * M), M=torch.from_numpy(M),
             obs_idx=torch.from_numpy(path.astype(np.int64)), start_X=torch.from_numpy(walk[:, 0].copy()),
             n_obs_ot=torch.full((B,), rows_per_path, dtype=torch.int64))
    return b, dt, n_steps * dt


def timed(step, min_window=0.3, min_steps=2, warm=2):
    """ms per call of ``step`` between two device events, over >= min_window seconds."""
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); step(); z.record(); z.synchronize()
    n = max(min_steps, int(np.ceil(min_window * 1e3 / max(a.elapsed_time(z), 1e-3))))
    a.record()
    for _ in range(n):
        step()
    z.record(); z.synchronize()
    return a.elapsed_time(z) / n, n


def measure(tag, cfg, b, delta_t, T, njode_cfg, quick):
    dev = 'cuda'
    X, M, sx = b['X'].to(dev), b['M'].to(dev), b['start_X'].to(dev)
    torch.manual_seed(0)
    kw = dict(input_size=cfg['d'], hidden_size=cfg['H'], p_hidden=cfg['PH'], prep_hidden=cfg['PR'], bias=True,
              cov_size=cfg['d'], cov_hidden=cfg['CH'], mixing=1e-4, dropout_rate=0.1, full_gru_ode=True,
              impute=cfg['impute'], options=dict(device_outputs=True))
    m = gru_ode_bayes.NNFOwithBayesianJumps(**kw).to(dev).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-4)

    def hip_step():
        opt.zero_grad()
        m(b['times'], b['time_ptr'], X, M, b['obs_idx'], delta_t, T, sx)[1].backward()
        opt.step()

    ms_hip, n_hip = timed(hip_step)
    _lib.profile_enable(1)
    _lib.profile_read()
    for _ in range(3):
        hip_step()
    prof = {k: v[1] / v[0] for k, v in _lib.profile_read().items() if k.startswith('k_gob')}
    _lib.profile_enable(0)
    K = m._schedules.get(b['times'], delta_t, T, True).n_steps

    # the restatement as plain torch ops on the GPU (dropout off: it draws nothing)
    p = gob_oracle.cast({k: v.detach() for k, v in m.state_dict().items()}, torch.float32, device=dev,
                        requires_grad=True)
    keys = gob_oracle.loss_keys(p)
    opt_t = torch.optim.Adam([p[k] for k in keys], lr=1e-3, weight_decay=5e-4)

    def torch_step():
        opt_t.zero_grad()
        gob_oracle.forward(p, b['times'], b['time_ptr'], X, M, b['obs_idx'], delta_t, T, sx, 1e-4)['loss'].backward()
        opt_t.step()

    ms_torch, n_torch = timed(torch_step, min_window=0.0 if (quick or K > 500) else 0.3, warm=1)

    # NJ-ODE's own fused step on the same batch
    torch.manual_seed(0)
    nj = models.NJODE(**njode_cfg).to(dev).train()
    opt_n = models.FusedAdam(nj, lr=1e-3, weight_decay=0.0005)
    idx, n_ot = b['obs_idx'].to(dev, torch.int32), b['n_obs_ot'].to(dev, torch.int32)
    masked = njode_cfg['options'].get('masked', False)

    def njode_step():
        nj.loss_and_grad(b['times'], b['time_ptr'], X, idx, delta_t, T, sx, n_ot, M=M if masked else None)
        opt_n.step()

    ms_nj, n_nj = timed(njode_step)
    B = int(sx.shape[0])
    row = dict(shape=tag, B=B, euler_steps=K, n_obs=int(b['time_ptr'][-1]), impute=bool(cfg['impute']),
               ms_per_step_hip=round(ms_hip, 4), steps_timed_hip=n_hip,
               ms_per_step_torch_gpu=round(ms_torch, 3), steps_timed_torch=n_torch,
               ms_per_step_njode=round(ms_nj, 4), steps_timed_njode=n_nj,
               kernel_ms={k: round(v, 4) for k, v in sorted(prof.items())},
               us_per_euler_step_fwd=round(1e3 * prof.get('k_gob_fwd', float('nan')) / K, 4),
               us_per_euler_step_bwd=round(1e3 * prof.get('k_gob_bwd', float('nan')) / K, 4),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'gob_bench.jsonl'))
    ap.add_argument('--quick', action='store_true', help='one torch-restatement window of 2 steps everywhere')
    args = ap.parse_args()
    rows = []
    small = dict(d=1, H=10, PH=10, PR=10, CH=10)
    nj_small = dict(input_size=1, hidden_size=10, output_size=1, ode_nn=NN50, readout_nn=NN50, enc_nn=NN50,
                    use_rnn=False, bias=True, dropout_rate=0.1, options={'device_outputs': True})
    for B in (100, 200, 1000):
        b, dt, T = bs_batch(B, 100)
        for impute in (False, True):
            rows.append(measure('d1_h10', dict(small, impute=impute), b, dt, T, nj_small, args.quick))
    clim = dict(d=5, H=50, PH=25, PR=10, CH=50)
    nj_clim = dict(input_size=5, hidden_size=50, output_size=5, ode_nn=NN50, readout_nn=NN50, enc_nn=NN50,
                   use_rnn=False, bias=True, dropout_rate=0.1,
                   options={'device_outputs': True, 'masked': True})
    b, dt, T = climate_batch(100, 2000)
    for impute in (False, True):
        rows.append(measure('climate', dict(clim, impute=impute), b, dt, T, nj_clim, args.quick))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
