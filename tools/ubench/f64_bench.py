"""Forward + backward times of the float64 route (njode_amd.float64.NJODE64) beside the fp32 route
and the CPU oracle in float64.  No thresholds: the float64 family exists for correctness and reach.

    python tools/ubench/f64_bench.py [--out profiles/f64_route.jsonl] [--reps 5] [--no-cpu]

Workloads: the demo model at B = 200; config 5 (PhysioNet-shaped, masked, d = H = 41) at B = 50 over
3 000 Euler steps; the 20 000-path Black-Scholes batch (no CPU oracle).  One JSON line per workload is
appended to --out: median and minimum milliseconds of forward + backward (autograd, inputs resident,
device synchronised around every repetition).
"""
import argparse
import contextlib
import copy
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

NN = ((50, 'tanh'), (50, 'tanh'))


def demo_cfg():
    return dict(input_size=1, hidden_size=10, output_size=1, ode_nn=NN, readout_nn=NN, enc_nn=NN,
                use_rnn=False, bias=True, dropout_rate=0.0, options={'device_outputs': True})


def config5_cfg():
    return dict(input_size=41, hidden_size=41, output_size=41, ode_nn=NN, readout_nn=NN, enc_nn=NN,
                use_rnn=False, bias=True, dropout_rate=0.0, options={'masked': True, 'device_outputs': True})


def bs_batch(n_paths):
    from njode_amd import data_utils
    hp = copy.deepcopy(data_utils.hyperparam_default)
    hp['nb_paths'] = n_paths
    paths, obs, nb_obs, meta = data_utils.create_dataset('BlackScholes', hp, seed=0)
    return data_utils.collate_arrays(paths, obs, nb_obs, meta['dt']), meta['dt'], meta['maturity']


def physio_batch(n_paths):
    from njode_amd import synthetic_physionet
    b = synthetic_physionet.make_batch(batch_size=n_paths, seed=0)
    return b, b['delta_t'], b['T']


def time_gpu(model, b, dt, T, reps):
    dev = 'cuda'
    args = (b['times'], b['time_ptr'], b['X'].to(dev), b['obs_idx'].to(dev, torch.int32), dt, T,
            b['start_X'].to(dev), b['n_obs_ot'].to(dev, torch.int32))
    M = b['M'].to(dev) if 'M' in b else None

    def one():
        for p in model.parameters():
            p.grad = None
        _, loss = model(*args, M=M)
        loss.backward()
        torch.cuda.synchronize()

    one()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        one()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'reps': reps}


def time_cpu_oracle(cfg, sd, b, dt, T):
    """One float64 forward + backward of the CPU oracle (torch's default thread count)."""
    from oracle import njode_oracle
    o = njode_oracle.make_oracle(cfg)
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd.items()}
    cast = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b.items()}
    t0 = time.perf_counter()
    _, loss = o.forward(params, cast['times'], cast['time_ptr'], cast['X'], cast['obs_idx'], dt, T,
                        cast['start_X'], cast['n_obs_ot'], M=cast.get('M'))
    loss.backward()
    return {'ms': round(1e3 * (time.perf_counter() - t0), 1), 'threads': torch.get_num_threads(), 'reps': 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'f64_route.jsonl'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--only', default='', help='comma-separated workload names')
    args = ap.parse_args()
    from njode_amd import models
    work = [('demo_B200', demo_cfg, lambda: bs_batch(200), True),
            ('config5_B50_K3000', config5_cfg, lambda: physio_batch(50), True),
            ('bs_20000_paths', demo_cfg, lambda: bs_batch(20000), False)]
    only = set(filter(None, args.only.split(',')))
    for name, cfg_fn, batch_fn, with_cpu in work:
        if only and name not in only:
            continue
        cfg = cfg_fn()
        b, dt, T = batch_fn()
        torch.manual_seed(0)
        with contextlib.redirect_stdout(sys.stderr):
            m32 = models.NJODE(**cfg).cuda().train()
            m64 = m32.float64()
        rec = {'kind': 'bench', 'workload': name, 'paths': int(b['start_X'].shape[0]),
               'rows': int(b['time_ptr'][-1]), 'what': 'forward + backward, ms',
               'f64_route': time_gpu(m64, b, dt, T, args.reps), 'fp32_route': time_gpu(m32, b, dt, T, args.reps)}
        if with_cpu and not args.no_cpu:
            rec['cpu_oracle_f64'] = time_cpu_oracle(cfg, m32.state_dict(), b, dt, T)
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
