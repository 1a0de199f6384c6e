"""The PhysioNet and climate evaluation protocols: the host route (``evaluate_model``: prediction
path on the GPU, copied to the host, rows and masked errors by numpy) against the device route
(``evaluate_model_device``) on the same model and the same batch.

    python tools/ubench/protocol_bench.py [--out profiles/protocol_bench.jsonl]

One process; warm-up calls first; the two routes alternate so that neither owns a quieter stretch
of the machine; each call ends in a device synchronise.  Per case one JSON line: median and
fastest call of either route, the prediction path alone (the masked forward both routes share) in
a column of its own with its share of the device route, and the bytes of ``path_y`` the host route
copies.  Cases: the PhysioNet batch of ``make_eval_batch`` at ``n_grid = 3000`` with B = 50 and
B = 800, and ``make_climate_batch`` at its defaults.  Results are appended to ``--out``.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from njode_amd import climate_eval, models, physionet_eval  # noqa: E402

NN = ((50, 'tanh'), (50, 'tanh'))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(out)), float(np.min(out))]


def bench(name, mod, batch, dim, hidden, reps):
    torch.manual_seed(0)
    model = models.NJODE(dim, hidden, dim, NN, NN, NN, False,
                         options={'device_outputs': True, 'masked': True}).to('cuda').eval()
    dt, T = batch['delta_t'], batch['T']
    B = batch['batch_size'] if 'batch_size' in batch else len(batch['pat_idx'])
    X, M = batch['X'].cuda(), batch['M'].cuda()
    n_obs_ot = torch.bincount(batch['obs_idx'].cuda(), minlength=B)
    start_X = torch.zeros(B, dim, device='cuda')

    def pred_only():
        with torch.no_grad():
            return model(batch['times'], batch['time_ptr'], X, batch['obs_idx'], dt, T, start_X, n_obs_ot,
                         until_T=True, return_path=True, get_loss=True, M=M)[4]

    host = lambda: mod.evaluate_model(model, [batch], 'cuda', dt, T)
    dev = lambda: mod.evaluate_model_device(model, [batch], 'cuda', dt, T)
    r_host, r_dev = host(), dev()
    n_rows = int(pred_only().shape[0])
    t_pred = timed(pred_only, 2, reps)
    t_host_a = timed(host, 1, reps)
    t_dev_a = timed(dev, 2, reps)
    t_host_b = timed(host, 0, reps)
    t_dev_b = timed(dev, 0, reps)
    dev_med = max(t_dev_a[0], t_dev_b[0])
    return {
        'case': name, 'B': B, 'dim': dim, 'path_rows': n_rows, 'held_out': int(len(batch['times_val'])),
        'path_y_bytes': 4 * n_rows * B * dim,
        'result_host': list(r_host), 'result_device': list(r_dev),
        'mse_rel_diff': abs(r_dev[1] - r_host[1]) / abs(r_host[1]),
        'prediction_path_ms_median_min': t_pred,
        'evaluate_host_ms_median_min': [t_host_a, t_host_b],
        'evaluate_device_ms_median_min': [t_dev_a, t_dev_b],
        'prediction_path_share_of_device_route': t_pred[0] / dev_med,
        'host_over_device_median': min(t_host_a[0], t_host_b[0]) / dev_med,
    }


def cases():
    for B, reps in ((50, 10), (800, 3)):
        b = physionet_eval.make_eval_batch(batch_size=B, n_grid=3000)
        yield 'physionet B={} n_grid=3000'.format(B), physionet_eval, b, 41, 41, reps
    b = climate_eval.make_climate_batch()
    yield 'climate B=100', climate_eval, b, climate_eval.CLIMATE_DIM, 10, 10


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: there is nothing to measure without one'
    for case in cases():
        r = bench(*case)
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')
