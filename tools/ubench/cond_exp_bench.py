"""Evaluation against the analytic conditional expectation: the host route (``NJODE.evaluate``:
prediction path on the GPU, the truth by numpy on the host) against the device route
(``NJODE.evaluate_device``) on the same model and the same validation batch.

    python tools/ubench/cond_exp_bench.py [--paths 4000 200000] [--out profiles/cond_exp_bench.jsonl]

Per size one JSON line: median and minimum wall time of a call of either route (each call ends
in a device synchronise; warm-up calls first), the prediction path alone, and -- from the
library's own kernel profile, taken in a window of its own -- the time of the fused metric kernel
``k_cond_exp_walk`` with the bytes it needs per second: the prediction read once plus the batch
arrays (``start_X``, ``X``, ``obs_idx``); the dense [n_times][B] row table it also reads is
reported next to it.
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from njode_amd import _lib, data_utils, device_data, models, stock_model  # noqa: E402

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
    return float(np.median(out)), float(np.min(out))


def bench(n_paths, seed=0):
    hp = copy.deepcopy(data_utils.hyperparam_default)
    hp['nb_paths'] = n_paths
    ds = device_data.DeviceDataset.generate('BlackScholes', hp, seed=seed)
    b = ds.collate()
    meta = ds.metadata
    sm = stock_model.BlackScholes(**meta)
    torch.manual_seed(0)
    model = models.NJODE(1, 10, 1, NN, NN, NN, False, options={'device_outputs': True}).to('cuda').eval()
    args = (b['times'], b['time_ptr'], b['X'], b['obs_idx'], meta['dt'], meta['maturity'], b['start_X'])
    host_reps = 10 if n_paths <= 10000 else 3
    dev_reps = 50 if n_paths <= 10000 else 20

    def pred_only():
        with torch.no_grad():
            return model(*args, None, return_path=True, get_loss=False, until_T=True)[4]

    host = lambda: float(model.evaluate(*args, b['n_obs_ot'], sm))
    dev = lambda: float(model.evaluate_device(*args, sm))          # (float(): the one host read)
    msd_host, msd_dev = host(), dev()
    t_pred = timed(pred_only, 3, dev_reps)
    # alternate the two routes so that neither owns a quieter stretch of the machine
    t_host_a = timed(host, 1, host_reps)
    t_dev_a = timed(dev, 3, dev_reps)
    t_host_b = timed(host, 0, host_reps)
    t_dev_b = timed(dev, 0, dev_reps)
    # the fused metric kernel alone (events around it slow the host: a window of its own)
    pred = pred_only()
    n_t, B, d = pred.shape
    n_obs, nt = int(b['X'].shape[0]), len(b['times'])
    metric = lambda: device_data.cond_exp(sm, *args, pred=pred)
    for _ in range(3):
        metric()
    torch.cuda.synchronize()
    _lib.profile_enable(1)
    _lib.profile_read()
    timed(metric, 0, dev_reps)
    launches, total_ms = _lib.profile_read()['k_cond_exp_walk']
    _lib.profile_enable(0)
    kernel_ms = total_ms / launches
    need = 4 * n_t * B * d + 4 * B * d + 4 * n_obs * d + 4 * n_obs
    table = 4 * nt * B
    return {
        'paths': n_paths, 'rows': n_t, 'n_obs': n_obs,
        'msd_host': msd_host, 'msd_device': msd_dev, 'msd_rel_diff': abs(msd_dev - msd_host) / abs(msd_host),
        'prediction_path_ms_median_min': t_pred,
        'evaluate_host_ms_median_min': [t_host_a, t_host_b],
        'evaluate_device_ms_median_min': [t_dev_a, t_dev_b],
        'speedup_median': min(t_host_a[0], t_host_b[0]) / max(t_dev_a[0], t_dev_b[0]),
        'metric_kernel_ms': kernel_ms, 'metric_kernel_launches': launches,
        'metric_bytes_pred_and_batch': need, 'metric_bytes_row_table': table,
        'metric_GBps_pred_and_batch': need / kernel_ms / 1e6,
        'metric_GBps_with_row_table': (need + table) / kernel_ms / 1e6,
    }


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--paths', type=int, nargs='+', default=[4000, 200000])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: there is nothing to measure without one'
    lines = []
    for n in a.paths:
        r = bench(n)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
