"""The regime-switch / Heston-without-Feller producer kernels beside their single-model siblings.

    python tools/ubench/regime_bench.py [--gen-paths 1000000] [--walk-paths 4000 200000]
                                        [--out profiles/regime_bench.jsonl]

One JSON line per measurement, each in a window of its own, warm-up first, median (and minimum):

* ``generate``: ``DeviceDataset.generate`` of N paths x 100 steps, 'Heston' (``k_generate``) and
  'HestonWOFeller' (``k_generate_stage``, with and without ``return_vol``): wall time of a call that
  ends in a device synchronise.  The same draw count per step; the fourth model takes a ``log`` and
  an ``exp`` more and, with ``return_vol``, writes twice the bytes.
* ``walk``: the fused-metric kernel ``k_cond_exp_walk`` (library profile) on ONE batch under two
  descriptions: the single Black-Scholes model of 100 steps (``njode_cond_exp_f64``) and the
  combined model of two Black-Scholes stages of 50 steps (``njode_cond_exp_staged_f64``) -- without
  a sine term the two datasets, clocks and paths are the same, so the difference is the staged
  entry point's alone.
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
from njode_amd import _lib, data_utils, device_data  # noqa: E402


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


def bench_generate(n_paths):
    hp = copy.deepcopy(data_utils.hyperparam_default)
    hp.update(nb_paths=n_paths, nb_steps=100, v0=1.0)
    out = {'what': 'generate', 'paths': n_paths, 'steps': 100}
    for tag, name, kw in (('heston', 'Heston', {}), ('hwf', 'HestonWOFeller', {}),
                          ('hwf_return_vol', 'HestonWOFeller', {'return_vol': True})):
        fn = lambda: device_data.DeviceDataset.generate(name, dict(hp, **kw), seed=1)
        out[tag + '_ms_median_min'] = timed(fn, 3, 20)
    out['hwf_over_heston'] = out['hwf_ms_median_min'][0] / out['heston_ms_median_min'][0]
    return out


def bench_walk(n_paths):
    hp = copy.deepcopy(data_utils.hyperparam_default)
    hp.update(nb_paths=n_paths)
    half = dict(hp, nb_steps=50, maturity=0.5)
    ds = device_data.DeviceDataset.generate('BlackScholes', hp, seed=0)
    two = device_data.DeviceDataset.generate_combined(['BlackScholes'] * 2, [half, half], seed=0)
    same = bool(torch.equal(ds.paths_tm, two.paths_tm))
    b = ds.collate()
    args = (b['times'], b['time_ptr'], b['X'], b['obs_idx'], hp['maturity'] / 100, 1.0, b['start_X'])
    pred = torch.randn((1 + 100 + len(b['times']), n_paths, 1), device='cuda')
    out = {'what': 'walk', 'paths': n_paths, 'rows': int(pred.shape[0]), 'same_dataset': same}
    res = {}
    for tag, meta in (('single', ds.metadata), ('staged', two.metadata)):
        call = lambda: device_data.cond_exp(meta, *args, pred=pred)
        for _ in range(3):
            res[tag] = call()[3].clone()
        torch.cuda.synchronize()
        _lib.profile_enable(1)
        _lib.profile_read()
        wall = timed(call, 0, 30)
        launches, total_ms = _lib.profile_read()['k_cond_exp_walk']
        _lib.profile_enable(0)
        out[tag + '_kernel_ms'] = total_ms / launches
        out[tag + '_call_ms_median_min'] = wall
    out['same_sq_diff_bits'] = bool(torch.equal(res['single'], res['staged']))
    out['staged_over_single_kernel'] = out['staged_kernel_ms'] / out['single_kernel_ms']
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--gen-paths', type=int, default=1000000)
    ap.add_argument('--walk-paths', type=int, nargs='+', default=[4000, 200000])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: there is nothing to measure without one'
    lines = [json.dumps(bench_generate(a.gen_paths))]
    print(lines[-1], flush=True)
    for n in a.walk_paths:
        lines.append(json.dumps(bench_walk(n)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
