"""The climate validation collate, the protocol call it feeds and one epoch of the climate loop,
device route against host route.

    python tools/ubench/climate_records_bench.py [--out profiles/climate_records_bench.jsonl]

One process, warm-up calls first, the two routes alternating, medians (and the fastest call)
after the warm-up; every timed call ends in a device synchronise and is timed with the wall clock
around it, because every route here contains host work of its own.

Per number of stations B = 100 and B = 1 000 (20 - 60 observed rows each, 1 - 3 rows after
``T_val`` = 150, 5 channels: the shape of ``climate_eval.make_climate_batch``):

* ``collate_val`` (GPU, one host wait for the counts) against ``collate_val_host`` + upload of
  every array the protocol call takes;
* ``climate_eval.evaluate_model_device`` on the resident batch against the same call on the
  host-collated batch (held-out arrays uploaded per call), and the prediction path alone (the
  model call both contain), ``delta_t`` = 0.1: 2 000 Euler steps;
* one epoch of ``train_climate_records`` (the B stations in batches of 100, validation and test
  set of B / 10 stations each) with ``device_collate`` on and off.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from njode_amd import climate_eval, models, records, train_records  # noqa: E402

NN = ((50, 'tanh'), (50, 'tanh'))
DT, T, T_VAL, DIM = climate_eval.CLIMATE_DELTA_T, climate_eval.CLIMATE_T, climate_eval.CLIMATE_T_VAL, 5


def make_stations(n, seed=0):
    """Records in the shape of ``make_climate_batch``: 20 - 60 rows up to ``T_val``, 1 - 3 after
    it, times with one decimal, each row with at least one channel on."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        ks = np.sort(rng.choice(np.arange(1, 1501), size=rng.randint(20, 61), replace=False))
        kv = np.sort(rng.choice(np.arange(1501, 2000), size=rng.randint(1, 4), replace=False))
        tt = (np.concatenate([ks, kv]) / 10.0).astype(np.float32)
        mask = rng.random_sample((len(tt), DIM)) < 0.4
        mask[~mask.any(axis=1), 0] = True
        out.append((tt, rng.standard_normal((len(tt), DIM)).astype(np.float32), mask.astype(np.float32)))
    return out


def med_min(ms):
    return [float(np.median(ms)), float(np.min(ms))]


def alternate(fns, warmup, reps):
    """Wall ms of each of ``fns`` (name -> callable), the routes taking turns."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3)
    return {k: med_min(v) for k, v in out.items()}


def upload_val(b):
    d = {k: b[k].cuda() for k in ('X', 'M', 'start_X', 'X_val', 'M_val')}
    d['obs_idx'], d['n_obs_ot'] = b['obs_idx'].cuda().int(), b['n_obs_ot'].cuda().int()
    d['times_val'] = torch.from_numpy(b['times_val']).cuda()
    d['index_val'] = torch.from_numpy(b['index_val']).cuda().int()
    return d


def case(B, reps):
    ds = records.RecordDataset.from_records(make_stations(B + 2 * (B // 10)), time_div=None,
                                            drop_unobserved=False, device='cuda')
    idx = np.arange(B)
    torch.manual_seed(0)
    model = models.NJODE(DIM, 10, DIM, NN, NN, NN, False, dropout_rate=0.1,
                         options={'device_outputs': True, 'masked': True}).to('cuda').eval()
    on_dev, on_host = ds.collate_val(idx, T_VAL, 3), ds.collate_val_host(idx, T_VAL, 3)
    t_collate = alternate({'device': lambda: ds.collate_val(idx, T_VAL, 3),
                           'host': lambda: upload_val(ds.collate_val_host(idx, T_VAL, 3))}, 2, reps)
    call = lambda b: (lambda: climate_eval.evaluate_model_device(model, [b], 'cuda', DT, T))  # noqa: E731
    r_dev, r_host = call(on_dev)(), call(on_host)()
    assert r_dev == r_host, (r_dev, r_host)

    def pred_only():
        with torch.no_grad():
            return model(on_dev['times'], on_dev['time_ptr'], on_dev['X'], on_dev['obs_idx'], DT, T,
                         on_dev['start_X'], on_dev['n_obs_ot'], until_T=True, return_path=True,
                         get_loss=True, M=on_dev['M'])[4]

    t_eval = alternate({'resident': call(on_dev), 'host_collated': call(on_host),
                        'prediction_path': pred_only}, 2, reps)
    tr, va, te = idx, np.arange(B, B + B // 10), np.arange(B + B // 10, B + 2 * (B // 10))
    kw = dict(epochs=1, batch_size=100, log=lambda s: None)
    loop = lambda on: (lambda: train_records.train_climate_records(  # noqa: E731
        ds, tr, va, te, device_collate=on, **kw))
    t_loop = alternate({'device_collate': loop(True), 'host_collate': loop(False)}, 1, max(reps // 3, 3))
    return {
        'case': 'climate records B={}'.format(B), 'B': B, 'dim': DIM, 'n_grid': ds.n_grid,
        'observed_rows': int(on_dev['time_ptr'][-1]), 'observed_times': len(on_dev['times']),
        'held_out_rows': int(on_dev['index_val'].numel()),
        'collate_val_wall_ms_median_min': t_collate['device'],
        'collate_val_host_plus_upload_wall_ms_median_min': t_collate['host'],
        'host_over_device_collate_median': t_collate['host'][0] / t_collate['device'][0],
        'result': list(r_dev),
        'evaluate_resident_wall_ms_median_min': t_eval['resident'],
        'evaluate_host_collated_wall_ms_median_min': t_eval['host_collated'],
        'prediction_path_wall_ms_median_min': t_eval['prediction_path'],
        'prediction_share_of_resident_call': t_eval['prediction_path'][0] / t_eval['resident'][0],
        'host_collated_over_resident_median': t_eval['host_collated'][0] / t_eval['resident'][0],
        'epoch_batches': -(-B // 100),
        'epoch_device_collate_wall_ms_median_min': t_loop['device_collate'],
        'epoch_host_collate_wall_ms_median_min': t_loop['host_collate'],
        'host_over_device_epoch_median': t_loop['host_collate'][0] / t_loop['device_collate'][0],
    }


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: there is nothing to measure without one'
    for B in (100, 1000):
        line = json.dumps(case(B, a.reps))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')
