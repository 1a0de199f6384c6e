"""The record collate against the training step it feeds, and the PhysioNet protocol call with
held-out arrays that never leave the GPU.

    python tools/ubench/records_bench.py [--out profiles/records_bench.jsonl]

One process, warm-up calls first, medians (and the fastest call) after them.  GPU work is timed
with HIP events on the current stream; calls that end in a host wait of their own
(``prepare_batches``, ``collate_host`` + upload, the protocol call) with the wall clock around a
device synchronise -- each figure says which.

Case 1, per batch size B = 50 and B = 800, on a PhysioNet-shaped store (8 000 records of 30-100
rows, 41 features, 3 001 grid points): ``prepare_batches`` for one epoch, ``fill_batch`` per
batch, ``collate_host`` + upload per batch, and -- the yardstick, code that the record collate
does not touch -- the training step ``model.loss_and_grad`` on that batch (3 000 Euler steps).
``fill_over_step`` is the fraction the per-batch device collate adds to the step.

Case 2, B = 800: ``physionet_eval.evaluate_model_device`` on the batch of
``tools/ubench/protocol_bench.py`` (held-out arrays in pageable host memory: the yardstick), on a
host-collated test-layout batch of the store (the same route), and on the device-collated one
(held-out arrays resident).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from njode_amd import models, physionet_eval, records, synthetic_physionet  # noqa: E402

NN = ((50, 'tanh'), (50, 'tanh'))
DT, T = synthetic_physionet.PHYSIONET_DELTA_T, synthetic_physionet.PHYSIONET_T
# the reference's own variable_time_collate_fn1 on records of this shape, measured on a CPU
REFERENCE_COLLATE_CPU_S = {50: {'train': 0.49}, 800: {'train': 8.2, 'test': 4.6}}
ds_test_prep = {}     # B -> a prepared test-layout batch of the first B records


def med_min(ms):
    return [float(np.median(ms)), float(np.min(ms))]


def timed_events(fn, warmup, reps):
    """GPU time of ``fn``'s work on the current stream, HIP events around each call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return med_min(out)


def timed_wall(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return med_min(out)


def model_41(train):
    torch.manual_seed(0)
    m = models.NJODE(41, 41, 41, NN, NN, NN, False, dropout_rate=0.1 if train else 0.0,
                     options={'device_outputs': True, 'masked': True}).to('cuda')
    return m.train() if train else m.eval()


def upload(b):
    return {'X': b['X'].cuda(), 'M': b['M'].cuda(), 'obs_idx': b['obs_idx'].cuda().int(),
            'n_obs_ot': b['n_obs_ot'].cuda().int(), 'start_X': b['start_X'].cuda()}


def collate_case(ds, B, reps):
    model = model_41(train=True)
    order = np.random.RandomState(B).permutation(ds.n_records)
    lists = [order[i:i + B] for i in range(0, len(order), B)]
    preps = ds.prepare_batches(lists, 'train')
    state = {'i': 0}

    def fill():
        state['i'] = (state['i'] + 1) % len(preps)
        return ds.fill_batch(preps[state['i']])

    batch = ds.fill_batch(preps[0])

    def step():
        model.loss_and_grad(batch['times'], batch['time_ptr'], batch['X'], batch['obs_idx'], DT, T,
                            batch['start_X'], batch['n_obs_ot'], M=batch['M'])

    t_prepare = timed_wall(lambda: ds.prepare_batches(lists, 'train'), 1, max(reps // 4, 3))
    t_fill = timed_events(fill, 3, reps)
    t_fill_wall = timed_wall(fill, 1, reps)
    t_fill_test = timed_events(lambda: ds.fill_batch(ds_test_prep[B]), 2, reps) if B in ds_test_prep else None
    t_host = timed_wall(lambda: upload(ds.collate_host(lists[0], 'train')), 1, max(reps // 4, 3))
    t_step = timed_events(step, 3, reps)
    return {
        'case': 'record collate B={}'.format(B), 'B': B, 'dim': ds.dim, 'n_records': ds.n_records,
        'n_grid': ds.n_grid, 'rows': int(batch['time_ptr'][-1]), 'union_times': len(batch['times']),
        'empty_slices': int((np.diff(batch['time_ptr']) == 0).sum()), 'batches_per_epoch': len(lists),
        'prepare_batches_per_epoch_wall_ms_median_min': t_prepare,
        'fill_batch_gpu_ms_median_min': t_fill,
        'fill_batch_wall_ms_median_min': t_fill_wall,
        'fill_batch_test_layout_gpu_ms_median_min': t_fill_test,
        'collate_host_plus_upload_wall_ms_median_min': t_host,
        'train_step_gpu_ms_median_min': t_step,
        'fill_over_step': t_fill[0] / t_step[0],
        'prepare_per_batch_over_step': t_prepare[0] / len(lists) / t_step[0],
        'host_collate_over_step': t_host[0] / t_step[0],
        'reference_collate_cpu_s_per_batch': REFERENCE_COLLATE_CPU_S[B],
        'reference_collate_note': "the reference's variable_time_collate_fn1 on a CPU, not a GPU figure",
    }


def protocol_case(ds, B, reps):
    model = model_41(train=False)
    yard = physionet_eval.make_eval_batch(batch_size=B, n_grid=3000)
    idx = np.arange(B)
    on_host = ds.collate_host(idx, 'test')
    on_dev = ds.fill_batch(ds_test_prep[B])
    call = lambda b: (lambda: physionet_eval.evaluate_model_device(model, [b], 'cuda', DT, T))  # noqa: E731
    r_host, r_dev = call(on_host)(), call(on_dev)()
    assert r_host == r_dev, (r_host, r_dev)

    def pred_only():
        with torch.no_grad():
            return model(on_dev['times'], on_dev['time_ptr'], on_dev['X'], on_dev['obs_idx'], DT, T,
                         on_dev['start_X'], on_dev['n_obs_ot'], until_T=True, return_path=True,
                         get_loss=True, M=on_dev['M'])[4]

    # the routes alternate so that none owns a quieter stretch of the machine
    t = {'yard': [], 'host': [], 'dev': []}
    for rnd in range(2):
        t['yard'].append(timed_wall(call(yard), 2 if rnd == 0 else 0, reps))
        t['host'].append(timed_wall(call(on_host), 1 if rnd == 0 else 0, reps))
        t['dev'].append(timed_wall(call(on_dev), 2 if rnd == 0 else 0, reps))
    t_pred = timed_wall(pred_only, 2, reps)
    held = 2 * 4 * B * len(on_dev['times_val']) * ds.dim
    return {
        'case': 'physionet protocol B={} n_grid=3000'.format(B), 'B': B, 'dim': ds.dim,
        'held_out_times': len(on_dev['times_val']), 'held_out_bytes': held,
        'yardstick_held_out_times': len(yard['times_val']),
        'result_host_collated': list(r_host), 'result_device_collated': list(r_dev),
        'prediction_path_wall_ms_median_min': t_pred,
        'yardstick_protocol_bench_batch_wall_ms_median_min': t['yard'],
        'host_collated_wall_ms_median_min': t['host'],
        'device_collated_wall_ms_median_min': t['dev'],
        'yardstick_over_device_collated_median': min(x[0] for x in t['yard']) / max(x[0] for x in t['dev']),
        'host_collated_over_device_collated_median': min(x[0] for x in t['host']) / max(x[0] for x in t['dev']),
    }


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--records', type=int, default=8000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: there is nothing to measure without one'
    recs, mn, mx = synthetic_physionet.make_records(a.records, 41, n_quant=3000, n_obs_range=(30, 100),
                                                    zero_mask_rows=True, seed=0)
    recs[1] = recs[2]         # (record 1 has no observed feature: its loss term would be 0 / 0)
    ds = records.RecordDataset.from_records(recs, mn, mx, device='cuda')
    ds_test_prep[800] = ds.prepare_batches([np.arange(800)], 'test')[0]
    for case, B, reps in ((collate_case, 50, 40), (collate_case, 800, 12), (protocol_case, 800, 3)):
        r = case(ds, B, reps)
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')
