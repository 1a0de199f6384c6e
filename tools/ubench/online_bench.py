"""Online filtering against what the same answer costs on the batch route.

    python tools/ubench/online_bench.py [--out profiles/online_bench.jsonl] [--kernels generic]

Per shape (demo: d = 1, H = 10, delta_t = 0.01; PhysioNet: d = H = 41, delta_t = 0.016 / 48) and
per number of resident series N = 1, 50, 1 000, one line with

* ``observe`` when the target is 1 Euler step ahead and when it is 30 steps ahead, every series of
  the state in one call, and ``predict`` with Q = 8 queries 4 steps apart: GPU time between HIP
  events on the current stream (the kernel and the upload of ids and times in front of it), and
  the wall clock around a device synchronise (what a caller waits for: host checks included);
  ``step_us`` = (observe 30 - observe 1) / 29 of the GPU medians -- a lone wave is latency-bound,
  so read it against the 0.27 / 0.63 us per Euler step of the wave-per-path kernels;
* the yardstick, code this feature does not touch: ``NJODE.get_pred`` over the series' full
  history on [0, 1] (100 Euler steps for the demo shape, 3 000 for PhysioNet), which is what an
  answer to "what do you predict now?" costs without a resident state.

``--kernels generic``: the shape-generic family (``NJODE.online(..., kernels='generic')``) on the
shapes the wave family refuses -- width 100 (d = 1, H = 10, delta_t = 0.01), the climate shape
(d = 5, H = 50, width 400, masked; 400 grid steps of history) and ``gru_w80`` (width 80 with the GRU
jump) -- with the same measurements; there ``step_us`` is the cost of one Euler step of a whole
TILE (a workgroup), to be read against k_gen_fwd's 13 100 cycles per step at width 100;
``tables_pack_*`` is one repack of the fragment tables, what the call after a parameter change pays.

``--run``: runs of events (``observe_many``) instead.  Per shape and N, K = 8 and K = 64 observations
per series, one Euler step apart, as ONE ``observe_many`` against K ``observe`` calls in the same
process (HIP events and wall clock, as above), and the warm start from the shape's history:
``reset`` + ``replay(fused=True)`` against ``reset`` + ``replay()`` against ``get_pred``.

One process, warm-up calls first, medians (and the fastest call) after them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from njode_amd import data_utils, models, synthetic_physionet  # noqa: E402

NN = ((50, 'tanh'), (50, 'tanh'))


def med_min(ms):
    return [float(np.median(ms)), float(np.min(ms))]


def timed(fn, warmup, reps):
    """(GPU ms between events, wall ms around a synchronise), median and minimum of each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    gpu, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        gpu.append(a.elapsed_time(b))
    return med_min(gpu), med_min(wall)


def history(shape, N):
    """(model, batch, delta_t, T) of ``N`` series observed on [0, 1]."""
    torch.manual_seed(0)
    if shape == 'demo':
        import copy
        hp = copy.deepcopy(data_utils.hyperparam_default)
        hp.update(nb_paths=N, nb_steps=100, obs_perc=0.1)
        paths, obs, nb_obs, meta = data_utils.create_dataset('BlackScholes', hp, seed=0)
        b = data_utils.collate_arrays(paths, obs, nb_obs, meta['dt'])
        m = models.NJODE(1, 10, 1, NN, NN, NN, False, options={'device_outputs': True})
        return m.to('cuda').eval(), b, meta['dt'], meta['maturity']
    if shape in ('w100', 'gru_w80'):
        w = 100 if shape == 'w100' else 80
        nn = ((w, 'tanh'), (w, 'tanh'))
        m, b, dt, T = history('demo', N)
        torch.manual_seed(0)
        m = models.NJODE(1, 10, 1, nn, nn, nn, shape == 'gru_w80', options={'device_outputs': True})
        return m.to('cuda').eval(), b, dt, T
    if shape == 'climate':
        nn = ((400, 'tanh'), (400, 'tanh'))
        b = synthetic_physionet.make_batch(batch_size=N, dim=5, n_grid=400, seed=0)
        m = models.NJODE(5, 50, 5, nn, nn, nn, False, options={'device_outputs': True, 'masked': True})
        return m.to('cuda').eval(), b, b['delta_t'], b['T']
    b = synthetic_physionet.make_batch(batch_size=N, n_grid=3000, seed=0)
    m = models.NJODE(41, 41, 41, NN, NN, NN, False, options={'device_outputs': True, 'masked': True})
    return m.to('cuda').eval(), b, b['delta_t'], b['T']


def case(shape, N, reps, kernels='wave'):
    m, b, delta_t, T = history(shape, N)
    d = b['start_X'].shape[1]
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    M = dev.get('M')

    def get_pred():
        return m.get_pred(dev['times'], dev['time_ptr'], dev['X'], dev['obs_idx'], delta_t, T, dev['start_X'], M=M)

    st = m.online(N, delta_t, kernels=kernels)
    st.reset(dev['start_X'])
    st.replay(b['times'], b['time_ptr'], dev['X'], b['obs_idx'], M)      # a warm start from the history
    st.check()
    X = torch.rand(N, d, device='cuda')
    Mo = (torch.rand(N, d, device='cuda') < 0.15).float() if M is not None else None
    clock = {'t': float(T)}

    def observe(k):
        def fn():
            clock['t'] += k * delta_t
            st.observe(np.full(N, clock['t']), X, Mo)
        return fn

    def predict():
        q = clock['t'] + 4 * delta_t * np.arange(1, 9)
        st.predict(np.broadcast_to(q, (N, 8)))

    # the routes alternate so that none owns a quieter stretch of the machine
    res = {'obs1': [], 'obs30': [], 'pred8': [], 'get_pred': []}
    for rnd in range(2):
        w = 3 if rnd == 0 else 0
        res['obs1'].append(timed(observe(1), w, reps))
        res['obs30'].append(timed(observe(30), w, reps))
        res['pred8'].append(timed(predict, w, reps))
        res['get_pred'].append(timed(get_pred, 2 if rnd == 0 else 0, max(reps // 8, 3)))
    st.check()
    pack = None
    if st.kernels == 'generic':      # what a change of the parameters costs the next call: one k_gen_pack launch
        def repack():
            st._tables_stamp = None
            st._ensure_tables(m)
        pack = timed(repack, 3, reps)
    best = {k: min(v, key=lambda r: r[0][0]) for k, v in res.items()}      # the quieter round
    g1, g30 = best['obs1'][0][0], best['obs30'][0][0]
    return {
        'case': 'online {} N={}'.format(shape, N), 'shape': shape, 'kernels': st.kernels, 'N': N, 'delta_t': delta_t,
        'history_euler_steps': int(round(T / delta_t)), 'history_rows': int(b['time_ptr'][-1]),
        'observe_1_step_gpu_ms_median_min': best['obs1'][0], 'observe_1_step_wall_ms_median_min': best['obs1'][1],
        'observe_30_steps_gpu_ms_median_min': best['obs30'][0],
        'observe_30_steps_wall_ms_median_min': best['obs30'][1],
        'predict_q8_32_steps_gpu_ms_median_min': best['pred8'][0],
        'predict_q8_32_steps_wall_ms_median_min': best['pred8'][1],
        'step_us': (g30 - g1) / 29.0 * 1e3,
        'get_pred_full_history_gpu_ms_median_min': best['get_pred'][0],
        'get_pred_full_history_wall_ms_median_min': best['get_pred'][1],
        'get_pred_over_observe_1_step_wall': best['get_pred'][1][0] / best['obs1'][1][0],
        'both_rounds_gpu_ms_median': {k: [r[0][0] for r in v] for k, v in res.items()},
        'tables_bytes': st._tables_bytes,
        'tables_pack_gpu_ms_median_min': pack[0] if pack else None,
        'tables_pack_wall_ms_median_min': pack[1] if pack else None,
    }


def run_case(shape, N, reps, kernels='wave'):
    m, b, delta_t, T = history(shape, N)
    d = b['start_X'].shape[1]
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    M = dev.get('M')

    def get_pred():
        return m.get_pred(dev['times'], dev['time_ptr'], dev['X'], dev['obs_idx'], delta_t, T, dev['start_X'], M=M)

    st = m.online(N, delta_t, kernels=kernels)

    def warm_start(fused):
        def fn():
            st.reset(dev['start_X'])
            st.replay(b['times'], b['time_ptr'], dev['X'], b['obs_idx'], M, fused=fused)
        return fn

    few = max(reps // 8, 3)
    res = {'replay_loop': [], 'replay_fused': [], 'get_pred': []}
    for rnd in range(2):
        w = 1 if rnd == 0 else 0
        res['replay_fused'].append(timed(warm_start(True), w, few))
        res['replay_loop'].append(timed(warm_start(False), w, few))
        res['get_pred'].append(timed(get_pred, 2 * w, few))
    st.check()
    clock = {'t': float(T)}
    out = {}
    for K in (8, 64):
        X = torch.rand(N * K, d, device='cuda')
        Mo = (torch.rand(N * K, d, device='cuda') < 0.15).float() if M is not None else None
        Xs = X.view(N, K, d).transpose(0, 1).contiguous()        # [K][N][d]: call k of the loop
        Ms = Mo.view(N, K, d).transpose(0, 1).contiguous() if Mo is not None else None
        ev_ptr = np.arange(N + 1) * K

        def one_run():
            t = clock['t'] + delta_t * np.arange(1, K + 1)
            clock['t'] = float(t[-1])
            st.observe_many(ev_ptr, np.tile(t, N), X, Mo)

        def k_calls():
            for k in range(K):
                clock['t'] += delta_t
                st.observe(np.full(N, clock['t']), Xs[k], None if Ms is None else Ms[k])

        r = {'run': [], 'calls': []}
        for rnd in range(2):
            w = 3 if rnd == 0 else 0
            r['run'].append(timed(one_run, w, reps))
            r['calls'].append(timed(k_calls, w, max(reps // 4, 3)))
        st.check()
        best = {k: min(v, key=lambda x: x[0][0]) for k, v in r.items()}
        out['run_k{}_gpu_ms_median_min'.format(K)] = best['run'][0]
        out['run_k{}_wall_ms_median_min'.format(K)] = best['run'][1]
        out['calls_k{}_gpu_ms_median_min'.format(K)] = best['calls'][0]
        out['calls_k{}_wall_ms_median_min'.format(K)] = best['calls'][1]
        out['calls_over_run_k{}_wall'.format(K)] = best['calls'][1][0] / best['run'][1][0]
    best = {k: min(v, key=lambda x: x[0][0]) for k, v in res.items()}
    out.update({
        'case': 'online run {} N={}'.format(shape, N), 'shape': shape, 'kernels': st.kernels, 'N': N, 'delta_t': delta_t,
        'history_euler_steps': int(round(T / delta_t)), 'history_rows': int(b['time_ptr'][-1]),
        'history_slices_with_rows': int(np.count_nonzero(np.diff(np.asarray(b['time_ptr'])))),
        'replay_loop_gpu_ms_median_min': best['replay_loop'][0], 'replay_loop_wall_ms_median_min': best['replay_loop'][1],
        'replay_fused_gpu_ms_median_min': best['replay_fused'][0],
        'replay_fused_wall_ms_median_min': best['replay_fused'][1],
        'get_pred_full_history_gpu_ms_median_min': best['get_pred'][0],
        'get_pred_full_history_wall_ms_median_min': best['get_pred'][1],
        'replay_loop_over_fused_wall': best['replay_loop'][1][0] / best['replay_fused'][1][0],
        'replay_fused_over_get_pred_wall': best['replay_fused'][1][0] / best['get_pred'][1][0],
    })
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--run', action='store_true', help='measure runs of events (observe_many, fused replay)')
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--kernels', default='wave', choices=('wave', 'generic'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: there is nothing to measure without one'
    for shape in (('demo', 'physionet') if a.kernels == 'wave' else ('w100', 'climate', 'gru_w80')):
        for N in (1, 50, 1000):
            line = json.dumps((run_case if a.run else case)(shape, N, a.reps, a.kernels))
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, 'a') as f:
                    f.write(line + '\n')
