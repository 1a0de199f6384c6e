"""Dropout training steps against float64, with the kernels' own masks.

The keep masks are a pure function of (call seed, global path id, time key, network, layer, unit):
oracle/dropout_oracle.py restates the three word streams the kernels draw from and the key
schedule (its docstring holds the table of which stream each route draws per network), and
oracle/njode_oracle.py takes them as a mask source in place of F.dropout.  So a dropout step is
compared deterministically with the float64 oracle of the SAME step, by the route matrix's rule
(hip_util.check_vs_oracle): err(HIP, f64) <= max(2 err(o32, f64), floor) for the loss, hT and every
gradient tensor, of the fused step (loss_and_grad) and of the autograd route (forward + backward,
C_ROWS_IN_FWD).  A mask drawn with the wrong key, layer, stream or scale moves the loss by O(p),
far above fp32 rounding.

Rows: every route of every compiled shape at p = 0.1 (test_hip_route_matrix's route table; its
`large` batch is the mixed route of the headline step), the VALU kernels (NJODE_ODE=valu), the
shape-generic kernels on both plans (width 100, depth 1 / 8, three differing networks with one of
depth 0, an odd width, width 1 024, use_rnn, masked data), and the edges: p = 0.5 / 0.9, a p whose
fp32 rounding decides thr16, a p > 0 with thr16 = 0, a seed with both halves nonzero, a path id
offset >= 2^32, two shards that add up to the whole batch, return_path in a training call
(path_h, path_y: the NET_DEC_ROW masks), a gradient through hT, a prefetched plan, K = 4 097.
nn_desc=None shapes draw no mask and must give the p = 0 result bit for bit.

Worst measured err(HIP, f64) / err(o32, f64) per family (MI355X; a ratio above 2 passes on the
floor, where both errors are at fp32 rounding): wave per item 6.08, split <= 384 tiles 4.94, split
385-768 tiles 1.00, mixed 6.86, one-wave tiles (mfma1) 6.10, one-wave shapes 8.09 / 3.06 / 6.33 (one
tile / small / large batch), VALU 6.27, GRU 7.76 / 3.97 (small / large), wave per path 2.60, four-wave
tiles 3.49, nn_desc=None 3.56, shape-generic 2.68, p = 0.5 1.15, p = 0.9 2.99, shards 1.86, return_path
1.49, hT gradient 1.66, K = 4 097 1.86.  The mixed route of the shape without residual maps (loss 16)
passes only on LARGE_FLOOR_G: its ODE gradients sit at 2.9e-5 relative L2 where the fp32 oracle's sit
at 5e-6 to 9e-6 (ratio 3 to 5, the same for all six ODE tensors; its loss matches to 1e-8: no mask is
off).  The module takes about 25 s: the oracle (about 23 s) runs while the children do.
"""
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest
import torch

import hip_util
import test_hip_generic_envelope as GE
import test_hip_route_matrix as RM
from hip_util import exact_k_batch, hip_model, kernel_names, oracle_pair
from njode_amd.build import CONFIGS, RELU
from oracle import dropout_oracle as do

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)

P = 0.1
STEP = 7                       # the model's step counter at every call of a row
DEMO = CONFIGS[0]
RELU20 = next(c for c in CONFIGS if c[5] == RELU)
ENVS = dict(RM.ENVS, valu={'NJODE_ODE': 'valu'})
# the VALU segment-plan kernels (njode_kernels.h)
VALU = ['k_encode_rows', 'k_ode_fwd_items', 'k_jump_rows', 'k_jump_rows_bwd', 'k_ode_bwd_items',
        'k_encode_rows_bwd']
P_FP32 = (6553.5 - 1e-7) / 65536.0      # float64 p 65536 + 0.5 truncates to 6553, fp32 to 6554
P_TINY = 5e-6                            # p > 0, thr16 = 0
# gradient floor (relative L2) of the `large` batch (900 paths, ~34 000 observation rows): measured, see
# the docstring
LARGE_FLOOR_G = 5e-5


def _w(n, act='tanh', layers=2):
    return tuple((n, act) for _ in range(layers))


# shape-generic rows: name -> (config, batch = (B, K, observations per path, masked?))
GEN = {
    'w100': (GE._cfg(1, 10, _w(100), _w(100), _w(100)), (17, 50, 4, False)),
    # depth 8 (every layer index of drop_word), depth 1, depth 0 (no mask), differing widths
    'deep8_1_0': (GE._cfg(1, 10, _w(40, 'tanh', 8), _w(33, 'relu', 1), None), (17, 40, 4, False)),
    'odd51': (GE._cfg(1, 10, _w(51), _w(51, 'relu'), _w(51)), (17, 40, 4, False)),
    'w1024': (GE._cfg(1, 10, _w(1024, layers=1), _w(1024, layers=1), _w(1024, layers=1)), (9, 30, 3, False)),
    'gru_h252': (GE._cfg(1, 252, _w(50), _w(50), _w(50), rnn=True), (9, 30, 3, False)),
    'masked_d20': (GE._cfg(20, 20, _w(40), _w(40), _w(40), masked=True), (17, 40, 3, True)),
}


def gen_batch(name):
    cfg, (B, K, n_obs, masked) = GEN[name]
    d = cfg['input_size']
    if masked:
        from njode_amd import synthetic_physionet
        b = synthetic_physionet.make_batch(batch_size=B, dim=d, n_grid=K, n_obs_range=(2, n_obs + 3), seed=B + d)
        return b, b['delta_t'], b['T']
    return exact_k_batch(B, K, obs_per_path=n_obs, seed=B * 7 + K + d, d=d)


SHARD_B, SHARD_B1, SHARD_K = 24, 10, 100


def shard_batch(lo, hi):
    """Paths lo .. hi - 1 of one demo batch on the 2^-10 grid; paths 0 and SHARD_B1 are observed at the
    last grid point, so each shard and the whole batch walk the same Euler steps (same time keys)."""
    from njode_amd import data_utils
    rng = np.random.RandomState(17)
    dt = 2.0 ** -10
    obs = np.zeros((SHARD_B, SHARD_K + 1), dtype=np.int64)
    for p in range(SHARD_B):
        obs[p, 1 + rng.choice(SHARD_K, size=4, replace=False)] = 1
    obs[0, SHARD_K] = obs[SHARD_B1, SHARD_K] = 1
    paths = np.cumsum(rng.normal(0.0, 0.05, size=(SHARD_B, 1, SHARD_K + 1)), axis=2) + 1.0
    b = data_utils.collate_arrays(paths[lo:hi], obs[lo:hi], obs[lo:hi, 1:].sum(axis=1), dt)
    return b, dt, SHARD_K * dt


def job_model_cfg(job):
    p = job['p']
    if isinstance(job['shape'], str):
        cfg = dict(GEN[job['shape']][0], dropout_rate=p)
    else:
        cfg = RM.model_cfg(tuple(job['shape']), p)
    cfg['options'] = dict(cfg['options'], dropout_seed=job.get('dseed', 0))
    return cfg


def job_state_dict(job):
    from njode_amd import models
    if isinstance(job['shape'], str):
        torch.manual_seed(11)
        cfg = GEN[job['shape']][0]
    else:
        torch.manual_seed(0)
        cfg = RM.model_cfg(tuple(job['shape']))
    return {k: v.detach().clone() for k, v in models.NJODE(**cfg).state_dict().items()}


def job_batch(job):
    kind = job['batch']
    if kind == 'gen':
        return gen_batch(job['shape'])
    if kind == 'shard':
        return shard_batch(*job['shard'])
    if kind == 'K4097x6':   # (six paths: the oracle of 4 097 steps is the costly part)
        return exact_k_batch(6, 4097, obs_per_path=3, seed=4097 % 97)
    return RM.make_batch(kind, tuple(job['shape']))


def c_hT(B, H):
    """the weight of hT in the objective of a gradient-through-hT row"""
    return (0.3 * np.cos(np.arange(B * H, dtype=np.float64) * 0.7)).reshape(B, H).astype(np.float32)


# ---- child side --------------------------------------------------------------------------------------
def _child(jobs, out_dir):
    meta = {}
    for job in jobs:
        b, dt, T = job_batch(job)
        m = hip_model(job_model_cfg(job), job_state_dict(job)).train()
        if job.get('offset'):
            m.dp_path_offset = int(job['offset'])
        if job.get('gb'):
            m.dp_global_batch = int(job['gb'])
        if job.get('plan') == 'lock':
            os.environ['NJODE_GEN_PLAN'] = 'lock'
        else:
            os.environ.pop('NJODE_GEN_PLAN', None)
        M = b['M'].cuda() if 'M' in b else None
        args = (b['times'], b['time_ptr'], b['X'].cuda(), b['obs_idx'].cuda().int(), dt, T,
                b['start_X'].cuda(), b['n_obs_ot'].cuda().int())
        res, info = {}, {'n_obs': int(b['time_ptr'][-1])}
        m._step_counter = STEP
        (_, loss), names = kernel_names(lambda: m.loss_and_grad(*args, M=M))
        res.update(loss_fused=float(loss), grad_fused=m.flat_grad().cpu().numpy().astype(np.float64))
        m._step_counter = STEP
        m.zero_grad()
        cw = torch.from_numpy(c_hT(len(b['start_X']), m.hidden_size)).cuda() if job.get('c_hT') else None

        def autograd_step():
            hT, loss2 = m(*args, M=M)
            (loss2 if cw is None else loss2 + (cw * hT).sum()).backward()
            return hT, loss2
        (hT, loss2), names2 = kernel_names(autograd_step)
        res['loss_auto'] = float(loss2)
        res['grad_auto'] = np.concatenate([p.grad.detach().cpu().numpy().ravel() for p in m.parameters()])
        res['hT'] = hT.detach().cpu().numpy().astype(np.float64)
        for k, p in m.named_parameters():
            res['g.' + k] = p.grad.detach().cpu().numpy().astype(np.float64)
        info.update(names=names, names_auto=names2)
        if job.get('prefetch'):
            m._step_counter = STEP
            m._plans.clear()
            m.prefetch_plan(*args, M=M, need_hT=False)
            (_, loss3), names3 = kernel_names(lambda: m.loss_and_grad(*args, M=M))
            res['loss_prefetch'] = float(loss3)
            res['grad_prefetch'] = m.flat_grad().cpu().numpy().astype(np.float64)
            info['names_prefetch'] = names3
        if job.get('predict'):
            # return_path in a TRAINING call: the path-output rows draw their own masks (NET_DEC_ROW)
            m._step_counter = STEP
            with torch.no_grad():
                out, names4 = kernel_names(lambda: m(*args, M=M, return_path=True))
            res['path_h'] = out[3].cpu().numpy().astype(np.float64)
            res['path_y'] = out[4].cpu().numpy().astype(np.float64)
            res['loss_path'] = float(out[1])
            info['names_predict'] = names4
        np.savez(os.path.join(out_dir, job['id'] + '.npz'), **res)
        meta[job['id']] = info
    with open(os.path.join(out_dir, 'meta.json'), 'w') as f:
        json.dump(meta, f)


_SNIPPET = r'''
import json, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {repo!r})
import test_hip_dropout_f64 as T
T._child(json.load(open({jobs!r})), {out!r})
'''


def run_child(tmp_path, tag, env, jobs, timeout=240):
    out = tmp_path / tag
    out.mkdir()
    with open(out / 'jobs.json', 'w') as f:
        json.dump(jobs, f)
    t0 = time.time()
    p = subprocess.run([sys.executable, '-c', _SNIPPET.format(tests=TESTS, repo=REPO, jobs=str(out / 'jobs.json'),
                                                               out=str(out))],
                       env=dict(os.environ, **env), cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=timeout)
    assert p.returncode == 0, (tag, p.stdout[-4000:])
    print('child {}: {} jobs, {:.1f} s'.format(tag, len(jobs), time.time() - t0))
    with open(out / 'meta.json') as f:
        meta = json.load(f)
    return {j['id']: (dict(np.load(out / (j['id'] + '.npz'))), meta[j['id']]) for j in jobs}


# ---- parent side: the masked oracle --------------------------------------------------------------------
def stream_of(job):
    """the stream the row's kernels draw (oracle/dropout_oracle.py's table); None: no hidden layer"""
    if isinstance(job['shape'], str):
        return 'gen'
    c = tuple(job['shape'])
    if c[3] == 0:
        return None
    if job['env'] == 'valu' or c[9]:     # NJODE_ODE=valu; use_rnn shapes run the VALU lockstep kernels
        return 'valu'
    return 'mc'


_ORACLE = {}
ORACLE_S = [0.0]


def truth(job, whole=None):
    """(f32, f64) masked-oracle results of a row (``whole``: the job of the whole batch, for shards)."""
    j = whole or job
    stream = stream_of(j)
    key = (json.dumps(j['shape']), j['batch'], j['p'], j.get('dseed', 0), j.get('offset', 0), bool(j.get('c_hT')),
           bool(j.get('predict')), stream)
    if key not in _ORACLE:
        t0 = time.time()
        b, dt, T = job_batch(j)
        masks = None if stream is None else do.KernelMasks(stream, do.call_seed(j.get('dseed', 0), STEP), j['p'],
                                                           gid0=j.get('offset', 0))
        kw = {}
        if j.get('c_hT'):
            kw['c_hT'] = c_hT(len(b['start_X']), job_model_cfg(j)['hidden_size'])
        _ORACLE[key] = oracle_pair(job_model_cfg(j), job_state_dict(j), b, dt, T, predict=bool(j.get('predict')),
                                   masks=masks, **kw)
        ORACLE_S[0] += time.time() - t0
    return _ORACLE[key]


RATIOS = {}


def check_row(job, res, info, family, must=(), must_not=(), floor_h=2e-6, floor_g=1e-5):
    jid = job['id']
    if isinstance(job['shape'], str):
        GE._check_names(jid, info['names'], job.get('plan') or 'seg')
        GE._check_names(jid + ' (autograd)', info['names_auto'], job.get('plan') or 'seg')
    else:
        RM.check_names(jid, info['names'], must, must_not)
        RM.check_names(jid + ' (autograd)', info['names_auto'],
                       [m for m in must if 'dw_stored' not in m and 'dw_pairs' not in m], must_not)
    if stream_of(job) is not None:
        assert res['loss_fused'] > 0 and np.isfinite(res['grad_fused']).all(), jid
    o32, o64 = truth(job)
    if job.get('c_hT'):
        # (the fused step has no hT term: only its loss is compared; the autograd step is the gradient)
        l64 = o64['loss']
        assert abs(res['loss_fused'] - l64) <= max(2 * abs(o32['loss'] - l64), 1e-6 * abs(l64)), jid
        res = dict(res, loss_fused=res['loss_auto'], grad_fused=res['grad_auto'])
    hip_util.check_vs_oracle(jid, o32, o64, res, RATIOS, family, floor_h, floor_g)
    if 'loss_prefetch' in res:
        assert res['loss_prefetch'] == res['loss_fused'] and np.array_equal(res['grad_prefetch'], res['grad_fused'])
    if job.get('predict'):
        # a training call with return_path: the lockstep plan (the wave-per-path kernels leave it to
        # the four-wave kernels when dropout is on)
        RM.check_names(jid + ' (return_path)', info['names_predict'],
                       ['k_paths_fwd_mfma'] if stream_of(job) == 'mc' else [], RM.ITEMS + RM.MIXED + ['k_paths_fwd_chain'])
        pr = {'hT': res['hT'], 'path_h': res['path_h'], 'path_y': res['path_y']}
        hip_util.check_vs_oracle(jid + ' (return_path)', o32, o64, pr, RATIOS, family + ' return_path', floor_h,
                                 floor_g, predict=True)
        l64 = o64['loss']
        assert abs(res['loss_path'] - l64) <= max(2 * abs(o32['loss'] - l64), 1e-6 * abs(l64)), (jid, 'loss_path')


def _job(jid, env, shape, batch, p=P, **kw):
    return dict(id=jid, env=env, shape=list(shape) if not isinstance(shape, str) else shape, batch=batch, p=p, **kw)


def route_jobs():
    """every route of every compiled shape at p = 0.1, with (must, must_not) kernel names"""
    out = []
    for i, c in enumerate(CONFIGS):
        for name, env, kind, must, must_not in RM.routes(c):
            if name == 'split768' and c != DEMO:   # (the oracle of 1 000 paths: once is enough)
                continue
            out.append((_job('c{}_{}'.format(i, name), env, c, kind), name, must, must_not))
        if c in (DEMO, RELU20):
            # the VALU kernels of the segment plan
            out.append((_job('c{}_valu'.format(i), 'valu', c, 'small'), 'valu', VALU,
                        RM.ITEMS + RM.MIXED + RM.ONE_WAVE))
    return out


def edge_jobs():
    small = lambda jid, **kw: (_job(jid, 'default', DEMO, 'small', **kw), jid, RM.ITEMS, RM.MIXED)
    out = [small('p50', p=0.5), small('p90', p=0.9), small('p_fp32', p=P_FP32), small('p_tiny', p=P_TINY),
           small('seed_hi', dseed=0x2545F4914F6CDD1D), small('offset_2_32', offset=2 ** 32 + 5),
           small('hT_grad', c_hT=True), small('prefetch', prefetch=True),
           # a training call with return_path: the lockstep plan and its NET_DEC_ROW masks
           (_job('path_demo', 'default', DEMO, 'small', predict=True), 'path_demo', RM.ITEMS, RM.MIXED),
           (_job('K4097', 'default', DEMO, 'K4097x6'), 'K4097', RM.ONE_WAVE, RM.ITEMS + RM.MIXED)]
    physio = RM.PHYSIO
    out.append((_job('path_physio', 'default', physio, 'physio', predict=True), 'path_physio',
                ['k_paths_fwd_chain'], ['k_paths_fwd_mfma']))
    return out


def gen_jobs():
    out = []
    for name in GEN:
        # (masked and use_rnn shapes run the lockstep plan only)
        for plan in ('lock',) if GEN[name][0]['use_rnn'] or GEN[name][0]['options'].get('masked') else ('seg', 'lock'):
            predict = name in ('w100', 'deep8_1_0') and plan == 'lock'
            out.append(_job('gen_{}_{}'.format(name, plan), 'default', name, 'gen', plan=plan, predict=predict))
    return out


def test_dropout_steps_against_float64_with_the_kernels_masks(tmp_path):
    t_start = time.time()
    routes = route_jobs()
    edges = edge_jobs()
    gens = gen_jobs()
    shards = [_job('shard0', 'default', DEMO, 'shard', shard=[0, SHARD_B1], gb=SHARD_B),
              _job('shard1', 'default', DEMO, 'shard', shard=[SHARD_B1, SHARD_B], offset=SHARD_B1, gb=SHARD_B)]
    whole = _job('whole', 'default', DEMO, 'shard', shard=[0, SHARD_B])
    # nn_desc=None shapes: p = 0.1 must be the p = 0 call bit for bit
    linear = [j for j, *_ in routes if j['shape'][3] == 0]
    linear0 = [dict(j, id=j['id'] + '_p0', p=0.0) for j in linear]
    jobs = {env: [] for env in ENVS}
    for j, *_ in routes + edges:
        jobs[j['env']].append(j)
    jobs['default'] += gens + shards + [whole] + linear0
    # the children run one after another on the GPU while this process computes the oracle
    got, child_err = {}, []

    def children():
        try:
            for env, js in jobs.items():
                got.update(run_child(tmp_path, env, ENVS[env], js))
        except BaseException as e:   # (re-raised below)
            child_err.append(e)
    th = threading.Thread(target=children)
    th.start()
    for j in [j for j, *_ in routes + edges] + gens + [whole]:
        truth(j)
    th.join()
    if child_err:
        raise child_err[0]
    t_child = time.time() - t_start
    errors = []

    def attempt(fn, jid):
        try:
            fn()
        except AssertionError as e:   # (every row is checked; the failures are reported together)
            errors.append('{}: {}'.format(jid, e))

    for j, name, must, must_not in routes + edges:
        family = name if name.startswith(('p', 'K', 'seed', 'offset', 'hT', 'path')) else j['id'].split('_', 1)[1]
        floors = ((RM.LONG_FLOOR_H, RM.LONG_FLOOR_G) if j['batch'] == 'K4097x6' else
                  (2e-6, LARGE_FLOOR_G) if j['batch'] == 'large' else ())
        attempt(lambda: check_row(j, *got[j['id']], family, must, must_not, *floors), j['id'])
    for j in gens:
        attempt(lambda: check_row(j, *got[j['id']], 'generic'), j['id'])
    for j in linear:
        r, r0 = got[j['id']][0], got[j['id'] + '_p0'][0]
        attempt(lambda: [np.testing.assert_array_equal(r[k], r0[k], err_msg=j['id'] + ' ' + k) for k in r], j['id'])

    def shard_sum():
        a, b = got['shard0'][0], got['shard1'][0]
        res = {k: (a[k] + b[k] if k.startswith(('loss', 'grad', 'g.')) else np.concatenate([a[k], b[k]]))
               for k in a}
        o32, o64 = truth(whole)
        hip_util.check_vs_oracle('shards', o32, o64, res, RATIOS, 'shards')
        # and the whole batch in one call
        hip_util.check_vs_oracle('whole', o32, o64, got['whole'][0], RATIOS, 'shards')
    attempt(shard_sum, 'shards')
    print('worst ratio per family:', json.dumps({k: round(v, 2) for k, v in sorted(RATIOS.items())}))
    print('children {:.1f} s, oracle {:.1f} s, total {:.1f} s'.format(t_child, ORACLE_S[0], time.time() - t_start))
    assert not errors, '\n'.join(errors)
