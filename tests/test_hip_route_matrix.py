"""Every compiled shape on every kernel route it can take, against the float64 oracle.

The library picks one of about six kernel families per call from the model shape (the
shape-specialised table ``njode_amd.build.CONFIGS``), the batch size, the row count, the Euler-step
count K and the record budget (``njode_route.h``: ``size_call`` decides what the workspace is sized
for, ``route_call`` what ``njode_api.hip`` launches).  This module derives the routes of every configuration from the
kernels' capability predicates (restated below), drives each one on purpose -- through batch sizes,
schedule lengths and the A/B environment switches -- and checks that the route ran by the kernel
names of ``njode_profile_read``.  Every route's loss, hT and gradients are compared with the oracle
in float64, with the fp32 oracle's own distance from float64 as the yardstick:

    err(HIP, f64) <= max(2 err(oracle fp32, f64), floor)

(max-abs for hT, relative L2 per gradient tensor, absolute for the loss), and never looser than
``hip_util``'s ATOL / RTOL / GRAD_REL_L2.  The switches are read once per process, so every distinct
environment runs in one child process, one after another; the parent runs the oracle.

Worst measured err(HIP, f64) / err(o32, f64) per route family (MI355X; a ratio above 2 passes on the
floor, where both errors are at fp32 rounding): wave per item 2.86, split <= 384 tiles 10.2, split 385-768
tiles 8.5, mixed > 2 048 tiles 11.7, one-wave tiles (mfma1) 2.83, one-wave shapes 2.57 / 2.09 / 9.06 (one
tile / small / large batch), nn_desc=None 3.56, use_rnn 2.65, wave per path 1.29, four-wave tiles 0.96, record-budget
rows 1.64, shape-generic 1.26, long schedules 1.04 / 1.42 / 1.06 / 15.2 / 24.5 at K = 511 / 512 / 4 095 /
4 096 / 4 097, split kernels at K = 4 095 2.17, mixed kernels at K = 4 070 2.28 (the long-K floors of
2e-5 / 1e-4 hold there).
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import hip_util
from hip_util import bs_batch, exact_k_batch, hip_model, kernel_names, oracle_pair, rel_l2
from njode_amd.build import CONFIGS, RELU

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)

# ---- capability predicates, restated ---------------------------------------------------------------
# njode_cfg.hip:33-54 and njode_kernels.h:184-194 (with SplitOk, njode_mfma_split.h:39, Q4Ok,
# njode_mfma_lock4.h:32, and MF<C>, njode_mfma.h:68-76)


def caps(c):
    d, H, DO, nh, W, act, masked, curt, res, rnn = c
    enc_case = 0 if not res else (1 if d <= H else 2)
    dec_case = 0 if not res else (1 if H <= DO else 2)
    mt1, mth = (W + 15) // 16, (H + 15) // 16
    mtb1 = (H + d + 15) // 16 if masked else mth
    two = nh == 2
    has_mfma = two and not masked and not rnn and DO <= 16 and W < 64
    has_mfma_lock = two and not rnn and W < 64 and H <= 64 and DO <= 64
    has_mfma_sweep = has_mfma_lock and (not masked or enc_case == 0 or (enc_case == 1 and d == H))
    # HAS_SPLIT: two hidden layers, (W + 15) / 16 == 4, H <= 16, unmasked, no GRU
    has_split = has_mfma and two and mt1 == 4 and mth == 1 and not masked and not rnn
    has_q4 = has_mfma_sweep and two and masked and not rnn and mt1 == 4 and d == DO and H <= 64 and \
        d <= 64 and mtb1 <= 8 and (enc_case == 0 or (enc_case == 1 and d == H)) and \
        (dec_case == 0 or (dec_case == 1 and DO == H))
    chain_ok = two and masked and not rnn and W <= 64 and H <= 64 and d <= 64 and DO <= 64 and d == DO and \
        (enc_case == 0 or (enc_case == 1 and d == H)) and (dec_case == 0 or (dec_case == 1 and DO == H))
    has_chain = has_q4 and chain_ok
    seg_chain_ok = two and not masked and not rnn and 16 < W <= 64 and H <= 16 and d <= 8
    has_seg_chain = has_split and has_mfma_sweep and seg_chain_ok
    return dict(HAS_MFMA=has_mfma, HAS_SPLIT=has_split, HAS_MFMA_LOCK=has_mfma_lock, HAS_MFMA_SWEEP=has_mfma_sweep,
                HAS_Q4=has_q4, HAS_CHAIN=has_chain, HAS_SEG_CHAIN=has_seg_chain)


ITEMS = ['k_seg_fwd_chain', 'k_seg_bwd_chain']
MIXED = ['k_ode_fwd_mixed', 'k_ode_bwd_mixed']
ONE_WAVE = ['k_ode_fwd_mfma', 'k_ode_bwd_mfma']
# the only route of the shapes without the matrix-core kernels (nn_desc=None, use_rnn): the names of
# the first green run
NN_NONE = ['k_ode_bwd_items', 'k_jump_rows_bwd', 'k_encode_rows_bwd']
GRU = ['k_paths_fwd', 'k_paths_bwd_adj', 'k_gru_dw_rows']


def routes(c):
    """(row name, environment tag, batch kind, kernels that must run, kernels that must not)."""
    k = caps(c)
    d, H, DO, nh, W, act, masked, curt, res, rnn = c
    out = []
    if k['HAS_SEG_CHAIN']:
        out += [('items', 'default', 'small', ITEMS + ['k_ode_dw_stored*'], MIXED),
                ('split384', 'tiles', 'tiles384', MIXED, ITEMS),
                ('split768', 'tiles', 'tiles768', MIXED, ITEMS),
                ('mixed', 'default', 'large', MIXED, ITEMS),
                ('mfma1', 'mfma1', 'small', ONE_WAVE, ITEMS + MIXED)]
    elif k['HAS_MFMA']:
        out += [('one_wave_1tile', 'default', 'tile1', ONE_WAVE, ITEMS + MIXED),
                ('one_wave', 'default', 'small', ONE_WAVE, ITEMS + MIXED),
                ('one_wave_large', 'default', 'large', ONE_WAVE, ITEMS + MIXED)]
    elif k['HAS_CHAIN']:
        out += [('chain', 'default', 'physio', ['k_paths_fwd_chain', 'k_paths_bwd_adj_chain'], ['k_paths_fwd_mfma']),
                ('lock4_pt1', 'tiles', 'physio', ['k_paths_fwd_mfma'], ['k_paths_fwd_chain']),
                ('lock4_pt16', 'mfma1', 'physio', ['k_paths_fwd_mfma'], ['k_paths_fwd_chain'])]
    elif rnn:
        out += [('gru', 'default', 'small', GRU, ITEMS + MIXED),
                ('gru_large', 'default', 'large', GRU, ITEMS + MIXED)]
    elif nh == 0:
        out += [('linear', 'default', 'small', NN_NONE, ITEMS + MIXED),
                ('linear_large', 'default', 'large', NN_NONE, ITEMS + MIXED)]
    return out


# environments of the route rows: one child each
ENVS = {
    'default': {},
    # the tiles of the segment plan (unmasked) and of the masked lockstep plan, one path per tile
    'tiles': {'NJODE_SEG_CHAIN_MAX': '0', 'NJODE_CHAIN_MAX': '0', 'NJODE_LOCK4_PT': '1'},
    # one-wave tiles of the segment plan; sixteen paths per tile of the masked lockstep plan
    'mfma1': {'NJODE_ODE': 'mfma1', 'NJODE_CHAIN_MAX': '0', 'NJODE_LOCK4_PT': '16'},
}


def model_cfg(c, dropout=0.0, which_loss=None, weight=None):
    d, H, DO, nh, W, act, masked, curt, res, rnn = c
    nn = None if nh == 0 else tuple((W, 'relu' if act == RELU else 'tanh') for _ in range(nh))
    opts = {'masked': bool(masked), 'input_current_t': bool(curt), 'residual_enc_dec': bool(res)}
    cfg = dict(input_size=d, hidden_size=H, output_size=DO, ode_nn=nn, readout_nn=nn, enc_nn=nn,
               use_rnn=bool(rnn), bias=True, dropout_rate=dropout, options=opts)
    if which_loss is not None:
        opts['which_loss'] = which_loss
    if weight is not None:
        cfg['weight'] = weight
    return cfg


def make_batch(kind, c):
    """(batch, delta_t, T) of a batch kind; deterministic, so parent and child build the same."""
    d = c[0]
    if kind == 'physio':
        from njode_amd import synthetic_physionet
        b = synthetic_physionet.make_batch(batch_size=37, dim=d, n_grid=60, n_obs_range=(3, 9), seed=3)
        return b, b['delta_t'], b['T']
    if kind == 'tile1':   # one tile of 16 rows
        return exact_k_batch(4, 100, obs_per_path=3, seed=5)
    if kind == 'K4070dense':   # n_obs + B > 16 384: the mixed kernels by default, > 768 tiles
        return exact_k_batch(24, 4070, obs_per_path=700, seed=11)
    if kind.startswith('K'):
        return exact_k_batch(24, int(kind[1:]), obs_per_path=3, seed=int(kind[1:]) % 97)
    B, perc, steps, seed = {'small': (24, 0.1, 100, 1),
                            # 22 tiles over 384 in the split kernels' all-four-wave launch .. 768
                            'tiles384': (500, 0.1, 100, 2), 'tiles768': (1000, 0.1, 100, 3),
                            # > MAX_WAVES = 2 048 tiles of 16 rows, n_obs + B > 16 384
                            'large': (900, 0.95, 40, 4)}[kind]
    b, meta = bs_batch(B, seed=seed, obs_perc=perc, nb_steps=steps)
    if d == 2:   # func_appl_X=['power-2']
        b = dict(b, X=torch.cat([b['X'], b['X'] ** 2], 1), start_X=torch.cat([b['start_X'], b['start_X'] ** 2], 1))
    return b, meta['dt'], meta['maturity']


# steps of the tail of an ``until_T`` job past the last observation: off the grid of delta_t
TAIL_STEPS = 2.6


def job_batch(job, c):
    """(batch, delta_t, T) of a job: ``make_batch`` of its kind, then the job's optional keys --
    ``irregular`` (``hip_util.irregular_batch`` with ``dt_factor``), ``dt_factor`` alone (delta_t scaled),
    ``until_T`` (T a few off-grid steps past the last observation).  Parent and child build the same."""
    b, dt, T = make_batch(job['batch'], c)
    if job.get('irregular'):
        b, dt = hip_util.irregular_batch(b, dt, job['dt_factor'])
    elif job.get('dt_factor'):
        dt = job['dt_factor'] * dt
    if job.get('until_T'):
        T = float(b['times'][-1]) + TAIL_STEPS * dt
    return b, dt, T


def job_cfg(job, c, dropout=0.0):
    return model_cfg(c, dropout, job.get('which_loss'), job.get('weight'))


def c_hT(B, H):
    """Upstream gradient of hT of an ``until_T`` job's autograd objective, loss + (c hT).sum()."""
    return 0.05 * torch.cos(torch.arange(B * H, dtype=torch.float32)).view(B, H)


# ---- child side --------------------------------------------------------------------------------------
def _child(jobs, out_dir):
    """Run every job of this environment; write its numbers (.npz) and kernel names (.json)."""
    meta = {}
    for job in jobs:
        c = tuple(job['cfg'])
        b, dt, T = job_batch(job, c)
        torch.manual_seed(0)
        from njode_amd import models
        m = hip_model(job_cfg(job, c, job['dropout']), models.NJODE(**model_cfg(c)).state_dict()).train()
        ws = []
        acq = m._acquire_ws
        m._acquire_ws = lambda n, dev: (ws.append(int(n)), acq(n, dev))[1]
        M = b['M'].cuda() if 'M' in b else None
        args = (b['times'], b['time_ptr'], b['X'].cuda(), b['obs_idx'].cuda().int(), dt, T,
                b['start_X'].cuda(), b['n_obs_ot'].cuda().int())
        m._step_counter = 7
        (_, loss), names = kernel_names(lambda: m.loss_and_grad(*args, M=M))
        res = {'loss_fused': float(loss), 'grad_fused': m.flat_grad().cpu().numpy().astype(np.float64)}
        # optional keys: an upstream gradient that is not 1; a tail after the last observation, which the
        # fused step does not take (it moves hT, not the loss) -- with a gradient through hT
        scale, until = job.get('grad_scale', 1.0), bool(job.get('until_T'))
        kw = dict(M=M, until_T=True) if until else dict(M=M)
        if until:
            del res['grad_fused']
        # the reference's call sequence
        m._step_counter = 7
        m.zero_grad()

        def autograd_step():
            hT, loss2 = m(*args, **kw)
            if until:
                (scale * loss2 + (c_hT(*hT.shape).cuda() * hT).sum()).backward()
            elif scale != 1.0:
                (scale * loss2).backward()
            else:
                loss2.backward()
            return hT, loss2
        (hT, loss2), names2 = kernel_names(autograd_step)
        res['loss_auto'] = float(loss2)
        res['grad_auto'] = np.concatenate([p.grad.detach().cpu().numpy().ravel() for p in m.parameters()])
        if scale != 1.0:   # (compared with the fused step's, whose upstream gradient is 1)
            res['grad_auto'] = res['grad_auto'].astype(np.float64) / scale
        res['hT'] = hT.detach().cpu().numpy().astype(np.float64)
        for k, p in m.named_parameters():
            res['g.' + k] = p.grad.detach().cpu().numpy().astype(np.float64)
        info = {'names': names, 'names_auto': names2, 'ws': ws[0], 'n_obs': int(b['time_ptr'][-1]),
                'B': len(b['start_X'])}
        if job.get('prefetch'):
            # the deferred plan of a call the single launch does not build; must give the same bits
            m._step_counter = 7
            m._plans.clear()
            m.prefetch_plan(*args, M=M, need_hT=False)
            (_, loss3), names3 = kernel_names(lambda: m.loss_and_grad(*args, M=M))
            res['loss_prefetch'] = float(loss3)
            res['grad_prefetch'] = m.flat_grad().cpu().numpy().astype(np.float64)
            info['names_prefetch'] = names3
        if job.get('predict'):
            m.eval()
            with torch.no_grad():
                (out, names4) = kernel_names(lambda: m(*args, M=M, return_path=True))
            res['path_h'] = out[3].cpu().numpy().astype(np.float64)
            info['names_predict'] = names4
        if job.get('predict_loss'):
            # the lockstep prediction call with its own loss code, up to T
            m.eval()
            with torch.no_grad():
                (out, names5) = kernel_names(lambda: m(*args, M=M, return_path=True, get_loss=True, until_T=True))
            res.update({'p.hT': out[0].cpu().numpy().astype(np.float64), 'p.loss': float(out[1]),
                        'p.path_h': out[3].cpu().numpy().astype(np.float64),
                        'p.path_y': out[4].cpu().numpy().astype(np.float64)})
            info['names_predict_loss'] = names5
        np.savez(os.path.join(out_dir, job['id'] + '.npz'), **res)
        meta[job['id']] = info
    with open(os.path.join(out_dir, 'meta.json'), 'w') as f:
        json.dump(meta, f)


_SNIPPET = r'''
import json, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {repo!r})
import test_hip_route_matrix as T
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


# ---- parent side: oracle and comparisons ------------------------------------------------------------
_ORACLE = {}


def truth(c, kind, predict=False):
    """(f32, f64) oracle results of configuration c on batch kind: dicts of loss, hT, grads[, path_h]."""
    key = (tuple(c), kind)
    if key not in _ORACLE or (predict and 'path_h' not in _ORACLE[key][1]):
        from njode_amd import models
        torch.manual_seed(0)
        sd = {k: v.detach().clone() for k, v in models.NJODE(**model_cfg(c)).state_dict().items()}
        b, dt, T = make_batch(kind, c)
        _ORACLE[key] = oracle_pair(model_cfg(c), sd, b, dt, T, predict=predict)
    return _ORACLE[key]


RATIOS = {}


def check_vs_oracle(tag, family, c, kind, res, floor_h=2e-6, floor_g=1e-5, predict=False):
    o32, o64 = truth(c, kind, predict)
    hip_util.check_vs_oracle(tag, o32, o64, res, RATIOS, family, floor_h, floor_g, predict)


def has(names, want):
    return any(n.startswith(want[:-1]) for n in names) if want.endswith('*') else want in names


def check_names(tag, names, must, must_not=()):
    for k in must:
        assert has(names, k), (tag, 'did not run', k, names)
    for k in must_not:
        assert not has(names, k), (tag, 'ran', k, names)


# ---- the tests -----------------------------------------------------------------------------------------
def test_route_table_covers_every_compiled_configuration():
    from njode_amd import _lib
    info = _lib.build_info()
    for c in CONFIGS:
        d, H, DO, nh, W, act, masked, curt, res, rnn = c
        flags = masked * 0x1 + curt * 0x2 + res * 0x4 + rnn * 0x10
        assert 'd{}.h{}.o{}.nh{}.w{}.a{}.f{};'.format(d, H, DO, nh, W if nh else 0, act if nh else 0,
                                                    flags) in info, (c, info)
        assert routes(c), ('no route for', c)


def check_sizes(kind, n_obs, B):
    """The row and path counts a batch kind stands for (the tile bounds of its route)."""
    if kind == 'tiles384':
        assert (n_obs + 15) // 16 <= 384, n_obs
    if kind == 'tiles768':
        assert 384 < (n_obs + 15) // 16 <= 768, n_obs
    if kind == 'tile1':
        assert n_obs <= 16, n_obs
    if kind == 'large':
        assert (n_obs + 15) // 16 > 2048 and n_obs + B > 16384, (n_obs, B)


def _check_row(jid, c, kind, must, must_not, predict, res, info):
    check_names(jid, info['names'], must, must_not)
    check_names(jid + ' (autograd)', info['names_auto'], [m for m in must if 'dw_stored' not in m and 'dw_pairs' not in m], must_not)
    if predict:
        # a prediction call: the lockstep plan, never the segment plan's kernels
        check_names(jid + ' (return_path)', info['names_predict'], [], ITEMS + MIXED)
    check_sizes(kind, info['n_obs'], len(res['hT']))
    check_vs_oracle(jid, jid.split('_', 1)[1], c, kind, res, predict=predict)


def test_every_configuration_on_every_route_against_float64(tmp_path):
    jobs = {env: [] for env in ENVS}
    rows = []
    for i, c in enumerate(CONFIGS):
        k = caps(c)
        for name, env, kind, must, must_not in routes(c):
            jid = 'c{}_{}'.format(i, name)
            predict = not c[6]   # (every unmasked row: a prediction call on the lockstep plan)
            jobs[env].append({'id': jid, 'cfg': list(c), 'batch': kind, 'dropout': 0.0, 'predict': predict})
            rows.append((jid, env, c, kind, must, must_not, predict))
            # dropout on: every route of the w50 and masked shapes draws the same masks
            if k['HAS_SEG_CHAIN'] and kind in ('small',) or k['HAS_CHAIN']:
                jobs[env].append({'id': jid + '_drop', 'cfg': list(c), 'batch': kind, 'dropout': 0.1})
        if k['HAS_SEG_CHAIN']:   # the same dropout batch on the other routes of the shape
            jobs['tiles'].append({'id': 'c{}_split_small_drop'.format(i), 'cfg': list(c), 'batch': 'small', 'dropout': 0.1})
    got = {}
    for env, js in jobs.items():
        got.update(run_child(tmp_path, env, ENVS[env], js))
    errors = []
    for jid, env, c, kind, must, must_not, predict in rows:
        try:
            _check_row(jid, c, kind, must, must_not, predict, *got[jid])
        except AssertionError as e:   # (every row is checked; the failures are reported together)
            errors.append('{}: {}'.format(jid, e))
    # dropout on: the routes of one shape agree (the masks are keyed by the path, not by the tile)
    for i, c in enumerate(CONFIGS):
        k = caps(c)
        if k['HAS_SEG_CHAIN']:
            groups = [['c{}_items_drop'.format(i), 'c{}_mfma1_drop'.format(i), 'c{}_split_small_drop'.format(i)]]
        elif k['HAS_CHAIN']:
            groups = [['c{}_chain_drop'.format(i), 'c{}_lock4_pt1_drop'.format(i), 'c{}_lock4_pt16_drop'.format(i)]]
        else:
            continue
        for g in groups:
            ref = got[g[0]][0]
            assert np.isfinite(ref['grad_fused']).all() and ref['loss_fused'] > 0
            # (the masks were drawn: dropout moves the loss away from the dropout-0 run of the route)
            off = got[g[0][:-len('_drop')]][0]['loss_fused']
            assert abs(ref['loss_fused'] - off) > 1e-4 * abs(off), (g[0], ref['loss_fused'], off)
            for other in g[1:]:
                o = got[other][0]
                assert o['loss_fused'] == pytest.approx(ref['loss_fused'], rel=2e-5), (g[0], other)
                assert rel_l2(o['grad_fused'], ref['grad_fused']) <= 1e-4, (g[0], other)
    print('worst ratio per route family:', json.dumps({k: round(v, 2) for k, v in sorted(RATIOS.items())}))
    assert not errors, '\n'.join(errors)


# ---- long schedules --------------------------------------------------------------------------------------
DEMO = CONFIGS[0]
LONG_K = (511, 512, 4095, 4096, 4097)
# float64 floors of the long schedules (hT max-abs, gradient relative L2): measured, see the docstring
LONG_FLOOR_H, LONG_FLOOR_G = 2e-5, 1e-4


def test_long_schedules_against_float64(tmp_path):
    from njode_amd.schedule import Schedule
    for K in LONG_K:
        b, dt, T = make_batch('K{}'.format(K), DEMO)
        s = Schedule(b['times'], dt, T, False)
        assert s.n_steps == K and not s.has_tail() and s.n_times <= K, (K, s.n_steps)
    jobs = [{'id': 'K{}'.format(K), 'cfg': list(DEMO), 'batch': 'K{}'.format(K), 'dropout': 0.0,
             'prefetch': K in (512, 4096)} for K in LONG_K]
    # K = 4 070 with > 16 384 items + paths: the mixed kernels by default, split point inside the range
    # K = 4 063 .. 4 095 where the layout kernel's tables once overran its LDS array
    jobs.append({'id': 'K4070dense', 'cfg': list(DEMO), 'batch': 'K4070dense', 'dropout': 0.0})
    got = run_child(tmp_path, 'long', {}, jobs, timeout=300)
    # the split kernels at their largest K
    got.update(run_child(tmp_path, 'long_tiles', {'NJODE_SEG_CHAIN_MAX': '0'},
                         [{'id': 'K4095_split', 'cfg': list(DEMO), 'batch': 'K4095', 'dropout': 0.0}]))
    n_obs = got['K4070dense'][1]['n_obs']
    assert n_obs + 24 > 16384 and (n_obs + 15) // 16 > 768, n_obs
    expect = {'K511': ITEMS, 'K512': ITEMS, 'K4095': ITEMS, 'K4096': ONE_WAVE, 'K4097': ONE_WAVE,
              'K4095_split': MIXED, 'K4070dense': MIXED}
    errors = []
    for jid, (res, info) in got.items():
        try:
            must = expect[jid]
            check_names(jid, info['names'], must, [n for n in ITEMS + MIXED + ONE_WAVE if n not in must])
            if 'loss_prefetch' in res:
                assert res['loss_prefetch'] == res['loss_fused'], jid
                assert np.array_equal(res['grad_prefetch'], res['grad_fused']), jid
            check_vs_oracle(jid, 'long_K', DEMO, jid.split('_')[0] if jid.endswith('_split') else jid, res,
                            floor_h=LONG_FLOOR_H,
                            floor_g=LONG_FLOOR_G)
        except AssertionError as e:
            errors.append('{}: {}'.format(jid, e))
    assert not errors, '\n'.join(errors)
    # the one-launch plan (k_plan_grid) needs K + 1 <= PLAN_KEYS = 512
    if any('k_plan_grid' in got[j][1]['names'] for j in got):
        assert 'k_plan_grid' in got['K511'][1]['names']
        assert 'k_plan_grid' not in got['K512'][1]['names']


# ---- record budget -----------------------------------------------------------------------------------------
PHYSIO = next(c for c in CONFIGS if caps(c)['HAS_CHAIN'] and c[1] == 41)
GENERIC72 = (41, 41, 41, 2, 72, 0, 1, 0, 1, 0)   # masked, width 72: the shape-generic kernels
CHAIN_ACT_FLOATS = 128                           # njode_kernels.h


def _budgets():
    """NJODE_REC_BUDGET_GB values: (middle, tiny).  size_call() (njode_route.h) keeps the records (Sizing::chain,
    seg_items) while B K (CHAIN_ACT_FLOATS 4 + 16) bytes fit, the deltas (Sizing::delta) while B K (2
    CHAIN_ACT_FLOATS 4 + 16) do."""
    from njode_amd.schedule import Schedule
    bk = []
    for kind, c in (('small', DEMO), ('physio', PHYSIO)):
        b, dt, T = make_batch(kind, c)
        B = len(b['start_X'])
        bk.append(B * Schedule(b['times'], dt, T, False).n_steps)
    acts = [x * (CHAIN_ACT_FLOATS * 4 + 16) for x in bk]
    both = [x * (2 * CHAIN_ACT_FLOATS * 4 + 16) for x in bk]
    assert max(acts) < min(both), (acts, both)   # one middle budget for both batches
    mid = (max(acts) + min(both)) / 2
    tiny = min(acts) / 4
    return mid / 1e9, tiny / 1e9


def test_record_budget_routes(tmp_path):
    mid, tiny = _budgets()
    jobs = [{'id': 'demo', 'cfg': list(DEMO), 'batch': 'small', 'dropout': 0.0, 'prefetch': True},
            {'id': 'physio', 'cfg': list(PHYSIO), 'batch': 'physio', 'dropout': 0.0}]
    gen = [{'id': 'gen72', 'cfg': list(GENERIC72), 'batch': 'physio', 'dropout': 0.0}]
    got = {}
    got['default'] = run_child(tmp_path, 'budget_default', {}, jobs)
    got['mid'] = run_child(tmp_path, 'budget_mid', {'NJODE_REC_BUDGET_GB': repr(mid)}, jobs)
    got['mid_nodelta'] = run_child(tmp_path, 'budget_mid_nodelta',
                                   {'NJODE_REC_BUDGET_GB': repr(mid), 'NJODE_CHAIN_DELTA': '0'}, jobs)
    got['tiny'] = run_child(tmp_path, 'budget_tiny', {'NJODE_REC_BUDGET_GB': repr(tiny)}, jobs + gen)
    # (the paths per tile the budget picks for the masked batch: 37 paths of 60 steps cannot fit any
    # tile's records at this budget, so Sizing::q4_pt goes up to 16)
    got['tiny_tiles'] = run_child(tmp_path, 'budget_tiny_tiles',
                                  {'NJODE_REC_BUDGET_GB': repr(tiny), 'NJODE_SEG_CHAIN_MAX': '0',
                                   'NJODE_CHAIN_MAX': '0', 'NJODE_LOCK4_PT': '16', 'NJODE_GEN_PT': '16'},
                                  jobs + gen)
    # (and the generic shape at one path per tile, which 37 paths take within the default budget)
    got['gen_pt1'] = run_child(tmp_path, 'budget_tiny_gen_pt1',
                               {'NJODE_REC_BUDGET_GB': repr(tiny), 'NJODE_GEN_PT': '1'}, gen)
    d, p = got['default']['demo'][1], got['default']['physio'][1]
    check_names('default demo', d['names'], ITEMS + ['k_ode_dw_stored*'], ['k_ode_dw_pairs_mfma'])
    check_names('default physio', p['names'], ['k_paths_fwd_chain', 'k_ode_dw_stored*'], ['k_ode_dw_pairs_mfma'])
    # activations fit, deltas do not: the recomputing pair kernel, the same bits as with the deltas off
    check_names('mid demo', got['mid']['demo'][1]['names'], ITEMS + ['k_ode_dw_pairs_mfma'], ['k_ode_dw_stored*'])
    check_names('mid physio', got['mid']['physio'][1]['names'], ['k_paths_fwd_chain', 'k_ode_dw_pairs_mfma'],
                ['k_ode_dw_stored*'])
    # tiny: neither wave-per-item nor wave-per-path records are taken
    t = got['tiny']
    print('tiny budget demo: kernels', t['demo'][1]['names'], 'workspace bytes', t['demo'][1]['ws'])
    check_names('tiny demo', t['demo'][1]['names'], MIXED, ITEMS)
    check_names('tiny physio', t['physio'][1]['names'], ['k_paths_fwd_mfma'], ['k_paths_fwd_chain'])
    # the shape-generic lockstep kernels: gen_paths_per_tile raises the paths per tile to 16 on its own
    # (the same bits as NJODE_GEN_PT=16, not those of one path per tile)
    check_names('tiny gen72', t['gen72'][1]['names'], ['k_gen_fwd', 'k_gen_bwd', 'k_gen_dw'],
                ['k_gseg_ode_fwd', 'k_paths_fwd_mfma', 'k_paths_fwd_chain'])
    assert t['gen72'][1]['ws'] != got['gen_pt1']['gen72'][1]['ws'], t['gen72'][1]['ws']   # (records of cdiv(B, PT) tiles)
    for a, b_ in (('mid', 'mid_nodelta'), ('tiny', 'tiny_tiles')):
        for jid in (('demo', 'physio', 'gen72') if a == 'tiny' else ('demo', 'physio')):
            ra, ia = got[a][jid]
            rb, ib = got[b_][jid]
            assert ia['names'] == ib['names'], (a, jid, ia['names'], ib['names'])
            if a == 'tiny':
                assert ia['ws'] == ib['ws'], (jid, ia['ws'], ib['ws'])
            for k in ra:
                assert np.array_equal(ra[k], rb[k]), (a, b_, jid, k)
    # a plan prefetched for the call is built for the route the call takes
    for tag in ('default', 'tiny'):
        r = got[tag]['demo'][0]
        assert r['loss_prefetch'] == r['loss_fused'] and np.array_equal(r['grad_prefetch'], r['grad_fused']), tag
    for tag in ('default', 'mid', 'mid_nodelta', 'tiny', 'tiny_tiles'):
        for jid in ('demo', 'physio'):
            check_vs_oracle('budget {} {}'.format(tag, jid), 'budget', DEMO if jid == 'demo' else PHYSIO,
                            'small' if jid == 'demo' else 'physio', got[tag][jid][0])
    check_vs_oracle('budget tiny gen72', 'generic', GENERIC72, 'physio', got['tiny']['gen72'][0])

