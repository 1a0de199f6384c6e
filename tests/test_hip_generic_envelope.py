"""The shape-generic kernels (njode_gen.h, njode_gen_seg.h) across their whole envelope, against
the float64 oracle.

The generic kernels take every shape at run time, so their risks sit in run-time branches: short
and long rows of the product loop (odd / even chunk counts, partial last chunk, the prefetch into
the padding behind the last table), several output tiles per wave and waves without one, the
weight-gradient GEMM's bias column alone in its tile or block column, its slab count at both
clamps, observations held in registers or read from LDS, dynamic LDS above 64 KB up to the limit.
Every shape below is chosen with the restatement of build_model (tests/gen_envelope.py), which
also labels the branches each row takes; the test asserts that together they take every one.

Each row runs a training step, fused and through autograd, on the segment plan and on the lockstep
plan (NJODE_GEN_PLAN=lock, read per step), and a return_path call; the results are compared with
the oracle in float64 by hip_util.check_vs_oracle (the route matrix's rule).  Four child processes
run the environments: the default, NJODE_GEN_PT=16 (read once per process), NJODE_GEN_NW=4 (what
every large segment-plan batch runs) and NJODE_GEN_NW=1 (one wave owns every tile; the observation
branch without registers).  The parent runs the oracle.

Worst measured err(HIP, f64) / err(o32, f64) per branch family (MI355X; a ratio above 2 passes on
the floor, where both errors are at fp32 rounding): short rows 27.5, long rows 19.9, LDS near the
limit 2.42, GRU 1.26, NW = 4 19.9, NW = 1 2.05, PT = 16 5.7, B = 1 7.07, an empty path with an
until_T tail 1.00, K = 4 097 1.13.  The module runs in about 17 s (four children of 3 s each).
Two mutations of njode_gen.h fail it: the partial chunk of a long row without its fourth k-step
(rows whose last quad's fourth k-step holds inputs: widths 400, 1 024 next to H = 228, GRU, masked
D = 209) and a zero bias column in k_gen_dw (every row's bias gradients).
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
from gen_envelope import labels, restate_cfg
from hip_util import exact_k_batch, hip_model, kernel_names, oracle_pair, rel_l2

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)

def _w(n, act='tanh', layers=2):
    return tuple((n, act) for _ in range(layers))


def _cfg(d, H, ode, enc, dec, DO=None, rnn=False, bias=True, **options):
    options.setdefault('residual_enc_dec', True)
    return dict(input_size=d, hidden_size=H, output_size=d if DO is None else DO, ode_nn=ode, readout_nn=dec,
                enc_nn=enc, use_rnn=rnn, bias=bias, dropout_rate=0.0, options=options)


MIXED8 = ((130, 'relu'), (17, 'tanh'), (64, 'relu'), (200, 'tanh'), (1, 'relu'), (48, 'tanh'), (176, 'relu'),
          (33, 'tanh'))
# name: (config, batch); batch = (B, K, observations per path, masked?)
ROWS = {
    'w1': (_cfg(1, 10, _w(1), _w(1), _w(1)), (17, 50, 4, False)),
    'w64': (_cfg(1, 10, _w(64), _w(64), _w(64)), (33, 60, 4, False)),
    'w127': (_cfg(1, 10, _w(127), _w(127, 'relu'), _w(127)), (17, 50, 4, False)),
    'w128': (_cfg(1, 10, _w(128), _w(128), _w(128, 'relu')), (17, 50, 4, False)),
    'w255_relu': (_cfg(1, 10, _w(255, 'relu'), _w(255, 'relu'), _w(255, 'relu')), (17, 50, 4, False)),
    'w256': (_cfg(1, 10, _w(256), _w(256), _w(256)), (17, 50, 4, False)),
    'w400': (_cfg(1, 10, _w(400), _w(400, 'relu'), _w(400)), (17, 40, 4, False)),
    'w1024': (_cfg(1, 10, _w(1024), _w(1024, layers=1), _w(1024, layers=1)), (17, 40, 3, False)),
    # within 64 bytes of the 160 KB LDS: the largest H next to width-1 024 layers
    'w1024_h228': (_cfg(1, 228, _w(1024, layers=1), _w(64, layers=1), _w(1024, layers=1)), (9, 30, 3, False)),
    'none_h628': (_cfg(1, 628, None, None, None, residual_enc_dec=False), (9, 30, 3, False)),
    'gru_h252': (_cfg(1, 252, _w(50), _w(50), _w(50), rnn=True), (9, 30, 3, False)),
    'gru_masked_h252': (_cfg(1, 252, _w(50), _w(50), _w(50), rnn=True, masked=True), (9, 30, 3, True)),
    'd251': (_cfg(251, 10, _w(24), _w(24), _w(24), residual_enc_dec=False), (9, 30, 3, False)),
    'masked_d209': (_cfg(209, 209, _w(100), _w(100), _w(100), masked=True), (9, 30, 3, True)),
    # n_out 17; residual enc_case 1 (x2) / dec_case 2 (x2)
    'd17_res12': (_cfg(17, 34, _w(48), _w(40, 'relu'), _w(72)), (17, 40, 4, False)),
    # residual enc_case 2 (x2) / dec_case 1 (x2)
    'd8_res21': (_cfg(8, 4, _w(33), _w(20, 'relu', 1), _w(72, 'tanh', 7)), (17, 40, 4, False)),
    'deep_456': (_cfg(1, 10, _w(40, 'relu', 4), _w(24, 'tanh', 5), _w(33, 'relu', 6)), (17, 40, 4, False)),
    # depth 8 / 0 / 3, mixed widths and activations, no bias, input_current_t, the 'easy' loss
    'deep_mixed': (_cfg(2, 6, MIXED8, None, ((255, 'relu'), (17, 'tanh'), (128, 'relu')), bias=False,
                        residual_enc_dec=False, input_current_t=True, which_loss='easy'), (17, 40, 4, False)),
    # output_size != input_size: prediction calls only
    'd3_do7': (_cfg(3, 12, _w(80), _w(80), _w(80), DO=7, residual_enc_dec=False), (17, 40, 4, False)),
    # narrow, D > 16: run under NJODE_GEN_NW=1 too
    'masked_d20': (_cfg(20, 20, _w(40), _w(40), _w(40), masked=True), (17, 40, 3, True)),
    'd24_w64': (_cfg(24, 24, _w(64), _w(64), _w(64)), (17, 40, 3, False)),
}
WIDE = ('w256', 'w400', 'w1024', 'w1024_h228', 'gru_h252', 'gru_masked_h252', 'none_h628')
NARROW_D = ('masked_d20', 'd24_w64', 'd251')
DROP = ('w255_relu', 'w1024')
ENVS = {'default': {}, 'pt16': {'NJODE_GEN_PT': '16'}, 'nw4': {'NJODE_GEN_NW': '4'}, 'nw1': {'NJODE_GEN_NW': '1'}}
NW = {'nw4': 4, 'nw1': 1}
SPECIALISED = ('k_ode_', 'k_seg_', 'k_paths_', 'k_jump_', 'k_encode_', 'k_gru_')


def make_batch(row, edge=None):
    """(batch, dt, T, until_T) of a row; deterministic, so parent and child build the same.
    edge: 'b1' one path; 'empty' a path without observations and an until_T tail; 'longK' K = 4 097."""
    cfg, (B, K, n_obs, masked) = ROWS[row]
    d = cfg['input_size']
    if edge == 'b1':
        B = 1
    if edge == 'longK':
        B, K, n_obs = 6, 4097, 5
    if masked:
        from njode_amd import synthetic_physionet
        b = synthetic_physionet.make_batch(batch_size=B, dim=d, n_grid=K, n_obs_range=(2, n_obs + 3), seed=B + d)
        return b, b['delta_t'], b['T'], False
    b, dt, T = exact_k_batch(B, K, obs_per_path=n_obs, seed=B * 7 + K + d, d=d)
    if edge == 'empty':
        rng = np.random.RandomState(5)
        obs = np.zeros((B, K + 1), dtype=np.int64)
        for p in range(B):
            if p != 2:   # path 2: no observations at all
                obs[p, 1 + rng.choice(K, size=n_obs, replace=False)] = 1
        obs[0, K] = 1    # an observation at T ...
        paths = np.cumsum(rng.normal(0.0, 0.05, size=(B, d, K + 1)), axis=2) + 1.0
        from njode_amd import data_utils
        b = data_utils.collate_arrays(paths, obs, obs[:, 1:].sum(axis=1), dt)
        return b, dt, T + 7.5 * dt, True   # ... and an until_T tail past it
    return b, dt, T, False


def state_dict(row):
    from njode_amd import models
    torch.manual_seed(11)
    return {k: v.detach().clone() for k, v in models.NJODE(**ROWS[row][0]).state_dict().items()}


# ---- child side ----------------------------------------------------------------------------------------
def _child(jobs, out_dir):
    meta = {}
    for job in jobs:
        row, edge = job['row'], job.get('edge')
        cfg = dict(ROWS[row][0], dropout_rate=job.get('dropout', 0.0))
        b, dt, T, until = make_batch(row, edge)
        m = hip_model(cfg, state_dict(row)).train()
        M = b['M'].cuda() if 'M' in b else None
        args = (b['times'], b['time_ptr'], b['X'].cuda(), b['obs_idx'].cuda().int(), dt, T,
                b['start_X'].cuda(), b['n_obs_ot'].cuda().int())
        kw = dict(M=M, until_T=until) if until else dict(M=M)
        res, info = {}, {'n_obs': int(b['time_ptr'][-1]), 'B': len(b['start_X'])}
        if job['plan'] == 'lock':
            os.environ['NJODE_GEN_PLAN'] = 'lock'
        else:
            os.environ.pop('NJODE_GEN_PLAN', None)
        if cfg['input_size'] == cfg['output_size']:
            m._step_counter = 7
            # (loss_and_grad has no until_T: the tail moves hT, not the loss)
            (_, loss), names = kernel_names(lambda: m.loss_and_grad(*args, M=M))
            flat = m.flat_grad().cpu().numpy().astype(np.float64)
            if m._flat_present is not None:   # (bias=False: the flat vector's slots without a parameter)
                flat = flat[m._flat_present.cpu().numpy() > 0]
            res.update(loss_fused=float(loss), grad_fused=flat)
            m._step_counter = 7
            m.zero_grad()

            def autograd_step():
                hT, loss2 = m(*args, **kw)
                loss2.backward()
                return hT, loss2
            (hT, loss2), names2 = kernel_names(autograd_step)
            res['loss_auto'] = float(loss2)
            res['grad_auto'] = np.concatenate([p.grad.detach().cpu().numpy().ravel() for p in m.parameters()])
            res['hT'] = hT.detach().cpu().numpy().astype(np.float64)
            for k, p in m.named_parameters():
                res['g.' + k] = p.grad.detach().cpu().numpy().astype(np.float64)
            info.update(names=names, names_auto=names2)
        if job.get('predict'):
            m.eval()
            get_loss = cfg['input_size'] == cfg['output_size']
            with torch.no_grad():
                out, names3 = kernel_names(lambda: m(*args, return_path=True, get_loss=get_loss, **kw))
            res['path_h'] = out[3].cpu().numpy().astype(np.float64)
            if not get_loss:
                res['hT'] = out[0].cpu().numpy().astype(np.float64)
            info['names_predict'] = names3
        np.savez(os.path.join(out_dir, job['id'] + '.npz'), **res)
        meta[job['id']] = info
    with open(os.path.join(out_dir, 'meta.json'), 'w') as f:
        json.dump(meta, f)


_SNIPPET = r'''
import json, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {repo!r})
import test_hip_generic_envelope as T
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


# ---- the table --------------------------------------------------------------------------------------------
def jobs_of_table():
    """{env: [job]}: every row on both plans by default; the lockstep plan at PT = 16; the wide rows
    under NW = 4 (both plans); the narrow rows with D > 16 under NW = 1 (lockstep); the edges and dropout."""
    jobs = {e: [] for e in ENVS}
    for row, (cfg, (B, K, _, masked)) in ROWS.items():
        loss = cfg['input_size'] == cfg['output_size']
        # (the segment plan serves unmasked loss calls without the GRU jump: njode_gen.hip, use_seg)
        plans = ['seg', 'lock'] if loss and not masked and not cfg['use_rnn'] else ['lock']
        for plan in plans:
            jobs['default'].append({'id': '{}.default.{}'.format(row, plan), 'row': row, 'plan': plan,
                                    'predict': not masked and plan == 'lock' or not loss})
        jobs['pt16'].append({'id': row + '.pt16.lock', 'row': row, 'plan': 'lock', 'predict': not loss})
        if row in WIDE:
            for plan in plans:
                jobs['nw4'].append({'id': '{}.nw4.{}'.format(row, plan), 'row': row, 'plan': plan, 'predict': not loss})
        if row in NARROW_D:
            jobs['nw1'].append({'id': row + '.nw1.lock', 'row': row, 'plan': 'lock', 'predict': not masked})
    for edge, row in (('b1', 'w128'), ('empty', 'w400'), ('longK', 'w64')):
        for plan in ('seg', 'lock'):
            jobs['default'].append({'id': '{}.{}.default.{}'.format(row, edge, plan), 'row': row, 'edge': edge,
                                    'plan': plan})
    for row in DROP:
        for env, plan in (('default', 'seg'), ('default', 'lock'), ('pt16', 'lock')):
            jobs[env].append({'id': '{}.drop.{}.{}'.format(row, env, plan), 'row': row, 'plan': plan, 'dropout': 0.1})
    return jobs


REQUIRED = {'short', 'long_odd', 'long_even', 'long_partial', 'long_full', 'prefetch_into_padding',
            'tiles_per_wave_2', 'tiles_per_wave_3', 'tiles_per_wave_4', 'tiles_per_wave_5+', 'idle_waves',
            'dw_bias_alone_in_tile', 'dw_bias_alone_in_block', 'dw_edge', 'S_8', 'S_mid', 'S_256',
            'x_regs', 'x_lds', 'lds_above_64k', 'lds_near_limit', 'gru',
            'enc_case_0', 'enc_case_1', 'enc_case_2', 'dec_case_0', 'dec_case_1', 'dec_case_2'}


def row_labels(row, env):
    why, model = restate_cfg(ROWS[row][0])
    assert why is None, (row, why)
    return labels(model, NW.get(env))


def test_envelope_table_takes_every_branch():
    """CPU side of the table: every row is admitted, and together the rows (in their environments)
    take every branch the module is about; prints each row's labels."""
    seen = set()
    for env, js in jobs_of_table().items():
        for j in js:
            lab = row_labels(j['row'], env)
            seen |= lab
            if j['plan'] == 'lock' and env == 'default' and not j.get('edge') and not j.get('dropout'):
                print('{:18s} {}'.format(j['row'], ' '.join(sorted(lab))))
    assert REQUIRED <= seen, REQUIRED - seen
    # the observation branch without registers is taken only under NJODE_GEN_NW
    assert all('x_regs' in row_labels(r, 'default') for r in ROWS)
    assert any('x_lds' in row_labels(r, 'nw1') for r in NARROW_D)
    # widths of the issue's list, depth 0 .. 8, n_out 1 / 17 / 255
    from njode_amd import models
    widths, depths, outs = set(), set(), set()
    for cfg, _ in ROWS.values():
        for k in ('ode_nn', 'enc_nn', 'readout_nn'):
            n, ws, _ = models._desc_of(cfg[k])
            widths |= set(ws)
            depths.add(n)
        outs.add(cfg['output_size'])
    assert {1, 64, 127, 128, 255, 256, 400, 1024} <= widths and set(range(0, 9)) <= depths
    assert {1, 17} <= outs and 255 in widths
    for e in ('pt16',):
        assert all(make_batch(j['row'])[0]['start_X'].shape[0] % 16 for j in jobs_of_table()[e]), e


def _check_names(tag, names, plan):
    gen = [n for n in names if n.startswith(('k_gen_', 'k_gseg_'))]
    assert gen, (tag, 'no generic kernel ran', names)
    assert not [n for n in names if n.startswith(SPECIALISED)], (tag, 'a specialised kernel ran', names)
    if plan == 'seg':
        assert 'k_gseg_ode_fwd' in names, (tag, names)
    else:
        assert 'k_gen_fwd' in names and not any(n.startswith('k_gseg_') for n in names), (tag, names)


_ORACLE = {}


def truth(row, edge, predict):
    key = (row, edge)
    if key not in _ORACLE or (predict and 'path_h' not in _ORACLE[key][1]):
        cfg = ROWS[row][0]
        b, dt, T, until = make_batch(row, edge)
        kw = {'until_T': True} if until else {}
        if cfg['input_size'] != cfg['output_size']:
            kw['get_loss'] = False
        _ORACLE[key] = oracle_pair(cfg, state_dict(row), b, dt, T, predict=predict, **kw)
    return _ORACLE[key]


def family(row, env, edge):
    if edge:
        return 'edge_' + edge
    if env != 'default':
        return env
    lab = row_labels(row, env)
    return 'gru' if 'gru' in lab else ('lds_near_limit' if 'lds_near_limit' in lab else
                                       ('long_rows' if 'long' in lab else 'short_rows'))


def test_generic_envelope_against_float64(tmp_path):
    t0 = time.time()
    jobs = jobs_of_table()
    got = {}
    for env, js in jobs.items():
        got.update(run_child(tmp_path, env, ENVS[env], js, timeout=300))
    ratios, errors = {}, []
    for env, js in jobs.items():
        for j in js:
            if j.get('dropout'):
                continue
            jid, row, edge = j['id'], j['row'], j.get('edge')
            res, info = got[jid]
            try:
                for key in ('names', 'names_auto', 'names_predict'):
                    if key in info:
                        _check_names(jid + ' ' + key, info[key], 'lock' if key == 'names_predict' else j['plan'])
                if env == 'pt16':
                    assert info['B'] % 16, (jid, info['B'])
                floors = (2e-5, 1e-4) if edge == 'longK' else (2e-6, 1e-5)
                o32, o64 = truth(row, edge, bool(j.get('predict')))
                hip_util.check_vs_oracle(jid, o32, o64, res, ratios, family(row, env, edge), *floors,
                                         predict=bool(j.get('predict')))
            except (AssertionError, KeyError, ValueError) as e:   # (every row is checked; reported together)
                errors.append('{}: {!r}'.format(jid, e))
    # dropout: the plans and the paths per tile draw the same masks; the masks move the loss
    for row in DROP:
        ids = ['{}.drop.{}.{}'.format(row, e, p) for e, p in (('default', 'seg'), ('default', 'lock'), ('pt16', 'lock'))]
        ref = got[ids[0]][0]
        try:
            assert np.isfinite(ref['grad_fused']).all() and ref['loss_fused'] > 0
            off = got['{}.default.seg'.format(row)][0]['loss_fused']
            assert abs(ref['loss_fused'] - off) > 1e-4 * abs(off), (row, ref['loss_fused'], off)
            for other in ids[1:]:
                o = got[other][0]
                assert o['loss_fused'] == pytest.approx(ref['loss_fused'], rel=2e-5), (ids[0], other)
                assert rel_l2(o['grad_fused'], ref['grad_fused']) <= 1e-4, (ids[0], other)
        except AssertionError as e:
            errors.append('dropout {}: {}'.format(row, e))
    print('worst ratio per branch family:', json.dumps({k: round(v, 2) for k, v in sorted(ratios.items())}))
    print('module wall time {:.1f} s'.format(time.time() - t0))
    assert not errors, '\n'.join(errors)
