"""Loss options and irregular schedules on every kernel route, against the float64 oracle.

``test_hip_route_matrix`` drives every compiled shape onto every kernel family with one call:
``which_loss='standard'``, ``weight = 0.5`` (the two coefficients of the loss equal), Euler steps that
divide the observation grid (one ``step_dt``) and upstream gradient 1.  The paper loss is written in
seven places of the library and the Euler clock is consumed in fourteen files, so this module runs, for
every ``(configuration, route)`` pair of that module's ``routes()``, on the route's own batch kind:

``easy_w075``     ``which_loss='easy'``, ``weight = 0.75``, the regular schedule;
``std_w02_irr``   ``which_loss='standard'``, ``weight = 0.2`` on ``hip_util.irregular_batch`` (a jump at
                  t = 0 with no Euler step before it, a time slice without rows, a path without
                  observations) at ``delta_t = 0.37 dt`` (every grid interval ends in a partial step),
                  the autograd step as ``(1.7 loss).backward()``;
``std_w02_irr_tail``  (demo, PhysioNet, GRU and ``nn_desc=None`` shapes) the same with ``until_T=True`` and
                  T 2.6 steps past the last observation: the lockstep backward through a tail, the
                  objective ``1.7 loss + (c hT).sum()``.  (The fused step has no ``until_T``; the tail
                  moves hT, not the loss: its loss is compared, its gradient is not.)

Every row runs the fused step and the autograd step, asserts the route's kernel names and batch sizes
like a route-matrix row, and makes an eval-mode prediction call (``return_path=True, get_loss=True,
until_T=True``) whose path_h, path_y, hT and loss are compared as well.  The yardstick is the route
matrix's: err(HIP, f64) <= max(2 err(oracle fp32, f64), floor) with ``check_vs_oracle``'s default floors
(2e-6 hT / paths, 1e-5 gradients, 1e-6 relative for a loss), never looser than ``hip_util``'s ATOL /
RTOL / GRAD_REL_L2 / LOSS_RTOL.  One child process per environment; the parent runs the oracle, cached
per (configuration, batch kind, options).

Worst measured err(HIP, f64) / err(o32, f64) per route family over both row kinds (MI355X, next to the
route matrix's table; a ratio above 2 passes on the default floor, where both errors are at fp32
rounding -- no row needed a higher floor): wave per item 3.75, split <= 384 tiles 8.71, split 385-768
tiles 7.28, mixed 3.90, one-wave tiles (mfma1) 3.76, one-wave shapes 6.03 / 3.80 / 75.0 (one tile / small /
large batch), nn_desc=None 8.98 / 6.84, use_rnn 2.23 / 4.15, wave per path 4.06, four-wave tiles 1.29 / 1.29
(1 / 16 paths per tile), tail rows 1.32 / 1.66 / 2.23 / 2.25 (demo / PhysioNet / GRU / nn_desc=None);
prediction calls at most 3.41.  The module takes 42 s on one MI355X (88 rows; the children 9 s, the
oracle the rest).
"""
import json

import numpy as np
import pytest
import torch

import hip_util
from hip_util import oracle_pair
from njode_amd.build import CONFIGS
from test_hip_route_matrix import (ENVS, GRU, ITEMS, MIXED, c_hT, caps, check_names, check_sizes, job_batch,
                                   job_cfg, model_cfg, routes, run_child)

pytestmark = pytest.mark.gpu

DT_FACTOR = 0.37     # in (0.3, 0.5), does not divide 1: steps of 0.37, 0.37, 0.26 of a grid interval
GRAD_SCALE = 1.7     # not a power of two
ROW_KINDS = {
    'easy_w075': dict(which_loss='easy', weight=0.75),
    'std_w02_irr': dict(which_loss='standard', weight=0.2, irregular=True, dt_factor=DT_FACTOR,
                        grad_scale=GRAD_SCALE),
}
TAIL_KIND = 'std_w02_irr_tail'
TAIL_OPTS = dict(ROW_KINDS['std_w02_irr'], until_T=True)
PLAN_KEYS, SPLIT_KMAX = 512, 4095   # njode_plan.h


def tail_shapes():
    """Index of the demo shape, one PhysioNet shape, the GRU shape and the nn_desc=None shape."""
    demo = 0
    physio = next(i for i, c in enumerate(CONFIGS) if caps(c)['HAS_CHAIN'])
    gru = next(i for i, c in enumerate(CONFIGS) if c[9])
    linear = next(i for i, c in enumerate(CONFIGS) if c[3] == 0)
    return [demo, physio, gru, linear]


def expected_rows():
    """Every (configuration index, route name, row kind) the module must have checked."""
    out = set()
    for i, c in enumerate(CONFIGS):
        for name, env, kind, must, must_not in routes(c):
            out |= {(i, name, 'easy_w075'), (i, name, 'std_w02_irr')}
    for i in tail_shapes():
        out.add((i, routes(CONFIGS[i])[0][0], TAIL_KIND))
    return out


# ---- parent side: the oracle -------------------------------------------------------------------------
_ORACLE = {}


def truth(c, job):
    """((f32, f64) of the training step, (f32, f64) of the prediction call) of a job."""
    key = (tuple(c), job['batch'], tuple(sorted((k, job.get(k)) for k in TAIL_OPTS)))
    if key not in _ORACLE:
        from njode_amd import models
        torch.manual_seed(0)
        sd = {k: v.detach().clone() for k, v in models.NJODE(**model_cfg(c)).state_dict().items()}
        cfg = job_cfg(job, c)
        b, dt, T = job_batch(job, c)
        scale = job.get('grad_scale', 1.0)
        kw = {}
        if job.get('until_T'):   # d (scale loss + (c hT).sum()) = scale d (loss + (c / scale hT).sum())
            kw = dict(until_T=True, c_hT=c_hT(len(b['start_X']), c[1]) / scale)
        train = oracle_pair(cfg, sd, b, dt, T, **kw)
        for o in train:
            o['g'] = {k: scale * v for k, v in o['g'].items()}
        pred = oracle_pair(cfg, sd, b, dt, T, predict=True, grads=False, until_T=True)
        _ORACLE[key] = (train, pred)
    return _ORACLE[key]


def check_schedule(jid, c, job, seg_plan):
    """The properties of the irregular batch the rows rely on, on the Schedule of the training call."""
    from njode_amd.schedule import Schedule
    b, dt, T = job_batch(job, c)
    until = bool(job.get('until_T'))
    s = Schedule(b['times'], dt, T, until)
    assert len(set(s.step_dt.tolist())) >= 2, (jid, 'one step_dt')
    assert s.has_tail() == until, (jid, 'tail')
    assert s.k_jump[0] == 0 and b['times'][0] == 0.0 and b['obs_idx'][0] == 0, (jid, 'no jump at t = 0')
    assert (np.diff(b['time_ptr']) == 0).any(), (jid, 'no empty slice')
    assert (b['n_obs_ot'] == 0).any(), (jid, 'every path observed')
    # the segment plan's one-launch plan needs K + 1 <= PLAN_KEYS
    assert s.n_steps < (PLAN_KEYS if seg_plan else SPLIT_KMAX), (jid, s.n_steps)


RATIOS = {}
# lockstep kernels of the tail rows' autograd step, by the name of the shape's first route
# (the names of the first green run)
TAIL_MUST = {'items': ['k_paths_fwd_mfma', 'k_paths_bwd_adj_mfma'], 'chain': ['k_paths_fwd_chain', 'k_paths_bwd_adj_chain'],
             'gru': GRU, 'linear': ['k_paths_fwd', 'k_paths_bwd_adj']}


def _check(jid, i, name, rk, c, job, env, must, must_not, res, info):
    kind = job['batch']
    masked, until = bool(c[6]), bool(job.get('until_T'))
    if job.get('irregular'):
        check_schedule(jid, c, job, seg_plan=not masked and not c[9] and not until)
    (o32, o64), (p32, p64) = truth(c, job)
    # (the fused step has no until_T: it stays on the route)
    check_names(jid, info['names'], must, must_not)
    if until:
        # the tail takes an unmasked shape off the segment plan, onto the lockstep kernels
        check_names(jid + ' (autograd, tail)', info['names_auto'], TAIL_MUST[name], ITEMS + MIXED)
    else:
        check_names(jid + ' (autograd)', info['names_auto'],
                    [m for m in must if 'dw_stored' not in m and 'dw_pairs' not in m], must_not)
    # a prediction call: the lockstep plan, never the segment plan's kernels
    check_names(jid + ' (prediction)', info['names_predict_loss'],
                ['k_paths_fwd_chain'] if masked and env == 'default' else [], ITEMS + MIXED)
    check_sizes(kind, info['n_obs'], info['B'])
    hip_util.check_vs_oracle(jid, o32, o64, res, RATIOS, name)
    pr = {'hT': res['p.hT'], 'path_h': res['p.path_h'], 'path_y': res['p.path_y'], 'loss_predict': float(res['p.loss'])}
    hip_util.check_vs_oracle(jid + ' (prediction)', p32, p64, pr, RATIOS, name + ' prediction', predict=True)


def test_loss_options_and_irregular_schedules_on_every_route(tmp_path):
    jobs = {env: [] for env in ENVS}
    rows = []
    for i, c in enumerate(CONFIGS):
        for r, (name, env, kind, must, must_not) in enumerate(routes(c)):
            kinds = dict(ROW_KINDS)
            if r == 0 and i in tail_shapes():
                kinds[TAIL_KIND] = TAIL_OPTS
            for rk, opts in kinds.items():
                jid = 'c{}_{}_{}'.format(i, name, rk)
                job = dict({'id': jid, 'cfg': list(c), 'batch': kind, 'dropout': 0.0, 'predict_loss': True}, **opts)
                jobs[env].append(job)
                rows.append((jid, i, name, rk, c, job, env, must, must_not))
    got = {}
    for env, js in jobs.items():
        got.update(run_child(tmp_path, 'opt_' + env, ENVS[env], js, timeout=600))
    errors, checked = [], set()
    for row in rows:
        jid, i, name, rk = row[:4]
        checked.add((i, name, rk))
        try:
            _check(*row, *got[jid])
        except AssertionError as e:   # (every row is checked; the failures are reported together)
            errors.append('{}: {}'.format(jid, e))
    print('worst ratio per route family:', json.dumps({k: round(v, 2) for k, v in sorted(RATIOS.items())}))
    assert not errors, '\n'.join(errors)
    # coverage: every (configuration, route) pair produced both rows, the four lockstep shapes their tail row
    want = expected_rows()
    assert checked == want, (sorted(want - checked), sorted(checked - want))
    assert sum(1 for x in checked if x[2] == TAIL_KIND) == 4
