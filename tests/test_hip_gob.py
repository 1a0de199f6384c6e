"""GRU-ODE-Bayes baseline on the GPU (include/njode_gob.h, njode_amd/gru_ode_bayes.py) against the
float64 run of the torch restatement (tests/gob_oracle.py).

The rule is the project's: err(HIP, f64) <= max(2 err(fp32 restatement, f64), floor), with
hip_util.check_vs_oracle's floors -- largest absolute error 2e-6 for hT / path_p / path_h, relative
L2 1e-5 for every gradient tensor, 1e-6 relative for loss and loss_1 -- and, for the golden cases,
SURVEY 8c's HIP-vs-CPU tolerances against the reference's own fp32 results (hip_util.ATOL / RTOL,
LOSS_RTOL, GRAD_REL_L2).  Every case prints its worst err(HIP) / err(fp32) ratio.

Cases: the golden shapes (d = 1 and the climate shape, both impute settings; eval, return_path and
training calls, gradients of loss, of loss + <c, hT> and of loss_1 alone); hip_util.irregular_batch
of the d = 1 batch (a jump at t = 0 with no step before it, an empty time slice, a delta_t that
does not divide the grid, a path without observations); the edges of the envelope (64-wide layers
with d = 32, prep_hidden d = 256, hidden 3 with prep 1, bias=False, B = 1, n_obs = 0, B = 70,
B = 1 030); the
climate clock (4 masked paths on 2 000 Euler steps); dropout with the kernels' own masks through
the restatement's mask source; determinism; five Adam steps; two epochs of train.train with
checkpoint resume; the C ABI's refusals and its buffer sizes between guard bands.

Measured on an MI355X, worst err(HIP) / err(fp32) per family: golden shapes 2.38 (a gradient at
1.4e-7 relative L2), irregular 1.43, envelope edges 2.34 on arrays (hT at 4.9e-8) and 35.6 on a
loss (1.6e-5 of 237: 6.6e-8 relative, where the fp32 restatement happened to land 1.9e-9 from float64),
climate clock 1.98, dropout 2.09, five Adam steps 1.06.  Wherever the ratio exceeds 2 the error is
below the floor; no floor was raised.

(The sweep gives every path its own slab up to 1 024 paths, so B = 70 runs 70 workgroups; a
workgroup takes several paths from B = 1 025 on, which the B = 1 030 case of the envelope runs at
the smallest model on four Euler steps.)
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import gob_util
import guarded
import hip_util
from gob_util import CASES, golden, golden_batch, golden_cfg, part, rel_l2
from njode_amd import _lib, data_utils, schedule
from oracle import dropout_oracle

pytestmark = pytest.mark.gpu

FLOOR_H, FLOOR_G, FLOOR_L = 2e-6, 1e-5, 1e-6


def hip_run(m, b, objective='loss', c_hT=None, return_path=False, grads=True):
    """dict of float64 numpy results of one HIP call: hT, loss, loss_1[, path_p, path_h][, g];
    ``objective``: 'loss', 'loss_1' or (a, b) for a * loss + b * loss_1 (``gob_util.objective_of``)."""
    m.zero_grad(set_to_none=True)
    if return_path:
        with torch.no_grad():
            hT, loss, _, path_t, path_p, path_h, et, ev = gob_util.hip_call(m, b, return_path=True)
        assert et.shape == ev.shape == (path_p.shape[0] - 1 - len(b['times']),) and not et.any() and not ev.any()
        return dict(hT=hT.cpu().numpy().astype(np.float64), loss=float(loss), path_t=path_t,
                    path_p=path_p.cpu().numpy().astype(np.float64), path_h=path_h.cpu().numpy().astype(np.float64))
    with torch.set_grad_enabled(grads):
        hT, loss, class_pred, loss_1 = gob_util.hip_call(m, b)
    assert class_pred.shape == (hT.shape[0], 1)
    res = dict(hT=hT.detach().cpu().numpy().astype(np.float64), loss=float(loss.detach()), loss_1=float(loss_1.detach()))
    if grads:
        c = None if c_hT is None else torch.as_tensor(c_hT, dtype=torch.float32, device=hT.device)
        gob_util.objective_of(objective, loss, loss_1, hT, c).backward()
        res['g'] = {}
        for k, p in m.named_parameters():
            if k.startswith(gob_util.SKIP):
                assert p.grad is None, k
            else:
                res['g'][k] = p.grad.detach().cpu().numpy().astype(np.float64)
    return res


def check(tag, hip, r32, r64, floor_h=FLOOR_H, floor_g=FLOOR_G):
    """The rule, on everything ``hip`` holds; prints the worst ratio."""
    worst, worst_of = 0.0, ''

    def ratio(e, e32, what):
        nonlocal worst, worst_of
        r = e / max(e32, 1e-300) if e > 0 else 0.0
        if r > worst:
            worst, worst_of = r, '{}: {:.2e} / {:.2e}'.format(what, e, e32)

    for key in ('loss', 'loss_1'):
        if key in hip:
            e, e32 = abs(hip[key] - r64[key]), abs(r32[key] - r64[key])
            print('  {:28s} {:10s} err {:.3e}  fp32 {:.3e}  value {:.6g}'.format(tag, key, e, e32, float(r64[key])))
            assert e <= max(2 * e32, FLOOR_L * abs(r64[key])), (tag, key, hip[key], float(r64[key]), e, e32)
            ratio(e, e32, key)
    for key in ('hT', 'path_p', 'path_h'):
        if key in hip:
            assert hip[key].shape == r64[key].shape, (tag, key)
            e, e32 = np.abs(hip[key] - r64[key]).max(), np.abs(r32[key] - r64[key]).max()
            print('  {:28s} {:10s} err {:.3e}  fp32 {:.3e}'.format(tag, key, e, e32))
            assert e <= max(2 * e32, floor_h), (tag, key, e, e32)
            ratio(e, e32, key)
    if 'g' in hip:
        assert set(hip['g']) == set(r64['g']), (tag, sorted(set(hip['g']) ^ set(r64['g'])))
        for k in r64['g']:
            e, e32 = rel_l2(hip['g'][k], r64['g'][k]), rel_l2(r32['g'][k], r64['g'][k])
            print('  {:28s} g.{:32s} err {:.3e}  fp32 {:.3e}'.format(tag, k, e, e32))
            assert e <= max(2 * e32, floor_g), (tag, k, e, e32)
            ratio(e, e32, 'g.' + k)
    print('{:30s} worst err(HIP, f64) / err(fp32, f64) = {:.2f}  ({})'.format(tag, worst, worst_of))


def pair(sd, b, mixing, **kw):
    return (gob_util.restate(sd, b, mixing, torch.float32, **kw),
            gob_util.restate(sd, b, mixing, torch.float64, **kw))


@functools.lru_cache(maxsize=None)
def golden_pair(name, objective='loss', with_c=False, return_path=False):
    g = golden(name)
    b, cfg = golden_batch(g), golden_cfg(g)
    c = c_of(b, cfg) if with_c else None
    return pair(part(g, 'sd.'), b, cfg['mixing'], objective=objective, c_hT=c, return_path=return_path,
                grads=not return_path)


def c_of(b, cfg):
    rng = np.random.RandomState(7)
    return rng.normal(size=(b['start_X'].shape[0], cfg['hidden_size'])).astype(np.float32)


def random_model(cfg, seed, bias=True, dropout_rate=0.0, **options):
    """A HIP model with its seeded initialisation and that state_dict as numpy arrays."""
    torch.manual_seed(seed)
    m = gob_util.hip_model(cfg, None, dropout_rate=dropout_rate, bias=bias, **options)
    return m, {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def random_batch(B, d, n_steps, dt, obs_per_path, seed, mask_p=None):
    """Paths of a random walk on a grid of ``n_steps`` steps of ``dt``; ``obs_per_path`` rows each;
    ``mask_p``: every feature observed with that probability (at least one per row), else M = 1."""
    rng = np.random.RandomState(seed)
    walk = np.cumsum(rng.normal(0.0, 0.2, size=(B, n_steps + 1, d)), axis=1)
    rows = []
    for p in range(B):
        for s in sorted(rng.choice(np.arange(1, n_steps + 1), size=min(obs_per_path, n_steps), replace=False)):
            mk = np.ones(d, dtype=np.float32)
            if mask_p is not None:
                mk = (rng.uniform(size=d) < mask_p).astype(np.float32)
                if mk.sum() == 0:
                    mk[rng.randint(d)] = 1.0
            rows.append((int(s), p, walk[p, s] * mk, mk))
    rows.sort(key=lambda r: (r[0], r[1]))
    grid = sorted({r[0] for r in rows})
    counts = [sum(1 for r in rows if r[0] == s) for s in grid]
    empty = np.zeros((0, d), dtype=np.float32)
    return dict(times=np.array(grid, dtype=np.float64) * dt,
                time_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                X=torch.tensor(np.stack([r[2] for r in rows]) if rows else empty, dtype=torch.float32),
                M=torch.tensor(np.stack([r[3] for r in rows]) if rows else empty, dtype=torch.float32),
                obs_idx=torch.tensor([r[1] for r in rows], dtype=torch.long),
                start_X=torch.tensor(walk[:, 0], dtype=torch.float32), delta_t=dt, T=n_steps * dt)


# ---- 1. the golden shapes ----------------------------------------------------------------------------

@pytest.mark.parametrize('name', CASES)
def test_golden_eval_and_path_calls(name):
    g = golden(name)
    b, cfg = golden_batch(g), golden_cfg(g)
    m = gob_util.hip_model(cfg, part(g, 'sd.')).eval()
    r32, r64 = golden_pair(name, return_path=True)
    ev = hip_run(m, b, grads=False)
    check(name + ' eval', ev, r32, r64)
    pa = hip_run(m, b, return_path=True)
    check(name + ' path', pa, r32, r64)
    assert pa['loss'] == ev['loss'] and np.array_equal(pa['hT'], ev['hT'])
    np.testing.assert_allclose(pa['path_t'], g['path_t'], rtol=0, atol=1e-12)
    # the reference's own fp32 results
    for key in ('loss', 'loss_1'):
        assert abs(ev[key] - float(g[key])) <= hip_util.LOSS_RTOL * abs(float(g[key])), key
    np.testing.assert_allclose(ev['hT'], g['hT'], atol=hip_util.ATOL, rtol=hip_util.RTOL)
    np.testing.assert_allclose(pa['path_h'], g['path_h'], atol=hip_util.ATOL, rtol=hip_util.RTOL)
    np.testing.assert_allclose(pa['path_p'], g['path_p'], atol=hip_util.ATOL, rtol=hip_util.RTOL)
    # evaluate / get_pred take the mean half of path_p with M = 1
    if cfg['input_size'] == 1:
        pred = m.get_pred(b['times'], b['time_ptr'], b['X'].cuda(), b['obs_idx'], b['delta_t'], b['T'],
                          b['start_X'].cuda())
        assert np.array_equal(pred['pred'].cpu().numpy().astype(np.float64), pa['path_p'][:, :, :1])
        assert np.array_equal(pred['pred_t'], pa['path_t'])


@pytest.mark.parametrize('objective, with_c', [('loss', False), ('loss', True), ('loss_1', False)])
@pytest.mark.parametrize('name', CASES)
def test_golden_training_call_gradients(name, objective, with_c):
    g = golden(name)
    b, cfg = golden_batch(g), golden_cfg(g)
    m = gob_util.hip_model(cfg, part(g, 'sd.')).train()
    r32, r64 = golden_pair(name, objective, with_c)
    res = hip_run(m, b, objective, c_of(b, cfg) if with_c else None)
    check('{} {}{}'.format(name, objective, '+c.hT' if with_c else ''), res, r32, r64)
    if objective == 'loss' and not with_c:
        for k, ref in part(g, 'g.').items():
            assert rel_l2(res['g'][k], ref) <= hip_util.GRAD_REL_L2, k


# ---- 2. irregular schedules ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['gob_d1_plain', 'gob_d1_impute'])
def test_irregular_batch(name):
    g = golden(name)
    b0, cfg = golden_batch(g), golden_cfg(g)
    hb = dict(times=b0['times'], time_ptr=b0['time_ptr'], X=b0['X'], M=b0['M'], obs_idx=b0['obs_idx'],
              start_X=b0['start_X'], n_obs_ot=torch.bincount(b0['obs_idx'], minlength=b0['start_X'].shape[0]))
    ib, dt = hip_util.irregular_batch(hb, b0['delta_t'])
    b = dict(ib, delta_t=dt, T=b0['T'])
    assert b['times'][0] == 0.0 and (np.diff(b['time_ptr']) == 0).any() and int(b['n_obs_ot'].min()) == 0
    sd = part(g, 'sd.')
    m = gob_util.hip_model(cfg, sd)
    r32, r64 = pair(sd, b, cfg['mixing'], c_hT=c_of(b, cfg))
    check(name + ' irregular', hip_run(m.train(), b, c_hT=c_of(b, cfg)), r32, r64)
    p32, p64 = pair(sd, b, cfg['mixing'], grads=False, return_path=True)
    check(name + ' irregular path', hip_run(m.eval(), b, return_path=True), p32, p64)


# ---- 3. the edges of the envelope ---------------------------------------------------------------------

ENVELOPE = [
    # tag, cfg, bias, B, n_steps, obs per path, mask_p
    ('wide64_d32', dict(input_size=32, hidden_size=64, p_hidden=64, prep_hidden=8, cov_hidden=64), True, 3, 12, 3, 0.5),
    ('prep256', dict(input_size=4, hidden_size=20, p_hidden=12, prep_hidden=64, cov_hidden=9), True, 3, 12, 3, 0.7),
    ('prep256_d1', dict(input_size=1, hidden_size=7, p_hidden=5, prep_hidden=256, cov_hidden=4), True, 2, 10, 3, None),
    ('tiny_h3_prep1', dict(input_size=2, hidden_size=3, p_hidden=1, prep_hidden=1, cov_hidden=1), True, 5, 12, 4, 0.6),
    ('no_bias', dict(input_size=2, hidden_size=11, p_hidden=9, prep_hidden=5, cov_hidden=6), False, 5, 12, 4, 0.6),
    ('B1', dict(input_size=1, hidden_size=10, p_hidden=10, prep_hidden=10, cov_hidden=10), True, 1, 20, 5, None),
    ('no_obs', dict(input_size=2, hidden_size=10, p_hidden=8, prep_hidden=4, cov_hidden=6), True, 4, 15, 0, None),
    ('B70', dict(input_size=1, hidden_size=10, p_hidden=10, prep_hidden=10, cov_hidden=10), True, 70, 16, 3, None),
    ('B1030_shared_slabs', dict(input_size=1, hidden_size=3, p_hidden=2, prep_hidden=2, cov_hidden=2), True, 1030, 4, 1,
     None),
]


@pytest.mark.parametrize('impute', [False, True])
@pytest.mark.parametrize('tag, cfg, bias, B, n_steps, n_obs_pp, mask_p', ENVELOPE, ids=[e[0] for e in ENVELOPE])
def test_envelope_edges(tag, cfg, bias, B, n_steps, n_obs_pp, mask_p, impute):
    cfg = dict(cfg, mixing=1e-3, impute=impute)
    m, sd = random_model(cfg, seed=len(tag), bias=bias)
    b = random_batch(B, cfg['input_size'], n_steps, 0.05, n_obs_pp, seed=B + n_steps, mask_p=mask_p)
    c = c_of(b, cfg)
    r32, r64 = pair(sd, b, cfg['mixing'], c_hT=c)
    res = hip_run(m.train(), b, c_hT=c)
    check('{} impute={}'.format(tag, impute), res, r32, r64)
    if tag == 'no_obs':
        assert res['loss'] == 0.0 and res['loss_1'] == 0.0
        # (p_model feeds the cell with impute; without it nothing reads it when nobody is observed)
        assert not res['g']['gru_obs.gru_d.weight_ih'].any()
        assert res['g']['p_model.0.weight'].any() == impute
        assert res['g']['gru_c.lin_hh.weight'].any() and res['g']['covariates_map.0.weight'].any()
    if not bias:
        assert 'p_model.0.bias' not in res['g'] and 'gru_obs.gru_d.bias_ih' not in res['g']


# ---- 4. the climate clock -----------------------------------------------------------------------------

def test_climate_clock_2000_steps():
    cfg = dict(input_size=5, hidden_size=50, p_hidden=25, prep_hidden=10, cov_hidden=50, mixing=1e-4, impute=False)
    m, sd = random_model(cfg, seed=21)
    b = random_batch(4, 5, 2000, 0.1, 20, seed=5, mask_p=0.6)
    assert b['T'] == 200.0 and b['delta_t'] == 0.1
    r32, r64 = pair(sd, b, cfg['mixing'])
    check('climate clock', hip_run(m.train(), b), r32, r64)


# ---- 5. dropout ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('p_drop', [0.1, 0.5])
@pytest.mark.parametrize('name', ['gob_d1_impute', 'gob_clim_plain'])
def test_dropout_with_the_kernels_masks(name, p_drop):
    g = golden(name)
    b, cfg = golden_batch(g), golden_cfg(g)
    sd = part(g, 'sd.')
    seed = 0x1234567 * 2 ** 32 + 0x89ABCDE
    m = gob_util.hip_model(cfg, sd, dropout_rate=p_drop, dropout_seed=seed).train()
    first = None
    for step in range(2):       # the step counter moves the masks
        masks = dropout_oracle.KernelMasks('gen', dropout_oracle.call_seed(seed, step), p_drop)
        r32, r64 = pair(sd, b, cfg['mixing'], masks=masks)
        res = hip_run(m, b)
        check('{} p={} step {}'.format(name, p_drop, step), res, r32, r64)
        if first is None:
            first = res
    assert first['loss'] != res['loss']


def test_eval_call_of_a_dropout_model_gives_the_p0_bits():
    g = golden('gob_d1_impute')
    b, cfg = golden_batch(g), golden_cfg(g)
    sd = part(g, 'sd.')
    a = hip_run(gob_util.hip_model(cfg, sd, dropout_rate=0.1).eval(), b, return_path=True)
    z = hip_run(gob_util.hip_model(cfg, sd, dropout_rate=0.0).eval(), b, return_path=True)
    for key in ('hT', 'path_p', 'path_h'):
        assert np.array_equal(a[key], z[key]), key
    assert a['loss'] == z['loss']


# ---- 6. determinism -----------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['gob_d1_impute', 'gob_clim_plain'])
def test_same_call_same_bits(name):
    g = golden(name)
    b, cfg = golden_batch(g), golden_cfg(g)
    runs = []
    for _ in range(2):
        m = gob_util.hip_model(cfg, part(g, 'sd.'), dropout_rate=0.1, dropout_seed=11).train()
        runs.append(hip_run(m, b, c_hT=c_of(b, cfg)))
    assert runs[0]['loss'] == runs[1]['loss'] and runs[0]['loss_1'] == runs[1]['loss_1']
    assert np.array_equal(runs[0]['hT'], runs[1]['hT'])
    for k in runs[0]['g']:
        assert np.array_equal(runs[0]['g'][k], runs[1]['g'][k]), k


# ---- 7. five Adam steps -------------------------------------------------------------------------------

def adam_restated(sd, b, mixing, dtype, steps=5):
    p = gob_util.gob_oracle.cast(sd, dtype, requires_grad=True)
    keys = gob_util.gob_oracle.loss_keys(p)
    opt = torch.optim.Adam([p[k] for k in keys], lr=1e-3, weight_decay=5e-4)
    cast = lambda t: t.to(dtype)
    for _ in range(steps):
        opt.zero_grad()
        out = gob_util.gob_oracle.forward(p, b['times'], b['time_ptr'], cast(b['X']), cast(b['M']), b['obs_idx'],
                                          b['delta_t'], b['T'], cast(b['start_X']), mixing)
        out['loss'].backward()
        opt.step()
    return {k: p[k].detach().numpy().astype(np.float64) for k in keys}


@pytest.mark.parametrize('name', ['gob_d1_plain', 'gob_clim_impute'])
def test_five_adam_steps(name):
    g = golden(name)
    b, cfg = golden_batch(g), golden_cfg(g)
    sd = part(g, 'sd.')
    m = gob_util.hip_model(cfg, sd).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-4)
    snap = {}
    for step in range(1, 6):
        opt.zero_grad()
        gob_util.hip_call(m, b)[1].backward()
        opt.step()
        if step in (1, 5):
            snap[step] = {k: v.cpu().numpy().copy() for k, v in m.state_dict().items()}
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        a32, a64 = (adam_restated(sd, b, cfg['mixing'], dt) for dt in (torch.float32, torch.float64))
    finally:
        torch.set_num_threads(threads)
    worst = 0.0
    for k in a64:
        # (what moved: the update, so that an error is not hidden behind the parameter's own size)
        e, e32 = rel_l2(got[k] - sd[k], a64[k] - sd[k]), rel_l2(a32[k] - sd[k], a64[k] - sd[k])
        print('  adam5 {:34s} err {:.3e}  fp32 {:.3e}'.format(k, e, e32))
        assert e <= max(2 * e32, FLOOR_G), (k, e, e32)
        worst = max(worst, e / max(e32, 1e-300))
    print('{} adam5 worst ratio {:.2f}'.format(name, worst))
    for k in sd:
        if k.startswith(gob_util.SKIP):
            assert np.array_equal(got[k], sd[k].astype(np.float64)), k
    # the reference's own fp32 run, with the tolerances tests/test_hip_parity.py holds NJ-ODE's trained
    # parameters to (Adam's first steps move every entry by about lr whatever its gradient's size, so an
    # entry whose gradient is within rounding of zero can differ by a fraction of lr = 1e-3)
    for step, params in snap.items():
        for k, ref in part(g, 'adam{}.'.format(step)).items():
            print('  adam{} vs golden {:34s} max abs {:.3e}'.format(step, k, np.abs(params[k] - ref).max()))
            np.testing.assert_allclose(params[k], ref, atol=2e-5, rtol=1e-4, err_msg='{} step {}'.format(k, step))


# ---- 8. the harness -----------------------------------------------------------------------------------

def test_train_two_epochs_checkpoint_and_resume(tmp_path):
    from njode_amd import train
    hp = copy.deepcopy(data_utils.hyperparam_default)
    hp.update(nb_paths=200, nb_steps=50, obs_perc=0.1)
    paths, obs, nb_obs, meta = data_utils.create_dataset('BlackScholes', hp, seed=1)
    kw = dict(batch_size=50, other_model='GRU_ODE_Bayes', log=lambda *a: None, dropout_seed=5,
              **{'GRU_ODE_Bayes-impute': True, 'GRU_ODE_Bayes-p_hidden': 8})
    model, metrics = train.train((paths, obs, nb_obs), meta, epochs=2, model_path=str(tmp_path / 'a'), **kw)
    assert len(metrics) == 2 and all(len(r) == len(train.METR_COLUMNS) for r in metrics)
    assert model.impute and model.p_hidden == 8 and model.prep_hidden == 10 and model.mixing == 0.0001
    with open(tmp_path / 'a' / 'id-1' / 'metric_id-1.csv') as f:
        assert f.readline().strip().split(',')[1:] == train.METR_COLUMNS
    # the eval loss of the last row: a fresh eval call on the returned model
    _, val_idx = train.split_indices(len(nb_obs), 0.2, 398)
    val = data_utils.collate_arrays(paths[val_idx], obs[val_idx], nb_obs[val_idx], meta['dt'])
    model.eval()
    with torch.no_grad():
        _, c_loss, _, _ = model(val['times'], val['time_ptr'], val['X'].cuda(), torch.ones_like(val['X']).cuda(),
                                val['obs_idx'], meta['dt'], meta['maturity'], val['start_X'].cuda())
    assert np.isfinite(metrics[1][4]) and float(c_loss) == metrics[1][4]
    # one epoch, then resumed from its checkpoint: the second epoch bit for bit
    train.train((paths, obs, nb_obs), meta, epochs=1, model_path=str(tmp_path / 'b'), **kw)
    resumed, m2 = train.train((paths, obs, nb_obs), meta, epochs=2, model_path=str(tmp_path / 'b'),
                              resume_training=True, **kw)
    assert len(m2) == 1 and m2[0][0] == 2 and m2[0][3] == metrics[1][3] and m2[0][4] == metrics[1][4]
    for (k, a), (_, r) in zip(model.state_dict().items(), resumed.state_dict().items()):
        assert torch.equal(a, r), k


# ---- 9. the C ABI -------------------------------------------------------------------------------------

def golden_abi(name):
    """(cfg, state dict, batch) of a golden case, as ``abi_call`` takes them."""
    g = golden(name)
    return golden_cfg(g), part(g, 'sd.'), golden_batch(g)


def abi_call(cfg, sd, b, phase, min_guard=None):
    """Forward (TRAIN | RETURN_PATH | SAVE_BWD) and backward of a model (with bias slots) on a batch
    through the C ABI with every buffer at exactly its stated size between guard bands."""
    L = _lib.lib()
    dims = _lib.NjodeGobDims(cfg['input_size'], cfg['hidden_size'], cfg['p_hidden'], cfg['prep_hidden'],
                             cfg['cov_hidden'], _lib.GOB_F_BIAS | (_lib.GOB_F_IMPUTE if cfg['impute'] else 0))
    flat = np.concatenate([sd[k].ravel() for k in sd if not k.startswith(gob_util.SKIP)]).astype(np.float32)
    assert flat.size == L.njode_gob_param_count(ctypes.byref(dims))
    sched = schedule.Schedule(b['times'], b['delta_t'], b['T'], True)
    host = np.zeros(sched.packed_nbytes() // 4 + 16, dtype=np.int32)
    sched.pack_into(host, b['time_ptr'].astype(np.int32))
    B, n_obs, H, D = b['start_X'].shape[0], int(b['time_ptr'][-1]), cfg['hidden_size'], cfg['input_size']
    flags = _lib.C_TRAIN | _lib.C_RETURN_PATH | _lib.C_SAVE_BWD
    need = ctypes.c_size_t(0)
    _lib.check(L.njode_gob_workspace_bytes(ctypes.byref(dims), B, n_obs, sched.n_times, sched.n_steps, flags,
                                           ctypes.byref(need)))
    A = guarded.Arena(phase=phase, min_guard=min_guard)
    A.add('params', flat.nbytes, 'nan32').add('start_X', B * D * 4, 'nan32').add('X', n_obs * D * 4, 'nan32')
    A.add('M', n_obs * D * 4, 'nan32').add('obs_idx', n_obs * 4, 'index', modulo=B)
    A.add('hT', B * H * 4).add('loss', 8).add('path_h', sched.n_rows * B * H * 4)
    A.add('path_p', sched.n_rows * B * 2 * D * 4).add('ws', need.value)
    A.add('grad_loss', 4, 'nan32').add('grad_loss_1', 4, 'nan32').add('grad_hT', B * H * 4, 'nan32')
    A.add('grad_params', flat.nbytes)
    A.build()
    A.put('params', torch.from_numpy(flat).cuda())
    A.put('start_X', b['start_X'].cuda()); A.put('X', b['X'].cuda()); A.put('M', b['M'].cuda())
    A.put('obs_idx', b['obs_idx'].to(torch.int32).cuda())
    A.put('grad_loss', torch.ones(1).cuda()); A.put('grad_loss_1', torch.zeros(1).cuda())
    A.put('grad_hT', torch.from_numpy(c_of(b, cfg)).cuda())
    batch = _lib.NjodeBatch(B, n_obs, A.ptr('start_X'), A.ptr('X'), A.ptr('M'), A.ptr('obs_idx'), None, float(B),
                            0, None, None)
    sc = sched.struct(host.ctypes.data)
    lead = (ctypes.byref(dims), A.ptr('params'), ctypes.byref(batch), ctypes.byref(sc), flags, cfg['mixing'],
            0.1, 77)
    stream = torch.cuda.current_stream().cuda_stream
    fwd = lambda ws_bytes=need.value, fl=flags, **kw: L.njode_gob_forward_f32(
        lead[0], kw.get('params', lead[1]), kw.get('batch', lead[2]), kw.get('sched', lead[3]), fl, *lead[5:],
        kw.get('hT', A.ptr('hT')), A.ptr('loss'), A.ptr('path_h'), A.ptr('path_p'), kw.get('ws', A.ptr('ws')),
        ws_bytes, stream)
    bwd = lambda ws_bytes=need.value, fl=flags, **kw: L.njode_gob_backward_f32(
        *lead[:4], fl, *lead[5:], kw.get('grad_loss', A.ptr('grad_loss')), A.ptr('grad_loss_1'), A.ptr('grad_hT'),
        kw.get('grad_params', A.ptr('grad_params')), A.ptr('ws'), ws_bytes, stream)
    A.keep = (host, sc, batch, dims)        # (the host schedule is read by every forward call)
    return A, fwd, bwd, need.value, (B, H, D, sched.n_rows, flat.size)


def test_abi_refusals_are_made_before_launch():
    A, fwd, bwd, need, _ = abi_call(*golden_abi('gob_d1_impute'), 0)
    before = A.mem.clone()
    E = _lib.E_BADARG
    assert fwd(params=None) == E and fwd(batch=None) == E and fwd(sched=None) == E and fwd(hT=None) == E
    assert fwd(ws=None) == E and fwd(ws=A.ptr('ws') + 4) == E
    assert fwd(ws_bytes=need - 1) == _lib.E_WORKSPACE and 'workspace' in _lib.lib().njode_last_error().decode()
    assert fwd(fl=_lib.C_GET_LOSS) == E and fwd(fl=0x1000) == E
    assert bwd(fl=_lib.C_TRAIN) == E and 'SAVE_BWD' in _lib.lib().njode_last_error().decode()
    assert bwd(grad_loss=None) == E and bwd(grad_params=None) == E
    assert bwd(ws_bytes=need - 1) == _lib.E_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(A.mem, before)       # nothing was launched


@pytest.mark.parametrize('name', ['gob_d1_impute', 'gob_clim_plain'])
def test_abi_stays_inside_buffers_of_exactly_the_stated_size(name):
    outs = []
    for phase in (0, 1):
        A, fwd, bwd, need, (B, H, D, n_rows, P) = abi_call(*golden_abi(name), phase)
        assert fwd() == 0, _lib.lib().njode_last_error()
        assert bwd() == 0, _lib.lib().njode_last_error()
        assert A.check() == []
        outs.append([A.view(n, torch.float32).clone() for n in ('hT', 'loss', 'path_h', 'path_p', 'grad_params')])
    for a, z in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, z)     # nothing read from in or around the buffers
