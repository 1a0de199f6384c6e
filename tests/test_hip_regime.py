"""Regime-switch and Heston-without-Feller datasets on the GPU: ``njode_generate_stage``,
``njode_cond_exp_staged_f64`` and their Python surface (``DeviceDataset.generate`` with
``'HestonWOFeller'``, ``DeviceDataset.generate_combined``, ``device_data.cond_exp`` with a
``HestonWOFeller`` / ``Combined`` description, ``NJODE.evaluate_device``, ``train(device_eval=True)``).

What is held to what (eps = 2**-52):

* **HestonWOFeller generation, step-local.**  The host's one-step formula
  (``stock_model.HestonWOFeller.generate_paths``) on the DEVICE's own previous spot and variance
  (a ``return_vol`` run stores both) against the device's next values; the run without
  ``return_vol`` must give the spot coordinates of the run with it bit for bit (same kernel, same
  draws).  With ``L = (log(s) + A dt) + B dW``, ``A = drift pc - 0.5 vp``, ``B = sqrt(vp)``,
  ``vp = max(v, 0)``, ``M = |log s| + |A| dt + |B dW|`` and the library bounds the repository
  already uses (``tests/test_hip_cond_exp.py``, ``tests/test_hip_producer_matrix.py``: host ``exp``
  / ``sin`` / ``log`` within 1 ulp, device ``exp`` 3, ``sin`` 4, ``log`` 3 ulp, ``sqrt`` within 1
  ulp of each other):

  - ``log(s)``: (3 + 1) eps ``|log s|``; ``pc = 1 + sin(c t)``: 7 eps absolute (as derived for the
    conditional expectation), times ``|drift| dt``; ``B``: 1 eps ``|B dW|``;
  - five re-rounded operations downstream of a perturbed operand (``drift pc``, ``- 0.5 vp``,
    ``* dt``, the two additions) and the product ``B dW``: at most one ulp of a term of ``M``
    each: 6 eps ``M``;
  - ``exp(L)``: (3 + 1) eps relative, and the argument's absolute error is relative in the result:

        allow_s = |s'| eps (4 + 4 |log s| + 7 |drift| dt + 7 M)        (6 M + 1 |B dW| <= 7 M)

  - the variance ``v' = (v + (-speed (vp - mean)) dt) + (volatility B) dZ`` has no libm call but
    the root: 1 eps of ``|volatility B dZ|`` from it, two re-rounded products and the re-rounded
    sum:  ``allow_v = eps (4 |volatility B dZ| + |v'|)``.

  On the Philox route the normals of the two sides differ as derived in
  ``tests/test_hip_producer_matrix.py``: ``dz = eps (K_Z |z| + K_TRIG R_MAX)``, K_Z = 4,
  K_TRIG = 8, R_MAX = 8.572; it enters ``L`` through ``B sqrt(dt) dz1`` and ``v'`` through
  ``volatility B sqrt(dt) (|rho| dz1 + sqrt(1 - rho^2) dz2)``, each with one more re-rounded
  product (1 eps of the term, inside the 7 M / the 4 above).
* **Staged generation.**  Every stage against its HOST generator on the restated draws (global
  grid index in the Philox counter), started from the device's previous slice; stages of at most
  7 steps: the suite's ``rtol = 1e-12`` for whole short trajectories.  The boundary slice is
  bit-identical before and after the later stage's call.  ``generate_combined`` of two equal
  stages without sine equals ``generate`` of twice the steps and maturity bit for bit (``T/S`` and
  ``2T/2S`` are the same double, the counters are the same); with sine they differ.
* **Staged conditional expectation**: the standards of ``tests/test_hip_cond_exp.py`` unchanged
  (step-local ``7 eps (|y| + |mean|)``, jumps bit for bit, trajectories ``8 eps (steps since the
  path's last reset + 1)``, loss 1e-12, fused metric ``(N - 1) eps``, reproducible bits), against
  the host ``Combined`` walk on float64 copies of the fp32 batch.  ``|rate| delta_t <= 0.025`` is
  asserted for every stage (the derivation's premise).
* A single old-model stage gives the bits of ``njode_cond_exp_f64``.

Measured on an MI355X: see DESIGN.md section 4e.
"""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from guarded import Arena
from hip_util import demo_cfg, hip_model, to_dev
from njode_amd import _lib, data_utils, device_data, schedule, stock_model, train
from oracle import producer_oracle as po

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
STEP_C = 7.0
K_Z, K_TRIG, R_MAX = 4.0, 8.0, 8.572
SINE = 2 * np.pi
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DDS = device_data.DeviceDataset


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hp(N, S, dim, sine=False, dt=0.01, **kw):
    """``dt = 2**-6`` where stages of different lengths must agree in ``maturity / nb_steps`` to the bit"""
    hp = copy.deepcopy(data_utils.hyperparam_default)
    hp.update(nb_paths=N, nb_steps=S, S0=[1.0] * dim if dim > 1 else 1, dimension=dim, maturity=S * dt)
    if sine:
        hp['sine_coeff'] = SINE
    hp.update(kw)
    return hp


# ---- HestonWOFeller generation -------------------------------------------------------------------
def hwf_step_ratio(hp, got, z, philox):
    """largest |device step - host one-step formula on the device's previous values| / allowance;
    ``got`` [N, 2 d, S + 1] of a return_vol run, ``z`` [N, S, 2, d]"""
    d, S = got.shape[1] // 2, hp['nb_steps']
    dt = hp['maturity'] / S
    sq, rho, sine = np.sqrt(dt), hp['correlation'], hp.get('sine_coeff')
    rho_c = np.sqrt(1 - rho ** 2)
    worst_s = worst_v = 0.0
    for k in range(1, S + 1):
        s, v = got[:, :d, k - 1], got[:, d:, k - 1]
        z1, z2 = z[:, k - 1, 0, :], z[:, k - 1, 1, :]
        pc = 1 if sine is None else (1 + np.sin(sine * ((k - 1) * dt)))
        dW = z1 * sq
        dZ = (rho * z1 + rho_c * z2) * sq
        vp = np.maximum(v, 0)
        A, B = hp['drift'] * pc - 0.5 * vp, np.sqrt(vp)
        want_s = np.exp(np.log(s) + A * dt + B * dW)
        want_v = v + (-hp['speed'] * (vp - hp['mean'])) * dt + (hp['volatility'] * B) * dZ
        M = np.abs(np.log(s)) + np.abs(A) * dt + np.abs(B * dW)
        dz1 = (K_Z * np.abs(z1) + K_TRIG * R_MAX) if philox else 0.0
        dz2 = (K_Z * np.abs(z2) + K_TRIG * R_MAX) if philox else 0.0
        allow_s = np.abs(want_s) * EPS * (4 + 4 * np.abs(np.log(s)) + 7 * abs(hp['drift']) * dt + 7 * M
                                          + B * sq * dz1)
        allow_v = EPS * (4 * np.abs(hp['volatility'] * B * dZ) + np.abs(want_v)
                         + hp['volatility'] * B * sq * (abs(rho) * dz1 + rho_c * dz2))
        worst_s = max(worst_s, float((np.abs(got[:, :d, k] - want_s) / allow_s).max()))
        worst_v = max(worst_v, float((np.abs(got[:, d:, k] - want_v) / allow_v).max()))
    return worst_s, worst_v


# every shape; the options rotate so that each value meets each N, S and dim
HWF_ROWS = [(N, S, dim, i % 2 == 1, (-0.7, 0.0, 1.0)[(i // 2) % 3], i % 4 >= 2)
            for i, (N, S, dim) in enumerate((N, S, dim) for N in (1, 63, 257) for S in (1, 2, 7) for dim in (1, 3))]


@pytest.mark.parametrize('row', HWF_ROWS, ids=lambda r: 'N{}-S{}-d{}-sine{}-rho{}-nofeller{}'.format(*r))
def test_generate_heston_wo_feller(row):
    N, S, dim, sine, rho, no_feller = row
    hp = _hp(N, S, dim, sine, correlation=rho, v0=0.3, maturity=S * 0.05, obs_perc=0.5)
    if no_feller:
        hp.update(volatility=2.5, mean=0.05, speed=0.5, v0=0.02)
        assert 2 * hp['speed'] * hp['mean'] < hp['volatility'] ** 2
    seed = 1000 + N + S
    for philox in (False, True):
        if philox:
            z = np.stack(po.path_normals(N, S, dim, seed), axis=2)           # [N, S, 2, d]
            normals = None
        else:
            z = np.random.RandomState(seed).standard_normal((N, S, 2, dim))   # the reference's draw order
            normals = z
        vol = DDS.generate('HestonWOFeller', dict(hp, return_vol=True), seed=seed, normals=normals)
        flat = DDS.generate('HestonWOFeller', dict(hp, return_vol=False), seed=seed, normals=normals)
        assert vol.dim == 2 * dim and flat.dim == dim and vol.metadata['model_name'] == 'HestonWOFeller'
        got, got_flat = vol.to_arrays()[0], flat.to_arrays()[0]
        assert got.shape == (N, 2 * dim, S + 1) and np.isfinite(got).all()
        assert np.array_equal(got[:, :dim, 0], np.full((N, dim), 1.0)) and np.all(got[:, dim:, 0] == hp['v0'])
        assert np.array_equal(got_flat, got[:, :dim])
        ws, wv = hwf_step_ratio(hp, got, z, philox)
        print('HWF-STEP-LOCAL {} philox {}: spot {:.4f} variance {:.4f} of the allowance'.format(row, philox, ws, wv))
        assert ws <= 1.0 and wv <= 1.0, (ws, wv)
        again = DDS.generate('HestonWOFeller', dict(hp, return_vol=True), seed=seed, normals=normals)
        assert torch.equal(again.paths_tm, vol.paths_tm)
    with pytest.raises(ValueError, match='unknown sampling scheme'):
        DDS.generate('HestonWOFeller', dict(hp, scheme='milstein'), seed=1)


def test_heston_wo_feller_clamp_is_exercised():
    hp = _hp(257, 7, 1, volatility=2.5, mean=0.05, speed=0.5, v0=0.02, maturity=0.35, return_vol=True)
    got = DDS.generate('HestonWOFeller', hp, seed=5).to_arrays()[0]
    assert (got[:, 1:, :] < 0).any() and np.isfinite(got).all() and (got[:, :1, :] > 0).all()


# ---- staged generation ----------------------------------------------------------------------------
def stage_draws(name, N, s0, S_i, S_total, dim, seed):
    """the draws njode_generate_stage takes for grid indices s0 + 1 .. s0 + S_i, host layout"""
    if name in ('Heston', 'HestonWOFeller'):
        return np.stack(po.path_normals(N, S_total, dim, seed), axis=2)[:, s0:s0 + S_i]
    return po.step_normals(N, S_total, dim, seed)[:, s0:s0 + S_i]


@pytest.mark.parametrize('names', [('BlackScholes', 'OrnsteinUhlenbeck', 'BlackScholes'),
                                   ('OrnsteinUhlenbeck', 'BlackScholes', 'HestonWOFeller'),
                                   ('Heston', 'OrnsteinUhlenbeck', 'OrnsteinUhlenbeck')])
@pytest.mark.parametrize('sine', [False, True])
def test_staged_generation_against_the_host_generators(names, sine):
    N, dim, steps, seed = 257, 3, (7, 1, 2), 0xC0FFEE
    S = sum(steps)
    hps = [_hp(N, s, dim, sine, dt=2.0 ** -6, v0=0.3, obs_perc=0.4) for s in steps]
    L = _lib.lib()
    paths = torch.full((S + 1, dim, N), float('nan'), dtype=torch.float64, device='cuda')
    s0 = 0
    for name, hp in zip(names, hps):
        st = device_data.stage_struct(name, hp, dim, first_step=s0)
        before = paths[s0].clone()
        _lib.check(L.njode_generate_stage(ctypes.byref(st), S, ctypes.c_uint64(seed), None, paths.data_ptr(), _stream()))
        torch.cuda.synchronize()
        if s0:
            assert torch.equal(paths[s0], before)                       # the boundary slice is only read
        assert bool(torch.isnan(paths[s0 + hp['nb_steps'] + 1:]).all())   # nothing beyond the stage
        got = paths[s0:s0 + hp['nb_steps'] + 1].permute(2, 1, 0).cpu().numpy()
        z = stage_draws(name, N, s0, hp['nb_steps'], S, dim, seed)
        with po._normal_draws(z):
            ref, _ = stock_model.STOCK_MODELS[name](**hp).generate_paths(start_X=None if s0 == 0 else got[:, :, 0])
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, err_msg='{} at {}'.format(name, s0))
        s0 += hp['nb_steps']
    # the wrapper: the same bits, the mask of one draw over the whole grid, the reference's metadata
    ds = DDS.generate_combined(names, hps, seed=seed)
    assert torch.equal(ds.paths_tm, paths)
    u = po.observation_uniforms(N, S, seed)
    _, obs, nb = ds.to_arrays()
    assert np.array_equal(obs, (u < 0.4) * 1) and np.array_equal(nb, obs[:, 1:].sum(1))
    m = ds.metadata
    assert set(m) == {'dt', 'maturity', 'dimension', 'nb_paths', 'model_name', 'stock_model_names', 'hyperparam_dicts'}
    assert m['model_name'] == 'combined' and m['stock_model_names'] == list(names) and m['nb_paths'] == N
    assert m['dt'] == 2.0 ** -6 and m['maturity'] == 10 * 2.0 ** -6
    assert [h['model_name'] for h in m['hyperparam_dicts']] == list(names)
    # supplied normals keep their meaning per stage: the stage's own [N][S_i](x2)[dim] block.  The
    # restated normals are numpy's Box-Muller values, a few ulp from the device's own, so the two
    # datasets agree to the suite's rtol for short trajectories, not to the bit
    zs = [stage_draws(n, N, o, s, S, dim, seed) for n, o, s in zip(names, (0, 7, 8), steps)]
    given = DDS.generate_combined(names, hps, seed=1, normals=zs)
    np.testing.assert_allclose(given.paths_tm.cpu().numpy(), paths.cpu().numpy(), rtol=1e-12, atol=0)
    assert torch.equal(DDS.generate_combined(names, hps, seed=2, normals=zs).paths_tm, given.paths_tm)


@pytest.mark.parametrize('name', ['BlackScholes', 'OrnsteinUhlenbeck'])
def test_two_equal_stages_are_one_run_of_twice_the_steps(name):
    N, dim, S = 257, 3, 7                     # an odd S: the second stage starts inside a pair
    hp = _hp(N, S, dim)
    two = DDS.generate_combined([name, name], [hp, hp], seed=9)
    one = DDS.generate(name, dict(hp, nb_steps=2 * S, maturity=2 * hp['maturity']), seed=9)
    assert hp['maturity'] / S == 2 * hp['maturity'] / (2 * S)
    assert torch.equal(two.paths_tm, one.paths_tm)
    assert torch.equal(two.observed_tm, one.observed_tm) and torch.equal(two.nb_obs, one.nb_obs)
    hs = dict(hp, sine_coeff=SINE)            # the stage-local time restarts: with sine they differ
    two = DDS.generate_combined([name, name], [hs, hs], seed=9)
    one = DDS.generate(name, dict(hs, nb_steps=2 * S, maturity=2 * hp['maturity']), seed=9)
    assert torch.equal(two.paths_tm[:S + 1], one.paths_tm[:S + 1])
    assert not torch.equal(two.paths_tm[S + 1:], one.paths_tm[S + 1:])


def test_generate_combined_refusals():
    hp = _hp(5, 4, 2)
    with pytest.raises(ValueError):
        DDS.generate_combined(['BlackScholes', 'HestonWOFeller'], [hp, dict(hp, return_vol=True)])
    with pytest.raises(ValueError):
        DDS.generate_combined(['BlackScholes', 'OrnsteinUhlenbeck'], [hp, dict(hp, nb_paths=6)])
    with pytest.raises(ValueError):
        DDS.generate_combined(['BlackScholes', 'OrnsteinUhlenbeck'], [hp, dict(hp, nb_steps=5)])
    with pytest.raises(KeyError):
        DDS.generate_combined(['BlackScholes', 'FractionalBM'], [hp, hp])


# ---- staged conditional expectation ----------------------------------------------------------------
def regime_case(names, dim, sine, B, seed=0):
    """(host batch, delta_t, Combined model, metadata).  20 steps of 0.01 per stage.
    B = 1: the second stage has no observation.  B = 63: delta_t = 0.37 dt (a partial step at every
    boundary), no observation on a boundary, path 1 unobserved.  B = 257: path 0 observed on every
    boundary, path 1 unobserved."""
    S = 20
    hps = [_hp(B, S, dim, sine, obs_perc=0.5 if B == 1 else 0.15) for _ in names]
    paths, obs, nb_obs, meta = data_utils.create_combined_dataset(list(names), hps, seed=seed)
    assert np.isfinite(paths).all()
    obs = obs.copy()
    bounds = [S * (i + 1) for i in range(len(names))]
    if B == 1:
        obs[:, S + 1:2 * S + 1] = 0
    if B == 63:
        obs[:, bounds] = 0
    if B == 257:
        obs[0, bounds] = 1
    if B >= 63:
        obs[1, :] = 0
    nb_obs = obs[:, 1:].sum(axis=1)
    b = data_utils.collate_arrays(paths, obs, nb_obs, meta['dt'])
    b = {k: b[k] for k in ('times', 'time_ptr', 'X', 'obs_idx', 'start_X', 'n_obs_ot')}
    delta_t = 0.37 * meta['dt'] if B == 63 else meta['dt']
    return b, delta_t, stock_model.Combined(**meta), meta


def host_walk(sm, b, delta_t, weight=0.5, T=None):
    return sm.compute_cond_exp(
        b['times'], b['time_ptr'], b['X'].numpy().astype(np.float64), b['obs_idx'].numpy(), delta_t, T,
        b['start_X'].numpy().astype(np.float64), b['n_obs_ot'].numpy(), return_path=True, get_loss=True,
        weight=weight)


def dev_call(sm, b, delta_t, T=0.0, **kw):
    d = to_dev(b)
    return device_data.cond_exp(sm, d['times'], d['time_ptr'], d['X'], d['obs_idx'], delta_t, T, d['start_X'],
                                n_obs_ot=d['n_obs_ot'], **kw)


def check_walk(tag, b, delta_t, sm, clock, stage_models, mean_of, T=None):
    """the standards of tests/test_hip_cond_exp.py on one case; ``stage_models[i]``: the single
    model of stage i, ``mean_of(stage) -> [d]`` the |mean| of the step-local allowance"""
    B, dim = b['start_X'].shape
    c = clock
    n_t = 1 + c.n_steps + c.n_times
    jrow = {int(r): i for i, r in enumerate(c.row_of_jump)}
    idx, ptr = b['obs_idx'].numpy(), np.asarray(b['time_ptr'])
    X64 = b['X'].numpy().astype(np.float64)
    loss_h, path_t_h, path_h = host_walk(sm, b, delta_t, 0.5, T)
    rng = np.random.RandomState(7)
    pred = torch.from_numpy((path_h * (1 + 0.05 * rng.standard_normal(path_h.shape))).astype(np.float32))
    kw = dict(want_path=True, want_loss=True, pred=pred.cuda(), weight=0.5)
    path_t, path_d, loss_d, sq_d = dev_call(sm, b, delta_t, T or 0.0, **kw)
    assert np.array_equal(path_t, path_t_h)
    assert path_d.dtype == torch.float64 and tuple(path_d.shape) == (n_t, B, dim) == path_h.shape
    y = path_d.cpu().numpy()
    assert np.array_equal(y[0], b['start_X'].numpy().astype(np.float64))
    worst, since, k = 0.0, np.zeros(B), 0
    for r in range(1, n_t):
        if r not in jrow:
            stage = int(np.searchsorted(c.stage_first, k, side='right')) - 1
            want = stage_models[stage].next_cond_exp(y[r - 1], c.step_dt[k], c.step_t[k])
            allow = STEP_C * EPS * (np.abs(y[r - 1]) + np.abs(mean_of(stage))[None, :])
            err = np.abs(y[r] - want)
            worst = max(worst, float((err / allow).max()))
            assert (err <= allow).all(), (tag, r, k, stage, float((err / allow).max()))
            since += 1
            k += 1
        else:
            i = jrow[r]
            rows = np.arange(ptr[i], ptr[i + 1])
            seen = np.zeros(B, dtype=bool)
            seen[idx[rows]] = True
            assert np.array_equal(y[r][idx[rows]], X64[rows]), (tag, r)
            assert np.array_equal(y[r][~seen], y[r - 1][~seen]), (tag, r)
            since[seen] = 0
        bound = 8 * EPS * (since + 1)[:, None] * np.abs(path_h[r])
        assert (np.abs(y[r] - path_h[r]) <= bound).all(), (tag, r)
    print('REGIME-STEP-LOCAL {}: largest error / allowance = {:.3f}'.format(tag, worst))
    assert float(loss_d) == pytest.approx(float(loss_h), rel=1e-12)
    loss_h8 = host_walk(sm, b, delta_t, 0.8, T)[0]
    loss_d8 = dev_call(sm, b, delta_t, T or 0.0, want_loss=True, weight=0.8)[2]
    assert float(loss_d8) == pytest.approx(float(loss_h8), rel=1e-12)
    N = y.size
    ref = np.mean((pred.numpy().astype(np.float64) - y) ** 2)
    assert ref > 0 and abs(float(sq_d) / N - ref) <= (N - 1) * EPS * ref
    _, path_2, loss_2, sq_2 = dev_call(sm, b, delta_t, T or 0.0, **kw)
    assert torch.equal(path_2, path_d) and torch.equal(loss_2, loss_d) and torch.equal(sq_2, sq_d)
    _, none_p, none_l, sq_3 = dev_call(sm, b, delta_t, T or 0.0, pred=pred.cuda())
    assert none_p is None and none_l is None and torch.equal(sq_3, sq_d)
    return y, path_h


REGIMES = [('BlackScholes', 'OrnsteinUhlenbeck'), ('Heston', 'HestonWOFeller'),
           ('OrnsteinUhlenbeck', 'HestonWOFeller', 'BlackScholes')]
REGIME_CASES = [(n, d, s, B) for n in REGIMES for d in (1, 3) for s in (False, True) for B in (1, 63, 257)]


@pytest.mark.parametrize('names,dim,sine,B', REGIME_CASES,
                         ids=lambda v: '-'.join(x[:2] for x in v) if isinstance(v, tuple) else str(v))
def test_staged_cond_exp_against_the_host_walk(names, dim, sine, B):
    b, delta_t, sm, meta = regime_case(names, dim, sine, B)
    hps = meta['hyperparam_dicts']
    mats = [h['maturity'] for h in hps]
    c = schedule.cond_exp_clock(b['times'], delta_t, 0.0, mats)
    singles = [stock_model.STOCK_MODELS[n](**h) for n, h in zip(names, hps)]
    for n, h in zip(names, hps):
        assert abs(h['speed'] if n == 'OrnsteinUhlenbeck' else h['drift']) * delta_t <= 0.025
    # the case reaches what it stands for
    ends = np.cumsum(mats)
    on_boundary = [bool(np.any(np.abs(b['times'] - e) <= 1e-10)) for e in ends]
    if B == 1:
        assert not np.any((b['times'] > ends[0] + 1e-9) & (b['times'] <= ends[1] + 1e-9))   # a stage without rows
    if B == 63:
        assert not any(on_boundary) and b['n_obs_ot'][1] == 0
        last = c.stage_first[1:] - 1
        assert np.all(c.step_dt[last] < delta_t * (1 - 1e-9))                               # partial steps
    if B == 257:
        assert all(on_boundary) and b['n_obs_ot'][1] == 0
    mean_of = lambda st: np.full(dim, float(hps[st]['mean']) if names[st] == 'OrnsteinUhlenbeck' else 0.0)
    check_walk('{} dim {} sine {} B {}'.format('>'.join(n[:3] for n in names), dim, sine, B), b, delta_t, sm, c,
               singles, mean_of)
    # the metadata dict describes the same model
    p1 = dev_call(meta, b, delta_t, want_path=True)[1]
    p2 = dev_call(sm, b, delta_t, want_path=True)[1]
    assert torch.equal(p1, p2)


@pytest.mark.parametrize('assets', [1, 3])
@pytest.mark.parametrize('sine', [False, True])
def test_return_vol_cond_exp(assets, sine):
    """both coordinate classes step-locally; the variance class without the periodic coefficient"""
    B, S = 63, 40
    hp = _hp(B, S, assets, sine, return_vol=True, v0=0.5, mean=0.4, speed=2.0, volatility=0.3, obs_perc=0.1)
    paths, obs, nb_obs, meta = data_utils.create_dataset('HestonWOFeller', hp, seed=4)
    assert paths.shape[1] == 2 * assets
    obs[1, :] = 0
    b = data_utils.collate_arrays(paths, obs, obs[:, 1:].sum(1), meta['dt'])
    delta_t, T = 0.37 * meta['dt'], meta['maturity']
    sm = stock_model.HestonWOFeller(**meta)
    c = schedule.cond_exp_clock(b['times'], delta_t, T)
    mean_of = lambda st: np.concatenate([np.zeros(assets), np.full(assets, hp['mean'])])
    y, _ = check_walk('return_vol assets {} sine {}'.format(assets, sine), b, delta_t, sm, c, [sm], mean_of, T=T)
    # the variance class spelled out: v e + mean (1 - e), e = exp(-speed step), whatever sine_coeff is
    jump = set(int(r) for r in c.row_of_jump)
    k = 0
    for r in range(1, len(y)):
        if r in jump:
            continue
        e = np.exp(-hp['speed'] * c.step_dt[k])
        want = y[r - 1][:, assets:] * e + hp['mean'] * (1 - e)
        assert (np.abs(y[r][:, assets:] - want) <= STEP_C * EPS * (np.abs(y[r - 1][:, assets:]) + hp['mean'])).all()
        k += 1
    assert torch.equal(dev_call(meta, b, delta_t, T, want_path=True)[1], torch.from_numpy(y).cuda())


@pytest.mark.parametrize('name', ['BlackScholes', 'OrnsteinUhlenbeck', 'Heston'])
def test_single_stage_gives_the_bits_of_the_single_model_call(name):
    B, dim = 257, 3
    hp = _hp(B, 50, dim, True, obs_perc=0.1)
    paths, obs, nb_obs, meta = data_utils.create_dataset(name, hp, seed=2)
    obs[1, :] = 0
    b = data_utils.collate_arrays(paths, obs, obs[:, 1:].sum(1), meta['dt'])
    delta_t, T = 0.37 * meta['dt'], meta['maturity']
    one = {'model_name': 'combined', 'stock_model_names': [name], 'hyperparam_dicts': [meta], 'dt': meta['dt'],
           'maturity': T, 'dimension': dim, 'nb_paths': B}
    pred = torch.randn(1 + schedule.cond_exp_clock(b['times'], delta_t, T).n_steps + len(b['times']), B, dim,
                       generator=torch.Generator().manual_seed(1)).cuda()
    old = dev_call(meta, b, delta_t, T, want_path=True, want_loss=True, pred=pred, weight=0.7)
    _lib.profile_enable(1)
    _lib.profile_read()
    try:
        new = dev_call(one, b, delta_t, T, want_path=True, want_loss=True, pred=pred, weight=0.7)
        assert list(_lib.profile_read()) == ['k_cond_exp_walk']
    finally:
        _lib.profile_enable(0)
    assert np.array_equal(old[0], new[0])
    for a, n in zip(old[1:], new[1:]):
        assert torch.equal(a, n)


# ---- goldens ----------------------------------------------------------------------------------------
def test_combined_golden_on_the_device():
    g = np.load(os.path.join(GOLDEN, 'g17_combined_condexp.npz'))
    meta = json.loads(str(g['meta_json']))
    b = {'times': g['times'], 'time_ptr': g['time_ptr'], 'X': torch.tensor(g['X']),
         'obs_idx': torch.tensor(g['obs_idx']), 'start_X': torch.tensor(g['start_X']),
         'n_obs_ot': torch.tensor(g['n_obs_ot'])}
    for w in (0.5, 0.8):
        path_t, path_y, loss, _ = dev_call(meta, b, float(g['delta_t']), float(g['T']), want_path=True,
                                           want_loss=True, weight=w)
        assert np.array_equal(path_t, g['path_t']) and len(path_t) == 69
        assert float(loss) == pytest.approx(float(g['loss_w{}'.format(w)]), rel=1e-9)
        np.testing.assert_allclose(path_y.cpu().numpy(), g['path_y'], rtol=8 * EPS * 69, atol=0)


# ---- end to end ---------------------------------------------------------------------------------------
def test_generate_combined_collate_cond_exp():
    names = ['BlackScholes', 'HestonWOFeller', 'OrnsteinUhlenbeck']
    hps = [_hp(300, 20, 2, True, obs_perc=0.1, v0=0.3) for _ in names]
    ds = DDS.generate_combined(names, hps, seed=11)
    idx = np.arange(300)[::-1][:257].copy()
    d = ds.collate(idx)
    dt = ds.metadata['dt']
    path_t, path_d, loss_d, _ = device_data.cond_exp(
        ds.metadata, d['times'], d['time_ptr'], d['X'], d['obs_idx'], dt, ds.metadata['maturity'], d['start_X'],
        n_obs_ot=d['n_obs_ot'], want_path=True, want_loss=True)
    paths, obs, nb_obs = ds.to_arrays()
    b = data_utils.collate_arrays(paths[idx], obs[idx], nb_obs[idx], dt)
    sm = stock_model.STOCK_MODELS['combined'](**ds.metadata)
    loss_h, path_t_h, path_h = host_walk(sm, b, dt)
    assert np.array_equal(path_t, path_t_h)
    assert float(loss_d) == pytest.approx(float(loss_h), rel=1e-12)
    np.testing.assert_allclose(path_d.cpu().numpy(), path_h, rtol=8 * EPS * 61, atol=0)


def _small_combined(n_paths):
    names = ['BlackScholes', 'OrnsteinUhlenbeck']
    hps = [dict(copy.deepcopy(data_utils.hyperparam_default), nb_paths=n_paths, nb_steps=50, maturity=0.5)
           for _ in names]
    return data_utils.create_combined_dataset(names, hps, seed=0)


def test_evaluate_device_on_a_combined_batch():
    paths, obs, nb_obs, meta = _small_combined(63)
    b = data_utils.collate_arrays(paths, obs, nb_obs, meta['dt'])
    d = to_dev(b)
    sm = stock_model.STOCK_MODELS[meta['model_name']](**meta)
    m = hip_model(demo_cfg()).eval()
    args = (d['times'], d['time_ptr'], d['X'], d['obs_idx'], meta['dt'], meta['maturity'], d['start_X'])
    msd_dev = m.evaluate_device(*args, meta)
    msd_host = m.evaluate(*args, d['n_obs_ot'], sm)
    assert float(msd_dev) == pytest.approx(float(msd_host), rel=1e-9)
    assert float(m.evaluate_device(*args, sm)) == float(msd_dev)


def test_train_on_a_combined_dataset():
    paths, obs, nb_obs, meta = _small_combined(200)
    kw = dict(epochs=2, batch_size=40, dropout_rate=0.1, evaluate=True, log=lambda s: None)
    m1, met1 = train.train((paths, obs, nb_obs), meta, **kw)
    m2, met2 = train.train((paths, obs, nb_obs), meta, device_eval=True, **kw)
    assert torch.equal(m1.flat_parameters(), m2.flat_parameters()) and len(met1) == len(met2) == 2
    for r1, r2 in zip(met1, met2):
        assert r1[0] == r2[0] and r1[3] == r2[3] and r1[4] == r2[4]
        assert np.isfinite(r1[5]) and r1[5] > 0
        assert r2[5] == pytest.approx(r1[5], rel=1e-9)
        assert r2[6] == pytest.approx(float(r1[6]), rel=1e-9)


# ---- C level --------------------------------------------------------------------------------------------
def test_c_level_refusals_of_the_staged_entry_points():
    L = _lib.lib()
    B, dim, n_obs, K, nt = 4, 2, 3, 10, 2
    dev = torch.device('cuda')
    start_X, X = torch.ones(B, dim, device=dev), torch.ones(n_obs, dim, device=dev)
    obs_idx = torch.tensor([0, 2, 1], dtype=torch.int32, device=dev)
    n_obs_ot = torch.tensor([1, 1, 1, 0], dtype=torch.int32, device=dev)
    pred = torch.zeros(1 + K + nt, B, dim, device=dev)
    out = torch.full(((1 + K + nt) * B * dim + 2,), -7.0, dtype=torch.float64, device=dev)
    step_dt, step_t = np.full(K, 0.1), np.arange(K) * 0.1
    k_jump, time_ptr = np.array([3, 7], dtype=np.int32), np.array([0, 2, 3], dtype=np.int32)
    need = ctypes.c_size_t(0)
    assert L.njode_cond_exp_staged_bytes(B, n_obs, nt, K, dim, 2, ctypes.byref(need)) == 0
    for bad in ((0, n_obs, nt, K, dim, 2), (B, -1, nt, K, dim, 2), (B, n_obs, nt, K, 0, 2), (B, n_obs, nt, K, dim, 0),
                (B, n_obs, nt, K, dim, _lib.MAX_STAGES + 1), (B, n_obs, nt, -1, dim, 1)):
        assert L.njode_cond_exp_staged_bytes(*bad, ctypes.byref(need)) == _lib.E_BADARG, bad
    assert L.njode_cond_exp_staged_bytes(B, n_obs, nt, K, dim, 2, None) == _lib.E_BADARG
    assert L.njode_cond_exp_staged_bytes(B, n_obs, nt, K, dim, 2, ctypes.byref(need)) == 0
    ws = torch.full((need.value,), 0xA5, dtype=torch.uint8, device=dev)
    p = lambda a: a.ctypes.data
    o = out.data_ptr()
    outs3 = (o, o + 8 * (out.numel() - 2), o + 8 * (out.numel() - 1))

    def call(models=(0, 1), firsts=(0, 5), rv=(0, 0), dims=None, n_stages=None, null=(), sched_kw=None,
             batch_kw=None, outs=outs3, ws_bytes=None):
        stages = (_lib.NjodeSdeStage * max(len(models), 1))()
        for i, m in enumerate(models):
            stages[i].sde = _lib.NjodeSde(model=m, dim=(dims or [dim] * len(models))[i], drift=2.0, mean=4.0, speed=2.0)
            stages[i].return_vol, stages[i].first_step, stages[i].v0 = rv[i], firsts[i], 1.0
        bk = dict(batch_size=B, n_obs=n_obs, start_X=start_X.data_ptr(), X=X.data_ptr(), M=None,
                  obs_idx=obs_idx.data_ptr(), n_obs_ot=n_obs_ot.data_ptr())
        bk.update(batch_kw or {})
        sk = dict(n_steps=K, n_times=nt, step_dt=p(step_dt), step_t=p(step_t), k_jump=p(k_jump), time_ptr=p(time_ptr))
        sk.update(sched_kw or {})
        batch, sched = _lib.NjodeBatch(**bk), _lib.NjodeCondExpSchedule(**sk)
        return L.njode_cond_exp_staged_f64(
            None if 'stages' in null else stages, len(models) if n_stages is None else n_stages,
            None if 'batch' in null else ctypes.byref(batch), None if 'sched' in null else ctypes.byref(sched),
            0.5, pred.data_ptr(), outs[0], outs[1], outs[2], ws.data_ptr(),
            need.value if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)

    refusals = {
        'null stages': dict(null=('stages',)), 'null batch': dict(null=('batch',)), 'null sched': dict(null=('sched',)),
        'no stage': dict(n_stages=0), 'negative stages': dict(n_stages=-1), 'too many stages': dict(n_stages=17),
        'first stage not at 0': dict(firsts=(1, 5)), 'offsets not increasing': dict(firsts=(0, 0)),
        'offsets decreasing': dict(models=(0, 1, 0), firsts=(0, 6, 5), rv=(0, 0, 0)),
        'negative offset': dict(firsts=(-1, 5)), 'offset beyond the clock': dict(firsts=(0, K + 1)),
        'unknown model': dict(models=(0, 4)), 'negative model': dict(models=(-1, 1)),
        'return_vol in two stages': dict(models=(0, 3), rv=(0, 1)),
        'return_vol of another model': dict(models=(2,), firsts=(0,), rv=(1,)),
        'stages of different width': dict(dims=[dim, dim + 1]),
        'B = 0': dict(batch_kw=dict(batch_size=0)), 'K < 0': dict(sched_kw=dict(n_steps=-1)),
        'no output': dict(outs=(None, None, None)), 'mask': dict(batch_kw=dict(M=X.data_ptr())),
        'null X': dict(batch_kw=dict(X=None)), 'null step_t': dict(sched_kw=dict(step_t=None)),
        'k_jump beyond the steps': dict(sched_kw=dict(n_steps=5), firsts=(0, 4)),
    }
    gen_out = torch.full((8 * 2 * 5,), -7.0, dtype=torch.float64, device=dev)

    def gen(model=3, N=5, gdim=2, S_i=3, s0=0, total=7, rv=0, rho=0.5, null=False, v_null=False):
        st = _lib.NjodeSdeStage()
        st.sde = _lib.NjodeSde(model=model, n_paths=N, dim=gdim, n_steps=S_i, drift=2.0, volatility=0.3, mean=4.0,
                               speed=2.0, correlation=rho, S0=1.0, maturity=0.1)
        st.return_vol, st.first_step, st.v0 = rv, s0, 1.0
        return L.njode_generate_stage(None if null else ctypes.byref(st), total, ctypes.c_uint64(1), None,
                                      None if v_null else gen_out.data_ptr(), _stream())

    gen_refusals = {
        'null stage': dict(null=True), 'null paths': dict(v_null=True), 'N = 0': dict(N=0), 'dim = 0': dict(gdim=0),
        'no steps': dict(S_i=0), 'negative offset': dict(s0=-1), 'stage beyond the grid': dict(s0=5),
        'stage longer than the grid': dict(S_i=8), 'unknown model': dict(model=4), 'negative model': dict(model=-1),
        'correlation': dict(rho=1.5), 'return_vol of another model': dict(model=2, rv=1),
        'return_vol off the start': dict(rv=1, s0=1, gdim=1),
    }
    torch.cuda.synchronize()
    _lib.profile_enable(1)
    _lib.profile_read()
    try:
        for what, kw in refusals.items():
            assert call(**kw) == _lib.E_BADARG, what
            assert L.njode_last_error(), what
        # return_vol with an odd width
        s1 = torch.ones(B, 3, device=dev)
        assert call(models=(3,), firsts=(0,), rv=(1,), dims=[3], batch_kw=dict(start_X=s1.data_ptr())) == _lib.E_BADARG
        assert call(ws_bytes=need.value - 1) == _lib.E_WORKSPACE
        for what, kw in gen_refusals.items():
            assert gen(**kw) == _lib.E_BADARG, what
            assert L.njode_last_error(), what
        torch.cuda.synchronize()
        assert _lib.profile_read() == {}                      # nothing was launched ...
        assert bool((out == -7.0).all()) and bool((gen_out == -7.0).all())   # ... nothing written
        assert bool((ws == 0xA5).all())
        assert call() == 0 and gen() == 0 and gen(rv=1, gdim=1, total=7, S_i=7) == 0
        torch.cuda.synchronize()
        assert list(_lib.profile_read()) == ['k_cond_exp_walk']
    finally:
        _lib.profile_enable(0)
    assert bool((out != -7.0).all())
    # BlackScholes for steps 0..4, OrnsteinUhlenbeck from step 5 on
    bs = stock_model.BlackScholes(drift=2.0, volatility=0.3, nb_paths=B, nb_steps=10, S0=1, maturity=1.0)
    ou = stock_model.OrnsteinUhlenbeck(volatility=0.3, nb_paths=B, nb_steps=10, S0=1, mean=4.0, speed=2.0, maturity=1.0)
    want = np.ones((B, dim))
    rows, k, i = [want], 0, 0
    for r in range(1, 1 + K + nt):
        if i < nt and k == k_jump[i]:
            i += 1
            want = want.copy()
            want[obs_idx.cpu().numpy()[time_ptr[i - 1]:time_ptr[i]]] = 1.0
        else:
            want = (bs if k < 5 else ou).next_cond_exp(want, step_dt[k], step_t[k])
            k += 1
        rows.append(want)
    np.testing.assert_allclose(out[:-2].cpu().numpy().reshape(1 + K + nt, B, dim), np.array(rows), rtol=1e-13)


@pytest.mark.parametrize('N,dim', [(1, 1), (37, 3), (65, 2)])
def test_staged_entry_points_stay_inside_their_buffers(N, dim):
    """arenas of exactly the stated sizes, no guard byte changed, the wrapper's bits (in the manner of
    tests/test_hip_buffer_bounds.py)"""
    L = _lib.lib()
    names, steps, seed = ['OrnsteinUhlenbeck', 'HestonWOFeller', 'BlackScholes'], (7, 1, 4), 5 + N
    S = sum(steps)
    hps = [_hp(N, s, dim, True, dt=2.0 ** -6, obs_perc=0.4, v0=0.3) for s in steps]
    ds = DDS.generate_combined(names, hps, seed=seed)
    vol_hp = _hp(N, 7, dim, True, return_vol=True, v0=0.3, obs_perc=0.4)
    vol = DDS.generate('HestonWOFeller', vol_hp, seed=seed)
    errors = []

    def finish(what, phase, rc, A, outputs):
        trips = A.check()
        if rc or trips:
            errors.append('{} phase {}: rc {} guards {}'.format(what, phase, rc, trips))
        for name, ref in outputs.items():
            if not torch.equal(A.view(name, ref.dtype).view(torch.uint8), ref.contiguous().reshape(-1).view(torch.uint8)):
                errors.append('{} phase {}: {} differs from the wrapper call'.format(what, phase, name))

    cases = [('combined', ds, ds.metadata, dim), ('return_vol', vol, vol.metadata, 2 * dim)]
    for phase in (0, 1):
        A = Arena('cuda', phase).add('paths', 8 * (S + 1) * dim * N).add('vol', 8 * 8 * 2 * dim * N).build()
        s0 = 0
        for name, hp in zip(names, hps):
            st = device_data.stage_struct(name, hp, dim, first_step=s0)
            rc = L.njode_generate_stage(ctypes.byref(st), S, ctypes.c_uint64(seed), None, ctypes.c_void_p(A.ptr('paths')),
                                        _stream())
            s0 += hp['nb_steps']
            finish('generate_stage ' + name, phase, rc, A, {} if s0 < S else {'paths': ds.paths_tm})
        st = device_data.stage_struct('HestonWOFeller', vol_hp, dim)
        rc = L.njode_generate_stage(ctypes.byref(st), 7, ctypes.c_uint64(seed), None, ctypes.c_void_p(A.ptr('vol')), _stream())
        finish('generate_stage return_vol', phase, rc, A, {'vol': vol.paths_tm})
        for tag, dset, meta, width in cases:
            b = dset.collate(None)
            n_obs = int(b['time_ptr'][-1])
            if not n_obs:
                continue
            stages, mats = device_data._stages_of(meta, width)
            dt = meta['dt']
            clock = schedule.cond_exp_clock(b['times'], 0.37 * dt, meta['maturity'], mats)
            K, nt = clock.n_steps, clock.n_times
            n_t = 1 + K + nt
            pred = torch.randn((n_t, N, width), generator=torch.Generator().manual_seed(N)).cuda()
            _, path_y, opt_loss, sq_diff = device_data.cond_exp(
                meta, b['times'], b['time_ptr'], b['X'], b['obs_idx'], 0.37 * dt, meta['maturity'], b['start_X'],
                b['n_obs_ot'], pred=pred, want_path=True, want_loss=True)
            need = ctypes.c_size_t(0)
            _lib.check(L.njode_cond_exp_staged_bytes(N, n_obs, nt, K, width, len(stages), ctypes.byref(need)))
            A = Arena('cuda', phase)
            A.add('start_X', 4 * N * width, 'nan32').add('X', 4 * n_obs * width, 'nan32')
            A.add('obs_idx', 4 * n_obs, 'index', modulo=min(N, 3)).add('n_obs_ot', 4 * N, 'index', base=1)
            A.add('pred', 4 * n_t * N * width, 'nan32').add('path_y', 8 * n_t * N * width).add('opt_loss', 8)
            A.add('sq_diff', 8).add('ws', need.value).build()
            A.put('start_X', b['start_X']), A.put('X', b['X']), A.put('obs_idx', b['obs_idx'])
            A.put('n_obs_ot', b['n_obs_ot']), A.put('pred', pred)
            host = [np.ascontiguousarray(clock.step_dt), np.ascontiguousarray(clock.step_t),
                    np.ascontiguousarray(clock.k_jump, dtype=np.int32), np.ascontiguousarray(b['time_ptr'], dtype=np.int32)]
            sched = _lib.NjodeCondExpSchedule(K, nt, *[h.ctypes.data for h in host])
            cs = (_lib.NjodeSdeStage * len(stages))(*stages)
            for stg, first in zip(cs, clock.stage_first):
                stg.first_step = int(first)
            cb = _lib.NjodeBatch(N, n_obs, A.ptr('start_X'), A.ptr('X'), None, A.ptr('obs_idx'), A.ptr('n_obs_ot'),
                                 float(N), 0, None)
            rc = L.njode_cond_exp_staged_f64(cs, len(stages), ctypes.byref(cb), ctypes.byref(sched), 0.5,
                                             ctypes.c_void_p(A.ptr('pred')), ctypes.c_void_p(A.ptr('path_y')),
                                             ctypes.c_void_p(A.ptr('opt_loss')), ctypes.c_void_p(A.ptr('sq_diff')),
                                             ctypes.c_void_p(A.ptr('ws')), need.value, _stream())
            finish('cond_exp_staged ' + tag, phase, rc, A,
                   {'path_y': path_y, 'opt_loss': opt_loss.reshape(1).clone(), 'sq_diff': sq_diff.reshape(1).clone()})
            del host
    assert not errors, '\n'.join(errors)
