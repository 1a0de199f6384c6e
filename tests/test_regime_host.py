"""Host side of the regime-switch and Heston-without-Feller datasets: ``stock_model.HestonWOFeller``
and ``Combined``, ``data_utils.create_combined_dataset``, the staged ``schedule.cond_exp_clock`` and
what ``device_data.cond_exp`` refuses before it touches the library.

Standards: the generators and the conditional-expectation walk are the reference's float64 numpy
arithmetic, so they are held to the reference's goldens (``tests/golden/make_golden_regime.py``)
**bit for bit** -- the vectorised ``np.exp`` / ``np.log`` / ``np.sqrt`` of ``HestonWOFeller``
reproduce the reference's per-path calls to the bit on this numpy, so no step-local allowance is
needed on the host.  The reference's ``Combined.compute_cond_exp`` only runs when path 0 is
observed at every stage's last grid point (its tail loop raises ``TypeError`` otherwise); batches
without such an observation are held to a hand concatenation of per-stage
``compute_cond_exp(start_time=...)`` calls of the single-model classes.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

from njode_amd import _lib, data_utils, device_data, schedule, stock_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
HWF = np.load(os.path.join(GOLDEN, 'g17_hwf_paths.npz'))
DATA = np.load(os.path.join(GOLDEN, 'g17_combined_data.npz'))
CE = np.load(os.path.join(GOLDEN, 'g17_combined_condexp.npz'))


def _json(z, key):
    return json.loads(str(z[key]))


# ---- HestonWOFeller -----------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['d1', 'd3_vol_v0', 'd1_no_feller_vol', 'd3_sine_no_feller'])
def test_heston_wo_feller_paths_bit_for_bit(tag):
    hp = _json(HWF, tag + '/hp_json')
    np.random.seed(int(HWF['seed']))
    sm = stock_model.STOCK_MODELS['HestonWOFeller'](**hp)
    paths, dt = sm.generate_paths()
    want = HWF[tag + '/paths']
    d = hp['dimension']
    assert paths.shape == want.shape == (hp['nb_paths'], d * (2 if hp['return_vol'] else 1), hp['nb_steps'] + 1)
    assert dt == float(HWF[tag + '/dt'])
    assert np.array_equal(paths, want)
    if hp['return_vol']:
        assert np.all(paths[:, d:, 0] == (hp['v0'] if hp['v0'] is not None else hp['mean']))
    if tag == 'd1_no_feller_vol':
        assert (paths[:, d:, :] < 0).any()           # the clamp at 0 was exercised
    if tag == 'd1':
        assert sm.v0 == hp['mean']                   # v0 defaults to mean


def test_heston_wo_feller_scheme_start_and_cond_exp():
    hp = dict(_json(HWF, 'd3_vol_v0/hp_json'), sine_coeff=3.0)
    with pytest.raises(ValueError, match='unknown sampling scheme'):
        stock_model.HestonWOFeller(**dict(hp, scheme='milstein')).generate_paths()
    sm = stock_model.HestonWOFeller(**hp)
    np.random.seed(1)
    paths, _ = sm.generate_paths(start_X=np.full((hp['nb_paths'], 3), 2.5))
    assert np.all(paths[:, :3, 0] == 2.5) and np.all(paths[:, 3:, 0] == 0.5)
    y = np.random.RandomState(0).rand(4, 6) + 0.5
    out = sm.next_cond_exp(y, 0.01, 0.3)
    pc = 1 + np.sin(3.0 * 0.3)
    e = np.exp(-hp['speed'] * 0.01)                  # no periodic coefficient on the variance
    assert np.array_equal(out[:, :3], y[:, :3] * np.exp(hp['drift'] * pc * 0.01))
    assert np.array_equal(out[:, 3:], y[:, 3:] * e + hp['mean'] * (1 - e))
    flat = stock_model.HestonWOFeller(**dict(hp, return_vol=False))
    assert np.array_equal(flat.next_cond_exp(y, 0.01, 0.3), y * np.exp(hp['drift'] * pc * 0.01))


# ---- create_combined_dataset ---------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['bs_ou', 'bs_ou_hwf'])
def test_create_combined_dataset_bit_for_bit(tag, tmp_path):
    names, hps = _json(DATA, tag + '/names_json'), _json(DATA, tag + '/hps_json')
    before = copy.deepcopy(hps)
    paths, obs, nb_obs, meta = data_utils.create_combined_dataset(names, hps, seed=int(DATA['seed']))
    assert hps == before                                        # the caller's dicts are left alone
    assert np.array_equal(paths, DATA[tag + '/paths'])
    assert np.array_equal(obs, DATA[tag + '/obs']) and np.array_equal(nb_obs, DATA[tag + '/nb_obs'])
    want = _json(DATA, tag + '/meta_json')
    assert set(meta) == set(want) == {'dt', 'maturity', 'dimension', 'nb_paths', 'model_name',
                                      'stock_model_names', 'hyperparam_dicts'}
    assert json.loads(json.dumps(meta, sort_keys=True)) == want
    assert meta['model_name'] == 'combined' and paths.shape[2] == sum(h['nb_steps'] for h in hps) + 1
    data_utils.save_dataset(str(tmp_path / 'ds'), paths, obs, nb_obs, meta)
    p2, o2, n2, m2 = data_utils.load_dataset_dir(str(tmp_path / 'ds'))
    assert np.array_equal(p2, paths) and np.array_equal(o2, obs) and np.array_equal(n2, nb_obs)
    assert m2 == want
    assert isinstance(stock_model.STOCK_MODELS[m2['model_name']](**m2), stock_model.Combined)


def test_create_combined_dataset_asserts_agreement():
    names, hps = _json(DATA, 'bs_ou/names_json'), _json(DATA, 'bs_ou/hps_json')
    for key, val in (('dimension', 2), ('nb_paths', 8), ('nb_steps', 10)):
        bad = copy.deepcopy(hps)
        bad[1][key] = val
        with pytest.raises(AssertionError):
            data_utils.create_combined_dataset(names, bad, seed=0)


# ---- Combined.compute_cond_exp -------------------------------------------------------------------
def _ce_batch():
    return dict(times=CE['times'], time_ptr=CE['time_ptr'], X=CE['X'].astype(np.float64),
                obs_idx=CE['obs_idx'], start_X=CE['start_X'].astype(np.float64), n_obs_ot=CE['n_obs_ot'])


def _walk(sm, b, delta_t, **kw):
    return sm.compute_cond_exp(b['times'], b['time_ptr'], b['X'], b['obs_idx'], delta_t, None, b['start_X'],
                               b['n_obs_ot'], **kw)


def test_combined_cond_exp_against_the_reference():
    meta = _json(CE, 'meta_json')
    sm = stock_model.STOCK_MODELS['combined'](**meta)
    b, delta_t = _ce_batch(), float(CE['delta_t'])
    for w in (0.5, 0.8):
        loss, path_t, path_y = _walk(sm, b, delta_t, return_path=True, get_loss=True, weight=w)
        assert loss == pytest.approx(float(CE['loss_w{}'.format(w)]), rel=1e-12)
        assert np.array_equal(path_t, CE['path_t']) and np.array_equal(path_y, CE['path_y'])
        assert len(path_t) == 69
        opt = sm.get_optimal_loss(b['times'], b['time_ptr'], b['X'], b['obs_idx'], delta_t, None,
                                  b['start_X'], b['n_obs_ot'], weight=w)
        assert opt == loss
    assert _walk(sm, b, delta_t, return_path=False, get_loss=True) == pytest.approx(float(CE['loss_w0.5']), rel=1e-12)


def hand_concatenation(names, hps, b, delta_t, weight=0.5):
    """per-stage compute_cond_exp(start_time=...) calls of the single-model classes, chained"""
    T, loss, pt, py = 0, 0, None, None
    for i, (n, hp) in enumerate(zip(names, hps)):
        T = T + hp['maturity']
        sm = stock_model.STOCK_MODELS[n](**hp)
        l, t, y = sm.compute_cond_exp(b['times'], b['time_ptr'], b['X'], b['obs_idx'], delta_t, T,
                                      b['start_X'] if i == 0 else py[-1], b['n_obs_ot'], return_path=True,
                                      get_loss=True, weight=weight, start_time=None if i == 0 else pt[-1])
        loss = loss + l
        pt, py = (t, y) if i == 0 else (np.concatenate([pt, t]), np.concatenate([py, y], axis=0))
    return loss, pt, py


def regime_batch(names, hps, seed, drop=()):
    """host batch of a combined dataset without the observations at the grid indices ``drop``"""
    paths, obs, nb_obs, meta = data_utils.create_combined_dataset(names, hps, seed=seed)
    obs = obs.copy()
    obs[:, list(drop)] = 0
    nb_obs = obs[:, 1:].sum(axis=1)
    b = data_utils.collate_arrays(paths, obs, nb_obs, meta['dt'])
    return dict(times=b['times'], time_ptr=b['time_ptr'], X=b['X'].numpy().astype(np.float64),
                obs_idx=b['obs_idx'].numpy(), start_X=b['start_X'].numpy().astype(np.float64),
                n_obs_ot=b['n_obs_ot'].numpy()), meta


CLOCK_CASES = {
    # name: (grid indices without observations, delta_t / dt)
    'boundary observed': ((), 1.0),
    'no boundary observation, partial steps': ((8, 16, 24), 0.37),
    'a stage without any observation': (tuple(range(9, 17)), 1.0),
    'boundary observed, partial steps': ((), 0.37),
    'nothing observed': (tuple(range(0, 25)), 0.7),
}


@pytest.mark.parametrize('case', sorted(CLOCK_CASES))
def test_staged_clock_and_host_walk(case):
    """the staged clock against Combined's path_t entry for entry; Combined against the hand
    concatenation (paths bit for bit: it is the same arithmetic)"""
    drop, ratio = CLOCK_CASES[case]
    names = ['BlackScholes', 'OrnsteinUhlenbeck', 'HestonWOFeller']
    hps = _json(DATA, 'bs_ou_hwf/hps_json')
    for hp in hps:
        hp.update(nb_paths=9, obs_perc=0.4, sine_coeff=2 * np.pi)
    b, meta = regime_batch(names, hps, 2, drop)
    delta_t = ratio * meta['dt']
    mats = [hp['maturity'] for hp in hps]
    if case == 'boundary observed':
        for k in (8, 16, 24):
            assert np.any(np.isclose(b['times'], k * meta['dt'], atol=1e-12))
    sm = stock_model.Combined(**meta)
    loss, path_t, path_y = _walk(sm, b, delta_t, return_path=True, get_loss=True)
    loss_h, pt_h, py_h = hand_concatenation(names, hps, b, delta_t)
    assert np.array_equal(path_t, pt_h) and np.array_equal(path_y, py_h) and loss == loss_h
    c = schedule.cond_exp_clock(b['times'], delta_t, 0.0, mats)
    assert np.array_equal(c.path_t, path_t)
    assert c.n_steps + c.n_times + 1 == len(path_t) and c.n_times == len(b['times'])
    assert list(c.stage_first[:1]) == [0] and np.all(np.diff(c.stage_first) > 0) and len(c.stage_first) == 3
    # the clock before the first step of a stage is where the previous stage ended
    T = 0
    for i in range(1, 3):
        T = T + mats[i - 1]
        assert abs(c.step_t[c.stage_first[i]] - T) <= 1e-10
    if 'partial' in case:
        ends = c.step_t[c.stage_first[1:] - 1] + c.step_dt[c.stage_first[1:] - 1]
        assert np.any(c.step_dt[c.stage_first[1:] - 1] < delta_t * (1 - 1e-9)) and np.allclose(ends, np.cumsum(mats)[:2])
    # every factor of the walk can be recomputed from the clock: stage of step k by its first index
    y, k, jump = b['start_X'], 0, set(int(r) for r in c.row_of_jump)
    for r in range(1, len(path_t)):
        if r in jump:
            continue
        stage = int(np.searchsorted(c.stage_first, k, side='right')) - 1
        one = stock_model.STOCK_MODELS[names[stage]](**hps[stage])
        assert np.array_equal(one.next_cond_exp(path_y[r - 1], c.step_dt[k], c.step_t[k]), path_y[r]), (r, k, stage)
        k += 1
    assert k == c.n_steps


def test_single_walk_clock_is_unchanged():
    times = np.array([0.1, 0.25, 0.7])
    c = schedule.cond_exp_clock(times, 0.03, 1.0)
    s = schedule.cond_exp_clock(times, 0.03, 123.0, [1.0])
    assert list(c.stage_first) == [0] == list(s.stage_first)
    for f in ('step_dt', 'step_t', 'k_jump', 'path_t', 'row_of_jump'):
        assert np.array_equal(getattr(c, f), getattr(s, f)), f
    for bad in ([], [0.5, -0.5], [0.5, float('nan')]):
        with pytest.raises(ValueError):
            schedule.cond_exp_clock(times, 0.03, 1.0, bad)
    with pytest.raises(ValueError):                           # beyond the accumulated T
        schedule.cond_exp_clock(times, 0.03, 1.0, [0.3, 0.3])


# ---- device_data: what is refused before the library is touched -------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError('the library was touched before the refusal')
    monkeypatch.setattr(_lib, 'lib', boom)


def _dev_args(d=1, B=3):
    return (np.array([0.1, 0.2]), np.array([0, 2, 3]), torch.ones(3, d), torch.tensor([0, 2, 1]), 0.01, 1.0,
            torch.ones(B, d))


def _combined_meta(d=1, **stage1):
    hp = dict(data_utils.hyperparam_default, nb_paths=3, nb_steps=50, maturity=0.5, dimension=d,
              S0=[1.] * d if d > 1 else 1)
    return {'model_name': 'combined', 'stock_model_names': ['BlackScholes', 'HestonWOFeller'],
            'hyperparam_dicts': [dict(hp), dict(hp, **stage1)], 'dt': 0.01, 'maturity': 1.0, 'dimension': d,
            'nb_paths': 3}


@pytest.mark.parametrize('what', ['start_time', 'return_vol stage', 'return_vol width', 'hwf lifted',
                                  'combined width', 'unknown stage', 'no stages', 'too many stages',
                                  'beyond the accumulated T'])
def test_refusals_before_the_library(what, no_library):
    args, kw, sm = _dev_args(), dict(want_path=True), _combined_meta()
    hwf = dict(data_utils.hyperparam_default, model_name='HestonWOFeller', nb_paths=3)
    if what == 'start_time':
        kw['start_time'] = 0.05
    elif what == 'return_vol stage':
        sm = _combined_meta(return_vol=True)
    elif what == 'return_vol width':                 # return_vol stores 2 d coordinates, not d
        sm = dict(hwf, return_vol=True)
    elif what == 'hwf lifted':
        sm, args = stock_model.HestonWOFeller(**hwf), _dev_args(d=2)
    elif what == 'combined width':
        args = _dev_args(d=2)
    elif what == 'unknown stage':
        sm['stock_model_names'][1] = 'FractionalBM'
    elif what == 'no stages':
        sm = dict(sm, stock_model_names=[], hyperparam_dicts=[])
    elif what == 'too many stages':
        sm = dict(sm, stock_model_names=['BlackScholes'] * 17, hyperparam_dicts=sm['hyperparam_dicts'][:1] * 17)
    elif what == 'beyond the accumulated T':         # the T argument is not what bounds a combined walk
        args = (np.array([0.1, 1.2]),) + _dev_args()[1:5] + (2.0,) + _dev_args()[6:]
    with pytest.raises(ValueError):
        device_data.cond_exp(sm, *args, **kw)


@pytest.mark.parametrize('sm,d', [
    (_combined_meta(), 1), (_combined_meta(d=3), 3), (stock_model.Combined(**_combined_meta()), 1),
    (dict(data_utils.hyperparam_default, model_name='HestonWOFeller'), 1),
    (dict(data_utils.hyperparam_default, model_name='HestonWOFeller', return_vol=True), 2),
    (stock_model.HestonWOFeller(**dict(data_utils.hyperparam_default, S0=[1., 1.], return_vol=True)), 4)])
def test_valid_descriptions_reach_the_device_check(sm, d, no_library):
    with pytest.raises(RuntimeError, match='GPU only'):
        device_data.cond_exp(sm, *_dev_args(d=d), want_path=True)


def test_stage_structs_and_exports():
    hp = dict(data_utils.hyperparam_default, S0=[1., 1.], return_vol=True, v0=0.25, sine_coeff=2.0)
    a = device_data._stages_of(stock_model.HestonWOFeller(**hp), 4)[0][0]
    b = device_data._stages_of(dict(hp, model_name='HestonWOFeller'), 4)[0][0]
    for st in (a, b):
        assert (st.sde.model, st.sde.dim, st.return_vol, st.v0, st.sde.has_sine) == (3, 4, 1, 0.25, 1)
        assert (st.sde.drift, st.sde.mean, st.sde.speed, st.sde.sine_coeff) == (2.0, 4.0, 2.0, 2.0)
    assert device_data.stage_struct('HestonWOFeller', dict(hp, v0=None), 2).v0 == 4.0     # v0 defaults to mean
    assert device_data._stages_of(stock_model.BlackScholes(**hp), 2) is None            # the old entry point
    stages, mats = device_data._stages_of(_combined_meta(), 1)
    assert [s.sde.model for s in stages] == [0, 3] and mats == [0.5, 0.5]
    assert 'HestonWOFeller' not in _lib.SDE_MODELS and _lib.SDE_MODELS_STAGED['HestonWOFeller'] == 3
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'njode_producer.h')).read()
    new = {'njode_generate_stage', 'njode_cond_exp_staged_bytes', 'njode_cond_exp_staged_f64'}
    assert new <= set(_lib.EXPORTS)
    for sym in new:
        assert 'int {}('.format(sym) in header
    assert 'NJODE_SDE_HESTON_WO_FELLER 3' in header and 'NJODE_MAX_STAGES {}'.format(_lib.MAX_STAGES) in header
    assert [f for f, _ in _lib.NjodeSdeStage._fields_] == ['sde', 'v0', 'return_vol', 'first_step']
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        for sym in new:
            assert hasattr(L, sym), sym
