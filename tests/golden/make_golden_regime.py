"""
Generate the regime-switch / Heston-without-Feller golden vectors under tests/golden/ by running
the REFERENCE itself (beside make_golden.py; needs the reference checkout, which never travels to
the GPU machine).  The committed ``g17_*.npz`` hold data only: hyper-parameters, seeds, masks and
the reference's outputs.  Usage:  python tests/golden/make_golden_regime.py

  g17_hwf_paths       HestonWOFeller.generate_paths (stock_model.py:288-335) under
                      np.random.seed: dim 1 / 3, return_vol on / off, v0 given, a parameter set
                      that violates the Feller condition (the clamp at 0 is exercised), sine
  g17_combined_data   create_combined_dataset (data_utils.py:111-195), run as it is in a scratch
                      directory and read back from the files it writes: BlackScholes ->
                      OrnsteinUhlenbeck, and BlackScholes -> OrnsteinUhlenbeck -> HestonWOFeller
  g17_combined_condexp  Combined.compute_cond_exp / get_optimal_loss (stock_model.py:421-466) on
                      the three-stage dataset, N = 5, 8 steps per stage, delta_t = dt / 2.  The
                      reference's tail loop raises TypeError (stock_model.py:139) whenever a
                      stage's last observation lies before the stage's end, so the mask forces
                      path 0 to be observed at every stage's last grid point.
"""
import contextlib
import copy
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('NJODE_REFERENCE') or os.path.join(os.path.dirname(REPO), 'reference')
sys.path.insert(0, REFERENCE)

with contextlib.redirect_stdout(io.StringIO()):
    import NJODE.data_utils as ref_data
    import NJODE.stock_model as ref_stock


def _hp(**kw):
    hp = copy.deepcopy(ref_data.hyperparam_default)
    hp.update(kw)
    return hp


HWF_CASES = {
    'd1': _hp(nb_paths=6, nb_steps=12, v0=None),
    'd3_vol_v0': _hp(nb_paths=6, nb_steps=12, S0=[1., 1., 1.], dimension=3, return_vol=True, v0=0.5),
    'd1_no_feller_vol': _hp(nb_paths=6, nb_steps=40, volatility=2.5, mean=0.05, speed=0.5, v0=0.02,
                            return_vol=True),
    'd3_sine_no_feller': _hp(nb_paths=6, nb_steps=40, S0=[1., 1., 1.], dimension=3, volatility=2.5,
                             mean=0.05, speed=0.5, v0=0.02, sine_coeff=2 * np.pi, correlation=-0.7),
}
HWF_SEED = 3


def make_hwf():
    out = {}
    for tag, hp in HWF_CASES.items():
        np.random.seed(HWF_SEED)
        paths, dt = ref_stock.HestonWOFeller(**hp).generate_paths()
        out[tag + '/paths'] = paths
        out[tag + '/dt'] = np.float64(dt)
        out[tag + '/hp_json'] = np.array(json.dumps(hp))
        if 'no_feller' in tag:      # the clamp must have been exercised
            v = paths[:, hp['dimension']:, :] if hp['return_vol'] else None
            assert 2 * hp['speed'] * hp['mean'] < hp['volatility'] ** 2
            assert v is None or (v < 0).any(), tag
    out['seed'] = np.int64(HWF_SEED)
    np.savez_compressed(os.path.join(HERE, 'g17_hwf_paths.npz'), **out)


def _stage_hps(names, nb_paths, nb_steps, maturity):
    hps = []
    for n in names:
        hp = _hp(nb_paths=nb_paths, nb_steps=nb_steps, maturity=maturity, obs_perc=0.3)
        if n == 'HestonWOFeller':
            hp.update(volatility=1.5, mean=0.05, speed=1.0, v0=0.04, drift=1.0)
        if n == 'OrnsteinUhlenbeck':
            hp.update(mean=1.5, speed=1.0)
        hps.append(hp)
    return hps


def ref_combined(names, hps, seed):
    """the reference's create_combined_dataset, run as it is (it writes ../data/ relative to the
    working directory) and read back"""
    hps = copy.deepcopy(hps)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'run'))
        os.chdir(os.path.join(tmp, 'run'))
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                path, _ = ref_data.create_combined_dataset(list(names), hps, seed=seed)
            with open(os.path.join(path, 'data.npy'), 'rb') as f:
                paths, obs, nb_obs = np.load(f), np.load(f), np.load(f)
            with open(os.path.join(path, 'metadata.txt')) as f:
                meta = json.load(f)
        finally:
            os.chdir(cwd)
    return paths, obs, nb_obs, meta


COMBINED = {
    'bs_ou': (('BlackScholes', 'OrnsteinUhlenbeck'), 7, 9, 0.09),
    'bs_ou_hwf': (('BlackScholes', 'OrnsteinUhlenbeck', 'HestonWOFeller'), 5, 8, 0.08),
}
COMBINED_SEED = 5


def make_combined_data():
    out = {'seed': np.int64(COMBINED_SEED)}
    for tag, (names, n, s, mat) in COMBINED.items():
        hps = _stage_hps(names, n, s, mat)
        paths, obs, nb_obs, meta = ref_combined(names, hps, COMBINED_SEED)
        out[tag + '/paths'], out[tag + '/obs'], out[tag + '/nb_obs'] = paths, obs, nb_obs
        out[tag + '/names_json'] = np.array(json.dumps(list(names)))
        out[tag + '/hps_json'] = np.array(json.dumps(hps))
        out[tag + '/meta_json'] = np.array(json.dumps(meta, sort_keys=True))
    np.savez_compressed(os.path.join(HERE, 'g17_combined_data.npz'), **out)
    return out


def make_combined_condexp(data):
    tag = 'bs_ou_hwf'
    names, n, s, mat = COMBINED[tag]
    paths, meta = data[tag + '/paths'], json.loads(str(data[tag + '/meta_json']))
    obs = data[tag + '/obs'].copy()
    obs[0, [s, 2 * s, 3 * s]] = 1          # path 0 sees every stage's last grid point
    nb_obs = np.sum(obs[:, 1:], axis=1)
    items = [{'idx': [i], 'stock_path': paths[[i]], 'observed_dates': obs[[i]],
              'nb_obs': nb_obs[[i]], 'dt': meta['dt']} for i in range(n)]
    b = ref_data.custom_collate_fn(items)
    # float64 copies of the batch's fp32 arrays: what the device widens exactly
    X = b['X'].numpy().astype(np.float64)
    start_X = b['start_X'].numpy().astype(np.float64)
    obs_idx, n_obs_ot = b['obs_idx'].numpy(), b['n_obs_ot'].numpy()
    delta_t = meta['dt'] / 2
    sm = ref_stock.STOCK_MODELS['combined'](**meta)
    out = {'times': b['times'], 'time_ptr': np.asarray(b['time_ptr']), 'X': b['X'].numpy(),
           'obs_idx': obs_idx, 'start_X': b['start_X'].numpy(), 'n_obs_ot': n_obs_ot,
           'delta_t': np.float64(delta_t), 'T': np.float64(meta['maturity']), 'observed': obs,
           'meta_json': np.array(json.dumps(meta, sort_keys=True))}
    for w in (0.5, 0.8):
        loss, path_t, path_y = sm.compute_cond_exp(b['times'], b['time_ptr'], X, obs_idx, delta_t,
                                                   meta['maturity'], start_X, n_obs_ot,
                                                   return_path=True, get_loss=True, weight=w)
        out['loss_w{}'.format(w)] = np.float64(loss)
        opt = sm.get_optimal_loss(b['times'], b['time_ptr'], X, obs_idx, delta_t, meta['maturity'],
                                  start_X, n_obs_ot, weight=w)
        assert opt == loss
    out['path_t'], out['path_y'] = path_t, path_y
    print('combined cond. exp.: {} path rows'.format(len(path_t)))
    np.savez_compressed(os.path.join(HERE, 'g17_combined_condexp.npz'), **out)


if __name__ == '__main__':
    make_hwf()
    make_combined_condexp(make_combined_data())
