"""GPU matrix of the batch producer (include/njode_producer.h, njode_amd/device_data.py): every
model, stream, lift and epoch path against a host computation.

**Generation** (``GEN_ROWS`` x the three models).  ``DeviceDataset.generate(name, hp, seed)``
without supplied draws against ``oracle.producer_oracle.philox_dataset``: the Philox streams
restated in numpy, fed through the host generators of ``njode_amd/stock_model.py``.  Mask and
``nb_obs`` are compared exactly.  Paths:

* Black-Scholes / Ornstein-Uhlenbeck, **step-local**: the host's one-step formula
  ``s' = (s + mu dt) + sig (z sqrt(dt))`` is applied in float64 to the DEVICE's own previous
  value and the oracle's normal of that step and compared with the device's next value, so one
  step's rounding is all that is compared and the error does not accumulate with S.  The device
  evaluates the same expression tree (no contraction) from the same ``s``; the two sides differ
  in ``z`` (device ``log`` / ``sqrt`` / ``sincospi`` against numpy's ``log`` / ``sqrt`` /
  ``cos(2 pi u)``) and, with a sine coefficient, in ``pc = 1 + sin(c t)``.  With
  eps = 2**-52 (one ulp, relative) the allowance is

      eps * ( K_SUM  * (|s| + |mu| dt + |sig| sqrt(dt) |z|)      # the recurrence
            + K_Z    * |sig| sqrt(dt) |z|                         # radius of the Box-Muller pair
            + K_TRIG * |sig| sqrt(dt) R_MAX                       # its angle
            + K_PC   * |mu / pc| dt )                             # sine rows only

  - K_SUM = 6: the perturbed ``z`` and ``pc`` are re-rounded in ``z sqrt(dt)``, ``sig dW``,
    ``mu`` (two products), ``mu dt`` and the two additions: at most one ulp of a term of the
    sum each, and every term is at most the unit in brackets.
  - K_Z = 4: ``rad = sqrt(-2 log(u1))``: ``log`` within 2 ulp on either side (4 ulp between
    them, halved by the root), one ulp for the two roots, one for the two products
    ``rad * trig``: 2 + 1 + 1.
  - K_TRIG = 8, ABSOLUTE on the trigonometric factor (|cos|, |sin| <= 1), because near a zero
    of the factor its error is not relative to it: numpy's angle ``2.0 * np.pi * u2`` is rounded
    once (<= eps/2 of an angle <= 2 pi: 3.2 eps) and carries the representation error of
    ``np.pi`` (3.9e-17 relative: 1.1 eps at 2 pi), then ``cos`` / ``sin`` within one ulp of a
    value <= 1 on either side (2 eps): 6.3 eps, taken as 8.  The device's ``sincospi`` reduces
    its argument exactly.  It multiplies the radius, bounded by
    R_MAX = sqrt(2 * 53 * ln 2) = 8.572 (u1 >= 2**-53).
  - K_PC = 4: ``sin`` within one ulp of a value <= 1 on either side (2 eps absolute on ``pc``,
    times ``|mu / pc|``: ``pc`` passes through zero, so the term is not relative to ``mu``)
    and the re-rounded products.
  At S <= 30 the whole trajectory is also held to the suite's ``rtol = 1e-12`` against the
  oracle's.
* Heston: the variance is not an output, so the whole trajectory is compared, with a tolerance
  measured on the REFERENCE side: the host generator run on the oracle's normals and on those
  normals moved by one ulp to EITHER neighbour (``np.nextafter(z, +inf)`` and
  ``np.nextafter(z, -inf)``: a libm result is off in either direction); the row's ``rtol`` is
  16 x the largest relative spread between the host runs (a few libm calls, each a few ulp off
  instead of one), floored at 1e-12.  Both neighbours are needed: a step that nearly cancels
  the spot (row N = 1000, S = 30, seed c0ffee9e3779b9, path 962: s_k / s_{k-1} = 8.3e-5)
  quantises its result in steps of 2.67e-12 relative, which the move towards -inf crosses
  (spread 2.67e-12) and the move towards +inf happens not to (6.8e-14 on the whole row,
  2.2e-15 on that path); the device lands on the -inf neighbour's value, 2.668e-12 away.  The host spot paths are asserted finite first: a negative variance
  would put a NaN into the spot at that step and every later one, so finite paths are paths
  whose variance stayed non-negative (the parameters are Feller-safe: 2 speed mean = 16 >
  volatility**2 = 0.09).

**Moments** with analytic spreads (100 000 paths x 100 steps): the Euler scheme's first and
second moments are exact recursions, and so are the standard errors of their estimators (BS: the
fourth-moment recursion; OU: Gaussian paths), bounded at 5 standard errors.

**Collate** (``COLLATE_ROWS``) bit-exact against ``data_utils.collate_arrays``; ``exp`` columns
may differ by one fp32 ulp (the device's ``exp`` and ``np.exp`` are float64 values a few ulp
apart, whose fp32 casts differ by at most one fp32 ulp); identity and power columns stay
bit-exact.  **Epoch form**: ``fill_batch(prepare_batches(lists)[i])`` against ``collate`` and
against the host collate.

Measured on an MI355X (figures also in DESIGN.md section 4e):
* step-local error / allowance, worst row: 0.158 (OU, N = 257, S = 301, dim 2, sine on);
  Black-Scholes 0.138 (N = 63, S = 301, dim 3).
* Heston, host spread -> device error (rtol = max(16 spread, 1e-12)), rows in table order:
  0 -> 1.3e-16; 1.4e-14 -> 1.5e-14; 2.0e-12 -> 4.9e-13; 2.67e-12 -> 2.67e-12; 6.6e-14 -> 6.8e-14;
  1.1e-14 -> 7.4e-15; 1.0e-14 -> 6.2e-15; 1.0e-12 -> 3.3e-13; 3.0e-15 -> 1.1e-15;
  7.1e-9 -> 3.4e-11 (N = 100 000, S = 4: dt = 1/4 at a spot volatility of 2, steps cross zero).
* moments: every mean, second moment and cross covariance within 2.2 standard errors.
* the module: 68 tests in 3.4 - 4.8 s.
"""
import numpy as np
import pytest
import torch

from hip_util import demo_cfg, hip_model
from njode_amd import _lib, data_utils, device_data, stock_model
from oracle import producer_oracle as po

pytestmark = pytest.mark.gpu
HP = dict(data_utils.hyperparam_default)
MODELS = ('BlackScholes', 'OrnsteinUhlenbeck', 'Heston')
EPS = 2.0 ** -52
K_SUM, K_Z, K_TRIG, K_PC = 6, 4, 8, 4
R_MAX = float(np.sqrt(2 * 53 * np.log(2.0)))
SEED_LONG = 0x1234567890ab
SEED_HI_A, SEED_HI_B = (0x00c0ffee << 32) | 0x9e3779b9, (0x00c0ffef << 32) | 0x9e3779b9

# ---- generation and sampling: every row runs for each model --------------------------------
# (N, S, dim, sine_coeff, seed, Heston correlation, obs_perc)
GEN_ROWS = [
    (1, 1, 1, None, 0, -0.7, 0.0),
    (63, 2, 2, 2.0, 5, 0.0, 1.0),
    (257, 7, 3, None, SEED_LONG, 0.5, 0.1),
    (1000, 30, 1, 2.0, SEED_HI_A, 1.0, 0.1),
    (1000, 30, 1, 2.0, SEED_HI_B, 1.0, 0.1),
    (257, 301, 2, 2.0, 5, -0.7, 0.1),
    (63, 301, 3, None, SEED_LONG, 0.0, 1.0),
    (1000, 7, 2, 2.0, 0, 0.5, 0.0),
    (1, 30, 3, 2.0, 5, 1.0, 1.0),
    (100000, 4, 3, None, 0, 0.5, 0.1),
]
GEN_AXES = {
    'N': (0, (1, 63, 257, 1000, 100000)),
    'S': (1, (1, 2, 7, 30, 301)),
    'dim': (2, (1, 2, 3)),
    'sine_coeff': (3, (None, 2.0)),
    'seed': (4, (0, 5, SEED_LONG, SEED_HI_A, SEED_HI_B)),
    'correlation': (5, (-0.7, 0.0, 0.5, 1.0)),
    'obs_perc': (6, (0.0, 0.1, 1.0)),
}
GEN_CASES = [(m, r) for m in MODELS for r in GEN_ROWS]


def _row_id(case):
    m, (n, s, d, sine, seed, rho, perc) = case
    return '{}-N{}-S{}-d{}-sine{}-seed{:x}-rho{}-p{}'.format(m, n, s, d, sine, seed, rho, perc)


def _hp(row):
    n, s, d, sine, _, rho, perc = row
    return dict(HP, nb_paths=n, nb_steps=s, S0=[1.0] * d if d > 1 else 1, sine_coeff=sine,
                correlation=rho, obs_perc=perc)


# ---- collate: (key, N, S, dim, lifts, grid times emptied, dataset) -----------------------------
# dataset: 'host' = create_dataset arrays uploaded, a model name = DeviceDataset.generate
COLLATE_ROWS = [
    ('exp-d1', 333, 60, 1, ('exp',), (17,), 'host'),
    ('exp-d3', 333, 60, 3, ('exp',), (17,), 'host'),
    ('pow2-exp-d1', 333, 60, 1, ('power-2', 'exp'), (17,), 'host'),
    ('pow2-exp-d3', 333, 60, 3, ('power-2', 'exp'), (17,), 'host'),
    ('four-d1', 333, 60, 1, ('exp', 'power-3', 'power-2', 'power-5'), (17,), 'host'),
    ('four-d3', 500, 60, 3, ('exp', 'power-3', 'power-2', 'power-5'), (17,), 'host'),
    ('S300', 450, 300, 2, ('power-2',), (17, 255, 256, 257, 258, 299), 'host'),
    ('S700', 300, 700, 1, (), (3, 256, 257, 300, 511, 512, 513, 514, 699), 'host'),
    ('S1', 100, 1, 2, ('power-2', 'exp'), (), 'host'),
    ('gen-BS', 600, 30, 2, ('power-2', 'exp'), (), 'BlackScholes'),
    ('gen-OU', 600, 30, 3, ('exp',), (), 'OrnsteinUhlenbeck'),
    ('gen-Heston', 600, 30, 1, ('power-3',), (), 'Heston'),
]
BIG_N = 20000                      # the headline batch: its own test, one case per index form
HEADLINE_FORMS = {'whole': BIG_N, 'permutation': BIG_N, 'replacement': BIG_N + 5000}   # form: B
SUB_BATCHES = (1, 63, 65, 257)
EPOCH_SIZES = (64, 64, None, 1, 257, 13)       # None: the batch of paths without any observation
EPOCH_ROWS = ('four-d3', 'S300', 'gen-BS', 'gen-OU')


def test_the_tables_cover_what_they_claim():
    for m in MODELS:
        rows = [r for mm, r in GEN_CASES if mm == m]
        for axis, (col, values) in GEN_AXES.items():
            seen = {r[col] for r in rows}
            assert set(values) <= seen, (m, axis, set(values) - seen)
    assert (SEED_HI_A ^ SEED_HI_B) >> 32 and not (SEED_HI_A ^ SEED_HI_B) & 0xFFFFFFFF
    a, b = [[r for r in GEN_ROWS if r[4] == s] for s in (SEED_HI_A, SEED_HI_B)]
    assert len(a) == len(b) == 1 and a[0][:4] + a[0][5:] == b[0][:4] + b[0][5:]
    assert any(r[0] == 100000 and r[1] == 4 and r[2] == 3 for r in GEN_ROWS)
    assert all(r[0] * r[1] * r[2] <= 1.3e6 for r in GEN_ROWS)        # counters of the numpy oracle
    # collate: a workgroup past index 256 with observations to place, empty grid times on both
    # sides of it, a batch of more than 4 passes of the 256-wide batch loop
    for key in ('S300', 'S700'):
        _, _, observed, _, _ = _collate_dataset(key)
        counts = observed[:, 1:].sum(0)
        assert (counts[257:] > 0).any(), key
        assert (counts[:256] == 0).any() and (counts[257:] == 0).any(), key
    assert set(HEADLINE_FORMS) == {'whole', 'permutation', 'replacement'}
    assert min(HEADLINE_FORMS.values()) > 256 * 4 and HEADLINE_FORMS['replacement'] > BIG_N
    for lifts in (('exp',), ('power-2', 'exp'), ('exp', 'power-3', 'power-2', 'power-5')):
        assert {r[3] for r in COLLATE_ROWS if r[4] == lifts and r[6] == 'host'} >= {1, 3}, lifts
    assert {r[6] for r in COLLATE_ROWS} >= set(MODELS)
    assert any(r[2] == 1 for r in COLLATE_ROWS)
    assert set(EPOCH_ROWS) <= {r[0] for r in COLLATE_ROWS}


# ================================ generation ==================================================
_GEN_CACHE = {}


def _generated(name, row):
    """(device paths [N, d, S+1], observed, nb_obs) of one row; kept for the tests that share it."""
    key = (name, row)
    if key not in _GEN_CACHE:
        if len(_GEN_CACHE) > 4:
            _GEN_CACHE.clear()
        ds = device_data.DeviceDataset.generate(name, _hp(row), seed=row[4])
        _GEN_CACHE[key] = ds.to_arrays()
    return _GEN_CACHE[key]


def _step_local_ratio(name, hp, got, z):
    """Largest |device step - host step formula on the device's previous value| / allowance."""
    S = hp['nb_steps']
    dt = hp['maturity'] / S
    sq = np.sqrt(dt)
    sine = hp['sine_coeff']
    worst = 0.0
    for k in range(1, S + 1):
        prev, zk = got[:, :, k - 1], z[:, k - 1, :]
        pc = 1 if sine is None else (1 + np.sin(sine * ((k - 1) * dt)))
        dW = zk * sq
        if name == 'BlackScholes':                       # stock_model.BlackScholes.generate_paths
            mu = hp['drift'] * pc * prev
            sig = hp['volatility'] * prev
            mu_pc1 = hp['drift'] * prev
        else:                                            # stock_model.OrnsteinUhlenbeck.generate_paths
            mu = -hp['speed'] * pc * (prev - hp['mean'])
            sig = hp['volatility'] * np.ones_like(prev)
            mu_pc1 = hp['speed'] * (prev - hp['mean'])
        want = prev + mu * dt + sig * dW
        noise = np.abs(sig) * sq
        allow = EPS * (K_SUM * (np.abs(prev) + np.abs(mu) * dt + noise * np.abs(zk))
                       + K_Z * noise * np.abs(zk) + K_TRIG * noise * R_MAX
                       + (K_PC * np.abs(mu_pc1) * dt if sine is not None else 0.0))
        worst = max(worst, float((np.abs(got[:, :, k] - want) / allow).max()))
    return worst


def _heston_tolerance(hp, normals, uniforms):
    """16 x the host generator's own relative spread under a one-ulp move of its normals, to
    either neighbour (see the module docstring)."""
    spread = 0.0
    with np.errstate(invalid='raise'):                   # sqrt of a negative variance
        a = po.host_dataset('Heston', hp, normals, uniforms)[0]
        assert np.isfinite(a).all() and (a != 0).all()
        for toward in (np.inf, -np.inf):
            b = po.host_dataset('Heston', hp, np.nextafter(normals, toward), uniforms)[0]
            assert np.isfinite(b).all()
            spread = max(spread, float((np.abs(a - b) / np.abs(a)).max()))
    return a, spread, max(16 * spread, 1e-12)


@pytest.mark.parametrize('case', GEN_CASES, ids=_row_id)
def test_generate_follows_the_oracle_dataset(case):
    name, row = case
    n, s, d, sine, seed, rho, perc = row
    hp = _hp(row)
    got_paths, got_obs, got_nb = _generated(name, row)
    assert got_paths.shape == (n, d, s + 1) and got_obs.shape == (n, s + 1) and got_nb.shape == (n,)
    normals, uniforms = po.dataset_draws(name, hp, seed)
    # -- mask: exact; column 0 follows the stream and is not counted
    want_obs = (uniforms < perc) * 1
    np.testing.assert_array_equal(got_obs, want_obs)
    np.testing.assert_array_equal(got_obs[:, 0], (uniforms[:, 0] < perc) * 1)
    np.testing.assert_array_equal(got_nb, want_obs[:, 1:].sum(1))
    np.testing.assert_array_equal(got_nb, got_obs[:, 1:].sum(1))
    if perc in (0.0, 1.0):
        assert (got_obs == int(perc)).all() and (got_nb == int(perc) * s).all()
    # -- paths
    assert np.isfinite(got_paths).all()
    np.testing.assert_array_equal(got_paths[:, :, 0], np.full((n, d), 1.0))
    if name == 'Heston':
        ref, spread, tol = _heston_tolerance(hp, normals, uniforms)
        err = float((np.abs(got_paths - ref) / np.abs(ref)).max())
        print('HESTON-ROW {} host spread {:.3e} rtol {:.3e} device err {:.3e}'.format(
            _row_id(case), spread, tol, err))
        assert err <= tol, (err, tol, spread)
    else:
        ratio = _step_local_ratio(name, hp, got_paths, normals)
        print('STEP-LOCAL {} worst error / allowance {:.4f}'.format(_row_id(case), ratio))
        assert ratio <= 1.0, ratio
        if s <= 30:
            ref = po.host_dataset(name, hp, normals, uniforms)[0]
            np.testing.assert_allclose(got_paths, ref, rtol=1e-12, atol=0)
    # -- the same seed again: the same bits
    if n <= 1000:
        ds = device_data.DeviceDataset.generate(name, hp, seed=seed)
        again = ds.to_arrays()
        for x, y in zip(again, (got_paths, got_obs, got_nb)):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize('name', MODELS)
def test_seeds_and_dimensions_give_different_draws(name):
    rows = {r[4]: r for r in GEN_ROWS}
    pa, oa, _ = _generated(name, rows[SEED_HI_A])
    pb, ob, _ = _generated(name, rows[SEED_HI_B])
    assert (pa[:, :, 1:] != pb[:, :, 1:]).all()          # high word only: every step differs
    assert (oa != ob).any() and abs((oa != ob).mean() - 2 * 0.1 * 0.9) < 0.02
    # another low word
    row = (1000, 30, 1, 2.0, SEED_HI_A + 1, 1.0, 0.1)
    ds = device_data.DeviceDataset.generate(name, _hp(row), seed=row[4])
    pc, oc, _ = ds.to_arrays()
    assert (pa[:, :, 1:] != pc[:, :, 1:]).all() and (oa != oc).any()
    # dimensions: no two share their draws (every path, every step from the first on)
    for row in (r for r in GEN_ROWS if r[2] == 3 and r[0] <= 1000):
        p, _, _ = _generated(name, row)
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert (p[:, i, 1:] != p[:, j, 1:]).all(), (row, i, j)


@pytest.mark.parametrize('name', MODELS)
def test_path_and_observation_streams_of_one_seed_are_uncorrelated(name):
    """The step's increment (monotone in the step's normal) against the uniform's indicator of
    the same (path, grid time): same 4-sigma form as the oracle's moment tests."""
    row = (1000, 30, 1, None, 5, 0.5, 0.5)
    ds = device_data.DeviceDataset.generate(name, _hp(row), seed=row[4])
    p, o, _ = ds.to_arrays()
    inc = p[:, 0, 1:] / p[:, 0, :-1] if name != 'OrnsteinUhlenbeck' else p[:, 0, 1:] - p[:, 0, :-1]
    for lag_obs in (o[:, 1:], o[:, :-1]):                # the step into grid time k / out of it
        a = inc - inc.mean(0)                            # per step: the drift differs by step
        b = lag_obs - lag_obs.mean(0)
        assert abs(np.mean(a * b)) < 4 * np.sqrt(np.mean(a * a) * np.mean(b * b) / a.size)


def _euler_moments(name, hp, n):
    """Exact moments of the Euler scheme's X_T and the standard errors of their estimators over
    n paths: (mean, se_mean, second, se_second, variance) -- ``second`` is E[X^2] and its
    estimator mean(x^2) for Black-Scholes, Var[X] and the sample variance for OU."""
    S = hp['nb_steps']
    dt = hp['maturity'] / S
    sine = hp['sine_coeff']
    if name == 'BlackScholes':
        m1 = m2 = m4 = 1.0
        for k in range(1, S + 1):
            pc = 1.0 if sine is None else 1.0 + np.sin(sine * (k - 1) * dt)
            a, b2 = 1.0 + hp['drift'] * pc * dt, hp['volatility'] ** 2 * dt
            m1 *= a
            m2 *= a * a + b2
            m4 *= a ** 4 + 6 * a * a * b2 + 3 * b2 * b2      # E[(a + b z)^4]
        var = m2 - m1 * m1
        return m1, np.sqrt(var / n), m2, np.sqrt((m4 - m2 * m2) / n), var
    mean, var = 1.0, 0.0
    for k in range(1, S + 1):
        pc = 1.0 if sine is None else 1.0 + np.sin(sine * (k - 1) * dt)
        mean = mean - hp['speed'] * pc * (mean - hp['mean']) * dt
        var = var * (1.0 - hp['speed'] * pc * dt) ** 2 + hp['volatility'] ** 2 * dt
    return mean, np.sqrt(var / n), var, var * np.sqrt(2.0 / (n - 1)), var


@pytest.mark.parametrize('name', ['BlackScholes', 'OrnsteinUhlenbeck'])
@pytest.mark.parametrize('dim,sine,seed', [(1, None, 5), (1, 2.0, 6), (2, None, 7), (2, 2.0, 8)])
def test_first_and_second_moments_within_analytic_standard_errors(name, dim, sine, seed):
    n = 100000
    hp = dict(HP, nb_paths=n, nb_steps=100, sine_coeff=sine, S0=[1.0] * dim if dim > 1 else 1)
    ds = device_data.DeviceDataset.generate(name, hp, seed=seed)
    xT = ds.paths_tm[-1].cpu().numpy()                    # [d, N]
    mean, se_mean, second, se_second, var = _euler_moments(name, hp, n)
    for j in range(dim):
        x = xT[j]
        est2 = np.mean(x * x) if name == 'BlackScholes' else x.var(ddof=1)
        print('MOMENTS {} d{}/{} sine {}: mean {:+.2f} se, second {:+.2f} se'.format(
            name, j, dim, sine, (x.mean() - mean) / se_mean, (est2 - second) / se_second))
        assert abs(x.mean() - mean) < 5 * se_mean
        assert abs(est2 - second) < 5 * se_second
    if dim == 2:
        cov = np.mean((xT[0] - mean) * (xT[1] - mean))    # independent: Var = var^2 / n
        print('MOMENTS {} sine {}: cross covariance {:+.2f} se'.format(name, sine, cov / (var / np.sqrt(n))))
        assert abs(cov) < 5 * var / np.sqrt(n)


# ================================== collate ===================================================
_COLLATE_CACHE = {}
_GENERATED_DATASETS = {}


def _collate_dataset(key):
    """(row, paths, observed, nb_obs, meta) of a COLLATE_ROWS entry on the host; generated rows
    are made on the device and read back (module cache: the epoch tests reuse them)."""
    if key in _COLLATE_CACHE:
        return _COLLATE_CACHE[key]
    row = next(r for r in COLLATE_ROWS if r[0] == key)
    _, n, s, d, _, empty, source = row
    hp = dict(HP, nb_paths=n, nb_steps=s, S0=[1.0] * d if d > 1 else 1,
              obs_perc=0.5 if s == 1 else 0.1)
    if source == 'host':
        paths, observed, nb_obs, meta = data_utils.create_dataset('BlackScholes', hp, seed=4)
        for t in empty:
            observed[:, t] = 0
        observed[:5, :] = 0                               # five paths without any observation
        nb_obs = observed[:, 1:].sum(1)
    else:
        # the object generate returned is the dataset under test (_device_dataset); the host side
        # is its to_arrays() and the HOST model's dt, not the device object's metadata
        ds = _GENERATED_DATASETS[key] = device_data.DeviceDataset.generate(source, hp, seed=9)
        paths, observed, nb_obs = ds.to_arrays()
        meta = dict(hp, dt=stock_model.STOCK_MODELS[source](**hp).generate_paths()[1])
        assert meta['dt'] == hp['maturity'] / hp['nb_steps']
    _COLLATE_CACHE[key] = (row, paths, observed, nb_obs, meta)
    return _COLLATE_CACHE[key]


def _device_dataset(key):
    """The dataset under test: host arrays uploaded, or, for the generated rows, the very
    ``DeviceDataset`` that ``generate`` returned."""
    row, paths, observed, nb_obs, meta = _collate_dataset(key)
    if row[6] != 'host':
        ds = _GENERATED_DATASETS[key]
        assert ds.metadata['dt'] == meta['dt'] and \
            (ds.n_paths, ds.dim, ds.n_steps) == (row[1], row[3], row[2])
        return ds
    return device_data.DeviceDataset.from_arrays(paths, observed, nb_obs, meta)


def _exp_columns(funcs, dim):
    return [(q + 1) * dim + j for q, f in enumerate(funcs) if f == 'exp' for j in range(dim)]


def _assert_values(got, ref, exp_cols):
    """fp32 [rows, width]: bit-exact, but the ``exp`` columns within one fp32 ulp."""
    got, ref = got.cpu().numpy(), ref.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    exact = np.ones(got.shape[1], dtype=bool)
    exact[exp_cols] = False
    np.testing.assert_array_equal(got[:, exact].view(np.int32), ref[:, exact].view(np.int32))
    if exp_cols and got.shape[0]:
        g, r = got[:, ~exact], ref[:, ~exact]
        assert (g > 0).all() and (r > 0).all()            # positive floats: ordered as integers
        ulps = np.abs(g.view(np.int32).astype(np.int64) - r.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, ulps.max()


def _assert_same_batch(got, ref, exp_cols=()):
    """A device batch against the host collate's, every field."""
    np.testing.assert_array_equal(got['times'], ref['times'])
    assert got['times'].dtype == np.float64
    np.testing.assert_array_equal(got['time_ptr'], ref['time_ptr'])
    np.testing.assert_array_equal(got['obs_idx'].cpu().numpy(), ref['obs_idx'].numpy())
    np.testing.assert_array_equal(got['n_obs_ot'].cpu().numpy(), ref['n_obs_ot'].numpy())
    _assert_values(got['X'], ref['X'], list(exp_cols))
    _assert_values(got['start_X'], ref['start_X'], list(exp_cols))


def _assert_identical(a, b):
    """Two device batches, bit for bit."""
    np.testing.assert_array_equal(a['times'], b['times'])
    np.testing.assert_array_equal(a['time_ptr'], b['time_ptr'])
    for k in ('obs_idx', 'n_obs_ot', 'X', 'start_X'):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def _host_batch(key, idx=None):
    row, paths, observed, nb_obs, meta = _collate_dataset(key)
    fns = [data_utils._get_func(f) for f in row[4]]
    if idx is None:
        idx = slice(None)
    return data_utils.collate_arrays(paths[idx], observed[idx], nb_obs[idx], meta['dt'], fns)


@pytest.mark.parametrize('key', [r[0] for r in COLLATE_ROWS])
def test_device_collate_matrix(key):
    row, paths, observed, nb_obs, meta = _collate_dataset(key)
    _, n, s, d, funcs, _, _ = row
    ds = _device_dataset(key)
    exp_cols = _exp_columns(funcs, d)
    whole = ds.collate(func_names=funcs)
    _assert_same_batch(whole, _host_batch(key), exp_cols)
    assert whole['X'].shape[1] == whole['start_X'].shape[1] == d * (1 + len(funcs))
    rng = np.random.RandomState(1)
    for B in SUB_BATCHES:
        idx = rng.permutation(n)[:B]
        _assert_same_batch(ds.collate(idx, func_names=funcs), _host_batch(key, idx), exp_cols)
    # idx as a device tensor (unchecked form) gives the same batch as the host list
    idx = rng.permutation(n)[:min(n, 130)]
    _assert_identical(ds.collate(torch.as_tensor(idx, dtype=torch.int64).cuda(), func_names=funcs),
                      ds.collate(idx.tolist(), func_names=funcs))
    # column order [x, lift1(x), ...] per dim block, from the float64 dataset directly
    fns = [lambda a: a] + [data_utils._get_func(f) for f in funcs]
    counts = observed[:, 1:].sum(0)
    t_of_row = np.repeat(np.nonzero(counts)[0] + 1, counts[counts > 0])
    b_of_row = whole['obs_idx'].cpu().numpy()
    X, start_X = whole['X'].cpu().numpy(), whole['start_X'].cpu().numpy()
    if d > 1:
        assert (paths[:, 0, 1:] != paths[:, 1, 1:]).all()    # a block out of place would show
    for q, f in enumerate(fns):
        for j in range(d):
            want = f(paths[b_of_row, j, t_of_row]).astype(np.float32)
            want0 = f(paths[:, j, 0]).astype(np.float32)
            col = q * d + j
            if col in exp_cols:
                np.testing.assert_allclose(X[:, col], want, rtol=2.0 ** -23, atol=0)
                np.testing.assert_allclose(start_X[:, col], want0, rtol=2.0 ** -23, atol=0)
            else:
                np.testing.assert_array_equal(X[:, col], want)
                np.testing.assert_array_equal(start_X[:, col], want0)


@pytest.mark.parametrize('form', sorted(HEADLINE_FORMS))
def test_collate_of_the_headline_batch(form):
    """B = 20 000 of N = 20 000 (79 passes of the batch loop): whole dataset, a permutation, and
    sampling with replacement, where B > N is legal."""
    hp = dict(HP, nb_paths=BIG_N, nb_steps=100)
    paths, observed, nb_obs, meta = data_utils.create_dataset('BlackScholes', hp, seed=1)
    observed[:, 50] = 0
    nb_obs = observed[:, 1:].sum(1)
    ds = device_data.DeviceDataset.from_arrays(paths, observed, nb_obs, meta)
    funcs = ('power-2',)
    fns = [data_utils._get_func(f) for f in funcs]
    rng = np.random.RandomState(2)
    B = HEADLINE_FORMS[form]
    idx = {'whole': None, 'permutation': rng.permutation(BIG_N),
           'replacement': rng.randint(0, BIG_N, size=B)}[form]
    sel = slice(None) if idx is None else idx
    ref = data_utils.collate_arrays(paths[sel], observed[sel], nb_obs[sel], meta['dt'], fns)
    got = ds.collate(idx, func_names=funcs)
    _assert_same_batch(got, ref)
    assert got['start_X'].shape[0] == B > 256 * 4                # more than 4 passes of the batch loop
    if form == 'replacement':
        assert len(np.unique(idx)) < len(idx) and len(idx) > BIG_N
    elif form == 'permutation':
        assert (np.sort(idx) == np.arange(BIG_N)).all() and (idx != np.arange(BIG_N)).any()


# ================================ epoch form ==================================================
def _epoch_lists(key, seed):
    """Batch lists of EPOCH_SIZES; the ``None`` entry is a batch of paths without observations."""
    _, _, observed, nb_obs, _ = _collate_dataset(key)
    dead = np.nonzero(nb_obs == 0)[0]
    assert len(dead) >= 3, (key, len(dead))
    live = np.random.RandomState(seed).permutation(np.nonzero(nb_obs > 0)[0])
    lists, at = [], 0
    for size in EPOCH_SIZES:
        if size is None:
            lists.append(dead[::-1].copy())
        else:
            lists.append(live[at:at + size])
            at += size
    assert at <= len(live)
    return lists


@pytest.mark.parametrize('key', EPOCH_ROWS)
def test_epoch_form_equals_collate_and_the_host_collate(key):
    row = _collate_dataset(key)[0]
    funcs, d = row[4], row[3]
    ds = _device_dataset(key)
    exp_cols = _exp_columns(funcs, d)
    lists = _epoch_lists(key, seed=0)
    preps = ds.prepare_batches(lists)
    assert len(preps) == len(lists)
    for i, (prep, idx) in enumerate(zip(preps, lists)):
        got = ds.fill_batch(prep, func_names=funcs)
        _assert_identical(got, ds.collate(idx, func_names=funcs))
        _assert_same_batch(got, _host_batch(key, idx), exp_cols)
        assert got['start_X'].shape[0] == len(idx) == prep['B']
    empty = ds.fill_batch(preps[EPOCH_SIZES.index(None)], func_names=funcs)
    assert empty['X'].shape[0] == 0 and len(empty['times']) == 0 and empty['time_ptr'].tolist() == [0]
    assert preps[EPOCH_SIZES.index(None) + 1]['time_ptr'][-1] > 0      # ... in the MIDDLE of the list


@pytest.mark.parametrize('key', ['four-d3', 'gen-OU'])
def test_next_epochs_prepare_does_not_disturb_pending_fills(key):
    """The training loop prepares epoch e + 1 before the fills of epoch e have run."""
    row = _collate_dataset(key)[0]
    funcs, d = row[4], row[3]
    ds = _device_dataset(key)
    exp_cols = _exp_columns(funcs, d)
    first, second = _epoch_lists(key, seed=1), _epoch_lists(key, seed=2)
    assert any((a != b).any() for a, b in zip(first, second) if len(a) == len(b) > 5)
    p1 = ds.prepare_batches(first)
    p2 = ds.prepare_batches(second)
    p3 = ds.prepare_batches(second[::-1])                # and one more, never filled
    for prep, idx in list(zip(p1, first)) + list(zip(p2, second)):
        _assert_same_batch(ds.fill_batch(prep, func_names=funcs), _host_batch(key, idx), exp_cols)
    assert len(p3) == len(second)


def test_training_step_on_the_epoch_form_of_a_generated_dataset():
    """generate -> prepare_batches -> fill_batch -> loss_and_grad, the chain the default loop
    runs: loss and flat gradient equal the step on the host-collated batch of the same rows."""
    hp = dict(HP, nb_paths=500, nb_steps=100)
    ds = device_data.DeviceDataset.generate('BlackScholes', hp, seed=3)
    paths, observed, nb_obs = ds.to_arrays()
    meta = dict(hp, dt=stock_model.BlackScholes(**hp).generate_paths()[1])    # the host model's dt
    assert ds.metadata['dt'] == meta['dt']
    perm = np.random.RandomState(0).permutation(500)
    lists = [perm[:200], perm[200:264], perm[264:500]]
    torch.manual_seed(0)
    m = hip_model(demo_cfg()).train()
    for prep, idx in zip(ds.prepare_batches(lists), lists):
        host = data_utils.collate_arrays(paths[idx], observed[idx], nb_obs[idx], meta['dt'])
        dev = ds.fill_batch(prep)
        _assert_same_batch(dev, host)
        out = []
        for b in (host, dev):
            _, loss = m.loss_and_grad(b['times'], b['time_ptr'], b['X'].cuda(), b['obs_idx'].cuda().int(),
                                      meta['dt'], meta['maturity'], b['start_X'].cuda(),
                                      b['n_obs_ot'].cuda().int())
            out.append((float(loss), m.flat_grad().clone()))
        assert np.isfinite(out[0][0]) and out[0][1].abs().sum() > 0
        assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])


# ================================ index check =================================================
class _NoLaunch:
    """The library with its collate entry points replaced by recorders that launch nothing."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        if name.startswith('njode_collate'):
            def refuse(*args):
                self.calls.append(name)
                raise AssertionError(name + ' was called')
            return refuse
        return getattr(self._real, name)


def test_rows_outside_the_dataset_are_refused_before_any_launch(monkeypatch):
    ds = _device_dataset('S1')
    n = ds.n_paths
    good = [np.array([0, n - 1, 3]), [n - 1], np.arange(n)]
    for prep, idx in zip(ds.prepare_batches(good), good):          # the bounds themselves pass
        _assert_same_batch(ds.fill_batch(prep), _strip_lifts('S1', idx))
    proxy = _NoLaunch(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: proxy)
    for bad in (-1, n, n + 7, 2 ** 31, -2 ** 31 - 1, 2 ** 32 + 1):
        for lists in ([[0, 1], [2, bad, 3]], [[bad]], [np.array([1, 2]), np.array([bad])]):
            with pytest.raises(ValueError, match='outside'):
                ds.prepare_batches(lists)
        for idx in ([bad], np.array([0, bad]), torch.tensor([1, bad])):
            with pytest.raises(ValueError, match='outside'):
                ds.collate(idx)
    for bad in ([1.5], [2.0], [2 ** 63], [2 ** 70]):                # nothing truncated or wrapped
        with pytest.raises(ValueError, match='integers'):
            ds.collate(bad)
        with pytest.raises(ValueError, match='integers'):
            ds.prepare_batches([[0, 1], bad])
    assert proxy.calls == []
    with pytest.raises(AssertionError, match='njode_collate_count was called'):
        ds.collate([0])                                             # the recorder does see a launch
    assert proxy.calls == ['njode_collate_count']


def _strip_lifts(key, idx):
    _, paths, observed, nb_obs, meta = _collate_dataset(key)
    return data_utils.collate_arrays(paths[idx], observed[idx], nb_obs[idx], meta['dt'])
