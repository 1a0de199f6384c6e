"""CPU tests of the batch producer's host logic and of the Philox restatement that checks the
device random streams (pinned to the algorithm's published known-answer vectors)."""
import os
import re

import numpy as np
import pytest

from njode_amd import _lib, data_utils, device_data
from oracle import producer_oracle as po

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123 kat_vectors, philox4x32-10: (counter, key, expected)
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_restatement_matches_known_answer_vectors():
    for ctr, key, want in KAT:
        got = po.philox4x32_10(np.array([ctr], dtype=np.uint32), np.array([key], dtype=np.uint32))
        assert tuple(int(x) for x in got[0]) == want


def test_u53_is_numpys_double_recipe():
    a = np.array([0, 0xffffffff, 0x12345678], dtype=np.uint32)
    b = np.array([0, 0xffffffff, 0x9abcdef0], dtype=np.uint32)
    want = ((a >> 5).astype(np.float64) * 67108864.0 + (b >> 6)) / 9007199254740992.0
    np.testing.assert_array_equal(po.u53(a, b), want)
    assert po.u53(a, b).max() < 1.0


def test_oracle_streams_have_the_right_moments():
    u = po.observation_uniforms(2000, 100, seed=7)
    assert u.shape == (2000, 101) and 0.0 <= u.min() and u.max() < 1.0
    assert abs(u.mean() - 0.5) < 4 * np.sqrt(1 / 12 / u.size)
    z1, z2 = po.path_normals(500, 100, 1, seed=7)
    for z in (z1, z2):
        assert abs(z.mean()) < 4 / np.sqrt(z.size)
        assert abs(z.var() - 1.0) < 4 * np.sqrt(2.0 / z.size)
    assert abs(np.mean(z1 * z2)) < 4 / np.sqrt(z1.size)
    zs = po.step_normals(50, 7, 2, seed=3)          # odd step count: the last pair is half used
    a, b = po.path_normals(50, 4, 2, seed=3)
    assert zs.shape == (50, 7, 2)
    np.testing.assert_array_equal(zs[:, 0::2], a)
    np.testing.assert_array_equal(zs[:, 1::2], b[:, :3])


def test_times_from_counts_reproduces_the_collate_clock():
    paths, observed, nb_obs, hp = data_utils.create_dataset(
        'BlackScholes', dict(data_utils.hyperparam_default, nb_paths=23, nb_steps=40), seed=3)
    observed[:, 7] = 0            # a grid time nobody observes
    ref = data_utils.collate_arrays(paths, observed, observed[:, 1:].sum(1), hp['dt'])
    counts = observed[:, 1:].sum(0)
    times, time_ptr = device_data.times_from_counts(counts, hp['dt'])
    np.testing.assert_array_equal(times, ref['times'])      # bit-exact float64 clock
    np.testing.assert_array_equal(time_ptr, ref['time_ptr'])


def test_parse_powers():
    assert device_data.parse_powers(None) == []
    assert device_data.parse_powers(['power-2', 'power-3', 'exp']) == [2, 3, 0]
    with pytest.raises(ValueError):
        device_data.parse_powers(['power-0.5'])


def test_every_producer_symbol_is_declared_and_exported():
    header = open(os.path.join(REPO, 'include', 'njode_producer.h')).read()
    declared = set(re.findall(r'\b(njode_[a-z0-9_]+)\s*\(', header))
    assert declared and declared <= set(_lib.EXPORTS)
    lib = _lib.lib()
    for name in declared:
        assert hasattr(lib, name), name


MODELS = ('BlackScholes', 'OrnsteinUhlenbeck', 'Heston')


@pytest.mark.parametrize('name', MODELS)
@pytest.mark.parametrize('dim,sine', [(1, None), (2, 2.0)])
def test_philox_dataset_on_numpys_legacy_draws_is_create_dataset(name, dim, sine, monkeypatch):
    """With its three streams replaced by numpy's legacy draws in ``create_dataset``'s order,
    ``philox_dataset`` must return ``create_dataset``'s arrays bit for bit: the oracle adds
    nothing to the host generators but the source of the draws."""
    hp = dict(data_utils.hyperparam_default, nb_paths=37, nb_steps=9, sine_coeff=sine,
              S0=[1.0] * dim if dim > 1 else 1)
    seed = 13
    monkeypatch.setattr(po, 'step_normals',
                        lambda n, s, d, seed: np.random.normal(0, 1, (n, s, d)))

    def legacy_pairs(n, s, d, seed):
        z = np.random.normal(0, 1, (n, s, 2, d))
        return z[:, :, 0, :], z[:, :, 1, :]
    monkeypatch.setattr(po, 'path_normals', legacy_pairs)
    monkeypatch.setattr(po, 'observation_uniforms',
                        lambda n, s, seed: np.random.random(size=(n, s + 1)))
    np.random.seed(seed)
    paths, observed, nb_obs = po.philox_dataset(name, hp, seed)
    ref_paths, ref_observed, ref_nb, _ = data_utils.create_dataset(name, hp, seed=seed)
    np.testing.assert_array_equal(paths, ref_paths)
    np.testing.assert_array_equal(observed, ref_observed)
    np.testing.assert_array_equal(nb_obs, ref_nb)
    assert np.isfinite(paths).all()
    x = np.random.normal(0, 1, 3)            # the patch of np.random.normal is gone again
    assert x.shape == (3,)


@pytest.mark.parametrize('name', MODELS)
def test_philox_dataset_mask_seed_and_dimensions(name):
    hp = dict(data_utils.hyperparam_default, nb_paths=50, nb_steps=7, S0=[1.0] * 3, obs_perc=0.3)
    lo = 0x89abcdef
    seed_a, seed_b = (0x1234 << 32) | lo, (0x1235 << 32) | lo      # differ in the high word only
    paths, observed, nb_obs = po.philox_dataset(name, hp, seed_a)
    assert paths.shape == (50, 3, 8) and observed.shape == (50, 8) and nb_obs.shape == (50,)
    u = po.observation_uniforms(50, 7, seed_a)
    np.testing.assert_array_equal(observed, (u < 0.3) * 1)
    np.testing.assert_array_equal(nb_obs, observed[:, 1:].sum(1))   # column 0 is not counted
    assert observed[:, 0].any() and not observed[:, 0].all()        # ... though it follows the stream
    paths_b, observed_b, _ = po.philox_dataset(name, hp, seed_b)
    assert not np.array_equal(paths_b[:, :, 1:], paths[:, :, 1:])
    assert not np.array_equal(observed_b, observed)
    for j in (1, 2):                                                # every path, from step 1 on
        assert (paths[:, j, 1:] != paths[:, 0, 1:]).all()
    assert (paths[:, 1, 1:] != paths[:, 2, 1:]).all()
    again, observed_again, _ = po.philox_dataset(name, hp, seed_a)
    np.testing.assert_array_equal(again, paths)
    np.testing.assert_array_equal(observed_again, observed)


def test_path_and_observation_draws_are_uncorrelated():
    """Same seed, same (path, step) counters, different key word: the normals that drive step k
    and the uniform that decides the observation at grid time k must not move together."""
    n, s = 2000, 100
    for name in ('BlackScholes', 'Heston'):
        hp = dict(data_utils.hyperparam_default, nb_paths=n, nb_steps=s)
        normals, u = po.dataset_draws(name, hp, seed=7)
        uc = u[:, 1:] - 0.5
        zs = [normals[:, :, 0]] if name == 'BlackScholes' else [normals[:, :, 0, 0], normals[:, :, 1, 0]]
        for z in zs:
            assert z.shape == uc.shape
            # Var(z (u - 1/2)) = 1 * 1/12
            assert abs(np.mean(z * uc)) < 4 * np.sqrt(1 / 12 / z.size)
            assert abs(np.mean(z * z * uc)) < 4 * np.sqrt(3 / 12 / z.size)


def test_host_rows_are_checked_against_the_dataset():
    rows = device_data._host_rows([0, 4, 2], 5)
    assert rows.dtype == np.int32 and rows.tolist() == [0, 4, 2]
    assert device_data._host_rows(np.arange(3, dtype=np.uint8), 3).tolist() == [0, 1, 2]
    for bad in (-1, 5, 2 ** 31, 2 ** 32 + 1, -2 ** 40):
        with pytest.raises(ValueError, match='outside'):
            device_data._host_rows([1, bad], 5)
    for bad in ([1, 2.7], [2.0], np.array([1.0]), [1, 2 ** 63], [2 ** 70], [True], ['1']):
        with pytest.raises(ValueError, match='integers'):       # nothing truncated or wrapped
            device_data._host_rows(bad, 5)
    assert device_data._host_rows([], 5).size == 0


def test_host_collate_of_a_batch_without_observations():
    """The device collate is checked against the host collate on such batches too."""
    paths, observed, nb_obs, hp = data_utils.create_dataset(
        'BlackScholes', dict(data_utils.hyperparam_default, nb_paths=4, nb_steps=6, S0=[1.0, 1.0]), seed=3)
    observed[:] = 0
    for funcs, width in (((), 2), ((np.exp, lambda a: a ** 2), 6)):
        b = data_utils.collate_arrays(paths, observed, observed[:, 1:].sum(1), hp['dt'], funcs)
        assert tuple(b['X'].shape) == (0, width) and tuple(b['start_X'].shape) == (4, width)
        assert len(b['times']) == 0 and b['time_ptr'].tolist() == [0] and len(b['obs_idx']) == 0
