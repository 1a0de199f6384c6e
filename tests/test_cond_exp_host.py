"""Host side of the analytic conditional expectation on the GPU (no GPU needed): the float64
clock ``schedule.cond_exp_clock`` against the host walk ``stock_model.compute_cond_exp``, the
refusals of ``device_data.cond_exp`` (all raised before the library is touched), and the
declaration / export of the new C ABI entries."""
import os
import re

import numpy as np
import pytest
import torch

from njode_amd import _lib, build, device_data, schedule, stock_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid_clock(n, dt):
    """the collate's grid times: a float64 running sum, not k * dt"""
    return np.cumsum(np.full(n, dt, dtype=np.float64))


def _clock_cases():
    dt = 0.01
    grid = _grid_clock(100, dt)
    cases = {
        'regular, every grid time, no tail': (grid, dt, 1.0),
        'regular, sparse, no tail': (grid[[2, 3, 17, 50, 99]], dt, 1.0),
        'regular, tail to T': (grid[[0, 9, 10, 42]], dt, 1.0),
        'skipped grid points, tail': (grid[[4, 30, 31, 80]], dt, 1.0),
        'no observation at all': (np.zeros(0), dt, 1.0),
        'off-grid delta_t (partial steps)': (grid[[1, 5, 6, 33, 99]], 0.37 * dt, 1.0),
        'off-grid times': (np.array([0.0031, 0.0312345, 0.5, 0.50000001, 0.777]), dt, 1.0),
        'off-grid times and delta_t, tail': (np.array([0.013, 0.2, 0.61]), 0.013, 0.9),
        'delta_t larger than every gap': (np.array([0.1, 0.25, 0.3]), 0.5, 1.0),
        'T = 1 + 1e-12': (grid[[3, 50, 99]], dt, 1.0 + 1e-12),
        'T = 1 + 1e-12, tail': (grid[[3, 50]], dt, 1.0 + 1e-12),
        'last time within 1e-10 beyond T': (np.array([0.5, 1.0 + 5e-11]), dt, 1.0),
        'T = 0.5 on a coarse grid': (_grid_clock(7, 1.0 / 14)[[0, 3, 6]], 1.0 / 14, 0.5),
    }
    return cases


def _host_walk(times, delta_t, T):
    """``compute_cond_exp`` of a one-path Black-Scholes model observed at every time"""
    n = len(times)
    sm = stock_model.BlackScholes(drift=2., volatility=0.3, nb_paths=1, nb_steps=100, S0=1, maturity=T)
    _, path_t, path_y = sm.compute_cond_exp(
        times, np.arange(n + 1), np.ones((n, 1)), np.zeros(n, dtype=np.int64), delta_t, T,
        np.ones((1, 1)), np.ones(1, dtype=np.int64))
    return path_t, path_y


@pytest.mark.parametrize('name', sorted(_clock_cases()))
def test_clock_reproduces_host_path_t(name):
    times, delta_t, T = _clock_cases()[name]
    path_t, path_y = _host_walk(times, delta_t, T)
    c = schedule.cond_exp_clock(times, delta_t, T)
    assert c.path_t.dtype == np.float64 and c.step_dt.dtype == np.float64 and c.step_t.dtype == np.float64
    assert c.k_jump.dtype == np.int32
    assert np.array_equal(c.path_t, path_t), name
    assert len(path_y) == 1 + c.n_steps + c.n_times == len(c.path_t)
    assert c.n_times == len(times) and c.n_steps == len(c.step_dt) == len(c.step_t)
    # the rows: a jump row repeats the observation time, a step row is clock + step
    rows_of_jump = 1 + c.k_jump + np.arange(c.n_times)
    assert np.array_equal(rows_of_jump, c.row_of_jump)
    assert np.array_equal(c.path_t[rows_of_jump], np.asarray(times, dtype=np.float64))
    step_rows = np.setdiff1d(np.arange(1, len(c.path_t)), rows_of_jump)
    assert np.array_equal(c.path_t[step_rows], c.step_t + c.step_dt)
    # (a partial step is target - clock with clock >= fl(target - delta_t): delta_t plus roundings
    # of the size of the clock's spacing)
    assert np.all(c.step_dt > 0) and np.all(c.step_dt <= delta_t + 4 * np.spacing(T + 1.0))
    # it is the model's clock before the fp32 rounding
    s = schedule.Schedule(times, delta_t, T, True)
    assert np.array_equal(s.path_t, c.path_t) and np.array_equal(s.k_jump, c.k_jump)
    assert np.array_equal(s.step_dt, c.step_dt.astype(np.float32))
    assert np.array_equal(s.step_t, c.step_t.astype(np.float32))


def test_clock_covers_partial_steps_and_tails():
    """the cases above contain what they are named for"""
    cases = _clock_cases()
    c = schedule.cond_exp_clock(*cases['off-grid delta_t (partial steps)'])
    assert np.any(c.step_dt < 0.37 * 0.01 * (1 - 1e-9))
    c = schedule.cond_exp_clock(*cases['regular, tail to T'])
    assert c.k_jump[-1] < c.n_steps
    c = schedule.cond_exp_clock(*cases['regular, every grid time, no tail'])
    assert c.k_jump[-1] == c.n_steps == 100
    c = schedule.cond_exp_clock(*cases['skipped grid points, tail'])
    assert np.any(np.diff(c.k_jump) > 1)


@pytest.mark.parametrize('times,T', [
    ([0.1, 0.1, 0.2], 1.0),            # not strictly increasing
    ([0.2, 0.1], 1.0),
    ([0.0, 0.1], 1.0),                 # the host walk skips t = 0
    ([-0.1, 0.1], 1.0),
    ([0.5, 1.0 + 2e-10], 1.0),         # the host walk stops there
    ([0.5, float('nan')], 1.0),
    ([0.5, float('inf')], 1.0),
])
def test_clock_refuses_what_the_host_walk_skips(times, T):
    with pytest.raises(ValueError):
        schedule.cond_exp_clock(np.asarray(times), 0.01, T)


def _batch(d=1, B=3):
    times = np.array([0.1, 0.2])
    return dict(times=times, time_ptr=np.array([0, 2, 3]), X=torch.ones(3, d),
                obs_idx=torch.tensor([0, 2, 1]), delta_t=0.01, T=1.0, start_X=torch.ones(B, d))


def _sm(d=1):
    return stock_model.BlackScholes(drift=2., volatility=0.3, nb_paths=3, nb_steps=100,
                                    S0=[1.] * d if d > 1 else 1, maturity=1.)


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError('the library was touched before the refusal')
    monkeypatch.setattr(_lib, 'lib', boom)


@pytest.mark.parametrize('what', ['not increasing', 'zero time', 'beyond T', 'lifted', 'mask', 'start_time',
                                  'nothing asked', 'loss without n_obs_ot', 'time_ptr', 'pred shape',
                                  'unknown model'])
def test_refusals_before_the_library(what, no_library):
    b, kw, sm = _batch(), dict(want_path=True), _sm()
    if what == 'not increasing':
        b['times'] = np.array([0.2, 0.2])
    elif what == 'zero time':
        b['times'] = np.array([0.0, 0.2])
    elif what == 'beyond T':
        b['times'] = np.array([0.1, 1.0 + 1e-9])
    elif what == 'lifted':                      # func_appl_X = ['power-2']: twice the model's width
        b = _batch(d=2)
    elif what == 'mask':
        kw['M'] = torch.ones(3, 1)
    elif what == 'start_time':
        kw['start_time'] = 0.05
    elif what == 'nothing asked':
        kw = {}
    elif what == 'loss without n_obs_ot':
        kw = dict(want_loss=True)
    elif what == 'time_ptr':
        b['time_ptr'] = np.array([0, 2, 4])
    elif what == 'pred shape':
        kw = dict(pred=torch.zeros(5, 3, 1))
    elif what == 'unknown model':
        sm = {'model_name': 'FractionalBM', 'S0': 1}
    with pytest.raises(ValueError):
        device_data.cond_exp(sm, b['times'], b['time_ptr'], b['X'], b['obs_idx'], b['delta_t'], b['T'],
                             b['start_X'], **kw)


def test_valid_call_reaches_the_device_check(no_library):
    """the same batch without a reason to refuse gets past every check (and, on the host, stops
    at the device check: there is no CPU route)"""
    b = _batch()
    with pytest.raises(RuntimeError, match='GPU only'):
        device_data.cond_exp(_sm(), b['times'], b['time_ptr'], b['X'], b['obs_idx'], b['delta_t'], b['T'],
                             b['start_X'], want_path=True)


def test_sde_mapping_is_shared():
    """a stock_model object and its metadata dict give the same NjodeSde; sine_coeff is kept"""
    hp = dict(drift=2., volatility=0.3, mean=4, speed=2., correlation=0.5, nb_paths=7, nb_steps=100,
              S0=[1., 1.], maturity=1., sine_coeff=6.283)
    for name in ('BlackScholes', 'OrnsteinUhlenbeck', 'Heston'):
        sm = stock_model.STOCK_MODELS[name](**hp)
        assert sm.sine_coeff == 6.283
        a = device_data._sde_of(sm, 2)
        b = device_data._sde_of(dict(hp, model_name=name), 2)
        c = device_data._sde_of(dict(hp, model_name='sine_' + name), 2)
        # what the walk reads (an object keeps only its own model's hyper-parameters)
        read = ('model', 'dim', 'has_sine', 'sine_coeff') + (
            ('mean', 'speed') if name == 'OrnsteinUhlenbeck' else ('drift',))
        for f in read:
            assert getattr(a, f) == getattr(b, f) == getattr(c, f), (name, f)
        assert (b.mean, b.speed, b.drift, b.sine_coeff) == (4.0, 2.0, 2.0, 6.283)
        assert a.model == _lib.SDE_MODELS[name] and a.dim == 2 and a.has_sine == 1
    assert stock_model.BlackScholes(drift=2., volatility=0.3, nb_paths=1, nb_steps=1, S0=1,
                                    maturity=1.).sine_coeff is None
    assert device_data._sde_of(_sm(), 1).has_sine == 0


def test_symbols_declared_exported_and_built():
    header = open(os.path.join(REPO, 'include', 'njode_producer.h')).read()
    declared = set(re.findall(r'\b(njode_[a-z0-9_]+)\s*\(', header))
    new = {'njode_cond_exp_bytes', 'njode_cond_exp_f64'}
    assert new <= declared and new <= set(_lib.EXPORTS)
    assert 'NjodeCondExpSchedule' in header
    assert [f for f, _ in _lib.NjodeCondExpSchedule._fields_] == ['n_steps', 'n_times', 'step_dt', 'step_t',
                                                                 'k_jump', 'time_ptr']
    src = open(build.__file__).read()
    assert 'njode_condexp.hip' in src and os.path.exists(os.path.join(build.CSRC, 'njode_condexp.hip'))
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        for sym in new:
            assert hasattr(L, sym), sym
        # the size query needs no GPU
        import ctypes
        need = ctypes.c_size_t(0)
        assert L.njode_cond_exp_bytes(4000, 40000, 100, 100, 1, ctypes.byref(need)) == 0
        assert need.value >= 100 * 4000 * 4 + 40000 * 8
        assert L.njode_cond_exp_bytes(0, 0, 0, 0, 1, ctypes.byref(need)) == _lib.E_BADARG
        assert L.njode_cond_exp_bytes(4, -1, 0, 0, 1, ctypes.byref(need)) == _lib.E_BADARG
        assert L.njode_cond_exp_bytes(4, 0, 0, 0, 1, None) == _lib.E_BADARG
