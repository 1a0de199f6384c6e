"""The analytic conditional expectation and the evaluation metrics on the GPU
(``device_data.cond_exp``, ``NJODE.evaluate_device``, ``train(device_eval=True)``; C ABI
``njode_cond_exp_f64``) against the host walk ``stock_model.compute_cond_exp``.

The host oracle is fed **float64 copies** of the batch's fp32 arrays, so the comparison does not
hang on numpy's scalar-promotion rules; the device widens the same fp32 values exactly.

What is held to what (eps = 2**-52, one ulp relative):

* **Step-local.**  For consecutive rows of a path that are not separated by the path's own jump,
  the host's one-step formula ``next_cond_exp`` on the DEVICE's previous value must give the
  device's next value within ``STEP_C * eps * (|y| + |mean|)`` (``mean`` = 0 for Black-Scholes
  and Heston), ``STEP_C = 7``; across a jump row that does not observe the path the value must be
  untouched bit for bit.  Derivation, from the loosest stated bounds of the two libraries (host
  libm / numpy: ``exp`` and ``sin`` within 1 ulp; device: the OpenCL full-profile bounds the ROCm
  device library states, ``exp`` within 3 ulp, ``sin`` within 4 ulp) and with
  ``|rate| * delta_t <= 0.025`` (asserted for every case; rate = drift or speed):

  - ``pc = 1 + sin(coeff * t)``: the two ``sin`` differ by at most (4 + 1) eps absolute (values
    <= 1), the addition re-rounds a value <= 2 on both sides: 7 eps absolute.
  - ``arg = (rate * pc) * step``: 0.025 * 7 eps from ``pc`` plus two re-rounded products on
    both sides of a value <= 0.05 (4 * eps / 2 * 0.05): <= 0.275 eps absolute.
  - ``a = exp(arg)``: (3 + 1) eps from the two ``exp`` and 0.275 eps from the argument:
    4.275 eps relative.
  - Black-Scholes / Heston ``y * a``: 4.275 eps plus the re-rounded product (1 eps), times
    ``a <= exp(0.05)``: 5.6 eps ``|y|``.
  - Ornstein-Uhlenbeck ``y * a + mean * (1 - a)`` (0 < a <= 1): ``y * a`` 5.275 eps ``|y|``;
    ``1 - a`` 4.275 eps absolute plus its rounding, times ``|mean|``, re-rounded: <= 5.275 eps
    ``|mean|`` plus one eps for the product; the final sum one eps of ``|y a| + |c|``:
    <= 6.3 eps ``(|y| + |mean|)``.

  Both are below ``STEP_C = 7``.  The bound is derived, not fitted; the largest observed error /
  allowance is printed per case and recorded in DESIGN section 4e.
* **Across a jump**: the observed entries equal ``float64(X[r])`` and the others are untouched,
  bit for bit.
* **Whole trajectories**: relative error <= ``8 eps (steps since the path's last reset + 1)``.
* **Optimal loss**: host ``get_optimal_loss`` at weight 0.5 and 0.8, rel 1e-12; the goldens'
  ``optimal_loss`` of ``g3_ckpt_*``, rel 1e-9 (``tests/test_oracle_golden.py``'s bound).
* **Fused metric**: ``sq_diff / N`` against numpy's mean on the materialised device path within
  ``(N - 1) eps`` relative (non-negative terms: the bound of any summation order);
  ``evaluate_device`` against the goldens' ``msd_cond_exp`` (rel 1e-3, the host route's bound in
  ``tests/test_hip_parity.py``) and against ``evaluate`` (rel 1e-9).
* **Reproducibility**: two calls bit-equal; metric-only and path + metric calls give the same
  ``sq_diff`` bit for bit.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from golden_util import Golden
from hip_util import bs_batch, hip_model, to_dev
from njode_amd import _lib, data_utils, device_data, schedule, stock_model, train

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
STEP_C = 7.0          # derived in the module docstring; the issue caps it at 16
MODELS = ('BlackScholes', 'OrnsteinUhlenbeck', 'Heston')
SINE = 2 * np.pi


# ---- batches ---------------------------------------------------------------------------------
def _hp(name, dim, sine, B, nb_steps=100, obs_perc=0.1):
    hp = copy.deepcopy(data_utils.hyperparam_default)
    hp.update(nb_paths=B, nb_steps=nb_steps, S0=[1.0] * dim if dim > 1 else 1, obs_perc=obs_perc)
    if sine:
        hp['sine_coeff'] = SINE
    return hp


def _reshape(b, drop_path=None, cut_after=None):
    """host batch (numpy / torch fields) without the rows of ``drop_path`` (its n_obs_ot becomes 0;
    slices it leaves empty stay) and without the times beyond ``cut_after`` (leaves a tail)"""
    times = np.asarray(b['times'], dtype=np.float64)
    ptr = np.asarray(b['time_ptr'], dtype=np.int64)
    idx = b['obs_idx'].numpy()
    slice_of = np.repeat(np.arange(len(times)), np.diff(ptr))
    keep = np.ones(len(idx), dtype=bool)
    if drop_path is not None:
        keep &= idx != drop_path
    nt = len(times) if cut_after is None else int(np.searchsorted(times, cut_after, side='right'))
    keep &= slice_of < nt
    counts = np.bincount(slice_of[keep], minlength=len(times))[:nt]
    B = b['start_X'].shape[0]
    kt = torch.from_numpy(keep)
    return {'times': times[:nt], 'time_ptr': np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
            'X': b['X'][kt], 'obs_idx': b['obs_idx'][kt], 'start_X': b['start_X'],
            'n_obs_ot': torch.from_numpy(np.bincount(idx[keep], minlength=B).astype(np.int64))}


def make_case(name, dim, sine, B, seed=0):
    """(batch, delta_t, T, stock model).  B = 1 and 63 (observed 3 % of the time): times skip grid
    points; B = 1 / 257: the schedule has a tail (the times beyond 0.9 are cut); B >= 63: path 1
    has no observation; B = 63: delta_t does not divide the grid, so every interval ends in a
    partial step."""
    hp = _hp(name, dim, sine, B, obs_perc=0.03 if B == 63 else 0.1)
    paths, obs, nb_obs, meta = data_utils.create_dataset(name, hp, seed=seed)
    b = data_utils.collate_arrays(paths, obs, nb_obs, meta['dt'])
    b = _reshape(b, drop_path=1 if B >= 63 else None, cut_after=0.9 if B in (1, 257) else None)
    delta_t = 0.37 * meta['dt'] if B == 63 else meta['dt']
    sm = stock_model.STOCK_MODELS[name](**meta)
    return b, delta_t, meta['maturity'], sm


def host_oracle(sm, b, delta_t, T, weight=0.5):
    """compute_cond_exp on float64 copies of the fp32 arrays"""
    return sm.compute_cond_exp(
        b['times'], b['time_ptr'], b['X'].numpy().astype(np.float64), b['obs_idx'].numpy(), delta_t, T,
        b['start_X'].numpy().astype(np.float64), b['n_obs_ot'].numpy(), return_path=True, get_loss=True,
        weight=weight)


def dev_call(sm, b, delta_t, T, **kw):
    d = to_dev(b)
    return device_data.cond_exp(sm, d['times'], d['time_ptr'], d['X'], d['obs_idx'], delta_t, T,
                                d['start_X'], n_obs_ot=d['n_obs_ot'], **kw)


def _rows(b, delta_t, T):
    """per row: ('step', k) or ('jump', i), and the [n_t, B] mask of paths observed at a jump row"""
    c = schedule.cond_exp_clock(b['times'], delta_t, T)
    kind = [None] * (1 + c.n_steps + c.n_times)
    kind[0] = ('start', 0)
    jrow = {int(r): i for i, r in enumerate(c.row_of_jump)}
    k = 0
    for r in range(1, len(kind)):
        if r in jrow:
            kind[r] = ('jump', jrow[r])
        else:
            kind[r] = ('step', k)
            k += 1
    B = b['start_X'].shape[0]
    seen = np.zeros((len(kind), B), dtype=bool)
    idx, ptr = b['obs_idx'].numpy(), b['time_ptr']
    for r, i in jrow.items():
        seen[r, idx[ptr[i]:ptr[i + 1]]] = True
    return c, kind, seen


# ---- the matrix ------------------------------------------------------------------------------
CASES = [(m, d, s, B) for m in MODELS for d in (1, 3) for s in (False, True) for B in (1, 63, 257, 4000)]


@pytest.mark.parametrize('name,dim,sine,B', CASES)
def test_against_host_walk(name, dim, sine, B):
    b, delta_t, T, sm = make_case(name, dim, sine, B)
    rate = sm.speed if name == 'OrnsteinUhlenbeck' else sm.drift
    mean = float(sm.mean) if name == 'OrnsteinUhlenbeck' else 0.0
    assert abs(rate) * delta_t <= 0.025            # the derivation's premise
    c, kind, seen = _rows(b, delta_t, T)
    n_t = len(kind)
    if B >= 63:
        assert b['n_obs_ot'][1] == 0 and not seen[:, 1].any()
    if B in (1, 257):
        assert c.k_jump[-1] < c.n_steps if c.n_times else c.n_steps > 0       # a tail
    if B == 4000:
        assert c.k_jump[-1] == c.n_steps and c.n_times == 100                # none, every grid time
    if B in (1, 63):
        assert c.n_times < 100                                               # grid points skipped
    if B == 63:
        assert np.any(c.step_dt < delta_t * (1 - 1e-9))                      # partial steps

    rng = np.random.RandomState(7)
    loss_h, path_t_h, path_h = host_oracle(sm, b, delta_t, T, 0.5)
    pred = torch.from_numpy((path_h * (1 + 0.05 * rng.standard_normal(path_h.shape))).astype(np.float32))
    path_t, path_d, loss_d, sq_d = dev_call(sm, b, delta_t, T, want_path=True, want_loss=True,
                                            pred=pred.cuda(), weight=0.5)
    assert np.array_equal(path_t, path_t_h)
    assert path_d.dtype == torch.float64 and tuple(path_d.shape) == (n_t, B, dim) == path_h.shape
    assert loss_d.dtype == sq_d.dtype == torch.float64 and loss_d.dim() == sq_d.dim() == 0
    y = path_d.cpu().numpy()
    X64 = b['X'].numpy().astype(np.float64)
    idx, ptr = b['obs_idx'].numpy(), b['time_ptr']

    # start row, step-local check, jumps
    assert np.array_equal(y[0], b['start_X'].numpy().astype(np.float64))
    worst = 0.0
    since = np.zeros(B)                 # Euler steps since the path's last reset
    for r in range(1, n_t):
        what, i = kind[r]
        if what == 'step':
            want = sm.next_cond_exp(y[r - 1], c.step_dt[i], c.step_t[i])
            allow = STEP_C * EPS * (np.abs(y[r - 1]) + abs(mean))
            err = np.abs(y[r] - want)
            worst = max(worst, float((err / allow).max()))
            assert (err <= allow).all(), (r, float((err / allow).max()))
            since += 1
        else:
            rows = np.arange(ptr[i], ptr[i + 1])
            assert np.array_equal(y[r][idx[rows]], X64[rows]), r           # observed: float64(X[r])
            assert np.array_equal(y[r][~seen[r]], y[r - 1][~seen[r]]), r   # the others: untouched
            since[seen[r]] = 0
        # whole trajectory against the host walk
        bound = 8 * EPS * (since + 1)[:, None] * np.abs(path_h[r])
        assert (np.abs(y[r] - path_h[r]) <= bound).all(), \
            (r, what, float((np.abs(y[r] - path_h[r]) / np.maximum(bound, 1e-300)).max()))
    print('step-local {} dim {} sine {} B {}: largest error / allowance = {:.3f}'.format(name, dim, sine, B, worst))

    # optimal loss
    assert float(loss_d) == pytest.approx(float(loss_h), rel=1e-12)
    loss_h8 = sm.get_optimal_loss(b['times'], b['time_ptr'], X64, idx, delta_t, T,
                                  b['start_X'].numpy().astype(np.float64), b['n_obs_ot'].numpy(), weight=0.8)
    _, _, loss_d8, _ = dev_call(sm, b, delta_t, T, want_loss=True, weight=0.8)
    assert float(loss_d8) == pytest.approx(float(loss_h8), rel=1e-12)
    if int(ptr[-1]) > 0:
        assert float(loss_h8) != float(loss_h) and float(loss_h) > 0

    # fused metric against numpy on the materialised device path
    N = y.size
    ref = np.mean((pred.numpy().astype(np.float64) - y) ** 2)
    assert ref > 0
    assert abs(float(sq_d) / N - ref) <= (N - 1) * EPS * ref, (float(sq_d) / N, ref)

    # reproducibility
    _, path_2, loss_2, sq_2 = dev_call(sm, b, delta_t, T, want_path=True, want_loss=True, pred=pred.cuda(),
                                       weight=0.5)
    assert torch.equal(path_2, path_d) and torch.equal(loss_2, loss_d) and torch.equal(sq_2, sq_d)
    _, none_p, none_l, sq_3 = dev_call(sm, b, delta_t, T, pred=pred.cuda())
    assert none_p is None and none_l is None and torch.equal(sq_3, sq_d)
    _, none_p, loss_3, sq_4 = dev_call(sm, b, delta_t, T, pred=pred.cuda(), want_loss=True)
    assert none_p is None and torch.equal(sq_4, sq_d) and torch.equal(loss_3, loss_d)
    _, path_5, none_l, none_s = dev_call(sm, b, delta_t, T, want_path=True)
    assert none_l is None and none_s is None and torch.equal(path_5, path_d)


def test_no_observation_at_all_and_dict_metadata():
    """a batch without rows: the walk to T alone, loss 0; the model given as its metadata dict"""
    hp = _hp('OrnsteinUhlenbeck', 2, True, 5)
    paths, obs, nb_obs, meta = data_utils.create_dataset('OrnsteinUhlenbeck', hp, seed=3)
    b = data_utils.collate_arrays(paths, obs * 0, nb_obs * 0, meta['dt'])
    assert len(b['times']) == 0 and b['X'].shape[0] == 0
    sm = stock_model.OrnsteinUhlenbeck(**meta)
    loss_h, path_t_h, path_h = host_oracle(sm, b, meta['dt'], 1.0)
    path_t, path_d, loss_d, _ = dev_call(meta, b, meta['dt'], 1.0, want_path=True, want_loss=True)
    assert np.array_equal(path_t, path_t_h) and float(loss_d) == 0.0 == float(loss_h)
    np.testing.assert_allclose(path_d.cpu().numpy(), path_h, rtol=8 * EPS * 101, atol=0)


# ---- goldens and the model ---------------------------------------------------------------------
@pytest.mark.parametrize('tag,name', [('BS', 'BlackScholes'), ('Heston', 'Heston'), ('OU', 'OrnsteinUhlenbeck')])
def test_shipped_checkpoints(tag, name):
    g = Golden('g3_ckpt_' + tag)
    b, meta = bs_batch(200, name=name)
    sm = stock_model.STOCK_MODELS[name](**meta)
    w = float(g['ckpt_weight'])
    _, _, opt, _ = dev_call(sm, b, meta['dt'], meta['maturity'], want_loss=True, weight=w)
    assert float(opt) == pytest.approx(float(g['optimal_loss']), rel=1e-9)
    d = to_dev(b)
    args = (d['times'], d['time_ptr'], d['X'], d['obs_idx'], meta['dt'], meta['maturity'], d['start_X'])
    for device_outputs in (True, False):
        m = hip_model(g.cfg, g.state_dict(), device_outputs=device_outputs).eval()
        m.weight = w
        msd_dev = m.evaluate_device(*args, sm)
        if device_outputs:
            assert torch.is_tensor(msd_dev) and msd_dev.is_cuda and msd_dev.dtype == torch.float64 \
                and msd_dev.dim() == 0
        else:
            assert isinstance(msd_dev, float)
        msd_host = m.evaluate(*args, d['n_obs_ot'], sm)
        print('{}: msd device {:.12e} host {:.12e} golden {:.12e}'.format(tag, float(msd_dev), float(msd_host),
                                                                          float(g['msd_cond_exp'])))
        assert float(msd_dev) == pytest.approx(float(g['msd_cond_exp']), rel=1e-3)
        assert float(msd_dev) == pytest.approx(float(msd_host), rel=1e-9)
    # the reference's 5-tuple, device tensors
    m = hip_model(g.cfg, g.state_dict()).eval()
    msd, path_t, true_t, path_y, true_y = m.evaluate_device(*args, meta, return_paths=True)
    msd_h, path_t_h, true_t_h, path_y_h, true_y_h = m.evaluate(*args, d['n_obs_ot'], sm, return_paths=True)
    assert np.array_equal(path_t, path_t_h) and np.array_equal(true_t, true_t_h)
    assert path_y.is_cuda and true_y.is_cuda and true_y.dtype == torch.float64
    assert torch.equal(path_y, path_y_h)
    np.testing.assert_allclose(true_y.cpu().numpy(), true_y_h, rtol=8 * EPS * 101, atol=0)
    assert float(msd) == pytest.approx(float(msd_h), rel=1e-9)
    with pytest.raises(ValueError):                       # lifted inputs: no analytic truth
        m2 = hip_model(dict(g.cfg, input_size=2, output_size=2), None).eval()
        m2.evaluate_device(d['times'], d['time_ptr'], torch.cat([d['X'], d['X'] ** 2], 1), d['obs_idx'],
                           meta['dt'], meta['maturity'], torch.cat([d['start_X'], d['start_X'] ** 2], 1), sm)


# ---- end to end ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dim,sine', [('BlackScholes', 2, True), ('OrnsteinUhlenbeck', 3, False),
                                           ('Heston', 1, True)])
def test_generate_collate_cond_exp(name, dim, sine):
    """a dataset made on the GPU against its analytic truth, without to_arrays(): equal to the
    route through the host copy and the host oracle"""
    hp = dict(_hp(name, dim, sine, 300), obs_perc=0.1)
    ds = device_data.DeviceDataset.generate(name, hp, seed=11)
    idx = np.arange(300)[::-1][:257].copy()
    d = ds.collate(idx)
    T = ds.metadata['maturity']
    path_t, path_d, loss_d, _ = device_data.cond_exp(
        ds.metadata, d['times'], d['time_ptr'], d['X'], d['obs_idx'], ds.metadata['dt'], T, d['start_X'],
        n_obs_ot=d['n_obs_ot'], want_path=True, want_loss=True)
    paths, obs, nb_obs = ds.to_arrays()
    b = data_utils.collate_arrays(paths[idx], obs[idx], nb_obs[idx], ds.metadata['dt'])
    sm = stock_model.STOCK_MODELS[name](**ds.metadata)
    loss_h, path_t_h, path_h = host_oracle(sm, b, ds.metadata['dt'], T)
    assert np.array_equal(path_t, path_t_h)
    assert float(loss_d) == pytest.approx(float(loss_h), rel=1e-12)
    c, kind, seen = _rows(b, ds.metadata['dt'], T)
    since, y = np.zeros(257), path_d.cpu().numpy()
    for r in range(1, len(kind)):
        if kind[r][0] == 'step':
            since += 1
        else:
            since[seen[r]] = 0
        assert (np.abs(y[r] - path_h[r]) <= 8 * EPS * (since + 1)[:, None] * np.abs(path_h[r])).all(), r


def test_train_device_eval_rows():
    hp = copy.deepcopy(data_utils.hyperparam_default)
    hp['nb_paths'] = 400
    paths, obs, nb_obs, meta = data_utils.create_dataset('OrnsteinUhlenbeck', hp, seed=0)
    kw = dict(epochs=2, batch_size=80, dropout_rate=0.1, evaluate=True, log=lambda s: None)
    m1, met1 = train.train((paths, obs, nb_obs), meta, **kw)
    m2, met2 = train.train((paths, obs, nb_obs), meta, device_eval=True, **kw)
    assert torch.equal(m1.flat_parameters(), m2.flat_parameters())
    assert len(met1) == len(met2) == 2
    for r1, r2 in zip(met1, met2):
        assert len(r1) == len(r2) == len(train.METR_COLUMNS) + 1
        assert r1[0] == r2[0] and r1[3] == r2[3] and r1[4] == r2[4]            # epoch, the loss columns
        assert isinstance(r2[5], float) and isinstance(r2[6], float)
        assert r2[5] == pytest.approx(r1[5], rel=1e-9)                          # optimal_eval_loss
        assert r2[6] == pytest.approx(float(r1[6]), rel=1e-9)                   # evaluation_mean_diff
    with pytest.raises(ValueError):
        train.train((paths, obs, nb_obs), meta, device_eval=True, func_appl_X=['power-2'], **kw)


# ---- C level ---------------------------------------------------------------------------------------
def test_c_level_refusals():
    L = _lib.lib()
    B, dim, n_obs, K, nt = 4, 1, 3, 10, 2
    dev = torch.device('cuda')
    start_X = torch.ones(B, dim, device=dev)
    X = torch.ones(n_obs, dim, device=dev)
    obs_idx = torch.tensor([0, 2, 1], dtype=torch.int32, device=dev)
    n_obs_ot = torch.tensor([1, 1, 1, 0], dtype=torch.int32, device=dev)
    pred = torch.zeros(1 + K + nt, B, dim, device=dev)
    out = torch.full(((1 + K + nt) * B * dim + 2,), -7.0, dtype=torch.float64, device=dev)
    step_dt = np.full(K, 0.1)
    step_t = np.arange(K) * 0.1
    k_jump = np.array([3, 7], dtype=np.int32)
    time_ptr = np.array([0, 2, 3], dtype=np.int32)
    need = ctypes.c_size_t(0)
    assert L.njode_cond_exp_bytes(B, n_obs, nt, K, dim, ctypes.byref(need)) == 0
    ws = torch.full((need.value,), 0xA5, dtype=torch.uint8, device=dev)
    p = lambda a: a.ctypes.data
    path_p, loss_p, sq_p = out.data_ptr(), out.data_ptr() + 8 * (out.numel() - 2), out.data_ptr() + 8 * (out.numel() - 1)

    def call(sde_kw=None, batch_kw=None, sched_kw=None, null=(), pred_p=pred.data_ptr(), outs=None, ws_p=None,
             ws_bytes=None, weight=0.5):
        sde = _lib.NjodeSde(model=0, dim=dim, drift=2.0, mean=4.0, speed=2.0)
        for k, v in (sde_kw or {}).items():
            setattr(sde, k, v)
        bk = dict(batch_size=B, n_obs=n_obs, start_X=start_X.data_ptr(), X=X.data_ptr(), M=None,
                  obs_idx=obs_idx.data_ptr(), n_obs_ot=n_obs_ot.data_ptr())
        bk.update(batch_kw or {})
        sk = dict(n_steps=K, n_times=nt, step_dt=p(step_dt), step_t=p(step_t), k_jump=p(k_jump),
                  time_ptr=p(time_ptr))
        sk.update(sched_kw or {})
        batch, sched = _lib.NjodeBatch(**bk), _lib.NjodeCondExpSchedule(**sk)
        o = (path_p, loss_p, sq_p) if outs is None else outs
        return L.njode_cond_exp_f64(
            None if 'sde' in null else ctypes.byref(sde), None if 'batch' in null else ctypes.byref(batch),
            None if 'sched' in null else ctypes.byref(sched), weight, pred_p, o[0], o[1], o[2],
            ws.data_ptr() if ws_p is None else ws_p, need.value if ws_bytes is None else ws_bytes,
            torch.cuda.current_stream().cuda_stream)

    refusals = {
        'null sde': dict(null=('sde',)), 'null batch': dict(null=('batch',)), 'null sched': dict(null=('sched',)),
        'null start_X': dict(batch_kw=dict(start_X=None)), 'null X': dict(batch_kw=dict(X=None)),
        'null obs_idx': dict(batch_kw=dict(obs_idx=None)), 'null step_dt': dict(sched_kw=dict(step_dt=None)),
        'null step_t': dict(sched_kw=dict(step_t=None)), 'null k_jump': dict(sched_kw=dict(k_jump=None)),
        'null time_ptr': dict(sched_kw=dict(time_ptr=None)), 'null ws': dict(ws_p=0),
        'B = 0': dict(batch_kw=dict(batch_size=0)), 'B < 0': dict(batch_kw=dict(batch_size=-1)),
        'n_obs < 0': dict(batch_kw=dict(n_obs=-1)), 'dim = 0': dict(sde_kw=dict(dim=0)),
        'K < 0': dict(sched_kw=dict(n_steps=-1)), 'nt < 0': dict(sched_kw=dict(n_times=-1)),
        'no output': dict(outs=(None, None, None)), 'sq_diff without pred': dict(pred_p=None),
        'opt_loss without n_obs_ot': dict(batch_kw=dict(n_obs_ot=None)),
        'mask': dict(batch_kw=dict(M=X.data_ptr())), 'unknown model': dict(sde_kw=dict(model=3)),
        'negative model': dict(sde_kw=dict(model=-1)),
        'time_ptr of another batch': dict(batch_kw=dict(n_obs=2)),
        'k_jump beyond the steps': dict(sched_kw=dict(n_steps=5)),
    }
    torch.cuda.synchronize()
    _lib.profile_enable(1)
    _lib.profile_read()
    try:
        for what, kw in refusals.items():
            assert call(**kw) == _lib.E_BADARG, what
            assert L.njode_last_error(), what
        assert call(ws_bytes=need.value - 1) == _lib.E_WORKSPACE
        torch.cuda.synchronize()
        assert _lib.profile_read() == {}                      # nothing was launched ...
        assert bool((out == -7.0).all())                      # ... and nothing written
        assert bool((ws == 0xA5).all())                       # ... not even to the workspace
        # the same arguments without a reason to refuse run
        assert call() == 0
        torch.cuda.synchronize()
        assert list(_lib.profile_read()) == ['k_cond_exp_walk']
    finally:
        _lib.profile_enable(0)
    assert bool((out != -7.0).all())
    sm = stock_model.BlackScholes(drift=2.0, volatility=0.3, nb_paths=B, nb_steps=10, S0=1, maturity=1.0)
    want = np.ones((B, 1))
    rows, k, i = [want], 0, 0
    for r in range(1, 1 + K + nt):
        if i < nt and k == k_jump[i]:
            i += 1            # every X is 1 and so is the path only at the start: a real reset
            want = want.copy()
            want[obs_idx.cpu().numpy()[time_ptr[i - 1]:time_ptr[i]]] = 1.0
        else:
            want = sm.next_cond_exp(want, step_dt[k], step_t[k])
            k += 1
        rows.append(want)
    np.testing.assert_allclose(out[:-2].cpu().numpy().reshape(1 + K + nt, B, dim), np.array(rows), rtol=1e-13)
