"""
GPU-resident datasets and the device-side collate (C ABI: include/njode_producer.h).

Host-side mirror of the reference's batch producer -- ``data_utils.create_dataset``
(``data_utils.py:56-105``: SDE paths + observation mask) and ``custom_collate_fn`` /
``CustomCollateFnGen`` (``data_utils.py:278-316, 352-416``) -- for training loops that run at
GPU speed: the dataset lives in HBM in time-major layout (paths f64 ``[S+1, d, N]``, observed
u8 ``[S+1, N]``), a batch is a device index list, and the only thing that crosses PCIe per
batch is the ``S`` per-time observation counts the host needs to lay out the Euler schedule
(``times`` / ``time_ptr`` stay numpy arrays exactly as ``NJODE.forward`` expects them).

No CPU fallback: everything here calls into ``libnjode_hip.so``.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ptr_arg as _ptr, stream_arg as _stream
from .schedule import PinnedRing, cond_exp_clock

_HP_KEYS = ('drift', 'volatility', 'mean', 'speed', 'correlation', 'S0', 'maturity')


def parse_powers(func_names):
    """``func_appl_X`` names -> lift codes of the C ABI (reference ``data_utils.py:319-335``:
    ``power-k`` -> k, ``exp`` -> 0)."""
    out = []
    for name in func_names or ():
        if name in ('exp', 'exponential'):
            out.append(0)
        elif name.startswith('power-') and float(name.split('-')[1]) == int(float(name.split('-')[1])) \
                and int(float(name.split('-')[1])) >= 1:
            out.append(int(float(name.split('-')[1])))
        else:
            raise ValueError('unsupported func_appl_X entry: {}'.format(name))
    if len(out) > 4:
        raise ValueError('at most 4 func_appl_X entries')
    return out


def sde_struct(stock_model_name, hp, dim, models=_lib.SDE_MODELS):
    """``NjodeSde`` of a model name and its hyper-parameter dict (``create_dataset``'s
    ``hyperparam_dict`` / a dataset's metadata); vector-valued entries contribute their first
    component.  ``sine_<Model>`` names the same model (its ``sine_coeff`` is in the dict)."""
    name = stock_model_name[5:] if stock_model_name.startswith('sine_') else stock_model_name
    if name not in models:
        raise ValueError('no analytic model named {!r}'.format(stock_model_name))
    sde = _lib.NjodeSde()
    sde.model = models[name]
    sde.n_paths, sde.dim, sde.n_steps = int(hp.get('nb_paths', 0)), int(dim), int(hp.get('nb_steps', 0))
    sc = hp.get('sine_coeff')
    sde.has_sine, sde.sine_coeff = (0, 0.0) if sc is None else (1, float(sc))
    for k in _HP_KEYS:
        v = hp.get(k)
        setattr(sde, k, float(np.ravel(v)[0]) if v is not None else 0.0)
    return sde


def _sde_of(sde, dim):
    """``NjodeSde`` of a ``stock_model`` object or a metadata dict, for inputs ``dim`` wide."""
    if isinstance(sde, dict):
        if 'model_name' not in sde:
            raise ValueError("a metadata dict needs 'model_name'")
        name, hp = sde['model_name'], sde
        own = int(np.size(sde.get('S0', 1)))      # (StockModel.dimensions)
    else:
        name = type(sde).__name__
        hp = {k: getattr(sde, k, None) for k in _HP_KEYS + ('sine_coeff',)}
        own = int(sde.dimensions)
    if own != dim:
        # (func_appl_X lifts append columns that have no analytic truth: the host route reports nan)
        raise ValueError('inputs are {} wide but the model has {} dimensions (lifted inputs have '
                         'no analytic conditional expectation)'.format(dim, own))
    return sde_struct(name, hp, dim)


def stage_struct(stock_model_name, hp, dim, first_step=0):
    """``NjodeSdeStage`` of the staged entry points: ``sde_struct`` with the fourth model,
    ``return_vol`` and ``v0`` (default: ``mean``, as ``HestonWOFeller``'s constructor)."""
    st = _lib.NjodeSdeStage()
    st.sde = sde_struct(stock_model_name, hp, dim, _lib.SDE_MODELS_STAGED)
    hwf = st.sde.model == _lib.SDE_MODELS_STAGED['HestonWOFeller']
    st.return_vol = int(bool(hp.get('return_vol'))) if hwf else 0
    v0 = hp.get('v0') if hwf else None
    st.v0 = float(np.ravel(v0)[0]) if v0 is not None else st.sde.mean
    st.first_step = int(first_step)
    return st


def _stages_of(sde, dim):
    """What the staged entry point needs of a ``HestonWOFeller`` / ``Combined`` object or their
    metadata: ``(list of NjodeSdeStage without first_step, stage maturities or None)``; None for
    everything ``_sde_of`` describes.  ``ValueError``: inputs of another width (``return_vol``:
    twice the model's dimensions), a combined description without stages, with more than
    ``_lib.MAX_STAGES`` or with a ``return_vol`` stage."""
    if isinstance(sde, dict):
        name, hp = sde.get('model_name'), sde
    else:
        name = type(sde).__name__
        hp = {k: getattr(sde, k, None) for k in _HP_KEYS + ('sine_coeff', 'return_vol', 'v0',
                                                           'stock_model_names', 'hyperparam_dicts')}
    if name in ('combined', 'Combined'):
        names, hps = hp.get('stock_model_names'), hp.get('hyperparam_dicts')
        if not names or hps is None or len(names) != len(hps):
            raise ValueError('a combined description needs stock_model_names and as many hyperparam_dicts')
        if len(names) > _lib.MAX_STAGES:
            raise ValueError('at most {} stages'.format(_lib.MAX_STAGES))
        stages = []
        for n, h in zip(names, hps):
            if h.get('return_vol') and n.endswith('HestonWOFeller'):
                raise ValueError('a return_vol stage cannot be combined: its paths are twice as wide')
            own = int(np.size(h.get('S0', 1)))
            if own != dim:
                raise ValueError('inputs are {} wide but stage {!r} has {} dimensions'.format(dim, n, own))
            stages.append(stage_struct(n, h, dim))
        return stages, [h['maturity'] for h in hps]
    if name in ('HestonWOFeller', 'sine_HestonWOFeller'):
        own = int(np.size(hp.get('S0', 1))) * (2 if hp.get('return_vol') else 1)
        if own != dim:
            raise ValueError('inputs are {} wide but the model stores {} coordinates (lifted inputs '
                             'have no analytic conditional expectation)'.format(dim, own))
        return [stage_struct('HestonWOFeller', hp, dim)], None
    return None


_ring = None


def cond_exp(sde, times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot=None, weight=0.5,
             pred=None, want_path=False, want_loss=False, M=None, start_time=None):
    """``StockModel.compute_cond_exp`` (``start_time=None``) on the GPU: the true conditional
    expectation of ``sde`` (a ``stock_model`` object or a dataset's metadata dict) along the
    batch's schedule, in float64, and the metrics taken against it.  A ``Combined`` object or
    ``'combined'`` metadata walks stage after stage as ``Combined.compute_cond_exp`` does (``T`` is
    then the accumulated sum of the stages' maturities); ``HestonWOFeller`` with ``return_vol``
    takes inputs ``2 d`` wide, the variance in the second half.  Returns
    ``(path_t, path_y, opt_loss, sq_diff)``:

    * ``path_t``  float64 numpy ``[n_t]`` -- the host walk's ``path_t``;
    * ``path_y``  float64 device ``[n_t, B, d]`` with ``want_path``, else None;
    * ``opt_loss`` 0-dim float64 device tensor with ``want_loss`` (needs ``n_obs_ot``): what
      ``get_optimal_loss(..., weight=weight)`` returns, else None;
    * ``sq_diff`` 0-dim float64 device tensor with ``pred`` (fp32 ``[n_t, B, d]``, the model's
      ``path_y`` of a ``return_path=True, until_T=True`` call): the sum of ``(pred - path_y)**2``
      over all entries, taken without storing the path; else None.

    A path has at most one row per time slice (what the collate produces); this is the caller's
    duty and is not checked -- a check would cost a host wait: with a duplicate (slice, path)
    pair it is undefined which row the path takes, and the results are no longer reproducible.

    Tensors stay on the device and nothing here waits for it.  ``ValueError``, before anything
    is launched: ``times`` not strictly increasing within ``(0, T + 1e-10]``, lifted inputs, a
    mask ``M``, a ``start_time``, no output asked for, ``want_loss`` without ``n_obs_ot``."""
    global _ring
    if M is not None:
        raise ValueError('masked batches have no analytic conditional expectation')
    if start_time:
        raise ValueError('start_time is not supported: the walk starts at 0')
    if not (want_path or want_loss or pred is not None):
        raise ValueError('nothing asked for: want_path, want_loss or pred')
    if want_loss and n_obs_ot is None:
        raise ValueError('want_loss needs n_obs_ot')
    if start_X.dim() != 2 or X.dim() != 2 or X.shape[1] != start_X.shape[1]:
        raise ValueError('start_X must be [B, d] and X [n_obs, d]')
    B, dim = int(start_X.shape[0]), int(start_X.shape[1])
    if B == 0:
        raise ValueError('empty batch')
    staged = _stages_of(sde, dim)
    if staged is None:
        cs = _sde_of(sde, dim)
        clock = cond_exp_clock(times, delta_t, T)
    else:
        clock = cond_exp_clock(times, delta_t, T, staged[1])
        if len(clock.stage_first) > 1 and np.any(np.diff(clock.stage_first) <= 0):
            raise ValueError('a stage of the combined model has no Euler step on this clock')
        cs = (_lib.NjodeSdeStage * len(staged[0]))(*staged[0])
        for st, first in zip(cs, clock.stage_first):
            st.first_step = int(first)
    tp = np.ascontiguousarray(time_ptr, dtype=np.int64).reshape(-1)
    n_obs = int(X.shape[0])
    if len(tp) != clock.n_times + 1 or tp[0] != 0 or tp[-1] != n_obs or np.any(np.diff(tp) < 0):
        raise ValueError('time_ptr must have len(times) + 1 non-decreasing entries from 0 to len(X)')
    if obs_idx.numel() != n_obs:
        raise ValueError('obs_idx must have one entry per row of X')
    K, nt = clock.n_steps, clock.n_times
    n_t = 1 + K + nt
    if pred is not None and tuple(pred.shape) != (n_t, B, dim):
        raise ValueError('pred must be [{}, {}, {}], not {}'.format(n_t, B, dim, tuple(pred.shape)))

    dev = start_X.device
    if dev.type != 'cuda':
        raise RuntimeError('device_data.cond_exp runs on the GPU only (inputs are on {}); the host '
                           'route is stock_model.compute_cond_exp'.format(dev))
    L = _lib.lib()
    f32, f64 = torch.float32, torch.float64
    start_X = start_X.to(f32).contiguous()
    X = X.to(device=dev, dtype=f32).contiguous()
    obs_idx = obs_idx.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
    if n_obs_ot is not None:
        n_obs_ot = n_obs_ot.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
        if n_obs_ot.numel() != B:
            raise ValueError('n_obs_ot must have one entry per path')
    if pred is not None:
        pred = pred.to(device=dev, dtype=f32).contiguous()
    # the float64 clock travels through a pinned buffer: [step_dt | step_t | k_jump | time_ptr]
    if _ring is None:
        _ring = PinnedRing()
    slot, pinned = _ring.acquire(16 * K + 4 * (2 * nt + 1))
    buf = pinned.numpy()
    d = buf[:4 * K].view(np.float64)
    d[:K] = clock.step_dt
    d[K:] = clock.step_t
    buf[4 * K:4 * K + nt] = clock.k_jump
    buf[4 * K + nt:4 * K + 2 * nt + 1] = tp
    base = pinned.data_ptr()
    sched = _lib.NjodeCondExpSchedule(K, nt, base, base + 8 * K, base + 16 * K, base + 16 * K + 4 * nt)
    batch = _lib.NjodeBatch(B, n_obs, start_X.data_ptr(), X.data_ptr() if n_obs else None, None,
                            obs_idx.data_ptr() if n_obs else None,
                            n_obs_ot.data_ptr() if n_obs_ot is not None else None, float(B), 0, None)
    need = C.c_size_t(0)
    if staged is None:
        _lib.check(L.njode_cond_exp_bytes(B, n_obs, nt, K, dim, C.byref(need)))
    else:
        _lib.check(L.njode_cond_exp_staged_bytes(B, n_obs, nt, K, dim, len(cs), C.byref(need)))
    ws = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
    path_y = torch.empty((n_t, B, dim), dtype=f64, device=dev) if want_path else None
    # (one allocation for both scalars: a caller that reads both fetches them in one copy)
    scal = torch.empty(2, dtype=f64, device=dev)
    opt_loss = scal[0] if want_loss else None
    sq_diff = scal[1] if pred is not None else None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        try:
            tail = (C.byref(batch), C.byref(sched), float(weight), _ptr(pred), _ptr(path_y),
                    _ptr(opt_loss), _ptr(sq_diff), _ptr(ws), ws.numel(), C.c_void_p(stream.cuda_stream))
            if staged is None:
                _lib.check(L.njode_cond_exp_f64(C.byref(cs), *tail))
            else:
                _lib.check(L.njode_cond_exp_staged_f64(cs, len(cs), *tail))
        finally:
            _ring.release_after(slot, stream)
    return clock.path_t.copy(), path_y, opt_loss, sq_diff


def times_from_counts(counts, dt):
    """``times`` / ``time_ptr`` of ``custom_collate_fn`` from the per-grid-time observation
    counts (index 0 = grid time 1).  The reference accumulates the clock in float64,
    ``current_time += dt`` (``data_utils.py:296``), so t_k is a running sum, not k * dt."""
    counts = np.asarray(counts, dtype=np.int64)
    clock = np.cumsum(np.full(len(counts), dt, dtype=np.float64))
    used = counts > 0
    time_ptr = np.concatenate([[0], np.cumsum(counts[used])]).astype(np.int64)
    return clock[used], time_ptr


def _host_rows(idx, n_paths):
    """Host row indices as a contiguous int32 array; ``ValueError`` for a row outside
    ``[0, n_paths)`` or of a non-integer type -- the collate kernels index the dataset with
    these values unchecked."""
    rows = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx)
    if rows.size and not (np.issubdtype(rows.dtype, np.integer) and rows.dtype != np.uint64):
        # (floats would be truncated silently; a Python int beyond int64 arrives as object / uint64)
        raise ValueError('dataset rows must be integers that fit int64, not {}'.format(rows.dtype))
    rows = rows.astype(np.int64).reshape(-1)
    if rows.size and (rows.min() < 0 or rows.max() >= n_paths):
        bad = rows[(rows < 0) | (rows >= n_paths)][0]
        raise ValueError('dataset row {} outside [0, {})'.format(int(bad), n_paths))
    return np.ascontiguousarray(rows, dtype=np.int32)


class DeviceDataset:
    """Synthetic dataset resident on one GPU."""

    def __init__(self, paths_tm, observed_tm, nb_obs, metadata):
        self.paths_tm = paths_tm          # f64 [S+1, d, N]
        self.observed_tm = observed_tm    # u8  [S+1, N]
        self.nb_obs = nb_obs              # i32 [N]
        self.metadata = dict(metadata)
        self.n_steps = paths_tm.shape[0] - 1
        self.dim = paths_tm.shape[1]
        self.n_paths = paths_tm.shape[2]
        self.device = paths_tm.device
        self._counts_host = torch.empty(self.n_steps, dtype=torch.int32).pin_memory()

    def __len__(self):
        return self.n_paths

    # -- construction --------------------------------------------------------------------
    @classmethod
    def generate(cls, stock_model_name, hyperparam_dict, seed=0, device='cuda',
                 normals=None, uniforms=None):
        """``create_dataset`` on the GPU.  ``normals`` / ``uniforms`` (numpy f64, reference
        draw order) replace the Philox streams -- used to pin the recurrences to the
        reference's numbers."""
        L = _lib.lib()
        hp = dict(hyperparam_dict)
        dev = torch.device(device)
        dim = int(np.size(hp.get('S0', 1)))
        if dim != 1 and np.ptp(np.asarray(hp['S0'], dtype=np.float64)) != 0:
            raise ValueError('S0 must be the same in every dimension')
        for key in ('nb_paths', 'nb_steps'):
            if key not in hp:
                raise KeyError(key)
        if stock_model_name not in _lib.SDE_MODELS_STAGED:   # (no 'sine_' aliases here: the name is stored)
            raise KeyError(stock_model_name)
        hwf = stock_model_name == 'HestonWOFeller'
        if hwf and hp.get('scheme', 'euler') != 'euler':
            raise ValueError('unknown sampling scheme')
        stage = stage_struct(stock_model_name, hp, dim)
        sde = stage.sde
        N, S = sde.n_paths, sde.n_steps
        paths = torch.empty((S + 1, dim * (2 if stage.return_vol else 1), N), dtype=torch.float64,
                            device=dev)
        observed = torch.empty((S + 1, N), dtype=torch.uint8, device=dev)
        nb_obs = torch.empty(N, dtype=torch.int32, device=dev)
        z = u = None
        if normals is not None:
            z = torch.as_tensor(np.ascontiguousarray(normals, dtype=np.float64)).to(dev)
            per = 2 if stock_model_name in ('Heston', 'HestonWOFeller') else 1
            if z.numel() != N * S * per * dim:
                raise ValueError('normals must have N * S * {} * dim entries'.format(per))
        if uniforms is not None:
            u = torch.as_tensor(np.ascontiguousarray(uniforms, dtype=np.float64)).to(dev)
            if u.numel() != N * (S + 1):
                raise ValueError('uniforms must have N * (S + 1) entries')
        with torch.cuda.device(dev):
            st = _stream(dev)
            if hwf:
                _lib.check(L.njode_generate_stage(C.byref(stage), S, C.c_uint64(seed), _ptr(z),
                                                  _ptr(paths), st))
            else:
                _lib.check(L.njode_generate_paths(C.byref(sde), C.c_uint64(seed), _ptr(z),
                                                  _ptr(paths), st))
            _lib.check(L.njode_sample_observations(N, S, float(hp['obs_perc']),
                                                   C.c_uint64(seed), _ptr(u), _ptr(observed),
                                                   _ptr(nb_obs), st))
        hp['dt'] = hp['maturity'] / hp['nb_steps']
        hp['model_name'] = stock_model_name
        return cls(paths, observed, nb_obs, hp)

    @classmethod
    def generate_combined(cls, stock_model_names, hyperparam_dicts, seed=0, device='cuda',
                          normals=None, uniforms=None):
        """``create_combined_dataset`` on the GPU: stage after stage into one buffer -- stage ``i``
        reads its start values from the last slice of stage ``i - 1`` -- then one observation draw
        over the concatenated grid with stage 0's ``obs_perc``; the reference's combined
        metadata.  ``normals``: one array per stage (reference draw order) or None."""
        L = _lib.lib()
        dev = torch.device(device)
        names = list(stock_model_names)
        hps = [dict(hp) for hp in hyperparam_dicts]
        if not names or len(names) != len(hps):
            raise ValueError('one hyperparam_dict per stock model name, at least one')
        if normals is not None and len(normals) != len(names):
            raise ValueError('normals: one array per stage')
        dim = int(np.size(hps[0].get('S0', 1)))
        stages, s0 = [], 0
        for i, (name, hp) in enumerate(zip(names, hps)):
            for key in ('nb_paths', 'nb_steps'):
                if key not in hp:
                    raise KeyError(key)
            if name not in _lib.SDE_MODELS_STAGED:
                raise KeyError(name)
            if name == 'HestonWOFeller' and hp.get('return_vol'):
                raise ValueError('a return_vol stage cannot be combined: its paths are twice as wide')
            if name == 'HestonWOFeller' and hp.get('scheme', 'euler') != 'euler':
                raise ValueError('unknown sampling scheme')
            if int(np.size(hp.get('S0', 1))) != dim or hp.get('dimension') != hps[0].get('dimension') \
                    or hp['nb_paths'] != hps[0]['nb_paths']:
                raise ValueError('stages must agree in dimension and nb_paths')
            if dim != 1 and np.ptp(np.asarray(hp['S0'], dtype=np.float64)) != 0:
                raise ValueError('S0 must be the same in every dimension')
            if hp['maturity'] / hp['nb_steps'] != hps[0]['maturity'] / hps[0]['nb_steps']:
                raise ValueError('stages must agree in dt')
            stages.append(stage_struct(name, hp, dim, first_step=s0))
            s0 += stages[-1].sde.n_steps
            hp['model_name'] = name
        N, S = stages[0].sde.n_paths, s0
        paths = torch.empty((S + 1, dim, N), dtype=torch.float64, device=dev)
        observed = torch.empty((S + 1, N), dtype=torch.uint8, device=dev)
        nb_obs = torch.empty(N, dtype=torch.int32, device=dev)
        zs = [None] * len(stages)
        if normals is not None:
            for i, (st, name) in enumerate(zip(stages, names)):
                zs[i] = torch.as_tensor(np.ascontiguousarray(normals[i], dtype=np.float64)).to(dev)
                per = 2 if name in ('Heston', 'HestonWOFeller') else 1
                if zs[i].numel() != N * st.sde.n_steps * per * dim:
                    raise ValueError('normals[{}] must have N * S_i * {} * dim entries'.format(i, per))
        u = None
        if uniforms is not None:
            u = torch.as_tensor(np.ascontiguousarray(uniforms, dtype=np.float64)).to(dev)
            if u.numel() != N * (S + 1):
                raise ValueError('uniforms must have N * (S + 1) entries')
        with torch.cuda.device(dev):
            stream = _stream(dev)
            for st, z in zip(stages, zs):
                _lib.check(L.njode_generate_stage(C.byref(st), S, C.c_uint64(seed), _ptr(z),
                                                  _ptr(paths), stream))
            _lib.check(L.njode_sample_observations(N, S, float(hps[0]['obs_perc']),
                                                   C.c_uint64(seed), _ptr(u), _ptr(observed),
                                                   _ptr(nb_obs), stream))
        maturity = 0
        for hp in hps:
            maturity = maturity + hp['maturity']
        meta = {'dt': hps[-1]['maturity'] / hps[-1]['nb_steps'], 'maturity': maturity,
                'dimension': hps[0].get('dimension'), 'nb_paths': hps[0]['nb_paths'],
                'model_name': 'combined', 'stock_model_names': names, 'hyperparam_dicts': hps}
        return cls(paths, observed, nb_obs, meta)

    @classmethod
    def from_arrays(cls, stock_paths, observed_dates, nb_obs, metadata, device='cuda'):
        """Upload a host dataset (``create_dataset`` / ``load_dataset_dir`` arrays:
        paths f64 ``[N, d, S+1]``, observed ``[N, S+1]``) in time-major layout."""
        dev = torch.device(device)
        p = torch.as_tensor(np.ascontiguousarray(np.transpose(stock_paths, (2, 1, 0)),
                                                 dtype=np.float64)).to(dev)
        o = torch.as_tensor(np.ascontiguousarray(observed_dates.T != 0).astype(np.uint8)).to(dev)
        n = torch.as_tensor(np.asarray(nb_obs, dtype=np.int32)).to(dev)
        return cls(p, o, n, metadata)

    def to_arrays(self):
        """Host copy in the reference's layout (paths ``[N, d, S+1]``, observed ``[N, S+1]``)."""
        return (self.paths_tm.permute(2, 1, 0).contiguous().cpu().numpy(),
                self.observed_tm.t().contiguous().cpu().numpy().astype(np.int64),
                self.nb_obs.cpu().numpy().astype(np.int64))

    # -- batches -------------------------------------------------------------------------
    def collate(self, idx=None, func_names=()):
        """The batch ``custom_collate_fn`` builds for dataset rows ``idx`` (device int32
        tensor / array-like in batch order; None = the whole dataset), with ``X``,
        ``start_X``, ``obs_idx`` (int32) and ``n_obs_ot`` (int32) on the device and
        ``times`` / ``time_ptr`` as numpy arrays.

        The per-time counts must reach the host before ``X`` can be sized, so the call waits for
        its own first kernel (``prepare_batches`` + ``fill_batch`` is the form without a wait per
        batch: one host round trip per epoch).

        Rows given on the host (a list, a numpy array, a CPU tensor) are checked: ``ValueError``
        for a row outside ``[0, n_paths)`` or a non-integer one, before anything is launched.  A
        device tensor is used as it is, unchecked -- a check would cost a host wait per batch --
        so its rows are the caller's responsibility: the kernels read the dataset at whatever
        row they are given."""
        L = _lib.lib()
        dev = self.device
        if idx is not None:
            if torch.is_tensor(idx) and idx.device.type != 'cpu':
                idx = idx.to(dev).to(torch.int32).contiguous().reshape(-1)
            else:
                idx = torch.from_numpy(_host_rows(idx, self.n_paths)).to(dev)
            B = idx.numel()
        else:
            B = self.n_paths
        if B == 0:
            raise ValueError('empty batch')
        powers = parse_powers(func_names)
        width = self.dim * (1 + len(powers))
        pw = (C.c_int32 * max(len(powers), 1))(*powers)
        counts = torch.empty(self.n_steps, dtype=torch.int32, device=dev)
        n_obs_ot = torch.empty(B, dtype=torch.int32, device=dev)
        start_X = torch.empty((B, width), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = _stream(dev)
            _lib.check(L.njode_collate_count(_ptr(self.observed_tm), _ptr(self.nb_obs),
                                             self.n_paths, self.n_steps, _ptr(idx), B,
                                             _ptr(counts), _ptr(n_obs_ot), st))
            self._counts_host.copy_(counts, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            times, time_ptr = times_from_counts(self._counts_host.numpy(), self.metadata['dt'])
            n_obs = int(time_ptr[-1])
            X = torch.empty((n_obs, width), dtype=torch.float32, device=dev)
            obs_idx = torch.empty(n_obs, dtype=torch.int32, device=dev)
            _lib.check(L.njode_collate_fill(_ptr(self.paths_tm), _ptr(self.observed_tm),
                                            self.n_paths, self.dim, self.n_steps, _ptr(idx), B,
                                            _ptr(counts), pw, len(powers), _ptr(start_X),
                                            _ptr(X) if n_obs else C.c_void_p(0),
                                            _ptr(obs_idx) if n_obs else C.c_void_p(0), st))
        return {'times': times, 'time_ptr': time_ptr, 'obs_idx': obs_idx, 'start_X': start_X,
                'n_obs_ot': n_obs_ot, 'X': X}

    # -- a whole epoch's batches: one host round trip instead of one per batch -----------------
    def prepare_batches(self, idx_list):
        """Phase 1 of the collate (per-time observation counts) for MANY batches at once: the
        count kernels of all batches are enqueued back to back, their results cross PCIe in ONE
        copy and the host waits ONCE -- a training loop at the reference's batch sizes
        (B = 100 / 200) is host-bound, and the per-batch wait for its own count kernel was the
        largest item of its step.  ``idx_list``: dataset rows of each batch (array-likes on the
        host, in batch order); ``ValueError`` for a row outside ``[0, n_paths)``, before anything is
        uploaded or launched.  Returns one descriptor per batch for ``fill_batch``."""
        L = _lib.lib()
        dev = self.device
        sizes = [len(ix) for ix in idx_list]
        if not sizes or min(sizes) <= 0:
            raise ValueError('empty batch')
        flat = _host_rows(np.concatenate([np.asarray(ix).reshape(-1) for ix in idx_list]),
                          self.n_paths)
        idx_dev = torch.as_tensor(flat).to(dev)                       # one upload per epoch
        n = len(sizes)
        counts = torch.empty((n, self.n_steps), dtype=torch.int32, device=dev)
        n_obs_ot = torch.empty(len(flat), dtype=torch.int32, device=dev)
        offs = np.concatenate([[0], np.cumsum(sizes)])
        with torch.cuda.device(dev):
            st = _stream(dev)
            for i in range(n):
                lo, hi = int(offs[i]), int(offs[i + 1])
                _lib.check(L.njode_collate_count(
                    _ptr(self.observed_tm), _ptr(self.nb_obs), self.n_paths, self.n_steps,
                    C.c_void_p(idx_dev.data_ptr() + 4 * lo), hi - lo,
                    C.c_void_p(counts.data_ptr() + 4 * i * self.n_steps),
                    C.c_void_p(n_obs_ot.data_ptr() + 4 * lo), st))
            counts_host = counts.cpu().numpy()                        # one copy, one wait
        out = []
        for i in range(n):
            lo, hi = int(offs[i]), int(offs[i + 1])
            times, time_ptr = times_from_counts(counts_host[i], self.metadata['dt'])
            out.append({'times': times, 'time_ptr': time_ptr, 'idx': idx_dev[lo:hi],
                        'counts': counts[i], 'n_obs_ot': n_obs_ot[lo:hi], 'B': hi - lo})
        return out

    def fill_batch(self, prep, func_names=()):
        """Phase 2 for one descriptor of ``prepare_batches``: two kernel launches, no host
        wait.  Same batch, bit for bit, as ``collate`` builds."""
        L = _lib.lib()
        dev = self.device
        B = prep['B']
        powers = parse_powers(func_names)
        width = self.dim * (1 + len(powers))
        pw = (C.c_int32 * max(len(powers), 1))(*powers)
        n_obs = int(prep['time_ptr'][-1])
        start_X = torch.empty((B, width), dtype=torch.float32, device=dev)
        X = torch.empty((n_obs, width), dtype=torch.float32, device=dev)
        obs_idx = torch.empty(n_obs, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.njode_collate_fill(_ptr(self.paths_tm), _ptr(self.observed_tm),
                                            self.n_paths, self.dim, self.n_steps,
                                            _ptr(prep['idx']), B, _ptr(prep['counts']), pw,
                                            len(powers), _ptr(start_X),
                                            _ptr(X) if n_obs else C.c_void_p(0),
                                            _ptr(obs_idx) if n_obs else C.c_void_p(0),
                                            _stream(dev)))
        return {'times': prep['times'], 'time_ptr': prep['time_ptr'], 'obs_idx': obs_idx,
                'start_X': start_X, 'n_obs_ot': prep['n_obs_ot'], 'X': X}
