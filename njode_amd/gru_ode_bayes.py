"""
GRU-ODE-Bayes, the baseline the reference trains with ``other_model='GRU_ODE_Bayes'``
(``GRU_ODE_Bayes/models_gru_ode_bayes.py:270-558``), on the GPU: ``NNFOwithBayesianJumps`` runs its
forward and its exact gradient in the kernels of ``include/njode_gob.h``
(``njode_amd/csrc/njode_gob.hip``), one wave per path.

Same constructor signature, ``state_dict`` keys and shapes, initialisation, ``forward`` signature
and return conventions as the reference's class.  Built: ``full_gru_ode=True``, ``logvar=True``,
``solver='euler'``, ``impute`` False or True, ``cov = start_X``.  Everything else is refused at
construction with ``NotImplementedError``.

The parameters the loss depends on are fp32 views of ONE flat vector in the C ABI's order (bias
slots always present), so plain ``torch.optim`` on ``parameters()`` trains with nothing else.
``classification_model.*`` and ``gru_obs.gru_debug.*`` are ordinary parameters outside that vector:
the loss does not depend on them, their ``.grad`` stays ``None`` after ``loss.backward()`` as in the
reference, and an optimizer with weight decay leaves them untouched.  ``class_pred`` is computed with
torch ops from the kernels' ``hT``.

Dropout: train-mode masks are the kernels' shape-generic stream (``oracle/dropout_oracle.py``,
``'gen'``), nets 5 (``covariates_map``), 6 (``p_model`` at the start and after Euler step k) and 7
(``p_model`` after time slice i, time key ``k_jump[i]``), path id = batch row; the call seed is
``(dropout_seed * 0x9E3779B97F4A7C15 + step counter) mod 2^64`` and a training call advances the
counter.  Options ``dropout_seed`` and ``device_outputs`` (keep the losses on the GPU; the default
returns them on the CPU, where the reference harness calls ``.numpy()``) are read from the keyword
``options``, as ``models.NJODE`` reads them.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._flat import FlatVector
from ._slabcall import _SlabCall, _SlabFunction, issuing
from .schedule import ScheduleCache


def init_weights(m):
    """Xavier on Linear weights, biases 0.05 (``models_gru_ode_bayes.py:264-268``)."""
    if type(m) == torch.nn.Linear:
        torch.nn.init.xavier_uniform_(m.weight)
        if m.bias is not None:
            m.bias.data.fill_(0.05)


class _GRUODECell(torch.nn.Module):
    """Parameter holder of the full GRU-ODE cell (``:99-174``): ``lin_x`` only with impute; the
    three ``lin_h*`` have no bias."""

    def __init__(self, input_size, hidden_size, bias):
        super().__init__()
        if input_size is not None:
            self.lin_x = torch.nn.Linear(input_size, hidden_size * 3, bias=bias)
        self.lin_hh = torch.nn.Linear(hidden_size, hidden_size, bias=False)
        self.lin_hz = torch.nn.Linear(hidden_size, hidden_size, bias=False)
        self.lin_hr = torch.nn.Linear(hidden_size, hidden_size, bias=False)


class _ObservationCell(torch.nn.Module):
    """Parameter holder of the observation cell with log-variance (``:176-190``)."""

    def __init__(self, input_size, hidden_size, prep_hidden, bias):
        super().__init__()
        self.gru_d = torch.nn.GRUCell(prep_hidden * input_size, hidden_size, bias=bias)
        self.gru_debug = torch.nn.GRUCell(prep_hidden * input_size, hidden_size, bias=bias)
        std = math.sqrt(2.0 / (4 + prep_hidden))
        self.w_prep = torch.nn.Parameter(std * torch.randn(input_size, 4, prep_hidden))
        self.bias_prep = torch.nn.Parameter(0.1 + torch.zeros(input_size, prep_hidden))


class NNFOwithBayesianJumps(FlatVector, torch.nn.Module):
    """Neural negative feedback ODE with Bayesian jumps on the GPU; the interface of the
    reference's class of the same name.  The autograd node of a saved forward (``_SlabFunction``)
    has the outputs (losses, hT), ``losses = [loss, loss_1]``."""
    _moved_error = 'the parameters of this forward were moved before its backward'

    def __init__(self, input_size, hidden_size, p_hidden, prep_hidden, bias=True, cov_size=1, cov_hidden=1,
                 classification_hidden=1, logvar=True, mixing=1, dropout_rate=0, full_gru_ode=False,
                 solver="euler", impute=True, **options):
        super().__init__()
        assert solver in ["euler", "midpoint", "dopri5"], \
            "Solver must be either 'euler' or 'midpoint' or 'dopri5'."
        if not full_gru_ode:
            raise NotImplementedError('full_gru_ode=False: only the full GRU-ODE cell has kernels '
                                      '(train.py constructs the model with full_gru_ode=True)')
        if not logvar:
            raise NotImplementedError('logvar=False: only the log-variance observation cell has kernels')
        if solver != 'euler':
            raise NotImplementedError("solver='{}': only the Euler solver has kernels".format(solver))
        if options.get('smoother'):
            raise NotImplementedError('smoother=True is not built')
        if options.pop('store_hist', False):
            raise NotImplementedError('store_hist is not built (it belongs to the dopri5 solver)')
        if cov_size != input_size:
            raise NotImplementedError('cov_size={} != input_size={}: the kernels take cov = start_X, as '
                                      'train.py passes it'.format(cov_size, input_size))
        options1 = options.get('options') or {}
        self.epoch = 1
        self.weight = mixing
        self.impute = bool(impute)
        self.solver = solver
        self.store_hist = False
        self.input_size, self.hidden_size = input_size, hidden_size
        self.p_hidden, self.prep_hidden, self.cov_hidden = p_hidden, prep_hidden, cov_hidden
        self.logvar = logvar
        self.mixing = mixing
        self.bias = bias
        self.dropout_rate = float(dropout_rate)
        self.device_outputs = bool(options1.get('device_outputs', options.get('device_outputs', False)))
        self.seed = int(options1.get('dropout_seed', options.get('dropout_seed', 0)))
        self._step_counter = 0
        self._flat = self._param_slices = self._flat_params = self._dims = self._ring = None
        self._fresh_runtime_state()
        self._get_dims()       # (refuses what the library has no kernels for)

        self.p_model = torch.nn.Sequential(
            torch.nn.Linear(hidden_size, p_hidden, bias=bias), torch.nn.ReLU(),
            torch.nn.Dropout(p=dropout_rate), torch.nn.Linear(p_hidden, 2 * input_size, bias=bias))
        self.classification_model = torch.nn.Sequential(
            torch.nn.Linear(hidden_size, classification_hidden, bias=bias), torch.nn.ReLU(),
            torch.nn.Dropout(p=dropout_rate), torch.nn.Linear(classification_hidden, 1, bias=bias))
        self.gru_c = _GRUODECell(2 * input_size if self.impute else None, hidden_size, bias)
        self.gru_obs = _ObservationCell(input_size, hidden_size, prep_hidden, bias)
        self.covariates_map = torch.nn.Sequential(
            torch.nn.Linear(cov_size, cov_hidden, bias=bias), torch.nn.ReLU(),
            torch.nn.Dropout(p=dropout_rate), torch.nn.Linear(cov_hidden, hidden_size, bias=bias),
            torch.nn.Tanh())
        self.apply(init_weights)
        self._ensure_flat()

    # -- the library's description of the model ---------------------------------------------
    def _get_dims(self):
        if self._dims is not None:
            return self._dims
        d = _lib.NjodeGobDims(self.input_size, self.hidden_size, self.p_hidden, self.prep_hidden,
                              self.cov_hidden, (_lib.GOB_F_BIAS if self.bias else 0)
                              | (_lib.GOB_F_IMPUTE if self.impute else 0))
        if not _lib.lib().njode_gob_supported(ctypes.byref(d)):
            why = _lib.lib().njode_last_error().decode('utf-8', 'replace')
            raise NotImplementedError(
                'libnjode_hip.so has no GRU-ODE-Bayes kernels for input_size={}, hidden_size={}, p_hidden={}, '
                'prep_hidden={}, cov_hidden={}: {}'.format(self.input_size, self.hidden_size, self.p_hidden,
                                                           self.prep_hidden, self.cov_hidden, why))
        self._dims = d
        return d

    # -- flat parameter storage ---------------------------------------------------------------
    def _flat_slots(self):
        """[(parameter or None, slot size, shape)] in the C ABI's order (bias slot always present)."""
        slots = []

        def linear(m):
            slots.append((m.weight, m.weight.numel(), tuple(m.weight.shape)))
            slots.append((m.bias, m.out_features, (m.out_features,)))

        linear(self.p_model[0])
        linear(self.p_model[3])
        if self.impute:
            linear(self.gru_c.lin_x)
        for m in (self.gru_c.lin_hh, self.gru_c.lin_hz, self.gru_c.lin_hr):
            slots.append((m.weight, m.weight.numel(), tuple(m.weight.shape)))
        g = self.gru_obs
        slots.append((g.w_prep, g.w_prep.numel(), tuple(g.w_prep.shape)))
        slots.append((g.bias_prep, g.bias_prep.numel(), tuple(g.bias_prep.shape)))
        H3 = 3 * self.hidden_size
        slots.append((g.gru_d.weight_ih, g.gru_d.weight_ih.numel(), tuple(g.gru_d.weight_ih.shape)))
        slots.append((g.gru_d.weight_hh, g.gru_d.weight_hh.numel(), tuple(g.gru_d.weight_hh.shape)))
        slots.append((getattr(g.gru_d, 'bias_ih', None), H3, (H3,)))
        slots.append((getattr(g.gru_d, 'bias_hh', None), H3, (H3,)))
        linear(self.covariates_map[0])
        linear(self.covariates_map[3])
        return slots

    def _ensure_flat(self):
        flat = self._flat
        super()._ensure_flat()
        if self._flat is not flat:      # (laid out anew: the library counts the same slots)
            assert self._flat.numel() == _lib.lib().njode_gob_param_count(ctypes.byref(self._get_dims()))

    def _fresh_runtime_state(self):
        self._schedules = ScheduleCache(16)

    def _backward_into(self, call, grads, grad_flat):
        """``njode_gob_backward_f32`` of a saved forward: the exact discrete adjoint."""
        grad_losses, grad_hT = grads
        mixing, p_drop, seed = call.extra
        dev = call.flat.device
        B, H = call.sizes[0], self.hidden_size
        gl = (torch.zeros(2, dtype=torch.float32, device=dev) if grad_losses is None
              else grad_losses.to(device=dev, dtype=torch.float32).reshape(2).contiguous())
        gh = None
        if grad_hT is not None:
            gh = grad_hT.to(device=dev, dtype=torch.float32).reshape(B, H).contiguous()
        _lib.check(_lib.lib().njode_gob_backward_f32(
            ctypes.byref(call.dims), call.flat.data_ptr(), ctypes.byref(call.batch), ctypes.byref(call.sched),
            call.flags, mixing, p_drop, seed, gl.data_ptr(), gl.data_ptr() + 4,
            _lib.ptr_arg(gh), grad_flat.data_ptr(), call.ws.data_ptr(), call.ws.numel(),
            _lib.stream_arg(dev)))

    # -- reference API ----------------------------------------------------------------------------
    def weight_decay_step(self):
        return self.mixing

    def forward(self, times, time_ptr, X, M, obs_idx, delta_t, T, cov, return_path=False, smoother=False,
                class_criterion=None, labels=None):
        """The contract of the reference's forward (``:365-494``): ``(hT, loss, class_pred, loss_1)``,
        or with ``return_path`` ``(hT, loss, class_pred, path_t, path_p, path_h, eval_times_total,
        eval_vals_total)``.  ``loss``, ``loss_1`` and ``hT`` are in the autograd graph (a
        ``return_path`` call builds none)."""
        if smoother:
            raise NotImplementedError('smoother=True is not built')
        dev = cov.device
        if dev.type != 'cuda':
            raise RuntimeError('njode_amd.NNFOwithBayesianJumps runs on an MI355X only (inputs are on {}); '
                               'there is no CPU path. Move the model and the batch to a cuda device.'
                               .format(dev))
        dims = self._get_dims()
        self._ensure_flat()
        if self._flat.device != dev:
            raise RuntimeError('model parameters are on {} but the batch is on {}'.format(self._flat.device, dev))
        trainable = (torch.is_grad_enabled() and not return_path
                     and any(p.requires_grad for p in self._flat_params))
        B = int(cov.shape[0])
        sched = self._schedules.get(times, delta_t, T, True)
        time_ptr = np.asarray(time_ptr, dtype=np.int32)
        assert len(times) + 1 == len(time_ptr)
        n_obs = int(time_ptr[-1])
        f32 = torch.float32
        cov = cov.to(f32).contiguous()
        X = X.to(device=dev, dtype=f32).contiguous()
        M = M.to(device=dev, dtype=f32).contiguous()
        idx = torch.as_tensor(obs_idx).to(device=dev, dtype=torch.int32).contiguous()
        assert cov.shape[1] == self.input_size and X.shape[0] >= n_obs and M.shape == X.shape

        call = _SlabCall()
        call.dims, call.keep = dims, [cov, X, M, idx]
        call.batch = _lib.NjodeBatch(B, n_obs, cov.data_ptr(), X.data_ptr() if n_obs else None,
                                     M.data_ptr() if n_obs else None, idx.data_ptr() if n_obs else None,
                                     None, float(B), 0, None, None)
        call.flags = ((_lib.C_TRAIN if self.training else 0) | (_lib.C_RETURN_PATH if return_path else 0)
                      | (_lib.C_SAVE_BWD if trainable else 0))
        call.sizes = (B, n_obs, sched.n_times, sched.n_steps)
        seed = (self.seed * 0x9E3779B97F4A7C15 + self._step_counter) & 0xFFFFFFFFFFFFFFFF
        call.extra = (float(self.mixing), self.dropout_rate, seed)
        if self.training:
            self._step_counter += 1
        L = _lib.lib()
        H, D2 = self.hidden_size, 2 * self.input_size
        with issuing(self, call, sched, time_ptr, L.njode_gob_workspace_bytes) as stream:
            hT = torch.empty(B, H, dtype=f32, device=dev)
            losses = torch.empty(2, dtype=f32, device=dev)
            path_h = path_p = None
            if return_path:
                path_h = torch.empty(sched.n_rows, B, H, dtype=f32, device=dev)
                path_p = torch.empty(sched.n_rows, B, D2, dtype=f32, device=dev)
            rc = L.njode_gob_forward_f32(
                ctypes.byref(dims), self._flat.data_ptr(), ctypes.byref(call.batch), ctypes.byref(call.sched),
                call.flags, *call.extra, hT.data_ptr(), losses.data_ptr(),
                _lib.ptr_arg(path_h), _lib.ptr_arg(path_p), call.ws.data_ptr(), call.ws.numel(),
                stream.cuda_stream)
        _lib.check(rc)
        if trainable:
            losses, hT = _SlabFunction.apply(self, call, (losses, hT), *self._flat_params)
        loss, loss_1 = losses[0], losses[1]
        if not self.device_outputs:
            loss, loss_1 = loss.cpu(), loss_1.cpu()
        class_pred = self.classification_model(hT)
        if return_path:
            eval_times_total = torch.zeros(sched.n_steps, dtype=torch.float64, device=dev)
            eval_vals_total = torch.zeros(sched.n_steps, dtype=f32, device=dev)
            return (hT, loss, class_pred, sched.path_t.copy(), path_p, path_h, eval_times_total,
                    eval_vals_total)
        return hT, loss, class_pred, loss_1

    def evaluate(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot, stockmodel,
                 cond_exp_fun_kwargs=None, diff_fun=lambda x, y: np.mean((x - y) ** 2), return_paths=False):
        """Distance of the predicted mean path to the true conditional expectation (``:497-537``)."""
        self.eval()
        with torch.no_grad():
            _, _, _, path_t, path_p, _, _, _ = self.forward(
                times, time_ptr, X, torch.ones_like(X), obs_idx, delta_t, T, start_X, return_path=True)
        path_y = torch.chunk(path_p, 2, dim=2)[0]
        _, true_path_t, true_path_y = stockmodel.compute_cond_exp(
            times, time_ptr, X.detach().cpu().numpy(), torch.as_tensor(obs_idx).detach().cpu().numpy(),
            delta_t, T, start_X.detach().cpu().numpy(), torch.as_tensor(n_obs_ot).detach().cpu().numpy(),
            return_path=True, get_loss=False)
        eval_loss = diff_fun(path_y.detach().cpu().numpy(), true_path_y)
        if return_paths:
            return eval_loss, path_t, true_path_t, path_y, true_path_y
        return eval_loss

    def get_pred(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, M=None):
        """Predicted mean path (``:540-558``); ``M``: the observation mask (default: all ones)."""
        with torch.no_grad():
            _, _, _, path_t, path_p, _, _, _ = self.forward(
                times, time_ptr, X, torch.ones_like(X) if M is None else M, obs_idx, delta_t, T, start_X,
                return_path=True)
        path_y = torch.chunk(path_p, 2, dim=2)[0]
        if not self.device_outputs:
            path_y = path_y.cpu()
        return {'pred': path_y, 'pred_t': path_t}


def from_options(input_size, hidden_size, bias, dropout_rate, options):
    """The model ``train.py:354-392`` builds from the ``'GRU_ODE_Bayes-*'`` options, with its
    defaults."""
    def opt(name, default):
        return options.get('GRU_ODE_Bayes-' + name, default)

    return NNFOwithBayesianJumps(
        input_size=input_size, hidden_size=hidden_size, p_hidden=opt('p_hidden', hidden_size),
        prep_hidden=opt('prep_hidden', hidden_size), bias=bias, cov_size=input_size,
        cov_hidden=opt('cov_hidden', hidden_size), logvar=opt('logvar', True), mixing=opt('mixing', 0.0001),
        dropout_rate=dropout_rate, full_gru_ode=opt('full_gru_ode', True), solver=opt('solver', 'euler'),
        impute=opt('impute', False),
        options=dict(device_outputs=True, dropout_seed=options.get('dropout_seed', 0)))
