"""
The float64 route: ``NJODE64`` evaluates, differentiates and trains an NJ-ODE in double precision
on the GPU (``include/njode_f64.h``, ``njode_amd/csrc/njode_f64.hip``).

It computes what the reference computes under ``model.double()`` with dropout off -- parameters,
inputs, activations, loss and gradients in float64; ``tau`` and ``tdiff`` stay the fp32 tensors the
reference makes them and are widened exactly; the Euler update uses the float64 step of the Python
clock.  ``models.NJODE.double()`` itself is unchanged (an fp32 evaluation); ``models.NJODE.float64()``
returns the twin defined here with the parameters widened exactly.

Same constructor arguments, ``state_dict`` keys, ``forward`` signature and return conventions as
``models.NJODE``.  The parameters are ``torch.float64`` views of ONE flat double vector in the C
ABI's order (bias slots always present), so plain ``torch.optim`` on ``parameters()`` trains in
double with nothing else.  Not built: the GRU jump (``use_rnn``) and dropout in train mode.
"""
import ctypes

import numpy as np
import torch

from . import _lib, models
from ._flat import FlatVector
from ._slabcall import _SlabCall, _SlabFunction, issuing
from .schedule import ScheduleCache, _walk_clock


class Schedule64:
    """The clock of one pass as the float64 route takes it: ``step_dt`` in float64 (the walk's own
    steps), ``step_t`` / ``time_f32`` rounded to fp32 where ATen rounds them, ``k_jump``."""
    __slots__ = ('step_dt', 'step_t', 'k_jump', 'time_f32', 'path_t', 'n_steps', 'n_times')

    def __init__(self, times, delta_t, T, until_T):
        times = np.asarray(times, dtype=np.float64)
        dts, ts, k_jump, path_t, _ = _walk_clock(times, delta_t, T, until_T)
        self.step_dt = np.asarray(dts, dtype=np.float64)
        self.step_t = np.asarray(ts, dtype=np.float64).astype(np.float32)
        self.k_jump = np.asarray(k_jump, dtype=np.int32)
        self.time_f32 = times.astype(np.float32)
        self.path_t = np.asarray(path_t, dtype=np.float64)
        self.n_steps, self.n_times = len(dts), len(times)

    @property
    def n_rows(self):
        return 1 + self.n_steps + self.n_times

    def packed_nbytes(self):
        return 8 * self.n_steps + 4 * (self.n_steps + 3 * self.n_times + 1)

    def pack_into(self, buf, time_ptr):
        """[step_dt (float64) | step_t | k_jump | time_f32 | time_ptr] into the int32 numpy view
        ``buf``; returns the ``NjodeSchedule64`` over it."""
        K, nt = self.n_steps, self.n_times
        buf[:2 * K].view(np.float64)[:] = self.step_dt
        w = buf[2 * K:]
        w[:K].view(np.float32)[:] = self.step_t
        w[K:K + nt] = self.k_jump
        w[K + nt:K + 2 * nt].view(np.float32)[:] = self.time_f32
        w[K + 2 * nt:K + 3 * nt + 1] = time_ptr
        return self.struct(buf.ctypes.data)

    def struct(self, base):
        """The ``NjodeSchedule64`` over a buffer ``pack_into`` has filled, at address ``base``."""
        K, nt = self.n_steps, self.n_times
        return _lib.NjodeSchedule64(K, nt, base, base + 8 * K, base + 12 * K, base + 12 * K + 4 * nt,
                                    base + 12 * K + 8 * nt)


def _nn_desc(desc):
    """``models.NJODE._descs`` entry -> the constructor's ``nn_desc``."""
    n, widths, acts = desc
    if n == 0:
        return None
    return tuple((w, 'tanh' if a == _lib.ACT_TANH else 'relu') for w, a in zip(widths, acts))


class NJODE64(FlatVector, torch.nn.Module):
    """NJ-ODE in float64 on the GPU; the interface of ``models.NJODE``.  The autograd node of a
    saved forward (``_SlabFunction``) has the outputs (loss, hT), or (hT,) of a ``get_loss=False``
    call; its backward takes the upstream gradient of hT as well."""
    _flat_dtype = torch.float64
    _moved_error = 'the parameters of this NJODE64 forward were moved before its backward'

    def __init__(self, input_size, hidden_size, output_size, ode_nn, readout_nn, enc_nn,
                 use_rnn, bias=True, dropout_rate=0, solver="euler", weight=0.5,
                 weight_decay=1., **options):
        super().__init__()
        self.epoch = 1
        self.weight = weight
        self.weight_decay = weight_decay
        self.use_rnn = use_rnn
        options1 = options['options']
        self.which_loss = options1.get('which_loss', 'standard')
        assert self.which_loss in models.LOSS_FUN_DICT
        self.residual_enc_dec = options1.get('residual_enc_dec', True)
        self.input_current_t = options1.get('input_current_t', False)
        self.masked = options1.get('masked', False)
        self.device_outputs = bool(options1.get('device_outputs', False))
        self.solver = solver
        self.input_size, self.hidden_size, self.output_size = input_size, hidden_size, output_size
        self.dropout_rate = float(dropout_rate)
        self.bias = bias
        self._descs = (models._desc_of(ode_nn), models._desc_of(enc_nn), models._desc_of(readout_nn))
        self._flat = self._param_slices = self._flat_params = self._dims = self._ring = None
        self._fresh_runtime_state()
        self._get_dims()       # (refuses what the library has no float64 kernels for: use_rnn)

        self.ode_f = models.ODEFunc(input_size, hidden_size, ode_nn, dropout_rate, bias,
                                    input_current_t=self.input_current_t)
        self.encoder_map = models.FFNN(input_size, hidden_size, enc_nn, dropout_rate, bias,
                                       masked=self.masked, residual=self.residual_enc_dec)
        self.readout_map = models.FFNN(hidden_size, output_size, readout_nn, dropout_rate, bias,
                                       residual=self.residual_enc_dec)
        self.apply(models.init_weights)
        self._ensure_flat()

    # -- the library's description of the model ---------------------------------------------
    def _get_dims(self):
        if self._dims is not None:
            return self._dims
        if self.solver != 'euler':
            raise ValueError("Unknown solver '{}'.".format(self.solver))
        flags = ((_lib.F_MASKED if self.masked else 0)
                 | (_lib.F_INPUT_CURRENT_T if self.input_current_t else 0)
                 | (_lib.F_RESIDUAL if self.residual_enc_dec else 0)
                 | (_lib.F_LOSS_EASY if self.which_loss == 'easy' else 0)
                 | (_lib.F_USE_RNN if self.use_rnn else 0))
        d = _lib.NjodeDims(self.input_size, self.hidden_size, self.output_size, 0, 0, 0, flags)
        d.per_net = 1
        for i, (n, ws, as_) in enumerate(self._descs):
            if n > _lib.MAX_HIDDEN:
                raise NotImplementedError('libnjode_hip.so runs networks with up to {} hidden layers; got {}'
                                          .format(_lib.MAX_HIDDEN, n))
            d.nets[i].n_hidden = n
            for l in range(n):
                d.nets[i].width[l], d.nets[i].act[l] = ws[l], as_[l]
        if not _lib.lib().njode_f64_supported(ctypes.byref(d)):
            why = _lib.lib().njode_last_error().decode('utf-8', 'replace')
            raise NotImplementedError(
                'libnjode_hip.so has no float64 kernels for input_size={}, hidden_size={}, output_size={}, '
                'ode/enc/readout nets={}, masked={}, use_rnn={}: {}'.format(
                    self.input_size, self.hidden_size, self.output_size, self._descs, self.masked,
                    self.use_rnn, why))
        self._dims = d
        return d

    # -- flat parameter storage ---------------------------------------------------------------
    def _flat_slots(self):
        """[(parameter or None, slot size, shape)] in the C ABI's order (bias slot always present)."""
        slots = []
        for seq in (self.ode_f.f, self.encoder_map.ffnn, self.readout_map.ffnn):
            for m in seq:
                if isinstance(m, torch.nn.Linear):
                    slots.append((m.weight, m.weight.numel(), tuple(m.weight.shape)))
                    slots.append((m.bias, m.out_features, (m.out_features,)))
        return slots

    def _fresh_runtime_state(self):
        self._schedules = ScheduleCache(16, make=Schedule64)

    def _backward_into(self, call, grads, grad_flat):
        """``njode_backward_f64`` of a saved forward: the exact discrete adjoint."""
        weight, has_loss = call.extra
        grad_loss, grad_hT = grads if has_loss else (None, grads[0])
        dev = call.flat.device
        B, H = call.sizes[0], self.hidden_size
        gl = gh = None
        if has_loss:
            gl = (torch.zeros(1, dtype=torch.float64, device=dev) if grad_loss is None
                  else grad_loss.to(device=dev, dtype=torch.float64).reshape(1).contiguous())
        if grad_hT is not None:
            gh = grad_hT.to(device=dev, dtype=torch.float64).reshape(B, H).contiguous()
        _lib.check(_lib.lib().njode_backward_f64(
            ctypes.byref(call.dims), call.flat.data_ptr(), ctypes.byref(call.batch), ctypes.byref(call.sched),
            call.flags, weight, _lib.ptr_arg(gl), _lib.ptr_arg(gh), grad_flat.data_ptr(),
            call.ws.data_ptr(), call.ws.numel(), _lib.stream_arg(dev)))

    # -- reference API ----------------------------------------------------------------------------
    def weight_decay_step(self):
        """weight <- 0.5 + (weight - 0.5) * weight_decay (``models.py:364-367``)."""
        inc = (self.weight - 0.5)
        self.weight = 0.5 + inc * self.weight_decay
        return self.weight

    def forward(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot,
                return_path=False, get_loss=True, until_T=False, M=None):
        """The contract of the reference's ``NJODE.forward`` (``models.py:379-518``) with float64
        tensors: ``(hT, loss)`` or ``(hT, loss, path_t, path_h, path_y)``; ``loss`` is the Python int
        0 when ``get_loss=False``.  ``X``, ``start_X`` and ``M`` may be fp32 or float64 (widened
        exactly).  ``loss`` and ``hT`` are both in the autograd graph."""
        if self.training and self.dropout_rate > 0:
            raise NotImplementedError(
                'NJODE64: dropout in train mode is not built for the float64 route (dropout_rate={}); '
                'call .eval(), or train with dropout_rate=0'.format(self.dropout_rate))
        dev = start_X.device
        if dev.type != 'cuda':
            raise RuntimeError('njode_amd.NJODE64 runs on an MI355X only (inputs are on {}); there is no '
                               'CPU path. Move the model and the batch to a cuda device.'.format(dev))
        dims = self._get_dims()
        self._ensure_flat()
        if self._flat.device != dev:
            raise RuntimeError('model parameters are on {} but the batch is on {}'.format(self._flat.device, dev))
        trainable = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if return_path:
            trainable = False       # (the reference's evaluation calls; a path call saves nothing)
        B = int(start_X.shape[0])
        sched = self._schedules.get(times, delta_t, T, until_T)
        time_ptr = np.asarray(time_ptr, dtype=np.int32)
        assert len(times) + 1 == len(time_ptr)
        n_obs = int(time_ptr[-1])
        f64 = torch.float64
        start_X = start_X.to(f64).contiguous()
        X = X.to(device=dev, dtype=f64).contiguous()
        idx = obs_idx.to(device=dev, dtype=torch.int32).contiguous()
        keep = [start_X, X, idx]
        M_d = n_d = None
        if self.masked:
            assert M is not None
            M_d = M.to(device=dev, dtype=f64).contiguous()
            keep.append(M_d)
        if get_loss:
            n_d = n_obs_ot.to(device=dev, dtype=torch.int32).contiguous()
            keep.append(n_d)

        call = _SlabCall()
        call.dims, call.keep, call.extra = dims, keep, (float(self.weight), bool(get_loss))
        call.batch = _lib.NjodeBatch64(B, n_obs, start_X.data_ptr(), X.data_ptr() if n_obs else None,
                                       M_d.data_ptr() if (M_d is not None and n_obs) else None,
                                       idx.data_ptr() if n_obs else None,
                                       n_d.data_ptr() if n_d is not None else None, float(B))
        call.flags = ((_lib.C_GET_LOSS if get_loss else 0) | (_lib.C_RETURN_PATH if return_path else 0)
                      | (_lib.C_SAVE_BWD if trainable else 0))
        call.sizes = (B, n_obs, sched.n_times, sched.n_steps)
        L = _lib.lib()
        with issuing(self, call, sched, time_ptr, L.njode_f64_workspace_bytes) as stream:
            hT = torch.empty(B, self.hidden_size, dtype=f64, device=dev)
            loss = torch.zeros(1, dtype=f64, device=dev) if get_loss else None
            path_h = path_y = None
            if return_path:
                path_h = torch.empty(sched.n_rows, B, self.hidden_size, dtype=f64, device=dev)
                path_y = torch.empty(sched.n_rows, B, self.output_size, dtype=f64, device=dev)
            rc = L.njode_forward_f64(
                ctypes.byref(dims), self._flat.data_ptr(), ctypes.byref(call.batch), ctypes.byref(call.sched),
                call.flags, call.extra[0], hT.data_ptr(), _lib.ptr_arg(loss), _lib.ptr_arg(path_h),
                _lib.ptr_arg(path_y), call.ws.data_ptr(), call.ws.numel(), stream.cuda_stream)
        _lib.check(rc)
        if trainable:
            outs = _SlabFunction.apply(self, call, (loss, hT) if get_loss else (hT,), *self._flat_params)
            loss, hT = outs if get_loss else (None, outs[0])
        loss_out = loss.reshape(()) if get_loss else 0
        if get_loss and not self.device_outputs:
            loss_out = loss_out.cpu()
        if return_path:
            return hT, loss_out, sched.path_t.copy(), path_h, path_y
        return hT, loss_out

    def get_pred(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, M=None):
        """Predicted path (reference ``models.py:564-584``)."""
        self.eval()
        _, _, path_t, path_h, path_y = self.forward(
            times, time_ptr, X, obs_idx, delta_t, T, start_X, None, return_path=True,
            get_loss=False, until_T=True, M=M)
        if not self.device_outputs:
            path_y = path_y.cpu()
        return {'pred': path_y, 'pred_t': path_t}


def twin_of(model):
    """``models.NJODE.float64()``: an ``NJODE64`` with ``model``'s settings and its parameters
    widened exactly, on ``model``'s device and in its train / eval mode."""
    ode, enc, dec = (_nn_desc(d) for d in model._descs)
    # (the constructor draws initial weights that are overwritten below: the caller's random stream
    # stays where it was)
    with torch.random.fork_rng(devices=[]):
        twin = NJODE64(model.input_size, model.hidden_size, model.output_size, ode, dec, enc, model.use_rnn,
                       bias=model.bias, dropout_rate=model.dropout_rate, solver=model.solver,
                       weight=model.weight, weight_decay=model.weight_decay,
                       options=dict(which_loss=model.which_loss, residual_enc_dec=model.residual_enc_dec,
                                    input_current_t=model.input_current_t, masked=model.masked,
                                    device_outputs=model.device_outputs))
    twin.epoch = model.epoch
    src = dict(model.named_parameters())
    twin.to(next(iter(src.values())).device)
    with torch.no_grad():
        for name, p in twin.named_parameters():
            p.copy_(src[name].detach().to(torch.float64))
    twin.train(model.training)
    return twin
