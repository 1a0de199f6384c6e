"""
NJ-ODE model with the operator surface of the reference's ``NJODE/models.py``,
executed by hand-written HIP kernels for gfx950 (libnjode_hip.so).

Same module-level names, constructor, ``forward`` signature and return
conventions, ``evaluate`` / ``get_pred`` / ``weight_decay_step``, checkpoint
helpers and ``state_dict`` keys as the reference (file:line cited per symbol),
so the class is constructed and called exactly like ``models.NJODE`` is by
``train.py`` / ``demo.py``.

What is different by construction:

* the sub-modules (``ode_f``, ``encoder_map``, ``readout_map``) only *hold*
  parameters under the reference's names; their math runs fused inside the
  kernels, so calling them directly raises.  There is no eager / CPU fallback:
  a model on a CPU device, or an unbuilt library, raises.
* all parameters are views of one flat fp32 vector (the layout of the C ABI),
  so the gradient comes back as one vector and the optimizer step can be fused.
* ``options['device_outputs']=True`` keeps ``loss`` / predictions on the GPU
  (no host sync); the default follows the reference harness, which calls
  ``.numpy()`` on them (``train.py:558,571,726``), and returns CPU tensors.
"""
import copy
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._calls import (CallLayer, _Call, _check_saved, _hT_and_loss_grads, _NJODEFunction,    # noqa: F401
                     _NJODEhTOnlyFunction, _Plan)
from ._flat import FlatParams
from .optim import FusedAdam, _raw_current_stream    # noqa: F401  (importable from here as before)
from .schedule import PinnedRing, ScheduleCache    # noqa: F401


# =====================================================================================
# module-level helpers with the reference's names
# =====================================================================================
def init_weights(m, bias=0.0):
    """Xavier-uniform weights, constant bias (reference ``models.py:21-26``)."""
    if type(m) == torch.nn.Linear:
        torch.nn.init.xavier_uniform_(m.weight)
        if m.bias is not None:
            m.bias.data.fill_(bias)


def save_checkpoint(model, optimizer, path, epoch):
    """``checkpt.tar`` with the reference's keys (``models.py:29-45``)."""
    if not os.path.exists(path):
        os.makedirs(path)
    torch.save({'epoch': epoch, 'weight': model.weight,
                'model_state_dict': model.state_dict(),
                'optimizer_state_dict': optimizer.state_dict()},
               os.path.join(path, 'checkpt.tar'))


def get_ckpt_model(ckpt_path, model, optimizer, device):
    """Load a checkpoint written by this build or by the reference, in place
    (``models.py:48-66``)."""
    ckpt_path = os.path.join(ckpt_path, 'checkpt.tar')
    if not os.path.exists(ckpt_path):
        raise Exception("Checkpoint " + ckpt_path + " does not exist.")
    checkpt = torch.load(ckpt_path, map_location='cpu', weights_only=False)
    if optimizer is not None:
        optimizer.load_state_dict(checkpt['optimizer_state_dict'])
    model.load_state_dict(checkpt['model_state_dict'])
    model.epoch = checkpt['epoch']
    model.weight = checkpt['weight']
    model.to(device)


def _norm(t, dim=1, eps=1e-10):
    return torch.sqrt(torch.sum(t, dim=dim) + eps)


def compute_loss(X_obs, Y_obs, Y_obs_bj, n_obs_ot, batch_size, eps=1e-10,
                 weight=0.5, M_obs=None):
    """Paper loss on tensors (reference ``models.py:71-106``).  Utility for
    callers that hold predictions; the training path computes the same
    expression inside the kernels."""
    m = 1.0 if M_obs is None else M_obs
    after = _norm(m * (X_obs - Y_obs) ** 2, eps=eps)
    before = _norm(m * (Y_obs_bj - Y_obs) ** 2, eps=eps)
    inner = (2 * weight * after + 2 * (1 - weight) * before) ** 2
    return torch.sum(inner / n_obs_ot) / batch_size


def compute_loss_2(X_obs, Y_obs, Y_obs_bj, n_obs_ot, batch_size, eps=1e-10,
                   weight=0.5, M_obs=None):
    """'easy' variant: second term uses X instead of Y (``models.py:109-126``)."""
    m = 1.0 if M_obs is None else M_obs
    after = _norm(m * (X_obs - Y_obs) ** 2, eps=eps)
    before = _norm(m * (Y_obs_bj - X_obs) ** 2, eps=eps)
    inner = (weight * after + (1 - weight) * before) ** 2
    return torch.sum(inner / n_obs_ot) / batch_size


LOSS_FUN_DICT = {'standard': compute_loss, 'easy': compute_loss_2}

nonlinears = {'tanh': torch.nn.Tanh, 'relu': torch.nn.ReLU}


def get_ffnn(input_size, output_size, nn_desc, dropout_rate, bias):
    """Parameter container with the reference's Sequential layout
    (``models.py:140-166``): Linear at indices 0, 3, 6, ... with activation and
    Dropout modules in between (kept so ``print(model)`` and the state_dict
    keys match)."""
    if nn_desc is None:
        layers = [torch.nn.Linear(input_size, output_size, bias=bias)]
    else:
        layers = [torch.nn.Linear(input_size, nn_desc[0][0], bias=bias)]
        for i in range(len(nn_desc) - 1):
            layers.append(nonlinears[nn_desc[i][1]]())
            layers.append(torch.nn.Dropout(p=dropout_rate))
            layers.append(torch.nn.Linear(nn_desc[i][0], nn_desc[i + 1][0], bias=bias))
        layers.append(nonlinears[nn_desc[-1][1]]())
        layers.append(torch.nn.Dropout(p=dropout_rate))
        layers.append(torch.nn.Linear(nn_desc[-1][0], output_size, bias=bias))
    return torch.nn.Sequential(*layers)


_FUSED_MSG = ('{} holds parameters only: its math runs inside the fused HIP kernels of '
              'NJODE.forward (libnjode_hip.so); there is no eager path.')


class ODEFunc(torch.nn.Module):
    """f_theta: parameters ``ode_f.f.*`` (reference ``models.py:170-199``)."""

    def __init__(self, input_size, hidden_size, ode_nn, dropout_rate=0.0, bias=True,
                 input_current_t=False):
        super().__init__()
        self.input_current_t = input_current_t
        add = 3 if input_current_t else 2
        self.f = get_ffnn(input_size=input_size + hidden_size + add, output_size=hidden_size,
                          nn_desc=ode_nn, dropout_rate=dropout_rate, bias=bias)

    def forward(self, x, h, tau, tdiff):
        raise RuntimeError(_FUSED_MSG.format('ODEFunc'))


class GRUCell(torch.nn.Module):
    """rho_theta: parameters ``obs_c.gru_d.*`` (reference ``models.py:202-217``)."""

    def __init__(self, input_size, hidden_size, bias=True):
        super().__init__()
        self.gru_d = torch.nn.GRUCell(input_size, hidden_size, bias=bias)
        self.input_size = input_size

    def forward(self, h, X_obs, i_obs):
        raise RuntimeError(_FUSED_MSG.format('GRUCell'))


class FFNN(torch.nn.Module):
    """Encoder / readout: parameters ``*.ffnn.*``; residual size rules and error
    messages of the reference (``models.py:220-276``)."""

    def __init__(self, input_size, output_size, nn_desc, dropout_rate=0.0, bias=True,
                 residual=False, masked=False):
        super().__init__()
        in_size = 2 * input_size if masked else input_size
        self.masked = masked
        self.ffnn = get_ffnn(input_size=in_size, output_size=output_size, nn_desc=nn_desc,
                             dropout_rate=dropout_rate, bias=bias)
        if residual:
            print('use residual network: input_size={}, output_size={}'.format(
                input_size, output_size))
            if input_size <= output_size:
                if output_size % input_size == 0:
                    self.case = 1
                    self.mult = int(output_size / input_size)
                else:
                    raise ValueError('for residual: output_size needs to be '
                                     'multiple of input_size')
            if input_size > output_size:
                if input_size % output_size == 0:
                    self.case = 2
                    self.mult = int(input_size / output_size)
                else:
                    raise ValueError('for residual: input_size needs to be '
                                     'multiple of output_size')
        else:
            self.case = 0

    def forward(self, nn_input, mask=None):
        raise RuntimeError(_FUSED_MSG.format('FFNN'))


# =====================================================================================
# the model
# =====================================================================================
def _desc_of(nn_desc):
    """(n_hidden, widths, acts) of a get_ffnn description (``nn_desc=None``: one Linear)."""
    if nn_desc is None:
        return (0, (), ())
    widths = tuple(int(w) for w, _ in nn_desc)
    for _, a in nn_desc:
        if a not in nonlinears:
            raise KeyError(a)
    acts = tuple(_lib.ACT_TANH if a == 'tanh' else _lib.ACT_RELU for _, a in nn_desc)
    return (len(nn_desc), widths, acts)


class NJODE(FlatParams, CallLayer, torch.nn.Module):
    """NJ-ODE model (reference ``models.py:280-584``), HIP-backed."""

    def __init__(self, input_size, hidden_size, output_size, ode_nn, readout_nn, enc_nn,
                 use_rnn, bias=True, dropout_rate=0, solver="euler", weight=0.5,
                 weight_decay=1., **options):
        super().__init__()
        self.epoch = 1
        self.weight = weight
        self.weight_decay = weight_decay
        self.use_rnn = use_rnn

        # the harness passes its whole params_dict; the model's own switches sit
        # under options['options'] (reference models.py:321)
        options1 = options['options']
        self.which_loss = options1.get('which_loss', 'standard')
        assert self.which_loss in LOSS_FUN_DICT
        print('using loss: {}'.format(self.which_loss))
        self.residual_enc_dec = options1.get('residual_enc_dec', True)
        self.input_current_t = options1.get('input_current_t', False)
        self.masked = options1.get('masked', False)
        self.device_outputs = bool(options1.get('device_outputs', False))
        # route the forward through torch.ops.njode_amd.forward (njode_amd/ops.py)
        self.torch_library_op = bool(options1.get('torch_library_op', False))

        self.ode_f = ODEFunc(input_size, hidden_size, ode_nn, dropout_rate, bias,
                             input_current_t=self.input_current_t)
        self.encoder_map = FFNN(input_size, hidden_size, enc_nn, dropout_rate, bias,
                                masked=self.masked, residual=self.residual_enc_dec)
        self.readout_map = FFNN(hidden_size, output_size, readout_nn, dropout_rate, bias,
                                residual=self.residual_enc_dec)
        if self.use_rnn:
            self.obs_c = GRUCell(input_size, hidden_size, bias=bias)

        self.solver = solver
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.output_size = output_size
        self.dropout_rate = float(dropout_rate)
        self.bias = bias
        self._descs = (_desc_of(ode_nn), _desc_of(enc_nn), _desc_of(readout_nn))

        self.apply(init_weights)

        # data-parallel sharding (set by the harness): global batch size used in the
        # loss denominator and the global index of this shard's first path
        self.dp_global_batch = None
        self.dp_path_offset = 0
        self.seed = int(options1.get('dropout_seed', 0))
        self._step_counter = 0

        self.dp_loss_in_bucket = False
        self._param_writes = 0       # writes to the flat vector through its raw pointer (FusedAdam.step)
        self._reset_runtime()

    def _reset_runtime(self):
        """What belongs to ONE instance's calls, as a fresh instance has it: device buffers in use,
        pinned slots, queued plans, streams (``_flat.py``, ``_calls.py``)."""
        self.__dict__.update(
            _flat=None, _flat_checks=0, _flat_grad=None, _grad_bucket=None, _flat_present=None,
            _param_slices=None, _flat_params=None, _ones=None, _sched_cache=ScheduleCache(), _ring=None,
            _ws_pool=[], _dims=None, _plans=[], _plan_pool=[], _plan_stream=None,
            # pinned schedule slots of plans whose launch is deferred, the plans themselves (their
            # buffers stay alive until launched) and the stream they were described on
            _deferred_slots=[], _deferred_plans=[], _deferred_stream=None, _last_hT_replay=None)

    # -- reference API ----------------------------------------------------------------
    def weight_decay_step(self):
        """weight <- 0.5 + (weight - 0.5) * weight_decay (``models.py:364-367``)."""
        inc = (self.weight - 0.5)
        self.weight = 0.5 + inc * self.weight_decay
        return self.weight

    def __deepcopy__(self, memo):
        """``copy.deepcopy(model)``: parameters, buffers, gradients and settings are copied; the copy
        starts with its own empty workspace pool, pinned ring, plan queue and schedule cache, and lays
        its parameters out in a flat vector of its own on first use."""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new._reset_runtime()
        for k, v in self.__dict__.items():
            if k not in new.__dict__:
                new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def float64(self):
        """A float64 twin (``njode_amd.float64.NJODE64``) with this model's parameters widened exactly:
        forward, gradients and training in double on the GPU.  ``double()`` stays an fp32 evaluation."""
        from .float64 import twin_of
        return twin_of(self)

    def flat_parameters(self):
        """The flat parameter vector all Linear parameters are views of."""
        self._ensure_flat()
        return self._flat

    def flat_grad(self):
        """A flat gradient vector whose slices are installed as ``.grad`` of the
        parameters (for the fused training step).  It is the head of ``grad_bucket()``."""
        self._ensure_flat()
        if self._flat_grad is None:
            # ONE bucket: the flat gradient and, behind it, one slot for the step's scalar loss,
            # so that a data-parallel step all-reduces both with a single collective
            # ("one RCCL all-reduce (sum) of the flat fp32 gradient [P] + the scalar loss")
            self._grad_bucket = torch.zeros(self._flat.numel() + 1, dtype=torch.float32,
                                            device=self._flat.device)
            self._flat_grad = self._grad_bucket[:-1]
            for p, g in zip(self._flat_params, self._split_flat(self._flat_grad)):
                p.grad = g
        return self._flat_grad

    def grad_bucket(self):
        """[P + 1] floats: ``flat_grad()`` followed by the loss slot (``loss_slot()``)."""
        self.flat_grad()
        return self._grad_bucket

    def loss_slot(self):
        """The last element of the bucket: where ``loss_and_grad`` writes the step's loss when
        ``dp_loss_in_bucket`` is set (``FusedAdam(distributed=True)`` sets it).  It then holds this
        rank's partial loss until ``FusedAdam.step()`` and the GLOBAL loss afterwards."""
        return self.grad_bucket()[-1:]

    # -- plan ahead (njode_plan_f32) --------------------------------------------------------
    def plan_defer_ok(self, n_obs):
        """Whether ``prefetch_plan`` defers a plan of ``n_obs`` observation rows into the next
        forward call's ODE-forward launch (``NJODE_C_PLAN_DEFER``) instead of building it on a helper
        stream.  Inside that launch the plan blocks share the memory system with a kernel that
        streams ~2 TB/s and take about twice their time on an idle chip; as long as they end before the
        forward does the step only pays their share of its slots: B = 100 0.250 -> 0.235 ms per step,
        B = 1 000 0.332 -> 0.317, 20 000 paths 0.877 -> 0.85; from 50 000 paths on the plan outlasts the
        forward (1.93 -> 1.95 ms; 125 000: 4.79 -> 4.85), so very large batches keep the helper stream
        (``profiles/r05_plan_in_forward.txt``).  ``NJODE_PLAN_DEFER=0`` switches it off,
        ``NJODE_PLAN_DEFER_MAX`` moves the limit (rows)."""
        if self.masked or self.use_rnn or os.environ.get('NJODE_PLAN_DEFER', '1') == '0':
            return False
        return 0 < n_obs <= int(os.environ.get('NJODE_PLAN_DEFER_MAX', '262144'))

    def prefetch_plan(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot,
                      M=None, need_hT=None, defer=None):
        """Build the execution plan of a coming ``loss_and_grad`` / training ``forward`` call
        for this batch NOW, on a helper stream, beside whatever the current stream is running
        (``include/njode_hip.h``: ``njode_plan_f32``).  The plan depends on the batch and the
        schedule only, not on the parameters; the call that later receives the same batch
        (same ``obs_idx`` tensor and ``time_ptr`` array, in the order they were prefetched)
        picks it up and skips its own plan stage.  Call it for batch i+1 right before the
        step on batch i.  Returns a handle that may be passed to that call as ``plan=``
        (otherwise the call finds it by the identity of ``obs_idx`` and ``time_ptr``).
        ``need_hT``: the coming call returns hT.  Default True -- ``forward`` always does;
        ``loss_and_grad`` of an unmasked model does not and simply ignores the tail order.
        ``defer`` (round 5; default: on for unmasked models without ``use_rnn``, ``NJODE_PLAN_DEFER=0``
        turns it off): no helper stream and no events -- the plan is built by the first blocks of the
        ODE-forward launch of the NEXT forward call on the current stream (``NJODE_C_PLAN_DEFER``,
        ``include/njode_hip.h``), i.e. of the step on batch i when this is called for batch i+1
        right before it; the batch's arrays must be ready on the current stream."""
        need_hT = True if need_hT is None else bool(need_hT)
        if defer is None:
            defer = self.plan_defer_ok(int(np.asarray(time_ptr)[-1]))
        call = self._describe_call(times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot, M=M,
                                   save_bwd=True)
        flags = call.flags | (_lib.C_NEED_HT if need_hT else 0)
        L = _lib.lib()
        need = ctypes.c_size_t(0)
        _lib.check(L.njode_plan_bytes(ctypes.byref(call.dims), *call.sizes, flags, ctypes.byref(need)))
        dev = start_X.device
        buf = self._plan_buffer(need.value, dev)
        if defer:
            # one queue: the job is only described now; the next forward call on this stream carries
            # it (or launches it in front of itself).  No helper stream, no event.
            stream, how = torch.cuda.current_stream(dev), _lib.C_PLAN_DEFER
        else:
            if self._plan_stream is None:
                self._plan_stream = torch.cuda.Stream(device=dev)
            stream, how = self._plan_stream, 0
            stream.wait_stream(torch.cuda.current_stream(dev))   # the batch's arrays are ready by now
        # (the library call, the ring and the event all take the stream explicitly: no
        # `with torch.cuda.stream(side)` -- entering and leaving it costs ~15 us of host time)
        _lib.check(L.njode_plan_f32(ctypes.byref(call.dims), ctypes.byref(call.batch), ctypes.byref(call.sched),
                                    flags | how, buf.data_ptr(), buf.numel(), stream.cuda_stream))
        plan = _Plan()
        plan.buf, plan.flags, plan.sizes, plan.keep, plan.pool = buf, flags, call.sizes, call.keep, self._plan_pool
        plan.obs_idx, plan.time_ptr, plan.taken = obs_idx, time_ptr, False
        plan.obs_version = getattr(obs_idx, '_version', 0)
        plan.pending, plan.stream, plan.done = bool(defer), stream if defer else None, None
        if defer:
            self._plan_deferred(plan, call.slot_i, stream)
        else:
            self._ring.release_after(call.slot_i, stream)
            plan.done = torch.cuda.Event()
            plan.done.record(stream)
        self._plans.append(plan)
        # plans nobody picks up (a prefetched batch that is then never stepped on) must not pile
        # up: keep the four newest
        while len(self._plans) > 4:
            self._plans.pop(0)
        return plan

    # -- forward -------------------------------------------------------------------------
    def forward(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot,
                return_path=False, get_loss=True, until_T=False, M=None, plan=None):
        """Same contract as the reference's ``NJODE.forward`` (``models.py:379-518``):
        returns ``(hT, loss)`` or ``(hT, loss, path_t, path_h, path_y)``; ``loss`` is
        the Python int 0 when ``get_loss=False``.  ``plan`` (optional, not in the reference):
        the handle ``prefetch_plan`` returned for this batch."""
        trainable = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        want_grad = trainable and get_loss
        if self.torch_library_op and not return_path:
            return self._forward_via_op(times, time_ptr, X, obs_idx, delta_t, T, start_X,
                                        n_obs_ot, get_loss, until_T, M, want_grad)
        call = self._describe_call(times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot,
                                   return_path=return_path, get_loss=get_loss, until_T=until_T, M=M,
                                   save_bwd=want_grad, rows_in_fwd=True)
        self._arm_call(call, plan, (obs_idx, time_ptr), want_hT=True)
        B, sched = call.sizes[0], call.sched_obj
        if trainable:
            self._track(call)
        dev = start_X.device
        hT = torch.empty(B, self.hidden_size, dtype=torch.float32, device=dev)
        loss = torch.zeros(1, dtype=torch.float32, device=dev) if get_loss else None
        path_h = path_y = None
        if return_path:
            path_h = torch.empty(sched.n_rows, B, self.hidden_size, dtype=torch.float32,
                                 device=dev)
            path_y = torch.empty(sched.n_rows, B, self.output_size, dtype=torch.float32,
                                 device=dev)
        try:
            self._run_forward(call, hT, loss, path_h, path_y)
        except Exception:
            self._release_ws(call)
            raise
        if want_grad:
            self._ensure_flat()
            loss_out, hT = _NJODEFunction.apply(self, call, (loss, hT), *self._flat_params)
            loss_out = loss_out.reshape(())
        else:
            self._release_ws(call)
            loss_out = loss.reshape(()) if get_loss else 0
            if not get_loss and trainable:
                self._ensure_flat()
                hT = _NJODEhTOnlyFunction.apply(self, call, (hT,), *self._flat_params)
        if get_loss and not self.device_outputs:
            loss_out = loss_out.cpu()       # reference harness calls .numpy() on it
        if return_path:
            return hT, loss_out, sched.path_t.copy(), path_h, path_y
        return hT, loss_out

    def _forward_via_op(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot,
                        get_loss, until_T, M, want_grad):
        """The same forward as one ``torch.library`` operator (``njode_amd/ops.py``)."""
        from . import ops
        self._ensure_flat()
        hT, loss, _ = torch.ops.njode_amd.forward(
            list(self._flat_params), start_X, X, obs_idx, n_obs_ot if get_loss else None,
            M if self.masked else None, torch.as_tensor(np.asarray(times, dtype=np.float64)),
            torch.as_tensor(np.asarray(time_ptr, dtype=np.int64)), float(delta_t), float(T),
            ops.register_model(self), bool(get_loss), bool(until_T), bool(want_grad))
        if not get_loss:
            return hT, 0
        loss_out = loss.reshape(())
        if not self.device_outputs:
            loss_out = loss_out.cpu()
        return hT, loss_out

    # -- fused training step (no autograd graph) ------------------------------------------
    def loss_and_grad(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot,
                      M=None, plan=None):
        """Forward + exact gradient in two library calls, no autograd bookkeeping:
        returns ``(None, loss)`` (device loss tensor; hT is not computed -- it would
        cost a per-path tail evolve nobody reads; masked and ``use_rnn`` models, whose
        lockstep plan produces it anyway, return it) and fills ``flat_grad()`` (whose
        slices are the parameters' ``.grad``).  The calls carry ``NJODE_C_LOSS_IN_BWD``:
        on the segment plan the forward skips its readout/loss pass over the observation
        rows and the backward, which evaluates the same readouts anyway, writes the loss.
        Used by the build's harness and bench."""
        grad = self.flat_grad()
        dev = start_X.device
        stream = torch.cuda.current_stream(dev)      # (one lookup per step: ~7 us each)
        lock = self.masked or self.use_rnn
        call = self._describe_call(times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot, M=M,
                                   save_bwd=True)
        self._arm_call(call, plan, (obs_idx, time_ptr), want_hT=lock, stream=stream)
        # (always written: sum of the terms; data parallel: written INTO the gradient bucket, see
        # loss_slot())
        loss = (self.loss_slot() if self.dp_loss_in_bucket
                else torch.empty(1, dtype=torch.float32, device=dev))
        # hT is only skipped on the segment plan (unmasked, no GRU jump): there it would cost an
        # extra per-path tail evolve; the lockstep plan (masked, use_rnn) produces it anyway
        hT = (torch.empty(call.sizes[0], self.hidden_size, dtype=torch.float32, device=dev)
              if lock else None)
        call.flags |= _lib.C_LOSS_IN_BWD
        try:
            self._run_forward(call, hT, loss, stream=stream)
            if self._ones is None or self._ones.device != dev:
                self._ones = torch.ones(1, dtype=torch.float32, device=dev)
            self._run_backward(call, self._ones, grad, loss=loss, stream=stream)
        finally:
            self._release_ws(call)
        return hT, loss.reshape(())

    # -- evaluation helpers ---------------------------------------------------------------
    def evaluate(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot,
                 stockmodel, cond_exp_fun_kwargs=None,
                 diff_fun=lambda x, y: np.mean((x - y) ** 2), return_paths=False, M=None):
        """Distance of the predicted path to the true conditional expectation
        (reference ``models.py:521-562``)."""
        self.eval()
        _, _, path_t, path_h, path_y = self.forward(
            times, time_ptr, X, obs_idx, delta_t, T, start_X, None, return_path=True,
            get_loss=False, until_T=True, M=M)
        _, true_path_t, true_path_y = stockmodel.compute_cond_exp(
            times, time_ptr, X.detach().cpu().numpy(), obs_idx.detach().cpu().numpy(),
            delta_t, T, start_X.detach().cpu().numpy(), n_obs_ot.detach().cpu().numpy(),
            return_path=True, get_loss=False)
        eval_loss = diff_fun(path_y.detach().cpu().numpy(), true_path_y)
        if return_paths:
            return eval_loss, path_t, true_path_t, path_y, true_path_y
        return eval_loss

    def evaluate_device(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, stockmodel,
                        return_paths=False):
        """``evaluate`` with the default ``diff_fun`` without leaving the GPU: the prediction
        path, then ``mean((path_y - true_path_y) ** 2)`` against the analytic conditional
        expectation of ``stockmodel`` (a ``stock_model`` object or a dataset's metadata dict)
        from ``device_data.cond_exp`` -- float64, fused: the true path is only stored with
        ``return_paths``.  Returns a 0-dim float64 device tensor with
        ``options['device_outputs']``, else a Python float; with ``return_paths`` the tuple
        ``(eval_loss, path_t, true_path_t, path_y, true_path_y)`` of ``evaluate`` with device
        tensors.  Unmasked synthetic data only (``ValueError`` for lifted inputs)."""
        from . import device_data
        self.eval()
        with torch.no_grad():
            _, _, path_t, _, path_y = self.forward(
                times, time_ptr, X, obs_idx, delta_t, T, start_X, None, return_path=True,
                get_loss=False, until_T=True)
        true_path_t, true_path_y, _, sq_diff = device_data.cond_exp(
            stockmodel, times, time_ptr, X, obs_idx, delta_t, T, start_X, pred=path_y,
            want_path=return_paths)
        eval_loss = sq_diff / path_y.numel()
        if not self.device_outputs:
            eval_loss = float(eval_loss)
        if return_paths:
            return eval_loss, path_t, true_path_t, path_y, true_path_y
        return eval_loss

    def get_pred(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, M=None):
        """Predicted path (reference ``models.py:564-584``)."""
        self.eval()
        _, _, path_t, path_h, path_y = self.forward(
            times, time_ptr, X, obs_idx, delta_t, T, start_X, None, return_path=True,
            get_loss=False, until_T=True, M=M)
        if not self.device_outputs:
            path_y = path_y.cpu()           # reference harness calls .numpy() on it
        return {'pred': path_y, 'pred_t': path_t}

    # -- online filtering (not in the reference) ------------------------------------------
    def online(self, n_series, delta_t, kernels='wave'):
        """The resident state of ``n_series`` series (``njode_amd/online.py``: ``reset``,
        ``observe``, ``advance``, ``predict``): each new measurement costs the Euler steps since the
        last one instead of a ``get_pred`` over the whole history.  Eval mode.  ``kernels='wave'``
        (the default): models with two hidden layers per network and sizes up to 64, no GRU jump
        (``NotImplementedError`` otherwise); ``kernels='generic'``: every model the shape-generic
        kernels run -- wider and deeper networks, ``nn_desc = None``, ``use_rnn``; ``'auto'``: the
        first where it applies, else the second."""
        from .online import OnlineState
        return OnlineState(self, n_series, delta_t, kernels=kernels)

