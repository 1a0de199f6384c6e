"""
The call layer under ``models.NJODE``: one description of a library call (``_Call``), the step
that arms it for launch, the functions that issue ``njode_forward_f32`` / ``njode_backward*_f32``,
and the pools those calls draw from.  Who owns what:

* workspace slots (``_ws_pool``, entries ``[buffer, taken]``): ``taken`` is set by ``_acquire_ws``
  and cleared by ``_Call.release`` -- which is ``_release_ws`` and ``_Call.__del__`` -- only;
* the plan queue (``_plans``): filled by ``NJODE.prefetch_plan``, emptied by ``_take_plan``;
* deferred-plan state (``_deferred_slots`` / ``_deferred_plans`` / ``_deferred_stream``): changed
  by ``_plan_deferred`` and ``_forward_issued`` only.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .schedule import PinnedRing


def _grown(nbytes, device):
    """A byte buffer for a request of ``nbytes``, with room to grow into (workspaces, plan buffers)."""
    return torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)


class _Call:
    """Everything one library call needs, kept alive until the stream has used it.
    Dropping the last reference (e.g. an autograd graph that is never back-propagated)
    returns the workspace to the model's pool."""
    __slots__ = ('dims', 'batch', 'sched', 'flags', 'sizes', 'weight', 'p_drop', 'seed', 'ws',
                 'keep', 'ws_slot', 'slot_i', 'pinned', 'sched_obj', 'time_ptr', 'inputs', 'flat',
                 'stamp')

    def release(self):
        slot = getattr(self, 'ws_slot', None)
        if slot is not None:
            slot[1] = False
            self.ws_slot = None

    __del__ = release

    def lead_args(self, flat):
        """The eight leading arguments of ``njode_forward_f32`` / ``njode_backward*_f32``."""
        return (ctypes.byref(self.dims), flat.data_ptr(), ctypes.byref(self.batch),
                ctypes.byref(self.sched), self.flags, self.weight, self.p_drop, self.seed)


class _Plan:
    """A plan built ahead by ``NJODE.prefetch_plan``; its buffer returns to the model's pool
    when the last call that reads it is gone.  It holds the ORIGINAL ``obs_idx`` / ``time_ptr``
    objects of its batch (so their ids cannot be recycled for another batch while the plan is
    queued) and the version counter ``obs_idx`` had: a call only takes a plan of the very same,
    unmodified objects."""
    __slots__ = ('buf', 'done', 'flags', 'sizes', 'keep', 'pool', 'obs_idx', 'time_ptr',
                 'obs_version', 'taken', 'pending', 'stream')

    def __del__(self):
        # a deferred plan nobody has launched yet must not outlive its buffer
        if getattr(self, 'pending', False):
            try:
                _lib.lib().njode_plan_flush()
            except Exception:
                pass
        pool, buf = getattr(self, 'pool', None), getattr(self, 'buf', None)
        if pool is not None and buf is not None and len(pool) < 4:
            pool.append(buf)


# =====================================================================================
# autograd bridge
# =====================================================================================
def _hT_and_loss_grads(model, call, grad_loss, grad_hT):
    """Flat parameter gradient of  grad_loss * loss + <grad_hT, hT>  for a saved forward ``call``.
    The loss term is the call's own backward (whatever plan it ran).  The hT term -- the reference
    returns hT inside its autograd graph, models.py:414-518 -- is a second pass: the same step once
    more on the LOCKSTEP plan (whose adjoint sweep can start from an upstream gradient of the final
    state: NjodeBatch.grad_hT) with the loss switched off (loss_batch_size = inf), same dropout
    seed, i.e. the same masks.  It costs a lockstep forward + backward and is only paid by a
    backward pass that really reaches hT (``train.py`` never does)."""
    grad_flat = torch.empty_like(model._flat)
    dev = model._flat.device
    if grad_loss is None:
        grad_loss = torch.zeros(1, device=dev)
    g = grad_loss.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
    model._run_backward(call, g, grad_flat)
    if grad_hT is not None:
        grad_flat += model._grad_through_hT(call, grad_hT)
    model._release_ws(call)
    return grad_flat


def _check_saved(ctx, model, call):
    """First statement of every backward: the forward's parameters and batch are still the ones it
    ran on (``NJODE._stamp``), as plain autograd checks its saved tensors.  Host-side state only: the
    parameters' version counters (``ctx.saved_tensors``), the flat vector's, the model's count of raw
    writes, the batch tensors' version counters.  On a mismatch the workspace goes back to the pool
    and nothing has been launched."""
    try:
        ctx.saved_tensors
        if call.flat is not model._flat or call.stamp != model._stamp(call):
            raise RuntimeError(
                'one of the variables needed for gradient computation has been modified by an inplace '
                'operation: the parameters (optimizer step, FusedAdam.step, a write to '
                'flat_parameters(), .to()) or the batch tensors (X, start_X, M, obs_idx, n_obs_ot) of '
                'this NJODE forward changed before its backward, which reads them again -- run the '
                'forward again, or back-propagate before the change')
    except RuntimeError:
        model._release_ws(call)
        raise


class _NJODEFunction(torch.autograd.Function):
    """(loss, hT) = F(params); backward = exact discrete adjoint (njode_backward_f32); a gradient
    that reaches hT adds the pass of ``_hT_and_loss_grads``."""

    @staticmethod
    def forward(ctx, model, call, outs, *params):
        ctx.model, ctx.call = model, call
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*params)
        # (``outs`` = the call's own fresh (loss, hT), handed over inside a tuple: returned as they are,
        # they are ordinary outputs of this node -- no copy, no launch, and no view of an input, on
        # which ``loss += reg`` or ``hT += 1`` would raise)
        return outs

    @staticmethod
    def backward(ctx, grad_loss, grad_hT):
        model, call = ctx.model, ctx.call
        _check_saved(ctx, model, call)
        grad_flat = _hT_and_loss_grads(model, call, grad_loss, grad_hT)
        return (None, None, None) + tuple(model._split_flat(grad_flat))


class _NJODEhTOnlyFunction(torch.autograd.Function):
    """hT = F(params) of a ``get_loss=False`` call: the reference's hT is differentiable there too
    (models.py:414-518).  Nothing was saved by the forward; a backward that reaches hT replays the
    step on the lockstep plan (``NJODE._grad_through_hT``)."""

    @staticmethod
    def forward(ctx, model, call, outs, *params):
        _NJODEFunction.forward(ctx, model, call, outs, *params)
        return outs[0]

    @staticmethod
    def backward(ctx, grad_hT):
        model = ctx.model
        _check_saved(ctx, model, ctx.call)
        if grad_hT is None:
            grad_flat = torch.zeros_like(model._flat)
        else:
            grad_flat = model._grad_through_hT(ctx.call, grad_hT)
        return (None, None, None) + tuple(model._split_flat(grad_flat))


# =====================================================================================
# the model's side
# =====================================================================================
class CallLayer:
    """Mixin of ``models.NJODE``: describe a call, arm it, issue it; the pools it draws from."""

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
        nh, widths, acts = self._descs[0]
        uniform = (len(set(self._descs)) == 1 and len(set(widths)) <= 1 and len(set(acts)) <= 1)
        if uniform:
            # the three networks share one hidden structure (every configuration of the
            # reference's own scripts): the compact description, which the shape-specialised
            # kernels of the build table are keyed by
            d = _lib.NjodeDims(self.input_size, self.hidden_size, self.output_size, nh,
                               widths[0] if nh else 0, acts[0] if nh else _lib.ACT_TANH, flags)
        else:
            # per-network descriptions (shape-generic kernels)
            d = _lib.NjodeDims(self.input_size, self.hidden_size, self.output_size, 0, 0, 0, flags)
            d.per_net = 1
            for i, (n, ws, as_) in enumerate(self._descs):
                if n > _lib.MAX_HIDDEN:
                    raise NotImplementedError(
                        'libnjode_hip.so runs networks with up to {} hidden layers; got {}'
                        .format(_lib.MAX_HIDDEN, n))
                d.nets[i].n_hidden = n
                for l in range(n):
                    d.nets[i].width[l] = ws[l]
                    d.nets[i].act[l] = as_[l]
        if not _lib.lib().njode_supported(ctypes.byref(d)):
            # (njode_supported leaves the shape-generic kernels' reason in njode_last_error)
            why = _lib.lib().njode_last_error().decode('utf-8', 'replace')
            raise NotImplementedError(
                'libnjode_hip.so has no gfx950 kernels for input_size={}, hidden_size={}, '
                'output_size={}, ode/enc/readout nets (n_hidden, widths, acts)={}, masked={}, '
                'input_current_t={}, residual={}, use_rnn={}: {}.  {}'
                .format(self.input_size, self.hidden_size, self.output_size, self._descs,
                        self.masked, self.input_current_t, self.residual_enc_dec,
                        self.use_rnn, why, _lib.build_info()))
        self._dims = d
        return d

    # -- workspace pool -------------------------------------------------------------------
    def _acquire_ws(self, nbytes, device):
        for slot in self._ws_pool:
            if not slot[1] and slot[0].device == device and slot[0].numel() >= nbytes:
                slot[1] = True
                return slot
        slot = [_grown(nbytes, device), True]
        # keep the pool small: drop free slots that are too small
        self._ws_pool = [s for s in self._ws_pool if s[1]] + [slot]
        return slot

    def _release_ws(self, call):
        call.release()

    def _take_ws(self, call):
        """Query the workspace of ``call`` (its sizes and flags as they stand) and take a slot."""
        need = ctypes.c_size_t(0)
        _lib.check(_lib.lib().njode_workspace_bytes(ctypes.byref(call.dims), *call.sizes, call.flags,
                                                    ctypes.byref(need)))
        call.ws_slot = self._acquire_ws(need.value, self._flat.device)
        call.ws = call.ws_slot[0]

    def _stamp(self, call):
        """The host-side state of what a saved forward's backward reads again: the flat parameter
        vector (its version counter; ``_param_writes`` for the writers that go through the raw
        pointer) and the batch tensors the call kept (the caller's own tensors where they were
        already fp32 / int32, contiguous and on the device; a copy otherwise, which nobody can
        reach).  The parameters' own version counters are held by the autograd node."""
        return (self._flat._version, self._param_writes) + tuple(t._version for t in call.inputs)

    def _track(self, call):
        call.flat = self._flat
        call.stamp = self._stamp(call)

    # -- one description of a call --------------------------------------------------------
    def _describe_call(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot, *,
                       return_path=False, get_loss=True, until_T=False, M=None, save_bwd=False,
                       rows_in_fwd=False):
        """The structs, flags and sizes of a call on this batch, its schedule packed into a pinned
        slot (``slot_i``).  Nothing is allocated on the device and nothing is counted: a plan
        description never advances the dropout stream (``_arm_call`` does, for a call)."""
        dev = start_X.device
        if dev.type != 'cuda':
            raise RuntimeError(
                'njode_amd.NJODE runs on an MI355X only (inputs are on {}); there is no '
                'CPU path. Move the model and the batch to a cuda device.'.format(dev))
        dims = self._get_dims()
        self._ensure_flat(full=True)
        if self._flat.device != dev:
            raise RuntimeError('model parameters are on {} but the batch is on {}'.format(
                self._flat.device, dev))
        if self._ring is None:
            self._ring = PinnedRing()
        B = int(start_X.shape[0])
        sched = self._sched_cache.get(times, delta_t, T, until_T)
        time_ptr = np.asarray(time_ptr, dtype=np.int32)
        assert len(times) + 1 == len(time_ptr)
        n_obs = int(time_ptr[-1])

        f32 = torch.float32
        start_X = start_X.to(f32).contiguous()
        X = X.to(device=dev, dtype=f32).contiguous()
        obs_idx_d = obs_idx.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
        keep = [start_X, X, obs_idx_d]
        M_ptr = n_ptr = None
        if self.masked:
            assert M is not None
            M = M.to(device=dev, dtype=f32).contiguous()
            keep.append(M)
            M_ptr = M.data_ptr()
        if get_loss:
            n_d = n_obs_ot.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
            keep.append(n_d)
            n_ptr = n_d.data_ptr()

        call = _Call()
        call.inputs = tuple(keep)
        call.slot_i, call.pinned = self._ring.acquire(sched.packed_nbytes())
        K, nt = sched.pack_into(call.pinned.numpy(), time_ptr)
        call.dims, call.sched = dims, sched.struct(call.pinned.data_ptr())
        call.sizes = (B, n_obs, nt, K)
        gb = float(self.dp_global_batch if self.dp_global_batch else B)
        call.batch = _lib.NjodeBatch(B, n_obs, start_X.data_ptr(), X.data_ptr() if n_obs else None,
                                     M_ptr, obs_idx_d.data_ptr() if n_obs else None, n_ptr, gb,
                                     int(self.dp_path_offset), None)
        call.flags = (
            (_lib.C_TRAIN if self.training else 0) | (_lib.C_GET_LOSS if get_loss else 0)
            | (_lib.C_RETURN_PATH if return_path else 0)
            | (_lib.C_SAVE_BWD if save_bwd else 0)
            # autograd route: the saving forward is followed by its backward, so the forward
            # runs the backward's pass over the observation rows itself (the readouts are
            # evaluated once instead of twice); carried to the backward by the flags
            | (_lib.C_ROWS_IN_FWD if (rows_in_fwd and save_bwd) else 0)
            # the plan decision travels with the call: the backward never re-reads the
            # pinned schedule buffer, which the ring may have handed to a later forward
            | _lib.C_SCHED_KNOWN | (_lib.C_SCHED_TAIL if sched.has_tail() else 0)
            # shape-generic kernels, A/B switch NJODE_GEN_PLAN=lock: read HERE, once per step,
            # and carried by the flags to the plan, the forward and the backward alike (a
            # plan prefetched under the other setting no longer matches and is dropped)
            | (_lib.C_GEN_LOCKSTEP if os.environ.get('NJODE_GEN_PLAN') == 'lock' else 0))
        call.weight, call.p_drop = float(self.weight), float(self.dropout_rate)
        call.keep = keep + [call.pinned]
        call.sched_obj, call.time_ptr = sched, time_ptr      # (what _grad_through_hT re-packs)
        call.ws_slot = call.ws = None
        return call

    def _arm_call(self, call, plan=None, plan_key=None, want_hT=True, stream=None):
        """Make a described call ready to launch: attach its prefetched plan, take its workspace,
        set its dropout seed (a training call advances ``_step_counter``).  ``plan`` = a handle
        returned by ``prefetch_plan``; else ``plan_key`` = the caller's original ``(obs_idx, time_ptr)``
        objects, looked up among the prefetched plans by identity; ``stream`` = the caller's current
        stream if it already looked it up (a lookup costs several microseconds of a step that, at
        the reference's batch sizes, the host bounds)."""
        if plan is not None or (plan_key is not None and self._plans):
            plan = self._take_plan(plan, plan_key, call.flags, call.sizes, want_hT)
        if plan is not None:
            call.batch.plan = plan.buf.data_ptr()
            call.flags |= _lib.C_PLAN_READY | (plan.flags & _lib.C_NEED_HT)
            use = stream if stream is not None else torch.cuda.current_stream(self._flat.device)
            if plan.done is not None:
                use.wait_event(plan.done)
            elif plan.stream is not None and plan.stream.cuda_stream != use.cuda_stream:
                # A deferred plan is ordered by its stream alone -- the one prefetch_plan saw.  A call
                # that consumes it on ANOTHER stream (loss_and_grad(stream=...), a torch.cuda.stream
                # context entered only around the step) would read a plan that may still be half
                # built: launch the job if it is still pending (the library runs it on its own
                # stream) and wait for that stream here.
                _lib.lib().njode_plan_flush()
                ev = torch.cuda.Event()
                ev.record(plan.stream)
                use.wait_event(ev)
            call.keep.append(plan)
        self._take_ws(call)
        # a fresh dropout stream per training forward, reproducible from `seed`
        call.seed = (self.seed * 0x9E3779B97F4A7C15 + self._step_counter) & 0xFFFFFFFFFFFFFFFF
        if self.training:
            self._step_counter += 1
        return call

    # -- the library calls ----------------------------------------------------------------
    def _run_forward(self, call, hT, loss, path_h=None, path_y=None, stream=None):
        """``njode_forward_f32`` of ``call`` -- its structs, flags, workspace and pinned slot."""
        if stream is None:
            stream = torch.cuda.current_stream()
        ptr = lambda t: t.data_ptr() if t is not None else None
        try:
            rc = _lib.lib().njode_forward_f32(
                *call.lead_args(self._flat), ptr(hT), ptr(loss), ptr(path_h), ptr(path_y),
                call.ws.data_ptr(), call.ws.numel(), stream.cuda_stream)
        finally:
            self._forward_issued(call.slot_i, stream)
        _lib.check(rc)

    def _run_backward(self, call, grad_loss, grad_flat, loss=None, stream=None):
        """``njode_backward_f32`` of ``call``; ``loss`` given: ``njode_backward_loss_f32``, the fused
        step's backward, which may also produce the loss (``NJODE_C_LOSS_IN_BWD``, see
        ``loss_and_grad``)."""
        L = _lib.lib()
        if stream is None:
            stream = torch.cuda.current_stream()
        if call.ws_slot is None:
            raise RuntimeError(
                'the workspace saved by this forward was already released: a second backward '
                'through the same NJODE forward (retain_graph) is not supported -- run the '
                'forward again')
        fn, out = ((L.njode_backward_f32, ()) if loss is None
                   else (L.njode_backward_loss_f32, (loss.data_ptr(),)))
        _lib.check(fn(*call.lead_args(self._flat), grad_loss.data_ptr(), grad_flat.data_ptr(), *out,
                      call.ws.data_ptr(), call.ws.numel(), stream.cuda_stream))

    def _grad_through_hT(self, call, grad_hT, stream=None):
        """d <grad_hT, hT> / d params (flat) for the saved forward ``call``: see
        ``_hT_and_loss_grads``.  A variant of the call -- loss switched off, lockstep plan, saving
        forward, own pinned slot and workspace -- goes through the same two functions."""
        dev = self._flat.device
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        b0 = call.batch
        B, H = call.sizes[0], self.hidden_size
        gh = grad_hT.to(device=dev, dtype=torch.float32).reshape(B, H).contiguous()
        n_ptr, n_dummy = b0.n_obs_ot, None
        if not n_ptr:     # (a get_loss=False call: the switched-off loss still wants a divisor)
            n_dummy = torch.ones(B, dtype=torch.int32, device=dev)
            n_ptr = n_dummy.data_ptr()
        v = _Call()
        v.dims, v.sizes, v.seed = call.dims, call.sizes, call.seed
        v.weight, v.p_drop = call.weight, call.p_drop
        # loss_batch_size = inf: every loss term (and its gradient) is scaled by 1 / inf = 0
        v.batch = _lib.NjodeBatch(b0.batch_size, b0.n_obs, b0.start_X, b0.X, b0.M, b0.obs_idx, n_ptr,
                                  float('inf'), b0.path_id_offset, None, None)
        v.flags = ((call.flags & (_lib.C_TRAIN | _lib.C_SCHED_KNOWN | _lib.C_SCHED_TAIL))
                   | _lib.C_GET_LOSS | _lib.C_SAVE_BWD | _lib.C_GEN_LOCKSTEP)
        self._take_ws(v)            # (before the pinned slot: a raise here holds nothing)
        try:
            v.slot_i, v.pinned = self._ring.acquire(call.sched_obj.packed_nbytes())
            call.sched_obj.pack_into(v.pinned.numpy(), call.time_ptr)
            v.sched = call.sched_obj.struct(v.pinned.data_ptr())
            hT2 = torch.empty(B, H, dtype=torch.float32, device=dev)
            loss2 = torch.zeros(1, dtype=torch.float32, device=dev)
            self._run_forward(v, hT2, loss2, stream=stream)    # (frees the pinned slot, whatever happens)
            self._last_hT_replay = hT2       # (the replayed hT: tests compare it with the call's own)
            out = torch.empty_like(self._flat)
            v.batch.grad_hT = gh.data_ptr()
            self._run_backward(v, torch.ones(1, dtype=torch.float32, device=dev), out, stream=stream)
        finally:
            self._release_ws(v)
        return out

    # -- prefetched plans -----------------------------------------------------------------
    def _plan_buffer(self, nbytes, device):
        for i, cand in enumerate(self._plan_pool):
            if cand.device == device and cand.numel() >= nbytes:
                return self._plan_pool.pop(i)     # (list.remove would compare tensors by value)
        return _grown(nbytes, device)

    def _plan_deferred(self, plan, slot_i, stream):
        """A plan was deferred: described on ``stream``, built by the next forward call there.  Its
        pinned schedule slot ``slot_i`` stays held until then.  A job that was still pending -- two
        prefetches without a forward between them -- has just been launched on ``stream`` by the
        library: its schedule slot is free behind that."""
        for p in self._deferred_slots:
            self._ring.release_after(p, stream)
        for pl in self._deferred_plans:
            pl.pending = False
        self._ring.hold(slot_i)
        self._deferred_slots[:], self._deferred_plans[:] = [slot_i], [plan]
        self._deferred_stream = stream

    def _forward_issued(self, slot_i, stream):
        """An ``njode_forward_f32`` call was issued on ``stream`` with pinned slot ``slot_i``: the
        slot is free once ``stream`` has passed it -- and so are the slots of deferred plans, which
        that call hosted or launched."""
        self._ring.release_after(slot_i, stream)
        ds = self._deferred_stream
        for p in self._deferred_slots:
            if ds is not None and ds.cuda_stream != stream.cuda_stream:
                self._ring.release_after(p, ds)     # (the job ran on the stream it was described on)
            else:
                self._ring.release_with(p, slot_i)
        del self._deferred_slots[:]
        for pl in self._deferred_plans:
            pl.pending = False
        del self._deferred_plans[:]

    def _take_plan(self, plan, key, flags, sizes, want_hT):
        """The prefetched plan of this call, or None (the call then builds its own in line).
        ``plan`` given: the handle ``prefetch_plan`` returned; else the oldest queued plan whose
        ``obs_idx`` / ``time_ptr`` ARE (identity) the caller's objects.  A plan that was made for
        a different kind of call (sizes, flags, no tail order although hT is wanted) or whose
        ``obs_idx`` was modified in place since is dropped, never used and never left to block
        the plans queued behind it."""
        if plan is None:
            obs_idx, time_ptr = key
            for cand in self._plans:
                if cand.obs_idx is obs_idx and cand.time_ptr is time_ptr:
                    plan = cand
                    break
            if plan is None:
                return None
        if plan.taken:
            raise RuntimeError('this prefetched plan was already consumed by an earlier call')
        if plan in self._plans:
            self._plans.remove(plan)
        plan.taken = True
        want = flags & ~(_lib.C_LOSS_IN_BWD | _lib.C_PLAN_READY | _lib.C_ROWS_IN_FWD)
        ok = (plan.sizes == sizes and (plan.flags & ~_lib.C_NEED_HT) == want
              and getattr(plan.obs_idx, '_version', 0) == plan.obs_version
              and (not want_hT or self.masked or (plan.flags & _lib.C_NEED_HT)))
        return plan if ok else None
