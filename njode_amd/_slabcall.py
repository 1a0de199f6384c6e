"""
The call scaffold of the routes that walk every path and sweep it backwards into gradient slabs
(``float64.NJODE64``, ``gru_ode_bayes.NNFOwithBayesianJumps``): the holder of one call, the
autograd node of a saved forward, and the steps around issuing a forward.  A model of these routes
is a ``_flat.FlatVector`` with a ``PinnedRing`` or ``None`` in ``_ring``, the text of
``_moved_error`` and ``_backward_into(call, grads, grad_flat)``, its backward library call.
"""
import contextlib
import ctypes

import torch

from . import _lib
from .schedule import PinnedRing


class _SlabCall:
    """One forward call: structs, flags, the buffers they point into and the workspace, kept alive
    for the backward.  ``extra``: the route's own scalars."""
    __slots__ = ('dims', 'batch', 'sched', 'flags', 'sizes', 'ws', 'keep', 'flat', 'extra')


class _SlabFunction(torch.autograd.Function):
    """outs = F(params), ``outs`` the forward's own fresh outputs; backward = the exact discrete
    adjoint of the route (``model._backward_into``), which takes every upstream gradient."""

    @staticmethod
    def forward(ctx, model, call, outs, *params):
        ctx.model, ctx.call = model, call
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*params)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        model, call = ctx.model, ctx.call
        ctx.saved_tensors       # (autograd's own check: the parameters are the forward's)
        if call.flat is not model._flat:
            raise RuntimeError(model._moved_error)
        grad_flat = torch.empty_like(call.flat)
        model._backward_into(call, grads, grad_flat)
        return (None, None, None) + tuple(model._split_flat(grad_flat))


@contextlib.contextmanager
def issuing(model, call, sched, time_ptr, workspace_bytes):
    """Around a forward library call of ``call`` (``dims``, ``sizes``, ``flags`` set): packs
    ``sched`` with ``time_ptr`` into a pinned slot (``call.sched``), allocates the workspace
    ``workspace_bytes`` (the route's query function) asks for (``call.ws``), pins the flat vector
    (``call.flat``) and yields the current stream; the pinned slot is free once that stream has
    passed, whatever the body did."""
    dev = model._flat.device
    if model._ring is None:
        model._ring = PinnedRing()
    slot, pinned = model._ring.acquire(sched.packed_nbytes())
    sched.pack_into(pinned.numpy(), time_ptr)
    call.sched = sched.struct(pinned.data_ptr())
    need = ctypes.c_size_t(0)
    _lib.check(workspace_bytes(ctypes.byref(call.dims), *call.sizes, call.flags, ctypes.byref(need)))
    call.ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    call.flat = model._flat
    stream = torch.cuda.current_stream(dev)
    try:
        yield stream
    finally:
        model._ring.release_after(slot, stream)      # (the pinned schedule: free once the stream passed)
