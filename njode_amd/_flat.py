"""
Flat parameter storage: every parameter of a model is a view of one vector laid out as the C ABI
expects, so the kernels read one pointer and the gradient comes back as one vector.
``lay_out_flat`` makes the vector; ``FlatVector`` is the storage of the float64 route and of
GRU-ODE-Bayes, ``FlatParams`` that of ``models.NJODE`` (fp32, with the hot loop's fast path).
"""
import copy

import torch


def lay_out_flat(slots, dtype):
    """``slots`` = [(parameter or None, slot size, shape)] in the C ABI's order -> (flat, slices,
    params, present): one ``dtype`` vector holding the parameters' values, which become views of it;
    ``(offset, size, shape)`` and the parameter of every slot that has one; ``present``: a mask with
    zeros over the slots that have none (``None`` when every slot has one)."""
    dev = slots[0][0].device
    total = sum(n for _, n, _ in slots)
    flat = torch.zeros(total, dtype=dtype, device=dev)
    slices, params, off, present = [], [], 0, None
    for p, n, shape in slots:
        if p is not None:
            flat[off:off + n].copy_(p.data.reshape(-1).to(dtype))
            p.data = flat[off:off + n].view(shape)
            slices.append((off, n, shape))
            params.append(p)
        else:
            # a slot without a parameter (bias=False, models.py:140-166): the kernels read it
            # as zeros and WRITE its gradient; it is not a parameter, so the fused optimizer
            # must leave it alone (FusedAdam.step multiplies the gradient by this mask)
            if present is None:
                present = torch.ones(total, dtype=dtype, device=dev)
            present[off:off + n] = 0.0
        off += n
    return flat, slices, params, present


class FlatVector:
    """Base of a ``torch.nn.Module`` (named before it) whose kernel parameters are ``_flat_dtype``
    views of one flat vector: ``_flat``, ``_flat_params``, ``_param_slices``.  The model says which
    parameters, in ``_flat_slots()``, and sets the three attributes to ``None`` before it creates
    its parameters."""
    _flat_dtype = torch.float32

    def _views_in_place(self, which=None):
        """Whether the parameters (``which``: indices, default all) still are views of the flat vector."""
        if self._flat is None:
            return False
        base, size = self._flat.data_ptr(), self._flat.element_size()
        for i in range(len(self._flat_params)) if which is None else which:
            p = self._flat_params[i]
            if p.data_ptr() != base + size * self._param_slices[i][0] or p.dtype != self._flat_dtype:
                return False
        return True

    def _ensure_flat(self):
        """Every kernel parameter a view of one flat vector (values are kept; a parameter of another
        dtype is converted).  Re-done after ``.to()`` / ``.cuda()`` moved the parameters."""
        if not self._views_in_place():
            self._flat, self._param_slices, self._flat_params, _ = lay_out_flat(self._flat_slots(),
                                                                                self._flat_dtype)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        if getattr(self, '_flat', None) is not None:
            self._ensure_flat()
        return out

    def _split_flat(self, flat):
        """A flat vector (gradient) as views shaped like the parameters, in ``_flat_params`` order."""
        return [flat[off:off + n].view(shape) for (off, n, shape) in self._param_slices]

    def flat_parameters(self):
        """The flat vector the kernels' parameters are views of."""
        self._ensure_flat()
        return self._flat

    def _fresh_runtime_state(self):
        """Hook: set what a new model and a copy of one start without (``_ring`` and ``_schedules``
        are ``None`` in a copy when this is called)."""

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        skip = ('_flat', '_param_slices', '_flat_params', '_ring', '_schedules')
        for k, v in self.__dict__.items():
            new.__dict__[k] = None if k in skip else copy.deepcopy(v, memo)
        new._fresh_runtime_state()
        new._ensure_flat()
        return new


class FlatParams:
    """Mixin of ``models.NJODE`` (``_flat``, ``_flat_params``, ``_param_slices``, ``_flat_present``)."""

    def _apply(self, fn, *args, **kwargs):
        """.to() / .cuda() / .float() move the parameters: the flat vector is rebuilt on next use."""
        out = super()._apply(fn, *args, **kwargs)
        self._flat_checks = 63          # next _ensure_flat walks all parameters
        return out

    def _flat_slots(self):
        """[(parameter or None, slot size, shape)] in the C ABI's order: the Linear
        layers of the three networks (bias slot always present), then the GRU cell."""
        slots = []
        for seq in (self.ode_f.f, self.encoder_map.ffnn, self.readout_map.ffnn):
            for m in seq:
                if isinstance(m, torch.nn.Linear):
                    slots.append((m.weight, m.weight.numel(), tuple(m.weight.shape)))
                    slots.append((m.bias, m.out_features, (m.out_features,)))
        if self.use_rnn:
            g = self.obs_c.gru_d
            H3 = 3 * self.hidden_size
            slots.append((g.weight_ih, g.weight_ih.numel(), tuple(g.weight_ih.shape)))
            slots.append((g.weight_hh, g.weight_hh.numel(), tuple(g.weight_hh.shape)))
            slots.append((getattr(g, 'bias_ih', None), H3, (H3,)))
            slots.append((getattr(g, 'bias_hh', None), H3, (H3,)))
        return slots

    def _views_in_place(self, which):
        """Whether the parameters ``which`` (indices) still are fp32 views of the flat vector."""
        base = self._flat.data_ptr()
        for i in which:
            p = self._flat_params[i]
            if p.data_ptr() != base + 4 * self._param_slices[i][0] or p.dtype != torch.float32:
                return False
        return True

    def _ensure_flat(self, full=False):
        """Make every parameter a view of one flat vector laid out as the C ABI expects
        (state_dict order; bias slots always present).  ``full``: walk all parameters (once per
        library call, from ``_describe_call``: a parameter re-pointed by ``p.data = ...`` or
        ``load_state_dict(assign=True)`` is caught before the kernels read the flat vector)."""
        if self._flat is not None and self._flat_params:
            # fast path (the hot loop calls this several times per step): first and last parameter
            # still sit where they were put; the full walk runs once per call, every 64th check
            # and after _apply()
            if not full:
                self._flat_checks += 1
                if self._flat_checks & 63 and self._views_in_place((0, -1)):
                    return
            if self._views_in_place(range(len(self._flat_params))):
                return
        self._flat, self._param_slices, self._flat_params, self._flat_present = lay_out_flat(
            self._flat_slots(), torch.float32)
        self._flat_grad = self._grad_bucket = None

    _split_flat = FlatVector._split_flat
