"""
Flat parameter storage of ``models.NJODE``: every parameter is a view of one fp32 vector laid out
as the C ABI expects, so the kernels read one pointer and the gradient comes back as one vector.
"""
import torch


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
        slots = self._flat_slots()
        dev = slots[0][0].device
        total = sum(n for _, n, _ in slots)
        flat = torch.zeros(total, dtype=torch.float32, device=dev)
        slices, params, off, present = [], [], 0, None
        for p, n, shape in slots:
            if p is not None:
                flat[off:off + n].copy_(p.data.reshape(-1).to(torch.float32))
                p.data = flat[off:off + n].view(shape)
                slices.append((off, n, shape))
                params.append(p)
            else:
                # a slot without a parameter (bias=False, models.py:140-166): the kernels read it
                # as zeros and WRITE its gradient; it is not a parameter, so the fused optimizer
                # must leave it alone (FusedAdam.step multiplies the gradient by this mask)
                if present is None:
                    present = torch.ones(total, dtype=torch.float32, device=dev)
                present[off:off + n] = 0.0
            off += n
        self._flat, self._param_slices, self._flat_params = flat, slices, params
        self._flat_present = present
        self._flat_grad = self._grad_bucket = None

    def _split_flat(self, flat):
        """A flat vector (gradient) as views shaped like the parameters, in ``_flat_params`` order."""
        return [flat[off:off + n].view(shape) for (off, n, shape) in self._param_slices]
