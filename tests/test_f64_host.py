"""Host side of the float64 route (``include/njode_f64.h``, ``njode_amd/float64.py``): what needs no GPU.
The envelope query and its reasons, the workspace promise's sanity, every refusal the two calls make
before they launch anything, and the Python twin's parameters."""
import ctypes
import os

import numpy as np
import pytest
import torch

from njode_amd import _lib, models

NN50 = ((50, 'tanh'), (50, 'tanh'))
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libnjode_hip.so not built')


def _cfg(d=1, H=10, DO=1, nn=NN50, use_rnn=False, bias=True, dropout=0.0, **options):
    return dict(input_size=d, hidden_size=H, output_size=DO, ode_nn=nn, readout_nn=nn, enc_nn=nn,
                use_rnn=use_rnn, bias=bias, dropout_rate=dropout, options=options)


def _dims(d=1, H=10, DO=1, nh=2, w=50, act=0, flags=_lib.F_RESIDUAL):
    return _lib.NjodeDims(d, H, DO, nh, w, act, flags)


def _why():
    return _lib.lib().njode_last_error().decode()


@needs_lib
def test_supported_envelope_and_reasons():
    L = _lib.lib()
    ok = [_dims(), _dims(flags=0), _dims(flags=_lib.F_RESIDUAL | _lib.F_INPUT_CURRENT_T | _lib.F_LOSS_EASY),
          _dims(41, 41, 41, flags=_lib.F_MASKED | _lib.F_RESIDUAL), _dims(41, 50, 41, flags=_lib.F_MASKED),
          _dims(1, 10, 1, nh=0, w=0), _dims(1, 10, 1, nh=8, w=24, act=_lib.ACT_RELU),
          _dims(1, 10, 5), _dims(2, 10, 20), _dims(3, 7, 3, flags=0), _dims(1, 10, 1, w=1024)]
    for d in ok:
        assert L.njode_f64_supported(ctypes.byref(d)) == 1, _why()
        # ... the same verdict as the fp32 library gives on these
        assert L.njode_supported(ctypes.byref(d)) == 1
    per = _dims(2, 6, 2, nh=0, w=0)
    per.per_net = 1
    per.nets[0].n_hidden = 3
    for l, (w, a) in enumerate(((48, 0), (40, 1), (72, 0))):
        per.nets[0].width[l], per.nets[0].act[l] = w, a
    per.nets[2].n_hidden = 1
    per.nets[2].width[0], per.nets[2].act[0] = 16, 1
    assert L.njode_f64_supported(ctypes.byref(per)) == 1, _why()

    refused = [(_dims(flags=_lib.F_RESIDUAL | _lib.F_USE_RNN), 'use_rnn'),
               (_dims(3, 7, 3), 'residual'), (_dims(3, 6, 5, flags=_lib.F_MASKED), 'input_size must equal'),
               (_dims(600, 10, 600, flags=0), 'out of range'), (_dims(1, 10, 1, nh=9), 'n_hidden'),
               (_dims(1, 10, 1, w=2000), 'network description'), (_dims(1, 10, 1, act=7), 'network description')]
    for d, word in refused:
        assert L.njode_f64_supported(ctypes.byref(d)) == 0
        assert word in _why(), (word, _why())
    assert L.njode_f64_supported(None) == 0 and 'null' in _why()


@needs_lib
def test_workspace_bytes_sanity_and_badarg():
    L = _lib.lib()
    d = _dims()
    out = ctypes.c_size_t(0)

    def need(B, n_obs, nt, K, flags):
        assert L.njode_f64_workspace_bytes(ctypes.byref(d), B, n_obs, nt, K, flags, ctypes.byref(out)) == 0, _why()
        return out.value

    P = 10071
    base = need(64, 600, 100, 100, _lib.C_GET_LOSS)
    assert base % 256 == 0 and base >= 8 * P + 4 * 64 * 100        # the transposed table, the row table
    save = need(64, 600, 100, 100, _lib.C_GET_LOSS | _lib.C_SAVE_BWD)
    # states before every step and jump, and one gradient slab per path (B <= the slab limit)
    assert save >= base + 8 * (100 * 64 * 10 + 600 * 11) + 8 * 64 * P
    assert need(128, 600, 100, 100, _lib.C_GET_LOSS | _lib.C_SAVE_BWD) > save
    assert need(64, 600, 100, 200, _lib.C_GET_LOSS | _lib.C_SAVE_BWD) > save
    assert need(64, 600, 100, 100, _lib.C_GET_LOSS | _lib.C_RETURN_PATH) == base       # paths are outputs
    assert need(1, 0, 0, 0, 0) > 0
    # the slab count is capped: 20 000 paths need less than 20 000 slabs
    assert need(20000, 100, 10, 10, _lib.C_SAVE_BWD) < 8 * 20000 * P
    for args in ((0, 1, 1, 1, 0), (4, -1, 1, 1, 0), (4, 1, -1, 1, 0), (4, 1, 1, -1, 0), (4, 1, 1, 1, _lib.C_TRAIN),
                 (4, 1, 1, 1, _lib.C_PLAN_READY)):
        assert L.njode_f64_workspace_bytes(ctypes.byref(d), *args, ctypes.byref(out)) == _lib.E_BADARG, args
    assert L.njode_f64_workspace_bytes(ctypes.byref(d), 4, 1, 1, 1, 0, None) == _lib.E_BADARG
    rnn = _dims(flags=_lib.F_USE_RNN)
    assert L.njode_f64_workspace_bytes(ctypes.byref(rnn), 4, 1, 1, 1, 0, ctypes.byref(out)) == _lib.E_UNSUPPORTED
    assert 'use_rnn' in _why()


class _HostCall:
    """A well-formed call on fake device addresses (never dereferenced: every refusal precedes the
    first launch) with a real host schedule."""

    def __init__(self, masked=False):
        self.dims = _dims(3, 6, 3, flags=_lib.F_MASKED if masked else 0)
        self.K, self.nt, self.B, self.n_obs = 4, 2, 3, 4
        self.step_dt = np.full(4, 0.25)
        self.step_t = np.arange(4, dtype=np.float32) * 0.25
        self.k_jump = np.array([2, 4], dtype=np.int32)
        self.time_f32 = np.array([0.5, 1.0], dtype=np.float32)
        self.time_ptr = np.array([0, 2, 4], dtype=np.int32)
        fake = 1 << 20
        self.batch = _lib.NjodeBatch64(self.B, self.n_obs, fake, fake, fake if masked else None, fake, fake, 3.0)
        self.ws, self.ws_bytes = fake, 1 << 40
        self.flags = _lib.C_GET_LOSS | _lib.C_SAVE_BWD
        self.params = self.hT = self.loss = self.grad = self.grad_loss = fake

    def sched(self):
        p = lambda a: a.ctypes.data
        return _lib.NjodeSchedule64(self.K, self.nt, p(self.step_dt), p(self.step_t), p(self.k_jump),
                                    p(self.time_f32), p(self.time_ptr))

    def forward(self, path=(None, None)):
        s = self.sched()
        return _lib.lib().njode_forward_f64(ctypes.byref(self.dims), self.params, ctypes.byref(self.batch),
                                            ctypes.byref(s), self.flags, 0.5, self.hT, self.loss, *path, self.ws,
                                            self.ws_bytes, None)

    def backward(self):
        s = self.sched()
        return _lib.lib().njode_backward_f64(ctypes.byref(self.dims), self.params, ctypes.byref(self.batch),
                                             ctypes.byref(s), self.flags, 0.5, self.grad_loss, None, self.grad,
                                             self.ws, self.ws_bytes, None)


def _mut(**kw):
    def apply(c):
        for k, v in kw.items():
            if k.startswith('batch_'):
                setattr(c.batch, k[6:], v)
            else:
                setattr(c, k, v)
    return apply


@needs_lib
def test_forward_refuses_before_launch():
    cases = [
        (_mut(params=None), 'null params'), (_mut(batch_start_X=None), 'null batch array'),
        (_mut(batch_X=None), 'null batch array'), (_mut(batch_obs_idx=None), 'null batch array'),
        (_mut(batch_batch_size=0), 'negative size'), (_mut(batch_n_obs=-1), 'negative size'), (_mut(K=-1), 'negative size'),
        (_mut(batch_n_obs_ot=None), 'n_obs_ot'), (_mut(batch_loss_batch_size=0.0), 'loss_batch_size'),
        (_mut(loss=None), 'null output'), (_mut(flags=_lib.C_GET_LOSS | _lib.C_TRAIN), 'call flag'),
        (_mut(flags=_lib.C_GET_LOSS | _lib.C_PLAN_READY), 'call flag'),
        (_mut(flags=_lib.C_GET_LOSS | _lib.C_RETURN_PATH), 'null output'),
        (_mut(ws=None), 'workspace'), (_mut(ws=(1 << 20) + 8), 'aligned'),
        (_mut(time_ptr=np.array([0, 3, 2], dtype=np.int32)), 'time_ptr'),
        (_mut(time_ptr=np.array([0, 2, 3], dtype=np.int32)), 'time_ptr'),
        (_mut(k_jump=np.array([3, 2], dtype=np.int32)), 'k_jump'), (_mut(k_jump=np.array([2, 5], dtype=np.int32)), 'k_jump'),
    ]
    for mut, word in cases:
        c = _HostCall()
        mut(c)
        assert c.forward() == _lib.E_BADARG, word
        assert word in _why(), (word, _why())
    c = _HostCall(masked=True)
    c.batch.M = None
    assert c.forward() == _lib.E_BADARG and 'M' in _why()
    c = _HostCall()
    c.dims = _dims(3, 6, 5, flags=0)        # output_size != input_size: prediction calls only
    assert c.forward() == _lib.E_BADARG and 'input_size == output_size' in _why()
    c = _HostCall()
    c.ws_bytes = 1024
    assert c.forward() == _lib.E_WORKSPACE and 'too small' in _why()
    c = _HostCall()
    c.dims = _dims(3, 6, 3, flags=_lib.F_USE_RNN)
    assert c.forward() == _lib.E_UNSUPPORTED and 'use_rnn' in _why()
    c = _HostCall()
    s = c.sched()
    L = _lib.lib()
    assert L.njode_forward_f64(ctypes.byref(c.dims), c.params, None, ctypes.byref(s), c.flags, 0.5, c.hT, c.loss,
                               None, None, c.ws, c.ws_bytes, None) == _lib.E_BADARG
    assert L.njode_forward_f64(ctypes.byref(c.dims), c.params, ctypes.byref(c.batch), None, c.flags, 0.5, c.hT,
                               c.loss, None, None, c.ws, c.ws_bytes, None) == _lib.E_BADARG


@needs_lib
def test_backward_refuses_before_launch():
    cases = [
        (_mut(params=None), 'null params'), (_mut(grad=None), 'grad_params'), (_mut(grad_loss=None), 'grad_loss'),
        (_mut(flags=_lib.C_GET_LOSS), 'SAVE_BWD'),
        (_mut(flags=_lib.C_GET_LOSS | _lib.C_SAVE_BWD | _lib.C_RETURN_PATH), 'RETURN_PATH'),
        (_mut(flags=_lib.C_GET_LOSS | _lib.C_SAVE_BWD | _lib.C_LOSS_IN_BWD), 'call flag'),
        (_mut(batch_start_X=None), 'null batch array'), (_mut(batch_n_obs_ot=None), 'n_obs_ot'),
        (_mut(ws=None), 'workspace'), (_mut(batch_batch_size=-2), 'negative size'),
    ]
    for mut, word in cases:
        c = _HostCall()
        mut(c)
        assert c.backward() == _lib.E_BADARG, word
        assert word in _why(), (word, _why())
    c = _HostCall()
    c.ws_bytes = 1024
    assert c.backward() == _lib.E_WORKSPACE
    c = _HostCall()
    c.dims = _dims(3, 6, 3, flags=_lib.F_USE_RNN)
    assert c.backward() == _lib.E_UNSUPPORTED and 'use_rnn' in _why()


# ---- the Python twin -------------------------------------------------------------------------------
@needs_lib
@pytest.mark.parametrize('cfg', [_cfg(), _cfg(41, 41, 41, masked=True), _cfg(2, 6, 2, nn=None),
                                 _cfg(1, 10, 1, bias=False), _cfg(1, 10, 5, nn=((32, 'relu'), (16, 'tanh')))],
                         ids=['demo', 'masked', 'linear', 'nobias', 'out5'])
def test_twin_keys_dtypes_and_flat_layout(cfg):
    from njode_amd.float64 import NJODE64
    ref, m = models.NJODE(**cfg), NJODE64(**cfg)
    assert list(m.state_dict()) == list(ref.state_dict())
    assert [tuple(p.shape) for p in m.parameters()] == [tuple(p.shape) for p in ref.parameters()]
    flat = m.flat_parameters()
    assert flat.dtype == torch.float64 and flat.dim() == 1
    # the C ABI's order with bias slots present: the parameter count the fp32 library states
    assert flat.numel() == _lib.lib().njode_param_count(ctypes.byref(ref._get_dims()))
    off = 0
    for seq in (m.ode_f.f, m.encoder_map.ffnn, m.readout_map.ffnn):
        for lin in (x for x in seq if isinstance(x, torch.nn.Linear)):
            assert lin.weight.dtype == torch.float64
            assert lin.weight.data_ptr() == flat.data_ptr() + 8 * off
            off += lin.weight.numel()
            if lin.bias is not None:
                assert lin.bias.dtype == torch.float64 and lin.bias.data_ptr() == flat.data_ptr() + 8 * off
            else:
                assert torch.count_nonzero(flat[off:off + lin.out_features]) == 0
            off += lin.out_features
    assert off == flat.numel()
    # a write through a parameter is a write to the flat vector; genuine float64 weights load exactly
    sd = {k: v + 2.0 ** -40 for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    assert m._views_in_place() and m.flat_parameters() is flat
    for k, p in m.named_parameters():
        assert torch.equal(p, sd[k])
        if k.endswith('weight'):        # (no fp32 number: nothing rounded the loaded values)
            assert (p.float().double() != p).any()
    # plain torch.optim works on the views
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = flat.clone()
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    assert m._views_in_place() and not torch.equal(before, flat)
    assert m.weight_decay_step() == 0.5 and m.epoch == 1


@needs_lib
def test_float64_widens_exactly():
    cfg = _cfg(41, 41, 41, masked=True, which_loss='easy')
    cfg.update(weight=0.75, weight_decay=0.9)
    ref = models.NJODE(**cfg)
    ref.epoch = 7
    ref.eval()
    torch.manual_seed(11)
    after = torch.rand(3)
    torch.manual_seed(11)
    twin = ref.float64()
    assert torch.equal(torch.rand(3), after)        # (the twin's throw-away initial weights drew nothing here)
    from njode_amd.float64 import NJODE64
    assert isinstance(twin, NJODE64) and not twin.training and twin.epoch == 7
    assert (twin.weight, twin.weight_decay, twin.which_loss, twin.masked) == (0.75, 0.9, 'easy', True)
    for (k, p), (k2, q) in zip(ref.named_parameters(), twin.named_parameters()):
        assert k == k2 and q.dtype == torch.float64 and torch.equal(q, p.detach().double())
        assert q.data_ptr() != p.data_ptr()
    # model.double() stays what it was: the flat vector the kernels read is fp32
    assert next(ref.parameters()).dtype == torch.float32


@needs_lib
def test_refusals_of_the_twin():
    from njode_amd.float64 import NJODE64
    with pytest.raises(NotImplementedError, match='use_rnn'):
        NJODE64(**_cfg(use_rnn=True))
    with pytest.raises(NotImplementedError, match='use_rnn'):
        models.NJODE(**_cfg(use_rnn=True)).float64()
    m = NJODE64(**_cfg(dropout=0.1))
    x = torch.zeros(2, 1)
    args = (np.array([0.5]), np.array([0, 1]), x[:1], torch.zeros(1, dtype=torch.long), 0.1, 1.0, x, torch.ones(2))
    with pytest.raises(NotImplementedError, match='dropout'):
        m.train()(*args)
    # eval mode is not refused for its dropout rate: it gets as far as the device check
    with pytest.raises(RuntimeError, match='no CPU path'):
        m.eval()(*args)
