"""Helpers of the tests of online filtering on the shape-generic kernels (a helper module, not a
conftest): the model shapes, their batches, and the float64 truth per series (``online_util``)."""
import numpy as np
import torch

import gen_envelope
import hip_util
import online_util
from njode_amd import _lib, synthetic_physionet
from njode_amd.build import CONFIGS

T_ = _lib.ACT_TANH


def _cfg(d, H, ode, enc, dec, d_out=None, use_rnn=False, **options):
    return dict(input_size=d, hidden_size=H, output_size=d if d_out is None else d_out, ode_nn=ode, readout_nn=dec,
                enc_nn=enc, use_rnn=use_rnn, bias=True, dropout_rate=0.0, options=options)


def _w(n, act='tanh', layers=2):
    return tuple((n, act) for _ in range(layers))


# name -> model config.  What each one is for (njode_gen.h / njode_gen_online.h):
SHAPES = {
    'w80': _cfg(1, 10, _w(80), _w(80), _w(80)),                       # short fragment rows, 5 output tiles
    'w160': _cfg(1, 10, _w(160), _w(160), _w(160)),                   # layer input 161: the long-row ring
    'none_h100': _cfg(1, 100, None, None, None),                      # single-Linear networks
    'deep_relu_curt': _cfg(1, 12, _w(24, 'relu', 4), _w(24, 'relu', 4), _w(24, 'relu', 4),
                           residual_enc_dec=False, input_current_t=True),
    'one_layer_easy': _cfg(2, 6, _w(70, 'tanh', 1), _w(18, 'relu', 1), _w(65, 'tanh', 1), which_loss='easy'),
    'gru_w80': _cfg(1, 10, _w(80), _w(80), _w(80), use_rnn=True),
    'gru_d2_h24': _cfg(2, 24, _w(33), _w(20, 'relu', 1), _w(72, 'tanh', 3), use_rnn=True, residual_enc_dec=False),
    'd8_h4': _cfg(8, 4, _w(20), _w(33, 'relu', 1), None, masked=True),  # encoder residual case 2
    'gru_masked': _cfg(5, 10, hip_util.NN50, hip_util.NN50, hip_util.NN50, use_rnn=True, masked=True),   # g15_rnn_masked's
    'out5': _cfg(1, 10, hip_util.NN50, hip_util.NN50, hip_util.NN50, d_out=5),   # g14_out5's: d_out != d
    'climate_w400_h50': _cfg(5, 50, _w(400), _w(400), _w(400), masked=True),
}
for _i in (online_util.DEMO, online_util.PHYSIO):
    SHAPES['cfg{}'.format(_i)] = online_util.model_cfg(CONFIGS[_i])

# shapes whose batch calls run the generic family as well, which is every shape outside the build
# table (the C ABI routes whatever it has no specialisation for to gen_forward): all but cfg0 / cfg6
GENERIC_BATCH = [name for name in sorted(SHAPES) if not name.startswith('cfg')]

# shapes the generic online family must refuse, as (D, H, DO, nets, flags) of gen_envelope.restate
_NN = (2, (50, 50), (T_, T_))
REFUSED = {
    'masked_d_ne_dout': (3, 10, 2, _NN, _lib.F_MASKED),
    'residual_mismatch': (3, 10, 3, _NN, _lib.F_RESIDUAL),
    'rnn_4h_above_1024': (1, 300, 1, _NN, _lib.F_USE_RNN),
    'lds_overflow': (1, 229, 1, (2, (1024, 1024), (T_, T_)), 0),
}


# build_model accepts it (163 648 bytes of LDS), and the 576 bytes of per-chain clocks do not fit behind
LDS_WINDOW = (4, 618, 4, (0, (), ()), 0)


def is_masked(cfg):
    return bool(cfg['options'].get('masked', False))


def raw_of_cfg(cfg):
    """(D, H, DO, nets, flags) of a model config."""
    nets, flags = gen_envelope.nets_of_cfg(cfg)
    return cfg['input_size'], cfg['hidden_size'], cfg['output_size'], nets, flags


def make_model(name, seed=0):
    cfg = SHAPES[name]
    sd = online_util.params_of(cfg, seed=seed)
    return cfg, sd, hip_util.hip_model(cfg, sd).eval()


def make_batch(cfg, N, seed=0):
    """(batch, delta_t, T): the smallest batches that take every branch of a shape."""
    d = cfg['input_size']
    if is_masked(cfg):
        b = synthetic_physionet.make_batch(batch_size=N, dim=d, n_grid=40, n_obs_range=(3, 6), seed=seed)
        b['start_X'] = 0.1 * torch.randn(N, d, generator=torch.Generator().manual_seed(seed))
        return b, b['delta_t'], b['T']
    return hip_util.exact_k_batch(N, 12, obs_per_path=3, seed=seed, d=d)


def slices(b):
    ptr = np.asarray(b['time_ptr'])
    for i, t in enumerate(np.asarray(b['times'], dtype=np.float64)):
        lo, hi = int(ptr[i]), int(ptr[i + 1])
        if hi > lo:
            yield float(t), lo, hi, b['obs_idx'][lo:hi].numpy()


def bits(st):
    return [t.clone() for t in (st.h, st.last_X, st.tau, st.now)]


def eq_bits(x, y):
    """Same shape, same bytes (NaN payloads and signed zeros included)."""
    return x.shape == y.shape and torch.equal(x.reshape(-1).contiguous().view(torch.uint8),
                                              y.reshape(-1).contiguous().view(torch.uint8))


def same_bits(a, b):
    return len(a) == len(b) and all(eq_bits(x, y) for x, y in zip(a, b))


def online(m, N, delta_t, spt=None):
    st = m.online(N, delta_t, kernels='generic')
    st.series_per_tile = spt
    return st
