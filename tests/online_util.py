"""Helpers of the online-filtering tests (a helper module, not a conftest): the float64 truth of a
series is the oracle's forward on the batch that consists of that series alone, with ``times`` =
the targets of the calls in order; a call without an observation is an empty time slice."""
import numpy as np
import torch

import hip_util
from njode_amd import schedule
from njode_amd.build import CONFIGS, RELU
from oracle import njode_oracle

# rows of njode_amd.build.CONFIGS the online kernel runs: two hidden layers, no GRU jump
ACCEPTED = [i for i, c in enumerate(CONFIGS) if c[3] == 2 and not c[9]]
REFUSED = [i for i in range(len(CONFIGS)) if i not in ACCEPTED]
DEMO, PHYSIO = 0, 6     # the demo shape and the PhysioNet shape (one per kernel family)


def model_cfg(c):
    d, H, DO, nh, W, act, masked, curt, res, rnn = c
    nn = None if nh == 0 else tuple((W, 'relu' if act == RELU else 'tanh') for _ in range(nh))
    opts = {'masked': bool(masked), 'input_current_t': bool(curt), 'residual_enc_dec': bool(res)}
    return dict(input_size=d, hidden_size=H, output_size=DO, ode_nn=nn, readout_nn=nn, enc_nn=nn,
                use_rnn=bool(rnn), bias=True, dropout_rate=0.0, options=opts)


def params_of(cfg, seed=0):
    """The oracle's initial parameters with non-zero biases (a wrong bias offset must show)."""
    sd = njode_oracle.make_oracle(cfg).init_params(seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in sd:
        if k.endswith('bias'):
            sd[k] = (0.1 * torch.randn(sd[k].shape, generator=g)).float()
    return sd


def series_events(b, s):
    """[(t, x row, m row or None)] of series ``s`` of a collated batch, in time order."""
    ptr, idx = np.asarray(b['time_ptr']), b['obs_idx'].numpy()
    out = []
    for i, t in enumerate(np.asarray(b['times'], dtype=np.float64)):
        for r in range(int(ptr[i]), int(ptr[i + 1])):
            if idx[r] == s:
                out.append((float(t), b['X'][r], b['M'][r] if 'M' in b else None))
    return out


def batch_of_one(events, start_x, d, masked):
    """The batch of one series: ``events`` = [(t, x or None, m or None)]; x None: an empty slice."""
    times = np.asarray([e[0] for e in events], dtype=np.float64)
    rows = [e for e in events if e[1] is not None]
    ptr = np.concatenate([[0], np.cumsum([e[1] is not None for e in events])]).astype(np.int64)
    X = torch.stack([e[1] for e in rows]).float() if rows else torch.zeros(0, d)
    b = dict(times=times, time_ptr=ptr, X=X, obs_idx=torch.zeros(len(rows), dtype=torch.long),
             start_X=start_x.reshape(1, d).float(), n_obs_ot=torch.tensor([max(len(rows), 1)]))
    if masked:
        b['M'] = torch.stack([e[2] for e in rows]).float() if rows else torch.zeros(0, d)
    return b


def truth(cfg, sd, events, start_x, delta_t, T=None):
    """(o32, o64, rows): the oracle pair of the batch of one (prediction call, ``until_T`` when a
    ``T`` is given) and the path row of every event; the row before it holds the state the event
    meets and its readout (``Y_before``)."""
    b = batch_of_one(events, start_x, cfg['input_size'], cfg['options'].get('masked', False))
    until_T = T is not None
    o32, o64 = hip_util.oracle_pair(cfg, sd, b, delta_t, T if until_T else 0.0, predict=True, get_loss=False,
                                    until_T=until_T)
    rows = schedule._walk_clock(b['times'], delta_t, T, until_T)[4]
    return o32, o64, rows


class Worst:
    """The issue's yardstick, ``check_vs_oracle(predict=True)``'s rule per quantity:
    err(online, f64) <= max(2 err(oracle fp32, f64), 2e-6), never looser than ATOL / RTOL."""

    def __init__(self):
        self.items = []

    def add(self, tag, got, v32, v64):
        self.items.append((tag, np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(v32).reshape(-1),
                           np.asarray(v64).reshape(-1)))

    def check(self, label):
        assert self.items
        by = {}
        for tag, got, v32, v64 in self.items:
            g, a, c = by.setdefault(tag.split(':')[0], ([], [], []))
            g.append(got), a.append(v32), c.append(v64)
        for what, (g, a, c) in by.items():
            g, a, c = np.concatenate(g), np.concatenate(a), np.concatenate(c)
            assert np.all(np.isfinite(g)), (label, what)
            e, e32 = np.abs(g - c).max(), np.abs(a - c).max()
            print('{:32s} {:8s} err(online, f64) = {:.2e}  err(o32, f64) = {:.2e}'.format(label, what, e, e32))
            assert e <= max(2 * e32, 2e-6), (label, what, e, e32)
            np.testing.assert_allclose(g, c, atol=hip_util.ATOL, rtol=hip_util.RTOL, err_msg=label + ' ' + what)
