"""The float64 route on the GPU (``njode_amd.float64.NJODE64``, ``include/njode_f64.h``) against the
float64 CPU oracle and the stored float64 truth.

Bound, per quantity (hT, path_h, path_y on max-abs; the loss; each gradient tensor on L2):

    err(HIP f64, f64 oracle) <= max(1e-6 x e32, 256 x 2^-52 x max|truth|)

with ``e32 = err(fp32 oracle, f64 oracle)`` (``hip_util.oracle_pair``) -- or, for the stored truth
``g13_f64_truth.npz``, the fixture's own fp32 golden -- as the yardstick.  The same recursion amplifies
both roundings, so the expected ratio is eps64 / eps32 = 2^-29 = 2e-9 times an ordering constant;
perturbing every parameter by up to one float64 ulp moves the float64 oracle by ratios of 1e-9 .. 1.3e-8
on ``g2_bs_grads_B64`` and ``g5_masked``; 1e-6 leaves about 75 x over the worst of these for another
summation order and another tanh.  Every figure is printed before it is asserted; with the environment
variable ``NJODE_F64_REPORT_DIR`` set, every measured ratio is also appended to
``f64_route_ratios.jsonl`` in that folder (``profiles/f64_route.jsonl`` holds a copy of one such run).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import hip_util
from golden_util import GOLDEN_DIR, Golden
from guarded import Arena
from njode_amd import _lib
from oracle import njode_oracle

pytestmark = pytest.mark.gpu

REL, FLOOR = 1e-6, 256 * 2.0 ** -52

GOLDENS = ['g2_bs_grads_B64', 'g5_masked', 'g6_current_t', 'g6_easy_loss', 'g6_weight075', 'g6_no_residual',
           'g6_power2', 'g6_relu_w20', 'g6_linear_nets', 'g6_none_h50', 'g6_mixed_nets', 'g6_w100',
           'g6_offgrid_dt', 'g6_sparse_B5']
PREDICT_ONLY = ['g14_out5', 'g14_out20']
TRUTH = ['g5_masked', 'g5_full', 'g5_w200']


def _report(rec):
    """With NJODE_F64_REPORT_DIR set: one line per case in ``f64_route_ratios.jsonl`` there."""
    out = os.environ.get('NJODE_F64_REPORT_DIR')
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'f64_route_ratios.jsonl'), 'a') as f:
        f.write(json.dumps(rec) + '\n')


class Checker:
    """Collects (quantity, err, e32, bound) of one case, prints every figure, asserts at the end."""

    def __init__(self, tag):
        self.tag, self.rows, self.bad = tag, {}, []

    def _add(self, key, e, e32, scale):
        bound = max(REL * e32, FLOOR * scale)
        self.rows[key] = {'err': e, 'e32': e32, 'ratio': e / e32 if e32 > 0 else None, 'bound': bound}
        print('{:28s} {:36s} err {:.3e}  e32 {:.3e}  bound {:.3e}'.format(self.tag, key, e, e32, bound))
        if not e <= bound:
            self.bad.append((key, e, e32, bound))

    def max_abs(self, key, got, o32, truth):
        got, o32, truth = (np.asarray(a, dtype=np.float64) for a in (got, o32, truth))
        assert got.shape == truth.shape, (self.tag, key, got.shape, truth.shape)
        self._add(key, float(np.abs(got - truth).max()), float(np.abs(o32 - truth).max()),
                  float(np.abs(truth).max()))

    def l2(self, key, got, o32, truth):
        got, o32, truth = (np.asarray(a, dtype=np.float64) for a in (got, o32, truth))
        assert got.shape == truth.shape, (self.tag, key, got.shape, truth.shape)
        self._add(key, float(np.linalg.norm(got - truth)), float(np.linalg.norm(o32 - truth)),
                  float(np.abs(truth).max()))

    def done(self):
        q = self.rows
        worst_key = max(q, key=lambda k: (q[k]['ratio'] or 0.0))
        # (a truth that is exactly zero -- the gradient behind a dead relu, a loss nobody is observed for --
        # has the bound 0: an exact result is 0 of it, anything else is beyond it and fails below)
        over = max((v['err'] / v['bound'] if v['bound'] > 0 else (0.0 if v['err'] == 0 else float('inf')))
                   for v in q.values())
        _report({'kind': 'ratio', 'case': self.tag, 'worst_ratio': q[worst_key]['ratio'] or 0.0,
                 'worst_quantity': worst_key, 'worst_err_over_bound': over, 'quantities': len(q)})
        assert not self.bad, (self.tag, self.bad)


def model64(cfg, sd, train=True):
    from njode_amd.float64 import NJODE64
    cfg = dict(cfg, options=dict(cfg.get('options', {}), device_outputs=True))
    m = NJODE64(**cfg)
    m.load_state_dict({k: v.double() for k, v in sd.items()})
    return m.cuda().train(train)


def fwd64(m, b, dt, T, **kw):
    d = hip_util.to_dev(b)
    return m(d['times'], d['time_ptr'], d['X'], d['obs_idx'], dt, T, d['start_X'], d.get('n_obs_ot'),
             M=d.get('M'), **kw)


def grads64(m):
    return {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}


def check_train(tag, cfg, sd, b, dt, T, c_hT=None, **kw):
    """A loss call with gradients (of loss + (c_hT hT).sum()) against the oracle pair."""
    okw = dict(kw, c_hT=c_hT) if c_hT is not None else kw
    o32, o64 = hip_util.oracle_pair(cfg, sd, b, dt, T, **okw)
    m = model64(cfg, sd)
    hT, loss = fwd64(m, b, dt, T, **kw)
    obj = loss if c_hT is None else loss + (torch.as_tensor(c_hT).double().cuda() * hT).sum()
    obj.backward()
    got = grads64(m)
    c = Checker(tag)
    c.max_abs('hT', hT.detach().cpu().numpy(), o32['hT'], o64['hT'])
    c.max_abs('loss', float(loss.detach()), o32['loss'], o64['loss'])
    for k in o64['g']:
        c.l2('grad/' + k, got[k], o32['g'][k], o64['g'][k])
    c.done()


def check_predict(tag, cfg, sd, b, dt, T, get_loss=True):
    """return_path=True, until_T=True: the path, hT and (with get_loss) the loss."""
    o32, o64 = hip_util.oracle_pair(cfg, sd, b, dt, T, predict=True, grads=False, until_T=True,
                                    get_loss=get_loss)
    m = model64(cfg, sd, train=False)
    with torch.no_grad():
        hT, loss, path_t, path_h, path_y = fwd64(m, b, dt, T, return_path=True, until_T=True, get_loss=get_loss)
    c = Checker(tag)
    c.max_abs('hT', hT.cpu().numpy(), o32['hT'], o64['hT'])
    c.max_abs('path_h', path_h.cpu().numpy(), o32['path_h'], o64['path_h'])
    c.max_abs('path_y', path_y.cpu().numpy(), o32['path_y'], o64['path_y'])
    if get_loss:
        c.max_abs('loss', float(loss), o32['loss'], o64['loss'])
    c.done()


# ---- goldens against the CPU oracle --------------------------------------------------------------
@pytest.mark.parametrize('name', GOLDENS)
def test_golden_loss_and_gradients(name):
    g = Golden(name)
    check_train(name + '/train', g.cfg, g.state_dict(), g.batch(), g.delta_t, g.T)


@pytest.mark.parametrize('name', GOLDENS)
def test_golden_paths_until_T(name):
    g = Golden(name)
    check_predict(name + '/path', g.cfg, g.state_dict(), g.batch(), g.delta_t, g.T)


@pytest.mark.parametrize('name', PREDICT_ONLY)
def test_golden_prediction_calls(name):
    """output_size != input_size: no loss, the path and hT."""
    g = Golden(name)
    check_predict(name + '/path', g.cfg, g.state_dict(), g.batch(), g.delta_t, g.T, get_loss=False)


# ---- widths between and beyond the goldens' -----------------------------------------------------------
def _wide_cfg(ode, enc, dec):
    return dict(input_size=1, hidden_size=10, output_size=1, ode_nn=ode, readout_nn=dec, enc_nn=enc,
                use_rnn=False, bias=True, dropout_rate=0.0, options={})


WIDE = {
    # widest layer 150: a workgroup of 256 threads; weight rows of 13 (a pass of 16 lanes), 150 (> 128 lanes),
    # 100 (<= 128), 1 and 10 inputs in one model
    'w150_100': _wide_cfg(((150, 'tanh'), (100, 'tanh')), ((100, 'relu'), (150, 'tanh')), ((150, 'tanh'),)),
    # widest layer 96: a workgroup of 128 threads with rows of 96 (128 lanes) and 65 inputs
    'w96_65': _wide_cfg(((96, 'tanh'), (65, 'tanh')), ((65, 'tanh'),), ((96, 'relu'), (65, 'tanh'))),
    # the widest layers the library takes: threads loop over units (four units each)
    'w1024': _wide_cfg(((1024, 'tanh'), (1024, 'relu')), ((1024, 'tanh'),), ((1024, 'tanh'),)),
}


@pytest.mark.parametrize('name', sorted(WIDE))
def test_widths_the_goldens_do_not_have(name):
    """Loss, hT, every gradient and the paths at workgroup sizes and weight-row lengths no golden has:
    rows shorter and longer than the lanes a pass deals them, and layers wider than the workgroup."""
    cfg = WIDE[name]
    b, meta = hip_util.bs_batch(5, seed=7, obs_perc=0.2, nb_steps=20)
    sd = _init_sd(cfg, 3)
    check_train(name + '/train', cfg, sd, b, meta['dt'], meta['maturity'])
    check_predict(name + '/path', cfg, sd, b, meta['dt'], meta['maturity'])


# ---- stored truth at full size -------------------------------------------------------------------
@pytest.mark.parametrize('name', TRUTH)
def test_stored_truth(name):
    """``g13_f64_truth.npz``: the reference under ``.double()``; yardstick: the fixture's fp32 golden.
    No CPU oracle run."""
    g = Golden(name)
    t = np.load(os.path.join(GOLDEN_DIR, 'g13_f64_truth.npz'), allow_pickle=False)
    m = model64(g.cfg, g.state_dict(), train=False)
    with torch.no_grad():
        hT, loss, _, _, path_y = fwd64(m, g.batch(), g.delta_t, g.T, return_path=True, get_loss=True, until_T=True)
    rows = g['path_rows'] if 'path_rows' in g else slice(None)
    c = Checker(name + '/truth')
    c.max_abs('path_y', path_y.cpu().numpy()[rows], g['path_y'], t[name + '/path_y'])
    c.max_abs('hT', hT.cpu().numpy(), g['hT'], t[name + '/hT'])
    c.max_abs('loss', float(loss), float(g['loss']), float(t[name + '/loss']))
    m.train()
    hT2, tl = fwd64(m, g.batch(), g.delta_t, g.T)
    tl.backward()
    got = grads64(m)
    c.max_abs('train_loss', float(tl.detach()), float(g['train_loss']), float(t[name + '/train_loss']))
    c.max_abs('train_hT', hT2.detach().cpu().numpy(), g['train_hT'], t[name + '/train_hT'])
    for k, ref32 in g.group('grad').items():
        c.l2('grad/' + k, got[k], ref32, t[name + '/grad/' + k])
    c.done()


# ---- irregular batches -----------------------------------------------------------------------------
MASKED_CFG = dict(input_size=41, hidden_size=41, output_size=41, ode_nn=hip_util.NN50, readout_nn=hip_util.NN50,
                  enc_nn=hip_util.NN50, use_rnn=False, bias=True, dropout_rate=0.0, options={'masked': True})


def _init_sd(cfg, seed=0):
    return njode_oracle.make_oracle(cfg).init_params(seed=seed)


def _shape_batch(shape, B=12, steps=30):
    """(cfg, sd, batch, dt, T) of the demo or the masked (PhysioNet) shape, a small regular batch."""
    if shape == 'demo':
        cfg = hip_util.demo_cfg()
        b, meta = hip_util.bs_batch(B, seed=4, obs_perc=0.2, nb_steps=steps)
        return cfg, _init_sd(cfg, 1), b, meta['dt'], meta['maturity']
    from njode_amd import synthetic_physionet
    b = synthetic_physionet.make_batch(batch_size=B, dim=41, n_grid=steps, n_obs_range=(2, 6), seed=9)
    return MASKED_CFG, _init_sd(MASKED_CFG, 2), b, b['delta_t'], b['T']


def _irregular(shape):
    cfg, sd, b, dt, T = _shape_batch(shape)
    b2, dt2 = hip_util.irregular_batch(b, dt)
    return cfg, sd, b2, dt2, T


@pytest.mark.parametrize('shape', ['demo', 'masked'])
def test_irregular_batch(shape):
    """A t = 0 jump, an empty slice, an inserted off-grid time, partial steps, a never-observed path."""
    cfg, sd, b, dt, T = _irregular(shape)
    assert int((b['n_obs_ot'] == 0).sum()) >= 1 and 0 in np.diff(b['time_ptr']) and b['times'][0] == 0.0
    check_train(shape + '/irregular', cfg, sd, b, dt, T)
    check_predict(shape + '/irregular/path', cfg, sd, b, dt, T)


@pytest.mark.parametrize('shape', ['demo', 'masked'])
def test_irregular_loss_call_with_tail(shape):
    """get_loss with until_T: Euler steps after the last jump, gradients through them via hT."""
    cfg, sd, b, dt, _ = _irregular(shape)
    T = float(b['times'][-1]) + 2.6 * dt
    B, H = b['start_X'].shape[0], cfg['hidden_size']
    c_hT = 0.05 * torch.cos(torch.arange(B * H, dtype=torch.float32)).view(B, H)
    check_train(shape + '/irregular/tail', cfg, sd, b, dt, T, c_hT=c_hT, until_T=True)


@pytest.mark.parametrize('shape', ['demo', 'masked'])
def test_single_path(shape):
    """B = 1."""
    cfg, sd, b, dt, T = _shape_batch(shape, B=1)
    check_train(shape + '/B1', cfg, sd, b, dt, T)
    check_predict(shape + '/B1/path', cfg, sd, b, dt, T)


# ---- gradient through hT ---------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ['demo', 'masked'])
def test_gradient_through_hT(shape):
    """Random c_hT: d (loss + (c_hT hT).sum()) / d params on the one plan of this route."""
    cfg, sd, b, dt, T = _shape_batch(shape)
    B, H = b['start_X'].shape[0], cfg['hidden_size']
    c_hT = torch.randn(B, H, generator=torch.Generator().manual_seed(5))
    check_train(shape + '/grad_hT', cfg, sd, b, dt, T, c_hT=c_hT)


# ---- determinism and independence from B -----------------------------------------------------------
def _bits(t):
    return t.detach().contiguous().view(torch.int64)


@pytest.mark.parametrize('shape', ['demo', 'masked'])
def test_same_call_twice_gives_the_same_bits(shape):
    cfg, sd, b, dt, T = _shape_batch(shape)
    res = []
    for _ in range(2):
        m = model64(cfg, sd)
        hT, loss = fwd64(m, b, dt, T)
        (loss + hT.sum()).backward()
        with torch.no_grad():
            _, _, _, path_h, path_y = fwd64(m, b, dt, T, return_path=True, until_T=True, get_loss=False)
        res.append([hT, loss, path_h, path_y] + [p.grad for p in m.parameters()])
    for a, c in zip(*res):
        assert torch.equal(_bits(a), _bits(c))


@pytest.mark.parametrize('shape', ['demo', 'masked'])
def test_paths_do_not_depend_on_the_batch(shape):
    """Paths 0-3 alone (same times, slices left empty) and inside a 24-path batch: bit-equal rows."""
    cfg, sd, b, dt, T = _shape_batch(shape, B=24)
    keep = b['obs_idx'] < 4
    slice_of = np.repeat(np.arange(len(b['times'])), np.diff(b['time_ptr']))
    counts = np.bincount(slice_of[keep.numpy()], minlength=len(b['times']))
    small = dict(b, X=b['X'][keep], obs_idx=b['obs_idx'][keep], start_X=b['start_X'][:4],
                 n_obs_ot=b['n_obs_ot'][:4], time_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    if 'M' in b:
        small['M'] = b['M'][keep]
    m = model64(cfg, sd, train=False)
    with torch.no_grad():
        big = fwd64(m, b, dt, T, return_path=True, until_T=True, get_loss=False)
        sml = fwd64(m, small, dt, T, return_path=True, until_T=True, get_loss=False)
    assert torch.equal(_bits(big[0][:4]), _bits(sml[0]))
    assert torch.equal(_bits(big[3][:, :4]), _bits(sml[3]))
    assert torch.equal(_bits(big[4][:, :4]), _bits(sml[4]))


# ---- exact buffer sizes between guard bands --------------------------------------------------------
@pytest.mark.parametrize('shape', ['demo', 'masked'])
def test_entry_points_stay_inside_their_buffers(shape):
    """Both entry points at exactly the stated workspace and array sizes between guard bands
    (``tests/guarded.py``): return code 0, every guard intact, the wrapper's bits, and the same bits
    under the other phase of the workspace / output pattern."""
    from njode_amd.float64 import Schedule64
    cfg, sd, b, dt, T = _irregular(shape)
    m = model64(cfg, sd)
    hT_w, loss_w = fwd64(m, b, dt, T)
    (0.7 * loss_w + (0.3 * hT_w).sum()).backward()
    with torch.no_grad():
        _, lp_w, _, ph_w, py_w = fwd64(m, b, dt, T, return_path=True, until_T=True)
    want = {'hT': hT_w.detach(), 'loss': loss_w.detach().reshape(1), 'grad': torch.cat(
        [p.grad.reshape(-1) for p in m.parameters()]), 'path_h': ph_w, 'path_y': py_w, 'loss_p': lp_w.reshape(1)}
    assert want['grad'].numel() == m.flat_parameters().numel()     # (bias=True: no empty slots)

    L, dims = _lib.lib(), m._get_dims()
    B, D, H, DO = b['start_X'].shape[0], cfg['input_size'], cfg['hidden_size'], cfg['output_size']
    n_obs = int(b['time_ptr'][-1])
    tp = np.asarray(b['time_ptr'], dtype=np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for phase in (0, 1):
        got = {}
        for mode in ('train', 'path'):
            sched = Schedule64(b['times'], dt, T, mode == 'path')
            host = np.zeros(sched.packed_nbytes() // 4 + 2, dtype=np.int32)
            cs = sched.pack_into(host, tp)
            K, nt = sched.n_steps, sched.n_times
            flags = _lib.C_GET_LOSS | (_lib.C_SAVE_BWD if mode == 'train' else _lib.C_RETURN_PATH)
            need = ctypes.c_size_t(0)
            assert L.njode_f64_workspace_bytes(ctypes.byref(dims), B, n_obs, nt, K, flags, ctypes.byref(need)) == 0
            A = Arena(phase=phase)
            A.add('params', 8 * m.flat_parameters().numel(), 'nan64').add('start_X', 8 * B * D, 'nan64')
            A.add('X', 8 * n_obs * D, 'nan64').add('obs_idx', 4 * n_obs, 'index', modulo=B)
            A.add('n_obs_ot', 4 * B, 'index', modulo=3, base=1)
            if 'M' in b:
                A.add('M', 8 * n_obs * D, 'nan64')
            A.add('ws', need.value).add('hT', 8 * B * H).add('loss', 8)
            if mode == 'train':
                A.add('grad_loss', 8, 'nan64').add('grad_hT', 8 * B * H, 'nan64').add('grad', 8 * m.flat_parameters().numel())
            else:
                n_rows = 1 + K + nt
                A.add('path_h', 8 * n_rows * B * H).add('path_y', 8 * n_rows * B * DO)
            A.build()
            A.put('params', m.flat_parameters()), A.put('start_X', b['start_X'].double().cuda())
            A.put('X', b['X'].double().cuda()), A.put('obs_idx', b['obs_idx'].int().cuda())
            A.put('n_obs_ot', b['n_obs_ot'].int().cuda())
            if 'M' in b:
                A.put('M', b['M'].double().cuda())
            cb = _lib.NjodeBatch64(B, n_obs, A.ptr('start_X'), A.ptr('X'), A.ptr('M') if 'M' in b else None,
                                   A.ptr('obs_idx'), A.ptr('n_obs_ot'), float(B))
            path = (A.ptr('path_h'), A.ptr('path_y')) if mode == 'path' else (None, None)
            rc = L.njode_forward_f64(ctypes.byref(dims), A.ptr('params'), ctypes.byref(cb), ctypes.byref(cs), flags,
                                     float(m.weight), A.ptr('hT'), A.ptr('loss'), *path, A.ptr('ws'), need.value,
                                     stream)
            assert rc == 0, L.njode_last_error()
            torch.cuda.synchronize()        # (the host schedule array is pageable: the copy has been made)
            if mode == 'train':
                A.put('grad_loss', torch.tensor([0.7], dtype=torch.float64)), A.put(
                    'grad_hT', torch.full((B, H), 0.3, dtype=torch.float64))
                rc = L.njode_backward_f64(ctypes.byref(dims), A.ptr('params'), ctypes.byref(cb), ctypes.byref(cs),
                                          flags, float(m.weight), A.ptr('grad_loss'), A.ptr('grad_hT'),
                                          A.ptr('grad'), A.ptr('ws'), need.value, stream)
                assert rc == 0, L.njode_last_error()
                got['hT'], got['loss'] = A.view('hT', torch.float64, (B, H)).clone(), A.view('loss', torch.float64).clone()
                got['grad'] = A.view('grad', torch.float64).clone()
            else:
                got['path_h'] = A.view('path_h', torch.float64, ph_w.shape).clone()
                got['path_y'] = A.view('path_y', torch.float64, py_w.shape).clone()
                got['loss_p'] = A.view('loss', torch.float64).clone()
            assert A.check() == [], (mode, phase, A.check())
        outs.append(got)
    for k, ref in want.items():
        assert torch.equal(_bits(outs[0][k]), _bits(ref)), k
        assert torch.equal(_bits(outs[1][k]), _bits(ref)), k


# ---- training ------------------------------------------------------------------------------------
def test_three_adam_steps_in_double():
    """torch.optim.Adam on an NJODE64 against ``oracle.njode_oracle.train_step`` in float64; the
    yardstick is the fp32 oracle's training run."""
    cfg, sd, b, dt, T = _shape_batch('demo', B=16)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        runs = {}
        for dtype in (torch.float32, torch.float64):
            o = njode_oracle.make_oracle(cfg)
            params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
            opt = torch.optim.Adam(list(params.values()), lr=1e-3)
            cast = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b.items()}
            losses = [float(njode_oracle.train_step(o, params, opt, cast, dt, T)) for _ in range(3)]
            runs[dtype] = (losses, {k: p.detach().numpy().astype(np.float64) for k, p in params.items()})
    finally:
        torch.set_num_threads(threads)
    m = model64(cfg, sd)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        _, loss = fwd64(m, b, dt, T)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert m._views_in_place()
    (l32, p32), (l64, p64) = runs[torch.float32], runs[torch.float64]
    c = Checker('demo/adam3')
    for i in range(3):
        c.max_abs('loss{}'.format(i), losses[i], l32[i], l64[i])
    got = {k: p.detach().cpu().numpy() for k, p in m.named_parameters()}
    for k in p64:
        c.l2('param/' + k, got[k], p32[k], p64[k])
    c.done()
