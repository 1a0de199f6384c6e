"""CPU tests of the host side of the HIP path: the float64 step schedule, the flat
parameter layout, the operator surface, and that libnjode_hip.so loads and exports
every symbol include/njode_hip.h declares (no compute without a GPU)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from golden_util import Golden, all_model_cases
from njode_amd import _lib, models
from njode_amd.schedule import Schedule, ScheduleCache

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', [n for n in all_model_cases() if n != 'g2_bs_grads_B64'])
def test_schedule_reproduces_reference_clock(name):
    """path_t of the reference (float64 clock incl. partial steps, t=0 jump, empty
    slices, until_T tail) is reproduced exactly; fp32 arrays are consistent with it."""
    g = Golden(name)
    s = Schedule(g['times'], g.delta_t, g.T, until_T=True)
    assert np.array_equal(s.path_t, g['path_t'])
    assert s.n_rows == len(g['path_t'])
    assert s.n_times == len(g['times'])
    assert np.all(np.diff(s.k_jump) >= 0)
    assert np.array_equal(s.time_f32, g['times'].astype(np.float32))
    # rows: jump i sits right after the row of Euler step k_jump[i]-1
    assert np.array_equal(s.path_t[s.row_of_jump], g['times'])
    # steps sum to the clock
    assert abs(float(s.step_dt.astype(np.float64).sum()) - s.path_t[-1]) < 1e-4


def test_schedule_without_tail_and_offgrid():
    g = Golden('g6_offgrid_dt')
    s = Schedule(g['times'], g.delta_t, g.T, until_T=False)
    assert s.n_steps == s.k_jump[-1]                       # no tail
    s2 = Schedule(g['times'], g.delta_t, g.T, until_T=True)
    assert s2.n_steps > s.n_steps                          # T=1.05 tail
    # dt 0.004 on a 0.01 grid: 2 full + 1 partial step per interval
    d = s.step_dt[:3].astype(np.float64)
    assert d[0] == pytest.approx(0.004) and d[2] == pytest.approx(0.002, rel=1e-5)


def test_schedule_grid_data_rounds_to_one_dt():
    g = Golden('g1_bs_eval_B200')
    s = Schedule(g['times'], g.delta_t, g.T, until_T=False)
    assert s.n_steps == 100 and len(set(s.step_dt.tolist())) == 1


def test_schedule_cache_and_packing():
    g = Golden('g1_bs_eval_B7')
    c = ScheduleCache(capacity=2)
    a = c.get(g['times'], g.delta_t, g.T, True)
    assert c.get(g['times'].copy(), g.delta_t, g.T, True) is a
    assert c.get(g['times'], g.delta_t, g.T, False) is not a
    buf = np.zeros(a.packed_nbytes() // 4 + 8, dtype=np.int32)
    K, nt = a.pack_into(buf, g['time_ptr'].astype(np.int32))
    f = buf.view(np.float32)
    assert np.array_equal(f[:K], a.step_dt) and np.array_equal(f[K:2 * K], a.step_t)
    assert np.array_equal(buf[2 * K:2 * K + nt], a.k_jump)
    assert np.array_equal(buf[2 * K + 2 * nt:2 * K + 3 * nt + 1], g['time_ptr'])


def _demo_model(**opts):
    nn = ((50, 'tanh'), (50, 'tanh'))
    return models.NJODE(1, 10, 1, nn, nn, nn, use_rnn=False, bias=True, dropout_rate=0.1,
                        options=opts, epochs=3, batch_size=100, dataset='BlackScholes')


def test_operator_surface_and_state_dict_keys():
    g = Golden('g1_bs_eval_B7')
    m = _demo_model()
    assert list(m.state_dict().keys()) == list(g.state_dict().keys())
    assert sum(p.numel() for p in m.parameters()) == 10071
    assert m.epoch == 1 and m.weight == 0.5
    m.load_state_dict(g.state_dict())
    for name in ('NJODE', 'ODEFunc', 'FFNN', 'GRUCell', 'get_ffnn', 'compute_loss',
                 'compute_loss_2', 'LOSS_FUN_DICT', 'nonlinears', 'init_weights',
                 'save_checkpoint', 'get_ckpt_model'):
        assert hasattr(models, name)
    m.weight, m.weight_decay = 0.9, 0.5
    assert m.weight_decay_step() == pytest.approx(0.7)
    with pytest.raises(RuntimeError):
        m.encoder_map(torch.zeros(1, 1))       # parameter container only: no eager path


def test_flat_parameter_views_follow_state_dict_and_to():
    g = Golden('g1_bs_eval_B7')
    m = _demo_model()
    flat = m.flat_parameters()
    assert flat.numel() == 10071
    m.load_state_dict(g.state_dict())          # in-place copy keeps the views
    assert m.flat_parameters() is flat
    sd = g.state_dict()
    off = 0
    for k in sd:                               # flat layout == state_dict order
        n = sd[k].numel()
        assert torch.equal(flat[off:off + n], sd[k].reshape(-1)), k
        off += n
    w = m.ode_f.f[0].weight
    with torch.no_grad():
        w.mul_(2.0)
    assert torch.equal(m.flat_parameters()[:w.numel()], w.reshape(-1))
    m.to(torch.float32)                        # no-op keeps views
    assert m.flat_parameters() is flat


def test_bias_free_model_keeps_zero_bias_slots():
    nn = ((50, 'tanh'), (50, 'tanh'))
    m = models.NJODE(1, 10, 1, nn, nn, nn, use_rnn=False, bias=False, options={})
    assert sum(p.numel() for p in m.parameters()) == 10071 - (50 + 50 + 10) * 2 - (50 + 50 + 1)
    flat = m.flat_parameters()
    assert flat.numel() == 10071
    assert float(flat[650:700].abs().sum()) == 0.0      # ode_f.f.0 bias slot


def test_gru_parameters_extend_the_flat_vector():
    g = Golden('g6_use_rnn')
    m = models.NJODE(**g.cfg)
    assert list(m.state_dict().keys()) == list(g.state_dict().keys())
    m.load_state_dict(g.state_dict())
    flat = m.flat_parameters()
    assert flat.numel() == 10071 + 3 * 10 * (1 + 10 + 2)
    sd, off = g.state_dict(), 0
    for k in sd:
        n = sd[k].numel()
        assert torch.equal(flat[off:off + n], sd[k].reshape(-1)), k
        off += n


def test_residual_size_errors_match_reference():
    nn = ((50, 'tanh'), (50, 'tanh'))
    with pytest.raises(ValueError, match='output_size needs to be multiple of input_size'):
        models.NJODE(41, 50, 41, nn, nn, nn, use_rnn=False, options={'masked': True})
    models.NJODE(41, 50, 41, nn, nn, nn, use_rnn=False,
                 options={'masked': True, 'residual_enc_dec': False})


def test_cpu_device_fails_loudly():
    g = Golden('g1_bs_eval_B7')
    m = _demo_model()
    b = g.batch()
    with pytest.raises((RuntimeError, ImportError)):
        m(b['times'], b['time_ptr'], b['X'], b['obs_idx'], g.delta_t, g.T, b['start_X'],
          b['n_obs_ot'])


def test_checkpoint_roundtrip(tmp_path):
    m = _demo_model()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=0.0005)
    m.weight = 0.7
    models.save_checkpoint(m, opt, str(tmp_path), epoch=4)
    ck = torch.load(str(tmp_path / 'checkpt.tar'), weights_only=False)
    assert set(ck) == {'epoch', 'weight', 'model_state_dict', 'optimizer_state_dict'}
    m2 = _demo_model()
    models.get_ckpt_model(str(tmp_path), m2, torch.optim.Adam(m2.parameters()), 'cpu')
    assert m2.epoch == 4 and m2.weight == 0.7
    assert torch.equal(m2.flat_parameters(), m.flat_parameters())


def test_fused_adam_state_dict_is_torch_adam_layout(tmp_path):
    """A checkpoint of the fused loop must load into torch.optim.Adam (what the reference's
    get_ckpt_model does, models.py:63) and the reverse."""
    m = _demo_model()
    ref = torch.optim.Adam(m.parameters(), lr=2e-3, betas=(0.8, 0.95), eps=1e-7,
                           weight_decay=0.0005)
    torch.manual_seed(3)
    before = m.flat_parameters().clone()
    for _ in range(3):                      # three reference steps on random gradients
        for p in m.parameters():
            p.grad = torch.randn_like(p)
        ref.step()
    # reference -> fused
    fused = models.FusedAdam(m)
    fused.load_state_dict(ref.state_dict())
    assert fused.step_count == 3 and fused.lr == 2e-3 and fused.betas == (0.8, 0.95)
    assert fused.eps == 1e-7 and fused.weight_decay == 0.0005
    idx = fused._param_index()
    for i, p in enumerate(m.parameters()):
        off, n, shape = idx[i]
        assert torch.equal(fused.exp_avg[off:off + n].view(shape), ref.state[p]['exp_avg'])
        assert torch.equal(fused.exp_avg_sq[off:off + n].view(shape), ref.state[p]['exp_avg_sq'])
    # fused -> reference (through the checkpoint file, like train.py / get_ckpt_model)
    models.save_checkpoint(m, fused, str(tmp_path), epoch=7)
    m2 = _demo_model()
    ref2 = torch.optim.Adam(m2.parameters())
    models.get_ckpt_model(str(tmp_path), m2, ref2, 'cpu')
    sd, sd2 = ref.state_dict(), ref2.state_dict()
    assert sd2['param_groups'][0]['lr'] == 2e-3 and sd2['param_groups'][0]['betas'] == (0.8, 0.95)
    assert sorted(sd2['state']) == sorted(sd['state'])
    for k in sd['state']:
        assert float(sd2['state'][k]['step']) == 3.0
        assert torch.equal(sd2['state'][k]['exp_avg'], sd['state'][k]['exp_avg'])
        assert torch.equal(sd2['state'][k]['exp_avg_sq'], sd['state'][k]['exp_avg_sq'])
    # the two optimizers continue identically from there
    g = [torch.randn_like(p) for p in m.parameters()]
    for opt, mm in ((ref, m), (ref2, m2)):
        for p, gi in zip(mm.parameters(), g):
            p.grad = gi.clone()
        opt.step()
    assert torch.equal(m.flat_parameters(), m2.flat_parameters())
    assert not torch.equal(m.flat_parameters(), before)
    # a fresh optimizer has no per-parameter state, exactly like torch's
    assert models.FusedAdam(_demo_model()).state_dict()['state'] == {}
    # and FusedAdam reads its own checkpoints
    f3 = models.FusedAdam(m2)
    f3.load_state_dict(fused.state_dict())
    assert f3.step_count == 3 and torch.equal(f3.exp_avg, fused.exp_avg)


def test_library_loads_and_exports_declared_symbols():
    """Every function declared in include/*.h is exported by the built library (built by
    __graft_entry__.build(); no GPU needed to load it)."""
    header = ''.join(open(os.path.join(REPO, 'include', n)).read()
                     for n in sorted(os.listdir(os.path.join(REPO, 'include'))))
    declared = set(re.findall(r'\b(njode_[a-z0-9_]+)\s*\(', header))
    assert declared == set(_lib.EXPORTS)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libnjode_hip.so not built in this checkout (run __graft_entry__.build())')
    L = _lib.lib()
    for sym in declared:
        assert hasattr(L, sym), sym
    info = _lib.build_info()
    assert info.startswith('gfx950;') and 'd1.h10.o1.nh2.w50' in info
    d = _lib.NjodeDims(1, 10, 1, 2, 50, 0, _lib.F_RESIDUAL)
    assert L.njode_supported(ctypes.byref(d)) == 1
    assert L.njode_param_count(ctypes.byref(d)) == 10071
    # a shape outside the build table runs on the shape-generic kernels ...
    d3 = _lib.NjodeDims(3, 7, 3, 2, 50, 0, 0)
    assert L.njode_supported(ctypes.byref(d3)) == 1
    assert L.njode_param_count(ctypes.byref(d3)) == (12 * 50 + 50) + (50 * 50 + 50) + (50 * 7 + 7) + \
        (3 * 50 + 50) + (50 * 50 + 50) + (50 * 7 + 7) + (7 * 50 + 50) + (50 * 50 + 50) + (50 * 3 + 3)
    # ... with per-network descriptions too
    d4 = _lib.NjodeDims(2, 6, 2, 0, 0, 0, _lib.F_RESIDUAL)
    d4.per_net = 1
    d4.nets[0].n_hidden = 3
    for l, w in enumerate((64, 32, 48)):
        d4.nets[0].width[l] = w
    d4.nets[1].n_hidden = 1
    d4.nets[1].width[0] = 30
    assert L.njode_supported(ctypes.byref(d4)) == 1
    assert L.njode_param_count(ctypes.byref(d4)) == \
        (10 * 64 + 64) + (64 * 32 + 32) + (32 * 48 + 48) + (48 * 6 + 6) + (2 * 30 + 30) + (30 * 6 + 6) + (6 * 2 + 2)
    # ... except what no kernel family covers: a GRU jump outside the table, residual sizes
    # that do not divide (the reference raises ValueError for those, models.py:243-249)
    # (round 4: the shape-generic kernels run the GRU jump for any shape ...)
    d5 = _lib.NjodeDims(3, 7, 3, 2, 50, 0, _lib.F_USE_RNN)
    assert L.njode_supported(ctypes.byref(d5)) == 1
    assert L.njode_param_count(ctypes.byref(d5)) == \
        (12 * 50 + 50) + (50 * 50 + 50) + (50 * 7 + 7) + (3 * 50 + 50) + (50 * 50 + 50) + (50 * 7 + 7) + \
        (7 * 50 + 50) + (50 * 50 + 50) + (50 * 3 + 3) + (21 * 3 + 21 * 7 + 21 + 21)
    # (round 5: ... and with masked data too -- models.py:353 has a TODO, but the model runs; the
    # masked encoder takes [x, mask]: 2 x 3 inputs)
    d2 = _lib.NjodeDims(3, 7, 3, 2, 50, 0, _lib.F_USE_RNN | _lib.F_MASKED)
    assert L.njode_supported(ctypes.byref(d2)) == 1
    assert L.njode_param_count(ctypes.byref(d2)) == L.njode_param_count(ctypes.byref(d5)) + 3 * 50
    # a GRU cell wider than the widest layer of the generic kernels (4 x hidden_size > 1 024)
    d2 = _lib.NjodeDims(3, 300, 3, 2, 50, 0, _lib.F_USE_RNN)
    assert L.njode_supported(ctypes.byref(d2)) == 0
    # round 5: output_size != input_size runs (prediction calls) -- unless masked
    assert L.njode_supported(ctypes.byref(_lib.NjodeDims(3, 6, 12, 2, 50, 0, 0))) == 1
    assert L.njode_supported(ctypes.byref(_lib.NjodeDims(3, 6, 12, 2, 50, 0, _lib.F_MASKED))) == 0
    assert L.njode_supported(ctypes.byref(_lib.NjodeDims(3, 7, 3, 2, 50, 0, _lib.F_RESIDUAL))) == 0
    need = ctypes.c_size_t(0)
    assert L.njode_workspace_bytes(ctypes.byref(d), 100, 1000, 100, 100,
                                   _lib.C_GET_LOSS | _lib.C_SAVE_BWD, ctypes.byref(need)) == 0
    assert need.value > 100 * 100 * 10 * 4
    assert L.njode_workspace_bytes(ctypes.byref(d2), 100, 1000, 100, 100, 0,
                                   ctypes.byref(need)) == _lib.E_UNSUPPORTED
    assert b'use_rnn' in L.njode_last_error()


def _envelope_grid():
    """Deterministic grid of (D, H, DO, nets, flags) around every bound of build_model: coarse
    sweeps of one size per family and flag combination, step 1 next to the first refused value the
    restatement finds, and the size / residual / depth / width / activation edges."""
    from gen_envelope import restate
    T, R = _lib.ACT_TANH, _lib.ACT_RELU
    grid = []

    def uni(n, w, act=T):
        return (n, (w,) * n, (act,) * n)

    def sweep(fam, lo, hi, flag_sets):
        for flags in flag_sets:
            first = next((x for x in range(lo, hi + 1) if restate(*fam(x), flags)[0] is not None), None)
            xs = set(range(lo, hi + 1, 37)) | {lo, hi}
            if first is not None:
                xs |= set(range(max(lo, first - 3), min(hi, first + 3) + 1))
            grid.extend(fam(x) + (flags,) for x in sorted(xs))

    every = range(32)
    unmasked = [f for f in every if not f & _lib.F_MASKED]
    sweep(lambda h: (1, h, 1, uni(0, 0)), 1, 1030, every)                       # nn_desc = None
    sweep(lambda h: (1, h, 1, uni(2, 50)), 1, 1030, every)                      # width 50 (use_rnn: 4H)
    sweep(lambda h: (1, h, 1, uni(2, 1024, R)), 1, 300, (0, 1, 2, 16, 17))      # width 1 024
    sweep(lambda d: (d, 10, d, uni(2, 24)), 1, 520, unmasked)                  # unmasked D = DO
    sweep(lambda d: (d, d, d, uni(2, 100)), 1, 520, [f for f in every if f & _lib.F_MASKED])   # masked D = H = DO
    sweep(lambda w: (1, 10, 1, uni(1, w)), 1, 1100, (0, 16))                   # widths
    sweep(lambda w: (2, 6, 2, uni(8, w, R)), 1, 1100, (4, 5))
    sweep(lambda w: (3, 7, 3, ((1, (w,), (T,)), (0, (), ()), (2, (40, 40), (T, R)))), 1, 1100, (0, 1))
    # sizes
    for D in (-1, 0, 1, 511, 512, 513):
        for H in (0, 1, 1023, 1024, 1025):
            for DO in (0, 1, 512, 513):
                grid.append((D, H, DO, uni(0, 0), 0))
    # residual cases and output_size != input_size
    for D in (1, 2, 3, 4, 6, 8, 12):
        for H in (1, 2, 3, 4, 6, 8, 12):
            for DO in (1, 2, 3, 4, 6, 8, 12):
                for flags in (4, 5, 0, 1):
                    grid.append((D, H, DO, uni(1, 20), flags))
    # depth, per-network descriptions, activations, bad widths
    for n in (-1, 0, 1, 4, 8, 9, 10):
        for flags in (0, 4, 16):
            grid.append((2, 4, 2, (n, (33,) * max(n, 0), (R,) * max(n, 0)), flags))
    for n0 in (0, 1, 8, 9):
        for n1 in (0, 3, 8):
            for n2 in (0, 2, 8, 9):
                ws = lambda n, b: tuple(b + 13 * l for l in range(n))
                acts = lambda n: tuple((T, R)[l % 2] for l in range(n))
                grid.append((3, 6, 3, ((n0, ws(n0, 17), acts(n0)), (n1, ws(n1, 64), acts(n1)),
                                       (n2, ws(n2, 127), acts(n2))), 4))
    for bad in ((2, (50, 0), (T, T)), (2, (50, -4), (T, T)), (2, (50, 50), (T, 2)), (2, (50, 50), (-1, T)),
                (1, (1024,), (T,)), (1, (1025,), (T,))):
        grid.append((1, 10, 1, (bad, (0, (), ()), (0, (), ())), 0))
        grid.append((1, 10, 1, ((0, (), ()), (0, (), ()), bad), 0))
    return grid


def _param_count_of_torch_model(D, H, DO, nets, flags):
    """Parameters of models.NJODE built on the meta device (no memory): the flat vector's length."""
    if not (len(nets) == 3 and isinstance(nets[0], tuple)):
        nets = (nets, nets, nets)

    def desc(n, ws, acts):
        return None if n == 0 else tuple((ws[l], 'tanh' if acts[l] == _lib.ACT_TANH else 'relu') for l in range(n))
    opts = {'masked': bool(flags & _lib.F_MASKED), 'input_current_t': bool(flags & _lib.F_INPUT_CURRENT_T),
            'residual_enc_dec': bool(flags & _lib.F_RESIDUAL),
            'which_loss': 'easy' if flags & _lib.F_LOSS_EASY else 'standard'}
    with torch.device('meta'):
        m = models.NJODE(D, H, DO, desc(*nets[0]), desc(*nets[2]), desc(*nets[1]),
                         use_rnn=bool(flags & _lib.F_USE_RNN), bias=True, dropout_rate=0.0, options=opts)
    return sum(p.numel() for p in m.parameters())


def test_generic_envelope_restatement_matches_the_library(capsys):
    """njode_supported agrees EXACTLY with a Python restatement of build_model (tests/gen_envelope.py)
    over a grid around every bound; njode_param_count with the torch model's parameter count; every
    refusal leaves its reason in njode_last_error, and NJODE._get_dims quotes it."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libnjode_hip.so not built in this checkout (run __graft_entry__.build())')
    import contextlib
    import io
    from gen_envelope import (R_LDS, R_MASKED, R_NET, R_NHIDDEN, R_RESIDUAL, R_RNN, R_SIZES, XR, dims_of,
                              restate)
    L = _lib.lib()
    grid = _envelope_grid()
    assert len(grid) >= 2000, len(grid)
    n_ok, reasons, mismatch = 0, {}, []
    for D, H, DO, nets, flags in grid:
        d = dims_of(D, H, DO, nets, flags)
        why, model = restate(D, H, DO, nets, flags)
        got = L.njode_supported(ctypes.byref(d))
        if got != (why is None):
            mismatch.append(((D, H, DO, nets, flags), why, got, L.njode_last_error()))
            continue
        if why is None:
            n_ok += 1
            P = L.njode_param_count(ctypes.byref(d))
            assert P == model['P'], ((D, H, DO, nets, flags), P, model['P'])
            with contextlib.redirect_stdout(io.StringIO()):   # (the model prints its loss name)
                assert P == _param_count_of_torch_model(D, H, DO, nets, flags), (D, H, DO, nets, flags)
            # at the default waves per workgroup every admitted shape holds its observations in
            # registers (k_gen_fwd's other branch runs only under NJODE_GEN_NW)
            assert D * 16 <= XR * 64 * model['nw'], (D, H, DO, nets, flags, model['nw'])
        else:
            err = L.njode_last_error().decode()
            assert err.startswith('generic kernels: ') and why in err, ((D, H, DO, nets, flags), why, err)
            assert L.njode_param_count(ctypes.byref(d)) == 0
            reasons[why] = reasons.get(why, 0) + 1
    assert not mismatch, mismatch[:10]
    assert set(reasons) >= {R_SIZES, R_MASKED, R_RESIDUAL, R_NHIDDEN, R_NET, R_RNN, R_LDS}, reasons
    # the first refused sizes of the documented families (include/njode_hip.h)
    T = _lib.ACT_TANH

    def first(fam, flags=0):
        return next(x for x in range(1, 1100) if restate(*fam(x), flags)[0] is not None)
    assert first(lambda h: (1, h, 1, (0, (), ()))) == 629
    assert first(lambda h: (1, h, 1, (2, (50, 50), (T, T))), _lib.F_USE_RNN) == 253
    assert first(lambda h: (1, h, 1, (2, (1024, 1024), (T, T)))) == 229
    assert first(lambda d: (d, 10, d, (2, (24, 24), (T, T)))) == 252
    assert first(lambda d: (d, d, d, (2, (100, 100), (T, T))), _lib.F_MASKED) == 210
    # NJODE._get_dims names the library's reason
    nn50 = ((50, 'tanh'), (50, 'tanh'))
    for kw, why in ((dict(input_size=513, hidden_size=10, output_size=513), R_SIZES),
                    (dict(input_size=3, hidden_size=6, output_size=12, options={'masked': True, 'residual_enc_dec': False}),
                     R_MASKED),
                    (dict(ode_nn=((1025, 'tanh'),)), R_NET),
                    (dict(ode_nn=((20, 'tanh'),) * 9, enc_nn=((20, 'tanh'),) * 9, readout_nn=((20, 'tanh'),) * 9),
                     R_NHIDDEN),
                    (dict(hidden_size=257, use_rnn=True), R_RNN),
                    (dict(hidden_size=629, ode_nn=None, enc_nn=None, readout_nn=None), R_LDS)):
        cfg = dict(input_size=1, hidden_size=10, output_size=1, ode_nn=nn50, readout_nn=nn50, enc_nn=nn50,
                   use_rnn=False, bias=True, dropout_rate=0.0, options={'residual_enc_dec': False})
        cfg.update(kw)
        with contextlib.redirect_stdout(io.StringIO()), torch.device('meta'):
            m = models.NJODE(**cfg)
        with pytest.raises(NotImplementedError) as e:
            m._get_dims()
        assert 'generic kernels: ' in str(e.value) and why in str(e.value), (kw, str(e.value))
    with capsys.disabled():
        print('\n[envelope] {} grid dims checked: {} accepted, refused {}'.format(len(grid), n_ok, reasons))


def test_torch_library_operator_is_registered_with_a_fake_implementation():
    """njode_amd/ops.py: torch.ops.njode_amd.forward exists (dispatcher-visible operator) and its
    fake implementation gives the output shapes without touching a GPU."""
    import njode_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    schema = str(torch.ops.njode_amd.forward.default._schema)
    assert 'Tensor[] params' in schema and '-> (Tensor, Tensor, Tensor)' in schema
    nn50 = ((50, 'tanh'), (50, 'tanh'))
    m = models.NJODE(input_size=1, hidden_size=10, output_size=1, ode_nn=nn50, readout_nn=nn50,
                     enc_nn=nn50, use_rnn=False, bias=True, dropout_rate=0.0, options={})
    mid = ops.register_model(m)
    with FakeTensorMode():
        hT, loss, cid = torch.ops.njode_amd.forward(
            [torch.empty(3)], torch.empty(7, 1), torch.empty(20, 1),
            torch.empty(20, dtype=torch.int64), torch.empty(7, dtype=torch.int32), None,
            torch.empty(5, dtype=torch.float64), torch.empty(6, dtype=torch.int64), 0.01, 1.0,
            mid, True, False, False)
    assert tuple(hT.shape) == (7, 10) and tuple(loss.shape) == (1,) and cid.dim() == 0


# ---- bench.py --gpus N without a launcher: no GPU needed for these --------
def _run_bench(args, env_extra, timeout=300):
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **env_extra)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(repo, 'bench.py')] + args, env=env, cwd=repo,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def test_gpu_count_comes_from_the_kfd_topology_not_the_runtime(tmp_path, monkeypatch):
    import bench
    root = tmp_path / 'nodes'
    for i, simd in enumerate((0, 1024, 1024, 1024)):          # one CPU node, three GPUs
        (root / str(i)).mkdir(parents=True)
        (root / str(i) / 'properties').write_text('cpu_cores_count 8\nsimd_count {}\n'.format(simd))
    real_listdir, real_open = os.listdir, open

    def fake_listdir(path):
        return real_listdir(str(root)) if path == '/sys/class/kfd/kfd/topology/nodes' else real_listdir(path)

    def fake_open(path, *a, **k):
        if isinstance(path, str) and path.startswith('/sys/class/kfd/kfd/topology/nodes/'):
            path = str(root) + path[len('/sys/class/kfd/kfd/topology/nodes'):]
        return real_open(path, *a, **k)

    monkeypatch.setattr(os, 'listdir', fake_listdir)
    monkeypatch.setattr('builtins.open', fake_open)
    for v in ('ROCR_VISIBLE_DEVICES', 'HIP_VISIBLE_DEVICES', 'CUDA_VISIBLE_DEVICES'):
        monkeypatch.delenv(v, raising=False)
    assert bench.count_gpus_without_runtime() == 3
    monkeypatch.setenv('HIP_VISIBLE_DEVICES', '0,2')
    assert bench.count_gpus_without_runtime() == 2


def test_self_spawned_ranks_that_fail_are_reported_with_their_stderr():
    """No GPU here: both ranks die at torch.cuda.set_device -- the parent must come back with
    their exit code and the tail of their stderr instead of hanging or hiding it."""
    p = _run_bench(['--gpus', '2', '--steps', '1', '--warmup', '0', '--rank-timeout', '240'],
                   {'NJODE_BENCH_SHARE_GPU': '1'})
    if p.returncode == 0:
        pytest.skip('this box has a GPU: the ranks ran')
    assert p.returncode not in (0, 124), p.stderr[-2000:]
    assert 'ranks exited with code' in p.stderr
    assert '  | ' in p.stderr                      # the relayed tail


def test_self_spawned_ranks_are_killed_after_the_rank_timeout():
    import time
    t0 = time.time()
    p = _run_bench(['--gpus', '2', '--steps', '1', '--warmup', '0', '--rank-timeout', '0.2'],
                   {'NJODE_BENCH_SHARE_GPU': '1'})
    assert p.returncode == 124, (p.returncode, p.stderr[-2000:])
    assert 'process group killed' in p.stderr
    assert time.time() - t0 < 60


def test_sigterm_to_the_spawning_parent_takes_the_ranks_down():
    """the ranks live in a session of their own, so a SIGTERM to bench.py must be
    passed on (kill the group, exit non-zero) -- not leave torchrun and N ranks orphaned."""
    import signal
    import subprocess
    import time
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NJODE_BENCH_SHARE_GPU='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    # a launcher that would run for minutes: the parent sits in child.wait()
    p = subprocess.Popen([sys.executable, os.path.join(repo, 'bench.py'), '--gpus', '2', '--steps', '1',
                          '--warmup', '0', '--rank-timeout', '600'], env=env, cwd=repo,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    # find the launcher child (torch.distributed.run, a session leader) before signalling
    child_pid = None
    for _ in range(100):
        time.sleep(0.1)
        out = subprocess.run(['ps', '-o', 'pid=,sid=,args=', '--ppid', str(p.pid)], stdout=subprocess.PIPE,
                             text=True).stdout
        for line in out.splitlines():
            f = line.split(None, 2)
            if len(f) == 3 and 'torch.distributed.run' in f[2]:
                child_pid = int(f[0])
        if child_pid or p.poll() is not None:
            break
    if p.poll() is not None:
        pytest.skip('the ranks finished before they could be signalled')
    assert child_pid is not None
    p.send_signal(signal.SIGTERM)
    rc = p.wait(timeout=60)
    assert rc == 128 + signal.SIGTERM
    for _ in range(100):                      # the launcher's whole session is gone
        alive = subprocess.run(['ps', '-o', 'pid=', '-s', str(child_pid)], stdout=subprocess.PIPE,
                               text=True).stdout.split()
        if not alive:
            break
        time.sleep(0.1)
    assert not alive, alive


def test_hosting_the_plan_does_not_cost_the_ode_forward_a_wave():
    """njode_plan.h: k_ode_fwd_mixed_plan runs the next batch's plan in its first blocks; a kernel's
    register count is the maximum over its branches, so plan code that needs more registers than the
    forward silently takes a wave per SIMD from EVERY forward block (seen: 64 loads in flight in the
    column walk -> 256 VGPRs, step 0.86 -> 1.07 ms).  The build records the compiler's per-kernel
    resources (njode_amd/csrc/_obj/kernel_resources.json): same occupancy with and without the plan."""
    import json
    import os
    import pytest
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'njode_amd', 'csrc',
                        '_obj', 'kernel_resources.json')
    if not os.path.exists(path):
        pytest.skip('no build record (python -m njode_amd.build writes it)')
    res = json.load(open(path))
    def targs(name, kernel):      # the template arguments: up to the mangled parameter list
        return name.split(kernel, 1)[1].split('EEEv', 1)[0]
    plain = {targs(k, 'k_ode_fwd_mixed'): v for k, v in res.items() if 'k_ode_fwd_mixedI' in k}
    hosted = {targs(k, 'k_ode_fwd_mixed_plan'): v for k, v in res.items() if 'k_ode_fwd_mixed_plan' in k}
    assert hosted and len(hosted) == len(plain) and hosted.keys() == plain.keys()   # every forward has its hosting twin
    for key, h in hosted.items():
        p = plain[key]
        assert h['occupancy'] == p['occupancy'] and h['vgpr_spill'] == 0, (key, h, p)


# ---- the options matrix's inputs (tests/test_hip_options_matrix.py) -------------------------------------
def _options_shapes():
    import test_hip_route_matrix as R
    return [(R.DEMO, 'small'), (R.PHYSIO, 'physio'), (R.DEMO, 'tile1')]


def test_irregular_batch_keeps_the_collate_invariants():
    import hip_util
    import test_hip_route_matrix as R
    for c, kind in _options_shapes():
        b0, dt, T = R.make_batch(kind, c)
        b, delta_t = hip_util.irregular_batch(b0, dt, 0.37)
        b_again, _ = hip_util.irregular_batch(R.make_batch(kind, c)[0], dt, 0.37)
        times, ptr, idx = b['times'], b['time_ptr'], b['obs_idx'].numpy()
        B = len(b['start_X'])
        assert delta_t == 0.37 * dt
        for k in ('times', 'time_ptr'):
            assert np.array_equal(b[k], b_again[k])
        assert all(torch.equal(b[k], b_again[k]) for k in ('X', 'obs_idx', 'n_obs_ot'))   # a pure function
        assert len(times) + 1 == len(ptr) and ptr[0] == 0 and ptr[-1] == len(idx) == len(b['X'])
        assert np.all(np.diff(times) > 0) and times[0] == 0.0 and times[-1] == b0['times'][-1]
        assert np.all(np.diff(ptr) >= 0)
        empty = np.nonzero(np.diff(ptr) == 0)[0]
        assert len(empty) and any(0 < e < len(times) - 1 for e in empty)   # an empty slice strictly inside
        assert ptr[-1] > ptr[-2]                                           # the last slice has rows
        for i in range(len(times)):
            rows = idx[ptr[i]:ptr[i + 1]]
            assert np.all(np.diff(rows) > 0)   # sorted by path, at most one row per path and slice
        assert idx[0] == 0 and ptr[1] >= 1     # the t = 0 jump of path 0
        assert np.array_equal(b['n_obs_ot'].numpy(), np.bincount(idx, minlength=B))
        gone = np.nonzero(b['n_obs_ot'].numpy() == 0)[0]
        assert len(gone) >= 1 and 0 not in gone and idx[-1] not in gone
        if 'M' in b:
            assert b['M'].shape == b['X'].shape and bool((b['M'].sum(1) > 0).all())
        # the schedule the rows rely on
        s = Schedule(times, delta_t, T, False)
        assert len(set(s.step_dt.tolist())) >= 2 and not s.has_tail() and s.k_jump[0] == 0 and s.n_steps < 512


@pytest.mark.parametrize('shape', [0, 1])
def test_options_rows_see_a_swapped_weight_and_the_other_loss_form(shape):
    """The oracle's loss of the two row kinds is more than 1 % away from the loss with weight and
    1 - weight swapped and from the loss of the other form: the rows cannot go blind to either."""
    import hip_util
    import test_hip_options_matrix as O
    import test_hip_route_matrix as R
    c, kind = _options_shapes()[shape]
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in models.NJODE(**R.model_cfg(c)).state_dict().items()}
    other = {'easy': 'standard', 'standard': 'easy'}
    for rk, opts in O.ROW_KINDS.items():
        job = dict({'id': rk, 'cfg': list(c), 'batch': kind}, **opts)
        b, dt, T = R.job_batch(job, c)

        def loss(which, weight):
            with torch.no_grad():
                out, _ = hip_util.oracle_forward(R.model_cfg(c, 0.0, which, weight), sd, b, dt, T)
            return float(out[1])
        w, which = opts['weight'], opts['which_loss']
        right = loss(which, w)
        for wrong in (loss(which, 1 - w), loss(other[which], w)):
            assert abs(wrong - right) > 0.01 * abs(right), (rk, kind, right, wrong)
