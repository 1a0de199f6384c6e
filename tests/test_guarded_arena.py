"""The guard-band arena (tests/guarded.py) on CPU tensors: exact lengths, aligned starts, guard
contents, and that a single byte written just outside a buffer is named."""
import numpy as np
import torch

from guarded import ALIGN, MIN_GUARD, Arena, guard_bytes

# (name, bytes, kind): odd lengths, a length that is no multiple of 4, one above 2 MiB, an empty one
SPECS = [('params', 4 * 6131, 'nan32'), ('obs_idx', 4 * 37, 'index'), ('n_obs_ot', 4 * 37, 'count'), ('observed', 101 * 37, 'index'),
         ('paths', 8 * 3 * 37, 'nan64'), ('hT', 4 * 37 * 10, 'pattern'), ('loss', 4, 'pattern'),
         ('workspace', 3 * MIN_GUARD + 256, 'pattern'), ('empty', 0, 'pattern')]


def make(phase=0):
    a = Arena('cpu', phase)
    for name, n, kind in SPECS:
        if kind == 'count':      # an integer input of small counts: never 0
            a.add(name, n, 'index', modulo=3, base=1)
        else:
            a.add(name, n, kind, modulo=3)
    return a.build()


def test_lengths_are_exact_and_starts_aligned():
    a = make()
    assert a.mem.data_ptr() % ALIGN == 0
    spans = []
    for name, n, kind in SPECS:
        assert a.nbytes(name) == n and a.view(name).numel() == n
        assert a.ptr(name) % ALIGN == 0, name
        off = a.ptr(name) - a.mem.data_ptr()
        assert a.view(name).data_ptr() == a.ptr(name) if n else True
        spans.append((off, off + n, guard_bytes(n)))
    assert guard_bytes(0) == MIN_GUARD and guard_bytes(3 * MIN_GUARD + 256) >= (3 * MIN_GUARD + 256) // 2
    # a guard of the stated size on both sides of every buffer, no two buffers closer than both guards
    assert spans[0][0] >= spans[0][2]
    for (s0, e0, g0), (s1, e1, g1) in zip(spans, spans[1:]):
        assert s1 - e0 >= g0 + g1
    assert a.mem.numel() - spans[-1][1] >= spans[-1][2]


def test_guard_contents_cannot_mislead_a_kernel():
    for phase in (0, 1):
        a = make(phase)
        for name, lo, start, size, hi, kind, modulo in a.layout:
            before = a.mem[lo:start]
            after = a.mem[(start + size + 3) // 4 * 4:hi]
            for g in (before, after):
                i32 = g.view(torch.int32)
                if kind == 'pattern':
                    assert int(i32.min()) >= 1 and int(i32.max()) <= 3
                    assert torch.isfinite(g.view(torch.float32)).all()
                elif kind == 'index':
                    base = modulo[0]
                    assert name != 'n_obs_ot' or base == 1
                    assert int(i32.min()) >= base and int(i32.max()) < base + 3
                elif kind == 'nan32':
                    assert torch.isnan(g.view(torch.float32)).all()
                else:
                    g8 = g[(-g.data_ptr()) % 8:]
                    assert torch.isnan(g8[:g8.numel() // 8 * 8].view(torch.float64)).all()
    # the two phases differ in every word of a pattern guard
    a, b = make(0), make(1)
    start, size = a.where['hT']
    wa = a.mem[start - 4096:start].view(torch.int32)
    wb = b.mem[start - 4096:start].view(torch.int32)
    assert (wa != wb).all() and (a.view('hT', torch.int32) != b.view('hT', torch.int32)).all()


def test_an_untouched_arena_reports_nothing():
    a = make()
    assert a.check() == []
    # writing every byte INSIDE every buffer is not reported
    for name, n, kind in SPECS:
        a.view(name).fill_(0xAB)
    a.put('loss', torch.tensor([1.5]))
    assert float(a.view('loss', torch.float32)[0]) == 1.5
    assert a.check() == []


def test_a_planted_byte_outside_a_buffer_is_named():
    a = make()
    for name, n, kind in SPECS:
        start = a.where[name][0]
        for side, off in (('after', n), ('before', -1), ('after', n + 5), ('before', -4097)):
            old = int(a.mem[start + off])
            a.mem[start + off] = old ^ 0x10
            assert a.check() == [(name, side, off)], (name, side, off, a.check())
            a.mem[start + off] = old
    assert a.check() == []
    # both sides of two buffers at once, the first changed byte of each
    s_h, n_h = a.where['hT']
    s_l, n_l = a.where['loss']
    for pos in (s_h - 8, s_h - 3, s_h + n_h + 2, s_h + n_h + 9, s_l + n_l):
        a.mem[pos] = 0xFF
    assert a.check() == [('hT', 'before', -8), ('hT', 'after', n_h + 2), ('loss', 'after', n_l)]
    assert np.all(a.view('hT').numpy() == a.image[s_h:s_h + n_h].numpy())


def test_the_bounds_table_is_well_formed():
    """CPU side of tests/test_hip_buffer_bounds.py: its shape-generic rows are shapes the generic
    kernels take, with sizes that are no multiples of 4, one with the GRU jump and one with
    per-network descriptions; every job has its expected kernels; every compiled shape has a route."""
    import test_hip_buffer_bounds as BB
    from gen_envelope import restate_cfg
    from njode_amd import models
    from njode_amd.build import CONFIGS
    for name, (cfg, (B, K, _), drop) in BB.GEN.items():
        why, model = restate_cfg(cfg)
        assert why is None, (name, why)
        assert all(cfg[k] % 4 for k in ('input_size', 'hidden_size', 'output_size')) and B % 16, name
        widths = [w for k in ('ode_nn', 'enc_nn', 'readout_nn') for w in models._desc_of(cfg[k])[1]]
        assert drop == 0.0 or max(widths) <= 64, name
    assert any(c['use_rnn'] for c, _, _ in BB.GEN.values())
    assert any(len({c['ode_nn'], c['enc_nn'], c['readout_nn']}) > 1 for c, _, _ in BB.GEN.values())
    envs, expect = BB.table()
    ids = [j['id'] for _, js in envs.values() for j in js]
    assert len(ids) == len(set(ids)) and set(expect) == set(ids) - {'adam'}
    for c in CONFIGS:
        assert BB.routes(c), c
