"""tests/plan_host.py, the host planner the device plan builders are held to
(tests/test_hip_plan_arrays.py), against a brute-force per-path loop: the yardstick is not taken
on trust.  No GPU."""
import numpy as np

import plan_host

KEYS = ('t_of_row', 'row_by_path', 'path_sorted', 'first_j', 'first_row', 'last_row', 'item_prev', 'item_next',
        'item_kbeg', 'item_len', 'order', 'len_hist', 'cnt', 'base_s', 'base16_s', 'tail_key', 'jlo', 'tile_len',
        'tile_base')


def _same(tag, got, ref):
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), np.asarray(ref[k], dtype=np.int64)), (tag, k, got[k], ref[k])


def test_host_planner_matches_the_per_path_loop_on_random_tiny_batches():
    rng = np.random.RandomState(20)
    seen = dict(empty_slice=0, empty_path=0, zero_len=0, jump0=0, partial_tile=0, two_tiles=0)
    for case in range(400):
        B, K, time_ptr, obs_idx, k_jump = plan_host.random_case(rng)
        got = plan_host.plan(B, K, time_ptr, obs_idx, k_jump)
        _same((case, B, K, time_ptr.tolist(), obs_idx.tolist(), k_jump.tolist()), got,
              plan_host.plan_loops(B, K, time_ptr, obs_idx, k_jump))
        seen['empty_slice'] += bool((np.diff(time_ptr) == 0).any())
        seen['empty_path'] += bool((got['first_row'] < 0).any())
        seen['zero_len'] += bool((got['item_len'] == 0).any())
        seen['jump0'] += bool(k_jump[0] == 0)
        seen['partial_tile'] += bool(got['n'] % 16)
        seen['two_tiles'] += bool(got['n'] > 16)
    assert all(v >= 20 for v in seen.values()), seen


def test_host_planner_invariants():
    """What the consuming kernels rely on, stated independently of either implementation."""
    rng = np.random.RandomState(21)
    for case in range(100):
        B, K, time_ptr, obs_idx, k_jump = plan_host.random_case(rng, B_max=40, nt_max=9, K_max=30)
        p = plan_host.plan(B, K, time_ptr, obs_idx, k_jump)
        n, ln, order = p['n'], p['item_len'], p['order']
        assert sorted(order.tolist()) == list(range(n))
        assert (np.diff(ln[order]) <= 0).all()
        eq = np.diff(ln[order]) == 0
        assert (np.diff(order)[eq] > 0).all()                     # stable
        assert p['len_hist'].sum() == n and (ln >= 0).all() and (ln <= K).all()
        # base_s is the record base of step s: the items still running at step s are a prefix of the order
        for s in range(K + 1):
            assert p['cnt'][s] == (ln > s).sum()
        assert p['base_s'][K] + p['cnt'][K] == ln.sum()
        assert (p['base16_s'] % 16 == 0).all() and (p['base16_s'] >= p['base_s']).all()
        # every path's items tile [0, its last jump) without a gap
        for b in range(B):
            r, k = p['first_row'][b], 0
            while r >= 0:
                assert p['item_kbeg'][r] == k and obs_idx[r] == b
                k += ln[r]
                assert k == k_jump[p['t_of_row'][r]]
                last, r = r, p['item_next'][r]
                assert r < 0 or p['item_prev'][r] == last
            assert p['tail_key'][b] == k and (p['first_row'][b] < 0 or p['last_row'][b] == last)
        assert (np.diff(p['jlo']) >= 0).all() and p['jlo'][0] == 0 and p['jlo'][K + 1] == len(k_jump)


def test_plan_view_lays_disjoint_arrays_inside_the_plan_buffer():
    """njode_debug_plan_view (include/njode_selftest.h) launches nothing: its offsets are checked here,
    without a GPU, for both kernel families -- every array the view defines lies inside
    njode_plan_bytes and overlaps no other."""
    import ctypes
    import os

    import pytest
    from njode_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libnjode_hip.so not built in this checkout (run __graft_entry__.build())')
    import test_hip_plan_arrays as T
    L = _lib.lib()
    dims = {'demo': _lib.NjodeDims(1, 10, 1, 2, 50, _lib.ACT_TANH, _lib.F_RESIDUAL),
            'masked': _lib.NjodeDims(41, 41, 41, 2, 50, _lib.ACT_TANH, _lib.F_MASKED | _lib.F_RESIDUAL),
            'generic': _lib.NjodeDims(3, 9, 3, 2, 33, _lib.ACT_TANH, _lib.F_RESIDUAL)}
    base = _lib.C_GET_LOSS | _lib.C_SAVE_BWD | _lib.C_TRAIN | _lib.C_SCHED_KNOWN
    kinds = set()
    for shape, d in dims.items():
        for name in ('tiny_1_1', 'n257', 'n16384', 'K512', 'K4096', 'nt1500', 'B65537'):
            for flags in (base, base | _lib.C_NEED_HT, base | _lib.C_NEED_HT | _lib.C_PLAN_DEFER):
                B, K, time_ptr, obs_idx, k_jump = T.make_case(T.CASES[name])
                n, nt = int(time_ptr[-1]), len(k_jump)
                v = _lib.plan_view(d, B, n, nt, K, flags)
                need = ctypes.c_size_t(0)
                _lib.check(L.njode_plan_bytes(ctypes.byref(d), B, n, nt, K, flags & ~_lib.C_PLAN_DEFER, ctypes.byref(need)))
                assert v['plan_bytes'] == need.value
                spans = [(v['sched'], 4 * (2 * K + 3 * nt + 1), 'sched')]
                for f in T.I32_FIELDS:
                    if v[f] >= 0:
                        spans.append((v[f], 4 * T._field_len(f, B, n, K, v), f))
                if v['base_s'] >= 0:
                    spans += [(v['base_s'], 8 * (K + 3), 'base_s'), (v['base16_s'], 8 * (K + 1), 'base16_s')]
                spans.sort()
                for (o0, l0, f0), (o1, _, f1) in zip(spans, spans[1:]):
                    assert o0 + l0 <= o1, (shape, name, f0, f1)
                assert spans[0][0] >= 0 and spans[-1][0] + spans[-1][1] <= need.value, (shape, name, spans[-1])
                kinds.add((v['generic'], v['seg'], v['sort_linked'], v['one_launch'], v['tails']))
                # what the header promises of each plan kind
                assert (v['order'] >= 0) == bool(v['seg'] and not v['links_only'])
                assert (v['t_order'] >= 0) == bool(v['tails'])
                assert (v['path_sorted'] >= 0) == bool(v['sort_linked'] and not v['generic'])
                assert (v['jlo'] >= 0) == bool(v['generic']) and (v['tile_base'] >= 0) == bool(v['generic'] and v['seg'])
    assert len(kinds) >= 6, kinds


def test_split_cost_by_hand():
    """Three tiles of lengths 8, 2, 1; two four-wave blocks at r = 2, four workers."""
    c = plan_host.SplitCost([8, 2, 1], ns=[2, 0], nw=[4, 4], r=[2.0, 2.0])
    assert c.cost(0, 0) == max(8, 11 / 4)                         # everything on the workers
    assert c.cost(1, 0) == max(max(8, 8 / 2) / 2.0, max(2, 3 / 4))
    assert c.cost(2, 0) == max(max(8, 10 / 2) / 2.0, max(1, 1 / 4))
    assert c.cost(3, 0) == max(8, 11 / 2) / 2.0                   # nothing left for the workers
    assert c.cost(0, 1) == 8 and np.isinf(c.cost(1, 1))           # no four-wave blocks: only T = 0
    assert np.array_equal(c.costs(0), [c.cost(T, 0) for T in range(4)])
    assert int(np.argmin(c.costs(0))) == 1                        # ties go to the smaller T
