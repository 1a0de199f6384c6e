"""Every plan builder's arrays against the host planner (tests/plan_host.py), exactly, at the sizes
where the builders branch.

The plan -- row times, per-path links, item lengths, the stable order by length, the trajectory
layout, the split points of the mixed kernels, the tail order -- is integer data and a function of
the batch ``(time_ptr, obs_idx, k_jump)`` alone.  ``njode_plan.h`` promises "same arrays, bit for
bit" from every builder; the parity tests only see a plan through the loss and gradient of
whatever batch they feed it, and cannot fail on a valid but unstable order, tiles of unequal
length or a wrong split point.  Here ``njode_plan_f32`` is called through ``ctypes`` on seeded
integer batches (no model, no values: ``X`` is a valid pointer and nothing else), the plan buffer
-- exactly ``njode_plan_bytes`` bytes inside a guard-band arena -- is cut into its arrays by
``njode_debug_plan_view`` (include/njode_selftest.h), and the parent compares every array the view
says this plan defines with the host planner's:

1. the schedule block is the packed host schedule, bit for bit (copied, or read from pinned memory);
2. rows, links, lengths, histogram, ``base_s`` / ``base16_s`` (and the sort-linked / generic arrays) are equal;
3. ``order`` is THE stable order, element for element;
4. ``t_order`` is a permutation with non-decreasing tail key (within a bin the order is timing-dependent
   by design, k_tail_order's comment);
5. the split points are within range, equal across the builders of a case, and optimal against the
   float64 cost up to the kernel's fp32 evaluation: ``cost(T_dev) <= min cost (1 + 16 * 2**-24)`` -- at most
   four roundings per side, division not correctly rounded.  The running sum of tile lengths stays
   below 2**24 (asserted), so it is exact in fp32 whatever the chunking: that is why equality across
   builders may be demanded.  Where every item has the same length the costs are exact integers on both
   sides and tie exactly: there T must be the smallest minimiser (the argmin's tie rule);
6. the rows together take every branch of the builders (``test_coverage``).

One child process per builder environment (the switches are read once per process); a child runs
its rows over the whole case list, writes the defined arrays to an ``.npz`` and ends with
``njode_plan_barrier_failures() == 0``.  Which builder a row stands for is asserted from the kernel
names of ``njode_profile_read``; a case a builder cannot take by the library's own predicate is
listed in ``FALLBACK`` and must have run the fallback builder.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import plan_host

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)


# ---- the cases -----------------------------------------------------------------------------------------
def _k_jump(rng, nt, K, mode):
    if mode == 'linspace':                    # equal steps between the slices
        return (np.arange(1, nt + 1) * K) // nt
    if mode == 'pow2':                        # geometric item lengths
        k = np.unique(np.concatenate([2 ** np.arange(0, max(int(np.log2(K)), 0) + 1), [K]]))
        assert len(k) == nt, (len(k), nt)
        return k
    if mode == 'repeat' or nt > K:            # repeated values: many zero-length items
        k = np.sort(rng.randint(0, K + 1, size=nt))
    else:
        k = np.sort(rng.choice(np.arange(1, K + 1), size=nt, replace=False))
    if mode == 'jump0':
        k[0] = 0
    k[-1] = K
    return k


def make_case(spec):
    """(B, K, time_ptr, obs_idx, k_jump) of a case description: seeded, a pure function of it."""
    B, nt, K, kind = spec['B'], spec['nt'], spec['K'], spec.get('kind', 'random')
    rng = np.random.RandomState(spec.get('seed', 1) + 7 * B + 13 * nt + K)
    k_jump = _k_jump(rng, nt, K, spec.get('kj', 'regular'))
    allowed = np.ones((nt, B), dtype=bool)
    if kind == 'all':                         # every path observed in every slice
        pick = np.arange(nt * B)
    elif kind == 'owner':                     # one path owns a row in every slice, the others have none
        pick = np.arange(nt) * B + spec['owner']
    elif kind == 'one_long':                  # one item of length K among length-1 items
        assert nt == K and spec['kj'] == 'linspace'
        allowed[:] = False
        left = spec['n'] - 1
        for p in range(1, B):                 # runs of consecutive slices from the first one
            m = min(K, left)
            allowed[:m, p] = True
            left -= m
        assert left == 0
        allowed[K - 1, 0] = True
        pick = np.flatnonzero(allowed.reshape(-1))
    elif kind == 'one_short':                 # ... and the reverse: one short item among items of length ~K
        allowed[:] = False
        allowed[nt - 1, :] = True
        allowed[0, 0] = True
        pick = np.flatnonzero(allowed.reshape(-1))
    else:
        if spec.get('skip_paths'):            # paths p with p % m == m - 1 have no rows
            allowed[:, np.arange(B) % spec['skip_paths'] == spec['skip_paths'] - 1] = False
        if spec.get('skip_slices'):           # empty time slices: repeated time_ptr values
            allowed[np.arange(nt) % spec['skip_slices'] == 1, :] = False
        if spec.get('no_last'):               # ... the paths below it: nothing after the first slice / no rows
            allowed[1:, :spec['no_last']] = False
        ok = np.flatnonzero(allowed.reshape(-1))
        pick = np.sort(rng.choice(ok, size=spec['n'], replace=False))
    sl, path = pick // B, pick % B
    time_ptr = np.concatenate([[0], np.cumsum(np.bincount(sl, minlength=nt))])
    assert int(time_ptr[-1]) == spec.get('n', len(pick)) and k_jump[-1] == K and (np.diff(k_jump) >= 0).all()
    return B, K, time_ptr.astype(np.int64), path.astype(np.int64), k_jump.astype(np.int64)


def _sized(n, K=100, nt=20, **kw):
    return dict(dict(B=n // 8 + 3, nt=nt, K=K, n=n), **kw)


def cases():
    c = {}
    # tiny
    c['tiny_1_1'] = dict(B=1, nt=1, K=1, n=1)
    c['tiny_1_5'] = dict(B=1, nt=5, K=9, kind='all')
    c['tiny_2_3'] = dict(B=2, nt=3, K=5, n=3)
    # n around every threshold of the builders (row blocks of the scan, block counts, count tables)
    for n in (63, 64, 65, 255, 256, 257, 2048, 2049, 4095, 4096, 4097, 8192, 8193, 16383, 16384, 16385):
        c['n{}'.format(n)] = _sized(n)
    c['n16384_K511'] = _sized(16384, K=511, nt=40)       # 32 row blocks: the last thread-per-key table
    c['n20000_K50'] = _sized(20000, K=50, nt=50)         # 79 row blocks: a partial 64-chunk of the wave scan
    # K at the LDS histogram's and the layout tables' limits (the row states its builder: FALLBACK)
    for K in (1, 2, 63, 64, 255, 256, 510, 511, 512, 4095, 4096):
        c['K{}'.format(K)] = dict(B=45, nt=min(K, 12), K=K, n=300 if K > 8 else 45 * min(K, 12) // 2,
                                  kj='regular' if K > 2 else 'repeat')
    # n_times at the plan's LDS limit: repeated k_jump values, i.e. many zero-length items
    for nt in (1, 2, 1499, 1500):
        c['nt{}'.format(nt)] = dict(B=7, nt=nt, K=511 if nt > 2 else 30, n=min(3000, 5 * nt), kj='repeat')
    # shapes of the length distribution
    c['equal_8192'] = dict(B=1024, nt=8, K=64, kind='all', kj='linspace', tie=True)
    c['equal_400'] = dict(B=50, nt=8, K=64, kind='all', kj='linspace', tie=True)
    c['one_long'] = dict(B=130, nt=64, K=64, n=8192, kind='one_long', kj='linspace')
    c['one_short'] = dict(B=8191, nt=3, K=200, kind='one_short')
    c['geometric'] = dict(B=900, nt=9, K=256, n=7000, kj='pow2')
    c['owner'] = dict(B=33, nt=40, K=100, kind='owner', owner=17)
    c['third_empty'] = dict(B=301, nt=20, K=100, n=1500, skip_paths=3)
    c['empty_slices'] = dict(B=99, nt=21, K=100, n=700, skip_slices=4)
    c['jump0'] = dict(B=50, nt=12, K=40, n=333, kj='jump0')
    # the odd dense cell under the coherent 8-byte stores; paths handed out grid-stride; B no multiple of 16
    c['odd_cells'] = dict(B=37, nt=9, K=100, n=200)
    c['grid_stride'] = dict(B=1003, nt=5, K=30, n=2500)
    # tails: paths whose last observation is at step 0 (a jump at 0 and nothing after), at K, or absent
    c['tails'] = dict(B=70, nt=10, K=60, n=250, kj='jump0', skip_paths=5, no_last=9)
    # k_tail_order's limit and the radix fallback past it (dense matrix: 0.5 MB)
    c['B65536'] = dict(B=65536, nt=2, K=20, n=70000)
    c['B65537'] = dict(B=65537, nt=2, K=20, n=70000)
    for name, spec in c.items():
        spec['name'] = name
    return c


CASES = cases()

# ---- the builders --------------------------------------------------------------------------------------
# environment tag -> (environment, [(row tag, shape, mode, extra call flags)]); modes: 'inline' (njode_plan_f32
# builds at once), 'flush' (deferred, launched by njode_plan_flush, schedule read from pinned memory),
# 'hosted' (deferred, carried by another batch's forward call)
TILES = {'NJODE_SEG_CHAIN_MAX': '0'}        # the consumer is the tile kernels: the plan goes on to order and layout
WHOLE = dict(TILES, NJODE_PLAN_INLINE_MAX='100000000')
ENVS = {
    'default': ({}, [('default', 'demo', 'inline', 0), ('generic', 'gen', 'inline', 0),
                     ('masked', 'masked', 'inline', 0)]),
    'tiles': (TILES, [('tiles', 'demo', 'inline', 0), ('flush', 'demo', 'flush', 0), ('hosted', 'demo', 'hosted', 0),
                      ('tails', 'demo', 'inline', 'NEED_HT'), ('tails_flush', 'demo', 'flush', 'NEED_HT')]),
    'blocks1': (dict(WHOLE, NJODE_PLAN_BLOCKS='1'), [('blocks1', 'demo', 'inline', 0)]),
    'blocks3': (dict(WHOLE, NJODE_PLAN_BLOCKS='3'), [('blocks3', 'demo', 'inline', 0)]),
    'blocks200': (dict(WHOLE, NJODE_PLAN_BLOCKS='200'), [('blocks200', 'demo', 'inline', 0)]),
    'stage2': (dict(TILES, NJODE_PLAN_INLINE_MAX='0'), [('stage2', 'demo', 'inline', 0)]),
    'multi': (dict(TILES, NJODE_PLAN_GRID='0'), [('multi', 'demo', 'inline', 0)]),
    'sort': (dict(TILES, NJODE_PLAN='sort'), [('sort', 'demo', 'inline', 0)]),
    'tails_rocprim': (dict(TILES, NJODE_TAIL_SORT='rocprim'), [('tails_rocprim', 'demo', 'inline', 'NEED_HT')]),
}
ONE_LAUNCH_ROWS = ('default', 'tiles', 'flush', 'hosted', 'tails', 'tails_flush', 'blocks1', 'blocks3', 'blocks200',
                   'stage2', 'tails_rocprim')
# Cases a one-launch row cannot take, by fill_plan_job's predicate (K + 1 > 512 keys, n_times + 1 > 1 500): they
# must have run the multi-launch plan instead.  ... and the deferred rows' own refusal: more paths than
# k_tail_order sorts (the plan is then built at once, by k_plan_grid)
FALLBACK = {row: {'K512', 'K4095', 'K4096', 'nt1500'} for row in ONE_LAUNCH_ROWS}
NOT_DEFERRED = {'tails_flush': {'K512', 'K4095', 'K4096', 'nt1500', 'B65537'},
                'flush': {'K512', 'K4095', 'K4096', 'nt1500'}, 'hosted': {'K512', 'K4095', 'K4096', 'nt1500'}}

I32_FIELDS = ('t_of_row', 'first_row', 'last_row', 'item_prev', 'item_next', 'item_kbeg', 'item_len', 'order',
              't_order', 'len_hist', 'path_sorted', 'row_by_path', 'first_j', 'jlo', 'tile_base')


def _gen_cfg():
    w = ((33, 'tanh'), (33, 'tanh'))
    return dict(input_size=3, hidden_size=9, output_size=3, ode_nn=w, readout_nn=w, enc_nn=w, use_rnn=False,
                bias=True, dropout_rate=0.0, options={'residual_enc_dec': True})


# ---- child side ----------------------------------------------------------------------------------------
def pack_schedule(K, time_ptr, k_jump, out=None):
    """The packed schedule block [step_dt | step_t | k_jump | time_f32 | time_ptr] as int32 words: a
    clock of K equal steps on [0, 1]."""
    nt = len(k_jump)
    buf = np.empty(2 * K + 3 * nt + 1, dtype=np.int32) if out is None else out
    f = buf.view(np.float32)
    f[0:K] = np.float32(1.0 / K)
    f[K:2 * K] = (np.arange(K) / K).astype(np.float32)
    buf[2 * K:2 * K + nt] = k_jump
    f[2 * K + nt:2 * K + 2 * nt] = (np.asarray(k_jump) / K).astype(np.float32)
    buf[2 * K + 2 * nt:] = time_ptr
    return buf


def _field_len(name, B, n, K, v):
    return {'first_row': B, 'last_row': B, 'first_j': B, 't_order': B, 'len_hist': K + 1, 'jlo': K + 2,
            'tile_base': v['n_tiles'] + 1}.get(name, n)


class Child:
    def __init__(self):
        import torch
        import test_hip_route_matrix as RM
        from guarded import Arena
        from hip_util import exact_k_batch, hip_model
        from njode_amd import _lib
        self.torch, self.lib, self.L, self.Arena = torch, _lib, _lib.lib(), Arena
        torch.manual_seed(0)
        self.make = {'demo': lambda: hip_model(RM.model_cfg(RM.DEMO)).eval(), 'gen': lambda: hip_model(_gen_cfg()).eval(),
                     'masked': lambda: hip_model(RM.model_cfg(RM.PHYSIO)).eval()}
        self.models = {}
        self.host_batch = exact_k_batch(48, 30, obs_per_path=4, seed=3)      # the batch whose forward hosts plans
        self.stream = torch.cuda.current_stream().cuda_stream
        self.base_flags = _lib.C_GET_LOSS | _lib.C_SAVE_BWD | _lib.C_TRAIN | _lib.C_SCHED_KNOWN

    def host_forward(self):
        from hip_util import hip_forward
        b, dt, T = self.host_batch
        with self.torch.no_grad():
            hip_forward(self.model('demo'), b, dt, T, get_loss=True)

    def model(self, shape):
        if shape not in self.models:
            self.models[shape] = self.make[shape]()
        return self.models[shape]

    def run_case(self, shape, mode, extra, spec, arrays, meta):
        torch, lib, L = self.torch, self.lib, self.L
        B, K, time_ptr, obs_idx, k_jump = make_case(spec)
        n, nt = int(time_ptr[-1]), len(k_jump)
        m = self.model(shape)
        dims, D = m._get_dims(), m.input_size
        flags = self.base_flags | (lib.C_NEED_HT if extra == 'NEED_HT' else 0)
        call_flags = flags | (lib.C_PLAN_DEFER if mode != 'inline' else 0)
        view = lib.plan_view(dims, B, n, nt, K, call_flags)
        need = ctypes.c_size_t(0)
        lib.check(L.njode_plan_bytes(ctypes.byref(dims), B, n, nt, K, flags, ctypes.byref(need)))
        assert need.value == view['plan_bytes'], (need.value, view['plan_bytes'])
        A = self.Arena('cuda', 0).add('plan', need.value).build()
        words = 2 * K + 3 * nt + 1
        if mode == 'inline':
            sched = pack_schedule(K, time_ptr, k_jump)
            base = sched.ctypes.data
        else:       # a pinned block: the plan's first block reads it from there
            pinned = torch.empty(words, dtype=torch.int32).pin_memory()
            sched = pack_schedule(K, time_ptr, k_jump, out=pinned.numpy())
            base = pinned.data_ptr()
        cs = lib.NjodeSchedule(K, nt, base, base + 4 * K, base + 8 * K, base + 8 * K + 4 * nt, base + 8 * K + 8 * nt)
        X = torch.zeros(max(n, 1) * D, device='cuda')
        start_X = torch.zeros(B * D, device='cuda')
        idx = torch.from_numpy(obs_idx.astype(np.int32)).cuda()
        counts = torch.ones(B, dtype=torch.int32, device='cuda')
        cb = lib.NjodeBatch(B, n, start_X.data_ptr(), X.data_ptr(), X.data_ptr() if m.masked else None,
                            idx.data_ptr(), counts.data_ptr(), float(B), 0, None, None)
        torch.cuda.synchronize()
        lib.profile_read()
        lib.check(L.njode_plan_f32(ctypes.byref(dims), ctypes.byref(cb), ctypes.byref(cs), call_flags,
                                   A.ptr('plan'), need.value, self.stream))
        info = {'view': view, 'B': B, 'n': n, 'nt': nt, 'K': K}
        if mode == 'flush':
            info['flushed'] = L.njode_plan_flush()
        elif mode == 'hosted':
            self.host_forward()
            info['flushed'] = L.njode_plan_flush()       # (0: the forward took it)
        torch.cuda.synchronize()
        info['names'] = {k: c for k, (c, _) in lib.profile_read().items()}      # launches per kernel name
        info['guards'] = [list(t) for t in A.check()]
        key = spec['name']
        arrays[key + '/sched_host'] = np.array(sched, dtype=np.int32)
        raw = A.view('plan', torch.uint8).cpu().numpy()
        arrays[key + '/sched'] = raw[view['sched']:view['sched'] + 4 * words].view(np.int32).copy()
        for name in I32_FIELDS:
            if view[name] >= 0:
                ln = _field_len(name, B, n, K, view)
                arrays[key + '/' + name] = raw[view[name]:view[name] + 4 * ln].view(np.int32).copy()
        if view['base_s'] >= 0:
            arrays[key + '/base_s'] = raw[view['base_s']:view['base_s'] + 8 * (K + 3)].view(np.int64).copy()
            arrays[key + '/base16_s'] = raw[view['base16_s']:view['base16_s'] + 8 * (K + 1)].view(np.int64).copy()
        meta[key] = info


def _child(rows, out_dir):
    ch = Child()
    ch.lib.profile_enable(1)
    res = {}
    for row, shape, mode, extra in rows:
        arrays, meta = {}, {}
        for spec in CASES.values():      # every row runs the whole case list
            ch.run_case(shape, mode, extra, spec, arrays, meta)
        np.savez(os.path.join(out_dir, row + '.npz'), **arrays)
        res[row] = meta
    ch.lib.profile_enable(0)
    res['barrier_failures'] = ch.L.njode_plan_barrier_failures()
    with open(os.path.join(out_dir, 'res.json'), 'w') as f:
        json.dump(res, f)


_SNIPPET = r'''
import json, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {repo!r})
import test_hip_plan_arrays as T
T._child(json.loads({rows!r}), {out!r})
'''

RESULTS, DEAD = {}, []


def run_env(tmp_root, tag, timeout=240):
    """The rows of one builder environment: {row: (meta, arrays)}; runs its child once per session."""
    if tag in RESULTS:
        return RESULTS[tag]
    assert not DEAD, 'a child process died {}: nothing more runs on the GPU'.format(DEAD)
    env, rows = ENVS[tag]
    out = tmp_root / tag
    out.mkdir()
    t0 = time.time()
    code = _SNIPPET.format(tests=TESTS, repo=REPO, rows=json.dumps(rows), out=str(out))
    # (a child that died -- a fault, an abort, its time limit -- ends the module: the tests behind it fail
    # before they start anything on the GPU)
    p = subprocess.run(['timeout', '-k', '10', str(timeout), sys.executable, '-c', code],
                       env=dict(os.environ, **env), cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    if p.returncode != 0:
        DEAD.append((tag, p.returncode))
    assert p.returncode == 0, (tag, p.returncode, p.stdout[-4000:])
    with open(out / 'res.json') as f:
        res = json.load(f)
    assert res.pop('barrier_failures') == 0, tag
    got = {row: (meta, dict(np.load(out / (row + '.npz')))) for row, meta in res.items()}
    print('child {}: {} rows, {} plans, {:.1f} s'.format(tag, len(got), sum(len(m) for m, _ in got.values()),
                                                      time.time() - t0))
    RESULTS[tag] = got
    return got


@pytest.fixture(scope='module')
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp('plans')


# ---- parent side ---------------------------------------------------------------------------------------
HOST = {}


def host(name):
    """The host plan of a case, computed once and shared by every row (read-only)."""
    if name not in HOST:
        B, K, time_ptr, obs_idx, k_jump = make_case(CASES[name])
        p = plan_host.plan(B, K, time_ptr, obs_idx, k_jump)
        p.update(B=B, K=K, sched=pack_schedule(K, time_ptr, k_jump))
        for a in p.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        HOST[name] = p
    return HOST[name]


def has(names, k):
    return any(x == k or x.startswith(k + '.') for x in names)


def expected_kernels(row, mode, name, info):
    """(must, must not, launches of k_plan_grid) of a row's kernel names, from what the view says the
    library decided.  (A hosting forward builds its own small plan in line: one k_plan_grid of its own.)"""
    v, must, must_not = info['view'], [], []
    if v['generic']:
        assert ('gen_plan.seg' in info['names']) == bool(v['seg']), info['names']
        return ['gen_plan'], ['k_plan_grid', 'k_dense_link', 'k_link'], 0
    deferred = mode != 'inline' and name not in NOT_DEFERRED[row]
    grids = 1 if mode == 'hosted' else 0
    if mode == 'hosted':
        must.append('k_ode_fwd_mixed')
    if v['one_launch']:
        grids += 0 if mode == 'hosted' and deferred else 1
        must_not += ['k_dense_link', 'k_link', 'k_traj_layout', 'k_cs_scatter', 'sort_rows_by_length']
        (must if v['plan_first_stage'] == 2 else must_not).append('k_row_time')
    else:
        must += ['k_row_time', 'k_link' if v['sort_linked'] else 'k_dense_link']
        must_not += ['k_dense_link' if v['sort_linked'] else 'k_link']
        if v['seg']:
            must += ['k_traj_layout', 'k_cs_scatter' if v['cs_shift'] else 'sort_rows_by_length']
            must_not += ['sort_rows_by_length' if v['cs_shift'] else 'k_cs_scatter']
    if v['tails']:
        must.append('k_tail_keys' if v['tail_radix'] else 'k_tail_order')
        must_not.append('k_tail_order' if v['tail_radix'] else 'k_tail_keys')
    return must, must_not, grids


SPLIT_TOL = 1.0 + 16 * 2.0 ** -24
SPLITS = {}        # case -> {row: (T backward, T forward)} and the host's cost curves


def check_plan(row, mode, name, info, arr, errors):
    """One plan against the host planner; every disagreement is one line of ``errors``."""
    h, v = host(name), info['view']
    B, K, n = h['B'], h['K'], h['n']
    tag = '{} / {}'.format(row, name)

    def get(field):
        return arr['{}/{}'.format(name, field)]

    def same(field, ref, what=None):
        got = get(field)
        ref = np.asarray(ref, dtype=np.int64)
        if not np.array_equal(got.astype(np.int64), ref):
            bad = np.flatnonzero(got.astype(np.int64) != ref)[:5] if got.shape == ref.shape else 'shape'
            errors.append('{}: {} differs from the host planner at {} (device {}, host {})'.format(
                tag, what or field, bad, got[bad] if got.shape == ref.shape else got.shape,
                ref[bad] if got.shape == ref.shape else ref.shape))

    if info['guards']:
        errors.append('{}: wrote outside the plan buffer: {}'.format(tag, info['guards']))
    try:
        must, must_not, grids = expected_kernels(row, mode, name, info)
        assert info['names'].get('k_plan_grid', 0) == grids, ('launches of k_plan_grid', info['names'], grids)
        for k in must:
            assert has(info['names'], k), ('did not run', k, info['names'])
        for k in must_not:
            assert not has(info['names'], k), ('ran', k, info['names'])
        if mode != 'inline':
            deferred = name not in NOT_DEFERRED[row]
            assert info['flushed'] == (1 if mode == 'flush' and deferred else 0), ('flushed', info['flushed'])
    except AssertionError as e:
        errors.append('{}: {}'.format(tag, e))
    # 1. the schedule block
    if not (np.array_equal(get('sched'), h['sched']) and np.array_equal(get('sched_host'), h['sched'])):
        errors.append('{}: the schedule block differs from the packed host schedule'.format(tag))
    # 2. rows, links, lengths, layout
    for f in ('t_of_row', 'first_row', 'last_row', 'item_prev', 'item_next', 'item_kbeg', 'item_len', 'len_hist',
              'path_sorted', 'row_by_path', 'first_j', 'jlo', 'tile_base'):
        if v[f] >= 0:
            same(f, h[f])
    if v['base_s'] >= 0:
        same('base_s', np.concatenate([h['base_s'], get('base_s')[K + 1:]]), 'base_s[0..K]')
        same('base16_s', h['base16_s'])
    # 3. THE stable order
    if v['order'] >= 0:
        same('order', h['order'])
    # 4. the tail order
    if v['t_order'] >= 0:
        t = get('t_order').astype(np.int64)
        if not np.array_equal(np.sort(t), np.arange(B)):
            errors.append('{}: t_order is no permutation of [0, B)'.format(tag))
        elif (np.diff(h['tail_key'][t]) < 0).any():
            errors.append('{}: t_order is not sorted by tail key'.format(tag))
    # 5. split points
    if v['base_s'] >= 0 and v['split_on'] and v['lds_cnt']:
        sp = SPLITS.setdefault(name, {'rows': {}, 'cfg': None})
        cfg = (v['split_ns'], v['split_nw'], v['split_r'])
        if sp['cfg'] is None:
            assert h['tile_len'].sum() < 2 ** 24, (name, 'the sum of tile lengths must stay exact in fp32')
            cost = plan_host.SplitCost(h['tile_len'], *cfg)
            sp.update(cfg=cfg, costs=[cost.costs(0), cost.costs(1)])
        if cfg != sp['cfg']:
            errors.append('{}: SplitCfg {} differs from the other rows\' {}'.format(tag, cfg, sp['cfg']))
        T = [int(x) for x in get('base_s')[K + 1:K + 3]]
        sp['rows'][row] = T
        n_tiles = (n + 15) // 16
        for w in (0, 1):
            costs = sp['costs'][w]
            if not 0 <= T[w] <= n_tiles:
                errors.append('{}: split point {} = {} outside [0, {}]'.format(tag, w, T[w], n_tiles))
            elif not costs[T[w]] <= costs.min() * SPLIT_TOL:
                errors.append('{}: split point {} = {} costs {!r}, the optimum T = {} costs {!r}'.format(
                    tag, w, T[w], costs[T[w]], int(np.argmin(costs)), costs.min()))
            elif CASES[name].get('tie') and T[w] != int(np.argmin(costs)):
                errors.append('{}: split point {} = {} is not the smallest of the tied minimisers (T = {})'.format(
                    tag, w, T[w], int(np.argmin(costs))))


@pytest.mark.parametrize('tag', list(ENVS))
def test_plan_arrays_equal_the_host_planner(tag, tmp_root):
    got = run_env(tmp_root, tag)
    errors, plans = [], 0
    modes = {row: mode for row, _, mode, _ in ENVS[tag][1]}
    for row, (meta, arr) in got.items():
        for name, info in meta.items():
            check_plan(row, modes[row], name, info, arr, errors)
            plans += 1
        # the cases this row's builder could not take, by name
        if row in FALLBACK:
            fell = {name for name, info in meta.items() if not info['view']['one_launch']}
            if fell != FALLBACK[row]:
                errors.append('{}: the multi-launch plan built {} where {} were expected'.format(row, fell, FALLBACK[row]))
    print('{}: {} plans compared'.format(tag, plans))
    assert not errors, '\n'.join(errors[:60])


def test_split_points_agree_across_builders_and_cover_both_ends(tmp_root):
    for tag in ENVS:
        run_env(tmp_root, tag)
    errors = []
    where = {'first': [], 'inside': [], 'last': []}
    for name, sp in SPLITS.items():
        Ts = set(map(tuple, sp['rows'].values()))
        if len(Ts) != 1:
            errors.append('{}: the builders disagree on the split points: {}'.format(name, sp['rows']))
        for w in (0, 1):      # where the HOST's optimum lies
            costs = sp['costs'][w]
            best = np.flatnonzero(costs <= costs.min())
            n_tiles = len(costs) - 1
            kind = 'first' if best[0] == 0 else ('last' if best[0] == n_tiles else 'inside')
            where[kind].append((name, w))
    assert len(SPLITS) >= 30, sorted(SPLITS)
    assert all(where.values()), where
    print('split points: {} cases; optimum at 0 / inside / at n_tiles: {} / {} / {}'.format(
        len(SPLITS), len(where['first']), len(where['inside']), len(where['last'])))
    assert not errors, '\n'.join(errors)


def test_coverage(tmp_root):
    """The rows together took every branch of the builders, read from the views and the kernel names."""
    for tag in ENVS:
        run_env(tmp_root, tag)
    seen = set()
    for tag, (_, rows) in ENVS.items():
        for row, shape, mode, _ in rows:
            meta = RESULTS[tag][row][0]
            for name, info in meta.items():
                v, names = info['view'], info['names']
                if v['generic']:
                    seen.add('generic seg' if v['seg'] else 'generic lockstep')
                    continue
                seen.add('sort-linked' if v['sort_linked'] else 'dense')
                seen.add('segment' if v['seg'] else 'lockstep')
                if v['one_launch']:
                    seen.add('one block' if v['plan_blocks'] == 1 else 'several blocks')
                    seen.add('whole' if v['plan_first_stage'] == 0 else 'from stage 2')
                    if v['links_only']:
                        seen.add('links only')
                    else:
                        seen.add('large table' if v['cs_large'] else 'small table')
                        seen.add('thread-per-key scan' if v['scan_thread_per_key'] else 'wave-per-key scan')
                        if v['cs_large'] and v['plan_first_stage'] == 0 and info['n'] == 16384:
                            seen.add('in-line and large table')
                    if mode == 'inline':
                        seen.add('in-line')
                    elif name not in NOT_DEFERRED[row]:
                        seen.add('hosted' if mode == 'hosted' and names.get('k_plan_grid', 0) == 1 else 'flushed')
                elif v['seg']:
                    seen.add('counting sort' if has(names, 'k_cs_scatter') else 'radix sort')
                    seen.add('lds_cnt on' if v['lds_cnt'] else 'lds_cnt off')
                    seen.add('multi-launch')
                if v['tails']:
                    seen.add('k_tail_order' if has(names, 'k_tail_order') else 'radix tail sort')
    want = {'generic seg', 'sort-linked', 'dense', 'segment', 'lockstep', 'one block', 'several blocks', 'whole',
            'from stage 2', 'links only', 'large table', 'small table', 'thread-per-key scan', 'wave-per-key scan',
            'in-line and large table', 'in-line', 'hosted', 'flushed', 'counting sort', 'radix sort', 'lds_cnt on',
            'lds_cnt off', 'multi-launch', 'k_tail_order', 'radix tail sort'}
    assert want <= seen, sorted(want - seen)
