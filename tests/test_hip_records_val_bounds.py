"""The caller-owned buffers of njode_records_val_count / _val_fill (include/njode_records.h) at
exactly their stated sizes inside the guard bands of tests/guarded.py, as
tests/test_hip_records_bounds.py holds the older entry points: the store, the batch indices,
``val_ptr``, the workspace of exactly ``njode_records_val_bytes`` and the four outputs lie in ONE
arena; a call must leave all guards as they were and give the wrapper's bits under both guard
images.  And every refusal of the two calls, made before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

from guarded import Arena
from njode_amd import _lib, records, synthetic_physionet

pytestmark = pytest.mark.gpu

SIZES = [(B, dim) for B in (1, 3, 65, 257) for dim in (1, 41)]
N_REC = 300


def _vp(A, name):
    return ctypes.c_void_p(A.ptr(name)) if A.nbytes(name) else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('normalise', [True, False], ids=['normalised', 'raw'])
def test_validation_collate_stays_inside_its_buffers(normalise):
    L = _lib.lib()
    errors, st = [], _stream()
    for B, dim in SIZES:
        tag = 'B={} dim={}'.format(B, dim)
        recs = synthetic_physionet.make_climate_records(N_REC, dim, n_obs_range=(1, 9), seed=B + dim)
        kw = {}
        if normalise:
            kw = dict(data_min=np.full(dim, 0.25, dtype=np.float32),
                      data_max=np.full(dim, 2.0, dtype=np.float32))
        ds = records.RecordDataset.from_records(recs, time_div=None, drop_unobserved=False,
                                                device='cuda', **kw)
        # (a device tensor: repeated records are allowed there)
        idx = torch.as_tensor(np.random.RandomState(B).randint(0, N_REC, size=B).astype(np.int32)).cuda()
        max_val = 3
        g_cut = ds.val_cut(120)
        ref = ds.collate_val(idx, 120, max_val)
        n_val = int(ref['index_val'].numel())
        ref_g = torch.from_numpy(np.searchsorted(ds.grid, ref['times_val'].cpu().numpy()).astype(np.int32))
        N, R, G, D = ds.n_records, ds.n_rows, ds.n_grid, dim
        need = ctypes.c_size_t(0)
        _lib.check(L.njode_records_val_bytes(B, ctypes.byref(need)))
        assert need.value == 8 * B
        for phase in (0, 1):
            A = Arena('cuda', phase)
            A.add('row_ptr', 4 * (N + 1), 'index', modulo=3).add('row_g', 4 * R, 'index', modulo=min(G, 3))
            A.add('vals', 4 * R * D, 'nan32').add('mask', R * D, 'index', modulo=2)
            A.add('att_min', 4 * D if normalise else 0, 'nan32').add('att_max', 4 * D if normalise else 0, 'nan32')
            A.add('idx', 4 * B, 'index', modulo=min(N, 3))
            A.add('val_ptr', 4 * (B + 1)).add('ws', need.value)
            A.add('X_val', 4 * n_val * D).add('M_val', 4 * n_val * D).add('g_val', 4 * n_val)
            A.add('index_val', 4 * n_val).build()
            for k in ('row_ptr', 'row_g', 'vals', 'mask'):
                A.put(k, ds._dev[k])
            if normalise:
                A.put('att_min', ds._dev['att_min']), A.put('att_max', ds._dev['att_max'])
            A.put('idx', idx)
            store = _lib.NjodeRecordStore(N, R, D, G, 0, 0, A.ptr('row_ptr'), A.ptr('row_g'),
                                          A.ptr('vals'), A.ptr('mask'),
                                          A.ptr('att_min') if normalise else None,
                                          A.ptr('att_max') if normalise else None)
            ws = ctypes.c_void_p(A.ptr('ws'))
            rc = L.njode_records_val_count(ctypes.byref(store), _vp(A, 'idx'), B, g_cut, max_val,
                                           _vp(A, 'val_ptr'), ws, need.value, st)
            trips = A.check()
            val_ptr = A.view('val_ptr', torch.int32).cpu().numpy()
            if rc or trips or val_ptr[-1] != n_val or np.any(np.diff(np.sort(val_ptr)) > max_val):
                errors.append('{} count phase {}: rc {} guards {} L {} (wrapper {})'.format(
                    tag, phase, rc, trips, val_ptr[-1], n_val))
                continue
            rc = L.njode_records_val_fill(ctypes.byref(store), _vp(A, 'idx'), B, g_cut, max_val,
                                          _vp(A, 'val_ptr'), n_val, _vp(A, 'X_val'), _vp(A, 'M_val'),
                                          _vp(A, 'g_val'), _vp(A, 'index_val'), ws, need.value, st)
            trips = A.check()
            if rc or trips:
                errors.append('{} fill phase {}: rc {} guards {}'.format(tag, phase, rc, trips))
            for name, want in (('X_val', ref['X_val']), ('M_val', ref['M_val']),
                               ('index_val', ref['index_val']), ('g_val', ref_g.cuda())):
                got = A.view(name, want.dtype)
                if not torch.equal(got.view(torch.uint8), want.contiguous().reshape(-1).view(torch.uint8)):
                    errors.append('{} fill phase {}: {} differs from the wrapper call'.format(tag, phase, name))
    assert not errors, '\n'.join(errors)


@pytest.fixture(scope='module')
def call():
    """One valid pair of calls on a small store, with everything a refusal test swaps out."""
    recs = synthetic_physionet.make_climate_records(20, 3, n_obs_range=(4, 9), seed=1)
    ds = records.RecordDataset.from_records(recs, time_div=None, drop_unobserved=False, device='cuda')
    B = 7
    idx = torch.arange(B, dtype=torch.int32, device='cuda')
    val_ptr = torch.zeros(B + 1, dtype=torch.int32, device='cuda')
    ws = torch.zeros(8 * B, dtype=torch.uint8, device='cuda')
    out = {k: torch.zeros(3 * B * 3, dtype=torch.float32, device='cuda') for k in ('X_val', 'M_val')}
    out.update({k: torch.zeros(3 * B, dtype=torch.int32, device='cuda') for k in ('g_val', 'index_val')})
    return ds, B, idx, val_ptr, ws, out


def _count(ds, B, idx, val_ptr, ws, out, store=None, g_cut=None, max_val=3, ws_bytes=None, null=()):
    p = lambda name, t: ctypes.c_void_p(None if name in null else t.data_ptr())  # noqa: E731
    return _lib.lib().njode_records_val_count(
        ctypes.byref(store or ds._store) if store is not False else None, p('idx', idx), B,
        ds.val_cut(150) if g_cut is None else g_cut, max_val, p('val_ptr', val_ptr), p('ws', ws),
        ws.numel() if ws_bytes is None else ws_bytes, _stream())


def _fill(ds, B, idx, val_ptr, ws, out, store=None, g_cut=None, max_val=3, ws_bytes=None, L=None,
          null=()):
    p = lambda name, t: ctypes.c_void_p(None if name in null else t.data_ptr())  # noqa: E731
    return _lib.lib().njode_records_val_fill(
        ctypes.byref(store or ds._store) if store is not False else None, p('idx', idx), B,
        ds.val_cut(150) if g_cut is None else g_cut, max_val, p('val_ptr', val_ptr),
        3 * B if L is None else L, p('X_val', out['X_val']), p('M_val', out['M_val']),
        p('g_val', out['g_val']), p('index_val', out['index_val']), p('ws', ws),
        ws.numel() if ws_bytes is None else ws_bytes, _stream())


def _altered(ds, **fields):
    s = ds._store
    kw = {name: getattr(s, name) for name, _ in _lib.NjodeRecordStore._fields_}
    kw.update(fields)
    return _lib.NjodeRecordStore(*[kw[name] for name, _ in _lib.NjodeRecordStore._fields_])


def test_workspace_one_byte_short_is_refused(call):
    ds, B = call[0], call[1]
    need = ctypes.c_size_t(0)
    _lib.check(_lib.lib().njode_records_val_bytes(B, ctypes.byref(need)))
    assert need.value == call[4].numel()
    for fn in (_count, _fill):
        assert fn(*call) == _lib.NJODE_OK
    torch.cuda.synchronize()
    call[3].zero_()
    for t in call[5].values():
        t.zero_()
    for fn in (_count, _fill):
        assert fn(*call, ws_bytes=need.value - 1) == _lib.E_WORKSPACE
        assert fn(*call, null=('ws',)) == _lib.E_WORKSPACE
    torch.cuda.synchronize()
    # refused before any launch: nothing was written
    for t in (call[3], *call[5].values()):
        assert not t.any()


def test_bad_arguments_are_refused(call):
    ds, B = call[0], call[1]
    L = _lib.lib()
    bad = _lib.E_BADARG
    for fn in (_count, _fill):
        assert fn(*call, store=False) == bad                                      # null store
        for field in ('row_ptr', 'row_g', 'vals', 'mask'):
            assert fn(*call, store=_altered(ds, **{field: None})) == bad, field   # null array
        for field in ('n_records', 'n_rows', 'dim', 'n_grid'):
            for v in (0, -1):
                assert fn(*call, store=_altered(ds, **{field: v})) == bad, field
        assert fn(*call, store=_altered(ds, drop_unobserved=1)) == bad
        assert fn(*call, null=('idx',)) == bad and fn(*call, null=('val_ptr',)) == bad
        for v in (0, -3):
            assert fn(call[0], v, *call[2:]) == bad                               # B
            assert fn(*call, max_val=v) == bad
        for g in (-1, ds.n_grid + 1):
            assert fn(*call, g_cut=g) == bad
        assert fn(*call, g_cut=0) == _lib.NJODE_OK and fn(*call, g_cut=ds.n_grid) == _lib.NJODE_OK
    assert _fill(*call, L=-1) == bad
    for name in ('X_val', 'M_val', 'g_val', 'index_val'):
        assert _fill(*call, null=(name,)) == bad, name                          # null output
    # ... which L = 0 allows
    assert _fill(*call, L=0, null=('X_val', 'M_val', 'g_val', 'index_val')) == _lib.NJODE_OK
    need = ctypes.c_size_t(0)
    assert L.njode_records_val_bytes(0, ctypes.byref(need)) == bad
    assert L.njode_records_val_bytes(4, None) == bad
    torch.cuda.synchronize()
