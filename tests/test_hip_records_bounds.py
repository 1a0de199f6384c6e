"""Every caller-owned buffer of include/njode_records.h at exactly its stated size inside the guard
bands of tests/guarded.py -- what tests/test_hip_buffer_bounds.py does for the older headers.  The
store, the batch indices, the phase-1 outputs, the workspace of exactly ``njode_records_bytes`` and
every output of the three entry points lie in ONE arena; a call must leave all guards as they
were and give the wrapper's bits under both guard images."""
import ctypes

import numpy as np
import pytest
import torch

from guarded import Arena
from njode_amd import _lib, records, synthetic_physionet

pytestmark = pytest.mark.gpu

SIZES = [(B, dim) for B in (1, 3, 65, 257) for dim in (1, 41)]


def _vp(A, name):
    return ctypes.c_void_p(A.ptr(name)) if A.nbytes(name) else ctypes.c_void_p(0)


def _check(errors, tag, what, phase, rc, A, outputs):
    trips = A.check()
    if rc or trips:
        errors.append('{} {} phase {}: rc {} guards {}'.format(tag, what, phase, rc, trips))
    for name, ref in outputs.items():
        got = A.view(name, ref.dtype)
        if not torch.equal(got.view(torch.uint8), ref.contiguous().reshape(-1).view(torch.uint8)):
            errors.append('{} {} phase {}: {} differs from the wrapper call'.format(tag, what, phase, name))


@pytest.mark.parametrize('normalise', [True, False], ids=['normalised', 'raw'])
def test_record_collate_stays_inside_its_buffers(normalise):
    L = _lib.lib()
    errors, calls = [], 0
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for B, dim in SIZES:
        tag = 'B={} dim={}'.format(B, dim)
        recs, mn, mx = synthetic_physionet.make_records(30, dim, n_quant=24, n_obs_range=(1, 7),
                                                        p_feature=0.3, seed=B + dim)
        kw = dict(data_min=mn, data_max=mx) if normalise else {}
        ds = records.RecordDataset.from_records(recs, drop_unobserved=normalise, device='cuda', **kw)
        idx = torch.as_tensor(np.random.RandomState(B).randint(0, 30, size=B).astype(np.int32)).cuda()
        ref = ds.collate(idx, 'test')
        N, R, G, D = ds.n_records, ds.n_rows, ds.n_grid, dim
        n_obs, n_val = int(ref['time_ptr'][-1]), len(ref['times_val'])
        present_g = np.concatenate([ref['times'], ref['times_val']])
        g_hi = int(np.searchsorted(ds.grid, ref['times_val'][0])) if n_val else G
        need = ctypes.c_size_t(0)
        _lib.check(L.njode_records_bytes(G, B, ctypes.byref(need)))
        for phase in (0, 1):
            A = Arena('cuda', phase)
            A.add('row_ptr', 4 * (N + 1), 'index', modulo=3).add('row_g', 4 * R, 'index', modulo=min(G, 3))
            A.add('vals', 4 * R * D, 'nan32').add('mask', R * D, 'index', modulo=2)
            A.add('att_min', 4 * D if normalise else 0, 'nan32').add('att_max', 4 * D if normalise else 0, 'nan32')
            A.add('idx', 4 * B, 'index', modulo=min(N, 3))
            A.add('present', 4 * G).add('count', 4 * G).add('ws', need.value)
            A.add('X', 4 * n_obs * D).add('M', 4 * n_obs * D).add('obs_idx', 4 * n_obs).add('n_obs_ot', 4 * B)
            A.add('vals_val', 4 * B * n_val * D).add('mask_val', 4 * B * n_val * D).build()
            for k in ('row_ptr', 'row_g', 'vals', 'mask'):
                A.put(k, ds._dev[k])
            if normalise:
                A.put('att_min', ds._dev['att_min']), A.put('att_max', ds._dev['att_max'])
            A.put('idx', idx)
            store = _lib.NjodeRecordStore(N, R, D, G, int(ds.drop_unobserved), 0, A.ptr('row_ptr'), A.ptr('row_g'),
                                          A.ptr('vals'), A.ptr('mask'),
                                          A.ptr('att_min') if normalise else None,
                                          A.ptr('att_max') if normalise else None)
            ws = ctypes.c_void_p(A.ptr('ws'))
            rc = L.njode_records_count(ctypes.byref(store), _vp(A, 'idx'), B, _vp(A, 'present'), _vp(A, 'count'),
                                       ws, need.value, st)
            _check(errors, tag, 'count', phase, rc, A, {})
            present = A.view('present', torch.int32).cpu().numpy()
            if not np.array_equal(ds.grid[np.nonzero(present)[0]], present_g):
                errors.append('{} count phase {}: present differs from the wrapper call'.format(tag, phase))
                continue
            rc = L.njode_records_fill(ctypes.byref(store), _vp(A, 'idx'), B, _vp(A, 'count'), 0, g_hi, n_obs,
                                      _vp(A, 'X'), _vp(A, 'M'), _vp(A, 'obs_idx'), _vp(A, 'n_obs_ot'), ws,
                                      need.value, st)
            _check(errors, tag, 'fill', phase, rc, A, {k: ref[k] for k in ('X', 'M', 'obs_idx', 'n_obs_ot')})
            rc = L.njode_records_heldout(ctypes.byref(store), _vp(A, 'idx'), B, _vp(A, 'present'), g_hi, n_val,
                                         _vp(A, 'vals_val'), _vp(A, 'mask_val'), ws, need.value, st)
            _check(errors, tag, 'heldout', phase, rc, A, {k: ref[k] for k in ('vals_val', 'mask_val')})
            calls += 3
    print('record collate: {} guarded calls, 16 buffers each'.format(calls))
    assert not errors, '\n'.join(errors)
