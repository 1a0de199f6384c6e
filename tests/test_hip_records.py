"""GPU collate of record datasets (include/njode_records.h, njode_amd/records.py) against the host
route ``RecordDataset.collate_host`` -- which tests/test_records_host.py holds to the reference's
own collates -- bit for bit on every field, at the sizes where a 256-thread ballot scan can go
wrong, and the C entry points' refusals."""
import ctypes

import numpy as np
import pytest
import torch

from njode_amd import _lib, records, synthetic_physionet

pytestmark = pytest.mark.gpu

FIELDS = ('X', 'M', 'obs_idx', 'n_obs_ot', 'start_X')


def _dataset(dim, normalise, drop, seed=0, n_records=40):
    """40 records on a 30-step grid plus a record of ONE row; record 0 starts at t = 0, record 1
    has no observed feature at all, about one row in eight is unobserved (empty slices)."""
    recs, mn, mx = synthetic_physionet.make_records(n_records, dim, n_quant=30, n_obs_range=(1, 8),
                                                    p_feature=0.3, seed=seed)
    recs.append((np.array([7.2], dtype=np.float32), np.full((1, dim), 3.5, dtype=np.float32),
                 np.ones((1, dim), dtype=np.float32)))
    mx = mx.copy()
    mx[0] = 0.0                                   # an att_max of 0 is taken as 1
    kw = dict(data_min=mn, data_max=mx) if normalise else {}
    return records.RecordDataset.from_records(recs, drop_unobserved=drop, device='cuda', **kw)


def _batch_idx(n_records, B, seed):
    """B records in batch order: records 0 (t = 0), 1 (nothing observed) and the last (one row)
    as far as they fit, the rest drawn with repetition."""
    idx = np.random.RandomState(seed).randint(0, n_records, size=B)
    for pos, rec in zip((0, B // 2, B - 1), (1, 0, n_records - 1)):
        if B >= 3:
            idx[pos] = rec
    if B >= 3:
        idx[1] = idx[2]                            # a record twice, side by side
    return idx


def assert_same(dev, host, layout):
    assert np.array_equal(dev['times'], host['times']) and dev['times'].dtype == np.float64
    assert np.array_equal(dev['time_ptr'], host['time_ptr']) and dev['time_ptr'].dtype == np.int64
    assert dev['batch_size'] == host['batch_size']
    for k in FIELDS:
        assert dev[k].is_cuda, k
        want = host[k]
        if k in ('obs_idx', 'n_obs_ot'):
            assert dev[k].dtype == torch.int32
            want = want.to(torch.int32)
        assert dev[k].shape == want.shape, k
        assert torch.equal(dev[k].cpu(), want), k
    if layout == 'test':
        assert np.array_equal(dev['times_val'], host['times_val'])
        for k in ('vals_val', 'mask_val'):
            assert dev[k].is_cuda and dev[k].dtype == torch.float32 and dev[k].is_contiguous()
            assert tuple(dev[k].shape) == host[k].shape, k
            assert np.array_equal(dev[k].cpu().numpy(), host[k]), k
    else:
        assert 'vals_val' not in dev


@pytest.mark.parametrize('dim', [1, 2, 41])
@pytest.mark.parametrize('B', [1, 3, 64, 65, 257])
def test_device_collate_equals_host_collate(B, dim):
    """Both layouts, with and without normalisation, drop_unobserved on and off; through
    ``collate`` and through ``prepare_batches`` + ``fill_batch``."""
    for normalise in (True, False):
        for drop in (True, False):
            ds = _dataset(dim, normalise, drop)
            idx = _batch_idx(ds.n_records, B, seed=B + dim)
            other = _batch_idx(ds.n_records, max(B - 1, 1), seed=B)
            for layout in ('train', 'test'):
                host = ds.collate_host(idx, layout)
                assert_same(ds.collate(idx, layout), host, layout)
                assert_same(ds.collate(torch.as_tensor(idx).cuda(), layout), host, layout)
                # a whole "epoch" of two batches of different sizes through one workspace
                preps = ds.prepare_batches([idx, other], layout)
                assert_same(ds.fill_batch(preps[1]), ds.collate_host(other, layout), layout)
                assert_same(ds.fill_batch(preps[0]), host, layout)
                if B >= 3 and drop:
                    assert int(host['n_obs_ot'].min()) == 0
                if B == 3 and drop:       # union times without rows
                    assert np.any(np.diff(host['time_ptr']) == 0) or layout == 'test'


def test_edges_are_in_the_cases():
    """What the parametrised comparison covers: a first time of 0, a record of one row, a record
    without any kept row, normalisation that is visible, an ``att_max`` of 0."""
    ds = _dataset(2, True, True)
    idx = _batch_idx(ds.n_records, 65, seed=67)
    host = ds.collate_host(idx, 'train')
    assert host['times'][0] == 0.0
    assert np.diff(ds.row_ptr)[-1] == 1 and idx[-1] == ds.n_records - 1
    assert int(host['n_obs_ot'][0]) == 0 and ds.att_max[0] == 0
    raw = _dataset(2, False, True).collate_host(idx, 'train')
    assert not torch.equal(raw['X'], host['X']) and torch.equal(raw['M'], host['M'])
    assert len(set(idx.tolist())) < len(idx)


def test_permuted_batch_and_both_parities_of_the_union():
    ds = _dataset(3, True, True, seed=4)
    idx = _batch_idx(ds.n_records, 65, seed=1)
    perm = np.random.RandomState(2).permutation(len(idx))
    a, b = ds.collate(idx, 'train'), ds.collate(idx[perm], 'train')
    assert np.array_equal(a['times'], b['times']) and np.array_equal(a['time_ptr'], b['time_ptr'])
    assert torch.equal(a['n_obs_ot'].cpu()[perm], b['n_obs_ot'].cpu())
    assert_same(b, ds.collate_host(idx[perm], 'train'), 'train')
    # rows of a slice: the same set, ordered by the new batch positions
    inv = np.argsort(perm)
    tp, oa, ob = a['time_ptr'], a['obs_idx'].cpu().numpy(), b['obs_idx'].cpu().numpy()
    Xa, Xb = a['X'].cpu().numpy(), b['X'].cpu().numpy()
    for i in range(len(tp) - 1):
        sl = slice(tp[i], tp[i + 1])
        order = np.argsort(inv[oa[sl]], kind='stable')
        assert np.array_equal(inv[oa[sl]][order], ob[sl])
        assert np.array_equal(Xa[sl][order], Xb[sl])
    # an odd and an even number of union times in test layout
    parities = {}
    for B in range(2, 12):
        ix = np.arange(B)
        n_union = len(ds.collate_host(ix, 'train')['times'])
        if n_union % 2 not in parities:
            parities[n_union % 2] = ix
    assert set(parities) == {0, 1}
    for ix in parities.values():
        host = ds.collate_host(ix, 'test')
        assert len(host['times']) == (len(host['times']) + len(host['times_val'])) // 2
        assert_same(ds.collate(ix, 'test'), host, 'test')


def test_host_indices_are_range_checked():
    ds = _dataset(2, True, True)
    for bad in ([ds.n_records], [-1], [0.5], []):
        with pytest.raises(ValueError):
            ds.collate(bad)
        with pytest.raises(ValueError):
            ds.prepare_batches([[0, 1], bad])
    with pytest.raises(ValueError):
        ds.collate([0], layout='validation')


def test_c_level_refusals():
    """NJODE_E_BADARG / NJODE_E_WORKSPACE before anything is launched: nulls, negative sizes, a
    workspace that is too small, g_lo > g_hi."""
    L = _lib.lib()
    ds = _dataset(2, True, True)
    B, G, D = 5, ds.n_grid, ds.dim
    i32, f32 = torch.int32, torch.float32
    idx = torch.arange(B, dtype=i32, device='cuda')
    need = ctypes.c_size_t(0)
    assert L.njode_records_bytes(G, B, ctypes.byref(need)) == 0 and need.value == 4 * G * B
    assert L.njode_records_bytes(G, B, None) == _lib.E_BADARG
    assert L.njode_records_bytes(0, B, ctypes.byref(need)) == _lib.E_BADARG
    assert L.njode_records_bytes(G, -1, ctypes.byref(need)) == _lib.E_BADARG
    ws = torch.empty(4 * G * B, dtype=torch.uint8, device='cuda')
    present, count = (torch.zeros(G, dtype=i32, device='cuda') for _ in range(2))
    n_obs = 4
    X, M = (torch.zeros((n_obs, D), dtype=f32, device='cuda') for _ in range(2))
    obs_idx = torch.zeros(n_obs, dtype=i32, device='cuda')
    n_obs_ot = torch.full((B,), -7, dtype=i32, device='cuda')
    vv, mv = (torch.zeros((B, 2, D), dtype=f32, device='cuda') for _ in range(2))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    null = ctypes.c_void_p(0)

    def store(**kw):
        s = _lib.NjodeRecordStore()
        ctypes.memmove(ctypes.byref(s), ctypes.byref(ds._store), ctypes.sizeof(s))
        for k, v in kw.items():
            setattr(s, k, v)
        return ctypes.byref(s)

    def count_call(s=None, idx_=p(idx), B_=B, pr=p(present), ct=p(count), ws_=p(ws), nb=ws.numel()):
        return L.njode_records_count(store() if s is None else s, idx_, B_, pr, ct, ws_, nb, st)

    def fill_call(s=None, idx_=p(idx), B_=B, ct=p(count), lo=0, hi=G, n=n_obs, X_=p(X), M_=p(M),
                  oi=p(obs_idx), no=p(n_obs_ot), ws_=p(ws), nb=ws.numel()):
        return L.njode_records_fill(store() if s is None else s, idx_, B_, ct, lo, hi, n, X_, M_, oi, no, ws_, nb, st)

    def held_call(s=None, idx_=p(idx), B_=B, pr=p(present), hi=1, n=2, v=p(vv), m=p(mv), ws_=p(ws),
                  nb=ws.numel()):
        return L.njode_records_heldout(store() if s is None else s, idx_, B_, pr, hi, n, v, m, ws_, nb, st)

    bad = _lib.E_BADARG
    for call in (count_call, fill_call, held_call):
        assert call(s=ctypes.POINTER(_lib.NjodeRecordStore)()) == bad
        for field in ('row_ptr', 'row_g', 'vals', 'mask', 'att_min', 'att_max'):
            assert call(s=store(**{field: None})) == bad, field
        for field in ('n_records', 'n_rows', 'dim', 'n_grid'):
            assert call(s=store(**{field: 0})) == bad and call(s=store(**{field: -3})) == bad, field
        assert call(idx_=null) == bad and call(B_=0) == bad and call(B_=-1) == bad
        assert call(ws_=null) == _lib.E_WORKSPACE
        assert call(nb=ws.numel() - 1) == _lib.E_WORKSPACE
        assert b'needed' in L.njode_last_error()
    assert count_call(pr=null) == bad and count_call(ct=null) == bad
    assert fill_call(ct=null) == bad and fill_call(no=null) == bad
    assert fill_call(X_=null) == bad and fill_call(M_=null) == bad and fill_call(oi=null) == bad
    assert fill_call(lo=3, hi=2) == bad and fill_call(lo=-1) == bad and fill_call(hi=G + 1) == bad
    assert fill_call(n=-1) == bad
    assert held_call(pr=null) == bad and held_call(v=null) == bad and held_call(m=null) == bad
    assert held_call(hi=-1) == bad and held_call(hi=G + 1) == bad and held_call(n=-1) == bad
    torch.cuda.synchronize()
    # nothing was launched by any of them
    assert int(n_obs_ot.min()) == -7 and int(present.abs().sum()) == 0 and int(count.abs().sum()) == 0
    # and the calls as they stand are accepted
    assert count_call() == 0
    assert fill_call(n=0, X_=null, M_=null, oi=null, hi=0) == 0
    torch.cuda.synchronize()
    assert int(n_obs_ot.abs().sum()) == 0
