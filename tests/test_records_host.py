"""Host route of the record collate (njode_amd/records.py: ``RecordDataset.collate_host``) against
the reference's own two collates, whose outputs on stored records are in
tests/golden/g18_records_{physionet,climate}.npz (tests/golden/make_golden_records.py), and the
store's own contracts.  No GPU and no library needed."""
import os

import numpy as np
import pytest
import torch

from njode_amd import records, synthetic_physionet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _load(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)


def _records(z, prefix=''):
    return [(z['{}rec{}/tt'.format(prefix, n)], z['{}rec{}/vals'.format(prefix, n)],
             z['{}rec{}/mask'.format(prefix, n)]) for n in range(int(z[prefix + 'n_records']))]


@pytest.fixture(scope='module')
def physionet():
    z = _load('g18_records_physionet')
    out = {}
    for dim in (5, 41):
        p = 'd{}/'.format(dim)
        out[dim] = records.RecordDataset.from_records(
            _records(z, p), z[p + 'data_min'], z[p + 'data_max'], device=None)
    return z, out


@pytest.mark.parametrize('layout', ['train', 'test'])
@pytest.mark.parametrize('batch', ['a', 'b'])
@pytest.mark.parametrize('dim', [5, 41])
def test_physionet_collate_equals_the_reference(physionet, dim, batch, layout):
    z, stores = physionet
    ds = stores[dim]
    q = 'd{}/{}/'.format(dim, batch)
    ref = {k[len(q + layout) + 1:]: z[k] for k in z.files if k.startswith(q + layout + '/')}
    got = ds.collate_host(z[q + 'idx'], layout)
    assert got['times'].dtype == np.float64 and ref['times'].dtype == np.float32
    assert np.array_equal(got['times'].astype(np.float32), ref['times'])
    assert np.array_equal(got['times'], ref['times'].astype(np.float64))
    assert got['time_ptr'].dtype == np.int64 and np.array_equal(got['time_ptr'], ref['time_ptr'])
    assert got['obs_idx'].dtype == torch.int64
    assert np.array_equal(got['obs_idx'].numpy(), ref['obs_idx'])
    for k in ('X', 'M'):
        assert got[k].dtype == torch.float32 and got[k].shape == ref[k].shape
        assert np.array_equal(got[k].numpy(), ref[k]), k
    B = len(z[q + 'idx'])
    assert got['batch_size'] == B
    assert torch.equal(got['start_X'], torch.zeros(B, dim))
    # physionet_train.py:336-340
    assert np.array_equal(got['n_obs_ot'].numpy(), np.bincount(ref['obs_idx'], minlength=B))
    if layout == 'test':
        assert np.array_equal(got['times_val'], ref['times_val'].astype(np.float64))
        for k in ('vals_val', 'mask_val'):
            assert got[k].dtype == np.float32 and got[k].shape == ref[k].shape
            assert np.array_equal(got[k], ref[k]), k
    else:
        assert 'times_val' not in got


def test_fixture_covers_the_edges(physionet):
    """What the comparison above is worth: empty slices, a first time of 0, a record without any
    collated row, a repeated record, normalisation with an ``att_max`` of 0, an odd and an even
    union in test layout."""
    z, stores = physionet
    a = stores[5].collate_host(z['d5/a/idx'], 'train')
    assert a['times'][0] == 0.0 and np.any(np.diff(a['time_ptr']) == 0)
    assert int(a['n_obs_ot'].min()) == 0
    assert len(set(z['d5/b/idx'].tolist())) < len(z['d5/b/idx'])
    assert z['d5/data_max'][1] == 0 and float(a['X'].abs().max()) > 1.5
    unions = {len(stores[41].collate_host(z['d41/{}/idx'.format(b)], 'train')['times']) % 2
              for b in 'ab'}
    assert unions == {0, 1}


@pytest.mark.parametrize('batch', ['a', 'b'])
def test_climate_collate_equals_the_reference(batch):
    z = _load('g18_records_climate')
    ds = records.RecordDataset.from_records(_records(z), time_div=None, drop_unobserved=False,
                                            device=None)
    q = batch + '/'
    got = ds.collate_host(z[q + 'idx'], 'train')
    assert np.array_equal(got['times'], z[q + 'times'].astype(np.float64))
    assert np.array_equal(got['time_ptr'], z[q + 'time_ptr'])
    tp = got['time_ptr']
    assert np.any(np.diff(tp) > 1)
    # the reference sorts by time with an unstable sort: inside a slice its order is not defined
    for i in range(len(tp) - 1):
        sl = slice(tp[i], tp[i + 1])
        order = np.argsort(z[q + 'obs_idx'][sl], kind='stable')
        assert np.array_equal(got['obs_idx'].numpy()[sl], z[q + 'obs_idx'][sl][order])
        assert np.array_equal(got['X'].numpy()[sl], z[q + 'X'][sl][order])
        assert np.array_equal(got['M'].numpy()[sl], z[q + 'M'][sl][order])


def test_batches_of_one_dataset_share_its_grid():
    recs, mn, mx = synthetic_physionet.make_records(30, 4, n_quant=25, seed=3)
    ds = records.RecordDataset.from_records(recs, mn, mx, device=None)
    assert np.all(np.diff(ds.grid) > 0)
    all_tt = np.unique(np.concatenate([r[0] for r in recs]))
    assert np.array_equal(ds.grid, (all_tt / np.float32(48.0)).astype(np.float64))
    rng = np.random.RandomState(0)
    for _ in range(4):
        idx = rng.choice(30, 7, replace=False)
        b = ds.collate_host(idx, 'test')
        for t in (b['times'], b['times_val']):
            assert np.all(np.isin(t, ds.grid))
        # the batch's own union, as the reference takes it per batch
        own = np.unique(np.concatenate([recs[n][0] for n in idx])) / np.float32(48.0)
        assert np.array_equal(np.concatenate([b['times'], b['times_val']]), own.astype(np.float64))
        assert len(b['times']) == len(own) // 2


def test_permuted_batch_permutes_the_rows():
    recs, mn, mx = synthetic_physionet.make_records(10, 3, n_quant=12, seed=5)
    ds = records.RecordDataset.from_records(recs, mn, mx, device=None)
    idx = np.arange(10)
    perm = np.random.RandomState(1).permutation(10)
    a, b = ds.collate_host(idx), ds.collate_host(idx[perm])
    assert np.array_equal(a['times'], b['times']) and np.array_equal(a['time_ptr'], b['time_ptr'])
    assert np.array_equal(a['n_obs_ot'].numpy()[perm], b['n_obs_ot'].numpy())
    key_a = set(map(tuple, np.column_stack([np.repeat(np.arange(len(a['times'])), np.diff(a['time_ptr'])),
                                            a['obs_idx'].numpy()]).tolist()))
    key_b = set(map(tuple, np.column_stack([np.repeat(np.arange(len(b['times'])), np.diff(b['time_ptr'])),
                                            perm[b['obs_idx'].numpy()]]).tolist()))
    assert key_a == key_b


def test_generators():
    recs, mn, mx = synthetic_physionet.make_records(12, 41, n_quant=40, seed=0)
    assert recs[0][0][0] == 0.0 and len(mn) == len(mx) == 41
    assert all(r[0].dtype == r[1].dtype == r[2].dtype == np.float32 for r in recs)
    assert any((r[2].sum(axis=1) == 0).any() for r in recs)
    assert float(mx.max()) > 100                       # a scale that makes normalisation visible
    assert all(np.all(np.diff(r[0]) > 0) and r[0].max() <= 48 for r in recs)
    full, _, _ = synthetic_physionet.make_records(12, 41, n_quant=40, seed=0, zero_mask_rows=False)
    assert all((r[2].sum(axis=1) > 0).all() for r in full)
    clim = synthetic_physionet.make_climate_records(8, 5, seed=1)
    for tt, vals, mask in clim:
        assert np.all(np.diff(tt) > 0) and tt.min() >= 0 and tt.max() <= 200
        assert np.array_equal(tt, np.round(tt.astype(np.float64), 1).astype(np.float32))
        assert (mask.sum(axis=1) > 0).all() and vals.shape == mask.shape == (len(tt), 5)


def test_refusals():
    tt = np.array([0.0, 1.0, 2.0], dtype=np.float32)
    v, m = np.ones((3, 2), dtype=np.float32), np.ones((3, 2), dtype=np.float32)
    make = lambda recs, **kw: records.RecordDataset.from_records(recs, device=None, **kw)  # noqa: E731
    with pytest.raises(ValueError):
        make([(tt[::-1].copy(), v, m)])                                   # unsorted
    with pytest.raises(ValueError):
        make([(np.array([0.0, 1.0, 1.0], dtype=np.float32), v, m)])       # not strictly increasing
    with pytest.raises(ValueError):
        make([(tt, v, m), (tt, np.ones((3, 3), dtype=np.float32), np.ones((3, 3), dtype=np.float32))])
    with pytest.raises(ValueError):
        make([(tt, v, m * 2)])                                            # mask outside {0, 1}
    with pytest.raises(ValueError):
        make([(tt, v, m)], data_min=np.zeros(2))                          # only one of the two
    with pytest.raises(ValueError):
        make([])
    ds = make([(tt, v, m), (tt, v, m)])
    for bad in ([2], [-1], [0, 5], [0.5], []):
        with pytest.raises(ValueError):
            ds.collate_host(bad)
    with pytest.raises(ValueError):
        ds.collate_host([0], layout='validation')
    with pytest.raises(RuntimeError):
        ds.collate([0])                                                   # host-only store
