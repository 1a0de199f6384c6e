"""Device route of the climate validation layout (``RecordDataset.collate_val`` /
``prepare_val_batches`` + ``fill_batch``: njode_records_count / _fill for the observed part,
njode_records_val_count / _val_fill for the held-out part) against the host route
``collate_val_host``, bit for bit on every array."""
import os

import numpy as np
import pytest
import torch

from njode_amd import records, synthetic_physionet

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _same(dev, host):
    """Every array of a device batch against the host batch (int32 against int64 values)."""
    assert np.array_equal(dev['times'], host['times']) and dev['times'].dtype == np.float64
    assert np.array_equal(dev['time_ptr'], host['time_ptr']) and dev['time_ptr'].dtype == np.int64
    for k in ('X', 'M', 'start_X', 'X_val', 'M_val'):
        assert dev[k].is_cuda and dev[k].dtype == torch.float32, k
        assert dev[k].shape == host[k].shape and torch.equal(dev[k].cpu(), host[k]), k
    for k in ('obs_idx', 'n_obs_ot', 'index_val'):
        assert dev[k].is_cuda and dev[k].dtype == torch.int32, k
        assert np.array_equal(dev[k].cpu().numpy().astype(np.int64), np.asarray(host[k])), k
    assert dev['times_val'].is_cuda and dev['times_val'].dtype == torch.float64
    assert np.array_equal(dev['times_val'].cpu().numpy(), host['times_val'])
    assert dev['batch_size'] == host['batch_size'] and list(dev['pat_idx']) == host['pat_idx']


def _store(n_records, dim, seed, normalise=False, n_obs_range=(3, 12)):
    recs = synthetic_physionet.make_climate_records(n_records, dim, n_obs_range=n_obs_range, seed=seed)
    kw = {}
    if normalise:
        rng = np.random.RandomState(seed)
        mx = rng.uniform(0.5, 3.0, dim).astype(np.float32)
        mx[0] = 0.0                                    # taken as 1
        kw = dict(data_min=rng.standard_normal(dim).astype(np.float32), data_max=mx)
    return records.RecordDataset.from_records(recs, time_div=None, drop_unobserved=False,
                                              device='cuda', **kw)


@pytest.mark.parametrize('max_val,batch', [(3, 'a'), (3, 'b'), (1, 'a')])
def test_fixture_batches(max_val, batch):
    z = np.load(os.path.join(GOLDEN, 'g19_records_climate_val.npz'), allow_pickle=False)
    recs = [(z['rec{}/tt'.format(n)], z['rec{}/vals'.format(n)], z['rec{}/mask'.format(n)])
            for n in range(int(z['n_records']))]
    ds = records.RecordDataset.from_records(recs, time_div=None, drop_unobserved=False, device='cuda')
    q = 'm{}/{}/'.format(max_val, batch)
    dev = ds.collate_val(z[q + 'records'], 150, max_val)
    _same(dev, ds.collate_val_host(z[q + 'records'], 150, max_val))
    # ... and so the reference's own arrays
    assert np.array_equal(dev['X_val'].cpu().numpy(), z[q + 'X_val'])
    assert np.array_equal(dev['index_val'].cpu().numpy(), z[q + 'index_val'])
    assert np.array_equal(dev['times_val'].cpu().numpy(), z[q + 'times_val'].astype(np.float64))
    assert np.array_equal(dev['obs_idx'].cpu().numpy(), z[q + 'obs_idx'])


@pytest.fixture(scope='module')
def stores():
    # 1100 records: a batch of 1 025 distinct ones crosses four workgroups of the ranking step
    return {dim: _store(1100, dim, seed=dim) for dim in (1, 5, 41)}


@pytest.mark.parametrize('max_val', [1, 3, 8])
@pytest.mark.parametrize('B', [1, 63, 257, 1025])
@pytest.mark.parametrize('dim', [1, 5, 41])
def test_generated_stores(stores, dim, B, max_val):
    ds = stores[dim]
    idx = np.random.RandomState(B + max_val).permutation(1100)[:B]
    dev = ds.collate_val(idx, 150, max_val)
    host = ds.collate_val_host(idx, 150, max_val)
    _same(dev, host)
    if B > 1:
        assert len(host['index_val']) > B // 2 and np.any(np.diff(host['index_val']) < 0)


@pytest.mark.parametrize('T_val,max_val', [(-1.0, 3), (0.05, 2), (200.0, 3), (1e6, 1), (100.0, 50),
                                           (199.5, 8)])
def test_cuts_at_the_edges(stores, T_val, max_val):
    """Nothing observed, nothing held out (L = 0: NULL outputs), every record with fewer rows after
    the cut than the cap."""
    ds = stores[5]
    idx = np.random.RandomState(3).permutation(1100)[:70]
    dev, host = ds.collate_val(idx, T_val, max_val), ds.collate_val_host(idx, T_val, max_val)
    _same(dev, host)
    if T_val < 0:
        assert len(dev['times']) == 0 and dev['X'].shape == (0, 5) and dev['time_ptr'].tolist() == [0]
        assert int(dev['n_obs_ot'].abs().sum()) == 0
    if T_val >= 200:
        assert dev['X_val'].shape == (0, 5) and dev['index_val'].numel() == 0
        assert dev['times_val'].shape == (0,) and dev['X'].shape[0] == int(dev['n_obs_ot'].sum())
    if max_val == 50:
        assert np.bincount(host['index_val'], minlength=70).max() < 50


def test_normalised_store():
    ds = _store(40, 5, seed=11, normalise=True)
    idx = np.random.RandomState(0).permutation(40)[:17]
    dev, host = ds.collate_val(idx, 120, 3), ds.collate_val_host(idx, 120, 3)
    _same(dev, host)
    xv, mv = host['X_val'].numpy(), host['M_val'].numpy()
    assert len(xv) > 17 and (xv[mv == 0] == 0).all() and (mv == 0).any() and (xv[mv == 1] != 0).all()


def _expected_heldout(ds, idx, g_cut, max_val):
    """The stated rule for any device index tensor: rows after the cut, at most ``max_val`` per
    position, ordered by (index value, batch position, time); an index outside the store has no
    rows."""
    rows, pos = [], []
    for b, n in enumerate(idx):
        if 0 <= n < ds.n_records:
            r = np.arange(ds.row_ptr[n], ds.row_ptr[n + 1])
            r = r[ds.row_g[r] >= g_cut][:max_val]
            rows.append(r), pos.append(np.full(len(r), b))
    rows, pos = np.concatenate(rows), np.concatenate(pos)
    order = np.lexsort((ds.row_g[rows], pos, np.asarray(idx)[pos]))
    return rows[order], pos[order]


def test_device_index_tensor_with_a_repeated_record_and_one_outside(stores):
    ds = stores[5]
    idx = np.array([7, 3, 7, 1100, 12, 3, -4, 7, 0], dtype=np.int32)
    dev = ds.collate_val(torch.from_numpy(idx).cuda(), 150, 2)
    rows, pos = _expected_heldout(ds, idx, ds.val_cut(150), 2)
    assert len(rows) > 8
    assert np.array_equal(dev['index_val'].cpu().numpy(), pos)
    assert np.array_equal(dev['X_val'].cpu().numpy(), ds.vals[rows])
    assert np.array_equal(dev['M_val'].cpu().numpy(), ds.mask[rows].astype(np.float32))
    assert np.array_equal(dev['times_val'].cpu().numpy(), ds.grid[ds.row_g[rows]])
    # the observed part: the positions outside the store have no rows, the repeated ones each theirs
    n_obs_ot = dev['n_obs_ot'].cpu().numpy()
    assert n_obs_ot[3] == 0 and n_obs_ot[6] == 0 and n_obs_ot[0] == n_obs_ot[2] == n_obs_ot[7] > 0
    assert int(dev['time_ptr'][-1]) == n_obs_ot.sum() == dev['X'].shape[0]
    assert np.array_equal(np.bincount(dev['obs_idx'].cpu().numpy(), minlength=9), n_obs_ot)


def test_many_batches_in_one_call_and_equal_bits(stores):
    ds = stores[41]
    rng = np.random.RandomState(5)
    lists = [rng.permutation(1100)[:n] for n in (9, 130, 40)]
    one = [ds.fill_batch(p) for p in ds.prepare_val_batches(lists, 140, 3)]
    again = [ds.fill_batch(p) for p in ds.prepare_val_batches(lists, 140, 3)]
    for ix, a, b in zip(lists, one, again):
        single = ds.collate_val(ix, 140, 3)
        _same(a, ds.collate_val_host(ix, 140, 3))
        for k in ('X', 'M', 'obs_idx', 'n_obs_ot', 'X_val', 'M_val', 'index_val', 'times_val'):
            assert torch.equal(a[k], single[k]) and torch.equal(a[k], b[k]), k
        assert np.array_equal(a['times'], single['times'])
        assert np.array_equal(a['time_ptr'], single['time_ptr'])


def test_refusals(stores):
    ds = stores[5]
    for call in (ds.collate_val, lambda ix, *a: ds.prepare_val_batches([ix], *a)):
        for bad in ([0, 3, 0], [1100], [-1], []):
            with pytest.raises(ValueError):
                call(bad)
        with pytest.raises(ValueError):
            call([0, 1], 150, 0)
        with pytest.raises(ValueError):
            call([0, 1], float('nan'))
    with pytest.raises(ValueError):
        ds.prepare_val_batches([])
    with pytest.raises(ValueError):
        ds.collate_val(torch.zeros(0, dtype=torch.int32, device='cuda'))
    recs = synthetic_physionet.make_climate_records(6, 5, seed=2)
    dropping = records.RecordDataset.from_records(recs, time_div=None, drop_unobserved=True,
                                                  device='cuda')
    with pytest.raises(ValueError, match='drop_unobserved'):
        dropping.collate_val([0, 1])
    # the layout has methods of its own: the old ones still refuse it
    with pytest.raises(ValueError):
        ds.collate([0], layout='validation')
    with pytest.raises(ValueError):
        ds.prepare_batches([[0]], layout='validation')
