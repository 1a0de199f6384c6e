"""Host route of the climate validation layout (njode_amd/records.py: ``val_cut``, ``eligible``,
``collate_val_host``) against the reference's own ``ODE_Dataset(validation=True)`` +
``custom_collate_fn``, whose outputs on stored records are in
tests/golden/g19_records_climate_val.npz (tests/golden/make_golden_records_val.py).  No GPU and no
library needed."""
import os

import numpy as np
import pytest
import torch

from golden_util import Golden
from njode_amd import climate_eval, records
from oracle import njode_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BATCHES = [(3, 'a'), (3, 'b'), (1, 'a')]


@pytest.fixture(scope='module')
def fixture():
    z = np.load(os.path.join(GOLDEN, 'g19_records_climate_val.npz'), allow_pickle=False)
    recs = [(z['rec{}/tt'.format(n)], z['rec{}/vals'.format(n)], z['rec{}/mask'.format(n)])
            for n in range(int(z['n_records']))]
    return z, recs, records.RecordDataset.from_records(recs, time_div=None, drop_unobserved=False,
                                                       device=None)


@pytest.mark.parametrize('max_val,batch', BATCHES)
def test_collate_equals_the_reference(fixture, max_val, batch):
    z, _, ds = fixture
    q = 'm{}/{}/'.format(max_val, batch)
    idx = z[q + 'records']
    got = ds.collate_val_host(idx, int(z['T_val']), max_val)
    assert z[q + 'times'].dtype == np.float32 and got['times'].dtype == np.float64
    assert np.array_equal(got['times'], z[q + 'times'].astype(np.float64))
    assert got['times_val'].dtype == np.float64
    assert np.array_equal(got['times_val'], z[q + 'times_val'].astype(np.float64))
    for k in ('time_ptr', 'index_val'):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], z[q + k]), k
    assert got['obs_idx'].dtype == torch.int64
    assert np.array_equal(got['obs_idx'].numpy(), z[q + 'obs_idx'])
    for k in ('X', 'M', 'X_val', 'M_val'):
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == z[q + k].shape
        assert np.array_equal(got[k].numpy(), z[q + k]), k
    B = len(idx)
    assert got['batch_size'] == B and got['pat_idx'] == idx.tolist()
    assert torch.equal(got['start_X'], torch.zeros(B, ds.dim))
    assert np.array_equal(got['n_obs_ot'].numpy(), np.bincount(z[q + 'obs_idx'], minlength=B))
    # the cut and the cap, as the reference has them
    assert got['times'].max() <= 150 < got['times_val'].min()
    assert np.bincount(got['index_val'], minlength=B).max() == max_val


def test_fixture_covers_the_edges(fixture):
    """What the comparison above is worth: a row at exactly ``T_val`` (observed), records with
    one and with two rows after the cut, tied observed times, held-out rows ordered by record and
    not by batch position, both refusals of the eligibility rule."""
    z, recs, ds = fixture
    after = [int((tt > 150).sum()) for tt, _, _ in recs]
    before = [int((tt <= 150).sum()) for tt, _, _ in recs]
    assert after[2] == 0 and before[5] == 0 and after[9] == 1 and after[11] == 2
    assert np.float32(150.0) in recs[7][0]
    b = ds.collate_val_host(z['m3/b/records'], 150, 3)
    assert {7, 9, 11} <= set(b['pat_idx']) and 150.0 in b['times']
    a = ds.collate_val_host(z['m3/a/records'], 150, 3)
    assert (np.diff(a['time_ptr']) >= 2).sum() >= 3
    for d in (a, b):
        assert np.any(np.diff(d['index_val']) < 0)                 # not by batch position ...
        rec = np.asarray(d['pat_idx'])[d['index_val']]
        assert np.array_equal(np.lexsort((d['times_val'], rec)), np.arange(len(rec)))   # ... by record
        assert sorted(np.bincount(d['index_val']).tolist())[0] < 3


def test_eligible_equals_the_reference(fixture):
    z, _, ds = fixture
    for m in (3, 1):
        kept = ds.eligible(z['idx'], int(z['T_val']))
        assert kept.dtype == np.int64 and np.array_equal(kept, z['m{}/kept'.format(m)])
    assert 2 not in kept and 5 not in kept and 13 not in kept
    # the order of idx is kept; a record outside the store is refused
    assert np.array_equal(ds.eligible(z['idx'][::-1], 150), z['m3/kept'][::-1])
    with pytest.raises(ValueError):
        ds.eligible([0, 14], 150)


def _small():
    tt = [np.array(t, dtype=np.float32) for t in ([1.0, 2.0, 3.5], [2.0, 3.0, 4.0, 5.0], [0.5, 6.0])]
    recs = [(t, np.arange(len(t) * 2, dtype=np.float32).reshape(-1, 2) + 10 * n,
             np.ones((len(t), 2), dtype=np.float32)) for n, t in enumerate(tt)]
    return records.RecordDataset.from_records(recs, time_div=None, drop_unobserved=False,
                                              device=None)


def test_val_cut():
    ds = _small()                                  # grid 0.5 1 2 3 3.5 4 5 6
    assert ds.grid.tolist() == [0.5, 1.0, 2.0, 3.0, 3.5, 4.0, 5.0, 6.0]
    assert ds.val_cut(3.0) == 4                    # on a grid point: that point is observed
    assert ds.val_cut(3.2) == 4                    # between two
    assert ds.val_cut(0.25) == 0 and ds.val_cut(-1) == 0
    assert ds.val_cut(6.0) == 8 and ds.val_cut(1e9) == 8
    # the comparison is made in fp32: a T_val that rounds onto a grid point observes it
    t = np.array([0.1, 0.2], dtype=np.float32)
    one = np.ones((2, 1), dtype=np.float32)
    d2 = records.RecordDataset.from_records([(t, one, one)], time_div=None, drop_unobserved=False,
                                            device=None)
    assert float(d2.grid[0]) > 0.1 and d2.val_cut(0.1) == 1
    # below the first grid point: nothing observed, everything (up to the cap) held out
    b = ds.collate_val_host([2, 0, 1], 0.25, 3)
    assert len(b['times']) == 0 and b['time_ptr'].tolist() == [0]
    assert tuple(b['X'].shape) == tuple(b['M'].shape) == (0, 2) and len(b['obs_idx']) == 0
    assert b['n_obs_ot'].tolist() == [0, 0, 0]
    assert b['index_val'].tolist() == [1, 1, 1, 2, 2, 2, 0, 0]
    assert b['times_val'].tolist() == [1.0, 2.0, 3.5, 2.0, 3.0, 4.0, 0.5, 6.0]
    assert b['X_val'][:, 0].tolist() == [0.0, 2.0, 4.0, 10.0, 12.0, 14.0, 20.0, 22.0]
    # above the last: everything observed, nothing held out
    b = ds.collate_val_host([2, 0, 1], 7, 3)
    full = ds.collate_host([2, 0, 1], 'train')
    for k in ('X', 'M', 'obs_idx', 'n_obs_ot'):
        assert torch.equal(b[k], full[k])
    assert np.array_equal(b['times'], full['times']) and np.array_equal(b['time_ptr'], full['time_ptr'])
    assert tuple(b['X_val'].shape) == tuple(b['M_val'].shape) == (0, 2)
    assert len(b['times_val']) == 0 and len(b['index_val']) == 0
    assert b['times_val'].dtype == np.float64 and b['index_val'].dtype == np.int64
    # in between, and the cap
    b = ds.collate_val_host([1, 0], 2.0, 1)
    assert b['times'].tolist() == [1.0, 2.0] and b['obs_idx'].tolist() == [1, 0, 1]
    assert b['times_val'].tolist() == [3.5, 3.0] and b['index_val'].tolist() == [1, 0]
    assert ds.eligible([0, 1, 2], 5.0).tolist() == [2]
    assert ds.eligible([2, 1, 0], 0.7).tolist() == [2] and ds.eligible([0, 1], 9).tolist() == []


def test_normalised_store_normalises_the_held_out_values():
    tt = np.array([1.0, 2.0, 3.0], dtype=np.float32)
    v = np.array([[2.0, 6.0], [4.0, 8.0], [6.0, 1.0]], dtype=np.float32)
    m = np.array([[1, 1], [1, 0], [0, 1]], dtype=np.float32)
    ds = records.RecordDataset.from_records([(tt, v, m)], np.array([1.0, 2.0]), np.array([2.0, 0.0]),
                                            time_div=None, drop_unobserved=False, device=None)
    b = ds.collate_val_host([0], 1.5, 3)
    assert b['X'].tolist() == [[0.5, 4.0]]
    assert b['X_val'].tolist() == [[1.5, 0.0], [0.0, -1.0]] and b['M_val'].tolist() == [[1, 0], [0, 1]]


class _OracleModel:
    def __init__(self, g):
        self.o = njode_oracle.make_oracle(g.cfg)
        self.params = g.state_dict()

    def eval(self):
        self.o.training = False

    def __call__(self, times, time_ptr, X, obs_idx, delta_t, T, start_X, n_obs_ot, **kw):
        return self.o.forward(self.params, times, time_ptr, X, obs_idx, delta_t, T, start_X,
                              n_obs_ot, **kw)


def test_evaluate_model_takes_the_host_batch(fixture):
    """The dict goes into the host protocol as it stands (the climate model of g8_climate_eval on the
    float64 oracle, a coarse step); the score is the one written out by hand."""
    z, _, ds = fixture
    g = Golden('g8_climate_eval')
    b = ds.collate_val_host(z['m3/b/records'], 150, 3)
    model = _OracleModel(g)
    loss_val, mse_val = climate_eval.evaluate_model(model, [b], 'cpu', 0.5, 200)
    assert np.isfinite(loss_val) and np.isfinite(mse_val) and mse_val > 0
    with torch.no_grad():
        _, loss, path_t, _, path_y = model(
            b['times'], b['time_ptr'], b['X'], b['obs_idx'], 0.5, 200, b['start_X'], b['n_obs_ot'],
            until_T=True, return_path=True, get_loss=True, M=b['M'])
    t_vec = np.around(path_t, 1).astype(np.float32)
    sq = n = 0.0
    for j, (t, i) in enumerate(zip(b['times_val'], b['index_val'])):
        k = np.nonzero(t_vec == t_vec[np.abs(t_vec.astype(np.float64) - t).argmin()])[0][0]
        sq += float((((b['X_val'][j].numpy() - path_y[k, i].numpy()) ** 2) * b['M_val'][j].numpy()).sum())
        n += float(b['M_val'][j].sum())
    assert loss_val == pytest.approx(float(loss)) and mse_val == pytest.approx(sq / n, rel=1e-6)


def test_refusals(fixture):
    _, recs, ds = fixture
    for bad in ([0, 3, 0], [14], [-1], [0.5], []):                         # twice, outside, empty
        with pytest.raises(ValueError):
            ds.collate_val_host(bad)
    for max_val in (0, -1, 1.5):
        with pytest.raises(ValueError):
            ds.collate_val_host([0, 1], 150, max_val)
    for T_val in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            ds.collate_val_host([0, 1], T_val)
        with pytest.raises(ValueError):
            ds.val_cut(T_val)
    dropping = records.RecordDataset.from_records(recs, time_div=None, drop_unobserved=True,
                                                  device=None)
    with pytest.raises(ValueError, match='drop_unobserved'):
        dropping.collate_val_host([0, 1])
    # the layout has methods of its own: the old ones still refuse it
    assert records.LAYOUTS == ('train', 'test')
    with pytest.raises(ValueError):
        ds.collate_host([0], layout='validation')
    # a host-only store has no device route
    for call in (lambda: ds.collate_val([0]), lambda: ds.prepare_val_batches([[0]])):
        with pytest.raises(RuntimeError):
            call()
