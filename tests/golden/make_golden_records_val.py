"""
Generate tests/golden/g19_records_climate_val.npz by running the REFERENCE's climate validation
dataset and collate themselves: ``ODE_Dataset(panda_df=..., idx=..., validation=True,
val_options={'T_val': 150, 'max_val_samples': n})`` and ``custom_collate_fn``
(GRU_ODE_Bayes/data_utils_gru_ode_bayes.py).

Runs only in the build container (needs /root/reference; the reference never travels to the GPU
box).  The committed ``*.npz`` holds data only: the raw records (``make_climate_records`` of
njode_amd.synthetic_physionet, edited as below and stored so that the fixture does not depend on
the generator staying as it is), the ``idx`` given to the reference, the records it kept (it
renumbers IDs: ``kept[i]`` is the record behind its ID ``i``), each batch's records in batch order
and the reference's outputs.  Usage:  python tests/golden/make_golden_records_val.py

The 14 records are edited so that the set holds: a record that ends before ``T_val`` (2) and one
that starts after it (5), neither of which the reference keeps; a record with a row at exactly
150.0 (7); a record with exactly one (9) and one with exactly two (11) rows after the cut; three
observed times that records 0 and 1 share.  Record 13 is not in ``idx``.  Datasets: ``max_val_samples``
3 with two batches in shuffled order (six records with 0 and 1 among them; five with 7, 9 and
11), and ``max_val_samples`` 1 with one batch of six (7 and 11 among them).

The reference sorts the batch's frame by Time with pandas' default sort, which is not stable: it
leaves the rows of a tied time in batch order for some shuffles and not for others (about every
second tie comes out reversed).  Its order is unspecified there, the repository's is by batch
position, so each batch takes the first shuffle seed from 19 on for which the reference leaves
every tie in batch order.  Everything else is compared as it comes: the generator asserts that
``RecordDataset.collate_val_host`` reproduces every array exactly.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = '/root/reference'

from njode_amd import records as records_mod, synthetic_physionet  # noqa: E402

T_VAL, DIM = 150, 5


def edited_records():
    recs = synthetic_physionet.make_climate_records(n_records=14, dim=DIM, n_obs_range=(20, 40),
                                                    seed=19)
    recs = [[tt.copy(), vals.copy(), mask.copy()] for tt, vals, mask in recs]

    def keep(n, sel):
        recs[n] = [a[sel] for a in recs[n]]

    keep(2, recs[2][0] < T_VAL)                                   # ends before T_val
    keep(5, recs[5][0] > T_VAL)                                   # starts after it
    tt = recs[7][0]
    tt[np.nonzero(tt <= T_VAL)[0][-1]] = np.float32(150.0)        # a row at exactly 150.0
    for n, n_after in ((9, 1), (11, 2)):                          # one / two rows after the cut
        tt = recs[n][0]
        keep(n, np.arange(len(tt)) < (tt <= T_VAL).sum() + n_after)
    # three observed times of record 0 become times of record 1
    t0, t1 = recs[0][0], recs[1][0]
    share = [t for t in t0[t0 < 100] if t not in t1][:3]
    t1[np.nonzero(t1 < 100)[0][:3]] = share
    recs[1][0] = np.sort(t1)
    assert len(np.unique(recs[1][0])) == len(t1) and len(share) == 3
    return [tuple(r) for r in recs]


def main():
    import pandas as pd
    if not hasattr(np, 'int'):
        np.int = int            # the reference predates numpy 1.24
    sys.path.insert(0, REF)
    from GRU_ODE_Bayes.data_utils_gru_ode_bayes import ODE_Dataset, custom_collate_fn

    recs = edited_records()
    ds = records_mod.RecordDataset.from_records(recs, time_div=None, drop_unobserved=False,
                                                device=None)
    frames = []
    for n, (tt, vals, mask) in enumerate(recs):
        cols = {'ID': np.full(len(tt), n, dtype=np.float32), 'Time': tt}
        cols.update({'Value_{}'.format(j): vals[:, j] for j in range(DIM)})
        cols.update({'Mask_{}'.format(j): mask[:, j] for j in range(DIM)})
        frames.append(pd.DataFrame(cols).astype(np.float32))
    frame = pd.concat(frames, ignore_index=True)
    idx = np.arange(13)

    # the conditions the fixture is there for
    after = [int((tt > T_VAL).sum()) for tt, _, _ in recs]
    before = [int((tt <= T_VAL).sum()) for tt, _, _ in recs]
    assert after[2] == 0 and before[2] > 0 and before[5] == 0 and after[5] > 0
    assert np.float32(150.0) in recs[7][0] and after[9] == 1 and after[11] == 2
    assert max(after) > 3
    shared = np.intersect1d(recs[0][0][recs[0][0] <= T_VAL], recs[1][0][recs[1][0] <= T_VAL])
    assert len(shared) >= 3

    arrays = {'n_records': len(recs), 'idx': idx.astype(np.int64), 'T_val': T_VAL}
    for n, (tt, vals, mask) in enumerate(recs):
        arrays['rec{}/tt'.format(n)] = tt
        arrays['rec{}/vals'.format(n)] = vals
        arrays['rec{}/mask'.format(n)] = mask

    def in_batch_order(res):
        tp, oi = res['time_ptr'], res['obs_idx'].numpy()
        return all(np.all(np.diff(oi[tp[k]:tp[k + 1]]) > 0) for k in range(len(tp) - 1))

    def draw(ref, kept, size, must):
        """The first seed from 19 on whose shuffled batch of ``size`` kept records holds the
        records ``must`` and whose tied times the reference happens to leave in batch order."""
        for seed in range(19, 100000):
            ref_ids = np.random.RandomState(seed).permutation(len(kept))[:size]
            if not set(must) <= set(kept[ref_ids].tolist()):
                continue
            res = custom_collate_fn([ref[int(i)] for i in ref_ids])
            if in_batch_order(res):
                return seed, ref_ids, res
        raise AssertionError('no seed found')

    plan = {3: {'a': (6, (0, 1)), 'b': (5, (7, 9, 11))}, 1: {'a': (6, (7, 11))}}
    for max_val in (3, 1):
        ref = ODE_Dataset(panda_df=frame.copy(), idx=idx, validation=True,
                          val_options={'T_val': T_VAL, 'max_val_samples': max_val})
        kept = np.array([n for n in idx if before[n] > 0 and after[n] > 0], dtype=np.int64)
        assert len(ref) == len(kept) == 11
        # (the reference numbers the kept records in the order of the frame: increasing)
        assert np.array_equal(ds.eligible(idx, T_VAL), kept)
        p = 'm{}/'.format(max_val)
        arrays[p + 'kept'] = kept
        for name, (size, must) in plan[max_val].items():
            seed, ref_ids, res = draw(ref, kept, size, must)
            assert res['pat_idx'] == [int(i) for i in ref_ids]
            pos = kept[np.asarray(ref_ids, dtype=np.int64)]
            q = p + name + '/'
            arrays[q + 'records'] = pos
            assert res['times'].dtype == np.float32 and res['times_val'].dtype == np.float32
            arrays[q + 'times'] = np.asarray(res['times'])
            arrays[q + 'time_ptr'] = np.asarray(res['time_ptr'], dtype=np.int64)
            arrays[q + 'obs_idx'] = np.asarray(res['obs_idx'].numpy(), dtype=np.int64)
            arrays[q + 'X'] = res['X'].numpy()
            arrays[q + 'M'] = res['M'].numpy()
            arrays[q + 'X_val'] = res['X_val'].numpy()
            arrays[q + 'M_val'] = res['M_val'].numpy()
            arrays[q + 'times_val'] = np.asarray(res['times_val'])
            arrays[q + 'index_val'] = np.asarray(res['index_val'], dtype=np.int64)
            # ... and the repository's host route reproduces all of it
            got = ds.collate_val_host(pos, T_VAL, max_val)
            assert np.array_equal(got['times'], arrays[q + 'times'].astype(np.float64))
            assert np.array_equal(got['times_val'], arrays[q + 'times_val'].astype(np.float64))
            for k in ('time_ptr', 'index_val'):
                assert np.array_equal(got[k], arrays[q + k]), (q, k)
            for k in ('X', 'M', 'obs_idx', 'X_val', 'M_val'):
                assert np.array_equal(got[k].numpy(), arrays[q + k]), (q, k)
            if 0 in pos and 1 in pos:
                tied = np.diff(arrays[q + 'time_ptr']) >= 2
                assert tied.sum() >= 3, 'fewer than three observed times shared by two records'
            print('   max_val_samples={} batch {} (seed {}): {} observed rows at {} times ({} shared), '
                  '{} held-out rows'.format(max_val, name, seed, len(arrays[q + 'obs_idx']),
                                            len(arrays[q + 'times']),
                                            int((np.diff(arrays[q + 'time_ptr']) >= 2).sum()),
                                            len(arrays[q + 'index_val'])))
    np.savez_compressed(os.path.join(HERE, 'g19_records_climate_val.npz'), **arrays)


if __name__ == '__main__':
    main()
