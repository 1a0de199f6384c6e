"""
PhysioNet-shaped synthetic batches for the masked NJ-ODE path (BASELINE config 5).

There is no network access, so the real PhysioNet-2012 records cannot be
downloaded; this generator reproduces the *layout* that the reference's
``latent_ODE/physionet_LODE.py:428-544`` (``variable_time_collate_fn1``) hands
to ``NJODE.forward`` through ``physionet_train.py:326-353``:

* the batch's time axis is the sorted union of all observation times (scaled to
  [0, 1]); one row of ``X`` / ``M`` per (time, patient) whose mask row has at
  least one observed feature; rows sorted by time then patient;
* ``X`` is zero where unobserved, ``M`` is the 0/1 feature mask;
* a time can be in the union while contributing **no rows** (``time_ptr`` has
  an empty slice) and the first time can be exactly ``t = 0.0`` (a jump with no
  preceding Euler step);
* ``start_X = 0 [B, d]``, ``T = 1 + 1e-12``, ``delta_t = 0.016 / 48``
  (3 000 Euler steps), ``options['masked'] = True``.

Recipe: per path ``n_t ~ U{lo..hi}`` distinct grid
times from a seeded ``RandomState``; per observation each feature is on with
probability ``p_feature`` (at least one on); values ``U[0,1) * mask``.

``make_records`` / ``make_climate_records`` build whole DATASETS in the raw form the reference's
loaders hand to their collates -- a ragged list of ``(tt, vals, mask)`` -- for
``records.RecordDataset``; ``make_batch`` is one ready-made batch with no dataset behind it.
"""
import numpy as np
import torch

PHYSIONET_DELTA_T = 0.016 / 48
PHYSIONET_T = 1 + 1e-12
PHYSIONET_DIM = 41


def make_batch(batch_size=50, dim=PHYSIONET_DIM, n_grid=3000, n_obs_range=(30, 100),
               p_feature=0.15, seed=0, with_time_zero=True, n_empty_slices=2):
    """Build one masked batch.

    :param n_grid: number of Euler grid intervals on [0, 1]; observation times
            are multiples of ``1 / n_grid`` (use a small value for tests)
    :param with_time_zero: force path 0 to have an observation at t = 0.0
    :param n_empty_slices: number of extra union times that carry no rows
    :return: dict with times, time_ptr, X, M, obs_idx, start_X, n_obs_ot,
             delta_t, T
    """
    rng = np.random.RandomState(seed)
    lo, hi = n_obs_range
    hi = min(hi, n_grid)
    lo = min(lo, hi)
    observed = np.zeros((batch_size, n_grid + 1), dtype=bool)
    for b in range(batch_size):
        n_t = rng.randint(lo, hi + 1)
        first = 0 if (with_time_zero and b == 0) else 1
        ks = rng.choice(np.arange(first, n_grid + 1), size=n_t, replace=False)
        observed[b, ks] = True
        if with_time_zero and b == 0:
            observed[b, 0] = True
    union = observed.any(axis=0)
    # union times that no patient contributes a row to
    free = np.nonzero(~union)[0]
    free = free[free > 0]
    if n_empty_slices and len(free):
        extra = rng.choice(free, size=min(n_empty_slices, len(free)),
                           replace=False)
        union[extra] = True
    grid_idx = np.nonzero(union)[0]
    times = grid_idx.astype(np.float64) / n_grid

    rows_x, rows_m, obs_idx, time_ptr = [], [], [], [0]
    for k in grid_idx:
        who = np.nonzero(observed[:, k])[0]
        for b in who:
            m = rng.random_sample(dim) < p_feature
            if not m.any():
                m[rng.randint(dim)] = True
            rows_m.append(m.astype(np.float32))
            rows_x.append((rng.random_sample(dim) * m).astype(np.float32))
            obs_idx.append(b)
        time_ptr.append(len(obs_idx))
    obs_idx = np.asarray(obs_idx, dtype=np.int64)
    n_obs_ot = np.bincount(obs_idx, minlength=batch_size).astype(np.int64)
    return {
        'times': times,
        'time_ptr': np.asarray(time_ptr, dtype=np.int64),
        'X': torch.tensor(np.stack(rows_x)),
        'M': torch.tensor(np.stack(rows_m)),
        'obs_idx': torch.tensor(obs_idx, dtype=torch.long),
        'start_X': torch.zeros(batch_size, dim),
        'n_obs_ot': torch.tensor(n_obs_ot),
        'delta_t': 1.0 / n_grid if n_grid != 3000 else PHYSIONET_DELTA_T,
        'T': PHYSIONET_T,
    }


def make_records(n_records=12, dim=PHYSIONET_DIM, n_quant=40, n_obs_range=(3, 10), p_feature=0.15,
                 seed=0, zero_mask_rows=True):
    """A synthetic record dataset in the raw form the reference's PhysioNet loader hands to its
    collate (``physionet_LODE.py:428-544``): a list of ``(tt [T_i], vals [T_i, D], mask [T_i, D])``
    fp32 arrays, and the per-feature ``data_min`` / ``data_max`` over the observed values
    (``utils_LODE.get_data_min_max``).  Returns ``(records, data_min, data_max)``.

    * times are hours on a quantisation grid, multiples of ``48 / n_quant`` in ``[0, 48]``, per
      record ``T_i ~ U{lo..hi}`` distinct grid times; record 0 has its first row at t = 0;
    * per row each feature is on with probability ``p_feature``; with ``zero_mask_rows`` about one
      row in eight keeps an all-zero mask (the collate drops it: a union time without rows, a
      record without any collated row), every other row has at least one feature on;
    * values sit on a clinical-looking scale, ``50 j + 20 u`` for feature j, so that normalisation
      is visible; they are 0 where the mask is 0, like the parsed PhysioNet files."""
    rng = np.random.RandomState(seed)
    lo, hi = n_obs_range
    hi = min(hi, n_quant + 1)
    lo = max(min(lo, hi), 1)
    records = []
    for n in range(n_records):
        n_t = rng.randint(lo, hi + 1)
        ks = np.sort(rng.choice(np.arange(n_quant + 1), size=n_t, replace=False))
        if n == 0:
            ks[0] = 0
        mask = rng.random_sample((n_t, dim)) < p_feature
        for r in range(n_t):
            if zero_mask_rows and rng.random_sample() < 0.125:
                mask[r] = False
            elif not mask[r].any():
                mask[r, rng.randint(dim)] = True
        if zero_mask_rows and n == 1:
            mask[:] = False            # a record none of whose rows is collated
        vals = (50.0 * np.arange(dim)[None, :] + 20.0 * rng.random_sample((n_t, dim))) * mask
        # (hours in float64, rounded to fp32 once: the last grid time is 48 exactly)
        records.append(((ks * 48.0 / n_quant).astype(np.float32), vals.astype(np.float32),
                        mask.astype(np.float32)))
    all_v = np.concatenate([r[1] for r in records])
    all_m = np.concatenate([r[2] for r in records]) > 0
    data_min = np.where(all_m.any(0), np.where(all_m, all_v, np.inf).min(0), 0).astype(np.float32)
    data_max = np.where(all_m.any(0), np.where(all_m, all_v, -np.inf).max(0), 0).astype(np.float32)
    return records, data_min, data_max


def make_climate_records(n_records=12, dim=5, n_obs_range=(3, 10), p_feature=0.5, seed=0):
    """Records shaped like the climate data of ``GRU_ODE_Bayes/data_utils_gru_ode_bayes.py``
    (``ODE_Dataset`` rows ``ID, Time, Value_*, Mask_*``): few features, float times in ``[0, 200]``
    with one decimal, every row with at least one feature on, values left as they are (also where
    the mask is 0).  For ``RecordDataset.from_records(..., time_div=None, drop_unobserved=False)``
    without normalisation.  Returns the list of ``(tt, vals, mask)`` fp32 arrays."""
    rng = np.random.RandomState(seed)
    lo, hi = n_obs_range
    records = []
    for n in range(n_records):
        n_t = rng.randint(lo, hi + 1)
        ks = np.sort(rng.choice(np.arange(2001), size=n_t, replace=False))
        mask = rng.random_sample((n_t, dim)) < p_feature
        for r in range(n_t):
            if not mask[r].any():
                mask[r, rng.randint(dim)] = True
        vals = rng.standard_normal((n_t, dim))
        records.append(((ks / 10.0).astype(np.float32), vals.astype(np.float32),
                        mask.astype(np.float32)))
    return records
