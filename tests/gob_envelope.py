"""The run-time choices of the GRU-ODE-Bayes baseline, restated in Python from ``build_model`` /
``make_layout`` of ``njode_amd/csrc/njode_gob.hip`` and ``slab_count`` of ``njode_pathwalk.h``: the
slots of the flat parameter vector, the parameter count, the slab count of the adjoint sweep and the
workspace byte count, together with labels of the branches a call takes -- how the prep layer's
``prep_hidden * input_size`` units fall on four 64-lane chunks, which layer is wider than which (the
kernels clamp lanes by a different bound per layer), and which clamp decides the slab count.  The case
table of ``test_hip_gob_envelope`` is defined here too, so that ``test_gob_envelope_host`` can hold
every case to the library (``njode_gob_param_count``, ``njode_gob_workspace_bytes``) without a GPU."""
import numpy as np

MAX_SLABS = 1024
SLAB_BUDGET = 256 << 20
LOSS_THREADS = 256                          # tree_sum_256: one workgroup, striding over the paths
C_TRAIN, C_RETURN_PATH, C_SAVE_BWD = 0x1, 0x4, 0x8      # NJODE_C_* (held to njode_amd._lib by the host test)
FLAG_SETS = (0, C_TRAIN, C_RETURN_PATH, C_SAVE_BWD, C_TRAIN | C_SAVE_BWD)      # those of test_gob_host


def slots(cfg):
    """[(name, size)] of the flat vector in ``build_model``'s order (bias slots always present)."""
    d, H, PH, PR, CH = (cfg[k] for k in ('input_size', 'hidden_size', 'p_hidden', 'prep_hidden', 'cov_hidden'))
    out = [('p_model.0.weight', PH * H), ('p_model.0.bias', PH),
           ('p_model.3.weight', 2 * d * PH), ('p_model.3.bias', 2 * d)]
    if cfg['impute']:
        out += [('gru_c.lin_x.weight', 3 * H * 2 * d), ('gru_c.lin_x.bias', 3 * H)]
    out += [('gru_c.lin_hh.weight', H * H), ('gru_c.lin_hz.weight', H * H), ('gru_c.lin_hr.weight', H * H),
            ('gru_obs.w_prep', d * 4 * PR), ('gru_obs.bias_prep', d * PR),
            ('gru_obs.gru_d.weight_ih', 3 * H * PR * d), ('gru_obs.gru_d.weight_hh', 3 * H * H),
            ('gru_obs.gru_d.bias_ih', 3 * H), ('gru_obs.gru_d.bias_hh', 3 * H),
            ('covariates_map.0.weight', CH * d), ('covariates_map.0.bias', CH),
            ('covariates_map.3.weight', H * CH), ('covariates_map.3.bias', H)]
    return out


def param_count(cfg):
    return sum(n for _, n in slots(cfg))


def slab_count(P, B):
    """min(budget / slab bytes, 1 024, B), at least 1."""
    return max(1, min(SLAB_BUDGET // (P * 4), MAX_SLABS, B))


def _take(total, nbytes):
    """Arena::take: every array starts on a 256-byte boundary."""
    return total + ((nbytes + 255) & ~255)


def workspace_bytes(cfg, B, n_obs, n_times, K, flags):
    """make_layout(...).total"""
    no, k, t = max(n_obs, 1), max(K, 1), max(n_times, 1)
    H, P = cfg['hidden_size'], param_count(cfg)
    total = 0
    for nbytes in ((2 * K + 3 * n_times + 1) * 4, P * 4, t * B * 4, 2 * B * 8):
        total = _take(total, nbytes)
    if flags & C_SAVE_BWD:
        for nbytes in (k * B * H * 4, no * H * 4, B * H * 4, slab_count(P, B) * P * 4):
            total = _take(total, nbytes)
    return total


VOCABULARY = {
    'chunks1', 'chunks2', 'chunks3', 'chunks4', 'last_chunk_partial', 'feature_straddles_chunk',
    'PH_gt_H', 'CH_gt_H', 'D2_gt_H', 'D_gt_CH',
    'S_eq_B', 'S_max_slabs', 'S_byte_budget', 'slab_takes_3',
    'B_gt_256', 'no_rows', 'b1', 'impute', 'no_bias',
}


def labels(cfg, B, n_obs, n_times, K, bias=True):
    """The run-time branches a training call of the model ``cfg`` on such a batch takes."""
    d, H, PH, PR, CH = (cfg[k] for k in ('input_size', 'hidden_size', 'p_hidden', 'prep_hidden', 'cov_hidden'))
    NG = PR * d
    assert H <= 64 and PH <= 64 and CH <= 64 and 2 * d <= 64 and NG <= 256, 'outside the envelope'
    out = {'chunks{}'.format((NG + 63) // 64)}
    if NG % 64:
        out.add('last_chunk_partial')
    # a lane boundary 64 q inside the units that is no feature boundary: that feature's units are summed
    # in two chunks by the prep adjoint
    if any(c % PR for c in range(64, NG, 64)):
        out.add('feature_straddles_chunk')
    for word, on in (('PH_gt_H', PH > H), ('CH_gt_H', CH > H), ('D2_gt_H', 2 * d > H), ('D_gt_CH', d > CH),
                     ('impute', cfg['impute']), ('no_bias', not bias), ('B_gt_256', B > LOSS_THREADS),
                     ('no_rows', n_obs == 0), ('b1', B == 1)):
        if on:
            out.add(word)
    S = slab_count(param_count(cfg), B)
    if S == B:
        out.add('S_eq_B')
    elif S == MAX_SLABS:
        out.add('S_max_slabs')
    else:
        assert S == SLAB_BUDGET // (param_count(cfg) * 4) < B
        out.add('S_byte_budget')
    if (B + S - 1) // S >= 3:
        out.add('slab_takes_3')
    return out


# ---- the case table of test_hip_gob_envelope ----------------------------------------------------------
def _cfg(d, H, PH, PR, CH, mixing=1e-3):
    return dict(input_size=d, hidden_size=H, p_hidden=PH, prep_hidden=PR, cov_hidden=CH, mixing=mixing)


STRADDLE250 = _cfg(5, 50, 50, 50, 50)       # from_options' defaults on five climate features at hidden 50
SHARED_REAL = _cfg(2, 11, 9, 5, 6)
BUDGET = _cfg(32, 64, 64, 8, 64)            # P = 89 984 / 102 464 (impute): 745 / 654 slabs in 256 MiB
LANES = ('straddle250', 'straddle255', 'd32_small', 'ng65', 'ng150', 'straddle250_nobias')
GOLDEN = ('gob_d1_impute', 'gob_clim_plain')
ALONE = (0, 1023, 1024, 1029)               # paths of shared_real/b1030 that are also run alone


def _random(B, d, n_steps, obs, mask_p):
    def make():
        from test_hip_gob import random_batch
        return random_batch(B, d, n_steps, 0.05, obs, seed=B + n_steps, mask_p=mask_p)
    return make


def one_path(b, p):
    """Path ``p`` of the batch alone: its rows on the batch's times (slices it leaves empty stay)."""
    import torch
    keep = (b['obs_idx'] == p).numpy()
    slice_of = np.repeat(np.arange(len(b['times'])), np.diff(b['time_ptr']))
    counts = np.bincount(slice_of[keep], minlength=len(b['times']))
    kt = torch.from_numpy(keep)
    return dict(b, X=b['X'][kt], M=b['M'][kt], obs_idx=torch.zeros(int(keep.sum()), dtype=torch.long),
                start_X=b['start_X'][p:p + 1], time_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))


def _golden(name, irregular=False, doubled=False):
    def make():
        import torch

        import gob_util
        import hip_util
        b = gob_util.golden_batch(gob_util.golden(name))
        if not irregular:
            return b
        hb = dict(times=b['times'], time_ptr=b['time_ptr'], X=b['X'], M=b['M'], obs_idx=b['obs_idx'],
                  start_X=b['start_X'], n_obs_ot=torch.bincount(b['obs_idx'], minlength=b['start_X'].shape[0]))
        ib, dt = hip_util.irregular_batch(hb, b['delta_t'])
        ib = dict(ib, delta_t=dt, T=b['T'])
        return two_slices_on_one_step(ib) if doubled else ib
    return make


def two_slices_on_one_step(b):
    """``b`` with a time inserted 1e-11 delta_t after an inner observed time, carrying one row of a path
    that is also observed at that inner time: no Euler step lies between the two slices."""
    import torch
    times, ptr = np.asarray(b['times'], dtype=np.float64), np.asarray(b['time_ptr'], dtype=np.int64)
    j = next(i for i in range(len(times) // 2 + 2, len(times) - 1) if ptr[i + 1] > ptr[i])
    r, at = int(ptr[j]), int(ptr[j + 1])            # the row that is repeated, where its copy goes
    t_new = times[j] + 1e-11 * b['delta_t']
    assert times[j] < t_new < times[j + 1]
    cat = lambda t, row: torch.cat([t[:at], row[None], t[at:]])
    out = dict(b, times=np.insert(times, j + 1, t_new), time_ptr=np.insert(ptr + (np.arange(len(ptr)) > j), j + 1, at),
               X=cat(b['X'], b['X'][r] + 0.03 * b['M'][r]), M=cat(b['M'], b['M'][r]),
               obs_idx=cat(b['obs_idx'], b['obs_idx'][r]))
    if 'n_obs_ot' in out:
        out['n_obs_ot'] = torch.bincount(out['obs_idx'], minlength=b['start_X'].shape[0])
    return out


def golden_cfg(name):
    """The golden case's model without its ``impute`` (the table's cfgs carry none: the tests set it)."""
    import gob_util
    c = gob_util.golden_cfg(gob_util.golden(name))
    return {k: v for k, v in c.items() if k != 'impute'}, c['impute']


def case_table():
    """{name: (cfg without 'impute', make, bias)}; ``make()`` -> the batch (with delta_t and T),
    deterministic.  The golden cases keep their own ``impute`` (``golden_cfg``)."""
    cases = {
        # the prep layer's units on the four 64-lane chunks, and layers wider than hidden_size
        'straddle250': (STRADDLE250, _random(6, 5, 12, 4, 0.6), True),
        'straddle255': (_cfg(3, 9, 64, 85, 64), _random(5, 3, 12, 4, 0.6), True),
        'd32_small': (_cfg(32, 5, 3, 7, 2), _random(5, 32, 12, 4, 0.5), True),
        'ng65': (_cfg(5, 33, 20, 13, 20), _random(4, 5, 12, 4, 0.6), True),
        'ng150': (_cfg(3, 12, 7, 50, 5), _random(4, 3, 12, 4, 0.6), True),     # (three chunks: no other row has them)
        'straddle250_nobias': (STRADDLE250, _random(6, 5, 12, 4, 0.6), False),
        # the slab clamps
        'shared_real/b1030': (SHARED_REAL, _random(1030, 2, 10, 3, 0.6), True),
        'shared_real/b2050': (SHARED_REAL, _random(2050, 2, 10, 3, 0.6), True),
        'budget/b760': (BUDGET, _random(760, 32, 4, 1, 0.5), True),
        'shared_real/no_rows': (SHARED_REAL, _random(3, 2, 10, 0, None), True),
    }
    for p in ALONE:
        cases['shared_real/alone{}'.format(p)] = (
            SHARED_REAL, lambda p=p: one_path(cases['shared_real/b1030'][1](), p), True)
    for name in GOLDEN:
        cfg = golden_cfg(name)[0]
        cases[name] = (cfg, _golden(name), True)
        cases[name + '/irregular'] = (cfg, _golden(name, True), True)
        cases[name + '/two_slices'] = (cfg, _golden(name, True, True), True)
    return cases


def call_sizes(b):
    """(B, n_obs, n_times, K) of the call ``NNFOwithBayesianJumps.forward`` makes of this batch."""
    from njode_amd import schedule
    s = schedule.Schedule(b['times'], b['delta_t'], b['T'], True)
    return int(b['start_X'].shape[0]), int(b['time_ptr'][-1]), s.n_times, s.n_steps


def case_labels(name, impute, b=None):
    cfg, make, bias = case_table()[name]
    return labels(dict(cfg, impute=impute), *call_sizes(make() if b is None else b), bias=bias)
