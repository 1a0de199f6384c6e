"""The restatement of the GRU-ODE-Bayes baseline's run-time choices (``tests/gob_envelope.py``) held to
the library through its pure host functions, and the case table of ``test_hip_gob_envelope`` held to the
label vocabulary: no GPU needed.  ``njode_gob_param_count`` and ``njode_gob_workspace_bytes`` equal to
the restated counts on every case under the five flag sets of ``test_gob_host`` are what pin the
parameter count P and the slab count S the GPU module's labels are computed from."""
import ctypes
import os

import pytest

import gob_envelope as ge
from njode_amd import _lib

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libnjode_hip.so not built in this checkout')


def _dims(cfg, bias=True):
    return _lib.NjodeGobDims(cfg['input_size'], cfg['hidden_size'], cfg['p_hidden'], cfg['prep_hidden'],
                             cfg['cov_hidden'], (_lib.GOB_F_BIAS if bias else 0)
                             | (_lib.GOB_F_IMPUTE if cfg['impute'] else 0))


_SIZES = {}


def sizes_of(name):
    if name not in _SIZES:
        _SIZES[name] = ge.call_sizes(ge.case_table()[name][1]())
    return _SIZES[name]


def imputes_of(name):
    """The ``impute`` settings the GPU module runs a case with."""
    return (ge.golden_cfg(name.split('/')[0])[1],) if name.startswith(ge.GOLDEN) else (False, True)


def test_flag_values_are_the_library_s():
    assert (ge.C_TRAIN, ge.C_RETURN_PATH, ge.C_SAVE_BWD) == (_lib.C_TRAIN, _lib.C_RETURN_PATH, _lib.C_SAVE_BWD)


def test_case_table_takes_every_label():
    """The cases of ``test_hip_gob_envelope`` together take every word of the vocabulary; prints each
    case's labels.  The cases the issue describes carry the labels it names."""
    seen = {}
    for name in ge.case_table():
        for impute in imputes_of(name):
            lab = ge.case_labels(name, impute)
            assert lab <= ge.VOCABULARY, lab - ge.VOCABULARY
            print('{:28s} impute={:d} {} {}'.format(name, impute, sizes_of(name), ' '.join(sorted(lab))))
            for k in lab:
                seen.setdefault(k, set()).add(name)
    assert ge.VOCABULARY <= set(seen), ge.VOCABULARY - set(seen)
    for name, must in (
            ('straddle250', {'chunks4', 'last_chunk_partial', 'feature_straddles_chunk', 'S_eq_B'}),
            ('straddle255', {'chunks4', 'last_chunk_partial', 'feature_straddles_chunk', 'PH_gt_H', 'CH_gt_H'}),
            ('d32_small', {'chunks4', 'last_chunk_partial', 'feature_straddles_chunk', 'D2_gt_H', 'D_gt_CH'}),
            ('ng65', {'chunks2', 'last_chunk_partial', 'feature_straddles_chunk'}),
            ('ng150', {'chunks3', 'last_chunk_partial', 'feature_straddles_chunk'}),
            ('straddle250_nobias', {'chunks4', 'feature_straddles_chunk', 'no_bias'}),
            ('shared_real/b1030', {'chunks1', 'S_max_slabs', 'B_gt_256'}),
            ('shared_real/b2050', {'S_max_slabs', 'slab_takes_3', 'B_gt_256'}),
            ('budget/b760', {'chunks4', 'S_byte_budget', 'B_gt_256'}),
            ('shared_real/no_rows', {'no_rows', 'S_eq_B'}), ('shared_real/alone1024', {'b1', 'S_eq_B'})):
        for impute in (False, True):
            lab = ge.case_labels(name, impute)
            assert must <= lab, (name, must - lab)
            assert ('impute' in lab) == impute
    assert 'slab_takes_3' not in ge.case_labels('shared_real/b1030', False)
    assert not {'last_chunk_partial', 'feature_straddles_chunk'} & ge.case_labels('budget/b760', True)
    # the shapes every GPU case had before: one chunk, or PR dividing 64, or one feature
    assert not {'feature_straddles_chunk', 'PH_gt_H', 'CH_gt_H'} & (ge.case_labels('gob_d1_impute', True)
                                                                    | ge.case_labels('gob_clim_plain', False))


def test_restated_counts_at_the_issue_s_sizes():
    plain, impute = dict(ge.BUDGET, impute=False), dict(ge.BUDGET, impute=True)
    assert ge.param_count(plain) == 89984 and ge.param_count(impute) == 102464
    assert ge.slab_count(89984, 760) == 745 and ge.slab_count(102464, 760) == 654
    assert ge.slab_count(89984, 745) == 745 and ge.slab_count(89984, 744) == 744
    for imp in (False, True):
        P = ge.param_count(dict(ge.SHARED_REAL, impute=imp))
        assert [ge.slab_count(P, B) for B in (1, 1023, 1024, 1025, 1030, 2050)] == [1, 1023, 1024, 1024, 1024, 1024]
    assert ge.param_count(dict(ge.STRADDLE250, impute=False)) == 59960     # (test_gob_host._count's formula)
    # two slices on one Euler step: the schedule gives both the same k_jump
    from njode_amd import schedule
    for name in ge.GOLDEN:
        b = ge.case_table()[name + '/two_slices'][1]()
        k = schedule.Schedule(b['times'], b['delta_t'], b['T'], True).k_jump
        assert (k[1:] == k[:-1]).sum() == 1 and b['times'][0] == 0.0 and k[0] == 0, k
        i = int((k[1:] == k[:-1]).argmax()) + 1
        lo, hi = b['time_ptr'][i - 1:i + 1], b['time_ptr'][i:i + 2]
        assert hi[1] - hi[0] == 1 and int(b['obs_idx'][hi[0]]) in b['obs_idx'][lo[0]:lo[1]].tolist()
        assert len(b['X']) == len(b['M']) == len(b['obs_idx']) == b['time_ptr'][-1]


@needs_lib
def test_param_count_and_workspace_bytes_match_on_every_case():
    L = _lib.lib()
    out = ctypes.c_size_t(0)
    for name, (cfg, _, bias) in ge.case_table().items():
        for impute in imputes_of(name):
            c = dict(cfg, impute=impute)
            d = _dims(c, bias)
            assert L.njode_gob_param_count(ctypes.byref(d)) == ge.param_count(c), name
            sizes = sizes_of(name)
            for flags in ge.FLAG_SETS:
                assert L.njode_gob_workspace_bytes(ctypes.byref(d), *sizes, flags, ctypes.byref(out)) == 0, name
                want = ge.workspace_bytes(c, *sizes, flags)
                assert out.value == want, (name, impute, sizes, flags, out.value, want)
            print('{:28s} impute={:d} B {:5d} n_obs {:5d} n_times {:3d} K {:4d}  P {:7d} S {:5d}  {:.1f} MB'.format(
                name, impute, *sizes, ge.param_count(c), ge.slab_count(ge.param_count(c), sizes[0]),
                ge.workspace_bytes(c, *sizes, ge.C_TRAIN | ge.C_SAVE_BWD) / 1e6))


@needs_lib
def test_slab_count_at_both_clamps():
    """S through the byte count at B = S - 1, S, S + 1 around both clamps, for the small and the largest
    model: B = S - 1 -> S adds a slab, B = S -> S + 1 adds none."""
    L = _lib.lib()
    out = ctypes.c_size_t(0)

    def lib_bytes(d, B, flags):
        assert L.njode_gob_workspace_bytes(ctypes.byref(d), B, 2 * B, 1, 1, flags, ctypes.byref(out)) == 0
        return out.value

    for cfg, impute in ((ge.SHARED_REAL, False), (ge.SHARED_REAL, True), (ge.BUDGET, False), (ge.BUDGET, True)):
        c = dict(cfg, impute=impute)
        d, P = _dims(c), ge.param_count(c)
        S = min(ge.SLAB_BUDGET // (4 * P), ge.MAX_SLABS)
        assert S == {1415: 1024, 1580: 1024, 89984: 745, 102464: 654}[P]
        got = {}
        for B in (1, 2, S - 1, S, S + 1, 2 * S, 2 * S + 1, 20000):
            for flags in ge.FLAG_SETS:
                got[B, flags] = lib_bytes(d, B, flags)
                assert got[B, flags] == ge.workspace_bytes(c, B, 2 * B, 1, 1, flags), (P, B, flags)
        assert [ge.slab_count(P, B) for B in (S - 1, S, S + 1)] == [S - 1, S, S]
        f = ge.C_SAVE_BWD
        # (what a path adds besides a slab is far below a slab -- four rows of H floats and 20 bytes, each
        # array rounded to 256 bytes, as is the block of slabs)
        assert got[S, f] - got[S - 1, f] >= 4 * P - 255 > 5 * 256 + 4 * 4 * c['hidden_size'] + 20
        assert 0 <= got[S + 1, f] - got[S, f] <= 5 * 256 + 4 * 4 * c['hidden_size'] + 20
