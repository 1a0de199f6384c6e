"""The restatement of the float64 route's run-time choices (``tests/f64_envelope.py``) held to the library
through its pure host functions, and the case table of ``test_hip_f64_envelope`` held to the label
vocabulary: no GPU needed.  ``njode_f64_workspace_bytes`` equal to the restated byte count on every case,
with and without ``NJODE_C_SAVE_BWD``, is what pins the parameter count P and the slab count S the GPU
module's labels are computed from."""
import ctypes
import os

import pytest

import f64_envelope as fe
import gen_envelope
from njode_amd import _lib

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libnjode_hip.so not built')

T = _lib.ACT_TANH


def _why():
    return _lib.lib().njode_last_error().decode()


_SIZES = {}


def sizes_of(name):
    """(B, n_obs, n_times, K) of a case's training call and of its path call (``until_T=True``)."""
    if name not in _SIZES:
        cfg, make = fe.case_table()[name]
        b, dt, T_, until = make()
        _SIZES[name] = (fe.call_sizes(b, dt, T_, until), fe.call_sizes(b, dt, T_, True))
    return _SIZES[name]


@needs_lib
def test_supported_gives_the_restatement_s_verdict():
    """Every case of the table is admitted; refused shapes carry the reason the restatement names."""
    L = _lib.lib()
    for name, (cfg, _) in fe.case_table().items():
        why, model = fe.restate_cfg(cfg)
        d = fe.dims_of_cfg(cfg)
        assert why is None and L.njode_f64_supported(ctypes.byref(d)) == 1, (name, why, _why())
    import test_hip_generic_envelope as env
    for row in fe.REFUSED_ROWS:
        why, _ = fe.restate_cfg(env.ROWS[row][0])
        d = fe.dims_of_cfg(env.ROWS[row][0])
        assert why == fe.R_RNN and L.njode_f64_supported(ctypes.byref(d)) == 0 and why in _why(), (row, why, _why())
    one = lambda w, n=2: (n, (w,) * n, (T,) * n)
    refused = [
        ((1, 10, 1, one(50), _lib.F_RESIDUAL | _lib.F_USE_RNN), fe.R_RNN),
        ((513, 10, 513, one(50), 0), fe.R_SIZES), ((1, 1025, 1, one(50), 0), fe.R_SIZES),
        ((3, 6, 5, one(50), _lib.F_MASKED), fe.R_MASKED),
        ((3, 7, 3, one(50), _lib.F_RESIDUAL), fe.R_RESIDUAL), ((8, 4, 6, one(50), _lib.F_RESIDUAL), fe.R_RESIDUAL),
        ((1, 10, 1, one(50, 9), 0), fe.R_NHIDDEN),
        ((1, 10, 1, (one(50), one(1025), one(50)), 0), fe.R_NET), ((1, 10, 1, (one(50), (9, (8,) * 9, (T,) * 9), one(50)), 0), fe.R_NET),
        ((1, 10, 1, (2, (50, 50), (7, 7)), 0), fe.R_NET),
        # the LDS of the fp32 family is the tighter one: H = 629 without hidden layers, 229 next to width 1 024
        ((1, 629, 1, (0, (), ()), 0), gen_envelope.R_LDS), ((1, 229, 1, one(1024), 0), gen_envelope.R_LDS),
    ]
    for shape, reason in refused:
        why, model = fe.restate(*shape)
        d = gen_envelope.dims_of(*shape)
        assert why == reason and model is None, (shape, why)
        assert L.njode_f64_supported(ctypes.byref(d)) == 0, shape
        assert reason in _why(), (shape, reason, _why())
    # ... and their neighbours inside
    for shape in ((251, 10, 251, one(50), 0), (1, 628, 1, (0, (), ()), 0), (1, 228, 1, one(1024, 1), 0),
                  (8, 4, 8, one(50), _lib.F_RESIDUAL), (1, 10, 1, one(50, 8), 0), (1, 10, 1, one(1024, 8), 0)):
        why, model = fe.restate(*shape)
        d = gen_envelope.dims_of(*shape)
        assert why is None and L.njode_f64_supported(ctypes.byref(d)) == 1, (shape, why, _why())


@needs_lib
def test_workspace_bytes_match_exactly_on_every_case():
    L = _lib.lib()
    out = ctypes.c_size_t(0)
    for name, (cfg, _) in fe.case_table().items():
        why, model = fe.restate_cfg(cfg)
        d = fe.dims_of_cfg(cfg)
        train, path = sizes_of(name)
        for sizes, flags in ((train, _lib.C_GET_LOSS | _lib.C_SAVE_BWD), (train, _lib.C_GET_LOSS), (train, 0),
                             (train, _lib.C_SAVE_BWD), (path, _lib.C_RETURN_PATH), (path, _lib.C_GET_LOSS | _lib.C_RETURN_PATH)):
            assert L.njode_f64_workspace_bytes(ctypes.byref(d), *sizes, flags, ctypes.byref(out)) == 0, (name, _why())
            want = fe.workspace_bytes(model, *sizes, flags)
            assert out.value == want, (name, sizes, flags, out.value, want)
        print('{:22s} B {:5d} n_obs {:6d} n_times {:4d} K {:5d}  P {:8d} S {:5d}  {:.1f} MB'.format(
            name, *train, model['P'], fe.slab_count(model, train[0]),
            fe.workspace_bytes(model, *train, _lib.C_GET_LOSS | _lib.C_SAVE_BWD) / 1e6))


@needs_lib
def test_slab_count_at_both_clamps():
    """S through the byte count at sizes around both clamps, on a small and a large parameter vector."""
    L = _lib.lib()
    out = ctypes.c_size_t(0)
    import hip_util
    for cfg, Bs in ((hip_util.demo_cfg(), (1, 2, 2047, 2048, 2049, 2100, 4096, 20000)),
                    (fe.budget_cfg(), (1, 17, 18, 19, 20, 36, 37, 3000))):
        why, model = fe.restate_cfg(cfg)
        d = fe.dims_of_cfg(cfg)
        for B in Bs:
            assert L.njode_f64_workspace_bytes(ctypes.byref(d), B, 3 * B, 4, 5, _lib.C_SAVE_BWD, ctypes.byref(out)) == 0
            assert out.value == fe.workspace_bytes(model, B, 3 * B, 4, 5, _lib.C_SAVE_BWD), (B, out.value)
    why, model = fe.restate_cfg(fe.budget_cfg())
    assert model['P'] == 7373333 and fe.slab_count(model, 20) == 18 and fe.slab_count(model, 18) == 18
    why, model = fe.restate_cfg(hip_util.demo_cfg())
    assert model['P'] == 10071 and fe.slab_count(model, fe.BIG_B) == 2048


REQUIRED = {
    'nth_64', 'nth_128', 'nth_256', 'units_loop',
    'row_1_lane', 'row_idle_lanes', 'row_exact', 'row_strided', 'idle_row_groups',
    'depth_0', 'depth_0_all', 'depth_8', 'depth_mixed',
    'enc_case_0', 'enc_case_1_mult2+', 'enc_case_2_mult2+', 'dec_case_0', 'dec_case_1_mult2+', 'dec_case_2_mult2+',
    'masked', 'masked_enc_case_1_mult2+', 'masked_enc_case_2_mult2+', 'input_current_t', 'loss_easy', 'no_bias',
    'do_ne_d', 'S_eq_B', 'S_max_slabs', 'S_budget', 'S_uneven', 'loss_tree_strided', 'rows_clear_strided', 'no_rows', 'b1',
}


def test_case_table_takes_every_label():
    """The rows of ``test_hip_f64_envelope`` together take every label of the vocabulary; prints each
    row's labels."""
    assert REQUIRED == fe.VOCABULARY
    seen = {}
    for name, (cfg, _) in fe.case_table().items():
        lab = fe.case_labels(cfg, sizes_of(name)[0])
        print('{:22s} {}'.format(name, ' '.join(sorted(lab))))
        for k in lab:
            seen.setdefault(k, []).append(name)
    assert REQUIRED <= set(seen), REQUIRED - set(seen)
    # the slab rows are what the issue says they are
    for name, must in (('slab/demo_b2100', {'S_max_slabs', 'S_uneven', 'loss_tree_strided'}),
                       ('slab/masked_b2100', {'S_max_slabs', 'S_uneven', 'loss_tree_strided', 'masked'}),
                       ('slab/budget', {'S_budget', 'S_uneven', 'units_loop', 'depth_8', 'row_strided'}),
                       ('slab/rows_clear', {'rows_clear_strided', 'S_max_slabs'}), ('no_rows', {'no_rows', 'S_eq_B'}),
                       ('env/w128/b1', {'b1'}), ('env/deep_mixed', {'no_bias', 'depth_0', 'depth_8', 'depth_mixed',
                                                                     'input_current_t', 'loss_easy', 'row_1_lane'}),
                       ('env/none_h628', {'depth_0_all', 'row_strided', 'units_loop'}), ('env/d3_do7', {'do_ne_d'}),
                       ('env/d17_res12', {'enc_case_1_mult2+', 'dec_case_2_mult2+'}),
                       ('env/d8_res21', {'enc_case_2_mult2+', 'dec_case_1_mult2+'}),
                       ('masked_res12', {'masked_enc_case_1_mult2+', 'dec_case_2_mult2+'}),
                       ('masked_res21', {'masked_enc_case_2_mult2+', 'dec_case_1_mult2+'}),
                       ('deep8_live', {'no_bias', 'depth_0', 'depth_8', 'depth_mixed'})):
        assert must <= fe.case_labels(fe.case_table()[name][0], sizes_of(name)[0]), (name, must)
    # every slab clamp is met by a row whose slabs take more than one path
    assert all(sizes_of(n)[0][0] > fe.slab_count(fe.restate_cfg(fe.case_table()[n][0])[1], sizes_of(n)[0][0])
               for n in seen['S_max_slabs'] + seen['S_budget'])


def test_layer_tables_of_the_lane_layouts():
    """The (n_in, n_out, lanes, rows per pass) the restatement derives, at each layout of the slab update."""
    one = lambda w, n=1: (n, (w,) * n, (T,) * n)
    lay = lambda shape: fe.layer_table(fe.restate(*shape)[1])
    # nth 64: a row of 1 input -> 1 lane, 64 rows; 13 inputs (D + H + 2) -> 16 lanes, 4 rows
    assert lay((1, 10, 1, one(1), 0)) == [(13, 1, 16, 4), (1, 10, 1, 64), (1, 1, 1, 64), (1, 10, 1, 64),
                                          (10, 1, 16, 4), (1, 1, 1, 64)]
    # nth 256 (widest 300): rows longer than the workgroup -> 256 lanes striding, one row per pass
    assert lay((1, 10, 1, one(300, 2), 0))[1] == (300, 300, 256, 1)
    # nth 128: 65 inputs -> 128 lanes; 96 -> 128 lanes; 64 -> 64 lanes, 2 rows
    t = lay((1, 10, 1, (one(96), (2, (65, 64), (T, T)), one(96)), 0))
    assert (65, 64, 128, 1) in t and (64, 10, 64, 2) in t and (10, 96, 16, 8) in t
    assert fe.restate(1, 10, 1, one(64), 0)[1]['nth'] == 64 and fe.restate(1, 10, 1, one(65), 0)[1]['nth'] == 128
    assert fe.restate(1, 10, 1, one(128), 0)[1]['nth'] == 128 and fe.restate(1, 10, 1, one(129), 0)[1]['nth'] == 256
    assert fe.restate(50, 12, 50, one(8), 0)[1]['nth'] == 64 and fe.restate(52, 12, 52, one(8), 0)[1]['nth'] == 128
