"""
ctypes binding of libnjode_hip.so (C ABI: include/njode_hip.h).

There is no CPU fallback: if the shared library has not been built
(``python -m njode_amd.build`` / ``__graft_entry__.build()``) importing this
module's ``lib()`` raises, and every product entry point goes through it.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (NJODE_LIB: another build of the same library, e.g. the diagnostic build of tools/ubench)
LIB_PATH = os.environ.get('NJODE_LIB') or os.path.join(_HERE, 'libnjode_hip.so')

# ---- constants mirrored from include/njode_hip.h -----------------------------------
NJODE_OK = 0
E_UNSUPPORTED, E_BADARG, E_WORKSPACE, E_HIP = 1, 2, 3, 4
ACT_TANH, ACT_RELU = 0, 1
F_MASKED, F_INPUT_CURRENT_T, F_RESIDUAL, F_LOSS_EASY, F_USE_RNN = 0x1, 0x2, 0x4, 0x8, 0x10
C_TRAIN, C_GET_LOSS, C_RETURN_PATH, C_SAVE_BWD, C_LOSS_IN_BWD = 0x1, 0x2, 0x4, 0x8, 0x10
C_SCHED_KNOWN, C_SCHED_TAIL = 0x20, 0x40
C_PLAN_READY, C_NEED_HT = 0x80, 0x100
C_ROWS_IN_FWD = 0x400       # saving forward also runs the backward's row pass (autograd bridge)
C_GEN_LOCKSTEP = 0x200      # shape-generic kernels: unmasked loss calls stay on the lockstep plan
C_PLAN_DEFER = 0x800        # njode_plan_f32: the plan rides in front of the next forward call's ODE-forward launch

EXPORTS = ('njode_supported', 'njode_param_count', 'njode_workspace_bytes',
           'njode_plan_bytes', 'njode_plan_f32', 'njode_plan_flush', 'njode_plan_barrier_failures',
           'njode_forward_f32', 'njode_backward_f32', 'njode_backward_loss_f32',
           'njode_adam_step_f32',
           'njode_last_error', 'njode_build_info', 'njode_profile_enable',
           'njode_profile_read',
           # include/njode_producer.h
           'njode_philox4x32_10', 'njode_generate_paths', 'njode_sample_observations',
           'njode_collate_count', 'njode_collate_fill',
           'njode_cond_exp_bytes', 'njode_cond_exp_f64',
           'njode_generate_stage', 'njode_cond_exp_staged_bytes', 'njode_cond_exp_staged_f64',
           # include/njode_protocol.h
           'njode_protocol_bytes', 'njode_protocol_rows', 'njode_protocol_score_f32',
           # include/njode_records.h
           'njode_records_bytes', 'njode_records_count', 'njode_records_fill',
           'njode_records_heldout', 'njode_records_val_bytes', 'njode_records_val_count',
           'njode_records_val_fill',
           # include/njode_online.h
           'njode_online_supported', 'njode_online_reset_f32', 'njode_online_advance_f32',
           'njode_online_observe_f32', 'njode_online_predict_f32', 'njode_online_run_f32',
           'njode_online_gen_supported', 'njode_online_tables_bytes', 'njode_online_tables_f32',
           'njode_online_gen_reset_f32', 'njode_online_gen_advance_f32', 'njode_online_gen_observe_f32',
           'njode_online_gen_predict_f32', 'njode_online_gen_run_f32',
           # include/njode_f64.h
           'njode_f64_supported', 'njode_f64_workspace_bytes', 'njode_forward_f64', 'njode_backward_f64',
           # include/njode_gob.h
           'njode_gob_supported', 'njode_gob_param_count', 'njode_gob_workspace_bytes',
           'njode_gob_forward_f32', 'njode_gob_backward_f32',
           # include/njode_selftest.h
           'njode_selftest_dropout_words', 'njode_debug_plan_stamps', 'njode_debug_plan_view')
ROWS_CLOSEST, ROWS_FIRST_NEAREST = 0, 1     # NJODE_ROWS_* (include/njode_protocol.h)
SDE_MODELS = {'BlackScholes': 0, 'OrnsteinUhlenbeck': 1, 'Heston': 2}
# (the fourth model is known to the staged entry points only: njode_generate_stage,
# njode_cond_exp_staged_f64)
SDE_MODELS_STAGED = dict(SDE_MODELS, HestonWOFeller=3)
MAX_STAGES = 16     # NJODE_MAX_STAGES (include/njode_producer.h)


MAX_HIDDEN = 8      # NJODE_MAX_HIDDEN (include/njode_hip.h)


class NjodeNet(C.Structure):
    _fields_ = [('n_hidden', C.c_int32), ('width', C.c_int32 * MAX_HIDDEN),
                ('act', C.c_int32 * MAX_HIDDEN)]


class NjodeDims(C.Structure):
    _fields_ = [('input_size', C.c_int32), ('hidden_size', C.c_int32),
                ('output_size', C.c_int32), ('n_hidden', C.c_int32),
                ('width', C.c_int32), ('act', C.c_int32), ('flags', C.c_int32),
                ('per_net', C.c_int32), ('nets', NjodeNet * 3)]


class NjodeSchedule(C.Structure):
    _fields_ = [('n_steps', C.c_int32), ('n_times', C.c_int32),
                ('step_dt', C.c_void_p), ('step_t', C.c_void_p),
                ('k_jump', C.c_void_p), ('time_f32', C.c_void_p),
                ('time_ptr', C.c_void_p)]


class NjodeBatch(C.Structure):
    _fields_ = [('batch_size', C.c_int32), ('n_obs', C.c_int32),
                ('start_X', C.c_void_p), ('X', C.c_void_p), ('M', C.c_void_p),
                ('obs_idx', C.c_void_p), ('n_obs_ot', C.c_void_p),
                ('loss_batch_size', C.c_float), ('path_id_offset', C.c_int64),
                ('plan', C.c_void_p), ('grad_hT', C.c_void_p)]


class NjodeSchedule64(C.Structure):
    """include/njode_f64.h: ``step_dt`` is the float64 clock's own step."""
    _fields_ = NjodeSchedule._fields_


class NjodeBatch64(C.Structure):
    _fields_ = [('batch_size', C.c_int32), ('n_obs', C.c_int32),
                ('start_X', C.c_void_p), ('X', C.c_void_p), ('M', C.c_void_p),
                ('obs_idx', C.c_void_p), ('n_obs_ot', C.c_void_p),
                ('loss_batch_size', C.c_double)]


GOB_F_BIAS, GOB_F_IMPUTE = 0x1, 0x2      # NJODE_GOB_F_* (include/njode_gob.h)


class NjodeGobDims(C.Structure):
    _fields_ = [('input_size', C.c_int32), ('hidden_size', C.c_int32), ('p_hidden', C.c_int32),
                ('prep_hidden', C.c_int32), ('cov_hidden', C.c_int32), ('flags', C.c_int32)]


class NjodeSde(C.Structure):
    _fields_ = [('model', C.c_int32), ('n_paths', C.c_int32), ('dim', C.c_int32),
                ('n_steps', C.c_int32), ('has_sine', C.c_int32), ('reserved', C.c_int32),
                ('drift', C.c_double), ('volatility', C.c_double), ('mean', C.c_double),
                ('speed', C.c_double), ('correlation', C.c_double), ('S0', C.c_double),
                ('maturity', C.c_double), ('sine_coeff', C.c_double)]


class NjodeSdeStage(C.Structure):
    _fields_ = [('sde', NjodeSde), ('v0', C.c_double), ('return_vol', C.c_int32),
                ('first_step', C.c_int32)]


class NjodeCondExpSchedule(C.Structure):
    _fields_ = [('n_steps', C.c_int32), ('n_times', C.c_int32),
                ('step_dt', C.c_void_p), ('step_t', C.c_void_p),
                ('k_jump', C.c_void_p), ('time_ptr', C.c_void_p)]


class NjodeProtocolJob(C.Structure):
    _fields_ = [('pred', C.c_void_p), ('n_rows', C.c_int32), ('B', C.c_int32), ('dim', C.c_int32),
                ('n_query', C.c_int32), ('rows', C.c_void_p), ('vals', C.c_void_p),
                ('mask', C.c_void_p), ('X_val', C.c_void_p), ('M_val', C.c_void_p),
                ('index_val', C.c_void_p)]


class NjodeRecordStore(C.Structure):
    _fields_ = [('n_records', C.c_int32), ('n_rows', C.c_int32), ('dim', C.c_int32),
                ('n_grid', C.c_int32), ('drop_unobserved', C.c_int32), ('reserved', C.c_int32),
                ('row_ptr', C.c_void_p), ('row_g', C.c_void_p), ('vals', C.c_void_p),
                ('mask', C.c_void_p), ('att_min', C.c_void_p), ('att_max', C.c_void_p)]


class NjodeOnlineState(C.Structure):
    _fields_ = [('h', C.c_void_p), ('last_X', C.c_void_p), ('tau', C.c_void_p), ('now', C.c_void_p),
                ('n_series', C.c_int32)]


class NjodePlanView(C.Structure):
    """include/njode_selftest.h: byte offsets of a plan's arrays (-1: not part of this plan) and
    which parts the call's plan defines."""
    OFFSETS = ('sched', 't_of_row', 'first_row', 'last_row', 'item_prev', 'item_next', 'item_kbeg',
               'item_len', 'order', 't_order', 'len_hist', 'base_s', 'base16_s', 'path_sorted',
               'row_by_path', 'first_j', 'jlo', 'tile_base')
    FLAGS = ('n_tiles', 'generic', 'seg', 'sort_linked', 'links_only', 'tails', 'one_launch',
             'plan_first_stage', 'plan_blocks', 'cs_shift', 'cs_nwb', 'cs_large', 'scan_thread_per_key', 'lds_cnt',
             'tail_radix', 'split_on')
    _fields_ = ([('plan_bytes', C.c_int64)] + [(n, C.c_int64) for n in OFFSETS]
                + [(n, C.c_int32) for n in FLAGS]
                + [('split_ns', C.c_int32 * 2), ('split_nw', C.c_int32 * 2), ('split_r', C.c_float * 2)])

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n in ('plan_bytes',) + self.OFFSETS + self.FLAGS}
        d.update(split_ns=list(self.split_ns), split_nw=list(self.split_nw), split_r=list(self.split_r))
        return d


def plan_view(dims, batch_size, n_obs, n_times, n_steps, call_flags):
    """``njode_debug_plan_view`` as a dict."""
    v = NjodePlanView()
    check(lib().njode_debug_plan_view(C.byref(dims), batch_size, n_obs, n_times, n_steps, call_flags,
                                      C.byref(v)))
    return v.as_dict()


class NjodeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('libnjode_hip error {}: {}'.format(code, msg))
        self.code = code


class NjodeUnsupported(NjodeError, NotImplementedError):
    pass


_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'njode_amd: {} not found. The NJ-ODE path has no CPU fallback; build '
            'the gfx950 library first: `python -m njode_amd.build` (needs hipcc).'
            .format(LIB_PATH))
    L = C.CDLL(LIB_PATH)
    vp, i32, f32, u64, sz = C.c_void_p, C.c_int32, C.c_float, C.c_uint64, C.c_size_t
    L.njode_supported.argtypes = [C.POINTER(NjodeDims)]
    L.njode_supported.restype = C.c_int
    L.njode_param_count.argtypes = [C.POINTER(NjodeDims)]
    L.njode_param_count.restype = sz
    L.njode_workspace_bytes.argtypes = [C.POINTER(NjodeDims), i32, i32, i32, i32, i32,
                                        C.POINTER(sz)]
    L.njode_workspace_bytes.restype = C.c_int
    L.njode_plan_bytes.argtypes = [C.POINTER(NjodeDims), i32, i32, i32, i32, i32, C.POINTER(sz)]
    L.njode_plan_bytes.restype = C.c_int
    L.njode_plan_f32.argtypes = [C.POINTER(NjodeDims), C.POINTER(NjodeBatch),
                                 C.POINTER(NjodeSchedule), i32, vp, sz, vp]
    L.njode_plan_f32.restype = C.c_int
    L.njode_plan_flush.argtypes = []
    L.njode_plan_flush.restype = C.c_int
    L.njode_plan_barrier_failures.argtypes = []
    L.njode_plan_barrier_failures.restype = C.c_int
    L.njode_forward_f32.argtypes = [C.POINTER(NjodeDims), vp, C.POINTER(NjodeBatch),
                                    C.POINTER(NjodeSchedule), i32, f32, f32, u64,
                                    vp, vp, vp, vp, vp, sz, vp]
    L.njode_forward_f32.restype = C.c_int
    L.njode_backward_f32.argtypes = [C.POINTER(NjodeDims), vp, C.POINTER(NjodeBatch),
                                     C.POINTER(NjodeSchedule), i32, f32, f32, u64,
                                     vp, vp, vp, sz, vp]
    L.njode_backward_f32.restype = C.c_int
    L.njode_backward_loss_f32.argtypes = [C.POINTER(NjodeDims), vp, C.POINTER(NjodeBatch),
                                          C.POINTER(NjodeSchedule), i32, f32, f32, u64,
                                          vp, vp, vp, vp, sz, vp]
    L.njode_backward_loss_f32.restype = C.c_int
    L.njode_adam_step_f32.argtypes = [vp, vp, vp, vp, sz, f32, f32, f32, f32, f32, i32,
                                      f32, vp]
    L.njode_adam_step_f32.restype = C.c_int
    L.njode_last_error.restype = C.c_char_p
    L.njode_build_info.restype = C.c_char_p
    L.njode_profile_enable.argtypes = [C.c_int]
    L.njode_profile_enable.restype = C.c_int
    L.njode_profile_read.argtypes = [C.c_char_p, sz]
    L.njode_profile_read.restype = C.c_int
    f64 = C.c_double
    L.njode_philox4x32_10.argtypes = [i32, vp, vp, vp, vp]
    L.njode_generate_paths.argtypes = [C.POINTER(NjodeSde), u64, vp, vp, vp]
    L.njode_sample_observations.argtypes = [i32, i32, f64, u64, vp, vp, vp, vp]
    L.njode_collate_count.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp]
    L.njode_collate_fill.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp,
                                     C.POINTER(C.c_int32), i32, vp, vp, vp, vp]
    L.njode_cond_exp_bytes.argtypes = [i32, i32, i32, i32, i32, C.POINTER(sz)]
    L.njode_cond_exp_f64.argtypes = [C.POINTER(NjodeSde), C.POINTER(NjodeBatch),
                                     C.POINTER(NjodeCondExpSchedule), f64, vp, vp, vp, vp, vp, sz,
                                     vp]
    L.njode_generate_stage.argtypes = [C.POINTER(NjodeSdeStage), i32, u64, vp, vp, vp]
    L.njode_cond_exp_staged_bytes.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(sz)]
    L.njode_cond_exp_staged_f64.argtypes = [C.POINTER(NjodeSdeStage), i32, C.POINTER(NjodeBatch),
                                            C.POINTER(NjodeCondExpSchedule), f64, vp, vp, vp, vp,
                                            vp, sz, vp]
    L.njode_protocol_bytes.argtypes = [i32, i32, i32, i32, C.POINTER(sz)]
    L.njode_protocol_rows.argtypes = [vp, i32, vp, i32, i32, vp, vp]
    L.njode_protocol_score_f32.argtypes = [C.POINTER(NjodeProtocolJob), vp, i32, vp, sz, vp]
    L.njode_records_bytes.argtypes = [i32, i32, C.POINTER(sz)]
    L.njode_records_count.argtypes = [C.POINTER(NjodeRecordStore), vp, i32, vp, vp, vp, sz, vp]
    L.njode_records_fill.argtypes = [C.POINTER(NjodeRecordStore), vp, i32, vp, i32, i32, i32, vp,
                                     vp, vp, vp, vp, sz, vp]
    L.njode_records_heldout.argtypes = [C.POINTER(NjodeRecordStore), vp, i32, vp, i32, i32, vp,
                                        vp, vp, sz, vp]
    L.njode_records_val_bytes.argtypes = [i32, C.POINTER(sz)]
    L.njode_records_val_count.argtypes = [C.POINTER(NjodeRecordStore), vp, i32, i32, i32, vp, vp,
                                          sz, vp]
    L.njode_records_val_fill.argtypes = [C.POINTER(NjodeRecordStore), vp, i32, i32, i32, vp, i32,
                                         vp, vp, vp, vp, vp, sz, vp]
    for name in ('njode_philox4x32_10', 'njode_generate_paths', 'njode_sample_observations',
                 'njode_collate_count', 'njode_collate_fill',
                 'njode_cond_exp_bytes', 'njode_cond_exp_f64',
                 'njode_generate_stage', 'njode_cond_exp_staged_bytes', 'njode_cond_exp_staged_f64',
                 'njode_protocol_bytes', 'njode_protocol_rows', 'njode_protocol_score_f32',
                 'njode_records_bytes', 'njode_records_count', 'njode_records_fill',
                 'njode_records_heldout', 'njode_records_val_bytes', 'njode_records_val_count',
           'njode_records_val_fill',
           # include/njode_selftest.h
           'njode_selftest_dropout_words', 'njode_debug_plan_stamps', 'njode_debug_plan_view'):
        getattr(L, name).restype = C.c_int
    dp, sp = C.POINTER(NjodeDims), C.POINTER(NjodeOnlineState)
    L.njode_online_supported.argtypes = [dp]
    L.njode_online_reset_f32.argtypes = [dp, vp, sp, vp, i32, vp, vp]
    L.njode_online_advance_f32.argtypes = [dp, vp, sp, vp, i32, vp, f64, i32, vp, vp]
    L.njode_online_observe_f32.argtypes = [dp, vp, sp, vp, i32, vp, vp, vp, f64, i32, vp, vp, vp, vp]
    L.njode_online_predict_f32.argtypes = [dp, vp, sp, vp, i32, vp, i32, f64, i32, vp, vp, vp]
    L.njode_online_run_f32.argtypes = [dp, vp, sp, vp, i32, vp, i32, vp, vp, vp, vp, f64, i32, vp, vp, vp, vp, vp]
    # the generic family: (dims, params, tables, tables_bytes, state, ids, n, ..., series_per_tile, ..., stream)
    L.njode_online_gen_supported.argtypes = [dp]
    L.njode_online_tables_bytes.argtypes = [dp, C.POINTER(sz)]
    L.njode_online_tables_f32.argtypes = [dp, vp, vp, sz, vp]
    L.njode_online_gen_reset_f32.argtypes = [dp, vp, vp, sz, sp, vp, i32, vp, i32, vp]
    L.njode_online_gen_advance_f32.argtypes = [dp, vp, vp, sz, sp, vp, i32, vp, f64, i32, i32, vp, vp]
    L.njode_online_gen_observe_f32.argtypes = [dp, vp, vp, sz, sp, vp, i32, vp, vp, vp, f64, i32, i32, vp, vp,
                                               vp, vp]
    L.njode_online_gen_predict_f32.argtypes = [dp, vp, vp, sz, sp, vp, i32, vp, i32, f64, i32, i32, vp, vp, vp]
    L.njode_online_gen_run_f32.argtypes = [dp, vp, vp, sz, sp, vp, i32, vp, i32, vp, vp, vp, vp, f64, i32, i32, vp,
                                           vp, vp, vp, vp]
    for name in ('njode_online_supported', 'njode_online_reset_f32', 'njode_online_advance_f32',
                 'njode_online_observe_f32', 'njode_online_predict_f32', 'njode_online_gen_supported',
                 'njode_online_tables_bytes', 'njode_online_tables_f32', 'njode_online_gen_reset_f32',
                 'njode_online_gen_advance_f32', 'njode_online_gen_observe_f32', 'njode_online_gen_predict_f32',
                 'njode_online_run_f32', 'njode_online_gen_run_f32'):
        getattr(L, name).restype = C.c_int
    L.njode_selftest_dropout_words.argtypes = [u64, u64, C.c_uint32, C.c_uint32, i32, vp, vp]
    L.njode_selftest_dropout_words.restype = C.c_int
    L.njode_debug_plan_stamps.argtypes = [vp, C.c_int]
    L.njode_debug_plan_view.argtypes = [C.POINTER(NjodeDims), i32, i32, i32, i32, i32,
                                        C.POINTER(NjodePlanView)]
    # include/njode_f64.h
    d64 = (dp, vp, C.POINTER(NjodeBatch64), C.POINTER(NjodeSchedule64), i32, f64)
    L.njode_f64_supported.argtypes = [dp]
    L.njode_f64_workspace_bytes.argtypes = [dp, i32, i32, i32, i32, i32, C.POINTER(sz)]
    L.njode_forward_f64.argtypes = [*d64, vp, vp, vp, vp, vp, sz, vp]
    L.njode_backward_f64.argtypes = [*d64, vp, vp, vp, vp, sz, vp]
    for name in ('njode_f64_supported', 'njode_f64_workspace_bytes', 'njode_forward_f64',
                 'njode_backward_f64'):
        getattr(L, name).restype = C.c_int
    # include/njode_gob.h
    gp = C.POINTER(NjodeGobDims)
    g32 = (gp, vp, C.POINTER(NjodeBatch), C.POINTER(NjodeSchedule), i32, f32, f32, u64)
    L.njode_gob_supported.argtypes = [gp]
    L.njode_gob_param_count.argtypes = [gp]
    L.njode_gob_param_count.restype = sz
    L.njode_gob_workspace_bytes.argtypes = [gp, i32, i32, i32, i32, i32, C.POINTER(sz)]
    L.njode_gob_forward_f32.argtypes = [*g32, vp, vp, vp, vp, vp, sz, vp]
    L.njode_gob_backward_f32.argtypes = [*g32, vp, vp, vp, vp, vp, sz, vp]
    for name in ('njode_gob_supported', 'njode_gob_workspace_bytes', 'njode_gob_forward_f32',
                 'njode_gob_backward_f32'):
        getattr(L, name).restype = C.c_int
    _lib = L
    return L


def stream_arg(device):
    """torch's current stream on ``device`` as a ``hipStream_t`` argument."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr_arg(t):
    """A tensor's address (None: the null pointer) as a pointer argument."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def check(rc):
    if rc == NJODE_OK:
        return
    msg = lib().njode_last_error().decode('utf-8', 'replace')
    if rc == E_UNSUPPORTED:
        raise NjodeUnsupported(rc, msg)
    raise NjodeError(rc, msg)


def build_info():
    return lib().njode_build_info().decode()


def profile_enable(on=True):
    """True / 1: every kernel; 2: the ODE backward kernel only (cheap enough for a timed region)."""
    check(lib().njode_profile_enable(int(on)))


def profile_read():
    """{kernel name: (launches, total_ms)} since the last read (synchronises)."""
    buf = C.create_string_buffer(1 << 16)
    check(lib().njode_profile_read(buf, len(buf)))
    out = {}
    for line in buf.value.decode().splitlines():
        name, n, ms = line.split()
        out[name] = (int(n), float(ms))
    return out
