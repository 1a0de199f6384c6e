// njode_online.hip -- the online entry points of libnjode_hip.so (include/njode_online.h): argument
// checks, the verdict on a shape, and the launch of the shape's kernel (njode_cfg.hip, part 6:
// njode_online.h).  The njode_online_gen_* functions live in njode_gen.hip, beside build_model; both
// share the checks of njode_online_check.h.  Host code only; nothing is kept between calls.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/njode_online.h"
#include "njode_hostlib.h"
#include "njode_online_check.h"

using namespace njode;

#define NJ_CFG(ID) namespace njode { const OnlineOps* njode_online_ops_##ID(); }
#include "_generated_cfgs.inc"
#undef NJ_CFG
typedef const OnlineOps* (*OnlineGetter)();
static const OnlineGetter g_online[] = {
#define NJ_CFG(ID) njode::njode_online_ops_##ID,
#include "_generated_cfgs.inc"
#undef NJ_CFG
};
static const int g_nonline = sizeof(g_online) / sizeof(g_online[0]);

static const int STRUCT_FLAGS = NJODE_F_MASKED | NJODE_F_INPUT_CURRENT_T | NJODE_F_RESIDUAL | NJODE_F_USE_RNN;

// The shape's entry, or null with the reason in njode_last_error().  The verdict follows from the
// description alone; the table is only asked whether the shape was compiled.
static const OnlineOps* online_find(const NjodeDims* d) {
  if (!d) {
    fail(NJODE_E_BADARG, "online: null dims");
    return nullptr;
  }
  if (d->per_net) {
    fail(NJODE_E_UNSUPPORTED, "online: per-network descriptions run on the shape-generic kernels, which have no online form");
    return nullptr;
  }
  if (d->flags & NJODE_F_USE_RNN) {
    fail(NJODE_E_UNSUPPORTED, "online: the GRU jump (use_rnn) is not built");
    return nullptr;
  }
  if (d->n_hidden != 2) {
    fail(NJODE_E_UNSUPPORTED, "online: networks of two hidden layers only (n_hidden = %d%s)", d->n_hidden,
         d->n_hidden == 0 ? ": nn_desc = None, a single Linear per network" : "");
    return nullptr;
  }
  if (d->input_size > 64 || d->hidden_size > 64 || d->output_size > 64 || d->width > 64) {
    fail(NJODE_E_UNSUPPORTED, "online: one unit per lane, sizes <= 64 (d = %d, H = %d, d_out = %d, width = %d)",
         d->input_size, d->hidden_size, d->output_size, d->width);
    return nullptr;
  }
  if ((d->flags & NJODE_F_MASKED) && d->input_size != d->output_size) {
    fail(NJODE_E_UNSUPPORTED, "online: a masked model imputes X with the readout (d = %d, d_out = %d)", d->input_size,
         d->output_size);
    return nullptr;
  }
  for (int i = 0; i < g_nonline; ++i) {
    const OnlineOps* o = g_online[i]();
    const NjodeDims& c = o->dims;
    if (c.input_size != d->input_size || c.hidden_size != d->hidden_size || c.output_size != d->output_size ||
        c.n_hidden != d->n_hidden || c.width != d->width || c.act != d->act ||
        (c.flags & STRUCT_FLAGS) != (d->flags & STRUCT_FLAGS))
      continue;
    if (!o->ok) break;
    fail(NJODE_OK, "online: one wave per series (d = %d, H = %d, d_out = %d, width = %d)", c.input_size,
         c.hidden_size, c.output_size, c.width);
    return o;
  }
  fail(NJODE_E_UNSUPPORTED,
       "online: shape d = %d, H = %d, d_out = %d, width = %d, act = %d, flags = 0x%x is not in the build table "
       "(NJODE_EXTRA_CONFIGS)",
       d->input_size, d->hidden_size, d->output_size, d->width, d->act, d->flags & STRUCT_FLAGS);
  return nullptr;
}

extern "C" int njode_online_supported(const NjodeDims* dims) { return online_find(dims) ? 1 : 0; }

namespace {

// what every entry point checks; fills the common part of the arguments
int online_common(const NjodeDims* dims, const float* params, const NjodeOnlineState* s, const int32_t* ids, int32_t n,
                  const OnlineOps** ops, OnlineArgs* a) {
  if (!dims) return fail(NJODE_E_BADARG, "online: null dims");
  *ops = online_find(dims);
  if (!*ops) return NJODE_E_UNSUPPORTED;   // (the reason is in place)
  return online_state(params, s, ids, n, a);
}
int online_run(const OnlineOps* ops, const OnlineArgs& a, int mode, njodeStream_t stream) {
  if (a.n == 0) return NJODE_OK;
  HIP_TRY(ops->launch(a, mode, (hipStream_t)stream));
  return NJODE_OK;
}

}  // namespace

extern "C" int njode_online_reset_f32(const NjodeDims* dims, const float* params, const NjodeOnlineState* state,
                                      const int32_t* ids, int32_t n, const float* start_X, njodeStream_t stream) {
  const OnlineOps* ops;
  OnlineArgs a;
  if (int rc = online_common(dims, params, state, ids, n, &ops, &a)) return rc;
  if (!start_X) return fail(NJODE_E_BADARG, "online: null start_X");
  a.X = start_X;
  return online_run(ops, a, ONLINE_RESET, stream);
}

extern "C" int njode_online_advance_f32(const NjodeDims* dims, const float* params, const NjodeOnlineState* state,
                                        const int32_t* ids, int32_t n, const double* t, double delta_t,
                                        int32_t max_steps, int32_t* status, njodeStream_t stream) {
  const OnlineOps* ops;
  OnlineArgs a;
  if (int rc = online_common(dims, params, state, ids, n, &ops, &a)) return rc;
  if (int rc = online_clock(delta_t, max_steps, t, status, &a)) return rc;
  a.status = status;
  return online_run(ops, a, ONLINE_ADVANCE, stream);
}

extern "C" int njode_online_observe_f32(const NjodeDims* dims, const float* params, const NjodeOnlineState* state,
                                        const int32_t* ids, int32_t n, const double* t, const float* X,
                                        const float* M, double delta_t, int32_t max_steps, float* Y_before,
                                        float* Y, int32_t* status, njodeStream_t stream) {
  const OnlineOps* ops;
  OnlineArgs a;
  if (int rc = online_common(dims, params, state, ids, n, &ops, &a)) return rc;
  if (int rc = online_clock(delta_t, max_steps, t, status, &a)) return rc;
  if (!X) return fail(NJODE_E_BADARG, "online: null X");
  const bool masked = (dims->flags & NJODE_F_MASKED) != 0;
  if (masked && !M) return fail(NJODE_E_BADARG, "online: a masked model needs M");
  if (!masked && M) return fail(NJODE_E_BADARG, "online: M given to an unmasked model");
  a.X = X;
  a.M = M;
  a.Y_before = Y_before;
  a.Y = Y;
  a.status = status;
  return online_run(ops, a, ONLINE_OBSERVE, stream);
}

extern "C" int njode_online_predict_f32(const NjodeDims* dims, const float* params, const NjodeOnlineState* state,
                                        const int32_t* ids, int32_t n, const double* t_query, int32_t Q,
                                        double delta_t, int32_t max_steps, float* Y, int32_t* status,
                                        njodeStream_t stream) {
  const OnlineOps* ops;
  OnlineArgs a;
  if (int rc = online_common(dims, params, state, ids, n, &ops, &a)) return rc;
  if (int rc = online_clock(delta_t, max_steps, t_query, status, &a)) return rc;
  if (Q <= 0) return fail(NJODE_E_BADARG, "online: Q = %d", Q);
  if (!Y) return fail(NJODE_E_BADARG, "online: null Y");
  a.Q = Q;
  a.Y = Y;
  a.status = status;
  return online_run(ops, a, ONLINE_PREDICT, stream);
}

extern "C" int njode_online_run_f32(const NjodeDims* dims, const float* params, const NjodeOnlineState* state,
                                    const int32_t* ids, int32_t n, const int32_t* ev_ptr, int32_t n_events,
                                    const double* t, const float* X, const float* M, const int32_t* kind,
                                    double delta_t, int32_t max_steps, float* Y_before, float* Y, int32_t* status,
                                    int32_t* n_done, njodeStream_t stream) {
  const OnlineOps* ops;
  OnlineArgs a;
  if (int rc = online_common(dims, params, state, ids, n, &ops, &a)) return rc;
  if (int rc = online_events(delta_t, max_steps, (dims->flags & NJODE_F_MASKED) != 0, ev_ptr, n_events, t, X, M, kind,
                             Y_before, Y, status, n_done, &a))
    return rc;
  return online_run(ops, a, ONLINE_RUN, stream);
}
