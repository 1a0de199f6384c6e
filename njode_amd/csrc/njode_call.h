// njode_call.h -- the call front both kernel families share (the compiled shapes: njode_api.hip /
// njode_planner.hip, the shape-generic kernels: njode_gen.hip): the refusals every njode_*_f32
// call makes whatever runs it, the schedule upload, the dropout context and the radix sort.  What
// only one family refuses stays in that family.  Host code only.
#pragma once
#include <stdint.h>

#include "njode_device.h"
#include "njode_hostlib.h"

namespace njode {

// dims_flags: NjodeDims.flags.  Reads no array the pointers lead to.
inline int check_call(const NjodeBatch* b, const NjodeSchedule* s, int dims_flags, int call_flags,
                      float dropout_p) {
  if (!b || !s) return fail(NJODE_E_BADARG, "null argument");
  const int n_obs = b->n_obs, K = s->n_steps, nt = s->n_times;
  if (b->batch_size <= 0 || n_obs < 0 || K < 0 || nt < 0) return fail(NJODE_E_BADARG, "negative size");
  if (!b->start_X || (n_obs > 0 && (!b->X || !b->obs_idx)))
    return fail(NJODE_E_BADARG, "null batch array");
  if ((K > 0 && (!s->step_dt || !s->step_t)) || (nt > 0 && (!s->k_jump || !s->time_f32)) || !s->time_ptr)
    return fail(NJODE_E_BADARG, "null schedule array");
  if ((dims_flags & NJODE_F_MASKED) && n_obs > 0 && !b->M) return fail(NJODE_E_BADARG, "masked model needs M");
  if ((call_flags & NJODE_C_GET_LOSS) && !b->n_obs_ot) return fail(NJODE_E_BADARG, "get_loss needs n_obs_ot");
  if (dropout_p < 0.0f || dropout_p >= 1.0f) return fail(NJODE_E_BADARG, "dropout_p");
  return NJODE_OK;
}

// The five host arrays of a schedule are ONE block in the order the device copy has them
// (step_dt, step_t, k_jump, time_f32, time_ptr): one copy, or none when the block is pinned.
inline bool schedule_contiguous(const NjodeSchedule* s) {
  const size_t bdt = (size_t)s->n_steps * 4, bt = (size_t)s->n_times * 4;
  const char* h0 = (const char*)s->step_dt;
  return s->n_steps > 0 && s->n_times > 0 && (const char*)s->step_t == h0 + bdt &&
         (const char*)s->k_jump == h0 + 2 * bdt && (const char*)s->time_f32 == h0 + 2 * bdt + bt &&
         (const char*)s->time_ptr == h0 + 2 * bdt + 2 * bt;
}
// dst: the schedule block of a plan prefix
inline int upload_schedule(char* dst, const NjodeSchedule* s, hipStream_t st) {
  const int K = s->n_steps, nt = s->n_times;
  const size_t bdt = (size_t)K * 4, bt = (size_t)nt * 4, bp = ((size_t)nt + 1) * 4;
  if (schedule_contiguous(s)) {
    HIP_TRY(hipMemcpyAsync(dst, s->step_dt, 2 * bdt + 2 * bt + bp, hipMemcpyHostToDevice, st));
  } else {
    if (K > 0) {
      HIP_TRY(hipMemcpyAsync(dst, s->step_dt, bdt, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(dst + bdt, s->step_t, bdt, hipMemcpyHostToDevice, st));
    }
    if (nt > 0) {
      HIP_TRY(hipMemcpyAsync(dst + 2 * bdt, s->k_jump, bt, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(dst + 2 * bdt + bt, s->time_f32, bt, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(dst + 2 * bdt + 2 * bt, s->time_ptr, bp, hipMemcpyHostToDevice, st));
  }
  return NJODE_OK;
}

// drop: the call draws masks (a training call with dropout_p > 0 of a model with hidden layers)
struct DropSetup { DropCtx dc; float keep; };
inline DropSetup make_drop_ctx(float dropout_p, uint64_t seed, bool drop) {
  DropSetup d;
  unsigned thr = (unsigned)(dropout_p * 65536.0f + 0.5f);
  if (thr > 65535u) thr = 65535u;
  d.dc.seed_lo = (uint32_t)seed;
  d.dc.seed_hi = (uint32_t)(seed >> 32);
  d.dc.thr16 = drop ? thr : 0;
  d.keep = 1.0f - (float)d.dc.thr16 / 65536.0f;
  d.dc.inv_keep = 1.0f / d.keep;
  return d;
}

// rocPRIM's radix sort of (key, value) pairs by the key bits [0, end_bit); tmp == nullptr: only the
// temporary size into `bytes`.  onesweep: inputs of ONESWEEP_MIN pairs and more take one or two
// Onesweep passes instead of rocPRIM's default dispatch (njode_planner.hip, which defines this --
// the one unit that compiles rocPRIM).
hipError_t sort_pairs(void* tmp, size_t& bytes, const unsigned* k_in, unsigned* k_out, const int* v_in,
                      int* v_out, int n, int end_bit, bool onesweep, hipStream_t st);

}  // namespace njode
