/*
 * njode_f64.h -- C ABI of the float64 route of libnjode_hip.so: NJ-ODE forward, exact discrete
 * adjoint and (through them) training in double precision on the MI355X (gfx950).
 *
 * What it computes is the reference's NJODE.forward under model.double() (models.py:379-518),
 * dropout off: every parameter, input, activation, loss term and gradient is a double.  Three
 * things stay what the reference makes them:
 *   - tau is an fp32 tensor (models.py:418): it holds fp32(obs_time);
 *   - tdiff = fp32(current_time) - tau is computed in fp32, and so is tau + tdiff of
 *     input_current_t; all three are then widened exactly;
 *   - the Euler update h + step * f uses the float64 step of the reference's Python clock.
 *
 * Conventions are those of njode_hip.h: extern "C"; device pointers unless stated; the caller owns
 * every buffer; all work is enqueued on the caller's stream and nothing synchronises; the library
 * keeps no state for these calls and allocates nothing; 0 on success, an NJODE_E_* code otherwise
 * with the message in the thread's last-error string; every NJODE_E_BADARG refusal is made before
 * anything is launched.  `workspace` must be aligned to 256 bytes.  Indices are int32.
 *
 * Parameter vector: the layout of njode_hip.h (three networks in state_dict order, each weight
 * [out][in] row-major, bias slots always present), as doubles.  use_rnn models are refused.
 *
 * One plan: a workgroup per path walks the whole schedule (Euler steps, jumps); a path's outputs
 * do not depend on the other paths of the call or on the batch size.  Gradients are deterministic:
 * no atomics anywhere, the same call gives the same bits.
 */
#ifndef NJODE_F64_H
#define NJODE_F64_H

#include "njode_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Time grid of one pass.  HOST arrays, copied to the workspace asynchronously by the forward call
 * (keep them valid until the stream has passed it; the backward call reads the workspace copy
 * only).  step_dt is the float64 clock's own step; the other arrays are those of NjodeSchedule.
 */
typedef struct NjodeSchedule64 {
  int32_t n_steps;         /* K: Euler steps in this pass (incl. the until_T tail)    */
  int32_t n_times;         /* number of observation times                            */
  const double* step_dt;   /* [K]  delta_t_k, float64                                */
  const float* step_t;     /* [K]  fp32(current_time before step k)                  */
  const int32_t* k_jump;   /* [n_times] Euler steps completed before jump i happens  */
  const float* time_f32;   /* [n_times] fp32(times[i])  (the value written to tau)   */
  const int32_t* time_ptr; /* [n_times+1] CSR offsets into X / obs_idx               */
} NjodeSchedule64;

/* NjodeBatch with double data arrays. */
typedef struct NjodeBatch64 {
  int32_t batch_size;      /* B                                                       */
  int32_t n_obs;           /* rows of X / obs_idx                                     */
  const double* start_X;   /* [B, d]                                                  */
  const double* X;         /* [n_obs, d]  sorted by time, then path                   */
  const double* M;         /* [n_obs, d]  0/1 mask, or NULL (required iff MASKED)     */
  const int32_t* obs_idx;  /* [n_obs]  path of each row, in [0, B); at most one row per path and
                              time slice.  A row whose index is outside [0, B) is ignored.  */
  const int32_t* n_obs_ot; /* [B] observations per path, or NULL if !GET_LOSS         */
  double loss_batch_size;  /* the `batch_size` of compute_loss (models.py:106)        */
} NjodeBatch64;

/* 1 if the float64 route runs `dims`, else 0 with the reason in the last-error string.  A pure
 * host function.  The envelope is that of the shape-generic fp32 kernels (njode_hip.h): any
 * sizes they take, 0 to NJODE_MAX_HIDDEN hidden layers, per_net descriptions, tanh / relu, every
 * residual case, input_current_t, masked models (input_size == output_size), unmasked models
 * with output_size != input_size (prediction calls).  use_rnn is refused. */
int njode_f64_supported(const NjodeDims* dims);

/* Bytes of workspace the two calls below need: an exact promise, as njode_workspace_bytes is.
 * call_flags: NJODE_C_GET_LOSS, NJODE_C_RETURN_PATH, NJODE_C_SAVE_BWD (others are refused);
 * the same flags go to the forward and its backward.  With SAVE_BWD the workspace holds the
 * state before every Euler step and jump ([K][B][H] and [n_obs][H + d] doubles) and the
 * per-workgroup weight-gradient slabs (a count that depends on dims and B only, times P doubles). */
int njode_f64_workspace_bytes(const NjodeDims* dims, int32_t batch_size, int32_t n_obs,
                              int32_t n_times, int32_t n_steps, int32_t call_flags, size_t* out);

/*
 * NJODE.forward in double.
 *   hT      [B, H]                  state at the end of the pass; may be NULL
 *   loss    [1]                     (written iff GET_LOSS)
 *   path_h  [n_rows, B, H]          (iff RETURN_PATH) n_rows = 1 + n_steps + n_times, in the
 *   path_y  [n_rows, B, d_out]      reference's row order
 * GET_LOSS needs input_size == output_size and n_obs_ot.
 */
int njode_forward_f64(const NjodeDims* dims, const double* params, const NjodeBatch64* batch,
                      const NjodeSchedule64* sched, int32_t call_flags, double weight, double* hT,
                      double* loss, double* path_h, double* path_y, void* workspace,
                      size_t workspace_bytes, njodeStream_t stream);

/*
 * The exact discrete adjoint of the call above.  Must follow a forward call with NJODE_C_SAVE_BWD
 * on the same workspace, dims, params, batch, weight and flags; of `sched` it reads n_steps and
 * n_times only.
 *   grad_loss    [1]     upstream gradient of the loss; NULL (as zero) without GET_LOSS
 *   grad_hT      [B, H]  upstream gradient of hT, or NULL.  Accepted on every supported model.
 *   grad_params  [P]     OVERWRITTEN with grad_loss * d loss / d params + d <grad_hT, hT> / d params
 */
int njode_backward_f64(const NjodeDims* dims, const double* params, const NjodeBatch64* batch,
                       const NjodeSchedule64* sched, int32_t call_flags, double weight,
                       const double* grad_loss, const double* grad_hT, double* grad_params,
                       void* workspace, size_t workspace_bytes, njodeStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NJODE_F64_H */
