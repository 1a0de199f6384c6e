/*
 * njode_gob.h -- C ABI of the GRU-ODE-Bayes baseline of libnjode_hip.so: forward, exact discrete
 * adjoint and (through them) training of the reference's NNFOwithBayesianJumps
 * (GRU_ODE_Bayes/models_gru_ode_bayes.py:270-494) on the MI355X (gfx950), in fp32.
 *
 * The model is the one NJODE/train.py:354-392 constructs: full_gru_ode=True, logvar=True,
 * solver='euler', impute False or True, cov = start_X (cov_size == input_size).
 *   start       h = covariates_map(start_X), p = p_model(h)
 *   Euler step  r = s(x_r + W_hr h), z = s(x_z + W_hz h), u = tanh(x_h + W_hh (r * h)),
 *               h <- h + dt (1 - z)(u - h); x = lin_x(p) with impute, else 0
 *   jump        mean | logvar = p; err = (X - mean) / exp(logvar / 2);
 *               loss_1 += sum 0.5 (err^2 + logvar + log 2 pi) M; prep layer; h <- GRUCell(g, h);
 *               p = p_model(h); loss_2 += sum KL(N(mean', s'^2) || N(X, 0.01^2)) M
 *   loss = loss_1 + mixing loss_2 (no division by the batch size); every path runs to T.
 *
 * Conventions are those of njode_f64.h: extern "C"; device pointers unless stated; the caller owns
 * every buffer; all work is enqueued on the caller's stream and nothing synchronises; the library
 * keeps no state for these calls and allocates nothing; 0 on success, an NJODE_E_* code otherwise
 * with the message in the thread's last-error string; every NJODE_E_BADARG refusal is made before
 * anything is launched.  `workspace` must be aligned to 256 bytes.  Indices are int32.
 *
 * Parameter vector: flat fp32, state_dict order, only what the loss depends on (the
 * classification head and gru_obs.gru_debug are not in it), weights [out][in] row-major, the bias
 * slot of every Linear / GRUCell always present (zero with bias=False):
 *     p_model.0.{weight [PH, H], bias}, p_model.3.{weight [2 d, PH], bias},
 *     [impute: gru_c.lin_x.{weight [3 H, 2 d], bias},]
 *     gru_c.lin_hh.weight, gru_c.lin_hz.weight, gru_c.lin_hr.weight   ([H, H] each, no bias)
 *     gru_obs.w_prep [d, 4, PR], gru_obs.bias_prep [d, PR],
 *     gru_obs.gru_d.{weight_ih [3 H, PR d], weight_hh [3 H, H], bias_ih, bias_hh},
 *     covariates_map.0.{weight [CH, d], bias}, covariates_map.3.{weight [H, CH], bias}
 *
 * One plan: a wave per path walks the whole schedule, a lane per unit.  Gradients are
 * deterministic: no atomics anywhere, the same call gives the same bits.
 */
#ifndef NJODE_GOB_H
#define NJODE_GOB_H

#include "njode_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NJODE_GOB_F_BIAS 0x1   /* bias=True (only recorded: the slots exist either way)  */
#define NJODE_GOB_F_IMPUTE 0x2 /* impute=True: the cell has lin_x and is fed p            */

typedef struct NjodeGobDims {
  int32_t input_size;  /* d   (2 d <= 64)                                  */
  int32_t hidden_size; /* H   (<= 64)                                      */
  int32_t p_hidden;    /* PH  (<= 64)                                      */
  int32_t prep_hidden; /* PR  (PR d <= 256)                                */
  int32_t cov_hidden;  /* CH  (<= 64)                                      */
  int32_t flags;       /* NJODE_GOB_F_*                                    */
} NjodeGobDims;

/* 1 if the kernels run `dims`, else 0 with the reason in the last-error string.  Pure host. */
int njode_gob_supported(const NjodeGobDims* dims);

/* Length of the flat parameter vector (0 if unsupported). */
size_t njode_gob_param_count(const NjodeGobDims* dims);

/* Bytes of workspace the two calls below need: an exact promise.  Pure host.  call_flags:
 * NJODE_C_TRAIN, NJODE_C_RETURN_PATH, NJODE_C_SAVE_BWD (others are refused); the same flags go to
 * the forward and its backward.  With SAVE_BWD the workspace holds the state before every Euler
 * step and jump and at the end ([K][B][H], [n_obs][H], [B][H] floats) and the per-workgroup
 * weight-gradient slabs (a count that depends on dims and B only, times P floats). */
int njode_gob_workspace_bytes(const NjodeGobDims* dims, int32_t batch_size, int32_t n_obs,
                              int32_t n_times, int32_t n_steps, int32_t call_flags, size_t* out);

/*
 * NNFOwithBayesianJumps.forward.  Of `batch` it reads batch_size, n_obs, start_X, X, M (always
 * required with n_obs > 0) and obs_idx; row b of the batch is dropout path b.
 *   hT      [B, H]               state at T
 *   loss    [2]                  {loss_1 + mixing loss_2, loss_1}
 *   path_h  [n_rows, B, H]       (iff RETURN_PATH) n_rows = 1 + n_steps + n_times: t = 0, after
 *   path_p  [n_rows, B, 2 d]     every Euler step, after every time slice (the reference's order)
 * dropout_p and seed are read by NJODE_C_TRAIN calls only: masks of the shape-generic stream,
 * layer 0, nets 5 (covariates_map), 6 (p_model at the start and after Euler step k, time key
 * k), 7 (p_model after time slice i, time key k_jump[i]).
 */
int njode_gob_forward_f32(const NjodeGobDims* dims, const float* params, const NjodeBatch* batch,
                          const NjodeSchedule* sched, int32_t call_flags, float mixing,
                          float dropout_p, uint64_t seed, float* hT, float* loss, float* path_h,
                          float* path_p, void* workspace, size_t workspace_bytes,
                          njodeStream_t stream);

/*
 * The exact discrete adjoint of the call above.  Must follow a forward call with NJODE_C_SAVE_BWD
 * on the same workspace, dims, params, batch, mixing, dropout_p, seed and flags; of `sched` it
 * reads n_steps and n_times only.
 *   grad_loss    [1]     upstream gradient of loss[0]
 *   grad_loss_1  [1]     upstream gradient of loss[1]
 *   grad_hT      [B, H]  upstream gradient of hT, or NULL
 *   grad_params  [P]     OVERWRITTEN
 */
int njode_gob_backward_f32(const NjodeGobDims* dims, const float* params, const NjodeBatch* batch,
                           const NjodeSchedule* sched, int32_t call_flags, float mixing,
                           float dropout_p, uint64_t seed, const float* grad_loss,
                           const float* grad_loss_1, const float* grad_hT, float* grad_params,
                           void* workspace, size_t workspace_bytes, njodeStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NJODE_GOB_H */
