/*
 * njode_producer.h -- C ABI of the GPU-side batch producer in libnjode_hip.so
 * (SURVEY.md section 8 row f1): synthetic SDE datasets resident in HBM and the
 * CSR-by-time collate that turns a set of paths into the arrays NJODE.forward consumes.
 *
 * Reference interfaces replaced (all Python, nothing native exists to mirror):
 *   njode_generate_paths       stock_model.py:356-375 (BlackScholes.generate_paths),
 *                              :397-418 (OrnsteinUhlenbeck), :181-221 (Heston)
 *   njode_sample_observations  data_utils.py:73-81 (observation mask of create_dataset)
 *   njode_collate_count/_fill  data_utils.py:278-316 (custom_collate_fn) and
 *                              :352-416 (CustomCollateFnGen, func_appl_X = power-k)
 *   njode_cond_exp_f64         stock_model.py:50-158 (compute_cond_exp, get_optimal_loss),
 *                              :178, :353, :393 (next_cond_exp), :471-481 (compute_loss)
 *   njode_generate_stage       stock_model.py:288-335 (HestonWOFeller.generate_paths) and the
 *                              three generators above started from start_X, as
 *                              data_utils.py:111-195 (create_combined_dataset) chains them
 *   njode_cond_exp_staged_f64  stock_model.py:421-466 (Combined.compute_cond_exp: stage i starts
 *                              where stage i - 1 ended), :277-286 (HestonWOFeller.next_cond_exp
 *                              with and without return_vol)
 *
 * Conventions are those of njode_hip.h (device pointers, caller-owned buffers, caller's
 * stream, int return code + njode_last_error()).
 *
 * Dataset layout in HBM ("time-major"): paths f64 [S+1][dim][N], observed u8 [S+1][N].
 * A time slice of all paths is contiguous, so generation (one thread per path walks the grid)
 * writes, and the collate (one workgroup per grid time scans the batch) reads, with unit
 * stride across lanes.  Values stay float64 like the reference's dataset; the collate casts
 * to fp32 at the same place the reference does (data_utils.py:291,314).
 */
#ifndef NJODE_PRODUCER_H
#define NJODE_PRODUCER_H

#include "njode_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NJODE_SDE_BLACK_SCHOLES 0
#define NJODE_SDE_ORNSTEIN_UHLENBECK 1
#define NJODE_SDE_HESTON 2

/* hyper-parameters of stock_model.StockModel (data_utils.hyperparam_default:25-31) */
typedef struct NjodeSde {
  int32_t model;    /* NJODE_SDE_*                                              */
  int32_t n_paths;  /* N                                                        */
  int32_t dim;      /* dimensions = np.size(S0)                                 */
  int32_t n_steps;  /* S  (grid has S + 1 points)                               */
  int32_t has_sine; /* sine_coeff given: periodic_coeff(t) = 1 + sin(coeff * t) */
  int32_t reserved;
  double drift, volatility, mean, speed, correlation, S0, maturity, sine_coeff;
} NjodeSde;

/* Philox4x32-10 on `n` (counter, key) pairs: ctr [n][4], key [n][2] -> out [n][4].
 * Exposed so the generator's random stream can be pinned to the published known-answer
 * vectors of the algorithm (Salmon et al., SC'11). */
int njode_philox4x32_10(int32_t n, const uint32_t* ctr, const uint32_t* key, uint32_t* out,
                        njodeStream_t stream);

/* Euler-Maruyama paths of `sde` into paths_tm f64 [S+1][dim][N].
 * normals == NULL : standard normals from Philox4x32-10 keyed by `seed`, Box-Muller on 53-bit
 *                   uniforms; counter = (path, step, dim) for Heston (both normals of the
 *                   pair are used by one step), (path, ceil(step / 2), dim) otherwise (the
 *                   pair feeds steps 2m - 1 and 2m).
 * normals != NULL : device f64 array in the reference's draw order, [N][S][dim]
 *                   (Heston: [N][S][2][dim]); the recurrences then reproduce the reference's
 *                   float64 arithmetic operation by operation. */
int njode_generate_paths(const NjodeSde* sde, uint64_t seed, const double* normals,
                         double* paths_tm, njodeStream_t stream);

/* observed_tm[t][n] = (u < obs_perc), nb_obs[n] = number of observations at t >= 1.
 * uniforms == NULL: Philox draws; else device f64 [N][S+1] in the reference's order. */
int njode_sample_observations(int32_t n_paths, int32_t n_steps, double obs_perc, uint64_t seed,
                              const double* uniforms, uint8_t* observed_tm, int32_t* nb_obs,
                              njodeStream_t stream);

/* Collate, phase 1.  batch_idx: device int32 [B] dataset rows of the batch in batch order
 * (NULL = rows 0..B-1).  Outputs: count_per_time [S] = observations of the batch at grid
 * time t = 1..S; n_obs_ot [B] = nb_obs gathered.  The caller copies count_per_time to the
 * host: times = the grid times with a positive count, time_ptr = their running sum. */
int njode_collate_count(const uint8_t* observed_tm, const int32_t* nb_obs, int32_t n_paths,
                        int32_t n_steps, const int32_t* batch_idx, int32_t B,
                        int32_t* count_per_time, int32_t* n_obs_ot, njodeStream_t stream);

/* Collate, phase 2.  Rows sorted by time, then batch position (custom_collate_fn's order):
 * X [n_obs][dim * (1 + n_powers)] fp32, obs_idx [n_obs] int32, start_X [B][dim * (1 +
 * n_powers)].  powers: HOST array of the lifts appended by func_appl_X (k >= 1: 'power-k',
 * 0: 'exp'), n_powers <= 4.  count_per_time as written by phase 1 (device). */
int njode_collate_fill(const double* paths_tm, const uint8_t* observed_tm, int32_t n_paths,
                       int32_t dim, int32_t n_steps, const int32_t* batch_idx, int32_t B,
                       const int32_t* count_per_time, const int32_t* powers, int32_t n_powers,
                       float* start_X, float* X, int32_t* obs_idx, njodeStream_t stream);

/* ---- analytic conditional expectation and the metrics taken against it -----------------
 * Reference: stock_model.py:50-158 (compute_cond_exp, get_optimal_loss), :178 / :353 / :393
 * (next_cond_exp of Heston / BlackScholes / OrnsteinUhlenbeck), :471-481 (compute_loss).
 *
 * The float64 clock of the walk, HOST (or pinned) arrays.  NjodeSchedule's fp32 roundings are
 * not enough here: the factor of a step is exp(rate * periodic_coeff(step_t) * step_dt) in
 * float64.  Python: schedule.cond_exp_clock. */
typedef struct NjodeCondExpSchedule {
  int32_t n_steps;         /* K: Euler steps up to T                                   */
  int32_t n_times;         /* number of observation times                              */
  const double* step_dt;   /* [K] length of step k                                     */
  const double* step_t;    /* [K] clock before step k                                  */
  const int32_t* k_jump;   /* [n_times] Euler steps completed when jump i happens      */
  const int32_t* time_ptr; /* [n_times + 1] rows of X per observation time (CSR)       */
} NjodeCondExpSchedule;

/* workspace of one call, in bytes */
int njode_cond_exp_bytes(int32_t B, int32_t n_obs, int32_t n_times, int32_t n_steps, int32_t dim,
                         size_t* out);

/* The true conditional expectation of `sde` along the batch's schedule, walked in float64 from
 * start_X (fp32 inputs are widened exactly): per Euler step y = y * a_k + c_k with
 * a_k = exp(rate * periodic_coeff(step_t[k]) * step_dt[k]) (rate = drift; OrnsteinUhlenbeck:
 * -speed and c_k = mean * (1 - a_k), else c_k = 0), at jump i y[obs_idx[r]] = X[r] for the rows
 * of slice i.  Rows of the path: [start | one per Euler step | one per jump] in the order of
 * the clock (the model's path_y of a RETURN_PATH call with the until-T tail).
 *
 * Of `sde` only model, dim, has_sine, sine_coeff, drift, mean and speed are read (n_paths and
 * n_steps are ignored); of `batch` batch_size, n_obs, start_X [B][dim], X [n_obs][dim],
 * obs_idx and n_obs_ot (device pointers; at most one row per path and time slice).
 *
 * Outputs (device, each may be NULL, not all three):
 *   path_y   f64 [1 + K + n_times][B][dim]
 *   opt_loss f64 [1]  loss of the true conditional expectation: the sum over the rows of
 *                     (2 w sqrt(eps) + 2 (1 - w) sqrt(sum_d (y_before_jump - X)^2 + eps))^2
 *                     / n_obs_ot[path], divided by B; eps = 1e-10, w = weight
 *   sq_diff  f64 [1]  sum over all rows, paths and dims of (pred - path_y)^2 against
 *                     pred fp32 [1 + K + n_times][B][dim]; the path is not stored for it
 * Sums are reduced in a fixed order: the same call gives the same bits.
 *
 * NJODE_E_BADARG: null or negative arguments, no output, sq_diff without pred, opt_loss
 * without n_obs_ot, a non-NULL batch->M, an unknown model, a time_ptr / k_jump that is not a
 * schedule of this batch.  NJODE_E_WORKSPACE: ws_bytes too small. */
int njode_cond_exp_f64(const NjodeSde* sde, const NjodeBatch* batch,
                       const NjodeCondExpSchedule* sched, double weight, const float* pred,
                       double* path_y, double* opt_loss, double* sq_diff, void* ws,
                       size_t ws_bytes, njodeStream_t stream);

/* ---- regime-switch datasets and Heston without the Feller condition ----------------------
 * The entry points above keep their model set; the fourth model and the stage-by-stage forms
 * arrive through the entry points below. */
#define NJODE_SDE_HESTON_WO_FELLER 3
#define NJODE_MAX_STAGES 16

/* One stage of a regime-switch dataset, or a single model with the options of the fourth. */
typedef struct NjodeSdeStage {
  NjodeSde sde;        /* model: any NJODE_SDE_*; n_steps = S_i and maturity of THIS stage     */
  double v0;           /* HestonWOFeller: variance at the stage's start (reference: mean)      */
  int32_t return_vol;  /* HestonWOFeller: the variance is stored as coordinates dim .. 2 dim-1 */
  int32_t first_step;  /* generation: s0, the grid index the stage starts at;
                          conditional expectation: index of the stage's first Euler step      */
} NjodeSdeStage;

/* Euler-Maruyama paths of one stage into slices [s0 .. s0 + S_i] of paths_tm
 * f64 [total_steps + 1][dim_out][N], dim_out = dim (return_vol: 2 dim).  s0 = 0: the stage starts
 * from S0 and writes slice 0.  s0 > 0: the start values are READ from slice s0 (the previous
 * stage's last slice), which is left untouched; the variance of Heston / HestonWOFeller starts
 * afresh (mean / v0), as the reference's generators do.
 * normals == NULL : Philox draws as in njode_generate_paths with the GLOBAL grid index s0 + k
 *                   in the counter's step word (Black-Scholes / OrnsteinUhlenbeck: pair
 *                   ceil((s0 + k) / 2), first normal at odd, second at even global index; a
 *                   stage at an odd s0 takes the second normal of a pair first).
 *                   periodic_coeff sees the stage-local time (k - 1) dt, dt = maturity / S_i.
 * normals != NULL : the stage's own draws, [N][S_i][dim] (Heston, HestonWOFeller:
 *                   [N][S_i][2][dim]).
 * HestonWOFeller (float64, no fused multiply-adds, vp = max(v, 0) of the PREVIOUS variance):
 *   s' = exp((log(s) + (drift pc - 0.5 vp) dt) + sqrt(vp) dW)
 *   v' = (v + (-speed (vp - mean)) dt) + (volatility sqrt(vp)) dZ
 * NJODE_E_BADARG: null or non-positive sizes, s0 < 0 or s0 + S_i > total_steps, an unknown
 * model, correlation outside [-1, 1], return_vol with another model or with s0 > 0. */
int njode_generate_stage(const NjodeSdeStage* stage, int32_t total_steps, uint64_t seed,
                         const double* normals, double* paths_tm, njodeStream_t stream);

/* workspace of one staged call, in bytes */
int njode_cond_exp_staged_bytes(int32_t B, int32_t n_obs, int32_t n_times, int32_t n_steps,
                                int32_t dim, int32_t n_stages, size_t* out);

/* njode_cond_exp_f64 for a chain of stages (HOST array, 1 <= n_stages <= NJODE_MAX_STAGES):
 * Euler step k takes the factors of the stage with the largest first_step <= k; the clock
 * (schedule.cond_exp_clock with stage maturities) carries the partial step that ends a stage.
 * step_t is the global clock: that is what a stage's periodic_coeff sees.  Of each stage
 * sde.model, has_sine, sine_coeff, drift, mean, speed, return_vol and first_step are read; the
 * width `dim` of the batch is stages[0].sde.dim.
 * Factors per coordinate class: class 0  a = exp(rate pc(t) step), c = 0 (OrnsteinUhlenbeck:
 * mean (1 - a)); class 1, the variance coordinates j >= dim / 2 of a return_vol stage:
 * a = exp(-speed step), c = mean (1 - a), no periodic coefficient.
 * Outputs, reductions and reproducibility as njode_cond_exp_f64; a single stage of one of its
 * three models gives the same bits as that call.
 * NJODE_E_BADARG: what njode_cond_exp_f64 refuses, n_stages outside [1, NJODE_MAX_STAGES],
 * first_step not strictly increasing from 0 or beyond n_steps, return_vol with an odd dim, with
 * another model or in a call of more than one stage, an unknown model. */
int njode_cond_exp_staged_f64(const NjodeSdeStage* stages, int32_t n_stages,
                              const NjodeBatch* batch, const NjodeCondExpSchedule* sched,
                              double weight, const float* pred, double* path_y, double* opt_loss,
                              double* sq_diff, void* ws, size_t ws_bytes, njodeStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NJODE_PRODUCER_H */
