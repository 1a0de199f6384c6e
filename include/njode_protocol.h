/*
 * njode_protocol.h -- C ABI of the real-data evaluation protocols in libnjode_hip.so: which rows
 * of a prediction path answer a list of held-out times, and the masked squared errors of the
 * prediction at those rows.  The prediction path stays in HBM; a call returns four doubles.
 *
 * Reference interfaces replaced (all Python, nothing native exists to mirror):
 *   njode_protocol_rows, NJODE_ROWS_CLOSEST        physionet_train.py:473-505
 *                                                  (get_comparison_times_ind)
 *   njode_protocol_rows, NJODE_ROWS_FIRST_NEAREST  data_utils_gru_ode_bayes.py:379-400
 *                                                  (extract_from_path)
 *   njode_protocol_score_f32, dense layout         physionet_train.py:411-470 (evaluate_model) and
 *                                                  likelihood_eval_LODE.py:171-193, 229-236
 *   njode_protocol_score_f32, sparse layout        climate_train.py:508-566 (evaluate_model)
 * Python: njode_amd/protocol.py, physionet_eval.evaluate_model_device,
 * climate_eval.evaluate_model_device.
 *
 * Conventions are those of njode_hip.h and njode_producer.h: device pointers, caller-owned
 * buffers, the caller's stream, int return code + njode_last_error(), no state kept in the
 * library, a workspace whose size the library states.  Nothing here waits for the device.
 */
#ifndef NJODE_PROTOCOL_H
#define NJODE_PROTOCOL_H

#include "njode_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NJODE_ROWS_CLOSEST 0
#define NJODE_ROWS_FIRST_NEAREST 1

/* rows[q] = the row of path_t that answers query[q].  path_t f64 [n_rows] (device,
 * non-decreasing, n_rows >= 1), query f64 [n_query] (device), rows i32 [n_query] (device).
 * One thread per query, binary searches on the float64 values the host functions compare; the
 * rows are equal to the host's.
 *
 * NJODE_ROWS_CLOSEST (get_comparison_times_ind): the first i in [0, n_rows - 2] with
 *   |path_t[i] - t| < 1e-10  or  path_t[i] <= t < path_t[i + 1];
 *   the answer is i if |t - path_t[i]| <= |t - path_t[i + 1]|, else i + 1; n_rows - 1 when there
 *   is no such i (a time at or past the last row).
 * NJODE_ROWS_FIRST_NEAREST (extract_from_path): of the distinct values of path_t the one nearest
 *   to t (|value - t| in float64, ties to the earlier value); the answer is the FIRST row that
 *   holds it -- where a jump repeats a time, the prediction before the jump.  The caller passes
 *   the path_t it has rounded and cast through float32 (climate_train.py:549-551), widened back
 *   to float64: the rounding stays on the host.
 *
 * NJODE_E_BADARG: a null pointer, n_rows < 1, n_query < 0, an unknown rule.  n_query = 0 is a
 * call that launches nothing. */
int njode_protocol_rows(const double* path_t, int32_t n_rows, const double* query, int32_t n_query,
                        int32_t rule, int32_t* rows, njodeStream_t stream);

/* One batch to score.  Exactly one of the two target layouts is given (the other's pointers are
 * all NULL); all pointers are device pointers.
 *   dense  (PhysioNet): vals, mask fp32 [B][n_query][dim]; the prediction for (b, j) is
 *                       pred[rows[j]][b]
 *   sparse (climate):   X_val, M_val fp32 [n_query][dim], index_val i32 [n_query]; the
 *                       prediction for l is pred[rows[l]][index_val[l]]
 * A rows[] entry outside [0, n_rows) or an index_val[] entry outside [0, B) is the caller's
 * mistake; such an entry contributes nothing and nothing is read out of bounds. */
typedef struct NjodeProtocolJob {
  const float* pred;        /* fp32 [n_rows][B][dim]: the model's path_y                  */
  int32_t n_rows;           /* rows of the path                                           */
  int32_t B;                /* paths of the batch                                         */
  int32_t dim;              /* output_size                                                */
  int32_t n_query;          /* dense: T2 held-out times, sparse: L held-out rows          */
  const int32_t* rows;      /* [n_query] rows of pred (njode_protocol_rows)               */
  const float* vals;        /* dense                                                      */
  const float* mask;        /* dense                                                      */
  const float* X_val;       /* sparse                                                     */
  const float* M_val;       /* sparse                                                     */
  const int32_t* index_val; /* sparse                                                     */
} NjodeProtocolJob;

/* workspace of one njode_protocol_score_f32 call of these sizes (either layout), in bytes;
 * non-decreasing in every argument.  NJODE_E_BADARG: a negative size, B or dim of 0, a null
 * `bytes`. */
int njode_protocol_bytes(int32_t n_rows, int32_t n_query, int32_t B, int32_t dim, size_t* bytes);

/* out f64 [4] (device) = { sq_sum, n_obs, attr_mse, 0 }:
 *   sq_sum   sum over the held-out entries of ((pred - val)^2 * mask): every term is formed in
 *            fp32 as numpy forms it on the host (subtract, square, multiply by the mask, no
 *            fused multiply-add), widened to float64 and summed
 *   n_obs    sum of mask (float64)
 *   attr_mse dense layout: in float64, per (path, attribute) the sum over the times with
 *            mask > 0 of (pred - val)^2 divided by their count (0 where the count is 0), the
 *            mean over the attributes, then the mean over the paths.  Sparse layout: 0.
 * accumulate != 0: out[0..2] += the call's values (each formed first, then added once by one
 * thread) and out[3] = 0; else out is overwritten.  Every sum is reduced in a fixed order --
 * per-thread float64 partials, a tree within the wave, the workgroups' partials in index order
 * -- without floating-point atomics: the same call gives the same bits.
 *
 * NJODE_E_BADARG: a null job, pred, rows, out or ws, a negative size, B or dim of 0, both or
 * neither target layout (or half of one).  NJODE_E_WORKSPACE: ws_bytes below
 * njode_protocol_bytes(n_rows, n_query, B, dim).  Nothing is launched by a refused call. */
int njode_protocol_score_f32(const NjodeProtocolJob* job, double* out, int32_t accumulate,
                             void* ws, size_t ws_bytes, njodeStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NJODE_PROTOCOL_H */
