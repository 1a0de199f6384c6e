/*
 * njode_records.h -- C ABI of the record collate in libnjode_hip.so: datasets of irregular,
 * feature-masked records resident in HBM and the two collates of the reference that turn a set
 * of records into the arrays the masked NJ-ODE model consumes.
 *
 * Reference interfaces replaced (all Python, nothing native exists to mirror):
 *   njode_records_count / _fill   latent_ODE/physionet_LODE.py:428-544
 *                                 (variable_time_collate_fn1: union time axis, rows with an
 *                                 observed feature, sorted by time then batch position) with
 *                                 latent_ODE/utils_LODE.py:370-385 (normalize_masked_data), and
 *                                 GRU_ODE_Bayes/data_utils_gru_ode_bayes.py:235-303
 *                                 (custom_collate_fn: every row, raw values); n_obs_ot as
 *                                 NJODE/physionet_train.py:336-340 recounts it from obs_idx
 *   njode_records_heldout         physionet_LODE.py:489-496 (data_type == "test": the dense
 *                                 second half of the batch's time axis)
 *   njode_records_val_count /     data_utils_gru_ode_bayes.py:160-183 (ODE_Dataset, validation:
 *   _val_fill                     df_before / df_after, groupby("ID").head(max_val_samples)) and
 *                                 :257-265 (custom_collate_fn: X_val, M_val, times_val,
 *                                 index_val sorted by ID, then Time)
 *
 * Conventions are those of njode_hip.h (device pointers, caller-owned buffers, caller's stream,
 * int return code + njode_last_error()).  Nothing is allocated, nothing is kept between calls:
 * every call rebuilds what it needs in the caller's workspace.  No atomics, no floating-point
 * reductions: the same call gives the same bits.
 *
 * Dataset layout in HBM: the rows of all records, sorted by record, then time.  A row's time is
 * an index into the dataset's sorted-unique time axis grid [G], which stays on the host
 * (float64): the kernels only ever order and compare grid indices.
 */
#ifndef NJODE_RECORDS_H
#define NJODE_RECORDS_H

#include "njode_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct NjodeRecordStore {
  int32_t n_records;        /* N                                                               */
  int32_t n_rows;           /* R: rows of all records                                          */
  int32_t dim;              /* D: features per row                                             */
  int32_t n_grid;           /* G: points of the dataset's time axis                            */
  int32_t drop_unobserved;  /* 1: a row whose mask is all zero is not collated (PhysioNet:
                               combined_mask[i, t_ind, :].sum() > 0); 0: every row is (climate) */
  int32_t reserved;
  const int32_t* row_ptr;   /* [N + 1] rows of record n: row_ptr[n] .. row_ptr[n + 1] - 1       */
  const int32_t* row_g;     /* [R] grid index of the row's time, strictly increasing within a
                               record                                                          */
  const float* vals;        /* [R][D] raw values                                               */
  const uint8_t* mask;      /* [R][D] 0 / 1 feature mask                                       */
  const float* att_min;     /* [D] normalisation, or both NULL: values are collated raw.        */
  const float* att_max;     /* x = (v - att_min[j]) / att_max[j] in fp32 (one subtraction, one
                               correctly rounded division; an att_max of 0 is taken as 1), 0
                               where the mask is 0: normalize_masked_data, which divides by
                               att_max and not by the range                                    */
} NjodeRecordStore;

/* workspace of one call of any of the three entry points below, in bytes: the slot table
 * int32 [G][B] (row of batch position b at grid index g, or "none") */
int njode_records_bytes(int32_t n_grid, int32_t B, size_t* out);

/* Collate, phase 1.  batch_idx: device int32 [B], the records of the batch in batch order; a
 * record may appear twice and then fills two batch positions; an index outside [0, N) counts as
 * a record without rows.  Outputs, per grid index g:
 *   present [G]  1 if some record of the batch has a row at g, else 0
 *   count   [G]  number of batch positions whose row at g is collated (kept)
 * The caller copies both to the host: times = grid[present], time_ptr = the running sum of
 * count[present]; a time that is present with a count of 0 is an empty slice. */
int njode_records_count(const NjodeRecordStore* store, const int32_t* batch_idx, int32_t B,
                        int32_t* present, int32_t* count, void* ws, size_t ws_bytes,
                        njodeStream_t stream);

/* Collate, phase 2, for the kept rows with g in [g_lo, g_hi), sorted by time, then batch
 * position: X fp32 [n_obs][D], M fp32 [n_obs][D], obs_idx int32 [n_obs]; n_obs_ot int32 [B] =
 * number of those rows per batch position.  count as written by phase 1 (device); n_obs is the
 * sum of count over the range and bounds every row written (X, M and obs_idx may be NULL when
 * it is 0). */
int njode_records_fill(const NjodeRecordStore* store, const int32_t* batch_idx, int32_t B,
                       const int32_t* count, int32_t g_lo, int32_t g_hi, int32_t n_obs, float* X,
                       float* M, int32_t* obs_idx, int32_t* n_obs_ot, void* ws, size_t ws_bytes,
                       njodeStream_t stream);

/* Collate, phase 2b: the held-out half of the test layout, dense.  vals_val, mask_val fp32
 * [B][n_val][D] for the grid indices g in [g_hi, G) that are present (as written by phase 1,
 * device), in increasing order; n_val must be their number.  Values as in X; a dropped row
 * (all-zero mask) keeps its place and its values; zero where the record has no row.  Every
 * cell of both outputs is written. */
int njode_records_heldout(const NjodeRecordStore* store, const int32_t* batch_idx, int32_t B,
                          const int32_t* present, int32_t g_hi, int32_t n_val, float* vals_val,
                          float* mask_val, void* ws, size_t ws_bytes, njodeStream_t stream);

/* All three: NJODE_E_BADARG for a null store, array or output, N, R, D, G or B not positive,
 * only one of att_min / att_max, a range that is not 0 <= g_lo <= g_hi <= G, a negative n_obs
 * or n_val; NJODE_E_WORKSPACE for a null or too small workspace -- before anything is
 * launched. */

/* ---- the climate validation layout ------------------------------------------------------------
 * ODE_Dataset(validation=True, val_options={T_val, max_val_samples}) + custom_collate_fn: the rows
 * up to the cut are observed, of the rows after it each record gives its first max_val, and
 * these are listed by (record index, time) with the batch position of their record beside them.
 * The cut is a grid index: g_cut = number of grid points <= float32(T_val) (the reference compares
 * the fp32 Time column); a row is observed if row_g < g_cut and held out otherwise.  The observed
 * part is njode_records_count / _fill with g_hi = g_cut; the two calls below build the held-out
 * part.  They take a store with drop_unobserved = 0 only: the layout belongs to the collate that
 * keeps every row. */

/* workspace of one call of either entry point below, in bytes: int32 [2][B] (held-out rows and
 * first held-out row of every batch position) */
int njode_records_val_bytes(int32_t B, size_t* out);

/* Held-out part, phase 1.  Every batch position finds its first row with row_g >= g_cut (binary
 * search) and holds min(max_val, rows left) rows.  val_ptr: device int32 [B + 1]; val_ptr[b] =
 * offset of position b's rows in the output order, which is by record index (the value of
 * batch_idx[b], compared as an int32), positions that hold the same record by batch position,
 * then time; val_ptr[B] = L, the number of held-out rows, which the caller copies to the host to
 * size the outputs.  An index outside [0, N) counts as a record without rows.  The order is an
 * exact count over all pairs of positions, in integers: any B, the same bits every time. */
int njode_records_val_count(const NjodeRecordStore* store, const int32_t* batch_idx, int32_t B,
                            int32_t g_cut, int32_t max_val, int32_t* val_ptr, void* ws,
                            size_t ws_bytes, njodeStream_t stream);

/* Held-out part, phase 2, with val_ptr as written by phase 1 (device) and L = val_ptr[B]:
 * X_val, M_val fp32 [L][D] (values as in X), g_val int32 [L] (grid index of the row's time:
 * times_val = grid[g_val]), index_val int32 [L] (batch position of the row's record).  Every
 * cell of the four outputs is written; L bounds every row written; the outputs may be NULL when
 * L is 0. */
int njode_records_val_fill(const NjodeRecordStore* store, const int32_t* batch_idx, int32_t B,
                           int32_t g_cut, int32_t max_val, const int32_t* val_ptr, int32_t L,
                           float* X_val, float* M_val, int32_t* g_val, int32_t* index_val,
                           void* ws, size_t ws_bytes, njodeStream_t stream);

/* Both: NJODE_E_BADARG for a null store, array, batch_idx, val_ptr or output, N, R, D, G, B or
 * max_val not positive, only one of att_min / att_max, a store with drop_unobserved = 1, g_cut
 * outside [0, G], B * min(max_val, R) beyond 31 bits, a negative L; NJODE_E_WORKSPACE for a null
 * or too small workspace -- before anything is launched. */

#ifdef __cplusplus
}
#endif
#endif /* NJODE_RECORDS_H */
