/*
 * njode_online.h -- C ABI of online filtering in libnjode_hip.so: the state of a set of series
 * stays in device memory between calls; a call feeds the listed series their next observation or
 * reads a forecast, at the cost of the Euler steps that are new.
 *
 * Reference interface replaced: none exists as code.  The reference only has the batch form,
 * NJODE.forward (NJODE/models.py:379-518), which starts at t = 0 and needs the whole record.  The
 * results of any sequence of calls below on one series are, by definition, those of that forward on
 * the batch that consists of the series alone, with `times` = the targets of the calls in order:
 *   njode_online_reset_f32    models.py:404-413  h = encoder_map(start_X) (masked: mask = 0),
 *                                                last_X = start_X, tau = 0, current_time = 0
 *   njode_online_advance_f32  models.py:430-445  the while loop of ONE time slice that nobody observes
 *   njode_online_observe_f32  models.py:430-489  that loop, then the jump: Y_bj = readout(h),
 *                                                h = encoder(X) (masked: encoder(X M + (1 - M) Y_bj, M)),
 *                                                Y = readout(h), last_X = X (masked: Y), tau = fp32(t)
 *   njode_online_predict_f32  models.py:564-584  get_pred's path_y at empty slices at the queries, on
 *                                                a copy of the state
 * Eval mode (no dropout), no loss, no backward pass.
 *
 * The clock.  Each series has its own float64 clock `now`; a target t is reached by
 *     while now < t - 1e-10 delta_t:  step = delta_t if now < t - delta_t else t - now;  now += step
 * in float64, exactly the reference's loop; an Euler step consumes fp32(step) and fp32(now before
 * it).  `now` changes through Euler steps only: a jump at t <= now takes no step and is legal.
 * The loop is counted: at most max_steps Euler steps are taken in front of ONE target (predict: in
 * front of each of its Q queries).  A series the bound stops keeps the state it has reached
 * (advance and observe write it; observe applies no jump and fills the series' rows of Y_before / Y
 * with NaN; predict fills the rows of the query it could not reach, and of those behind it, with
 * NaN) and gets status 1.
 *
 * Conventions are those of njode_hip.h: device pointers, caller-owned buffers, the caller's stream,
 * int return code + njode_last_error(), no state in the library, nothing allocated, nothing
 * synchronised.  `dims` and `params` as for njode_forward_f32 (the same flat vector).  One wave
 * per listed series; no atomics: the same call on the same state gives the same bits.
 */
#ifndef NJODE_ONLINE_H
#define NJODE_ONLINE_H

#include "njode_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Struct of arrays; row i belongs to series i. */
typedef struct NjodeOnlineState {
  float* h;         /* [n_series][hidden_size]                                               */
  float* last_X;    /* [n_series][input_size]                                                */
  float* tau;       /* [n_series] fp32 time of the series' last observation                  */
  double* now;      /* [n_series] the series' clock                                          */
  int32_t n_series;
} NjodeOnlineState;

/* 1 if the entry points below run this model, else 0; the reason (either way) is left in
 * njode_last_error().  A pure host function.  Runs: a shape of the build table (per_net = 0) with
 * two hidden layers per network, input_size, hidden_size, output_size and width <= 64, no GRU jump
 * (masked models: input_size == output_size).  Refused: nn_desc = None and any other depth,
 * use_rnn, wider models, per-network descriptions, shapes that were not compiled. */
int njode_online_supported(const NjodeDims* dims);

/* Arguments common to the entry points:
 *   ids     device int32 [n], the series of the call's rows, each in [0, n_series); NULL: 0 .. n-1
 *           (then n <= n_series).  The ids of one call must be DISTINCT: two rows on one series
 *           are two waves that race on its state -- the caller's contract, not checked.  An id
 *           outside the state is not followed: its row gets status 2 and touches nothing.
 *   n       rows of the call, 0 <= n (0: nothing is launched)
 *   t       device float64 [n] (predict: [n][Q]), the targets
 *   delta_t, max_steps   the Euler step and the bound described above
 *   status  device int32 [n], every entry written: 0 reached, 1 stopped by the bound, 2 bad id
 *           (njode_online_run_f32: 3 bad event range)
 * Every call returns NJODE_E_UNSUPPORTED for a model njode_online_supported refuses and
 * NJODE_E_BADARG -- before anything is launched -- for a null dims, params, state, state array,
 * t, status or required input, n_series <= 0, n < 0, n > n_series with ids == NULL, a delta_t that
 * is not finite and positive, max_steps <= 0, Q <= 0, M given to an unmasked model or missing
 * for a masked one. */

/* start_X: device fp32 [n][input_size].  Writes h, last_X, tau = 0, now = 0 of the listed series. */
int njode_online_reset_f32(const NjodeDims* dims, const float* params, const NjodeOnlineState* state,
                           const int32_t* ids, int32_t n, const float* start_X, njodeStream_t stream);

/* An empty time slice at t: the clock and h of the listed series move, last_X and tau do not. */
int njode_online_advance_f32(const NjodeDims* dims, const float* params, const NjodeOnlineState* state,
                             const int32_t* ids, int32_t n, const double* t, double delta_t,
                             int32_t max_steps, int32_t* status, njodeStream_t stream);

/* advance to t, then the jump.  X: device fp32 [n][input_size]; M: device fp32 [n][input_size],
 * masked models only (else NULL).  Y_before, Y: device fp32 [n][output_size], each may be NULL:
 * the readout before and after the jump. */
int njode_online_observe_f32(const NjodeDims* dims, const float* params, const NjodeOnlineState* state,
                             const int32_t* ids, int32_t n, const double* t, const float* X,
                             const float* M, double delta_t, int32_t max_steps, float* Y_before,
                             float* Y, int32_t* status, njodeStream_t stream);

/* t_query: device float64 [n][Q], ascending within a row (a query below its predecessor takes no
 * step).  Y: device fp32 [n][Q][output_size], the readout at each query; a later query goes on
 * from where the earlier one stopped, its partial step included.  No byte of the state is
 * written. */
int njode_online_predict_f32(const NjodeDims* dims, const float* params, const NjodeOnlineState* state,
                             const int32_t* ids, int32_t n, const double* t_query, int32_t Q,
                             double delta_t, int32_t max_steps, float* Y, int32_t* status,
                             njodeStream_t stream);

/* A run of events per series in one launch.  Events are laid out BY SERIES (CSR): row r of the call
 * owns events ev_ptr[r] .. ev_ptr[r + 1] - 1 and applies them, in that order, to series ids[r].
 *   ev_ptr   device int32 [n + 1]
 *   n_events rows of t, X, M, kind, Y_before and Y, >= 0 (0: every range is empty; t, X, M may be NULL)
 *   t        device float64 [n_events]; the times of a series need not ascend (a jump at t <= now takes
 *            no step)
 *   X, M     device fp32 [n_events][input_size] (M: masked models only, else NULL)
 *   kind     device int32 [n_events] or NULL (all 1).  1: an observation, exactly
 *            njode_online_observe_f32 at t[e].  0: an empty slice, exactly njode_online_advance_f32
 *            at t[e]; its rows of X / M are never read, and Y_before[e] and Y[e] both receive the
 *            readout of the state it arrives at (what njode_online_predict_f32 with Q = 1 at t[e]
 *            would have returned before the call).
 *   Y_before, Y   device fp32 [n_events][output_size], each may be NULL
 *   n_done   device int32 [n], every entry written: the events of the row that were applied
 * The result of a run on a series -- the state after it and every output row -- is, in bits, the
 * result of the same events fed one call at a time.  max_steps bounds the step loop in front of EACH
 * event's target.  A series the bound stops at its event k keeps the state it reached, applies no jump
 * at k and skips its remaining events: rows k .. end of its range of Y_before / Y are NaN, status 1,
 * n_done = k.  Otherwise status 0 and n_done = the length of the range.  An id outside the state:
 * status 2, n_done 0, nothing touched.  A range that does not satisfy
 * 0 <= ev_ptr[r] <= ev_ptr[r + 1] <= n_events: status 3, n_done 0; no event is read, nothing of the
 * state is touched and no output row written.  Every loop is counted: events by the checked range,
 * steps by max_steps.  NJODE_E_BADARG as for observe, and for a null ev_ptr or n_done, n_events < 0,
 * and n_events > 0 with a null t or X (masked: or M). */
int njode_online_run_f32(const NjodeDims* dims, const float* params, const NjodeOnlineState* state,
                         const int32_t* ids, int32_t n, const int32_t* ev_ptr, int32_t n_events,
                         const double* t, const float* X, const float* M, const int32_t* kind,
                         double delta_t, int32_t max_steps, float* Y_before, float* Y, int32_t* status,
                         int32_t* n_done, njodeStream_t stream);

/* ---- The same calls on the shape-generic matrix-core kernels --------------------------------------
 * For the models njode_online_supported refuses: any sizes within the envelope of njode_supported's
 * generic family, 0 .. NJODE_MAX_HIDDEN hidden layers, per-network descriptions (per_net = 1), tanh /
 * relu, every residual case, input_current_t, masked (input_size == output_size), unmasked with
 * output_size != input_size, and the GRU jump (use_rnn, 4 hidden_size <= 1024, masked or not; the
 * cell sees X as given).  The state is the same NjodeOnlineState: on a shape both families accept
 * it moves freely between them.  Semantics, status values, the clock and the bound are those
 * above, word for word; the results for a series are the bits njode_forward_f32 gives on the batch
 * of that series alone where that call runs the generic family.
 *
 * One workgroup per tile of `series_per_tile` listed series (0: the smallest power of two <= 16
 * with at most 256 tiles; else 1, 2, 4, 8 or 16).  A series' results do not depend on the tile
 * size, on its place in the tile or on the other series of the call.  No atomics.
 *
 * `tables`: device buffer of njode_online_tables_bytes() bytes, owned by the caller, filled by
 * njode_online_tables_f32 from `params` on the caller's stream and read by the four calls.  It
 * must be filled again whenever the parameters change.
 *
 * NJODE_E_BADARG -- before anything is launched -- for everything the entry points above refuse,
 * a null `tables`, tables_bytes below njode_online_tables_bytes() and a series_per_tile outside
 * {0, 1, 2, 4, 8, 16}; NJODE_E_UNSUPPORTED for a model njode_online_gen_supported refuses. */

/* 1 if the njode_online_gen_* entry points run this model, else 0; the reason, "online: ...", is
 * left in njode_last_error().  A pure host function. */
int njode_online_gen_supported(const NjodeDims* dims);

int njode_online_tables_bytes(const NjodeDims* dims, size_t* out);

int njode_online_tables_f32(const NjodeDims* dims, const float* params, void* tables, size_t tables_bytes,
                            njodeStream_t stream);

int njode_online_gen_reset_f32(const NjodeDims* dims, const float* params, const void* tables,
                               size_t tables_bytes, const NjodeOnlineState* state, const int32_t* ids,
                               int32_t n, const float* start_X, int32_t series_per_tile,
                               njodeStream_t stream);

int njode_online_gen_advance_f32(const NjodeDims* dims, const float* params, const void* tables,
                                 size_t tables_bytes, const NjodeOnlineState* state, const int32_t* ids,
                                 int32_t n, const double* t, double delta_t, int32_t max_steps,
                                 int32_t series_per_tile, int32_t* status, njodeStream_t stream);

int njode_online_gen_observe_f32(const NjodeDims* dims, const float* params, const void* tables,
                                 size_t tables_bytes, const NjodeOnlineState* state, const int32_t* ids,
                                 int32_t n, const double* t, const float* X, const float* M,
                                 double delta_t, int32_t max_steps, int32_t series_per_tile,
                                 float* Y_before, float* Y, int32_t* status, njodeStream_t stream);

int njode_online_gen_predict_f32(const NjodeDims* dims, const float* params, const void* tables,
                                 size_t tables_bytes, const NjodeOnlineState* state, const int32_t* ids,
                                 int32_t n, const double* t_query, int32_t Q, double delta_t,
                                 int32_t max_steps, int32_t series_per_tile, float* Y, int32_t* status,
                                 njodeStream_t stream);

/* njode_online_run_f32 on this family: a tile runs as many rounds as its longest range has events;
 * a chain whose range is exhausted idles. */
int njode_online_gen_run_f32(const NjodeDims* dims, const float* params, const void* tables,
                             size_t tables_bytes, const NjodeOnlineState* state, const int32_t* ids,
                             int32_t n, const int32_t* ev_ptr, int32_t n_events, const double* t,
                             const float* X, const float* M, const int32_t* kind, double delta_t,
                             int32_t max_steps, int32_t series_per_tile, float* Y_before, float* Y,
                             int32_t* status, int32_t* n_done, njodeStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NJODE_ONLINE_H */
