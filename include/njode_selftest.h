/*
 * njode_selftest.h -- test hooks of libnjode_hip.so (C ABI).  Not needed to use the library:
 * they expose device-side building blocks whose behaviour is pinned by tests
 * (tests/test_dropout_stream.py).
 */
#ifndef NJODE_SELFTEST_H
#define NJODE_SELFTEST_H

#include <stdint.h>

#include "njode_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The dropout keep-bit stream of the matrix-core kernels (njode_amd/csrc/njode_device.h:
 * drop_state; njode_mfma.h: keep_bits): for lane group g = 0..3 the first `n_words`
 * xorshift32 words of the stream keyed by (seed, global path id, time key, network id, g),
 * written to out_words[g * n_words + i] (device pointer, uint32).  The reference has no such
 * function (torch's nn.Dropout draws the masks, models.py:148-160); the stream is restated in
 * oracle/dropout_oracle.py and compared word for word.
 */
int njode_selftest_dropout_words(uint64_t seed, uint64_t path_id, uint32_t time_key, uint32_t net,
                                 int32_t n_words, uint32_t* out_words, void* stream);

/*
 * Maintainer aid of the one-launch plan (njode_amd/csrc/njode_plan.h), active with NJODE_PLAN_STAMPS=1
 * in the environment: the 100 MHz wall clock every plan block wrote at its stage ends during the LAST
 * plan launch on the current device.  out[block * 8 + slot]: slot 6 = entry, slots 0..5 = end of stage
 * 0..5.  Synchronises the device.  Returns the number of blocks copied (0: none / switched off).
 */
int njode_debug_plan_stamps(unsigned long long* out, int cap_blocks);

/*
 * Where the arrays of a plan sit in the buffer njode_plan_f32 fills, and which of them this call's
 * plan defines (tests/test_hip_plan_arrays.py compares exactly those with a host planner).  Launches
 * nothing and touches no buffer: the offsets are those of the layout and of the route the plan call
 * itself prepares from the same arguments.  Byte offsets into a buffer of `plan_bytes` bytes; -1: not
 * part of this plan.  All arrays are int32 except base_s / base16_s (int64).  A call without
 * NJODE_C_SCHED_KNOWN is viewed as one whose schedule ends at its last observation; NJODE_C_NEED_HT
 * and NJODE_C_PLAN_DEFER mean what they mean to njode_plan_f32.
 *
 * Which arrays a plan defines (n = n_obs, B = batch_size, K = n_steps; nothing but `sched` at n = 0):
 *   every plan         sched: step_dt[K] step_t[K] k_jump[n_times] time_f32[n_times] time_ptr[n_times + 1]
 *   compiled shapes    t_of_row[n], first_row[B], last_row[B], item_prev / _next / _kbeg / _len[n],
 *                      len_hist[K + 1];
 *     sort_linked      + path_sorted[n], row_by_path[n], first_j[B] (the lockstep plan, NJODE_PLAN=sort,
 *                      calls without a dense matrix); a dense plan defines none of the three
 *     seg, not         + order[n], base_s[K + 1], base16_s[K + 1]; with split_on and lds_cnt also the split
 *     links_only         points base_s[K + 1] (backward) and base_s[K + 2] (forward)
 *     tails            + t_order[B]
 *   generic family     jlo[K + 2]; on its segment plan (seg) also t_of_row, first_row, last_row, the four
 *                      item arrays, order, t_order and tile_base[n_tiles + 1]
 */
typedef struct NjodePlanView {
  int64_t plan_bytes;                                     /* = njode_plan_bytes of the same arguments */
  int64_t sched;
  int64_t t_of_row, first_row, last_row;
  int64_t item_prev, item_next, item_kbeg, item_len;
  int64_t order, t_order;
  int64_t len_hist, base_s, base16_s, path_sorted, row_by_path, first_j;   /* compiled shapes */
  int64_t jlo, tile_base;                                                  /* generic family */
  int32_t n_tiles;       /* generic family, segment plan: item tiles of 16 */
  int32_t generic;       /* the shape-generic kernels run this model */
  int32_t seg;           /* segment plan (else lockstep) */
  int32_t sort_linked;   /* rows linked through the (path, time) sort (else through the dense matrix) */
  int32_t links_only;    /* the one-launch plan stops behind the links (wave-per-item consumer) */
  int32_t tails;         /* the tail order is part of the plan */
  /* how the compiled shapes' plan is built in this process (the NJODE_PLAN_* switches applied) */
  int32_t one_launch;    /* k_plan_grid builds it: whole (plan_first_stage 0) or behind k_row_time (2) */
  int32_t plan_first_stage;
  int32_t plan_blocks;   /* blocks of that launch (a deferred plan: of its share of the hosting launch) */
  int32_t cs_shift, cs_nwb;   /* counting sort: 2^cs_shift rows per row block, cs_nwb row blocks (0: radix sort) */
  int32_t cs_large;      /* its count table sits in the key_sorted buffer (else in the small table) */
  int32_t scan_thread_per_key;   /* one launch: a thread scans each key's row of the table (else a wave) */
  int32_t lds_cnt;       /* the layout takes its workgroup scans (and finds split points) */
  int32_t tail_radix;    /* the tail order comes from the radix sort (else from k_tail_order) */
  int32_t split_on;      /* SplitCfg of the layout: on, ns[2], nw[2], r[2] -- [0] backward, [1] forward */
  int32_t split_ns[2], split_nw[2];
  float split_r[2];
} NjodePlanView;
int njode_debug_plan_view(const NjodeDims* dims, int32_t batch_size, int32_t n_obs, int32_t n_times,
                          int32_t n_steps, int32_t call_flags, NjodePlanView* out);

#ifdef __cplusplus
}
#endif
#endif
