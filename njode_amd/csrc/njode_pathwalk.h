// njode_pathwalk.h -- what the routes that walk every path forwards and sweep it backwards into
// slabs share (the float64 route, njode_f64.hip; the GRU-ODE-Bayes baseline, njode_gob.hip): the
// row table, the transposed weight copy, the loss tree, the slab sum, and the refusals, slab count
// and workspace checks of their calls.  Both units link into one library: everything here has
// internal linkage.  The ProfScope label of a launch is its caller's.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "njode_hostlib.h"

namespace njode {
namespace {

// ---- row table: row_of[nt][B] = the observation row of (time slice, path), or -1 ----------------

__global__ void k_rows_clear(int* row_of, size_t n) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x)
    row_of[e] = -1;
}
__global__ void k_rows_fill(const int* __restrict__ obs_idx, const int* __restrict__ time_ptr, int n_obs,
                            int nt, int B, int* row_of) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_obs || nt <= 0) return;
  const int p = obs_idx[r];
  if (p < 0 || p >= B) return;
  int lo = 0, hi = nt - 1;   // the last slice whose first row is <= r
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (time_ptr[mid] <= r) lo = mid; else hi = mid - 1;
  }
  row_of[(size_t)lo * B + p] = r;
}
// (obs_idx, time_ptr: device arrays)
inline void build_row_table(int* row_of, const int* obs_idx, const int* time_ptr, int n_obs, int nt, int B,
                            const char* prof_name, hipStream_t st) {
  if (nt <= 0) return;
  ProfScope ps(prof_name, st);
  const size_t n = (size_t)nt * B;
  k_rows_clear<<<cdiv(n, 256) > 2048 ? 2048 : cdiv(n, 256), 256, 0, st>>>(row_of, n);
  if (n_obs > 0) k_rows_fill<<<cdiv(n_obs, 256), 256, 0, st>>>(obs_idx, time_ptr, n_obs, nt, B, row_of);
}

// ---- transposed weights: WT[i][j] = W[j][i] of every matrix of the table, at the matrix's own
// offset in the flat parameter vector (what lies between the matrices is not written)

constexpr int MAX_MATS = 3 * (NJODE_MAX_HIDDEN + 1);
struct MatTable {
  int n;
  int off[MAX_MATS], n_out[MAX_MATS], n_in[MAX_MATS];   // (n_out == 0: an empty entry)
  void add(int o, int rows, int cols) { off[n] = o; n_out[n] = rows; n_in[n] = cols; ++n; }
};
template <class T>
__global__ void k_transpose(const MatTable t, int P, const T* __restrict__ params, T* __restrict__ wt) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < P; e += gridDim.x * blockDim.x)
    for (int m = 0; m < t.n; ++m) {
      const int q = e - t.off[m];
      if (t.n_out[m] > 0 && q >= 0 && q < t.n_in[m] * t.n_out[m]) {
        const int j = q / t.n_in[m], i = q - j * t.n_in[m];
        wt[t.off[m] + (size_t)i * t.n_out[m] + j] = params[e];
      }
    }
}
template <class T>
inline void transpose_weights(const MatTable& t, int P, const T* params, T* wt, const char* prof_name,
                              hipStream_t st) {
  ProfScope ps(prof_name, st);
  k_transpose<T><<<cdiv(P, 256) > 1024 ? 1024 : cdiv(P, 256), 256, 0, st>>>(t, P, params, wt);
}

// ---- loss tree: out[c] = the sum of part[c * stride + p], p < B, for a workgroup of 256 threads --
// thread t adds its paths t, t + 256, ... in order, then a halving tree in LDS; every thread returns
// with the sums
template <int N>
__device__ inline void tree_sum_256(const double* __restrict__ part, int B, int stride, double out[N]) {
  __shared__ double red[N][256];
  double acc[N];
#pragma unroll
  for (int c = 0; c < N; ++c) acc[c] = 0.0;
  for (int p = threadIdx.x; p < B; p += 256) {
#pragma unroll
    for (int c = 0; c < N; ++c) acc[c] += part[(size_t)c * stride + p];
  }
#pragma unroll
  for (int c = 0; c < N; ++c) red[c][threadIdx.x] = acc[c];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int c = 0; c < N; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < N; ++c) out[c] = red[c][0];
}

// ---- gradient: the slabs summed in slab order, in double -------------------------------------------

template <class T>
__global__ void k_slab_reduce(const T* __restrict__ slabs, int S, int P, T* __restrict__ grad) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += (double)slabs[(size_t)s * P + e];
  grad[e] = (T)acc;
}
template <class T>
inline void reduce_slabs(const T* slabs, int S, int P, T* grad, const char* prof_name, hipStream_t st) {
  ProfScope ps(prof_name, st);
  k_slab_reduce<T><<<cdiv(P, 256), 256, 0, st>>>(slabs, S, P, grad);
}

// ---- host: sizes ----------------------------------------------------------------------------------------

// slabs of the sweep: as many as the budget holds, at most max_slabs, at most one per path, at least 1
inline int slab_count(size_t slab_bytes, size_t budget, int max_slabs, int B) {
  size_t s = budget / slab_bytes;
  if (s > (size_t)max_slabs) s = max_slabs;
  if (s > (size_t)B) s = B;
  return s < 1 ? 1 : (int)s;
}
// (an array of no elements still gets a slot of the workspace)
inline size_t at_least_1(int n) { return n > 0 ? n : 1; }

// ---- host: the refusals of a call, in the order the routes make them ------------------------------------
// Batch / Sched: NjodeBatch / NjodeSchedule or NjodeBatch64 / NjodeSchedule64 (same field names)

// the head of the list; bad_flag: the route's message for a call flag it does not take
template <class Batch, class Sched>
inline int check_sizes_and_params(const Batch* b, const Sched* s, int flags, int known_flags,
                                  const char* bad_flag, const void* params) {
  if (!b || !s) return fail(NJODE_E_BADARG, "null argument");
  if (flags & ~known_flags) return fail(NJODE_E_BADARG, "%s", bad_flag);
  if (b->batch_size <= 0 || b->n_obs < 0 || s->n_steps < 0 || s->n_times < 0)
    return fail(NJODE_E_BADARG, "negative size");
  if (!params) return fail(NJODE_E_BADARG, "null params");
  return NJODE_OK;
}
inline int check_workspace_ptr(const void* ws) {
  if (!ws || ((uintptr_t)ws & 255)) return fail(NJODE_E_BADARG, "workspace null or not aligned to 256 bytes");
  return NJODE_OK;
}
// the forward's walk over the host schedule: whatever the kernels index with
template <class Sched>
inline int check_schedule_walk(const Sched* s, int n_obs) {
  const int K = s->n_steps, nt = s->n_times;
  if ((K > 0 && (!s->step_dt || !s->step_t)) || (nt > 0 && (!s->k_jump || !s->time_f32)) || !s->time_ptr)
    return fail(NJODE_E_BADARG, "null schedule array");
  if (s->time_ptr[0] != 0 || s->time_ptr[nt] != n_obs) return fail(NJODE_E_BADARG, "time_ptr does not span the rows");
  int kprev = 0;
  for (int i = 0; i < nt; ++i) {
    if (s->time_ptr[i + 1] < s->time_ptr[i]) return fail(NJODE_E_BADARG, "time_ptr decreases");
    if (s->k_jump[i] < kprev || s->k_jump[i] > K) return fail(NJODE_E_BADARG, "k_jump out of order or range");
    kprev = s->k_jump[i];
  }
  return NJODE_OK;
}
inline int check_workspace_size(size_t ws_bytes, size_t total) {
  if (ws_bytes < total) return fail(NJODE_E_WORKSPACE, "workspace too small: %zu < %zu", ws_bytes, total);
  return NJODE_OK;
}

}  // namespace
}  // namespace njode
