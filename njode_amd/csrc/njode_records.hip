// njode_records.hip -- the record collate (include/njode_records.h): a batch of irregular,
// feature-masked records of an HBM-resident store becomes the CSR-by-time arrays of the masked
// NJ-ODE model, in the train and in the test layout of the reference's PhysioNet collate.
//
// Every call first scatters the batch's rows into a dense slot table int32 [G][B] in the
// caller's workspace (one wave per batch position walks its record; cell (g, b) has exactly one
// writer because a record's grid indices are strictly increasing), then one workgroup per grid
// index scans its B cells: counts them (phase 1), ranks them with the ballot scan of
// k_collate_fill (njode_producer.hip) and writes their rows (phase 2), or spreads them over the
// dense held-out arrays (phase 2b).  Byte / fp32 streaming work, no matrix cores, no atomics.
//
// The climate validation layout (njode_records_val_*) needs no table for its held-out part: a
// record's rows after the cut are contiguous in the store, so a binary search per batch position,
// an exact rank of the positions by (record, position) and a contiguous copy per position do it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/njode_records.h"
#include "njode_hostlib.h"

namespace {

using namespace njode;


constexpr int CB = 256;   // workgroup of every kernel here (4 waves)

// A cell of the slot table: SLOT_NONE, a kept row r as r >= 0, a dropped row r (all-zero mask
// in a store with drop_unobserved) as -2 - r.
constexpr int SLOT_NONE = -1;
__device__ __forceinline__ int slot_row(int cell) { return cell >= 0 ? cell : -2 - cell; }

__device__ __forceinline__ int block_sum(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// normalize_masked_data (utils_LODE.py:370-385): (v - att_min) / att_max with att_max == 0 taken
// as 1, then 0 where the mask is 0; without normalisation the raw value
__device__ __forceinline__ float norm_value(float v, uint8_t m, const float* __restrict__ att_min,
                                            const float* __restrict__ att_max, int j) {
  if (!att_min) return v;
  float mx = att_max[j];
  if (mx == 0.0f) mx = 1.0f;
  const float x = (v - att_min[j]) / mx;
  return m ? x : 0.0f;
}

__global__ void __launch_bounds__(CB) k_records_clear(int* __restrict__ table, long long n) {
  for (long long i = (long long)blockIdx.x * CB + threadIdx.x; i < n; i += (long long)gridDim.x * CB)
    table[i] = SLOT_NONE;
}

// wave w of the launch = batch position b: its record's rows go into column b of the table.
// n_obs_ot (phase 2 only): the kept rows of b with g in [g_lo, g_hi).
__global__ void __launch_bounds__(CB) k_records_scatter(NjodeRecordStore s,
                                                        const int* __restrict__ idx, int B,
                                                        int* __restrict__ table, int g_lo, int g_hi,
                                                        int* __restrict__ n_obs_ot) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (CB / 64) + (threadIdx.x >> 6);
  if (b >= B) return;   // wave-uniform
  const int n = idx[b];
  int r0 = 0, r1 = 0;
  if (n >= 0 && n < s.n_records) {
    r0 = max(s.row_ptr[n], 0);
    r1 = min(s.row_ptr[n + 1], s.n_rows);
  }
  int kept_in_range = 0;
  for (int r = r0 + lane; r < r1; r += 64) {
    const int g = s.row_g[r];
    if (g < 0 || g >= s.n_grid) continue;
    bool kept = true;
    if (s.drop_unobserved) {
      const uint8_t* m = s.mask + (size_t)r * s.dim;
      int any = 0;
      for (int j = 0; j < s.dim; ++j) any |= m[j];
      kept = any != 0;
    }
    table[(size_t)g * B + b] = kept ? r : -2 - r;
    kept_in_range += kept && g >= g_lo && g < g_hi;
  }
  if (n_obs_ot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept_in_range += __shfl_xor(kept_in_range, o);
    if (lane == 0) n_obs_ot[b] = kept_in_range;
  }
}

// block g: does the batch have a row at g, and how many of them are kept
__global__ void __launch_bounds__(CB) k_records_count(const int* __restrict__ table, int B,
                                                      int* __restrict__ present,
                                                      int* __restrict__ count) {
  __shared__ int sh[4];
  const int* row = table + (size_t)blockIdx.x * B;
  int any = 0, kept = 0;
  for (int b = threadIdx.x; b < B; b += CB) {
    const int c = row[b];
    any += c != SLOT_NONE;
    kept += c >= 0;
  }
  any = block_sum(any, sh);
  kept = block_sum(kept, sh);
  if (threadIdx.x == 0) {
    present[blockIdx.x] = any != 0;
    count[blockIdx.x] = kept;
  }
}

// block i writes the rows of grid index g = g_lo + i: base = rows of the earlier grid indices of
// the range, rank within g = number of earlier batch positions kept at g (ballot scan).  The
// ranked rows of a chunk of CB batch positions are parked in LDS and then written by the whole
// workgroup with unit stride along the features.
__global__ void __launch_bounds__(CB) k_records_fill(NjodeRecordStore s, int B,
                                                     const int* __restrict__ table,
                                                     const int* __restrict__ count, int g_lo,
                                                     int n_obs, float* __restrict__ X,
                                                     float* __restrict__ M,
                                                     int* __restrict__ obs_idx) {
  __shared__ int sh[4];
  __shared__ int wave_cnt[4];
  __shared__ int chunk_row[CB];
  const int g = g_lo + blockIdx.x;
  int before = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += CB) before += count[g_lo + i];
  int base = block_sum(before, sh);
  if (count[g] == 0) return;   // block-uniform
  const int* row = table + (size_t)g * B;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int D = s.dim;
  for (int b0 = 0; b0 < B; b0 += CB) {
    const int b = b0 + threadIdx.x;
    const int cell = b < B ? row[b] : SLOT_NONE;
    const bool on = cell >= 0 && cell < s.n_rows;
    const unsigned long long m = __ballot(on);
    __syncthreads();   // (the previous chunk's readers of chunk_row are done)
    if (lane == 0) wave_cnt[w] = __popcll(m);
    __syncthreads();
    int k = __popcll(m & ((1ull << lane) - 1ull));
    for (int i = 0; i < w; ++i) k += wave_cnt[i];
    const int n_chunk = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    if (on) {
      chunk_row[k] = cell;
      if ((unsigned)(base + k) < (unsigned)n_obs) obs_idx[base + k] = b;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n_chunk * D; e += CB) {
      const int q = e / D, j = e - q * D;
      const int out = base + q;
      if ((unsigned)out >= (unsigned)n_obs) continue;
      const size_t src = (size_t)chunk_row[q] * D + j;
      const uint8_t mk = s.mask[src];
      X[(size_t)out * D + j] = norm_value(s.vals[src], mk, s.att_min, s.att_max, j);
      M[(size_t)out * D + j] = mk ? 1.0f : 0.0f;
    }
    base += n_chunk;
  }
}

// block i handles grid index g = g_hi + i; if the batch has a row there it is held-out time
// v = number of present grid indices in [g_hi, g), and the block writes [b][v][:] for every b
__global__ void __launch_bounds__(CB) k_records_heldout(NjodeRecordStore s, int B,
                                                        const int* __restrict__ table,
                                                        const int* __restrict__ present, int g_hi,
                                                        int n_val, float* __restrict__ vals_val,
                                                        float* __restrict__ mask_val) {
  __shared__ int sh[4];
  const int g = g_hi + blockIdx.x;
  int before = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += CB) before += present[g_hi + i] != 0;
  const int v = block_sum(before, sh);
  if (present[g] == 0 || v >= n_val) return;   // block-uniform
  const int* row = table + (size_t)g * B;
  const int D = s.dim;
  for (int e = threadIdx.x; e < B * D; e += CB) {   // (B * D fits an int: check_call)
    const int b = e / D, j = e - b * D;
    const int cell = row[b];
    float x = 0.0f, mk = 0.0f;
    if (cell != SLOT_NONE) {
      const int r = slot_row(cell);
      if (r >= 0 && r < s.n_rows) {
        const size_t src = (size_t)r * D + j;
        const uint8_t m8 = s.mask[src];
        x = norm_value(s.vals[src], m8, s.att_min, s.att_max, j);
        mk = m8 ? 1.0f : 0.0f;
      }
    }
    const size_t dst = ((size_t)b * n_val + v) * D + j;
    vals_val[dst] = x;
    mask_val[dst] = mk;
  }
}

// ---- the climate validation layout: the rows after the cut, by (record, batch position, time) ----
// Workspace of the three kernels below: int32 [2][B], n_val[b] then first[b] (row of the store).

// thread b: a binary search in its record's strictly increasing row_g for the first row with
// row_g >= g_cut; it holds min(max_val, rows left) held-out rows.  31 halvings cover any range.
__global__ void __launch_bounds__(CB) k_records_val_search(NjodeRecordStore s,
                                                           const int* __restrict__ idx, int B,
                                                           int g_cut, int max_val,
                                                           int* __restrict__ n_val,
                                                           int* __restrict__ first) {
  const int b = blockIdx.x * CB + threadIdx.x;
  if (b >= B) return;
  const int n = idx[b];
  int r0 = 0, r1 = 0;
  if (n >= 0 && n < s.n_records) {
    r0 = min(max(s.row_ptr[n], 0), s.n_rows);
    r1 = max(min(s.row_ptr[n + 1], s.n_rows), r0);
  }
  int lo = r0, hi = r1;   // first row >= g_cut lies in [lo, hi]
  for (int it = 0; it < 31; ++it) {
    if (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (s.row_g[mid] < g_cut) lo = mid + 1; else hi = mid;
    }
  }
  n_val[b] = min(max_val, r1 - lo);
  first[b] = lo;
}

// thread b: val_ptr[b] = held-out rows of the batch positions that come before b in the order
// (record index, batch position) -- an exact count over all positions, staged through LDS in
// tiles of CB; integers only, so any B gives the same bits.  val_ptr[B] = all of them.
__global__ void __launch_bounds__(CB) k_records_val_rank(const int* __restrict__ idx, int B,
                                                         const int* __restrict__ n_val,
                                                         int* __restrict__ val_ptr) {
  __shared__ int sh_key[CB];
  __shared__ int sh_n[CB];
  const int b = blockIdx.x * CB + threadIdx.x;
  const int key = b < B ? idx[b] : 0;
  int before = 0, total = 0;
  for (int b0 = 0; b0 < B; b0 += CB) {   // (block-uniform bounds: the barriers are safe)
    const int o = b0 + threadIdx.x;
    __syncthreads();
    sh_key[threadIdx.x] = o < B ? idx[o] : 0;
    sh_n[threadIdx.x] = o < B ? n_val[o] : 0;
    __syncthreads();
    const int m = min(CB, B - b0);
    for (int i = 0; i < m; ++i) {
      const int k = sh_key[i], c = sh_n[i];
      total += c;
      before += (k < key || (k == key && b0 + i < b)) ? c : 0;
    }
  }
  if (b < B) val_ptr[b] = before;
  if (b == B - 1) val_ptr[B] = total;
}

// wave w of the launch = batch position b: its n_val[b] held-out rows are contiguous in the store
// (first[b] ...) and contiguous in the outputs (val_ptr[b] ...), so the wave copies n_val * D
// elements with unit stride on both sides.  L bounds every row written.
__global__ void __launch_bounds__(CB) k_records_val_fill(NjodeRecordStore s, int B,
                                                         const int* __restrict__ n_val,
                                                         const int* __restrict__ first,
                                                         const int* __restrict__ val_ptr, int L,
                                                         float* __restrict__ X_val,
                                                         float* __restrict__ M_val,
                                                         int* __restrict__ g_val,
                                                         int* __restrict__ index_val) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (CB / 64) + (threadIdx.x >> 6);
  if (b >= B) return;   // wave-uniform
  const int n = n_val[b], r0 = first[b], base = val_ptr[b];
  const int D = s.dim;
  if (n <= 0 || r0 < 0 || n > s.n_rows - r0) return;   // (rebuilt by this call: cannot happen)
  for (int q = lane; q < n; q += 64) {
    const int out = base + q;
    if ((unsigned)out >= (unsigned)L) continue;
    g_val[out] = s.row_g[r0 + q];
    index_val[out] = b;
  }
  const long long cells = (long long)n * D;
  for (long long e = lane; e < cells; e += 64) {
    const int q = (int)(e / D), j = (int)(e - (long long)q * D);
    const int out = base + q;
    if ((unsigned)out >= (unsigned)L) continue;
    const size_t src = (size_t)(r0 + q) * D + j;
    const uint8_t mk = s.mask[src];
    X_val[(size_t)out * D + j] = norm_value(s.vals[src], mk, s.att_min, s.att_max, j);
    M_val[(size_t)out * D + j] = mk ? 1.0f : 0.0f;
  }
}

size_t val_ws_bytes(int B) { return 2 * (size_t)B * sizeof(int32_t); }

// what the two validation entry points refuse about the store, the batch and the workspace
int check_val_call(const NjodeRecordStore* s, const int32_t* batch_idx, int32_t B, int32_t g_cut,
                   int32_t max_val, const int32_t* val_ptr, const void* ws, size_t ws_bytes) {
  if (!s) return fail(NJODE_E_BADARG, "null store");
  if (s->n_records <= 0 || s->n_rows <= 0 || s->dim <= 0 || s->n_grid <= 0)
    return fail(NJODE_E_BADARG, "n_records, n_rows, dim and n_grid must be positive");
  if (!s->row_ptr || !s->row_g || !s->vals || !s->mask)
    return fail(NJODE_E_BADARG, "null array in the store");
  if ((s->att_min == nullptr) != (s->att_max == nullptr))
    return fail(NJODE_E_BADARG, "att_min and att_max come together or not at all");
  if (s->drop_unobserved)
    return fail(NJODE_E_BADARG, "the validation layout belongs to a store that keeps every row "
                                "(drop_unobserved = 0)");
  if (!batch_idx || !val_ptr) return fail(NJODE_E_BADARG, "null batch_idx or val_ptr");
  if (B <= 0 || max_val <= 0) return fail(NJODE_E_BADARG, "B and max_val must be positive");
  if (g_cut < 0 || g_cut > s->n_grid)
    return fail(NJODE_E_BADARG, "g_cut %d outside [0, %d]", g_cut, s->n_grid);
  const int per = max_val < s->n_rows ? max_val : s->n_rows;
  if ((long long)B * per > 0x7fffffffLL)
    return fail(NJODE_E_BADARG, "B * min(max_val, n_rows) must fit 31 bits");
  const size_t need = val_ws_bytes(B);
  if (!ws || ws_bytes < need)
    return fail(NJODE_E_WORKSPACE, "workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0,
                need);
  return NJODE_OK;
}

size_t table_bytes(int G, int B) { return (size_t)G * (size_t)B * sizeof(int32_t); }

// what every entry point refuses about the store, the batch and the workspace
int check_call(const NjodeRecordStore* s, const int32_t* batch_idx, int32_t B, const void* ws,
               size_t ws_bytes) {
  if (!s) return fail(NJODE_E_BADARG, "null store");
  if (s->n_records <= 0 || s->n_rows <= 0 || s->dim <= 0 || s->n_grid <= 0)
    return fail(NJODE_E_BADARG, "n_records, n_rows, dim and n_grid must be positive");
  if (!s->row_ptr || !s->row_g || !s->vals || !s->mask)
    return fail(NJODE_E_BADARG, "null array in the store");
  if ((s->att_min == nullptr) != (s->att_max == nullptr))
    return fail(NJODE_E_BADARG, "att_min and att_max come together or not at all");
  if (!batch_idx) return fail(NJODE_E_BADARG, "null batch_idx");
  if (B <= 0) return fail(NJODE_E_BADARG, "B must be positive");
  if ((long long)B * s->dim > 0x7fffffffLL || (long long)B * s->n_grid > 0x7fffffffLL)
    return fail(NJODE_E_BADARG, "B * dim and B * n_grid must fit 31 bits");
  const size_t need = table_bytes(s->n_grid, B);
  if (!ws || ws_bytes < need)
    return fail(NJODE_E_WORKSPACE, "workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0,
                need);
  return NJODE_OK;
}

void build_table(const NjodeRecordStore* s, const int32_t* batch_idx, int32_t B, int* table,
                 int g_lo, int g_hi, int* n_obs_ot, hipStream_t st) {
  const long long cells = (long long)s->n_grid * B;
  const long long blocks = (cells + CB - 1) / CB;
  k_records_clear<<<(int)(blocks < 4096 ? blocks : 4096), CB, 0, st>>>(table, cells);
  k_records_scatter<<<cdiv(B, CB / 64), CB, 0, st>>>(*s, batch_idx, B, table, g_lo, g_hi, n_obs_ot);
}

}  // namespace

extern "C" int njode_records_bytes(int32_t n_grid, int32_t B, size_t* out) {
  if (!out) return fail(NJODE_E_BADARG, "null argument");
  if (n_grid <= 0 || B <= 0) return fail(NJODE_E_BADARG, "n_grid and B must be positive");
  *out = table_bytes(n_grid, B);
  return NJODE_OK;
}

extern "C" int njode_records_count(const NjodeRecordStore* store, const int32_t* batch_idx,
                                   int32_t B, int32_t* present, int32_t* count, void* ws,
                                   size_t ws_bytes, njodeStream_t stream) {
  if (const int rc = check_call(store, batch_idx, B, ws, ws_bytes)) return rc;
  if (!present || !count) return fail(NJODE_E_BADARG, "null output");
  hipStream_t st = (hipStream_t)stream;
  build_table(store, batch_idx, B, (int*)ws, 0, 0, nullptr, st);
  k_records_count<<<store->n_grid, CB, 0, st>>>((const int*)ws, B, present, count);
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}

extern "C" int njode_records_fill(const NjodeRecordStore* store, const int32_t* batch_idx,
                                  int32_t B, const int32_t* count, int32_t g_lo, int32_t g_hi,
                                  int32_t n_obs, float* X, float* M, int32_t* obs_idx,
                                  int32_t* n_obs_ot, void* ws, size_t ws_bytes,
                                  njodeStream_t stream) {
  if (const int rc = check_call(store, batch_idx, B, ws, ws_bytes)) return rc;
  if (!count || !n_obs_ot) return fail(NJODE_E_BADARG, "null argument");
  if (g_lo < 0 || g_lo > g_hi || g_hi > store->n_grid)
    return fail(NJODE_E_BADARG, "grid range [%d, %d) outside 0 <= g_lo <= g_hi <= %d", g_lo, g_hi,
                store->n_grid);
  if (n_obs < 0) return fail(NJODE_E_BADARG, "negative n_obs");
  if (n_obs > 0 && (!X || !M || !obs_idx)) return fail(NJODE_E_BADARG, "null output");
  hipStream_t st = (hipStream_t)stream;
  build_table(store, batch_idx, B, (int*)ws, g_lo, g_hi, n_obs_ot, st);
  if (n_obs > 0 && g_hi > g_lo)
    k_records_fill<<<g_hi - g_lo, CB, 0, st>>>(*store, B, (const int*)ws, count, g_lo, n_obs, X, M,
                                               obs_idx);
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}

extern "C" int njode_records_heldout(const NjodeRecordStore* store, const int32_t* batch_idx,
                                     int32_t B, const int32_t* present, int32_t g_hi,
                                     int32_t n_val, float* vals_val, float* mask_val, void* ws,
                                     size_t ws_bytes, njodeStream_t stream) {
  if (const int rc = check_call(store, batch_idx, B, ws, ws_bytes)) return rc;
  if (!present) return fail(NJODE_E_BADARG, "null argument");
  if (g_hi < 0 || g_hi > store->n_grid)
    return fail(NJODE_E_BADARG, "g_hi %d outside [0, %d]", g_hi, store->n_grid);
  if (n_val < 0) return fail(NJODE_E_BADARG, "negative n_val");
  if (n_val > 0 && (!vals_val || !mask_val)) return fail(NJODE_E_BADARG, "null output");
  if (n_val == 0 || g_hi == store->n_grid) return NJODE_OK;
  hipStream_t st = (hipStream_t)stream;
  build_table(store, batch_idx, B, (int*)ws, 0, 0, nullptr, st);
  k_records_heldout<<<store->n_grid - g_hi, CB, 0, st>>>(*store, B, (const int*)ws, present, g_hi,
                                                        n_val, vals_val, mask_val);
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}

extern "C" int njode_records_val_bytes(int32_t B, size_t* out) {
  if (!out) return fail(NJODE_E_BADARG, "null argument");
  if (B <= 0) return fail(NJODE_E_BADARG, "B must be positive");
  *out = val_ws_bytes(B);
  return NJODE_OK;
}

extern "C" int njode_records_val_count(const NjodeRecordStore* store, const int32_t* batch_idx,
                                       int32_t B, int32_t g_cut, int32_t max_val,
                                       int32_t* val_ptr, void* ws, size_t ws_bytes,
                                       njodeStream_t stream) {
  if (const int rc = check_val_call(store, batch_idx, B, g_cut, max_val, val_ptr, ws, ws_bytes))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  int* n_val = (int*)ws;
  k_records_val_search<<<cdiv(B, CB), CB, 0, st>>>(*store, batch_idx, B, g_cut, max_val, n_val,
                                                   n_val + B);
  k_records_val_rank<<<cdiv(B, CB), CB, 0, st>>>(batch_idx, B, n_val, val_ptr);
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}

extern "C" int njode_records_val_fill(const NjodeRecordStore* store, const int32_t* batch_idx,
                                      int32_t B, int32_t g_cut, int32_t max_val,
                                      const int32_t* val_ptr, int32_t L, float* X_val,
                                      float* M_val, int32_t* g_val, int32_t* index_val, void* ws,
                                      size_t ws_bytes, njodeStream_t stream) {
  if (const int rc = check_val_call(store, batch_idx, B, g_cut, max_val, val_ptr, ws, ws_bytes))
    return rc;
  if (L < 0) return fail(NJODE_E_BADARG, "negative L");
  if (L > 0 && (!X_val || !M_val || !g_val || !index_val))
    return fail(NJODE_E_BADARG, "null output");
  if (L == 0) return NJODE_OK;
  hipStream_t st = (hipStream_t)stream;
  int* n_val = (int*)ws;
  k_records_val_search<<<cdiv(B, CB), CB, 0, st>>>(*store, batch_idx, B, g_cut, max_val, n_val,
                                                   n_val + B);
  k_records_val_fill<<<cdiv(B, CB / 64), CB, 0, st>>>(*store, B, n_val, n_val + B, val_ptr, L,
                                                      X_val, M_val, g_val, index_val);
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}
