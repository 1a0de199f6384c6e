// njode_protocol.hip -- the PhysioNet and climate evaluation protocols on the device
// (include/njode_protocol.h: njode_protocol_bytes / njode_protocol_rows / njode_protocol_score_f32;
// reference physionet_train.py:411-510, climate_train.py:508-566,
// data_utils_gru_ode_bayes.py:379-408, likelihood_eval_LODE.py:171-193).
//
// HBM-bound streaming work (no matrix cores): the held-out arrays are read once with unit stride,
// the prediction is gathered a row of `dim` floats at a time.  The dense layout runs one workgroup
// per (path, chunk of held-out times); its lanes are laid over (time, attribute) so that a lane
// keeps its attribute across strides, and the (path, chunk, attribute) partials wait in the
// workspace for a second, per-path pass.  This unit is compiled with -ffp-contract=off: the fp32
// terms are numpy's (subtract, square, multiply by the mask), no fused multiply-adds.
//
// Every result reaches memory through ordinary stores; sums are reduced in a fixed order (no
// float atomics), so two calls give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/njode_protocol.h"
#include "njode_hostlib.h"

namespace {

using namespace njode;

inline long long minl(long long a, long long b) { return a < b ? a : b; }
inline long long maxl(long long a, long long b) { return a > b ? a : b; }
inline size_t pad256(size_t v) { return (v + 255) / 256 * 256; }

constexpr int WB = 256;            // workgroup of the scoring kernels (4 waves)
constexpr int SUM_B = 1024;        // workgroup of the final reduction
constexpr int SLOTS_AIM = 1024;    // dense layout: workgroups to aim for when B alone is too few
constexpr int SPARSE_WG = 1024;    // sparse layout: at most this many workgroups

// How the dense layout is cut.  A attributes per pass over the lanes, G times per stride
// (A * G <= WB active lanes), n_chunks chunks of chunk_len times (a multiple of G but for the
// last chunk's remainder).
struct DensePlan {
  int A, G, chunk_len, n_chunks;
};

DensePlan dense_plan(long long T2, long long B, long long dim) {
  DensePlan p;
  p.A = (int)minl(dim, WB);
  p.G = WB / p.A;
  const long long most = cdiv(T2, p.G);                       // a chunk is at least one stride
  const long long nc = maxl(1, minl(most, cdiv(SLOTS_AIM, B)));
  p.chunk_len = (int)(cdiv(cdiv(T2, nc), p.G) * p.G);
  p.n_chunks = T2 > 0 ? cdiv(T2, p.chunk_len) : 0;
  return p;
}

// workspace of one call: what either layout may use of it
struct Layout {
  size_t part, attr_se, attr_cnt, path_mean, total;
};

Layout layout(long long n_query, long long B, long long dim) {
  // B * n_chunks <= min(B + SLOTS_AIM, B * max(1, ceil(T2 / G))): both non-decreasing in T2, B, dim
  const long long G = WB / minl(dim, WB);
  const long long slots = minl(B + SLOTS_AIM, B * maxl(1, cdiv(n_query, G)));
  const long long sparse = minl(cdiv(n_query * dim, WB), SPARSE_WG);
  Layout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += pad256(bytes); return at; };
  L.part = take((size_t)maxl(maxl(slots, sparse), 1) * 16);    // [slot] { sq, n_obs }
  L.attr_se = take((size_t)slots * dim * 8);                  // [slot][dim]
  L.attr_cnt = take((size_t)slots * dim * 4);                 // [slot][dim]
  L.path_mean = take((size_t)B * 8);                          // [B]
  L.total = o;
  return L;
}

const char* bad_sizes(long long n_rows, long long n_query, long long B, long long dim) {
  if (n_rows < 0 || n_query < 0 || B < 0 || dim < 0) return "sizes must not be negative";
  if (B == 0 || dim == 0) return "B and dim must be positive";
  if (B * dim > 0x7fffffffLL || n_query * dim > 0x7fffffffLL) return "B * dim and n_query * dim must fit int32";
  return nullptr;
}

// ---- rows ----------------------------------------------------------------------------------------
// One thread per query.  p is non-decreasing and a rounded difference is monotone in its operand,
// so each "first index with ..." below is a binary search over a monotone predicate.
__global__ void __launch_bounds__(256) k_protocol_rows(const double* __restrict__ p, int n,
                                                       const double* __restrict__ query, int nq,
                                                       int rule, int* __restrict__ rows) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const double t = query[q];
  int res;
  if (rule == NJODE_ROWS_CLOSEST) {
    // |p[i] - t| < 1e-10 holds on a run of rows: its first one is the first i with
    // p[i] - t > -1e-10, if that one is below +1e-10 as well
    int lo = 0, hi = n - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p[mid] - t > -1e-10) hi = mid; else lo = mid + 1;
    }
    const int near = lo;
    const bool has_near = near < n - 1 && fabs(p[near] - t) < 1e-10;
    // p[i] <= t < p[i + 1]: i + 1 is the first row beyond t
    lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int inside = lo - 1;
    const bool has_inside = lo >= 1 && lo <= n - 1;
    int i = -1;
    if (has_near) i = near;
    if (has_inside && (i < 0 || inside < i)) i = inside;
    if (i < 0) res = n - 1;
    else res = fabs(t - p[i]) <= fabs(t - p[i + 1]) ? i : i + 1;
  } else {
    int lo = 0, hi = n;          // first row at or beyond t
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p[mid] >= t) hi = mid; else lo = mid + 1;
    }
    const int lb = lo;
    if (lb == 0) {
      res = 0;
    } else {
      const double d_lo = fabs(p[lb - 1] - t);
      if (lb < n && !(d_lo <= fabs(p[lb] - t))) {
        res = lb;                // p[lb - 1] < t <= p[lb]: lb is the first row of its value
      } else {
        // the earlier value wins (ties included): the first row that is as near as it
        lo = 0, hi = lb - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (fabs(p[mid] - t) <= d_lo) hi = mid; else lo = mid + 1;
        }
        res = lo;
      }
    }
  }
  rows[q] = res;
}

// ---- scores ----------------------------------------------------------------------------------------
// the workgroup's { sq, n_obs }: xor tree inside the wave, then the four waves in turn
__device__ __forceinline__ void wg_sum2(double sq, double no, double* __restrict__ dst) {
  __shared__ double sh[2][WB / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sq = sq + __shfl_xor(sq, o);
    no = no + __shfl_xor(no, o);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = sq;
    sh[1][threadIdx.x >> 6] = no;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    dst[0] = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
    dst[1] = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
  }
}

// Dense layout.  Workgroup = (path b, chunk c); lane = g * A + a: time j0 + g, j0 + g + G, ... of
// the chunk, attribute a (+ A per pass where dim > WB).  With dim <= WB the A * G active lanes read
// G whole rows of vals / mask per stride, unit stride across the lanes.
__global__ void __launch_bounds__(WB) k_protocol_dense(const float* __restrict__ pred,
                                                       const int* __restrict__ rows,
                                                       const float* __restrict__ vals,
                                                       const float* __restrict__ mask, int n_rows,
                                                       int B, int dim, int T2, DensePlan pl,
                                                       double* __restrict__ part,
                                                       double* __restrict__ attr_se,
                                                       int* __restrict__ attr_cnt) {
  __shared__ double sh_se[WB];
  __shared__ int sh_cnt[WB];
  const int slot = blockIdx.x;
  const int b = slot / pl.n_chunks, c = slot % pl.n_chunks;
  const int j0 = c * pl.chunk_len;
  const int j1 = min(T2, j0 + pl.chunk_len);
  const int lane = threadIdx.x;
  const int g = lane / pl.A, a_in = lane % pl.A;
  const size_t BD = (size_t)B * dim;
  const float* __restrict__ pb = pred + (size_t)b * dim;
  const float* __restrict__ vb = vals + (size_t)b * T2 * dim;
  const float* __restrict__ mb = mask + (size_t)b * T2 * dim;
  double sq = 0.0, no = 0.0;
  for (int a0 = 0; a0 < dim; a0 += pl.A) {
    const int a = a0 + a_in;
    double se = 0.0;
    int cnt = 0;
    if (g < pl.G && a < dim) {
      for (int j = j0 + g; j < j1; j += pl.G) {
        const int r = rows[j];
        if ((unsigned)r >= (unsigned)n_rows) continue;
        const float pv = pb[(size_t)r * BD + a];
        const float v = vb[(size_t)j * dim + a];
        const float m = mb[(size_t)j * dim + a];
        const float d = pv - v;
        const float s = d * d;
        sq = sq + (double)(s * m);
        no = no + (double)m;
        if (m > 0.f) {
          const double e = (double)pv - (double)v;
          se = se + e * e;
          cnt += 1;
        }
      }
    }
    sh_se[lane] = se;
    sh_cnt[lane] = cnt;
    __syncthreads();
    if (lane < pl.A && a < dim) {       // the G lanes of attribute a, in order
      double s = sh_se[lane];
      int n = sh_cnt[lane];
      for (int gg = 1; gg < pl.G; ++gg) {
        s = s + sh_se[gg * pl.A + lane];
        n += sh_cnt[gg * pl.A + lane];
      }
      attr_se[(size_t)slot * dim + a] = s;
      attr_cnt[(size_t)slot * dim + a] = n;
    }
    __syncthreads();
  }
  wg_sum2(sq, no, part + 2 * (size_t)slot);
}

// Sparse layout: one thread per (held-out row, attribute), grid-stride over n_wg workgroups.
__global__ void __launch_bounds__(WB) k_protocol_sparse(const float* __restrict__ pred,
                                                        const int* __restrict__ rows,
                                                        const float* __restrict__ X_val,
                                                        const float* __restrict__ M_val,
                                                        const int* __restrict__ index_val,
                                                        int n_rows, int B, int dim, int L,
                                                        double* __restrict__ part) {
  const size_t BD = (size_t)B * dim;
  const long long total = (long long)L * dim;
  const long long stride = (long long)gridDim.x * WB;
  double sq = 0.0, no = 0.0;
  for (long long e = (long long)blockIdx.x * WB + threadIdx.x; e < total; e += stride) {
    const int l = (int)(e / dim), a = (int)(e % dim);
    const int r = rows[l], b = index_val[l];
    if ((unsigned)r >= (unsigned)n_rows || (unsigned)b >= (unsigned)B) continue;
    const float pv = pred[(size_t)r * BD + (size_t)b * dim + a];
    const float m = M_val[e];
    const float d = X_val[e] - pv;
    const float s = d * d;
    sq = sq + (double)(s * m);
    no = no + (double)m;
  }
  wg_sum2(sq, no, part + 2 * (size_t)blockIdx.x);
}

// path_mean[b] = mean over the attributes of (sum over the chunks of se) / (sum of cnt), 0 where
// nothing was observed; chunks in index order, attributes a, a + WB, ... per thread, then the tree
__global__ void __launch_bounds__(WB) k_protocol_attr(int dim, int n_chunks,
                                                      const double* __restrict__ attr_se,
                                                      const int* __restrict__ attr_cnt,
                                                      double* __restrict__ path_mean) {
  __shared__ double sh[WB / 64];
  const int b = blockIdx.x;
  double acc = 0.0;
  for (int a = threadIdx.x; a < dim; a += WB) {
    double s = 0.0;
    long long n = 0;
    for (int c = 0; c < n_chunks; ++c) {
      const size_t at = ((size_t)b * n_chunks + c) * dim + a;
      s = s + attr_se[at];
      n += attr_cnt[at];
    }
    acc = acc + (n > 0 ? s / (double)n : 0.0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) path_mean[b] = (((sh[0] + sh[1]) + sh[2]) + sh[3]) / (double)dim;
}

// sum of v[0], v[step], ...: strided partial sums per thread, then a tree through LDS (one
// workgroup, so the order is fixed); the result is valid in thread 0
__device__ __forceinline__ double wg_sum_strided(const double* __restrict__ v, long long n, int step,
                                                 double* sh) {
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += SUM_B) s = s + v[i * step];
  __syncthreads();      // sh may still be read by the previous sum
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = SUM_B / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

// out = { sq_sum, n_obs, attr_mse, 0 } of this call, or added to what out holds
__global__ void __launch_bounds__(SUM_B) k_protocol_final(const double* __restrict__ part,
                                                          long long n_part,
                                                          const double* __restrict__ path_mean,
                                                          int n_paths, int accumulate,
                                                          double* __restrict__ out) {
  __shared__ double sh[SUM_B];
  const double sq = wg_sum_strided(part, n_part, 2, sh);
  const double no = wg_sum_strided(part + 1, n_part, 2, sh);
  double attr = 0.0;
  if (n_paths > 0) attr = wg_sum_strided(path_mean, n_paths, 1, sh) / (double)n_paths;
  if (threadIdx.x == 0) {
    if (accumulate) {
      out[0] = out[0] + sq;
      out[1] = out[1] + no;
      out[2] = out[2] + attr;
    } else {
      out[0] = sq;
      out[1] = no;
      out[2] = attr;
    }
    out[3] = 0.0;
  }
}

}  // namespace

extern "C" int njode_protocol_bytes(int32_t n_rows, int32_t n_query, int32_t B, int32_t dim,
                                    size_t* bytes) {
  if (!bytes) return fail(NJODE_E_BADARG, "null argument");
  if (const char* why = bad_sizes(n_rows, n_query, B, dim)) return fail(NJODE_E_BADARG, "%s", why);
  *bytes = layout(n_query, B, dim).total;
  return NJODE_OK;
}

extern "C" int njode_protocol_rows(const double* path_t, int32_t n_rows, const double* query,
                                   int32_t n_query, int32_t rule, int32_t* rows,
                                   njodeStream_t stream) {
  if (!path_t || !query || !rows) return fail(NJODE_E_BADARG, "null argument");
  if (n_rows < 1 || n_query < 0) return fail(NJODE_E_BADARG, "n_rows must be positive, n_query not negative");
  if (rule != NJODE_ROWS_CLOSEST && rule != NJODE_ROWS_FIRST_NEAREST)
    return fail(NJODE_E_BADARG, "unknown row rule %d", rule);
  if (n_query == 0) return NJODE_OK;
  hipStream_t st = (hipStream_t)stream;
  k_protocol_rows<<<cdiv(n_query, 256), 256, 0, st>>>(path_t, n_rows, query, n_query, rule, rows);
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}

extern "C" int njode_protocol_score_f32(const NjodeProtocolJob* job, double* out, int32_t accumulate,
                                        void* ws, size_t ws_bytes, njodeStream_t stream) {
  if (!job || !out) return fail(NJODE_E_BADARG, "null argument");
  if (const char* why = bad_sizes(job->n_rows, job->n_query, job->B, job->dim))
    return fail(NJODE_E_BADARG, "%s", why);
  const bool dense = job->vals || job->mask;
  const bool sparse = job->X_val || job->M_val || job->index_val;
  if (dense == sparse) return fail(NJODE_E_BADARG, "exactly one target layout: vals / mask or X_val / M_val / index_val");
  if (dense ? (!job->vals || !job->mask) : (!job->X_val || !job->M_val || !job->index_val))
    return fail(NJODE_E_BADARG, "half a target layout");
  const int nq = job->n_query, B = job->B, dim = job->dim;
  if (!job->pred || (nq > 0 && !job->rows)) return fail(NJODE_E_BADARG, "null pred or rows");
  if (nq > 0 && job->n_rows < 1) return fail(NJODE_E_BADARG, "held-out entries but no row to score them at");
  const Layout L = layout(nq, B, dim);
  if (!ws) return fail(NJODE_E_BADARG, "null workspace");
  if (ws_bytes < L.total)
    return fail(NJODE_E_WORKSPACE, "workspace of %zu bytes, %zu needed", ws_bytes, L.total);

  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  double* part = (double*)(w + L.part);
  double* path_mean = (double*)(w + L.path_mean);
  long long n_part = 0;
  if (dense) {
    const DensePlan pl = dense_plan(nq, B, dim);
    double* attr_se = (double*)(w + L.attr_se);
    int* attr_cnt = (int*)(w + L.attr_cnt);
    n_part = (long long)B * pl.n_chunks;
    if (n_part > 0) {
      ProfScope ps("k_protocol_dense", st);
      k_protocol_dense<<<(int)n_part, WB, 0, st>>>(job->pred, job->rows, job->vals, job->mask,
                                                   job->n_rows, B, dim, nq, pl, part, attr_se, attr_cnt);
    }
    k_protocol_attr<<<B, WB, 0, st>>>(dim, pl.n_chunks, attr_se, attr_cnt, path_mean);
  } else {
    n_part = minl(cdiv((long long)nq * dim, WB), SPARSE_WG);
    if (n_part > 0) {
      ProfScope ps("k_protocol_sparse", st);
      k_protocol_sparse<<<(int)n_part, WB, 0, st>>>(job->pred, job->rows, job->X_val, job->M_val,
                                                    job->index_val, job->n_rows, B, dim, nq, part);
    }
  }
  k_protocol_final<<<1, SUM_B, 0, st>>>(part, n_part, path_mean, dense ? B : 0, accumulate != 0, out);
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}
