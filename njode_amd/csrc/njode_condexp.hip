// njode_condexp.hip -- the analytic conditional expectation of the synthetic SDEs along a batch's
// observation schedule and the evaluation metrics taken against it (include/njode_producer.h:
// njode_cond_exp_bytes / njode_cond_exp_f64 and their staged siblings for regime-switch datasets;
// reference stock_model.py:50-158, 178, 277-286, 353, 393, 421-466, 471-481).
//
// HBM-bound float64 streaming work (no matrix cores).  The Euler factors depend on the step
// only, so a small kernel evaluates exp / sin once per call into a table [K]; one thread per
// (path, dim) then walks the rows [start | one per Euler step | one per jump] with y * a + c per
// step.  Nothing a thread loads depends on its y, so every load of a group of ROWS_AHEAD rows is
// issued before the group's serial multiply chain.  This unit is compiled with -ffp-contract=off:
// the host's float64 expression trees, no fused multiply-adds.
//
// Every result reaches memory through ordinary stores; sums are reduced in a fixed order (no
// float atomics), so two calls give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/njode_producer.h"
#include "njode_hostlib.h"

namespace {

using namespace njode;

inline size_t pad256(size_t v) { return (v + 255) / 256 * 256; }

constexpr int WB = 256;          // workgroup of the walk (4 waves)
constexpr int ROWS_AHEAD = 8;    // rows whose loads are in flight ahead of the multiply chain
constexpr int SUM_B = 1024;      // workgroup of the final reduction

// workspace of one call
struct Layout {
  size_t a, c, step_dt, step_t, k_jump, time_ptr, desc, dense, sq_rows, terms, partials, total;
  size_t a1, c1;   // staged calls: the factors of coordinate class 1
  long long n_rows, n_blocks;
};

Layout layout(long long B, long long n_obs, long long nt, long long K, long long dim,
              bool staged = false) {
  Layout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += pad256(bytes); return at; };
  L.n_rows = 1 + K + nt;
  L.n_blocks = cdiv(B * dim, WB);
  L.step_dt = take((size_t)K * 8);
  L.step_t = take((size_t)K * 8);
  L.a = take((size_t)K * 8);
  L.c = take((size_t)K * 8);
  L.k_jump = take((size_t)nt * 4);
  L.time_ptr = take((size_t)(nt + 1) * 4);
  L.desc = take((size_t)L.n_rows * 4);
  L.dense = take((size_t)nt * B * 4);
  L.sq_rows = take((size_t)n_obs * dim * 8);
  L.terms = take((size_t)n_obs * 8);
  L.partials = take((size_t)L.n_blocks * 8);
  L.a1 = L.c1 = 0;
  if (staged) {
    L.a1 = take((size_t)K * 8);
    L.c1 = take((size_t)K * 8);
  }
  L.total = o;
  return L;
}

// ---- per-call tables --------------------------------------------------------------------
// Thread k < K: the factors of Euler step k and its row; thread K + i: the row of jump i.
// desc[row] = k for the row written after step k, -(i + 1) for the row of jump i.  Rows follow
// Schedule.path_t: step k comes after every jump whose k_jump <= k.
// row of Euler step t: it comes after every jump whose k_jump <= t
__device__ __forceinline__ int step_row(int t, int nt, const int* __restrict__ k_jump) {
  int lo = 0, hi = nt;     // number of jumps with k_jump <= t
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (k_jump[mid] <= t) lo = mid + 1; else hi = mid;
  }
  return 1 + t + lo;
}

// what the staged table reads of a stage
struct StageP {
  int model, has_sine, return_vol, first_step;
  double drift, mean, speed, sine_coeff;
};
struct Stages {
  int n;
  StageP s[NJODE_MAX_STAGES];
};

// k_cond_exp_table for a chain of stages: step t takes the stage with the largest first_step <= t
// (binary search); class 0 factors into a / c, the variance class of a return_vol stage into
// a1 / c1 (stock_model.py:281-282: no periodic coefficient)
__global__ void __launch_bounds__(256) k_cond_exp_table_staged(Stages sg, int K, int nt,
                                                               const double* __restrict__ step_dt,
                                                               const double* __restrict__ step_t,
                                                               const int* __restrict__ k_jump,
                                                               double* __restrict__ a,
                                                               double* __restrict__ c,
                                                               double* __restrict__ a1,
                                                               double* __restrict__ c1,
                                                               int* __restrict__ desc) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) desc[0] = 0;
  if (t < K) {
    int lo = 0, hi = sg.n;   // number of stages with first_step <= t (at least one: the first is 0)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sg.s[mid].first_step <= t) lo = mid + 1; else hi = mid;
    }
    const StageP& p = sg.s[lo - 1];
    const double step = step_dt[t], now = step_t[t];
    const double rate = p.model == NJODE_SDE_ORNSTEIN_UHLENBECK ? -p.speed : p.drift;
    const double rp = p.has_sine ? rate * (1.0 + sin(p.sine_coeff * now)) : rate;
    const double f = exp(rp * step);
    a[t] = f;
    c[t] = p.model == NJODE_SDE_ORNSTEIN_UHLENBECK ? p.mean * (1.0 - f) : 0.0;
    if (p.return_vol) {
      const double e = exp(-p.speed * step);
      a1[t] = e;
      c1[t] = p.mean * (1.0 - e);
    }
    desc[step_row(t, nt, k_jump)] = t;
  } else if (t < K + nt) {
    const int i = t - K;
    desc[1 + k_jump[i] + i] = -(i + 1);
  }
}

__global__ void __launch_bounds__(256) k_cond_exp_table(NjodeSde p, int K, int nt,
                                                        const double* __restrict__ step_dt,
                                                        const double* __restrict__ step_t,
                                                        const int* __restrict__ k_jump,
                                                        double* __restrict__ a,
                                                        double* __restrict__ c,
                                                        int* __restrict__ desc) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) desc[0] = 0;   // the start row (never read as a step)
  if (t < K) {
    const double step = step_dt[t], now = step_t[t];
    // stock_model.py:353 / :393 / :178: (rate * periodic_coeff(t)) * delta_t, the coefficient the
    // int 1 without a sine term
    const double rate = p.model == NJODE_SDE_ORNSTEIN_UHLENBECK ? -p.speed : p.drift;
    const double rp = p.has_sine ? rate * (1.0 + sin(p.sine_coeff * now)) : rate;
    const double f = exp(rp * step);
    a[t] = f;
    c[t] = p.model == NJODE_SDE_ORNSTEIN_UHLENBECK ? p.mean * (1.0 - f) : 0.0;
    int lo = 0, hi = nt;     // number of jumps with k_jump <= t
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (k_jump[mid] <= t) lo = mid + 1; else hi = mid;
    }
    desc[1 + t + lo] = t;
  } else if (t < K + nt) {
    const int i = t - K;
    desc[1 + k_jump[i] + i] = -(i + 1);
  }
}

// dense[i][b] = row of path b in time slice i (-1: none); one thread per row, the slice by
// binary search in time_ptr (empty slices are stepped over)
__global__ void __launch_bounds__(256) k_cond_exp_rows(const int* __restrict__ time_ptr, int nt,
                                                       int n_obs, const int* __restrict__ obs_idx,
                                                       int B, int* __restrict__ dense) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_obs) return;
  int lo = 0, hi = nt;       // first slice whose end is beyond r
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (time_ptr[mid + 1] <= r) lo = mid + 1; else hi = mid;
  }
  const int b = obs_idx[r];
  if (lo < nt && (unsigned)b < (unsigned)B) dense[(size_t)lo * B + b] = r;
}

// ---- the walk ------------------------------------------------------------------------------
// Thread tid = b * dim + j.  Rows are taken in groups of ROWS_AHEAD: first every load of the
// group (the prediction, the dense table and through it the observation -- none depends on y),
// then the serial chain.  desc / a / c are wave-uniform.  MODE 0: y * a; 1: y * a + c; 2 (a
// return_vol stage): the spot coordinates j < dim / 2 take y * a, the variance coordinates
// y * a1 + c1.
template <int MODE, bool PATH, bool LOSS, bool METRIC>
__global__ void __launch_bounds__(WB) k_cond_exp_walk(int B, int dim, int n_rows,
                                                      const float* __restrict__ start_X,
                                                      const float* __restrict__ X,
                                                      const int* __restrict__ desc,
                                                      const int* __restrict__ dense,
                                                      const double* __restrict__ a,
                                                      const double* __restrict__ c,
                                                      const double* __restrict__ a1,
                                                      const double* __restrict__ c1,
                                                      const float* __restrict__ pred,
                                                      double* __restrict__ path_y,
                                                      double* __restrict__ sq_rows,
                                                      double* __restrict__ partials) {
  __shared__ double sh[WB / 64];
  const long long BD = (long long)B * dim;
  const long long tid = (long long)blockIdx.x * WB + threadIdx.x;
  const bool live = tid < BD;
  double acc = 0.0;
  if (live) {
    const int b = (int)(tid / dim), j = (int)(tid % dim);
    double y = (double)start_X[tid];
    const bool vol = MODE == 2 && j >= dim / 2;
    const double* fa_of = vol ? a1 : a;
    const double* fc_of = vol ? c1 : c;
    if (PATH) path_y[tid] = y;
    if (METRIC) {
      const double e = (double)pred[tid] - y;
      acc = e * e;
    }
    for (int r0 = 1; r0 < n_rows; r0 += ROWS_AHEAD) {
      int dsc[ROWS_AHEAD], row[ROWS_AHEAD];
      float xo[ROWS_AHEAD], pr[ROWS_AHEAD];
      double fa[ROWS_AHEAD], fc[ROWS_AHEAD];
#pragma unroll
      for (int u = 0; u < ROWS_AHEAD; ++u) {
        const int r = r0 + u;
        dsc[u] = r < n_rows ? desc[r] : -1;
        row[u] = -1;
        fa[u] = 1.0;
        fc[u] = 0.0;
        if (r < n_rows && dsc[u] < 0) row[u] = dense[(size_t)(-dsc[u] - 1) * B + b];
        if (r < n_rows && dsc[u] >= 0) {
          fa[u] = fa_of[dsc[u]];
          if (MODE == 1 || vol) fc[u] = fc_of[dsc[u]];
        }
        if (METRIC) pr[u] = r < n_rows ? pred[(size_t)r * BD + tid] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < ROWS_AHEAD; ++u) xo[u] = row[u] >= 0 ? X[(size_t)row[u] * dim + j] : 0.f;
#pragma unroll
      for (int u = 0; u < ROWS_AHEAD; ++u) {
        const int r = r0 + u;
        if (r < n_rows) {
          if (dsc[u] >= 0) {
            y = (MODE == 1 || vol) ? y * fa[u] + fc[u] : y * fa[u];
          } else if (row[u] >= 0) {
            const double x = (double)xo[u];
            if (LOSS) {
              const double e = y - x;              // the value before the jump
              sq_rows[(size_t)row[u] * dim + j] = e * e;
            }
            y = x;
          }
          if (PATH) path_y[(size_t)r * BD + tid] = y;
          if (METRIC) {
            const double e = (double)pr[u] - y;
            acc = acc + e * e;
          }
        }
      }
    }
  }
  if (METRIC) {
    // fixed order: xor tree inside the wave, then the four waves in turn
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  }
}

// term of row r: (2 w sqrt(eps) + 2 (1 - w) sqrt(sum_d (y_bj - X)^2 + eps))^2 / n_obs_ot[b]
// (stock_model.py:471-481; the distance after the jump is exactly 0)
__global__ void __launch_bounds__(256) k_cond_exp_terms(int n_obs, int dim, int B,
                                                        const double* __restrict__ sq_rows,
                                                        const int* __restrict__ obs_idx,
                                                        const int* __restrict__ n_obs_ot,
                                                        double w2_after, double w2_before,
                                                        double eps, double* __restrict__ terms) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_obs) return;
  const int b = obs_idx[r];
  if ((unsigned)b >= (unsigned)B) {   // no path walked this row: it carries no term
    terms[r] = 0.0;
    return;
  }
  double s = 0.0;
  for (int j = 0; j < dim; ++j) s = s + sq_rows[(size_t)r * dim + j];
  const double inner = w2_after + w2_before * sqrt(s + eps);
  terms[r] = (inner * inner) / (double)n_obs_ot[b];
}

// out[0] = (sum of v[0..n)) / div: strided partial sums per thread, then a tree through LDS --
// one workgroup, so the order is fixed
__global__ void __launch_bounds__(SUM_B) k_cond_exp_sum(const double* __restrict__ v, long long n,
                                                        double div, double* __restrict__ out) {
  __shared__ double sh[SUM_B];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += SUM_B) s = s + v[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = SUM_B / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0] / div;
}

template <int MODE>
void launch_walk(bool path, bool loss, bool metric, int grid, hipStream_t st, int B, int dim,
                 int n_rows, const float* start_X, const float* X, const int* desc,
                 const int* dense, const double* a, const double* c, const double* a1,
                 const double* c1, const float* pred, double* path_y, double* sq_rows,
                 double* partials) {
#define NJ_WALK(P, L, M)                                                                       \
  k_cond_exp_walk<MODE, P, L, M><<<grid, WB, 0, st>>>(B, dim, n_rows, start_X, X, desc, dense, \
                                                       a, c, a1, c1, pred, path_y, sq_rows,    \
                                                       partials)
  const int sel = (path ? 4 : 0) | (loss ? 2 : 0) | (metric ? 1 : 0);
  switch (sel) {
    case 1: NJ_WALK(false, false, true); break;
    case 2: NJ_WALK(false, true, false); break;
    case 3: NJ_WALK(false, true, true); break;
    case 4: NJ_WALK(true, false, false); break;
    case 5: NJ_WALK(true, false, true); break;
    case 6: NJ_WALK(true, true, false); break;
    case 7: NJ_WALK(true, true, true); break;
    default: break;
  }
#undef NJ_WALK
}

// what both entry points refuse about the sizes
const char* bad_sizes(long long B, long long n_obs, long long nt, long long K, long long dim) {
  if (B <= 0 || dim <= 0) return "batch_size and dim must be positive";
  if (n_obs < 0 || nt < 0 || K < 0) return "n_obs, n_times and n_steps must not be negative";
  if (B * dim > 0x7fffffffLL || n_obs * dim > 0x7fffffffLL || 1 + K + nt > 0x7fffffffLL)
    return "batch_size * dim, n_obs * dim and the row count must fit int32";
  return nullptr;
}


// Both entry points after their own checks of the model(s): the rest of the refusals, then the
// launches.  sg == nullptr: the single model `sde`; else the chain of stages.
int cond_exp_run(const NjodeSde* sde, const Stages* sg, int dim, int mode, const NjodeBatch* batch,
                 const NjodeCondExpSchedule* sched, double weight, const float* pred,
                 double* path_y, double* opt_loss, double* sq_diff, void* ws, size_t ws_bytes,
                 njodeStream_t stream) {
  const int B = batch->batch_size, n_obs = batch->n_obs;
  const int K = sched->n_steps, nt = sched->n_times;
  if (!path_y && !opt_loss && !sq_diff) return fail(NJODE_E_BADARG, "no output asked for");
  if (sq_diff && !pred) return fail(NJODE_E_BADARG, "sq_diff needs pred");
  if (opt_loss && !batch->n_obs_ot) return fail(NJODE_E_BADARG, "opt_loss needs n_obs_ot");
  if (batch->M) return fail(NJODE_E_BADARG, "masked batches have no analytic conditional expectation");
  if (!batch->start_X || (n_obs > 0 && (!batch->X || !batch->obs_idx)))
    return fail(NJODE_E_BADARG, "null batch array");
  if ((K > 0 && (!sched->step_dt || !sched->step_t)) || (nt > 0 && !sched->k_jump) || !sched->time_ptr)
    return fail(NJODE_E_BADARG, "null schedule array");
  // the schedule is on the host: whatever the kernels index with is checked here
  if (sched->time_ptr[0] != 0 || sched->time_ptr[nt] != n_obs)
    return fail(NJODE_E_BADARG, "time_ptr must run from 0 to n_obs");
  for (int i = 0; i < nt; ++i) {
    if (sched->time_ptr[i + 1] < sched->time_ptr[i]) return fail(NJODE_E_BADARG, "time_ptr decreases");
    if (sched->k_jump[i] < (i ? sched->k_jump[i - 1] : 0) || sched->k_jump[i] > K)
      return fail(NJODE_E_BADARG, "k_jump must be non-decreasing within [0, n_steps]");
  }
  if (sg)
    for (int i = 0; i < sg->n; ++i)
      if (sg->s[i].first_step > K)
        return fail(NJODE_E_BADARG, "stage %d starts at step %d of %d", i, sg->s[i].first_step, K);
  const Layout L = layout(B, n_obs, nt, K, dim, sg != nullptr);
  if (!ws) return fail(NJODE_E_BADARG, "null workspace");
  if (ws_bytes < L.total)
    return fail(NJODE_E_WORKSPACE, "workspace of %zu bytes, %zu needed", ws_bytes, L.total);

  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  double *a = (double*)(w + L.a), *c = (double*)(w + L.c);
  double *a1 = (double*)(w + L.a1), *c1 = (double*)(w + L.c1);
  double *d_dt = (double*)(w + L.step_dt), *d_t = (double*)(w + L.step_t);
  int *d_kj = (int*)(w + L.k_jump), *d_tp = (int*)(w + L.time_ptr);
  int *desc = (int*)(w + L.desc), *dense = (int*)(w + L.dense);
  double *sq_rows = (double*)(w + L.sq_rows), *terms = (double*)(w + L.terms);
  double* partials = (double*)(w + L.partials);
  if (K > 0) {
    HIP_TRY(hipMemcpyAsync(d_dt, sched->step_dt, (size_t)K * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_t, sched->step_t, (size_t)K * 8, hipMemcpyHostToDevice, st));
  }
  if (nt > 0) HIP_TRY(hipMemcpyAsync(d_kj, sched->k_jump, (size_t)nt * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_tp, sched->time_ptr, (size_t)(nt + 1) * 4, hipMemcpyHostToDevice, st));
  if (nt > 0) HIP_TRY(hipMemsetAsync(dense, 0xFF, (size_t)nt * B * 4, st));
  const int table_grid = cdiv(K + nt > 0 ? K + nt : 1, 256);
  if (sg)
    k_cond_exp_table_staged<<<table_grid, 256, 0, st>>>(*sg, K, nt, d_dt, d_t, d_kj, a, c, a1, c1, desc);
  else
    k_cond_exp_table<<<table_grid, 256, 0, st>>>(*sde, K, nt, d_dt, d_t, d_kj, a, c, desc);
  if (n_obs > 0)
    k_cond_exp_rows<<<cdiv(n_obs, 256), 256, 0, st>>>(d_tp, nt, n_obs, batch->obs_idx, B, dense);
  const bool want_loss = opt_loss && n_obs > 0;
  // (a row no path walks -- obs_idx outside the batch -- must not leave its squares unwritten)
  if (want_loss) HIP_TRY(hipMemsetAsync(sq_rows, 0, (size_t)n_obs * dim * 8, st));
  {
    ProfScope ps("k_cond_exp_walk", st);
#define NJ_MODE(M)                                                                                  \
  launch_walk<M>(path_y != nullptr, want_loss, sq_diff != nullptr, (int)L.n_blocks, st, B, dim,      \
                 (int)L.n_rows, batch->start_X, batch->X, desc, dense, a, c, a1, c1, pred, path_y,   \
                 sq_rows, partials)
    if (mode == 2) NJ_MODE(2);
    else if (mode == 1) NJ_MODE(1);
    else NJ_MODE(0);
#undef NJ_MODE
  }
  if (opt_loss) {
    if (n_obs > 0) {
      const double eps = 1e-10;
      const double after = __builtin_sqrt(0.0 + eps);
      k_cond_exp_terms<<<cdiv(n_obs, 256), 256, 0, st>>>(
          n_obs, dim, B, sq_rows, batch->obs_idx, batch->n_obs_ot, 2 * weight * after,
          2 * (1 - weight), eps, terms);
    }
    k_cond_exp_sum<<<1, SUM_B, 0, st>>>(terms, n_obs, (double)B, opt_loss);
  }
  if (sq_diff) k_cond_exp_sum<<<1, SUM_B, 0, st>>>(partials, L.n_blocks, 1.0, sq_diff);
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}

}  // namespace

extern "C" int njode_cond_exp_bytes(int32_t B, int32_t n_obs, int32_t n_times, int32_t n_steps,
                                    int32_t dim, size_t* out) {
  if (!out) return fail(NJODE_E_BADARG, "null argument");
  if (const char* why = bad_sizes(B, n_obs, n_times, n_steps, dim)) return fail(NJODE_E_BADARG, "%s", why);
  *out = layout(B, n_obs, n_times, n_steps, dim).total;
  return NJODE_OK;
}

extern "C" int njode_cond_exp_f64(const NjodeSde* sde, const NjodeBatch* batch,
                                  const NjodeCondExpSchedule* sched, double weight,
                                  const float* pred, double* path_y, double* opt_loss,
                                  double* sq_diff, void* ws, size_t ws_bytes,
                                  njodeStream_t stream) {
  if (!sde || !batch || !sched) return fail(NJODE_E_BADARG, "null argument");
  if (const char* why = bad_sizes(batch->batch_size, batch->n_obs, sched->n_times, sched->n_steps, sde->dim))
    return fail(NJODE_E_BADARG, "%s", why);
  if (sde->model != NJODE_SDE_BLACK_SCHOLES && sde->model != NJODE_SDE_ORNSTEIN_UHLENBECK &&
      sde->model != NJODE_SDE_HESTON)
    return fail(NJODE_E_BADARG, "unknown SDE model %d", sde->model);
  return cond_exp_run(sde, nullptr, sde->dim, sde->model == NJODE_SDE_ORNSTEIN_UHLENBECK ? 1 : 0, batch,
                      sched, weight, pred, path_y, opt_loss, sq_diff, ws, ws_bytes, stream);
}

extern "C" int njode_cond_exp_staged_bytes(int32_t B, int32_t n_obs, int32_t n_times,
                                           int32_t n_steps, int32_t dim, int32_t n_stages,
                                           size_t* out) {
  if (!out) return fail(NJODE_E_BADARG, "null argument");
  if (const char* why = bad_sizes(B, n_obs, n_times, n_steps, dim)) return fail(NJODE_E_BADARG, "%s", why);
  if (n_stages < 1 || n_stages > NJODE_MAX_STAGES)
    return fail(NJODE_E_BADARG, "n_stages must be in [1, %d]", NJODE_MAX_STAGES);
  *out = layout(B, n_obs, n_times, n_steps, dim, true).total;
  return NJODE_OK;
}

extern "C" int njode_cond_exp_staged_f64(const NjodeSdeStage* stages, int32_t n_stages,
                                         const NjodeBatch* batch, const NjodeCondExpSchedule* sched,
                                         double weight, const float* pred, double* path_y,
                                         double* opt_loss, double* sq_diff, void* ws,
                                         size_t ws_bytes, njodeStream_t stream) {
  if (!stages || !batch || !sched) return fail(NJODE_E_BADARG, "null argument");
  if (n_stages < 1 || n_stages > NJODE_MAX_STAGES)
    return fail(NJODE_E_BADARG, "n_stages must be in [1, %d]", NJODE_MAX_STAGES);
  const int dim = stages[0].sde.dim;
  if (const char* why = bad_sizes(batch->batch_size, batch->n_obs, sched->n_times, sched->n_steps, dim))
    return fail(NJODE_E_BADARG, "%s", why);
  Stages sg;
  sg.n = n_stages;
  int mode = 0;
  for (int i = 0; i < n_stages; ++i) {
    const NjodeSde& p = stages[i].sde;
    if (p.model < NJODE_SDE_BLACK_SCHOLES || p.model > NJODE_SDE_HESTON_WO_FELLER)
      return fail(NJODE_E_BADARG, "unknown SDE model %d in stage %d", p.model, i);
    if (p.dim != dim) return fail(NJODE_E_BADARG, "stage %d is %d wide, stage 0 %d", i, p.dim, dim);
    if (i ? stages[i].first_step <= stages[i - 1].first_step : stages[i].first_step != 0)
      return fail(NJODE_E_BADARG, "first_step must increase strictly from 0");
    const int rv = stages[i].return_vol != 0;
    if (rv && (p.model != NJODE_SDE_HESTON_WO_FELLER || n_stages > 1 || (dim & 1)))
      return fail(NJODE_E_BADARG, "return_vol: a single HestonWOFeller stage of even width only");
    if (p.model == NJODE_SDE_ORNSTEIN_UHLENBECK) mode = 1;
    if (rv) mode = 2;
    sg.s[i] = StageP{p.model, p.has_sine, rv, stages[i].first_step, p.drift, p.mean, p.speed, p.sine_coeff};
  }
  for (int i = n_stages; i < NJODE_MAX_STAGES; ++i) sg.s[i] = StageP{0, 0, 0, 0x7fffffff, 0.0, 0.0, 0.0, 0.0};
  return cond_exp_run(nullptr, &sg, dim, mode, batch, sched, weight, pred, path_y, opt_loss, sq_diff, ws,
                      ws_bytes, stream);
}
