// njode_planner.hip -- the batch plan of the compiled shapes (njode_planner.h): CSR-by-time ->
// per-path links -> length-sorted segment items, the tail order and the trajectory layout, as
// launches of their own or as the one-launch plan of njode_plan.h, built in line, ahead
// (njode_plan_f32) or deferred into the next forward's ODE launch.  The one unit that compiles
// rocPRIM: it also defines the sort_pairs of njode_call.h.
#include <hip/hip_runtime.h>

#include <string.h>  // before rocprim: its texture iterator calls memset unqualified
#include <algorithm>

#include <rocprim/rocprim.hpp>

#include "njode_call.h"
#include "njode_layout.h"

using namespace njode;

// rocPRIM's default dispatch sorts up to 2^20 pairs with a merge sort (16 launches for the
// 200 000 rows of a 20 000-path batch, ~100 us); the keys here are 7-15 bit integers, for
// which one or two Onesweep passes are several times cheaper.  Small inputs keep the default
// (single-block sort / short merge sort).
using OnesweepCfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                               rocprim::default_config, 0>;
constexpr int ONESWEEP_MIN = 32768;
namespace njode {
hipError_t sort_pairs(void* tmp, size_t& bytes, const unsigned* k_in, unsigned* k_out, const int* v_in,
                      int* v_out, int n, int end_bit, bool onesweep, hipStream_t st) {
  if (onesweep && n >= ONESWEEP_MIN)
    return rocprim::radix_sort_pairs<OnesweepCfg>(tmp, bytes, k_in, k_out, v_in, v_out, (size_t)n,
                                                  0u, (unsigned)end_bit, st);
  return rocprim::radix_sort_pairs(tmp, bytes, k_in, k_out, v_in, v_out, (size_t)(n > 0 ? n : 1),
                                   0u, (unsigned)end_bit, st);
}
size_t plan_sort_temp_bytes(int n_obs, int B, int K) {
  const auto temp = [](int n, int end_bit) {
    size_t bytes = 0;
    (void)sort_pairs(nullptr, bytes, nullptr, nullptr, nullptr, nullptr, n, end_bit, !env().sort_merge, (hipStream_t)0);
    return bytes;
  };
  return std::max({temp(n_obs, bits_for((unsigned)(B > 0 ? B - 1 : 0))), temp(n_obs, bits_for((unsigned)K)),
                   temp(B, bits_for((unsigned)K))});
}
}  // namespace njode

namespace {

// ---- plan kernels -------------------------------------------------------------------------
__global__ void k_row_time(const int* __restrict__ time_ptr, int n_times, int n_obs,
                           int* __restrict__ t_of_row, int* __restrict__ iota, int K,
                           int* __restrict__ len_hist, const int* __restrict__ obs_idx, int B,
                           int* __restrict__ dense) {
  if (blockIdx.x == 0)   // histogram of segment lengths, filled by k_link
    for (int s = threadIdx.x; s <= K; s += blockDim.x) len_hist[s] = 0;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_obs) return;
  int lo = 0, hi = n_times;  // time_ptr[lo] <= r < time_ptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (time_ptr[mid] <= r) lo = mid; else hi = mid;
  }
  t_of_row[r] = lo;
  iota[r] = r;
  if (dense) dense[(size_t)lo * B + obs_idx[r]] = r;   // dense plan: scatter (see k_dense_link)
}

// NJODE_VALIDATE=1: preconditions of the batch layout (include/njode_hip.h).  flag bits:
// 1 obs_idx out of [0, B); 2 a path twice in one time slice; 4 n_obs_ot <= 0 for an observed path
__global__ void k_validate_rows(const int* __restrict__ obs_idx, int n_obs, int B,
                                const int* __restrict__ t_of_row, const int* __restrict__ dense,
                                const int* __restrict__ n_obs_ot, int* __restrict__ flag) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_obs) return;
  const int b = obs_idx[r];
  int bad = 0;
  if (b < 0 || b >= B) bad |= 1;
  else {
    if (dense && dense[(size_t)t_of_row[r] * B + b] != r) bad |= 2;
    if (n_obs_ot && n_obs_ot[b] <= 0) bad |= 4;
  }
  if (bad) atomicOr(flag, bad);
}
__global__ void k_range_rows(const int* __restrict__ obs_idx, int n_obs, int B, int* __restrict__ flag) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_obs && (obs_idx[r] < 0 || obs_idx[r] >= B)) atomicOr(flag, 1);
}

// rows sorted by (path, time): link every row to the previous / next row of its path
__global__ void k_link(int n_obs, int K, const int* __restrict__ path_sorted,
                       const int* __restrict__ row_by_path, const int* __restrict__ t_of_row,
                       const int* __restrict__ k_jump, int* __restrict__ first_j,
                       int* __restrict__ first_row, int* __restrict__ last_row,
                       int* __restrict__ item_prev, int* __restrict__ item_next,
                       int* __restrict__ item_kbeg, int* __restrict__ item_len,
                       unsigned* __restrict__ sort_key, int* __restrict__ len_hist) {
  // per-block histogram of the segment lengths in LDS (integer atomics: deterministic)
  constexpr int HB = 4096;
  __shared__ int hist[HB];
  const bool lds_hist = K < HB;
  if (lds_hist) {
    for (int s = threadIdx.x; s <= K; s += blockDim.x) hist[s] = 0;
    __syncthreads();
  }
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n_obs) {
  const int p = path_sorted[j], r = row_by_path[j];
  const bool has_prev = j > 0 && path_sorted[j - 1] == p;
  const bool has_next = j + 1 < n_obs && path_sorted[j + 1] == p;
  const int prev = has_prev ? row_by_path[j - 1] : -1;
  const int kend = k_jump[t_of_row[r]];
  const int kbeg = has_prev ? k_jump[t_of_row[prev]] : 0;
  item_prev[r] = prev;
  item_next[r] = has_next ? row_by_path[j + 1] : -1;
  item_kbeg[r] = kbeg;
  item_len[r] = kend - kbeg;
  sort_key[r] = (unsigned)(K - (kend - kbeg));  // ascending key == descending length
  if (!has_prev) { first_j[p] = j; first_row[p] = r; }
  if (!has_next) last_row[p] = r;
  const int len = kend - kbeg;
  if (len >= 0 && len <= K) atomicAdd(lds_hist ? &hist[len] : &len_hist[len], 1);
  }
  if (lds_hist) {
    __syncthreads();
    for (int s = threadIdx.x; s <= K; s += blockDim.x)
      if (hist[s]) atomicAdd(&len_hist[s], hist[s]);
  }
}

// ---- segment plan without the (path, time) sort: within one time slice a path has at most
// one row (both of the reference's collates guarantee it), so the rows are scattered into a
// dense [time slice][path] matrix (by k_row_time) and every path walks its column in time order.
__global__ void k_dense_link(int B, int n_times, int K, const int* __restrict__ dense,
                             const int* __restrict__ k_jump, int* __restrict__ first_row,
                             int* __restrict__ last_row, int* __restrict__ item_prev,
                             int* __restrict__ item_next, int* __restrict__ item_kbeg,
                             int* __restrict__ item_len, unsigned* __restrict__ sort_key,
                             int* __restrict__ len_hist) {
  constexpr int HB = 4096;
  __shared__ int hist[HB];
  const bool lds_hist = K < HB;
  if (lds_hist) {
    for (int s = threadIdx.x; s <= K; s += blockDim.x) hist[s] = 0;
    __syncthreads();
  }
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    int prev = -1, kprev = 0;
    constexpr int CH = 16;   // 16 independent loads in flight instead of one per iteration
    for (int i0 = 0; i0 < n_times; i0 += CH) {
      int rr[CH];
#pragma unroll
      for (int q = 0; q < CH; ++q) rr[q] = i0 + q < n_times ? dense[(size_t)(i0 + q) * B + b] : -1;
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int r = rr[q];
        if (r < 0) continue;
        const int kend = k_jump[i0 + q];
        const int len = kend - kprev;
        item_prev[r] = prev;
        if (prev >= 0) item_next[prev] = r; else first_row[b] = r;
        item_kbeg[r] = kprev;
        item_len[r] = len;
        sort_key[r] = (unsigned)(K - len);   // ascending key == descending length
        if (len >= 0 && len <= K) atomicAdd(lds_hist ? &hist[len] : &len_hist[len], 1);
        prev = r;
        kprev = kend;
      }
    }
    if (prev >= 0) { item_next[prev] = -1; last_row[b] = prev; }
    else { first_row[b] = -1; last_row[b] = -1; }   // (this path replaces the memset of first3)
  }
  if (lds_hist) {
    __syncthreads();
    for (int s = threadIdx.x; s <= K; s += blockDim.x)
      if (hist[s]) atomicAdd(&len_hist[s], hist[s]);
  }
}

// ---- stable counting sort of the rows by segment length (keys 0 .. K, ascending key ==
// descending length).  rocPRIM's Onesweep needs three kernels and three memsets for this
// (~75 us at 200 000 rows, all of it on the critical path in front of the ODE forward,
// profiles/r02_step_timeline.txt); the keys are tiny integers, so:
//   count    one wave per row block counts its rows per key (one round per distinct key of
//            64 rows, the same loop as the scatter: no atomics) -> table[key][row block];
//   scan     one wave per key: base of the key (from the length histogram) + exclusive scan
//            over the row blocks;
//   scatter  one wave per row block ranks its rows in row order (equal keys keep their row
//            order: nothing depends on timing).
// Row blocks are RW = 2^rw_shift rows, the largest table that fits the (otherwise unused)
// key_sorted buffer: nkeys * ceil(n / RW) <= n.
constexpr int CS_KEYS = 512;
__global__ void __launch_bounds__(256) k_cs_count(const unsigned* __restrict__ key, int n, int nkeys,
                                                  int nwb, int rw_shift, int* __restrict__ tab) {
  __shared__ int cnt_all[4][CS_KEYS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wb = blockIdx.x * 4 + w;
  if (wb >= nwb) return;   // (no workgroup barrier below: every wave works on its own counters)
  int* cnt = cnt_all[w];
  for (int s = lane; s < nkeys; s += 64) cnt[s] = 0;
  const int r0 = wb << rw_shift, rounds = 1 << (rw_shift - 6);
  for (int it = 0; it < rounds; ++it) {
    const int r = r0 + it * 64 + lane;
    const bool ok = r < n;
    const int k = ok ? min((int)key[r], nkeys - 1) : -1;
    unsigned long long todo = __ballot(ok);
    while (todo) {
      const int first = __ffsll((long long)todo) - 1;
      const int k0 = __shfl(k, first);
      const unsigned long long m = __ballot(ok && k == k0);
      if (lane == first) cnt[k0] += __popcll(m);
      todo &= ~m;
    }
  }
  for (int s = lane; s < nkeys; s += 64) tab[(size_t)s * nwb + wb] = cnt[s];
}
constexpr int CS_SCAN_CHUNKS = 32;   // row blocks per key held in registers: 64 x 32 = 2048
__global__ void __launch_bounds__(64) k_cs_scan(int* __restrict__ tab, const int* __restrict__ len_hist,
                                                int K, int nwb) {
  const int key = blockIdx.x, lane = threadIdx.x;
  int* row = tab + (size_t)key * nwb;
  int v[CS_SCAN_CHUNKS];   // all loads in flight before the first scan
#pragma unroll
  for (int q = 0; q < CS_SCAN_CHUNKS; ++q) {
    const int j = q * 64 + lane;
    v[q] = j < nwb ? row[j] : 0;
  }
  int run = 0;
  for (int i = lane; i < key; i += 64) run += len_hist[K - i];   // rows with a smaller key
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) run += __shfl_xor(run, o);
#pragma unroll
  for (int q = 0; q < CS_SCAN_CHUNKS; ++q) {
    if (q * 64 < nwb) {
      const int j = q * 64 + lane;
      int incl = v[q];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
      }
      if (j < nwb) row[j] = run + incl - v[q];
      run += __shfl(incl, 63);
    }
  }
}
__global__ void __launch_bounds__(256) k_cs_scatter(const unsigned* __restrict__ key, int n, int nkeys,
                                                    int nwb, int rw_shift, const int* __restrict__ tab,
                                                    int* __restrict__ order) {
  __shared__ int cnt_all[4][CS_KEYS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wb = blockIdx.x * 4 + w;
  if (wb >= nwb) return;   // (no workgroup barrier below: every wave works on its own counters)
  int* cnt = cnt_all[w];
  for (int s = lane; s < nkeys; s += 64) cnt[s] = tab[(size_t)s * nwb + wb];
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int r0 = wb << rw_shift, rounds = 1 << (rw_shift - 6);
  for (int it = 0; it < rounds; ++it) {
    const int r = r0 + it * 64 + lane;
    const bool ok = r < n;
    const int k = ok ? min((int)key[r], nkeys - 1) : -1;
    unsigned long long todo = __ballot(ok);
    int pos = 0;
    while (todo) {   // one round per distinct key of these 64 rows
      const int first = __ffsll((long long)todo) - 1;
      const int k0 = __shfl(k, first);
      const bool mine = ok && k == k0;
      const unsigned long long m = __ballot(mine);
      if (mine) pos = cnt[k0] + __popcll(m & lt);
      if (lane == first) cnt[k0] += __popcll(m);   // (one wave: its LDS accesses execute in order)
      todo &= ~m;
    }
    if (ok) order[pos] = r;
  }
}

// tail items (hT): path b evolves from its last observation (Euler step kbeg) to the end;
// ascending kbeg == descending tail length
__global__ void k_tail_keys(int B, const int* __restrict__ last_row,
                            const int* __restrict__ t_of_row, const int* __restrict__ k_jump,
                            unsigned* __restrict__ key, int* __restrict__ iota) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int lr = last_row[b];
  key[b] = lr >= 0 ? (unsigned)k_jump[t_of_row[lr]] : 0u;
  iota[b] = b;
}

// Tail order in ONE launch of ONE workgroup (round 5; B <= TAIL_ORDER_MAX): key of path b = the
// Euler step its tail starts at (ascending key == descending tail length), counting sort through
// LDS -- histogram, scan over the K + 1 bins, scatter through per-bin cursors.  The scatter's order
// WITHIN a bin depends on timing; nothing downstream does: the order only groups paths into tiles
// of 16 of (nearly) equal tail length, and a path's hT does not depend on its tile mates.  Replaces
// k_tail_keys + rocPRIM's radix sort: eight launches, ~240 us beside a busy forward
// (profiles/r04_autograd_route_timeline.txt), in front of the tails' kernel of every step that
// returns hT.
constexpr int TAIL_ORDER_MAX = 65536;
constexpr int TAIL_BINS_MAX = 4096;
// (asked by tail_order, plan_call and describe_plan alike) k_tail_order can sort these tails (else: the radix sort, and no deferred plan)
bool tail_order_fits(int B, int K) { return B <= TAIL_ORDER_MAX && K <= TAIL_BINS_MAX; }
bool tail_uses_radix(int B, int K) { return !tail_order_fits(B, K) || env().tail_sort_rocprim; }
__global__ void __launch_bounds__(1024) k_tail_order(int B, int K, const int* __restrict__ last_row,
                                                     const int* __restrict__ t_of_row,
                                                     const int* __restrict__ k_jump,
                                                     int* __restrict__ t_order) {
  __shared__ int bin[TAIL_BINS_MAX + 1];
  __shared__ int wsum[16];
  const int tid = threadIdx.x, nb = K + 1;
  for (int s = tid; s < nb; s += 1024) bin[s] = 0;
  __syncthreads();
  auto key_of = [&](int b) {
    const int lr = last_row[b];
    const int k = lr >= 0 ? k_jump[t_of_row[lr]] : 0;
    return k < 0 ? 0 : (k > K ? K : k);
  };
  for (int b = tid; b < B; b += 1024) atomicAdd(&bin[key_of(b)], 1);
  __syncthreads();
  // exclusive scan of the bins: thread t owns the chunk [t * ch, (t + 1) * ch)
  const int ch = (nb + 1023) / 1024;
  int loc = 0;
  for (int q = 0; q < ch; ++q) {
    const int s = tid * ch + q;
    if (s < nb) loc += bin[s];
  }
  int incl = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o);
    if ((tid & 63) >= o) incl += up;
  }
  if ((tid & 63) == 63) wsum[tid >> 6] = incl;
  __syncthreads();
  int before = 0;
  for (int i = 0; i < (tid >> 6); ++i) before += wsum[i];
  int run = before + incl - loc;
  __syncthreads();
  for (int q = 0; q < ch; ++q) {
    const int s = tid * ch + q;
    if (s < nb) {
      const int h = bin[s];
      bin[s] = run;      // the bin's cursor
      run += h;
    }
  }
  __syncthreads();
  for (int b = tid; b < B; b += 1024) t_order[atomicAdd(&bin[key_of(b)], 1)] = b;
}

// Trajectory layout and split point, one workgroup.
// Items are sorted by length (descending), so the items still running at step s are the
// prefix [0, cnt_s); base_s = sum_{s' < s} cnt_s'.
// Split point of the mixed ODE kernels (njode_mfma_split.h): tiles of 16 items are sorted by
// length; the T longest go to `ns` blocks that run a tile four waves wide (a tile-step ~R
// times faster than one wave does it), the rest to `nw` single-wave workers.  T minimises
//   max( max(L_0, H(T) / ns) / R ,  max(L_T, (S - H(T)) / nw) ),   H = prefix sum of lengths,
// with L_t = #{s : cnt_s > 16 t} and H(t) = sum_s min(t, ceil(cnt_s / 16)) -- everything
// from the K + 1 counts held in LDS.  out[0] / out[1]: backward / forward kernel.
constexpr int LAYOUT_THREADS = 1024;
__global__ void __launch_bounds__(LAYOUT_THREADS) k_traj_layout(const int* __restrict__ len_hist,
                                                                int n_obs, int K,
                                                                long long* __restrict__ base_s,
                                                                long long* __restrict__ base16_s,
                                                                SplitCfg sc) {
  // (cnt[K + 1] and the scans' tables behind it: SPLIT_KMAX + 1 + 64 ints lost best_t of the split point
  // for K >= 4 063 -- reads past the array returned 0 and the mixed kernels ran a wrong split)
  constexpr int LDS_INTS = SPLIT_KMAX + 2 + 6 * (LAYOUT_THREADS / 64);
  static_assert(LDS_INTS >= traj_layout_lds_ints(SPLIT_KMAX, LAYOUT_THREADS), "layout tables exceed lds");
  __shared__ __attribute__((aligned(16))) int lds[LDS_INTS];
  traj_layout_body<LAYOUT_THREADS>(len_hist, n_obs, K, base_s, base16_s, sc, lds, K <= SPLIT_KMAX);
}

// ---- the whole segment plan in ONE launch (njode_plan.h): as a kernel of its own for calls that
// build their plan in line; a plan built AHEAD (njode_plan_f32 with NJODE_C_PLAN_DEFER) rides in
// front of the next forward call's ODE-forward launch instead (k_ode_fwd_mixed)
__global__ void __launch_bounds__(PLAN_THREADS) k_plan_grid(PlanJob j) {
  __shared__ __attribute__((aligned(16))) int lds[PLAN_LDS_INTS];
  plan_grid_body(j, blockIdx.x, lds);
}

// A helper stream per device plus a small ring of events, created on first use and kept for
// the life of the process (DeviceState, njode_hostlib.h): the
// segment plan's link / sort / layout kernels (~90 us at 20 000 paths, tiny grids) run on it
// BESIDE the fragment packing and the encoder rows kernel, which only need t_of_row (round 2:
// the latter two moved to the helper stream, the plan back to the caller's).
// NJODE_PLAN_STREAM=0 keeps everything on the caller's stream.
bool side_streams(SideInfo* si) {
  DeviceLock g = device_state();
  if (!g.d) return false;
  DeviceState& d = *g.d;
  if (!d.st) {
    // lowest priority: the helper stream carries the throughput kernel (encoder rows); the
    // tiny latency-bound plan kernels on the caller's stream must not queue behind its blocks
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (hipStreamCreateWithPriority(&d.st, hipStreamNonBlocking, least) != hipSuccess) return false;
    // (the tails' stream: default priority -- they are to SHARE the chip with the ODE forward)
    if (hipStreamCreateWithFlags(&d.st2, hipStreamNonBlocking) != hipSuccess) return false;
    for (int i = 0; i < 8; ++i)
      for (int j = 0; j < 3; ++j)
        if (hipEventCreateWithFlags(&d.ev[i][j], hipEventDisableTiming) != hipSuccess) return false;
  }
  const unsigned i = d.next++ % 8;
  si->st = d.st;
  si->e0 = d.ev[i][0];
  si->e1 = d.ev[i][1];
  si->e2 = d.ev[i][2];
  si->st2 = d.st2;
  si->tails_sorted_on_st2 = 0;
  return true;
}

SplitCfg split_cfg(const KArgs& a) {
  SplitCfg sc;
  sc.on = a.ode_split;
  sc.ns[0] = a.n_split_blocks;
  sc.nw[0] = 4 * (a.n_blocks_bwd - a.n_split_blocks);
  sc.ns[1] = a.n_split_fwd;
  sc.nw[1] = 4 * (a.n_blocks_fwd - a.n_split_fwd);
  sc.r[0] = env().split_r_bwd;
  sc.r[1] = env().split_r_fwd;
  return sc;
}

// The tail order is read by the tails' kernel only.  With helper streams (large batches) that
// kernel runs on a stream of its own beside the items' ODE forward (njode_cfg.hip), and so does
// this sort -- eight small launches (~50 us at 20 000 paths) that used to sit in front of the
// forward of every step that returns hT.  (own_stream: only when the items' sort is the counting
// sort: rocPRIM's temporary storage is one buffer.)
hipError_t tail_order(Call& c, char* w, bool own_stream, hipStream_t st) {
  KArgs& a = c.a;
  const int B = a.B, K = a.K;
  unsigned* tkey = (unsigned*)(w + c.L.tail4);
  unsigned* tkey_sorted = tkey + B;
  int* tiota = (int*)(tkey + 2 * (size_t)B);
  hipStream_t ts = st;
  if (a.plan_ready && own_stream) {
    hipError_t e = hipEventRecord(c.side.e2, st);          // last_row (k_dense_link) is enqueued
    if (e == hipSuccess) e = hipStreamWaitEvent(c.side.st2, c.side.e2, 0);
    if (e != hipSuccess) return e;
    ts = c.side.st2;
    c.side.tails_sorted_on_st2 = 1;
  }
  if (!tail_uses_radix(B, K)) {
    ProfScope ps("k_tail_order", ts);
    k_tail_order<<<1, 1024, 0, ts>>>(B, K, a.last_row, a.t_of_row, a.k_jump, (int*)a.t_order);
    return hipSuccess;
  }
  ProfScope ps("k_tail_keys", ts);
  k_tail_keys<<<cdiv(B, 256), 256, 0, ts>>>(B, a.last_row, a.t_of_row, a.k_jump, tkey, tiota);
  size_t tmp = c.L.sort_tmp_bytes;
  return sort_pairs(w + c.L.sort_tmp, tmp, (const unsigned*)tkey, tkey_sorted, (const int*)tiota,
                    (int*)a.t_order, B, bits_for((unsigned)K), !env().sort_merge, ts);
}

// ---- the one-launch plan (njode_plan.h) ------------------------------------------------------
constexpr int PLAN_BLOCKS_CAP = 256;   // (all resident from the start: one per CU at most)
constexpr size_t PLAN_STAMP_BYTES = (size_t)PLAN_BLOCKS_CAP * 8 * sizeof(unsigned long long);
// What the library keeps per device for the one-launch plan: ONE word that a plan barrier sets when
// it gives up waiting (plan_sync, njode_plan.h) and the stage stamps of the last job (maintainer aid,
// NJODE_PLAN_STAMPS=1).  The barrier COUNTERS are not here: every plan has its own eight words in its
// own buffer (round 5 handed out 16 shared sets round-robin, which two overlapping launches on one
// set could corrupt silently: ADVICE r5).
unsigned* plan_sync_mem() {
  DeviceLock g = device_state();
  if (!g.d) return nullptr;
  unsigned*& mem = g.d->plan_mem;      // [0] the failure word, then the stamps
  if (!mem) {
    const size_t bytes = 64 + PLAN_STAMP_BYTES;
    if (hipMalloc((void**)&mem, bytes) != hipSuccess) return nullptr;
    // (a memset is asynchronous to the host and the null stream does not order the callers' streams:
    // the word must BE zero before the first plan kernel runs -- once per process and device)
    if (hipMemset(mem, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
      (void)hipFree(mem);
      mem = nullptr;
    }
  }
  return mem;
}
unsigned long long* plan_stamps() {
  unsigned* m = plan_sync_mem();
  return m ? (unsigned long long*)(m + 16) : nullptr;
}

int plan_blocks(int n) {
  const int fixed = env().plan_blocks;
  if (fixed >= 1) return fixed > PLAN_BLOCKS_CAP ? PLAN_BLOCKS_CAP : fixed;
  if (n <= 2048) return 1;
  // (20 000 paths = 200 000 rows, hosted by the ODE forward: 32 blocks outlast it -- 0.90 ms per step --,
  // 48 end with it: 0.847, 64 / 96 / 128: 0.864 / 0.866 / 0.874 -- more blocks take more of the
  // forward's slots; profiles/r05_plan_in_forward.txt)
  const int p = cdiv(n, 4096) + 1;
  return p < 2 ? 2 : (p > 64 ? 64 : p);
}
// Smallest row block (2^shift rows) of the counting sort whose count table fits the key_sorted buffer
// and the scan's registers (`scan_chunks` x 64 row blocks per key); 0: none does.
int cs_shift_for(int n, int K, int scan_chunks) {
  for (int sh = env().cs_shift < 7 ? 7 : env().cs_shift; sh <= 12; ++sh)
    if ((size_t)(K + 1) * cdiv(n, 1 << sh) <= (size_t)n && cdiv(n, 1 << sh) <= 64 * scan_chunks) return sh;
  return 0;
}
// The rows of a segment-plan call are linked through the dense matrix (else: sorted by path and time)
bool plan_is_dense(const Call& c) {
  return c.route.seg && c.route.size.dense_cells && !env().plan_sort && c.a.n_obs > 0;
}
// The questions build_plan, plan_call and describe_plan (njode_debug_plan_view) all ask, each stated once.
// row-block shift of the multi-launch plan's counting sort; 0: rocPRIM's radix sort orders the rows
int multi_launch_cs_shift(bool dense_plan, int n, int K) {
  return (dense_plan && !env().sort_rocprim && n >= 16384 && K + 1 <= CS_KEYS) ? cs_shift_for(n, K, CS_SCAN_CHUNKS) : 0;
}
// an in-line plan of n rows is ONE whole launch (else: k_row_time, then the body from its third stage)
bool inline_plan_whole(int n) { return n <= env().plan_inline_max; }
int stage2_plan_blocks() { return std::min(std::max(env().plan_inline_blocks, 2), PLAN_BLOCKS_CAP); }
// the one-launch plan's scan of the count table takes a thread per key (else a wave per key: njode_plan.h, stage 4)
bool scan_thread_per_key(int cs_nwb) { return cs_nwb <= PLAN_SCAN_CHUNKS; }

// The job of the call `c` whose plan prefix is at `w`; false: this plan is not one the single launch
// builds (no dense matrix, a schedule that is too long for its LDS tables, NJODE_VALIDATE).
// sched_src: device-visible pinned copy of the packed schedule, or null when it is already in place.
bool fill_plan_job(const Call& c, char* w, const int* sched_src, PlanJob& j) {
  const KArgs& a = c.a;
  const int n = a.n_obs, B = a.B, K = a.K;
  if (!env().plan_grid || !plan_is_dense(c) || env().validate) return false;
  if (K + 1 > PLAN_KEYS || a.n_times + 1 > PLAN_TIMES) return false;
  j = PlanJob{};
  j.n = n; j.B = B; j.K = K; j.n_times = a.n_times;
  if (n < 16384) {
    int sh = 7;
    while (cdiv(n, 1 << sh) > PLAN_CS_SMALL_BLOCKS) ++sh;
    j.cs_shift = sh;
    j.cs_tab = (int*)(w + c.L.cs_small);
  } else {
    j.cs_shift = cs_shift_for(n, K, PLAN_SCAN_CHUNKS);
    if (!j.cs_shift) return false;
    j.cs_tab = (int*)(w + c.L.key_sorted);
  }
  j.cs_nwb = cdiv(n, 1 << j.cs_shift);
  j.P = plan_blocks(n);
  j.last_stage = c.route.seg_chain ? 2 : 5;
  j.sched_src = sched_src;
  j.sched_dst = (int*)(w + c.L.sched);
  j.sched_ints = 2 * K + 3 * a.n_times + 1;
  j.time_ptr = (const int*)(a.time_f32 + a.n_times);
  j.k_jump = a.k_jump;
  j.obs_idx = a.obs_idx;
  j.t_of_row = (int*)a.t_of_row;
  j.dense = (int*)(w + c.L.dense);
  j.first_row = (int*)a.first_row;
  j.last_row = (int*)a.last_row;
  j.item_prev = (int*)a.item_prev;
  j.item_next = (int*)a.item_next;
  j.item_kbeg = (int*)a.item_kbeg;
  j.item_len = (int*)a.item_len;
  j.sort_key = (unsigned*)(w + c.L.sort_key);
  j.len_hist = (int*)(w + c.L.len_hist);
  j.order = (int*)a.order;
  j.base_s = (long long*)a.base_s;
  j.base16_s = (long long*)a.base16_s;
  j.sc = split_cfg(a);
  // the plan's OWN grid-barrier counters: eight words of its buffer (behind the validation flag)
  j.sync = (unsigned*)(w + c.L.vflag + 64);
  j.sync_base = 0;
  return true;
}
// Right before the job's launch is enqueued: its barrier counters are zeroed on the stream that
// carries the launch.  No counters: one block builds the plan.
void arm_plan_job(PlanJob& j, hipStream_t st, unsigned** zero_later = nullptr) {
  j.fail = nullptr;
  if (j.P > 1) {
    // the plan's own counters start at zero, on the stream that carries its launch
    j.fail = plan_sync_mem();
    j.sync_base = 0;
    if (j.fail && zero_later) {
      // (hosted by an ODE forward: the fragment-pack launch in front of it, same stream, zeroes them)
      *zero_later = j.sync;
    } else if (!j.fail || hipMemsetAsync(j.sync, 0, 8 * sizeof(unsigned), st) != hipSuccess) {
      (void)hipGetLastError();
      j.P = 1;
    }
  }
  if (env().plan_stamps) j.stamps = plan_stamps();
}

thread_local PendingPlan g_pending;

}  // namespace

namespace njode {

void pending_tails(const PendingPlan& p) {
  if (!p.tails) return;
  ProfScope ps("k_tail_order", p.st);
  k_tail_order<<<1, 1024, 0, p.st>>>(p.tB, p.tK, p.t_last_row, p.t_t_of_row, p.t_k_jump, p.t_order);
}
bool pending_flush() {
  if (!g_pending.on) return false;
  g_pending.on = false;
  ProfScope ps("k_plan_grid", g_pending.st);
  arm_plan_job(g_pending.job, g_pending.st);
  k_plan_grid<<<g_pending.job.P, PLAN_THREADS, 0, g_pending.st>>>(g_pending.job);
  pending_tails(g_pending);
  return true;
}

int build_plan(Call& c, void* ws, hipStream_t st) {
  KArgs& a = c.a;
  a.plan_ready = nullptr;
  char* w = (char*)ws;
  const int n = a.n_obs, B = a.B, K = a.K;
  const bool dense_plan = plan_is_dense(c), validate = env().validate;
  // first_j / first_row / last_row = -1 for paths without rows (the dense link writes the two
  // it needs itself)
  if (!dense_plan) HIP_TRY(hipMemsetAsync(w + c.L.first3, 0xFF, (size_t)B * 4 * 3, st));
  if (n == 0) return NJODE_OK;
  const int* time_ptr = (const int*)(a.time_f32 + a.n_times);
  int* iota = (int*)(w + c.L.iota);
  int* len_hist = (int*)(w + c.L.len_hist);
  int* dense = dense_plan ? (int*)(w + c.L.dense) : nullptr;
  int* vflag = (int*)(w + c.L.vflag);
  if (validate) {
    // an index out of range must be caught BEFORE the scatter below writes through it
    HIP_TRY(hipMemsetAsync(vflag, 0, 4, st));
    k_range_rows<<<cdiv(n, 256), 256, 0, st>>>(a.obs_idx, n, B, vflag);
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, vflag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h) return fail(NJODE_E_BADARG, "obs_idx has entries outside [0, batch_size)");
  }
  // the whole plan in one launch (njode_plan.h): small plans, where every dispatch counts
  // (NJODE_PLAN_INLINE_MAX rows: 10 000 rows 58 us against ~70 us of launches; larger plans keep the
  // launches below, which fill the chip: 200 000 rows ~100 us against 137 us on 64 blocks)
  PlanJob job;
  if (dense_plan && inline_plan_whole(n) && fill_plan_job(c, w, nullptr, job)) {
    {
      ProfScope ps("k_plan_grid", st);
      arm_plan_job(job, st);
      k_plan_grid<<<job.P, PLAN_THREADS, 0, st>>>(job);
    }
    if (c.route.tails) HIP_TRY(tail_order(c, w, false, st));
    HIP_TRY(hipGetLastError());
    return NJODE_OK;
  }
  if (dense_plan) HIP_TRY(hipMemsetAsync(dense, 0xFF, (size_t)a.n_times * B * 4, st));
  // counting sort of the rows by length (kernels above): where its table fits
  const int cs_shift = multi_launch_cs_shift(dense_plan, n, K);
  const int cs_nwb = cs_shift ? cdiv(n, 1 << cs_shift) : 0;
  int* cs_tab = cs_shift ? (int*)(w + c.L.key_sorted) : nullptr;
  {
    ProfScope ps("k_row_time", st);
    k_row_time<<<cdiv(n, 256), 256, 0, st>>>(time_ptr, a.n_times, n, (int*)a.t_of_row, iota, K,
                                             len_hist, a.obs_idx, B, dense);
  }
  if (validate) {
    k_validate_rows<<<cdiv(n, 256), 256, 0, st>>>(a.obs_idx, n, B, a.t_of_row, dense, a.n_obs_ot, vflag);
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, vflag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h & 2) return fail(NJODE_E_BADARG, "a path has two rows in one time slice");
    if (h & 4) return fail(NJODE_E_BADARG, "n_obs_ot <= 0 for a path that has observation rows");
  }
  // everything below is needed by the ODE kernels only, and the forward starts with pack +
  // encoder rows, which only need t_of_row: those two go to the helper stream (njode_cfg.hip),
  // the plan stays here -- it is the longer chain (~110 us against ~55 at 20 000 paths), and a
  // cross-stream hop costs ~10 us at each end (profiles/r02_step_timeline.txt: with the plan on
  // the helper stream the ODE forward started 74 us after the encoder rows had finished)
  // (only where there is something to hide: small batches lose more on the event hops)
  if (env().plan_stream && !c.plan_only && c.route.seg_mfma && n >= 65536 && side_streams(&c.side)) {
    HIP_TRY(hipEventRecord(c.side.e0, st));
    a.plan_ready = (void*)&c.side;
  }
  // Large plans built in line (the autograd route, calls that prefetch nothing): links, counting sort
  // and layout as ONE launch of the plan body from its third stage on (njode_plan.h; k_row_time above
  // has filled the dense matrix and the row times, which is all the helper stream waits for): five
  // dispatches with their gaps, ~115 us at 200 000 rows, become one kernel of ~70.  NJODE_PLAN_GRID_TAIL=0
  // keeps the launches.
  if (dense_plan && env().plan_grid_tail && fill_plan_job(c, w, nullptr, job)) {
    job.first_stage = 2;
    job.P = stage2_plan_blocks();
    arm_plan_job(job, st);
    {
      ProfScope ps("k_plan_grid", st);
      k_plan_grid<<<job.P, PLAN_THREADS, 0, st>>>(job);
    }
    if (c.route.tails) HIP_TRY(tail_order(c, w, true, st));
    HIP_TRY(hipGetLastError());
    return NJODE_OK;
  }
  size_t tmp = c.L.sort_tmp_bytes;
  unsigned* sort_key = (unsigned*)(w + c.L.sort_key);
  if (dense_plan) {
    // (the lockstep kernels need the path-major arrays of the sort below; the segment plan
    // only the links)
    ProfScope ps("k_dense_link", st);
    k_dense_link<<<cdiv(B, 256), 256, 0, st>>>(B, a.n_times, K, dense, a.k_jump, (int*)a.first_row,
                                               (int*)a.last_row, (int*)a.item_prev,
                                               (int*)a.item_next, (int*)a.item_kbeg,
                                               (int*)a.item_len, sort_key, len_hist);
  } else {
    ProfScope ps("k_link", st);
    HIP_TRY(sort_pairs(w + c.L.sort_tmp, tmp, (const unsigned*)a.obs_idx, (unsigned*)a.path_sorted,
                       (const int*)iota, (int*)a.row_by_path, n, bits_for((unsigned)(B - 1)), !env().sort_merge, st));
    k_link<<<cdiv(n, 256), 256, 0, st>>>(n, K, a.path_sorted, a.row_by_path, a.t_of_row, a.k_jump,
                                         (int*)a.first_j, (int*)a.first_row, (int*)a.last_row,
                                         (int*)a.item_prev, (int*)a.item_next, (int*)a.item_kbeg,
                                         (int*)a.item_len, sort_key, len_hist);
  }
  if (c.route.seg) {
    unsigned* key_sorted = (unsigned*)(w + c.L.key_sorted);
    if (cs_tab) {
      ProfScope ps("k_cs_scatter", st);
      k_cs_count<<<cdiv(cs_nwb, 4), 256, 0, st>>>(sort_key, n, K + 1, cs_nwb, cs_shift, cs_tab);
      k_cs_scan<<<K + 1, 64, 0, st>>>(cs_tab, len_hist, K, cs_nwb);
      k_cs_scatter<<<cdiv(cs_nwb, 4), 256, 0, st>>>(sort_key, n, K + 1, cs_nwb, cs_shift, cs_tab,
                                                   (int*)a.order);
    } else {
      ProfScope ps("sort_rows_by_length", st);
      tmp = c.L.sort_tmp_bytes;
      HIP_TRY(sort_pairs(w + c.L.sort_tmp, tmp, (const unsigned*)sort_key, key_sorted,
                         (const int*)iota, (int*)a.order, n, bits_for((unsigned)K), !env().sort_merge, st));
    }
    {
      ProfScope ps("k_traj_layout", st);
      k_traj_layout<<<1, LAYOUT_THREADS, 0, st>>>(len_hist, n, K, (long long*)a.base_s,
                                                  (long long*)a.base16_s, split_cfg(a));
    }
    if (c.route.tails) HIP_TRY(tail_order(c, w, cs_tab != nullptr, st));
  }
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}

int plan_call(Call& c, const NjodeSchedule* sched, int call_flags, hipStream_t st) {
  int rc;
  const bool tails = c.route.tails;
  if (call_flags & NJODE_C_PLAN_DEFER) {
    pending_flush();   // (an older job nobody hosted)
    PendingPlan& p = g_pending;
    const bool tails_ok = !tails || tail_order_fits(c.a.B, c.a.K);
    if (tails_ok && fill_plan_job(c, c.pw, nullptr, p.job)) {
      // the schedule: read by the plan's first block from the caller's pinned copy when there is
      // one (no copy command on the queue), else copied now
      void* dptr = nullptr;
      if (schedule_contiguous(sched) && hipHostGetDevicePointer(&dptr, (void*)sched->step_dt, 0) == hipSuccess && dptr) {
        p.job.sched_src = (const int*)dptr;
      } else {
        (void)hipGetLastError();
        if ((rc = upload_schedule(c.pw + c.L.sched, sched, st))) return rc;
      }
      p.st = st;
      p.tails = tails;
      p.tB = c.a.B;
      p.tK = c.a.K;
      p.t_last_row = c.a.last_row;
      p.t_t_of_row = c.a.t_of_row;
      p.t_k_jump = c.a.k_jump;
      p.t_order = (int*)c.a.t_order;
      p.on = true;
      return NJODE_OK;
    }
  }
  if ((rc = upload_schedule(c.pw + c.L.sched, sched, st))) return rc;
  if ((rc = build_plan(c, c.pw, st))) return rc;
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}

void describe_plan(const Call& c, int call_flags, NjodePlanView* v) {
  const KArgs& a = c.a;
  const int n = a.n_obs, B = a.B, K = a.K;
  const bool dense = plan_is_dense(c);
  v->seg = c.route.seg ? 1 : 0;
  v->sort_linked = dense ? 0 : 1;
  v->tails = c.route.tails ? 1 : 0;
  PlanJob job;
  const bool fits = n > 0 && fill_plan_job(c, c.pw, nullptr, job);
  // (the same order of questions as plan_call and build_plan)
  const bool tails_ok = !c.route.tails || tail_order_fits(B, K);
  const bool deferred = (call_flags & NJODE_C_PLAN_DEFER) && tails_ok && fits;
  const bool whole = deferred || (fits && inline_plan_whole(n));
  const bool from2 = !whole && fits && env().plan_grid_tail;
  v->one_launch = (whole || from2) ? 1 : 0;
  v->plan_first_stage = from2 ? 2 : 0;
  v->tail_radix = (c.route.tails && !deferred && tail_uses_radix(B, K)) ? 1 : 0;   // (a deferred plan's tails: k_tail_order)
  if (v->one_launch) {
    v->plan_blocks = from2 ? stage2_plan_blocks() : job.P;
    v->links_only = job.last_stage <= 2 ? 1 : 0;
    v->cs_shift = job.cs_shift;
    v->cs_nwb = job.cs_nwb;
    v->cs_large = job.cs_tab == (int*)(c.pw + c.L.key_sorted) ? 1 : 0;
    v->scan_thread_per_key = scan_thread_per_key(job.cs_nwb) ? 1 : 0;
    v->lds_cnt = 1;
  } else if (c.route.seg && n > 0) {
    const int sh = multi_launch_cs_shift(dense, n, K);
    v->cs_shift = sh;
    v->cs_nwb = sh ? cdiv(n, 1 << sh) : 0;
    v->cs_large = sh ? 1 : 0;
    v->lds_cnt = K <= SPLIT_KMAX ? 1 : 0;
  }
  const SplitCfg sc = split_cfg(a);
  v->split_on = sc.on;
  for (int i = 0; i < 2; ++i) { v->split_ns[i] = sc.ns[i]; v->split_nw[i] = sc.nw[i]; v->split_r[i] = sc.r[i]; }
}

void pending_host_or_flush(Call& c, hipStream_t st, PendingPlan& hosted) {
  if (!g_pending.on) return;
  const bool own = c.planned && (char*)c.pw + c.L.sched == (char*)g_pending.job.sched_dst;   // this call's own plan
  if (c.route.hosts_plan && g_pending.st == st && !own) {
    hosted = g_pending;
    g_pending.on = false;
    arm_plan_job(hosted.job, st, &c.a.plan_sync_zero);
    c.a.plan_job = &hosted.job;
  } else {
    pending_flush();
  }
}

}  // namespace njode

// maintainer aid (NJODE_PLAN_STAMPS=1): the 100 MHz wall clock every block of the LAST one-launch
// plan wrote at its stage ends: out[block * 8 + slot], slot 6 = entry, 0..5 = end of stage 0..5
extern "C" int njode_debug_plan_stamps(unsigned long long* out, int cap_blocks) {
  unsigned long long* d = plan_stamps();
  if (!d || !out || cap_blocks <= 0) return 0;
  const int nb = cap_blocks < PLAN_BLOCKS_CAP ? cap_blocks : PLAN_BLOCKS_CAP;
  if (hipDeviceSynchronize() != hipSuccess) return 0;
  if (hipMemcpy(out, d, (size_t)nb * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return nb;
}

// 1 when a grid barrier of a one-launch plan gave up waiting since the last call (the plans built since
// are garbage: the caller must rebuild them), 0 otherwise, -1 on a HIP error.  Synchronises the device.
extern "C" int njode_plan_barrier_failures(void) {
  unsigned* m = plan_sync_mem();
  if (!m) return 0;
  unsigned v = 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(&v, m, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (v && hipMemset(m, 0, sizeof(v)) != hipSuccess) return -1;
  if (v) (void)fail(NJODE_E_HIP, "a grid barrier of the one-launch plan timed out (njode_plan.h: plan_sync)");
  return v ? 1 : 0;
}

extern "C" int njode_plan_flush(void) { return pending_flush() ? 1 : 0; }
