// njode_gob.hip -- the GRU-ODE-Bayes baseline (include/njode_gob.h): forward and exact discrete
// adjoint of the reference's NNFOwithBayesianJumps in fp32.  The latency regime of DESIGN 4h:
// one wave per path walks the whole schedule, lane j holds unit j of every vector (h, the gates,
// p, the p_model / covariates_map hidden layers; the prep layer's up to 256 units as four
// registers per lane).  A layer is out_j = b_j + sum_i W[j][i] in_i with in_i broadcast out of
// lane i's register (v_readlane into the scalar operand of the fma) -- no LDS round trip, no
// barrier of any kind inside an Euler step.  The three cell matrices live in a per-workgroup LDS
// table filled once (row stride H | 1: lane j reading row j and lane i reading column i are both
// free of bank conflicts); the other layers read a table transposed once per call into the
// workspace (lane j = output unit j reads consecutive floats), the adjoint reads them in their own
// [out][in] order (lane i = input unit i).
//
// p_model is evaluated only where its value is used: at a jump (the value the previous event
// left, and the new one for loss_2), for a path row, and at every event with impute.
//
// Backward: the forward stores h before every Euler step and jump and at the end; the sweep
// walks the events in reverse, recomputes the gates, and carries the adjoints of h and of p (p is
// replaced at every event, so its adjoint is alive only between a consumer and the event that
// produced it).  Weight gradients: every workgroup (one wave) of the sweep owns one slab of P
// floats; the cell matrices accumulate in LDS and are written to the slab once, the rest is
// added to the slab in place, each element always by the same lane, paths in order; a last
// kernel sums the slabs in slab order -- no atomics, the same bits every time.
#define NJ_ACC_TANH 1
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/njode_gob.h"
#include "njode_call.h"
#include "njode_pathwalk.h"

using namespace njode;

namespace {

constexpr int MAX_SLABS = 1024;
constexpr size_t SLAB_BUDGET = (size_t)256 << 20;
constexpr uint32_t NET_COV = 5, NET_P = 6, NET_P_JUMP = 7;
constexpr uint32_t TKEY_START = 0xffffffffu;
constexpr int NMAT = 7;   // matrices with a transposed copy

struct GModel {
  int D, H, PH, PR, CH, NG, D2, HS, impute, P;
  int p0w, p0b, p3w, p3b, lxw, lxb, hh, hz, hr, wp, bp, wih, whh, bih, bhh, c0w, c0b, c3w, c3b;
  int t_off[NMAT], t_out[NMAT], t_in[NMAT];
};

struct GArgs {
  GModel m;
  int B, n_obs, nt, K, flags, S, drop;
  float mixing;
  DropCtx dc;
  const float *params, *wt;
  const float *start_X, *X, *M;
  const int* obs_idx;
  const float* step_dt;
  const int *k_jump, *time_ptr;
  int* row_of;            // [nt][B] row of (time slice, path) or -1
  float *hT, *path_h, *path_p;
  double* loss_part;      // [2][B]
  float *h_step, *h_bj, *h_end;
  const float *grad_loss, *grad_loss_1, *grad_hT;
  float* slabs;
};

// ---- device ------------------------------------------------------------------------------------

extern __shared__ __attribute__((aligned(16))) float gob_smem[];

// the value of lane i's register (i wave-uniform)
NJ_DEV float bcast(float v, int i) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}
// sigmoid and exp: the library's expf and an IEEE division
NJ_DEV float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// the shape-generic stream (njode_gen.h drop_base / drop_word), layer 0, unit = lane
NJ_DEV bool keep_unit(const GArgs& A, int b, uint32_t tkey, uint32_t net, int lane) {
  if (!A.drop) return true;
  const uint32_t base = drop_state(A.dc, (uint32_t)b, 0u, tkey, net);
  const uint32_t w = fmix32(base ^ ((uint32_t)(lane >> 1) * 0x85ebca6bu + 0x632be5abu));
  return ((lane & 1) ? (w >> 16) : (w & 0xffffu)) >= A.dc.thr16;
}

// out_j = acc0 + sum_i WT[i][j] x_i: WT [n_in][n_out] (transposed copy), j = this lane's unit
// (clamped by the caller), x_i in lane i's register
NJ_DEV float dot_t(const float* __restrict__ wt, int n_out, int jc, float x, int n_in, float acc) {
  // (four loads in flight per round: a loop of single dependent loads pays the full memory latency
  // per term; the sum keeps its order)
  const float* w = wt + jc;
  int i = 0;
  for (; i + 4 <= n_in; i += 4) {
    const float w0 = w[(size_t)i * n_out], w1 = w[(size_t)(i + 1) * n_out], w2 = w[(size_t)(i + 2) * n_out],
                w3 = w[(size_t)(i + 3) * n_out];
    acc = fmaf(w0, bcast(x, i), acc);
    acc = fmaf(w1, bcast(x, i + 1), acc);
    acc = fmaf(w2, bcast(x, i + 2), acc);
    acc = fmaf(w3, bcast(x, i + 3), acc);
  }
  for (; i < n_in; ++i) acc = fmaf(w[(size_t)i * n_out], bcast(x, i), acc);
  return acc;
}
// g_i = sum_j W[j][i] d_j: W [n_out][stride] in its own order, i = this lane's (clamped) input unit
NJ_DEV float dot_in(const float* __restrict__ w0p, int stride, int ic, float d, int n_out, float acc) {
  const float* w = w0p + ic;
  int j = 0;
  for (; j + 4 <= n_out; j += 4) {
    const float w0 = w[(size_t)j * stride], w1 = w[(size_t)(j + 1) * stride], w2 = w[(size_t)(j + 2) * stride],
                w3 = w[(size_t)(j + 3) * stride];
    acc = fmaf(w0, bcast(d, j), acc);
    acc = fmaf(w1, bcast(d, j + 1), acc);
    acc = fmaf(w2, bcast(d, j + 2), acc);
    acc = fmaf(w3, bcast(d, j + 3), acc);
  }
  for (; j < n_out; ++j) acc = fmaf(w[(size_t)j * stride], bcast(d, j), acc);
  return acc;
}
// G[j][i] += d_j x_i for j < n_out, this lane's column i (on = i < n_in)
NJ_DEV void outer_add(float* __restrict__ g0, int stride, int i, bool on, float d, int n_out, float x) {
  float* g = g0 + i;
  int j = 0;
  for (; j + 4 <= n_out; j += 4) {
    const float d0 = bcast(d, j), d1 = bcast(d, j + 1), d2 = bcast(d, j + 2), d3 = bcast(d, j + 3);
    if (on) {
      const float a0 = g[(size_t)j * stride], a1 = g[(size_t)(j + 1) * stride], a2 = g[(size_t)(j + 2) * stride],
                  a3 = g[(size_t)(j + 3) * stride];
      g[(size_t)j * stride] = fmaf(d0, x, a0);
      g[(size_t)(j + 1) * stride] = fmaf(d1, x, a1);
      g[(size_t)(j + 2) * stride] = fmaf(d2, x, a2);
      g[(size_t)(j + 3) * stride] = fmaf(d3, x, a3);
    }
  }
  for (; j < n_out; ++j) {
    const float dj = bcast(d, j);
    if (on) g[(size_t)j * stride] = fmaf(dj, x, g[(size_t)j * stride]);
  }
}

struct PMv { float apre, ad, p; bool kept; };
// p = p_model(h): Linear -> ReLU -> Dropout -> Linear
NJ_DEV PMv pm_fwd(const GArgs& A, float h, uint32_t net, uint32_t tkey, int b, int lane) {
  const GModel& m = A.m;
  PMv v;
  const int jc = lane < m.PH ? lane : m.PH - 1;
  v.apre = dot_t(A.wt + m.p0w, m.PH, jc, h, m.H, A.params[m.p0b + jc]);
  v.kept = keep_unit(A, b, tkey, net, lane);
  float a = fmaxf(v.apre, 0.0f);
  if (A.drop) a = v.kept ? a * A.dc.inv_keep : 0.0f;
  v.ad = lane < m.PH ? a : 0.0f;
  const int cc = lane < m.D2 ? lane : m.D2 - 1;
  const float p = dot_t(A.wt + m.p3w, m.D2, cc, v.ad, m.PH, A.params[m.p3b + cc]);
  v.p = lane < m.D2 ? p : 0.0f;
  return v;
}
// its adjoint at the same h: lp = adjoint of p; adds the weight gradients to the slab, returns
// the adjoint of h
NJ_DEV float pm_bwd(const GArgs& A, float* __restrict__ slab, const PMv& v, float h, float lp, int lane) {
  const GModel& m = A.m;
  outer_add(slab + m.p3w, m.PH, lane, lane < m.PH, lp, m.D2, v.ad);
  if (lane < m.D2) slab[m.p3b + lane] += lp;
  const int ic = lane < m.PH ? lane : m.PH - 1;
  float da = dot_in(A.params + m.p3w, m.PH, ic, lp, m.D2, 0.0f);
  if (A.drop) da = v.kept ? da * A.dc.inv_keep : 0.0f;
  const float dpre = (lane < m.PH && v.apre > 0.0f) ? da : 0.0f;
  outer_add(slab + m.p0w, m.H, lane, lane < m.H, dpre, m.PH, h);
  if (lane < m.PH) slab[m.p0b + lane] += dpre;
  const int hc = lane < m.H ? lane : m.H - 1;
  const float dh = dot_in(A.params + m.p0w, m.H, hc, dpre, m.PH, 0.0f);
  return lane < m.H ? dh : 0.0f;
}

struct Cov { float cpre, ad; bool kept; };
// h0 = covariates_map(x0): Linear -> ReLU -> Dropout -> Linear -> Tanh
NJ_DEV float cov_fwd(const GArgs& A, float x0, int b, int lane, Cov& c) {
  const GModel& m = A.m;
  const int jc = lane < m.CH ? lane : m.CH - 1;
  c.cpre = dot_t(A.wt + m.c0w, m.CH, jc, x0, m.D, A.params[m.c0b + jc]);
  c.kept = keep_unit(A, b, TKEY_START, NET_COV, lane);
  float a = fmaxf(c.cpre, 0.0f);
  if (A.drop) a = c.kept ? a * A.dc.inv_keep : 0.0f;
  c.ad = lane < m.CH ? a : 0.0f;
  const int hc = lane < m.H ? lane : m.H - 1;
  const float z = dot_t(A.wt + m.c3w, m.H, hc, c.ad, m.CH, A.params[m.c3b + hc]);
  return lane < m.H ? tanh_f(z) : 0.0f;
}

// the cell's three pre-activation sums from the LDS table; x* = lin_x(p) or 0
struct Gates { float r, z, u; };
NJ_DEV void lin_x(const GArgs& A, float p, int lane, float& xr, float& xz, float& xh) {
  const GModel& m = A.m;
  xr = xz = xh = 0.0f;
  if (!m.impute) return;
  const int hc = lane < m.H ? lane : m.H - 1;
  const float* wt = A.wt + m.lxw;
  const int n3 = 3 * m.H;
  xr = A.params[m.lxb + hc];
  xz = A.params[m.lxb + m.H + hc];
  xh = A.params[m.lxb + 2 * m.H + hc];
  for (int i = 0; i < m.D2; ++i) {
    const float pi = bcast(p, i);
    xr = fmaf(wt[(size_t)i * n3 + hc], pi, xr);
    xz = fmaf(wt[(size_t)i * n3 + m.H + hc], pi, xz);
    xh = fmaf(wt[(size_t)i * n3 + 2 * m.H + hc], pi, xh);
  }
}
NJ_DEV Gates cell_gates(const GModel& m, const float* tbl, float h, float xr, float xz, float xh, int lane) {
  const int H = m.H, HS = m.HS;
  const int hc = lane < H ? lane : H - 1;
  const float* tr = tbl + hc * HS;
  const float* tz = tr + H * HS;
  const float* th = tz + H * HS;
  float ar = xr, az = xz;
  int i = 0;
  for (; i + 4 <= H; i += 4) {   // (eight LDS reads in flight per round; the sums keep their order)
    const float r0 = tr[i], r1 = tr[i + 1], r2 = tr[i + 2], r3 = tr[i + 3];
    const float z0 = tz[i], z1 = tz[i + 1], z2 = tz[i + 2], z3 = tz[i + 3];
    const float h0 = bcast(h, i), h1 = bcast(h, i + 1), h2 = bcast(h, i + 2), h3 = bcast(h, i + 3);
    ar = fmaf(r0, h0, ar); az = fmaf(z0, h0, az);
    ar = fmaf(r1, h1, ar); az = fmaf(z1, h1, az);
    ar = fmaf(r2, h2, ar); az = fmaf(z2, h2, az);
    ar = fmaf(r3, h3, ar); az = fmaf(z3, h3, az);
  }
  for (; i < H; ++i) {
    const float hi = bcast(h, i);
    ar = fmaf(tr[i], hi, ar);
    az = fmaf(tz[i], hi, az);
  }
  Gates g;
  g.r = sigmoid_f(ar);
  g.z = sigmoid_f(az);
  const float q = lane < H ? g.r * h : 0.0f;
  float au = xh;
  for (i = 0; i + 4 <= H; i += 4) {
    const float u0 = th[i], u1 = th[i + 1], u2 = th[i + 2], u3 = th[i + 3];
    au = fmaf(u0, bcast(q, i), au);
    au = fmaf(u1, bcast(q, i + 1), au);
    au = fmaf(u2, bcast(q, i + 2), au);
    au = fmaf(u3, bcast(q, i + 3), au);
  }
  for (; i < H; ++i) au = fmaf(th[i], bcast(q, i), au);
  g.u = tanh_f(au);
  return g;
}
// table rows: [hr | hz | hh], each [H][HS]
NJ_DEV void fill_table(const GArgs& A, float* tbl, int lane) {
  const GModel& m = A.m;
  const int HH = m.H * m.H;
  const int src[3] = {m.hr, m.hz, m.hh};
  for (int q = 0; q < 3; ++q)
    for (int e = lane; e < HH; e += 64) {
      const int j = e / m.H, i = e - j * m.H;
      tbl[q * m.H * m.HS + j * m.HS + i] = A.params[src[q] + e];
    }
  wave_lds_sync();
}

// what a jump computes from (p, X, M, h), kept for its adjoint
struct Jump {
  float X, Mk, mean, lv, sig, err;   // lane f < D
  float pre[4], g[4];                // prep units e = lane + 64 q
  float gir, giz, gin, ghr, ghz, ghn, r, z, n;
};
NJ_DEV float jump_fwd(const GArgs& A, int row, float p, float h, int lane, Jump& J) {
  const GModel& m = A.m;
  const int D = m.D, H = m.H;
  const bool fon = lane < D;
  J.X = fon ? A.X[(size_t)row * D + lane] : 0.0f;
  J.Mk = fon ? A.M[(size_t)row * D + lane] : 0.0f;
  J.mean = fon ? p : 0.0f;
  J.lv = __shfl(p, fon ? lane + D : lane);
  if (!fon) J.lv = 0.0f;
  J.sig = expf(0.5f * J.lv);
  J.err = (J.X - J.mean) / J.sig;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = lane + 64 * q;
    const bool on = e < m.NG;
    const int f = on ? e / m.PR : 0, j = on ? e - f * m.PR : 0;
    const float xf = __shfl(J.X, f), mf = __shfl(J.mean, f), lf = __shfl(J.lv, f), ef = __shfl(J.err, f);
    const float mk = __shfl(J.Mk, f);
    const float* w = A.params + m.wp + (size_t)f * 4 * m.PR + j;
    float s = xf * w[0];
    s = fmaf(mf, w[m.PR], s);
    s = fmaf(lf, w[2 * m.PR], s);
    s = fmaf(ef, w[3 * m.PR], s);
    s += A.params[m.bp + f * m.PR + j];
    J.pre[q] = on ? s : 0.0f;
    J.g[q] = on ? fmaxf(s, 0.0f) * mk : 0.0f;
  }
  const int hc = lane < H ? lane : H - 1;
  const int n3 = 3 * H;
  J.gir = A.params[m.bih + hc];
  J.giz = A.params[m.bih + H + hc];
  J.gin = A.params[m.bih + 2 * H + hc];
  const float* wi = A.wt + m.wih;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = m.NG - 64 * q < 64 ? m.NG - 64 * q : 64;
    for (int i = 0; i < n; ++i) {
      const float gv = bcast(J.g[q], i);
      const float* w = wi + (size_t)(64 * q + i) * n3 + hc;
      J.gir = fmaf(w[0], gv, J.gir);
      J.giz = fmaf(w[H], gv, J.giz);
      J.gin = fmaf(w[2 * H], gv, J.gin);
    }
  }
  J.ghr = A.params[m.bhh + hc];
  J.ghz = A.params[m.bhh + H + hc];
  J.ghn = A.params[m.bhh + 2 * H + hc];
  const float* wh = A.wt + m.whh;
  for (int i = 0; i < H; ++i) {
    const float hv = bcast(h, i);
    const float* w = wh + (size_t)i * n3 + hc;
    J.ghr = fmaf(w[0], hv, J.ghr);
    J.ghz = fmaf(w[H], hv, J.ghz);
    J.ghn = fmaf(w[2 * H], hv, J.ghn);
  }
  J.r = sigmoid_f(J.gir + J.ghr);
  J.z = sigmoid_f(J.giz + J.ghz);
  J.n = tanh_f(J.gin + J.r * J.ghn);
  const float hn = J.n + J.z * (h - J.n);
  return lane < H ? hn : 0.0f;
}

// sum over lanes f < n of v, in lane order, in double
NJ_DEV double lane_sum(float v, int n) {
  double s = 0.0;
  for (int f = 0; f < n; ++f) s += (double)bcast(v, f);
  return s;
}

// key of the mask p carries at schedule position (k Euler steps done, time slices < i_hi done):
// the last event before it
NJ_DEV void prev_key(const int* __restrict__ k_jump, int i_hi, int k, uint32_t& net, uint32_t& tkey) {
  if (i_hi > 0 && k_jump[i_hi - 1] >= k) { net = NET_P_JUMP; tkey = (uint32_t)k_jump[i_hi - 1]; }
  else if (k > 0) { net = NET_P; tkey = (uint32_t)(k - 1); }
  else { net = NET_P; tkey = TKEY_START; }
}

__global__ void __launch_bounds__(64) k_gob_fwd(const GArgs A) {
  const GModel& m = A.m;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int B = A.B, D = m.D, H = m.H, D2 = m.D2;
  float* tbl = gob_smem;
  fill_table(A, tbl, lane);
  const bool want_path = A.flags & NJODE_C_RETURN_PATH, save = A.flags & NJODE_C_SAVE_BWD;
  const bool eager = want_path || m.impute;

  Cov cv;
  const float x0 = lane < D ? A.start_X[(size_t)b * D + lane] : 0.0f;
  float h = cov_fwd(A, x0, b, lane, cv);
  float p = 0.0f;
  bool p_valid = false;
  uint32_t p_net = NET_P, p_tkey = TKEY_START;
  double l1 = 0.0, l2 = 0.0;
  size_t row = 0;

  auto event_done = [&](uint32_t net, uint32_t tkey, bool force) {
    p_net = net; p_tkey = tkey; p_valid = false;
    if (eager || force) { p = pm_fwd(A, h, net, tkey, b, lane).p; p_valid = true; }
  };
  auto record = [&]() {
    if (!want_path) return;
    if (lane < H) A.path_h[(row * B + b) * H + lane] = h;
    if (lane < D2) A.path_p[(row * B + b) * D2 + lane] = p;
    ++row;
  };
  event_done(NET_P, TKEY_START, false);
  record();

  auto step = [&](int k) {
    const float dt = A.step_dt[k];   // (loaded first: its latency hides behind the gates)
    float xr, xz, xh;
    lin_x(A, p, lane, xr, xz, xh);
    const Gates g = cell_gates(m, tbl, h, xr, xz, xh, lane);
    if (save && lane < H) A.h_step[((size_t)k * B + b) * H + lane] = h;
    const float dh = (1.0f - g.z) * (g.u - h);
    h = lane < H ? h + dt * dh : 0.0f;
    event_done(NET_P, (uint32_t)k, false);
    record();
  };
  auto slice = [&](int i, int kj) {
    const int r = A.row_of[(size_t)i * B + b];
    if (r >= 0) {
      if (!p_valid) p = pm_fwd(A, h, p_net, p_tkey, b, lane).p;
      if (save && lane < H) A.h_bj[(size_t)r * H + lane] = h;
      Jump J;
      h = jump_fwd(A, r, p, h, lane, J);
      const float t1 = lane < D ? 0.5f * (J.err * J.err + J.lv + 1.8378770664093453f) * J.Mk : 0.0f;
      l1 += lane_sum(t1, D);
      event_done(NET_P_JUMP, (uint32_t)kj, true);
      // KL(N(mean', s'^2) || N(X, 0.01^2)) (models_gru_ode_bayes.py:561-575)
      float lv2 = __shfl(p, lane < D ? lane + D : lane);
      const float sd = expf(0.5f * lv2), df = p - J.X;
      const float kl = (-4.605170185988091f - logf(sd)) + (sd * sd + df * df) / 2.0e-4f - 0.5f;
      l2 += lane_sum(lane < D ? kl * J.Mk : 0.0f, D);
    } else {
      event_done(NET_P_JUMP, (uint32_t)kj, false);
    }
    record();
  };

  int k = 0;
  const int K = A.K;
  for (int i = 0; i < A.nt; ++i) {
    int kj = A.k_jump[i];
    kj = kj < 0 ? 0 : (kj > K ? K : kj);
    for (; k < kj; ++k) step(k);
    slice(i, kj);
  }
  for (; k < K; ++k) step(k);

  if (lane < H) {
    A.hT[(size_t)b * H + lane] = h;
    if (save) A.h_end[(size_t)b * H + lane] = h;
  }
  if (lane == 0) {
    A.loss_part[b] = l1;
    A.loss_part[B + b] = l2;
  }
}

__global__ void __launch_bounds__(64) k_gob_bwd(const GArgs A) {
  const GModel& m = A.m;
  const int lane = threadIdx.x;
  const int B = A.B, D = m.D, H = m.H, D2 = m.D2, HS = m.HS, K = A.K;
  float* tbl = gob_smem;
  float* acc = gob_smem + 3 * H * HS;   // [hr | hz | hh] gradients, [H][H] each
  fill_table(A, tbl, lane);
  for (int e = lane; e < 3 * H * H; e += 64) acc[e] = 0.0f;
  wave_lds_sync();
  float* slab = A.slabs + (size_t)blockIdx.x * m.P;
  const float c1 = A.grad_loss[0] + A.grad_loss_1[0];   // on the terms of loss_1
  const float c2 = A.grad_loss[0] * A.mixing;           // on the terms of loss_2
  const int hc = lane < H ? lane : H - 1;
  const bool hon = lane < H;

  for (int b = blockIdx.x; b < B; b += A.S) {
    float lam = (A.grad_hT && hon) ? A.grad_hT[(size_t)b * H + lane] : 0.0f;
    float lp = 0.0f;        // adjoint of p (lane c < 2 D)
    bool live = false;      // ... is not zero
    float hcur = hon ? A.h_end[(size_t)b * H + lane] : 0.0f;

    // the event that produced p from hcur: its p_model, backwards
    auto p_part = [&](uint32_t net, uint32_t tkey) {
      if (!live) return;
      const PMv v = pm_fwd(A, hcur, net, tkey, b, lane);
      lam += pm_bwd(A, slab, v, hcur, lp, lane);
      lp = 0.0f;
      live = false;
    };

    auto step = [&](int k, int i_hi) {
      p_part(NET_P, (uint32_t)k);
      const float hp = hon ? A.h_step[((size_t)k * B + b) * H + lane] : 0.0f;
      float pprev = 0.0f, xr, xz, xh;
      if (m.impute) {
        uint32_t net, tkey;
        prev_key(A.k_jump, i_hi, k, net, tkey);
        pprev = pm_fwd(A, hp, net, tkey, b, lane).p;
      }
      lin_x(A, pprev, lane, xr, xz, xh);
      const Gates g = cell_gates(m, tbl, hp, xr, xz, xh, lane);
      const float dt = A.step_dt[k];
      const float q = hon ? g.r * hp : 0.0f;
      const float du = lam * dt * (1.0f - g.z);
      const float dz = -lam * dt * (g.u - hp);
      float lnew = lam * (1.0f - dt * (1.0f - g.z));
      const float dau = hon ? du * (1.0f - g.u * g.u) : 0.0f;
      const float daz = hon ? dz * g.z * (1.0f - g.z) : 0.0f;
      // d q = W_hh^T d a_u (column = this lane: conflict-free with the odd row stride)
      float dq = 0.0f;
      const float* th = tbl + 2 * H * HS + hc;
      {
        int j = 0;
        for (; j + 4 <= H; j += 4) {
          const float w0 = th[j * HS], w1 = th[(j + 1) * HS], w2 = th[(j + 2) * HS], w3 = th[(j + 3) * HS];
          dq = fmaf(w0, bcast(dau, j), dq);
          dq = fmaf(w1, bcast(dau, j + 1), dq);
          dq = fmaf(w2, bcast(dau, j + 2), dq);
          dq = fmaf(w3, bcast(dau, j + 3), dq);
        }
        for (; j < H; ++j) dq = fmaf(th[j * HS], bcast(dau, j), dq);
      }
      const float dar = hon ? dq * hp * g.r * (1.0f - g.r) : 0.0f;
      lnew = fmaf(dq, g.r, lnew);
      float dhh = 0.0f;
      const float* tr = tbl + hc;
      const float* tz = tbl + H * HS + hc;
      float* gr = acc + hc;
      float* gz = acc + H * H + hc;
      float* gh = acc + 2 * H * H + hc;
      int j = 0;
      for (; j + 2 <= H; j += 2) {   // (ten LDS reads in flight per round; sums and updates keep their order)
        const float ar0 = bcast(dar, j), az0 = bcast(daz, j), au0 = bcast(dau, j);
        const float ar1 = bcast(dar, j + 1), az1 = bcast(daz, j + 1), au1 = bcast(dau, j + 1);
        const float wr0 = tr[j * HS], wz0 = tz[j * HS], wr1 = tr[(j + 1) * HS], wz1 = tz[(j + 1) * HS];
        if (hon) {
          const float a0 = gr[j * H], b0 = gz[j * H], c0 = gh[j * H];
          const float a1 = gr[(j + 1) * H], b1 = gz[(j + 1) * H], c1v = gh[(j + 1) * H];
          gr[j * H] = fmaf(ar0, hp, a0);
          gz[j * H] = fmaf(az0, hp, b0);
          gh[j * H] = fmaf(au0, q, c0);
          gr[(j + 1) * H] = fmaf(ar1, hp, a1);
          gz[(j + 1) * H] = fmaf(az1, hp, b1);
          gh[(j + 1) * H] = fmaf(au1, q, c1v);
        }
        dhh = fmaf(wr0, ar0, dhh);
        dhh = fmaf(wz0, az0, dhh);
        dhh = fmaf(wr1, ar1, dhh);
        dhh = fmaf(wz1, az1, dhh);
      }
      for (; j < H; ++j) {
        const float ar = bcast(dar, j), az = bcast(daz, j), au = bcast(dau, j);
        dhh = fmaf(tr[j * HS], ar, dhh);
        dhh = fmaf(tz[j * HS], az, dhh);
        if (hon) {
          gr[j * H] = fmaf(ar, hp, gr[j * H]);
          gz[j * H] = fmaf(az, hp, gz[j * H]);
          gh[j * H] = fmaf(au, q, gh[j * H]);
        }
      }
      lam = hon ? lnew + dhh : 0.0f;
      if (m.impute) {   // x = lin_x(p): rows [r | z | h] of lin_x get [d a_r | d a_z | d a_u]
        const int n2 = D2;
        const bool on = lane < n2;
        const int ic = on ? lane : n2 - 1;
        float dp = 0.0f;
        const float dx[3] = {dar, daz, dau};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          outer_add(slab + m.lxw + c * H * n2, n2, lane, on, dx[c], H, pprev);
          if (hon) slab[m.lxb + c * H + lane] += dx[c];
          dp = dot_in(A.params + m.lxw + c * H * n2, n2, ic, dx[c], H, dp);
        }
        lp = on ? dp : 0.0f;
        live = true;
      }
      hcur = hp;
    };

    auto slice = [&](int i, int kj) {
      const int r = A.row_of[(size_t)i * B + b];
      if (r < 0) {
        p_part(NET_P_JUMP, (uint32_t)kj);
        return;
      }
      const float hp = hon ? A.h_bj[(size_t)r * H + lane] : 0.0f;
      uint32_t net, tkey;
      prev_key(A.k_jump, i, kj, net, tkey);
      const float pprev = pm_fwd(A, hp, net, tkey, b, lane).p;
      Jump J;
      jump_fwd(A, r, pprev, hp, lane, J);   // (its result is hcur)
      {   // loss_2 on p' = p_model(hcur), then that p_model backwards
        const PMv v = pm_fwd(A, hcur, NET_P_JUMP, (uint32_t)kj, b, lane);
        const int f = lane < D ? lane : (lane < D2 ? lane - D : 0);
        const float xf = __shfl(J.X, f), mk = __shfl(J.Mk, f);
        float add = 0.0f;
        if (lane < D) add = (v.p - xf) / 1.0e-4f * mk;
        else if (lane < D2) { const float sd = expf(0.5f * v.p); add = (sd * sd / 2.0e-4f - 0.5f) * mk; }
        lp = fmaf(c2, add, lp);
        lam += pm_bwd(A, slab, v, hcur, lp, lane);
        lp = 0.0f;
      }
      // GRUCell, backwards
      const float dn = lam * (1.0f - J.z);
      const float dz = lam * (hp - J.n);
      float lnew = lam * J.z;
      const float dan = hon ? dn * (1.0f - J.n * J.n) : 0.0f;
      const float dr = dan * J.ghn;
      const float dar = hon ? dr * J.r * (1.0f - J.r) : 0.0f;
      const float daz = hon ? dz * J.z * (1.0f - J.z) : 0.0f;
      const float dgi[3] = {dar, daz, dan};
      const float dgh[3] = {dar, daz, hon ? dan * J.r : 0.0f};
      float dg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      float dhh = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = lane + 64 * q;
          const bool on = e < m.NG;
          if (64 * q < m.NG) {
            outer_add(slab + m.wih + (size_t)c * H * m.NG, m.NG, e, on, dgi[c], H, J.g[q]);
            dg[q] = dot_in(A.params + m.wih + (size_t)c * H * m.NG, m.NG, on ? e : m.NG - 1, dgi[c], H, dg[q]);
          }
        }
        outer_add(slab + m.whh + c * H * H, H, lane, hon, dgh[c], H, hp);
        dhh = dot_in(A.params + m.whh + c * H * H, H, hc, dgh[c], H, dhh);
        if (hon) {
          slab[m.bih + c * H + lane] += dgi[c];
          slab[m.bhh + c * H + lane] += dgh[c];
        }
      }
      lam = hon ? lnew + dhh : 0.0f;
      // prep layer, backwards: per feature f the adjoints of (mean, logvar, err)
      float dmean = 0.0f, dlv = 0.0f, derr = 0.0f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = lane + 64 * q;
        const bool on = e < m.NG;
        const int f = on ? e / m.PR : 0, j = on ? e - f * m.PR : 0;
        const float xf = __shfl(J.X, f), mf = __shfl(J.mean, f), lf = __shfl(J.lv, f), ef = __shfl(J.err, f);
        const float mk = __shfl(J.Mk, f);
        const float dpre = (on && J.pre[q] > 0.0f) ? dg[q] * mk : 0.0f;
        float t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
        if (on) {
          float* gw = slab + m.wp + (size_t)f * 4 * m.PR + j;
          const float* w = A.params + m.wp + (size_t)f * 4 * m.PR + j;
          gw[0] = fmaf(dpre, xf, gw[0]);
          gw[m.PR] = fmaf(dpre, mf, gw[m.PR]);
          gw[2 * m.PR] = fmaf(dpre, lf, gw[2 * m.PR]);
          gw[3 * m.PR] = fmaf(dpre, ef, gw[3 * m.PR]);
          slab[m.bp + f * m.PR + j] += dpre;
          t1 = dpre * w[m.PR];
          t2 = dpre * w[2 * m.PR];
          t3 = dpre * w[3 * m.PR];
        }
        // sum over the units j of feature f, in unit order (a chunk holds units 64 q ... 64 q + 63)
        if (64 * q < m.NG) {
          const int f_lo = (64 * q) / m.PR;
          const int e_hi = m.NG < 64 * q + 64 ? m.NG : 64 * q + 64;
          const int f_hi = (e_hi - 1) / m.PR;
          for (int ff = f_lo; ff <= f_hi; ++ff) {
            const int e0 = ff * m.PR > 64 * q ? ff * m.PR : 64 * q;
            const int e1 = (ff + 1) * m.PR < e_hi ? (ff + 1) * m.PR : e_hi;
            float s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
            for (int ee = e0; ee < e1; ++ee) {
              s1 += bcast(t1, ee - 64 * q);
              s2 += bcast(t2, ee - 64 * q);
              s3 += bcast(t3, ee - 64 * q);
            }
            if (lane == ff) { dmean += s1; dlv += s2; derr += s3; }
          }
        }
      }
      if (lane < D) {
        derr = fmaf(c1 * J.Mk, J.err, derr);       // loss_1: err is not detached
        dlv = fmaf(c1 * J.Mk, 0.5f, dlv);
        dmean -= derr / J.sig;                     // err = (X - mean) exp(-logvar / 2)
        dlv = fmaf(-0.5f * derr, J.err, dlv);
      } else {
        dmean = dlv = 0.0f;
      }
      const float up = __shfl(dlv, lane >= D && lane < D2 ? lane - D : 0);
      lp = lane < D ? dmean : (lane < D2 ? up : 0.0f);
      live = true;
      hcur = hp;
    };

    int k = K;
    for (int i = A.nt - 1; i >= 0; --i) {
      int kj = A.k_jump[i];
      kj = kj < 0 ? 0 : (kj > K ? K : kj);
      while (k > kj) { --k; step(k, i + 1); }
      slice(i, kj);
    }
    while (k > 0) { --k; step(k, 0); }

    // the start: p_model at h0, then covariates_map
    p_part(NET_P, TKEY_START);
    Cov cv;
    const float x0 = lane < D ? A.start_X[(size_t)b * D + lane] : 0.0f;
    const float h0 = cov_fwd(A, x0, b, lane, cv);
    const float d3 = hon ? lam * (1.0f - h0 * h0) : 0.0f;
    outer_add(slab + m.c3w, m.CH, lane, lane < m.CH, d3, H, cv.ad);
    if (hon) slab[m.c3b + lane] += d3;
    float da = dot_in(A.params + m.c3w, m.CH, lane < m.CH ? lane : m.CH - 1, d3, H, 0.0f);
    if (A.drop) da = cv.kept ? da * A.dc.inv_keep : 0.0f;
    const float d0 = (lane < m.CH && cv.cpre > 0.0f) ? da : 0.0f;
    outer_add(slab + m.c0w, D, lane, lane < D, d0, m.CH, x0);
    if (lane < m.CH) slab[m.c0b + lane] += d0;
  }

  wave_lds_sync();
  const int HH = H * H;
  for (int e = lane; e < HH; e += 64) {
    slab[m.hr + e] = acc[e];
    slab[m.hz + e] = acc[HH + e];
    slab[m.hh + e] = acc[2 * HH + e];
  }
}

// loss = {loss_1 + mixing loss_2, loss_1}: the paths' terms in a fixed tree
__global__ void k_gob_loss(const double* __restrict__ part, int B, float mixing, float* loss) {
  double sum[2];
  tree_sum_256<2>(part, B, B, sum);
  if (threadIdx.x == 0) {
    loss[0] = (float)(sum[0] + (double)mixing * sum[1]);
    loss[1] = (float)sum[0];
  }
}

// ---- host ----------------------------------------------------------------------------------------

bool build_model(const NjodeGobDims* d, GModel& m) {
  memset(&m, 0, sizeof(m));
  if (!d) { fail(NJODE_E_UNSUPPORTED, "GRU-ODE-Bayes: null dims"); return false; }
  const int D = d->input_size, H = d->hidden_size, PH = d->p_hidden, PR = d->prep_hidden, CH = d->cov_hidden;
  if (D < 1 || H < 1 || PH < 1 || PR < 1 || CH < 1) {
    fail(NJODE_E_UNSUPPORTED, "GRU-ODE-Bayes: sizes must be positive");
    return false;
  }
  if (d->flags & ~(NJODE_GOB_F_BIAS | NJODE_GOB_F_IMPUTE)) {
    fail(NJODE_E_UNSUPPORTED, "GRU-ODE-Bayes: unknown model flag");
    return false;
  }
  if (H > 64 || PH > 64 || CH > 64 || 2 * D > 64) {
    fail(NJODE_E_UNSUPPORTED,
         "GRU-ODE-Bayes: a lane per unit needs hidden_size, p_hidden, cov_hidden and 2 * input_size <= 64 "
         "(got %d, %d, %d, %d)", H, PH, CH, 2 * D);
    return false;
  }
  if ((long long)PR * D > 256) {
    fail(NJODE_E_UNSUPPORTED, "GRU-ODE-Bayes: prep_hidden * input_size = %lld exceeds 256", (long long)PR * D);
    return false;
  }
  m.D = D; m.H = H; m.PH = PH; m.PR = PR; m.CH = CH;
  m.NG = PR * D; m.D2 = 2 * D; m.HS = H | 1;
  m.impute = (d->flags & NJODE_GOB_F_IMPUTE) ? 1 : 0;
  int o = 0, t = 0;
  auto mat = [&](int& w, int n_out, int n_in, bool transposed) {
    w = o;
    if (transposed) { m.t_off[t] = o; m.t_out[t] = n_out; m.t_in[t] = n_in; ++t; }
    o += n_out * n_in;
  };
  auto vec = [&](int& v, int n) { v = o; o += n; };
  mat(m.p0w, PH, H, true); vec(m.p0b, PH);
  mat(m.p3w, m.D2, PH, true); vec(m.p3b, m.D2);
  if (m.impute) { mat(m.lxw, 3 * H, m.D2, true); vec(m.lxb, 3 * H); }
  mat(m.hh, H, H, false); mat(m.hz, H, H, false); mat(m.hr, H, H, false);
  vec(m.wp, D * 4 * PR); vec(m.bp, D * PR);
  mat(m.wih, 3 * H, m.NG, true); mat(m.whh, 3 * H, H, true); vec(m.bih, 3 * H); vec(m.bhh, 3 * H);
  mat(m.c0w, CH, D, true); vec(m.c0b, CH);
  mat(m.c3w, H, CH, true); vec(m.c3b, H);
  m.P = o;
  return true;
}

// the matrices the forward reads transposed (GModel keeps its own lists: it is a kernel argument
// of the walk and the sweep, whose layout stays as it is)
MatTable transposed_matrices(const GModel& m) {
  MatTable t = {};
  for (int i = 0; i < NMAT; ++i) t.add(m.t_off[i], m.t_out[i], m.t_in[i]);
  return t;
}

struct Layout : Arena {
  size_t sched, wt, row_of, loss_part, h_step, h_bj, h_end, slabs;
  int S;
};

Layout make_layout(const GModel& m, int B, int n_obs, int nt, int K, int flags) {
  Layout L;
  const size_t b = B, no = at_least_1(n_obs), k = at_least_1(K), t = at_least_1(nt);
  L.sched = L.take(((size_t)2 * K + 3 * (size_t)nt + 1) * 4);
  L.wt = L.take((size_t)m.P * 4);
  L.row_of = L.take(t * b * 4);
  L.loss_part = L.take(2 * b * 8);
  L.S = slab_count((size_t)m.P * 4, SLAB_BUDGET, MAX_SLABS, B);
  L.h_step = L.h_bj = L.h_end = L.slabs = 0;
  if (flags & NJODE_C_SAVE_BWD) {
    L.h_step = L.take(k * b * m.H * 4);
    L.h_bj = L.take(no * m.H * 4);
    L.h_end = L.take(b * m.H * 4);
    L.slabs = L.take((size_t)L.S * m.P * 4);
  }
  return L;
}

constexpr int KNOWN_FLAGS = NJODE_C_TRAIN | NJODE_C_RETURN_PATH | NJODE_C_SAVE_BWD;
constexpr const char* BAD_FLAG = "call flag the GRU-ODE-Bayes calls do not take";

// every refusal a call makes before it launches anything (array contents: the host schedule only)
int check_gob(const NjodeBatch* b, const NjodeSchedule* s, int flags, const float* params, const void* ws,
              float dropout_p, bool forward) {
  if (int rc = check_sizes_and_params(b, s, flags, KNOWN_FLAGS, BAD_FLAG, params)) return rc;
  const int n_obs = b->n_obs, nt = s->n_times;
  if (!b->start_X || (n_obs > 0 && (!b->X || !b->obs_idx || !b->M))) return fail(NJODE_E_BADARG, "null batch array");
  if (n_obs > 0 && nt == 0) return fail(NJODE_E_BADARG, "observation rows without observation times");
  if (!(dropout_p >= 0.0f && dropout_p < 1.0f)) return fail(NJODE_E_BADARG, "dropout_p");
  if (int rc = check_workspace_ptr(ws)) return rc;
  return forward ? check_schedule_walk(s, n_obs) : NJODE_OK;
}

void fill_args(GArgs& A, const GModel& m, const Layout& L, char* ws, const NjodeBatch* b, const NjodeSchedule* s,
               int flags, float mixing, float dropout_p, uint64_t seed, const float* params) {
  memset(&A, 0, sizeof(A));
  A.m = m;
  A.B = b->batch_size; A.n_obs = b->n_obs; A.nt = s->n_times; A.K = s->n_steps;
  A.flags = flags; A.S = L.S;
  A.drop = ((flags & NJODE_C_TRAIN) && dropout_p > 0.0f) ? 1 : 0;
  A.dc = make_drop_ctx(dropout_p, seed, A.drop != 0).dc;
  A.mixing = mixing;
  A.params = params;
  A.wt = (const float*)(ws + L.wt);
  A.start_X = b->start_X; A.X = b->X; A.M = b->M; A.obs_idx = b->obs_idx;
  const size_t K = s->n_steps, nt = s->n_times;
  A.step_dt = (const float*)(ws + L.sched);
  A.k_jump = (const int*)(ws + L.sched) + 2 * K;
  A.time_ptr = (const int*)(ws + L.sched) + 2 * K + 2 * nt;
  A.row_of = (int*)(ws + L.row_of);
  A.loss_part = (double*)(ws + L.loss_part);
  if (flags & NJODE_C_SAVE_BWD) {
    A.h_step = (float*)(ws + L.h_step);
    A.h_bj = (float*)(ws + L.h_bj);
    A.h_end = (float*)(ws + L.h_end);
    A.slabs = (float*)(ws + L.slabs);
  }
}

}  // namespace

extern "C" int njode_gob_supported(const NjodeGobDims* dims) {
  GModel m;
  return build_model(dims, m) ? 1 : 0;
}

extern "C" size_t njode_gob_param_count(const NjodeGobDims* dims) {
  GModel m;
  return build_model(dims, m) ? (size_t)m.P : 0;
}

extern "C" int njode_gob_workspace_bytes(const NjodeGobDims* dims, int32_t B, int32_t n_obs, int32_t nt,
                                         int32_t K, int32_t call_flags, size_t* out) {
  GModel m;
  if (!build_model(dims, m)) return NJODE_E_UNSUPPORTED;
  if (!out || B <= 0 || n_obs < 0 || nt < 0 || K < 0) return fail(NJODE_E_BADARG, "bad size");
  if (call_flags & ~KNOWN_FLAGS) return fail(NJODE_E_BADARG, "%s", BAD_FLAG);
  *out = make_layout(m, B, n_obs, nt, K, call_flags).total;
  return NJODE_OK;
}

extern "C" int njode_gob_forward_f32(const NjodeGobDims* dims, const float* params, const NjodeBatch* b,
                                     const NjodeSchedule* s, int32_t flags, float mixing, float dropout_p,
                                     uint64_t seed, float* hT, float* loss, float* path_h, float* path_p,
                                     void* workspace, size_t ws_bytes, njodeStream_t st) {
  GModel m;
  if (!build_model(dims, m)) return NJODE_E_UNSUPPORTED;
  int rc = check_gob(b, s, flags, params, workspace, dropout_p, true);
  if (rc) return rc;
  if (!hT || !loss) return fail(NJODE_E_BADARG, "null output");
  if ((flags & NJODE_C_RETURN_PATH) && (!path_h || !path_p)) return fail(NJODE_E_BADARG, "null output");
  const int B = b->batch_size, n_obs = b->n_obs, nt = s->n_times, K = s->n_steps;
  const Layout L = make_layout(m, B, n_obs, nt, K, flags);
  if ((rc = check_workspace_size(ws_bytes, L.total))) return rc;
  char* ws = (char*)workspace;
  const int lds = 3 * m.H * m.HS * 4;
  if ((rc = set_lds((const void*)k_gob_fwd, lds))) return rc;
  if ((rc = upload_schedule(ws + L.sched, s, st))) return rc;

  GArgs A;
  fill_args(A, m, L, ws, b, s, flags, mixing, dropout_p, seed, params);
  A.hT = hT;
  A.path_h = path_h;
  A.path_p = path_p;
  transpose_weights(transposed_matrices(m), m.P, params, (float*)(ws + L.wt), "k_gob_transpose", st);
  build_row_table(A.row_of, b->obs_idx, A.time_ptr, n_obs, nt, B, "k_gob_rows", st);
  {
    ProfScope ps("k_gob_fwd", st);
    k_gob_fwd<<<B, 64, lds, st>>>(A);
  }
  {
    ProfScope ps("k_gob_loss", st);
    k_gob_loss<<<1, 256, 0, st>>>(A.loss_part, B, mixing, loss);
  }
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}

extern "C" int njode_gob_backward_f32(const NjodeGobDims* dims, const float* params, const NjodeBatch* b,
                                      const NjodeSchedule* s, int32_t flags, float mixing, float dropout_p,
                                      uint64_t seed, const float* grad_loss, const float* grad_loss_1,
                                      const float* grad_hT, float* grad_params, void* workspace,
                                      size_t ws_bytes, njodeStream_t st) {
  GModel m;
  if (!build_model(dims, m)) return NJODE_E_UNSUPPORTED;
  int rc = check_gob(b, s, flags, params, workspace, dropout_p, false);
  if (rc) return rc;
  if (!(flags & NJODE_C_SAVE_BWD)) return fail(NJODE_E_BADARG, "the backward needs the forward's NJODE_C_SAVE_BWD");
  if (!grad_params || !grad_loss || !grad_loss_1) return fail(NJODE_E_BADARG, "null gradient argument");
  const int B = b->batch_size, n_obs = b->n_obs, nt = s->n_times, K = s->n_steps;
  const Layout L = make_layout(m, B, n_obs, nt, K, flags);
  if ((rc = check_workspace_size(ws_bytes, L.total))) return rc;
  char* ws = (char*)workspace;
  const int lds = (3 * m.H * m.HS + 3 * m.H * m.H) * 4;
  if ((rc = set_lds((const void*)k_gob_bwd, lds))) return rc;
  GArgs A;
  fill_args(A, m, L, ws, b, s, flags, mixing, dropout_p, seed, params);
  A.grad_loss = grad_loss;
  A.grad_loss_1 = grad_loss_1;
  A.grad_hT = grad_hT;
  HIP_TRY(hipMemsetAsync(A.slabs, 0, (size_t)L.S * m.P * 4, st));
  {
    ProfScope ps("k_gob_bwd", st);
    k_gob_bwd<<<L.S, 64, lds, st>>>(A);
  }
  reduce_slabs(A.slabs, L.S, m.P, grad_params, "k_gob_reduce", st);
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}
