// njode_f64.hip -- the float64 route (include/njode_f64.h): NJ-ODE forward and exact discrete
// adjoint in double precision.  One plan: a workgroup per path walks the schedule in lockstep with
// the host clock; sizes are run-time values and threads loop over units.  Layer inputs live in
// LDS; the forward reads weights from a table transposed once per call into the workspace (lane j
// = output unit j reads consecutive doubles), the adjoint reads them in their own [out][in] order
// (lane i = input unit i).  Weight gradients: every workgroup of the sweep owns one slab of P
// doubles, adds delta (x) activation of its paths (path order, each element always by the same
// thread) and a last kernel sums the slabs in slab order -- no atomics, the same bits every time.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/njode_f64.h"
#include "njode_gen_host.h"
#include "njode_pathwalk.h"

using namespace njode;

namespace {

constexpr int MAXL = NJODE_MAX_HIDDEN + 1;
constexpr int LDS_LIMIT = 160 * 1024;
constexpr int MAX_SLABS = 2048;
constexpr size_t SLAB_BUDGET = (size_t)1 << 30;
constexpr double LOSS_EPS = 1e-10;

struct FLayer {
  int n_in, n_out, act;   // act: NJODE_ACT_* behind the layer, -1: none (the last one)
  int w_off, b_off;       // offsets into the flat parameter vector (doubles)
  int a_off;              // offset of this layer's input in the activation store
  int cw_log2;            // slab update: 2^cw_log2 lanes run along a weight row
};
struct FNet {
  int nl, n_in, n_out, act_total;
  FLayer l[MAXL];
};

struct FModel {
  int D, H, DO, masked, curt, loss_easy, IN0;
  int enc_case, enc_mult, dec_case, dec_mult;
  int maxv, act_max, nth, P;
  FNet ode, enc, dec;
};

struct FArgs {
  FModel m;
  int B, n_obs, nt, K, flags, S;
  double weight, lbs;
  const double *params, *wt;
  const double *start_X, *X, *M;
  const int *obs_idx, *n_obs_ot;
  // device copy of the schedule
  const double* step_dt;
  const float *step_t, *time_f32;
  const int *k_jump, *time_ptr;
  int* row_of;            // [nt][B] row of (time slice, path) or -1
  double *hT, *path_h, *path_y, *loss_part;
  // what the sweep reads back
  double *h_step, *h_bj, *x_prev, *x_end;
  float *tau_prev, *tau_end;
  const double *grad_loss, *grad_hT;
  double* slabs;
};

// ---- device ------------------------------------------------------------------------------------

extern __shared__ __attribute__((aligned(16))) char f64_smem[];

__device__ inline double act_fn(double v, int act) {
  if (act == NJODE_ACT_TANH) return tanh(v);
  if (act == NJODE_ACT_RELU) return v > 0.0 ? v : 0.0;
  return v;
}
// derivative of the activation from its OUTPUT a
__device__ inline double act_der(double a, int act) {
  if (act == NJODE_ACT_TANH) return 1.0 - a * a;
  if (act == NJODE_ACT_RELU) return a > 0.0 ? 1.0 : 0.0;
  return 1.0;
}

// One network on the input already written to a[l[0].a_off ...]: every layer's input stays in the
// activation store `a`; the last layer's output goes to `out` (skipped with with_last = false).
__device__ void net_fwd(const FNet& N, const double* __restrict__ wt, const double* __restrict__ params,
                        double* a, double* out, bool with_last) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int nl = with_last ? N.nl : N.nl - 1;
  for (int l = 0; l < nl; ++l) {
    const FLayer& L = N.l[l];
    const double* in = a + L.a_off;
    double* o = (l == N.nl - 1) ? out : a + N.l[l + 1].a_off;
    const int n_in = L.n_in, n_out = L.n_out;
    for (int j = tid; j < n_out; j += nth) {
      double acc = params[L.b_off + j];
      const double* w = wt + L.w_off + j;
#pragma unroll 16
      for (int i = 0; i < n_in; ++i) acc = fma(w[(size_t)i * n_out], in[i], acc);
      o[j] = act_fn(acc, L.act);
    }
    __syncthreads();
  }
}

// Adjoint of net_fwd.  d_cur holds the adjoint of the network's output; the two buffers alternate.
// Adds delta (x) input and delta to the slab; returns the buffer holding the adjoint of the
// network's input vector.
__device__ double* net_bwd(const FNet& N, const double* __restrict__ params, const double* a,
                           double* d_cur, double* d_other, double* __restrict__ slab) {
  const int tid = threadIdx.x, nth = blockDim.x;
  for (int l = N.nl - 1; l >= 0; --l) {
    const FLayer& L = N.l[l];
    const double* in = a + L.a_off;
    const int n_in = L.n_in, n_out = L.n_out;
    {
      const int cw = 1 << L.cw_log2, rows = nth >> L.cw_log2;
      const int i0 = tid & (cw - 1), j0 = tid >> L.cw_log2;
      for (int j = j0; j < n_out; j += rows) {
        const double dj = d_cur[j];
        double* g = slab + L.w_off + (size_t)j * n_in;
#pragma unroll 4
        for (int i = i0; i < n_in; i += cw) g[i] = fma(dj, in[i], g[i]);
      }
      for (int j = tid; j < n_out; j += nth) slab[L.b_off + j] += d_cur[j];
    }
    const int prev_act = l > 0 ? N.l[l - 1].act : -1;
    for (int i = tid; i < n_in; i += nth) {
      double acc = 0.0;
      const double* w = params + L.w_off + i;
#pragma unroll 16
      for (int j = 0; j < n_out; ++j) acc = fma(w[(size_t)j * n_in], d_cur[j], acc);
      d_other[i] = l > 0 ? acc * act_der(in[i], prev_act) : acc;
    }
    __syncthreads();
    double* t = d_cur;
    d_cur = d_other;
    d_other = t;
  }
  return d_cur;
}

// FFNN residual (models.py:261-276) of input x [n_in] at output unit j
__device__ inline double res_fwd(int cs, int mult, const double* x, int n_in, int n_out, int j) {
  if (cs == 1) return x[j % n_in];
  if (cs == 2) {
    double s = 0.0;
    for (int c = 0; c < mult; ++c) s += x[c * n_out + j];
    return s / (double)mult;
  }
  return 0.0;
}
// ... and its adjoint at input unit i, from the output adjoint g [n_out]
__device__ inline double res_bwd(int cs, int mult, const double* g, int n_in, int n_out, int i) {
  if (cs == 1) {
    double s = 0.0;
    for (int c = 0; c < mult; ++c) s += g[i + c * n_in];
    return s;
  }
  if (cs == 2) return g[i % n_out] / (double)mult;
  return 0.0;
}

// LDS vectors of one path
struct Lds {
  double *h, *lastX, *tlx, *xin, *y, *ybj, *tmpH, *tmpO, *act;
  double *lam, *lamx, *gY, *gYbj, *hn, *dA, *dB;   // sweep only
};
__device__ inline Lds carve(const FModel& m, bool bwd) {
  Lds s;
  double* p = (double*)f64_smem;
  const int HO = m.H > m.DO ? m.H : m.DO;
  s.h = p; p += m.H;
  s.lastX = p; p += m.D;
  s.tlx = p; p += m.D;
  s.xin = p; p += m.D;
  s.y = p; p += m.DO;
  s.ybj = p; p += m.DO;
  s.tmpH = p; p += m.H;
  s.tmpO = p; p += HO;
  s.act = p; p += m.act_max;
  if (bwd) {
    s.lam = p; p += m.H;
    s.lamx = p; p += m.D;
    s.gY = p; p += m.DO;
    s.gYbj = p; p += m.DO;
    s.hn = p; p += m.H;
    s.dA = p; p += m.maxv;
    s.dB = p; p += m.maxv;
  }
  return s;
}
inline int lds_doubles(const FModel& m, bool bwd) {
  const int HO = m.H > m.DO ? m.H : m.DO;
  int n = m.H + 3 * m.D + 2 * m.DO + m.H + HO + m.act_max;
  if (bwd) n += 2 * m.H + m.D + 2 * m.DO + 2 * m.maxv;
  return n;
}

// y = readout(h): tanh(h) -> net -> + residual of the raw h
__device__ void readout(const FArgs& A, const Lds& s, const double* h, double* y, bool with_last) {
  const FModel& m = A.m;
  for (int j = threadIdx.x; j < m.H; j += blockDim.x) s.act[j] = tanh(h[j]);
  __syncthreads();
  net_fwd(m.dec, A.wt, A.params, s.act, s.tmpO, with_last);
  if (with_last) {
    for (int j = threadIdx.x; j < m.DO; j += blockDim.x)
      y[j] = s.tmpO[j] + res_fwd(m.dec_case, m.dec_mult, h, m.H, m.DO, j);
    __syncthreads();
  }
}
// hnew = encoder(x [, mask]); mask == nullptr with a masked model: zeros (the start state)
__device__ void encode(const FArgs& A, const Lds& s, const double* x, const double* mask, double* hnew,
                       bool with_last) {
  const FModel& m = A.m;
  for (int d = threadIdx.x; d < m.D; d += blockDim.x) {
    s.act[d] = tanh(x[d]);
    if (m.masked) s.act[m.D + d] = mask ? mask[d] : 0.0;
  }
  __syncthreads();
  net_fwd(m.enc, A.wt, A.params, s.act, s.tmpH, with_last);
  if (with_last) {
    for (int j = threadIdx.x; j < m.H; j += blockDim.x)
      hnew[j] = s.tmpH[j] + res_fwd(m.enc_case, m.enc_mult, x, m.D, m.H, j);
    __syncthreads();
  }
}
// input of the ODE network for state h: [tanh(last_X), tanh(h), tau, tdiff (, tau + tdiff)]; the
// clock terms are fp32 arithmetic of the reference, widened exactly
__device__ void ode_input(const FArgs& A, const Lds& s, float tau, float t0) {
  const FModel& m = A.m;
  for (int d = threadIdx.x; d < m.D; d += blockDim.x) s.act[d] = s.tlx[d];
  for (int j = threadIdx.x; j < m.H; j += blockDim.x) s.act[m.D + j] = tanh(s.h[j]);
  if (threadIdx.x == 0) {
    const float tdiff = t0 - tau;
    s.act[m.D + m.H] = (double)tau;
    s.act[m.D + m.H + 1] = (double)tdiff;
    if (m.curt) s.act[m.D + m.H + 2] = (double)(tau + tdiff);
  }
  __syncthreads();
}
__device__ inline void set_last_x(const FArgs& A, const Lds& s, const double* src) {
  for (int d = threadIdx.x; d < A.m.D; d += blockDim.x) {
    const double v = src[d];
    s.lastX[d] = v;
    s.tlx[d] = tanh(v);
  }
  __syncthreads();
}

__global__ void k_f64_fwd(const FArgs A) {
  const FModel& m = A.m;
  const int p = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
  const int B = A.B, D = m.D, H = m.H, DO = m.DO;
  const Lds s = carve(m, false);
  const bool want_path = A.flags & NJODE_C_RETURN_PATH, want_loss = A.flags & NJODE_C_GET_LOSS,
             save = A.flags & NJODE_C_SAVE_BWD;

  const double* x0 = A.start_X + (size_t)p * D;
  for (int d = tid; d < D; d += nth) s.xin[d] = x0[d];
  __syncthreads();
  encode(A, s, s.xin, nullptr, s.h, true);
  set_last_x(A, s, s.xin);
  float tau = 0.0f;
  double loss_acc = 0.0;
  size_t row = 0;

  auto record = [&](bool fresh_y) {
    if (!want_path) return;
    if (fresh_y) readout(A, s, s.h, s.y, true);
    double* ph = A.path_h + (row * B + p) * H;
    double* py = A.path_y + (row * B + p) * DO;
    for (int j = tid; j < H; j += nth) ph[j] = s.h[j];
    for (int j = tid; j < DO; j += nth) py[j] = s.y[j];
  };
  record(true);

  auto step = [&](int k) {
    ode_input(A, s, tau, A.step_t[k]);
    net_fwd(m.ode, A.wt, A.params, s.act, s.tmpH, true);
    const double dt = A.step_dt[k];
    double* hs = save ? A.h_step + ((size_t)k * B + p) * H : nullptr;
    for (int j = tid; j < H; j += nth) {
      const double hv = s.h[j];
      if (save) hs[j] = hv;
      s.h[j] = __dadd_rn(hv, __dmul_rn(dt, s.tmpH[j]));   // h + step * f: a product, then a sum
    }
    __syncthreads();
    ++row;
    record(true);
  };

  auto jump = [&](int i) {
    const int r = A.row_of[(size_t)i * B + p];
    if (r >= 0) {
      const double* X = A.X + (size_t)r * D;
      const double* M = m.masked ? A.M + (size_t)r * D : nullptr;
      if (save) {
        for (int j = tid; j < H; j += nth) A.h_bj[(size_t)r * H + j] = s.h[j];
        for (int d = tid; d < D; d += nth) A.x_prev[(size_t)r * D + d] = s.lastX[d];
        if (tid == 0) A.tau_prev[r] = tau;
      }
      if (want_path) {   // (the row before this one holds the readout of this very state)
        for (int j = tid; j < DO; j += nth) s.ybj[j] = s.y[j];
        __syncthreads();
      } else if (want_loss || m.masked) {
        readout(A, s, s.h, s.ybj, true);
      }
      for (int d = tid; d < D; d += nth)
        s.xin[d] = m.masked ? X[d] * M[d] + (1.0 - M[d]) * s.ybj[d] : X[d];
      __syncthreads();
      encode(A, s, s.xin, M, s.h, true);
      if (want_path || want_loss || m.masked) readout(A, s, s.h, s.y, true);
      if (want_loss && tid == 0) {
        double sa = 0.0, sb = 0.0;
        for (int d = 0; d < D; ++d) {
          const double mk = M ? M[d] : 1.0;
          const double e1 = X[d] - s.y[d];
          const double e2 = s.ybj[d] - (m.loss_easy ? X[d] : s.y[d]);
          sa += mk * (e1 * e1);
          sb += mk * (e2 * e2);
        }
        const double after = sqrt(sa + LOSS_EPS), before = sqrt(sb + LOSS_EPS);
        const double w = A.weight;
        const double sum = m.loss_easy ? w * after + (1.0 - w) * before
                                       : 2.0 * w * after + 2.0 * (1.0 - w) * before;
        loss_acc += sum * sum / (double)A.n_obs_ot[p];
      }
      set_last_x(A, s, m.masked ? s.y : X);
      tau = A.time_f32[i];
    }
    ++row;
    record(false);
  };

  int k = 0;
  const int K = A.K;
  for (int i = 0; i < A.nt; ++i) {
    const int kj = A.k_jump[i];
    for (; k < kj && k < K; ++k) step(k);
    jump(i);
  }
  for (; k < K; ++k) step(k);

  if (A.hT)
    for (int j = tid; j < H; j += nth) A.hT[(size_t)p * H + j] = s.h[j];
  if (want_loss && tid == 0) A.loss_part[p] = loss_acc;
  if (save) {
    for (int d = tid; d < D; d += nth) A.x_end[(size_t)p * D + d] = s.lastX[d];
    if (tid == 0) A.tau_end[p] = tau;
  }
}

__global__ void k_f64_bwd(const FArgs A) {
  const FModel& m = A.m;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int B = A.B, D = m.D, H = m.H, DO = m.DO, K = A.K;
  const Lds s = carve(m, true);
  double* slab = A.slabs + (size_t)blockIdx.x * m.P;
  const bool want_loss = (A.flags & NJODE_C_GET_LOSS) && A.grad_loss;
  const double gl = want_loss ? A.grad_loss[0] : 0.0;

  for (int p = blockIdx.x; p < B; p += A.S) {
    for (int j = tid; j < H; j += nth) s.lam[j] = A.grad_hT ? A.grad_hT[(size_t)p * H + j] : 0.0;
    for (int d = tid; d < D; d += nth) s.lamx[d] = 0.0;
    set_last_x(A, s, A.x_end + (size_t)p * D);
    float tau = A.tau_end[p];

    auto step = [&](int k) {
      const double* hs = A.h_step + ((size_t)k * B + p) * H;
      for (int j = tid; j < H; j += nth) s.h[j] = hs[j];
      __syncthreads();
      ode_input(A, s, tau, A.step_t[k]);
      net_fwd(m.ode, A.wt, A.params, s.act, s.tmpH, false);
      const double dt = A.step_dt[k];
      for (int j = tid; j < H; j += nth) s.dA[j] = dt * s.lam[j];
      __syncthreads();
      const double* din = net_bwd(m.ode, A.params, s.act, s.dA, s.dB, slab);
      for (int j = tid; j < H; j += nth) {
        const double th = s.act[D + j];
        s.lam[j] += din[D + j] * (1.0 - th * th);
      }
      if (m.masked)
        for (int d = tid; d < D; d += nth) {
          const double th = s.tlx[d];
          s.lamx[d] += din[d] * (1.0 - th * th);
        }
      __syncthreads();
    };

    auto jump = [&](int i) {
      const int r = A.row_of[(size_t)i * B + p];
      if (r < 0) return;
      const double* X = A.X + (size_t)r * D;
      const double* M = m.masked ? A.M + (size_t)r * D : nullptr;
      for (int j = tid; j < H; j += nth) s.h[j] = A.h_bj[(size_t)r * H + j];
      __syncthreads();
      // the jump once more: Y_bj, the encoder input, the new state, Y (whose activations stay)
      readout(A, s, s.h, s.ybj, true);
      for (int d = tid; d < D; d += nth)
        s.xin[d] = m.masked ? X[d] * M[d] + (1.0 - M[d]) * s.ybj[d] : X[d];
      __syncthreads();
      encode(A, s, s.xin, M, s.hn, true);
      readout(A, s, s.hn, s.y, true);
      // adjoints of Y and Y_bj: the loss term, and last_X = Y of a masked model
      if (want_loss) {
        if (tid == 0) {   // the two sums of the loss term, once per row
          double sa = 0.0, sb = 0.0;
          for (int d = 0; d < D; ++d) {
            const double mk = M ? M[d] : 1.0;
            const double e1 = X[d] - s.y[d];
            const double e2 = s.ybj[d] - (m.loss_easy ? X[d] : s.y[d]);
            sa += mk * (e1 * e1);
            sb += mk * (e2 * e2);
          }
          s.dB[0] = sqrt(sa + LOSS_EPS);
          s.dB[1] = sqrt(sb + LOSS_EPS);
        }
        __syncthreads();
        // (a path with a row has n_obs_ot >= 1)
        const double c_loss = gl / ((double)A.n_obs_ot[p] * A.lbs);
        const double after = s.dB[0], before = s.dB[1];
        const double w = A.weight;
        const double ca = m.loss_easy ? w : 2.0 * w, cb = m.loss_easy ? 1.0 - w : 2.0 * (1.0 - w);
        for (int j = tid; j < DO; j += nth) {
          const double dsum = c_loss * 2.0 * (ca * after + cb * before);
          const double mk = M ? M[j] : 1.0;
          const double e1 = mk * (X[j] - s.y[j]) / after;
          const double e2 = mk * (s.ybj[j] - (m.loss_easy ? X[j] : s.y[j])) / before;
          s.gY[j] = dsum * (-ca * e1 - (m.loss_easy ? 0.0 : cb * e2)) + (m.masked ? s.lamx[j] : 0.0);
          s.gYbj[j] = dsum * cb * e2;
        }
      } else {
        for (int j = tid; j < DO; j += nth) {
          s.gY[j] = m.masked ? s.lamx[j] : 0.0;
          s.gYbj[j] = 0.0;
        }
      }
      for (int j = tid; j < DO; j += nth) s.dA[j] = s.gY[j];
      __syncthreads();
      // readout at the new state
      const double* din = net_bwd(m.dec, A.params, s.act, s.dA, s.dB, slab);
      for (int i2 = tid; i2 < H; i2 += nth) {
        const double th = s.act[i2];
        s.tmpH[i2] = s.lam[i2] + din[i2] * (1.0 - th * th) + res_bwd(m.dec_case, m.dec_mult, s.gY, H, DO, i2);
      }
      __syncthreads();
      // encoder
      encode(A, s, s.xin, M, nullptr, false);
      for (int j = tid; j < H; j += nth) s.dA[j] = s.tmpH[j];
      __syncthreads();
      din = net_bwd(m.enc, A.params, s.act, s.dA, s.dB, slab);
      if (m.masked) {   // x_in = X M + (1 - M) Y_bj
        for (int d = tid; d < D; d += nth) {
          const double th = s.act[d];
          const double gx = din[d] * (1.0 - th * th) + res_bwd(m.enc_case, m.enc_mult, s.tmpH, D, H, d);
          s.gYbj[d] += (1.0 - M[d]) * gx;
        }
      }
      __syncthreads();
      // readout before the jump
      readout(A, s, s.h, nullptr, false);
      for (int j = tid; j < DO; j += nth) s.dA[j] = s.gYbj[j];
      __syncthreads();
      din = net_bwd(m.dec, A.params, s.act, s.dA, s.dB, slab);
      for (int i2 = tid; i2 < H; i2 += nth) {
        const double th = s.act[i2];
        s.lam[i2] = din[i2] * (1.0 - th * th) + res_bwd(m.dec_case, m.dec_mult, s.gYbj, H, DO, i2);
      }
      for (int d = tid; d < D; d += nth) s.lamx[d] = 0.0;
      __syncthreads();
      set_last_x(A, s, A.x_prev + (size_t)r * D);
      tau = A.tau_prev[r];
    };

    int k = K;
    for (int i = A.nt - 1; i >= 0; --i) {
      int kj = A.k_jump[i];
      if (kj < 0) kj = 0;
      while (k > kj) step(--k);
      jump(i);
    }
    while (k > 0) step(--k);

    // the start state
    const double* x0 = A.start_X + (size_t)p * D;
    for (int d = tid; d < D; d += nth) s.xin[d] = x0[d];
    __syncthreads();
    encode(A, s, s.xin, nullptr, nullptr, false);
    for (int j = tid; j < H; j += nth) s.dA[j] = s.lam[j];
    __syncthreads();
    net_bwd(m.enc, A.params, s.act, s.dA, s.dB, slab);
  }
}

// loss = (sum of the paths' terms, in a fixed tree) / loss_batch_size
__global__ void k_f64_loss(const double* __restrict__ part, int B, double lbs, double* loss) {
  double sum[1];
  tree_sum_256<1>(part, B, 0, sum);
  if (threadIdx.x == 0) loss[0] = sum[0] / lbs;
}

// ---- host ----------------------------------------------------------------------------------------

bool build_net(FNet& N, int n_in, int n_out, const NjodeNet& d, int& p_off, int& maxv) {
  if (d.n_hidden < 0 || d.n_hidden > NJODE_MAX_HIDDEN) return false;
  N.nl = d.n_hidden + 1;
  N.n_in = n_in;
  N.n_out = n_out;
  int a_off = 0;
  for (int l = 0; l < N.nl; ++l) {
    FLayer& L = N.l[l];
    L.n_in = l == 0 ? n_in : d.width[l - 1];
    L.n_out = l == d.n_hidden ? n_out : d.width[l];
    if (L.n_in <= 0 || L.n_out <= 0 || L.n_in > NJODE_GEN_MAX_WIDTH + 64 || L.n_out > NJODE_GEN_MAX_WIDTH)
      return false;
    L.act = l < d.n_hidden ? d.act[l] : -1;
    if (l < d.n_hidden && L.act != NJODE_ACT_TANH && L.act != NJODE_ACT_RELU) return false;
    L.w_off = p_off;
    L.b_off = p_off + L.n_in * L.n_out;
    p_off = L.b_off + L.n_out;
    L.a_off = a_off;
    a_off += L.n_in;
    if (L.n_in > maxv) maxv = L.n_in;
    if (L.n_out > maxv) maxv = L.n_out;
  }
  N.act_total = a_off;
  return true;
}

void set_row_lanes(FNet& N, int nth) {
  for (int l = 0; l < N.nl; ++l) {
    int lg = 0;
    while ((1 << lg) < N.l[l].n_in && (1 << lg) < nth) ++lg;
    N.l[l].cw_log2 = lg;
  }
}

bool build_model(const NjodeDims* d, FModel& m, const char** why) {
  memset(&m, 0, sizeof(m));
  if (!d) { *why = "null dims"; return false; }
  if (d->flags & NJODE_F_USE_RNN) {
    *why = "use_rnn: the GRU jump has no float64 kernels";
    return false;
  }
  const int D = d->input_size, H = d->hidden_size, DO = d->output_size;
  if (D <= 0 || H <= 0 || DO <= 0 || D > 512 || H > 1024 || DO > 512) {
    *why = "sizes out of range (input_size, output_size <= 512, hidden_size <= 1024)";
    return false;
  }
  m.D = D; m.H = H; m.DO = DO;
  m.masked = (d->flags & NJODE_F_MASKED) ? 1 : 0;
  m.curt = (d->flags & NJODE_F_INPUT_CURRENT_T) ? 1 : 0;
  m.loss_easy = (d->flags & NJODE_F_LOSS_EASY) ? 1 : 0;
  if (m.masked && D != DO) {
    *why = "masked mode feeds the readout back as the input: input_size must equal output_size";
    return false;
  }
  m.IN0 = D + H + (m.curt ? 3 : 2);
  m.enc_case = m.dec_case = 0;
  m.enc_mult = m.dec_mult = 1;
  if (d->flags & NJODE_F_RESIDUAL) {   // FFNN residual rules (models.py:240-259)
    if (D <= H) { if (H % D) { *why = "residual: output_size needs to be multiple of input_size"; return false; } m.enc_case = 1; m.enc_mult = H / D; }
    else { if (D % H) { *why = "residual: input_size needs to be multiple of output_size"; return false; } m.enc_case = 2; m.enc_mult = D / H; }
    if (H <= DO) { if (DO % H) { *why = "residual: output_size needs to be multiple of input_size"; return false; } m.dec_case = 1; m.dec_mult = DO / H; }
    else { if (H % DO) { *why = "residual: input_size needs to be multiple of output_size"; return false; } m.dec_case = 2; m.dec_mult = H / DO; }
  }
  NjodeNet nets[3];
  if (d->per_net) {
    for (int i = 0; i < 3; ++i) nets[i] = d->nets[i];
  } else {
    if (d->n_hidden < 0 || d->n_hidden > NJODE_MAX_HIDDEN) { *why = "n_hidden out of range"; return false; }
    for (int i = 0; i < 3; ++i) {
      nets[i].n_hidden = d->n_hidden;
      for (int l = 0; l < NJODE_MAX_HIDDEN; ++l) { nets[i].width[l] = d->width; nets[i].act[l] = d->act; }
    }
  }
  int p_off = 0, maxv = 1;
  if (!build_net(m.ode, m.IN0, H, nets[0], p_off, maxv) ||
      !build_net(m.enc, m.masked ? 2 * D : D, H, nets[1], p_off, maxv) ||
      !build_net(m.dec, H, DO, nets[2], p_off, maxv)) {
    *why = "network description out of range (<= 8 hidden layers, widths <= 1024, layer inputs <= 1088, tanh / relu)";
    return false;
  }
  m.P = p_off;
  m.maxv = maxv;
  m.act_max = m.ode.act_total;
  if (m.enc.act_total > m.act_max) m.act_max = m.enc.act_total;
  if (m.dec.act_total > m.act_max) m.act_max = m.dec.act_total;
  // threads of a workgroup: one per unit of the widest layer, a POWER OF TWO in 64 .. 256 -- the
  // slab update deals 2^cw_log2 <= nth lanes to a weight row and nth >> cw_log2 >= 1 rows to a pass,
  // which covers every element once only when the lane count divides the workgroup
  m.nth = maxv <= 64 ? 64 : (maxv <= 128 ? 128 : 256);
  set_row_lanes(m.ode, m.nth);
  set_row_lanes(m.enc, m.nth);
  set_row_lanes(m.dec, m.nth);
  if (lds_doubles(m, true) * 8 > LDS_LIMIT) {
    *why = "the per-path vectors and layer inputs of the adjoint sweep exceed the 160 KB LDS of a workgroup";
    return false;
  }
  return true;
}

// the envelope: what the shape-generic fp32 family takes, minus use_rnn
bool supported(const NjodeDims* dims, FModel& m) {
  const char* why = "";
  if (!build_model(dims, m, &why)) {
    fail(NJODE_E_UNSUPPORTED, "float64 route: %s", why);
    return false;
  }
  return gen::gen_supported(dims);   // (leaves its own reason)
}

// every layer's matrix: the forward reads them transposed (bias slots are not used)
MatTable weight_matrices(const FModel& m) {
  MatTable t = {};
  for (const FNet* N : {&m.ode, &m.enc, &m.dec})
    for (int l = 0; l < N->nl; ++l) t.add(N->l[l].w_off, N->l[l].n_out, N->l[l].n_in);
  return t;
}

struct Layout : Arena {
  size_t step_dt, step_t, k_jump, time_f32, time_ptr, wt, row_of, loss_part;
  size_t h_step, h_bj, x_prev, tau_prev, x_end, tau_end, slabs;
  int S;
};

Layout make_layout(const FModel& m, int B, int n_obs, int nt, int K, int flags) {
  Layout L;
  const size_t b = B, no = at_least_1(n_obs), k = at_least_1(K), t = at_least_1(nt);
  L.step_dt = L.take(k * 8);
  L.step_t = L.take(k * 4);
  L.k_jump = L.take(t * 4);
  L.time_f32 = L.take(t * 4);
  L.time_ptr = L.take((t + 1) * 4);
  L.wt = L.take((size_t)m.P * 8);
  L.row_of = L.take(t * b * 4);
  L.loss_part = L.take(b * 8);
  L.S = slab_count((size_t)m.P * 8, SLAB_BUDGET, MAX_SLABS, B);
  if (flags & NJODE_C_SAVE_BWD) {
    L.h_step = L.take(k * b * m.H * 8);
    L.h_bj = L.take(no * m.H * 8);
    L.x_prev = L.take(no * m.D * 8);
    L.tau_prev = L.take(no * 4);
    L.x_end = L.take(b * m.D * 8);
    L.tau_end = L.take(b * 4);
    L.slabs = L.take((size_t)L.S * m.P * 8);
  }
  return L;
}

constexpr int KNOWN_FLAGS = NJODE_C_GET_LOSS | NJODE_C_RETURN_PATH | NJODE_C_SAVE_BWD;
constexpr const char* BAD_FLAG = "call flag the float64 route does not take";

// every refusal a call makes before it launches anything (array contents: the host schedule only)
int check_call(const FModel& m, const NjodeBatch64* b, const NjodeSchedule64* s, int flags, const double* params,
               const void* ws, bool forward) {
  if (int rc = check_sizes_and_params(b, s, flags, KNOWN_FLAGS, BAD_FLAG, params)) return rc;
  const int n_obs = b->n_obs, nt = s->n_times;
  if (!b->start_X || (n_obs > 0 && (!b->X || !b->obs_idx))) return fail(NJODE_E_BADARG, "null batch array");
  if (m.masked && n_obs > 0 && !b->M) return fail(NJODE_E_BADARG, "masked model needs M");
  if (flags & NJODE_C_GET_LOSS) {
    if (!b->n_obs_ot) return fail(NJODE_E_BADARG, "get_loss needs n_obs_ot");
    if (m.D != m.DO) return fail(NJODE_E_BADARG, "get_loss needs input_size == output_size");
    if (!(b->loss_batch_size > 0.0)) return fail(NJODE_E_BADARG, "loss_batch_size must be positive");
  }
  if (n_obs > 0 && nt == 0) return fail(NJODE_E_BADARG, "observation rows without observation times");
  if (int rc = check_workspace_ptr(ws)) return rc;
  return forward ? check_schedule_walk(s, n_obs) : NJODE_OK;
}

void fill_args(FArgs& A, const FModel& m, const Layout& L, char* ws, const NjodeBatch64* b,
               const NjodeSchedule64* s, int flags, double weight, const double* params) {
  memset(&A, 0, sizeof(A));
  A.m = m;
  A.B = b->batch_size; A.n_obs = b->n_obs; A.nt = s->n_times; A.K = s->n_steps;
  A.flags = flags; A.S = L.S;
  A.weight = weight; A.lbs = b->loss_batch_size;
  A.params = params;
  A.wt = (const double*)(ws + L.wt);
  A.start_X = b->start_X; A.X = b->X; A.M = b->M;
  A.obs_idx = b->obs_idx; A.n_obs_ot = b->n_obs_ot;
  A.step_dt = (const double*)(ws + L.step_dt);
  A.step_t = (const float*)(ws + L.step_t);
  A.k_jump = (const int*)(ws + L.k_jump);
  A.time_f32 = (const float*)(ws + L.time_f32);
  A.time_ptr = (const int*)(ws + L.time_ptr);
  A.row_of = (int*)(ws + L.row_of);
  A.loss_part = (double*)(ws + L.loss_part);
  if (flags & NJODE_C_SAVE_BWD) {
    A.h_step = (double*)(ws + L.h_step);
    A.h_bj = (double*)(ws + L.h_bj);
    A.x_prev = (double*)(ws + L.x_prev);
    A.tau_prev = (float*)(ws + L.tau_prev);
    A.x_end = (double*)(ws + L.x_end);
    A.tau_end = (float*)(ws + L.tau_end);
    A.slabs = (double*)(ws + L.slabs);
  }
}

}  // namespace

extern "C" int njode_f64_supported(const NjodeDims* dims) {
  FModel m;
  return supported(dims, m) ? 1 : 0;
}

extern "C" int njode_f64_workspace_bytes(const NjodeDims* dims, int32_t B, int32_t n_obs, int32_t nt,
                                         int32_t K, int32_t call_flags, size_t* out) {
  FModel m;
  if (!supported(dims, m)) return NJODE_E_UNSUPPORTED;
  if (!out || B <= 0 || n_obs < 0 || nt < 0 || K < 0) return fail(NJODE_E_BADARG, "bad size");
  if (call_flags & ~KNOWN_FLAGS) return fail(NJODE_E_BADARG, "%s", BAD_FLAG);
  *out = make_layout(m, B, n_obs, nt, K, call_flags).total;
  return NJODE_OK;
}

extern "C" int njode_forward_f64(const NjodeDims* dims, const double* params, const NjodeBatch64* b,
                                 const NjodeSchedule64* s, int32_t flags, double weight, double* hT,
                                 double* loss, double* path_h, double* path_y, void* workspace,
                                 size_t ws_bytes, njodeStream_t st) {
  FModel m;
  if (!supported(dims, m)) return NJODE_E_UNSUPPORTED;
  int rc = check_call(m, b, s, flags, params, workspace, true);
  if (rc) return rc;
  if ((flags & NJODE_C_GET_LOSS) && !loss) return fail(NJODE_E_BADARG, "null output");
  if ((flags & NJODE_C_RETURN_PATH) && (!path_h || !path_y)) return fail(NJODE_E_BADARG, "null output");
  const int B = b->batch_size, n_obs = b->n_obs, nt = s->n_times, K = s->n_steps;
  const Layout L = make_layout(m, B, n_obs, nt, K, flags);
  if ((rc = check_workspace_size(ws_bytes, L.total))) return rc;
  char* ws = (char*)workspace;
  const int lds = lds_doubles(m, false) * 8;
  if ((rc = set_lds((const void*)k_f64_fwd, lds))) return rc;

  if (K > 0) {
    HIP_TRY(hipMemcpyAsync(ws + L.step_dt, s->step_dt, (size_t)K * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ws + L.step_t, s->step_t, (size_t)K * 4, hipMemcpyHostToDevice, st));
  }
  if (nt > 0) {
    HIP_TRY(hipMemcpyAsync(ws + L.k_jump, s->k_jump, (size_t)nt * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ws + L.time_f32, s->time_f32, (size_t)nt * 4, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemcpyAsync(ws + L.time_ptr, s->time_ptr, ((size_t)nt + 1) * 4, hipMemcpyHostToDevice, st));

  FArgs A;
  fill_args(A, m, L, ws, b, s, flags, weight, params);
  A.hT = hT;
  A.path_h = path_h;
  A.path_y = path_y;
  transpose_weights(weight_matrices(m), m.P, params, (double*)(ws + L.wt), "k_f64_transpose", st);
  build_row_table(A.row_of, b->obs_idx, A.time_ptr, n_obs, nt, B, "k_f64_rows", st);
  {
    ProfScope ps("k_f64_fwd", st);
    k_f64_fwd<<<B, m.nth, lds, st>>>(A);
  }
  if (flags & NJODE_C_GET_LOSS) {
    ProfScope ps("k_f64_loss", st);
    k_f64_loss<<<1, 256, 0, st>>>(A.loss_part, B, A.lbs, loss);
  }
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}

extern "C" int njode_backward_f64(const NjodeDims* dims, const double* params, const NjodeBatch64* b,
                                  const NjodeSchedule64* s, int32_t flags, double weight,
                                  const double* grad_loss, const double* grad_hT, double* grad_params,
                                  void* workspace, size_t ws_bytes, njodeStream_t st) {
  FModel m;
  if (!supported(dims, m)) return NJODE_E_UNSUPPORTED;
  int rc = check_call(m, b, s, flags, params, workspace, false);
  if (rc) return rc;
  if (!(flags & NJODE_C_SAVE_BWD)) return fail(NJODE_E_BADARG, "the backward needs the forward's NJODE_C_SAVE_BWD");
  if (flags & NJODE_C_RETURN_PATH) return fail(NJODE_E_BADARG, "a RETURN_PATH call has no backward");
  if (!grad_params) return fail(NJODE_E_BADARG, "null grad_params");
  if ((flags & NJODE_C_GET_LOSS) && !grad_loss) return fail(NJODE_E_BADARG, "null grad_loss");
  const int B = b->batch_size, n_obs = b->n_obs, nt = s->n_times, K = s->n_steps;
  const Layout L = make_layout(m, B, n_obs, nt, K, flags);
  if ((rc = check_workspace_size(ws_bytes, L.total))) return rc;
  char* ws = (char*)workspace;
  const int lds = lds_doubles(m, true) * 8;
  if ((rc = set_lds((const void*)k_f64_bwd, lds))) return rc;
  FArgs A;
  fill_args(A, m, L, ws, b, s, flags, weight, params);
  A.grad_loss = (flags & NJODE_C_GET_LOSS) ? grad_loss : nullptr;
  A.grad_hT = grad_hT;
  HIP_TRY(hipMemsetAsync(A.slabs, 0, (size_t)L.S * m.P * 8, st));
  {
    ProfScope ps("k_f64_bwd", st);
    k_f64_bwd<<<L.S, m.nth, lds, st>>>(A);
  }
  reduce_slabs(A.slabs, L.S, m.P, grad_params, "k_f64_reduce", st);
  HIP_TRY(hipGetLastError());
  return NJODE_OK;
}
