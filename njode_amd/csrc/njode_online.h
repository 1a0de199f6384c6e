// njode_online.h -- online filtering: a series' state (h, last_X, tau, now) stays in HBM between
// calls; a call walks the listed series to their targets, ONE WAVE PER SERIES, a lane is a unit of the
// layer being evaluated (the plan of njode_chain.h: the ODE network's rows in registers, the encoder's
// and the readout's in the block's LDS tables, c1 = b1 + W1x tanh(last_X) + w_tau tau once per segment).
//
// What is new is the clock.  Every series walks its own: the reference's float64 loop
// (models.py:430-439; schedule._walk_clock operation for operation)
//     guard = t - 1e-10 delta_t;  while now < guard: step = now < t - delta_t ? delta_t : t - now
// with fp32(step) and fp32(now before the step) consumed by the Euler step.  Every operation of it is
// ONE float64 instruction on values the host cannot contract (1e-10 delta_t arrives multiplied), and
// the values are the same in all lanes, so the loop condition is a scalar one.  The loop is COUNTED:
// at most max_steps steps in front of one target, whatever the inputs hold; a series the bound stops
// keeps the state it reached (no jump, no readout) and reports status 1.
//
// One body, five modes (OnlineMode): advance (1 target, no jump, state written), observe (1 target,
// jump, readouts before and after it, state written), predict (Q targets, a readout at each, on a
// register copy of the state: nothing written back), reset (h = encoder(start_X, mask 0)), run (the
// row's range of events ev_ptr[row] .. ev_ptr[row + 1] - 1 in order, each an observe (kind 1) or an
// advance with a readout (kind 0), around the state in registers: the ODE rows are loaded and the
// tables filled once, the state is written once, at the end or where the bound stopped the series).
// A run leaves the bits of the single calls: between two calls h, last_X and tau pass through fp32
// memory unchanged and th, c1 are functions of them, so after a jump the run takes th = tanh_f(h_new)
// and c1 = segment_c1(tanh_f(last_X_new), tau_new) from the same functions.
//
// Residual cases: every one of FFNN (models.py:240-259), not only the identity ChainOk admits --
// case 1 with out = m in: y[o] += x[o % in], case 2 with in = m out: y[o] += mean_c x[c out + o]; the
// input vector goes through a 64-float scratch row of the wave's own.
#pragma once
#include "njode_chain.h"
#include "njode_online_args.h"

namespace njode {

template <class C, bool TWO = (C::NH == 2)> struct OnlineOk { static constexpr bool value = false; };
template <class C> struct OnlineOk<C, true> {
  static constexpr bool value = !C::RNN && C::W <= 64 && C::H <= 64 && C::D <= 64 && C::DO <= 64 &&
                                (!C::MASKED || C::D == C::DO);
};

// the identity path's addend for the own unit u (< NOUT; the caller masks the others): `own` is the
// input vector's own unit, zero for units >= NIN
template <int CASE, int NIN, int NOUT> NJ_DEV float online_residual(float own, int u, lfp scr) {
  if constexpr (CASE == 0) {
    return 0.0f;
  } else if constexpr (NIN == NOUT) {
    return own;
  } else {
    static_assert(NIN <= 64 && NOUT <= 64, "one scratch row");
    wave_lds_sync();   // (the row's previous readers are done)
    scr[u] = own;      // (u < 64: every lane owns one float of the row)
    wave_lds_sync();
    if constexpr (CASE == 1) {
      return scr[u % NIN];
    } else {
      constexpr int mult = NIN / NOUT;
      const int j = u < NOUT ? u : 0;
      float s = 0.0f;
#pragma unroll
      for (int c = 0; c < mult; ++c) s += scr[c * NOUT + j];
      return s * (1.0f / mult);
    }
  }
}

// ---- dot products with FOUR accumulators: every block of four quads (16 units) sums into one of its
// own, (a0 + a2) + (a1 + a3) at the end.  dpp_dot / chain_dot_lds alternate two; a masked series
// feeds its own predictions back at every jump, which amplifies the rounding of each sum, and with
// chains of at most 16 terms the 41-wide residual shape stays within the fp32 reference's own
// distance from float64.  Same fma count, two more additions.
template <int K, int B> NJ_DEV void online_dot_blocks(float (&acc)[4], const float (&R)[4], const float (&w)[K]) {
  constexpr int Q = 4 * B, FULL = K / 4 - Q;   // full quads left
  if constexpr (FULL >= 4) {
    dpp_block<Q, 4>(acc[B], R, w + 4 * Q);
    if constexpr (B < 3) online_dot_blocks<K, B + 1>(acc, R, w);
  } else {
    if constexpr (FULL >= 1) dpp_block<Q, FULL>(acc[B], R, w + 4 * Q);
    if constexpr (K % 4 != 0) dpp_tail<K / 4, K % 4>(acc[B], R, w + 4 * (K / 4));
  }
}
template <int K> NJ_DEV float online_dot(float init, const float (&R)[4], const float (&w)[K]) {
  static_assert(K >= 1 && K <= 64, "one unit per lane");
  float acc[4] = {init, 0.0f, 0.0f, 0.0f};
  online_dot_blocks<K, 0>(acc, R, w);
  return (acc[0] + acc[2]) + (acc[1] + acc[3]);
}
// ... with the lane's row in an LDS table of chain_fill (padding entries zero: every quad is full)
template <int NQ, int B> NJ_DEV void online_lds_blocks(float (&acc)[4], lfp tab_lane, const float (&R)[4]) {
  constexpr int Q = 4 * B, N = NQ - Q >= 4 ? 4 : NQ - Q;
  float w[16];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f4 v = *(lf4p)(tab_lane + (Q + (j < N ? j : 0)) * 256);
    w[4 * j] = v.x;
    w[4 * j + 1] = v.y;
    w[4 * j + 2] = v.z;
    w[4 * j + 3] = v.w;
  }
  dpp_block<Q, N>(acc[B], R, w);
  if constexpr (Q + 4 < NQ) online_lds_blocks<NQ, B + 1>(acc, tab_lane, R);
}
template <int NK> NJ_DEV float online_dot_lds(lfp tab_lane, const float (&R)[4], float init) {
  constexpr int NQ = chain_q(NK);
  static_assert(NQ >= 1 && NQ <= 16, "one input vector is at most 64 units");
  float acc[4] = {init, 0.0f, 0.0f, 0.0f};
  online_lds_blocks<NQ, 0>(acc, tab_lane, R);
  return (acc[0] + acc[2]) + (acc[1] + acc[3]);
}

// a value every lane holds alike, as a scalar condition
NJ_DEV bool online_uniform(bool v) { return __builtin_amdgcn_readfirstlane(v ? 1 : 0) != 0; }
// ... and a float64 every lane holds alike, as a scalar (the bits are untouched)
NJ_DEV double online_uniform_f64(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <class C, int MODE>
__global__ void __launch_bounds__(64 * ONLINE_WAVES) k_online(OnlineArgs a) {
  using NO = typename C::Ode;
  using NE = typename C::Enc;
  using ND = typename C::Dec;
  using L = ChainLds<C>;
  constexpr int D = C::D, H = C::H, DO = C::DO, W = C::W, EIN = C::ENC_IN, OIN = C::ODE_IN;
  constexpr bool RUN = MODE == ONLINE_RUN;
  constexpr bool JUMP = MODE == ONLINE_OBSERVE || RUN, RESET = MODE == ONLINE_RESET;
  constexpr bool NEED_ENC = JUMP || RESET, NEED_DEC = JUMP || MODE == ONLINE_PREDICT;
  __shared__ __attribute__((aligned(16))) float lds_raw[L::FWD_FLOATS];
  __shared__ float scr_raw[64 * ONLINE_WAVES];
  lfp T = (lfp)lds_raw;
  const int lane = threadIdx.x & 63, u = dpp_unit(lane);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  lfp scr = (lfp)scr_raw + wv * 64;
  const float* Po = a.P + C::OFF_ODE;
  const float* Pe = a.P + C::OFF_ENC;
  const float* Pd = a.P + C::OFF_DEC;
  {   // the tables the mode reads; every wave of the block fills, the first a.spb go on
    const int tid = threadIdx.x, nt = blockDim.x;
    if constexpr (NEED_ENC) {
      chain_fill<D>(T + L::FE1, Pe + NE::woff(0), W, EIN, 1, tid, nt);
      if constexpr (C::MASKED) chain_fill<D>(T + L::FE1M, Pe + NE::woff(0) + D, W, EIN, 1, tid, nt);
      chain_fill<W>(T + L::FE2, Pe + NE::woff(1), W, W, 1, tid, nt);
      chain_fill<W>(T + L::FE3, Pe + NE::woff(2), H, W, 1, tid, nt);
    }
    if constexpr (NEED_DEC) {
      chain_fill<H>(T + L::FD1, Pd + ND::woff(0), W, H, 1, tid, nt);
      chain_fill<W>(T + L::FD2, Pd + ND::woff(1), W, W, 1, tid, nt);
      chain_fill<W>(T + L::FD3, Pd + ND::woff(2), DO, W, 1, tid, nt);
    }
    if constexpr (!RESET) chain_fill<D>(T + L::FX1, Po + NO::woff(0), W, OIN, 1, tid, nt);   // (x columns: 0 .. D-1)
  }
  __syncthreads();
  if (wv >= a.spb) return;
  const int row = blockIdx.x * a.spb + wv;   // (wave-uniform)
  if (row >= a.n) return;
  const int sid = __builtin_amdgcn_readfirstlane(a.ids ? a.ids[row] : row);
  if (sid < 0 || sid >= a.n_series) {   // (nothing of the state is touched through such an id)
    if (!RESET && lane == 0) a.status[row] = 2;
    if (RUN && lane == 0) a.n_done[row] = 0;
    return;
  }
  [[maybe_unused]] int ev0 = 0, ev1 = 0;   // run: the row's events (wave-uniform); a range outside the call reads none
  if constexpr (RUN) {
    ev0 = __builtin_amdgcn_readfirstlane(a.ev_ptr[row]);
    ev1 = __builtin_amdgcn_readfirstlane(a.ev_ptr[row + 1]);
    if (ev0 < 0 || ev1 < ev0 || ev1 > a.n_events) {
      if (lane == 0) {
        a.status[row] = 3;
        a.n_done[row] = 0;
      }
      return;
    }
  }

  lfp tE1 = T + L::FE1 + lane * 4, tE1M = T + L::FE1M + lane * 4, tE2 = T + L::FE2 + lane * 4,
      tE3 = T + L::FE3 + lane * 4, tD1 = T + L::FD1 + lane * 4, tD2 = T + L::FD2 + lane * 4,
      tD3 = T + L::FD3 + lane * 4, tX1 = T + L::FX1 + lane * 4;
  const bool uW = u < W, uH = u < H, uD = u < D, uO = u < DO;
  const int jW = uW ? u : 0, jH = uH ? u : 0, jD = uD ? u : 0, jO = uO ? u : 0;
  const float eb1 = uW ? Pe[NE::boff(0) + jW] : 0.0f, eb2 = uW ? Pe[NE::boff(1) + jW] : 0.0f,
              eb3 = uH ? Pe[NE::boff(2) + jH] : 0.0f;
  const float db1 = uW ? Pd[ND::boff(0) + jW] : 0.0f, db2 = uW ? Pd[ND::boff(1) + jW] : 0.0f,
              db3 = uO ? Pd[ND::boff(2) + jO] : 0.0f;

  // layers 2 and 3 of a network whose rows come from the LDS tables (a1o: the first hidden
  // activation of the own unit)
  auto net_tail = [&](lfp t2, lfp t3, float a1o, float bb2, float bb3) {
    float R[4];
    dpp_replicate(a1o, R);
    const float a2o = chain_hidden<C::ACT, false>(online_dot_lds<W>(t2, R, bb2), 0, 1.0f);
    dpp_replicate(a2o, R);
    return online_dot_lds<W>(t3, R, bb3);
  };
  // readout of the state hq (own unit; thq its tanh)
  auto readout = [&](float hq, float thq) {
    float R[4];
    dpp_replicate(thq, R);
    const float a1o = chain_hidden<C::ACT, false>(online_dot_lds<H>(tD1, R, db1), 0, 1.0f);
    float y = net_tail(tD2, tD3, a1o, db2, db3);
    y += online_residual<C::DEC_CASE, H, DO>(hq, u, scr);
    return uO ? y : 0.0f;
  };
  // encoder of [tanh(xin), mask] (own units txin, m)
  auto encode = [&](float xin, float txin, float m) {
    float R[4];
    dpp_replicate(txin, R);
    float z = online_dot_lds<D>(tE1, R, eb1);
    if constexpr (C::MASKED) {
      dpp_replicate(m, R);
      z = online_dot_lds<D>(tE1M, R, z);
    }
    const float a1o = chain_hidden<C::ACT, false>(z, 0, 1.0f);
    float hq = net_tail(tE2, tE3, a1o, eb2, eb3);
    hq += online_residual<C::ENC_CASE, D, H>(xin, u, scr);
    return uH ? hq : 0.0f;
  };

  float* const st_h = a.h + (size_t)sid * H + jH;
  float* const st_x = a.last_X + (size_t)sid * D + jD;
  if constexpr (RESET) {
    // h = encoder_map(start_X), mask = 0 (models.py:404-413); last_X = start_X, tau = 0, now = 0
    const float xs = uD ? a.X[(size_t)row * D + jD] : 0.0f;
    const float h0 = encode(xs, uD ? tanh_f(xs) : 0.0f, 0.0f);
    if (uH) *st_h = h0;
    if (uD) *st_x = xs;
    if (lane == 0) {
      a.tau[sid] = 0.0f;
      a.now[sid] = 0.0;
    }
    return;
  } else {
    // the ODE network's rows in registers: state columns of W1, tau / tdiff (/ t) columns, W2, W3
    float w1h[H], w2[W], w3[W];
    chain_load_row<H>(w1h, Po + NO::woff(0) + (size_t)jW * OIN + D, uW, 1);
    chain_load_row<W>(w2, Po + NO::woff(1) + (size_t)jW * W, uW, 1);
    chain_load_row<W>(w3, Po + NO::woff(2) + (size_t)jH * W, uH, 1);
    const float w1tau = uW ? Po[NO::woff(0) + (size_t)jW * OIN + D + H] : 0.0f;
    const float w1td = uW ? Po[NO::woff(0) + (size_t)jW * OIN + D + H + 1] : 0.0f;
    const float w1ct = (C::CURT && uW) ? Po[NO::woff(0) + (size_t)jW * OIN + D + H + 2] : 0.0f;
    const float ob1 = uW ? Po[NO::boff(0) + jW] : 0.0f, ob2 = uW ? Po[NO::boff(1) + jW] : 0.0f,
                ob3 = uH ? Po[NO::boff(2) + jH] : 0.0f;
    // the segment's constant part of the ODE network's first layer: b1 + W1x tanh(x) + w_tau tau
    auto segment_c1 = [&](float txq, float tauq) {
      float R[4];
      dpp_replicate(txq, R);
      return fmaf(w1tau, tauq, online_dot_lds<D>(tX1, R, ob1));
    };

    float h = uH ? *st_h : 0.0f, th = uH ? tanh_f(h) : 0.0f;
    const float xl = uD ? *st_x : 0.0f;
    float tau = a.tau[sid];
    double now = a.now[sid];
    float c1 = segment_c1(uD ? tanh_f(xl) : 0.0f, tau);

    // Euler step (models.py:369-377, 430-445) of length dt from the clock value t
    auto euler_step = [&](float dt, float t) {
      float R[4];
      float z = fmaf(w1td, t - tau, c1);
      if constexpr (C::CURT) z = fmaf(w1ct, tau + (t - tau), z);
      dpp_replicate(th, R);
      z = online_dot<H>(z, R, w1h);
      const float a1l = chain_hidden<C::ACT, false>(z, 0, 1.0f);
      dpp_replicate(a1l, R);
      z = online_dot<W>(ob2, R, w2);
      const float a2l = chain_hidden<C::ACT, false>(z, 0, 1.0f);
      dpp_replicate(a2l, R);
      const float f = online_dot<W>(ob3, R, w3);
      h = uH ? fmaf(dt, f, h) : 0.0f;
      th = uH ? tanh_f(h) : 0.0f;
    };
    // the clock up to `target`; false: the bound stopped it short
    const double delta_t = a.delta_t, eps_dt = a.eps_dt;
    const int max_steps = a.max_steps;
    auto walk = [&](double target) {
      const double guard = target - eps_dt, last_full = target - delta_t;
      for (int s = 0; s < max_steps; ++s) {
        if (!online_uniform(now < guard)) return true;
        const double step = now < last_full ? delta_t : target - now;
        euler_step((float)step, (float)now);
        now = now + step;
      }
      return !online_uniform(now < guard);
    };
    const float qnan = __uint_as_float(0x7fc00000u);

    if constexpr (MODE == ONLINE_PREDICT) {
      // a register copy of the state walks through the queries; nothing is written back
      float* yp = a.Y + (size_t)row * a.Q * DO + jO;
      bool ok = true;
      for (int q = 0; q < a.Q; ++q) {
        if (ok) ok = walk(a.t[(size_t)row * a.Q + q]);
        const float y = ok ? readout(h, th) : qnan;   // (ok is wave-uniform)
        if (uO) yp[(size_t)q * DO] = y;
      }
      if (lane == 0) a.status[row] = ok ? 0 : 1;
    } else {
      // the jump (models.py:457-489) with row `r` of X / M; the new last_X of the own unit
      [[maybe_unused]] auto jump = [&](float ybj, size_t r, float& yn) {
        const float x = uD ? a.X[r * D + jD] : 0.0f;
        const float m = (C::MASKED && uD) ? a.M[r * D + jD] : 0.0f;
        const float xin = C::MASKED ? x * m + (1.0f - m) * ybj : x;
        const float hn = encode(xin, uD ? tanh_f(xin) : 0.0f, m);
        const float thn = uH ? tanh_f(hn) : 0.0f;
        yn = readout(hn, thn);
        h = hn;
        th = thn;
        return C::MASKED ? yn : x;
      };
      if constexpr (RUN) {
        // the row's events in order around the register state; e, the kinds and the targets are scalars
        bool ok = true, jumped = false;
        float xnew = xl;
        int e = ev0;
        for (; e < ev1; ++e) {
          const double target = online_uniform_f64(a.t[e]);
          const int kd = a.kind ? __builtin_amdgcn_readfirstlane(a.kind[e]) : 1;
          ok = walk(target);
          if (!ok) break;
          const float ybj = readout(h, th);
          float yn = ybj;   // (an empty slice: the readout of the state it arrives at, twice)
          if (kd != 0) {
            xnew = jump(ybj, (size_t)e, yn);
            tau = (float)target;
            c1 = segment_c1(uD ? tanh_f(xnew) : 0.0f, tau);
            jumped = true;
          }
          if (uO && a.Y_before) a.Y_before[(size_t)e * DO + jO] = ybj;
          if (uO && a.Y) a.Y[(size_t)e * DO + jO] = yn;
        }
        const int done = e - ev0;
        for (; e < ev1; ++e) {   // the event the bound stopped the series at, and those behind it
          if (uO && a.Y_before) a.Y_before[(size_t)e * DO + jO] = qnan;
          if (uO && a.Y) a.Y[(size_t)e * DO + jO] = qnan;
        }
        if (uH) *st_h = h;
        if (jumped && uD) *st_x = xnew;
        if (lane == 0) {
          if (jumped) a.tau[sid] = tau;
          a.now[sid] = now;
          a.status[row] = ok ? 0 : 1;
          a.n_done[row] = done;
        }
      } else {
        const double target = a.t[row];
        const bool ok = walk(target);
        if constexpr (JUMP) {
          float* const yb_p = a.Y_before ? a.Y_before + (size_t)row * DO + jO : nullptr;
          float* const y_p = a.Y ? a.Y + (size_t)row * DO + jO : nullptr;
          if (ok) {
            const float ybj = readout(h, th);
            float yn;
            const float xnew = jump(ybj, (size_t)row, yn);
            if (uO && yb_p) *yb_p = ybj;
            if (uO && y_p) *y_p = yn;
            if (uD) *st_x = xnew;
            if (lane == 0) a.tau[sid] = (float)target;
          } else {
            if (uO && yb_p) *yb_p = qnan;
            if (uO && y_p) *y_p = qnan;
          }
        }
        if (uH) *st_h = h;
        if (lane == 0) {
          a.now[sid] = now;
          a.status[row] = ok ? 0 : 1;
        }
      }
    }
  }
}

}  // namespace njode
