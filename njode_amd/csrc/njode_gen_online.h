// njode_gen_online.h -- online filtering on the shape-generic matrix-core family (njode_gen.h): the
// resident state (h, last_X, tau, now) of include/njode_online.h for every model build_model
// (njode_gen.hip) accepts -- any widths and depths, per-network descriptions, nn_desc = None, the GRU
// jump -- where the one-wave-per-series kernels of njode_online.h stop at two hidden layers of 64.
//
// Execution model: k_gen_fwd's.  One workgroup of m.nw waves owns a TILE of PT <= 16 listed series, a
// chain (column of the MFMA B operand) each; chains >= nv and rows with an id outside the state idle
// on zeros and write nothing.  Every network evaluation is net_forward on the tile with the fragment
// tables of k_gen_pack, every vector operation the one k_gen_fwd applies, in its order: columns of a
// matrix product are independent, so a series gets the bits the batch kernel gives the batch of that
// series alone, whatever its neighbours in the tile do and whichever column it sits in.
//
// What is new is the clock: one per CHAIN (njode_online.h has one per wave).  Lane c < 16 of the
// workgroup walks chain c's float64 clock, the host loop of schedule._walk_clock one instruction per
// operation (1e-10 delta_t arrives multiplied: no product to contract),
//     guard = t - eps_dt;  while now < guard: step = now < t - delta_t ? delta_t : t - now;  now += step
// and leaves fp32(step), fp32(now before it) and an `active` flag in LDS.  The step loop is counted
// (s < max_steps) and leaves when no chain of the tile is active -- every thread reads the sixteen
// flags behind a barrier, so the decision is block-uniform (net_forward holds barriers).  A chain that
// has arrived, or that the bound stopped, is PREDICATED: its column still rides through the product
// (the lanes are there anyway), but f never reaches its h.
//
// Modes (OnlineMode, njode_online_args.h): reset, advance, observe (the jump of k_gen_fwd for the
// chains with status 0), predict (Q targets, one readout of the tile per query; the state lives in
// LDS and is never written back), run (rounds of events: round k applies the k-th event of every
// chain's range ev_ptr[row] .. ev_ptr[row + 1] - 1, a walk of the tile, one readout of the tile, and
// the jump for the chains whose event is an observation; a chain whose range is exhausted, or that the
// bound stopped, idles as an arrived chain does.  The cursor and the range live in registers of lanes
// c < 16, the round's event, kind and range end per chain in the free words of S.misc, so the LDS
// size is that of the other modes.  h and now go to HBM once, at the end; last_X and tau have no raw
// copy in LDS (S.tx holds tanh(last_X)) and are written at each jump, as observe writes them).
// Eval mode: drop = false, rec = nullptr.
#pragma once
#include "njode_gen.h"
#include "njode_online_args.h"

namespace njode {
namespace gen {

// floats behind GLds: now[16], target[16] (float64), dt[16], t[16] (fp32 of the step in flight),
// active[16], alive[16], sid[16] (int)
constexpr int GON_CLOCK_FLOATS = 2 * 32 + 5 * 16;

// ode_input with the clock value per chain (tq[c]: fp32 of chain c's clock before the step)
NJ_DEV void ode_input_chain_t(const GArgs& a, lfp in, lfp tx, lfp h, lfp tau, lfp tq) {
  const int n = (a.D + a.H) * 16;
  for (int e = threadIdx.x; e < n; e += blockDim.x)
    in[pix(e)] = e < a.D * 16 ? tx[e] : tanh_acc(h[e - a.D * 16]);
  if (threadIdx.x < 16) {
    const int c = threadIdx.x;
    const float ta = tau[c], td = tq[c] - ta;
    in[pix((a.D + a.H) * 16 + c)] = ta;
    in[pix((a.D + a.H + 1) * 16 + c)] = td;
    if (a.curt) in[pix((a.D + a.H + 2) * 16 + c)] = ta + td;
    in[pix(a.IN0 * 16 + c)] = 1.0f;                                                        // bias unit
  }
}

__global__ void __launch_bounds__(1024) k_gen_online(GArgs a, OnlineArgs o, int PT, int mode) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  GLds S;
  S.carve((lfp)smem, a);
  const int tid = threadIdx.x, nth = blockDim.x;
  const int nlds = gen_lds_floats(a.img_rows, a.D, a.H, a.DO);
  for (int e = tid; e < nlds + GON_CLOCK_FLOATS; e += nth) ((lfp)smem)[e] = 0.0f;
  typedef double __attribute__((address_space(3))) * ldp;
  typedef int __attribute__((address_space(3))) * lip;
  lfp clk = (lfp)smem + nlds;                                  // (nlds is a multiple of 16 floats)
  ldp nowv = (ldp)clk, tgtv = (ldp)(clk + 32);
  lfp dtv = clk + 64, tqv = clk + 80;
  lip actv = (lip)(clk + 96), alive = (lip)(clk + 112), sidv = (lip)(clk + 128);
  lfp tau = S.misc;
  // run: the event of the round per chain (-1: none), its kind, the end of the chain's range, the
  // range's length -- S.misc + 16 .. + 79, which only the batch kernels use
  lip evv = (lip)(S.misc + 16), knd = (lip)(S.misc + 32), endv = (lip)(S.misc + 48), lenv = (lip)(S.misc + 64);
  const int r0 = blockIdx.x * PT;
  const int nv = o.n - r0 < PT ? o.n - r0 : PT;            // listed series of this tile
  const int D = a.D, H = a.H, DO = a.DO;
  const bool reset = mode == ONLINE_RESET, run = mode == ONLINE_RUN;
  int ev_cur = 0, ev_end = 0;                                  // run, lanes < 16: the chain's cursor and range end
  __syncthreads();
  // ---- the series of every chain; an id outside the state is not followed, nor is a range of
  // events outside the call
  if (tid < 16) {
    int sid = -1;
    if (tid < nv) {
      sid = o.ids ? o.ids[r0 + tid] : r0 + tid;
      if (sid < 0 || sid >= o.n_series) {
        sid = -1;
        if (!reset) o.status[r0 + tid] = 2;
        if (run) o.n_done[r0 + tid] = 0;
      } else if (run) {
        ev_cur = o.ev_ptr[r0 + tid];
        ev_end = o.ev_ptr[r0 + tid + 1];
        if (ev_cur < 0 || ev_end < ev_cur || ev_end > o.n_events) {
          sid = -1;
          ev_cur = ev_end = 0;
          o.status[r0 + tid] = 3;
          o.n_done[r0 + tid] = 0;
        }
      }
    }
    sidv[tid] = sid;
    alive[tid] = sid >= 0;
    if (run) {
      endv[tid] = ev_end;
      lenv[tid] = ev_end - ev_cur;
    }
  }
  __syncthreads();

  if (reset) {
    // h = encoder(start_X) with a zero mask (k_gen_fwd's start), last_X = start_X, tau = 0, now = 0
    for (int e = tid; e < D * 16; e += nth) {
      const int q = e >> 4, c = e & 15;
      S.xr[e] = sidv[c] >= 0 ? o.X[(size_t)(r0 + c) * D + q] : 0.0f;
      S.mk[e] = 0.0f;
    }
    __syncthreads();
    enc_input(a, S.img0, S.xr, S.mk);
    __syncthreads();
    lfp out = net_forward(a, a.enc, S.img0, S.img1, nullptr, false, 0u);
    img_get(S.h, out, H);
    __syncthreads();
    enc_residual(a, S.h, S.xr);
    __syncthreads();
    for (int e = tid; e < nv * H; e += nth) {
      const int c = e / H, j = e - c * H, sid = sidv[c];
      if (sid >= 0) o.h[(size_t)sid * H + j] = S.h[j * 16 + c];
    }
    for (int e = tid; e < nv * D; e += nth) {
      const int c = e / D, q = e - c * D, sid = sidv[c];
      if (sid >= 0) o.last_X[(size_t)sid * D + q] = S.xr[q * 16 + c];
    }
    if (tid < nv && sidv[tid] >= 0) {
      o.tau[sidv[tid]] = 0.0f;
      o.now[sidv[tid]] = 0.0;
    }
    return;
  }

  // ---- the tile's copy of the state (idle chains: zeros)
  for (int e = tid; e < nv * H; e += nth) {
    const int c = e / H, j = e - c * H, sid = sidv[c];
    if (sid >= 0) S.h[j * 16 + c] = o.h[(size_t)sid * H + j];
  }
  for (int e = tid; e < nv * D; e += nth) {
    const int c = e / D, q = e - c * D, sid = sidv[c];
    if (sid >= 0) S.tx[q * 16 + c] = tanh_acc(o.last_X[(size_t)sid * D + q]);
  }
  if (tid < nv && sidv[tid] >= 0) {
    tau[tid] = o.tau[sidv[tid]];
    nowv[tid] = o.now[sidv[tid]];
  }
  __syncthreads();

  const double delta_t = o.delta_t, eps_dt = o.eps_dt;
  // every live chain to the target in tgtv (lane c set chain c's); a chain the bound stops is no
  // longer alive
  auto walk_targets = [&]() __attribute__((always_inline)) {
    for (int s = 0; s < o.max_steps; ++s) {
      if (tid < 16) {
        const double now = nowv[tid], target = tgtv[tid];
        const double guard = target - eps_dt, last_full = target - delta_t;
        const bool act = alive[tid] && now < guard;
        if (act) {
          const double step = now < last_full ? delta_t : target - now;
          dtv[tid] = (float)step;
          tqv[tid] = (float)now;
          nowv[tid] = now + step;
        }
        actv[tid] = act;
      }
      __syncthreads();
      bool any = false;
#pragma unroll
      for (int c = 0; c < 16; ++c) any |= actv[c] != 0;
      if (!any) break;                                         // (block-uniform: sixteen LDS words)
      ode_input_chain_t(a, S.img0, S.tx, S.h, tau, tqv);
      __syncthreads();
      lfp out = net_forward(a, a.ode, S.img0, S.img1, nullptr, false, 0u);
      for (int e = tid; e < H * 16; e += nth)
        if (actv[e & 15]) S.h[e] = fmaf(dtv[e & 15], out[pix(e)], S.h[e]);
      __syncthreads();
    }
    if (tid < 16 && alive[tid] && nowv[tid] < tgtv[tid] - eps_dt) alive[tid] = 0;
    __syncthreads();
  };
  // ... to its q-th target of the call's row
  auto walk = [&](int q) {
    if (tid < 16 && alive[tid]) tgtv[tid] = o.t[(size_t)(r0 + tid) * o.Q + q];
    walk_targets();
  };
  // dst = readout(hs) of the tile (k_gen_fwd's emit_row)
  auto readout = [&](lfp dst, lfp hs) {
    dec_input(a, S.img0, hs);
    __syncthreads();
    lfp out = net_forward(a, a.dec, S.img0, S.img1, nullptr, false, 0u);
    img_get(dst, out, DO);
    __syncthreads();
    dec_residual(a, dst, hs);
    __syncthreads();
  };
  const float qnan = __uint_as_float(0x7fc00000u);
  auto write_y = [&](float* Y, size_t stride, size_t off, lfp src) {   // rows of the live chains, NaN for the stopped
    if (!Y) return;
    for (int e = tid; e < nv * DO; e += nth) {
      const int c = e / DO, j = e - c * DO;
      if (sidv[c] >= 0) Y[(size_t)(r0 + c) * stride + off + j] = alive[c] ? src[j * 16 + c] : qnan;
    }
  };

  if (mode == ONLINE_PREDICT) {
    for (int q = 0; q < o.Q; ++q) {
      walk(q);
      readout(S.y, S.h);
      write_y(o.Y, (size_t)o.Q * DO, (size_t)q * DO, S.y);
    }
    if (tid < nv && sidv[tid] >= 0) o.status[r0 + tid] = alive[tid] ? 0 : 1;
    return;
  }

  // S.ybj = readout(S.h) of the tile, in front of a jump
  auto readout_before = [&]() __attribute__((always_inline)) {
    dec_input(a, S.img0, S.h);
    __syncthreads();
    lfp out = net_forward(a, a.dec, S.img0, S.img1, nullptr, false, 0u);
    img_get(S.ybj, out, DO);
    __syncthreads();
    dec_residual(a, S.ybj, S.h);
  };
  // the jump of k_gen_fwd for the chains with S.rows >= 0 (S.rows[c]: chain c's row of X / M), behind
  // readout_before; S.y = readout(h_new); commit: h <- h_new, last_X <- X (masked: Y), tau <- fp32(t)
  auto jump = [&]() __attribute__((always_inline)) {
    for (int e = tid; e < D * 16; e += nth) {
      const int q = e >> 4, c = e & 15;
      const bool on = S.rows[c] >= 0;
      const size_t src = (size_t)(on ? S.rows[c] : 0) * D + q;
      S.xr[e] = on ? o.X[src] : 0.0f;
      S.mk[e] = a.masked ? (on ? o.M[src] : 0.0f) : 1.0f;
    }
    __syncthreads();
    if (a.rnn) {
      gru_jump_fwd(a, S, nullptr);
    } else {
      for (int e = tid; e < D * 16; e += nth)
        S.xin[e] = a.masked ? S.xr[e] * S.mk[e] + (1.0f - S.mk[e]) * S.ybj[e] : S.xr[e];
      __syncthreads();
      enc_input(a, S.img0, S.xin, S.mk);
      __syncthreads();
      lfp out = net_forward(a, a.enc, S.img0, S.img1, nullptr, false, 0u);
      img_get(S.hn, out, H);
      __syncthreads();
      enc_residual(a, S.hn, S.xin);
      __syncthreads();
    }
    // y = readout(h_new); the other chains keep their state
    for (int e = tid; e < H * 16; e += nth)
      if (S.rows[e & 15] < 0) S.hn[e] = S.h[e];
    __syncthreads();
    dec_input(a, S.img0, S.hn);
    __syncthreads();
    {
      lfp out = net_forward(a, a.dec, S.img0, S.img1, nullptr, false, 0u);
      for (int e = tid; e < DO * 16; e += nth) S.y[e] = out[pix(e)];
      __syncthreads();
      for (int e = tid; e < DO * 16; e += nth) {
        const int j = e >> 4, c = e & 15;
        float s = 0.0f;
        if (a.dec_case == 1) s = S.hn[(j % H) * 16 + c];
        else if (a.dec_case == 2) {
          for (int q = 0; q < a.dec_mult; ++q) s += S.hn[(q * DO + j) * 16 + c];
          s *= 1.0f / a.dec_mult;
        }
        S.y[e] += s;
      }
      __syncthreads();
    }
    for (int e = tid; e < H * 16; e += nth)
      if (S.rows[e & 15] >= 0) S.h[e] = S.hn[e];
    for (int e = tid; e < nv * D; e += nth) {
      const int c = e / D, q = e - c * D;
      if (S.rows[c] >= 0) o.last_X[(size_t)sidv[c] * D + q] = a.masked ? S.y[q * 16 + c] : S.xr[q * 16 + c];
    }
    if (run) {   // the next event's segment starts from the values the next call would load
      for (int e = tid; e < D * 16; e += nth)
        if (S.rows[e & 15] >= 0) S.tx[e] = tanh_acc(a.masked ? S.y[e] : S.xr[e]);
      if (tid < 16 && S.rows[tid] >= 0) tau[tid] = (float)tgtv[tid];
    }
    if (tid < nv && S.rows[tid] >= 0) o.tau[sidv[tid]] = (float)tgtv[tid];
    __syncthreads();
  };

  if (run) {
    // ---- rounds of events: as many as the tile's longest range (block-uniform: sixteen LDS words)
    int rounds = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) rounds = lenv[c] > rounds ? lenv[c] : rounds;
    for (int k = 0; k < rounds; ++k) {
      if (tid < 16) {
        const bool part = alive[tid] && ev_cur < ev_end;
        evv[tid] = part ? ev_cur : -1;
        knd[tid] = part && (!o.kind || o.kind[ev_cur] != 0);
        tgtv[tid] = part ? o.t[ev_cur] : -INFINITY;           // (no clock is below it: the chain idles)
      }
      __syncthreads();
      bool any = false;
#pragma unroll
      for (int c = 0; c < 16; ++c) any |= evv[c] >= 0;
      if (!any) break;                                         // (every chain left is stopped)
      walk_targets();
      if (tid < 16) S.rows[tid] = (alive[tid] && knd[tid]) ? evv[tid] : -1;
      readout_before();
      __syncthreads();
      bool anyj = false;
#pragma unroll
      for (int c = 0; c < 16; ++c) anyj |= S.rows[c] >= 0;
      if (anyj) jump();
      // the round's rows: an empty slice has the readout of the state it arrived at, twice; a chain
      // the bound stopped in this round has NaN from this event to the end of its range
      for (int e = tid; e < nv * DO; e += nth) {
        const int c = e / DO, j = e - c * DO, ev = evv[c];
        if (ev < 0 || !alive[c]) continue;
        if (o.Y_before) o.Y_before[(size_t)ev * DO + j] = S.ybj[j * 16 + c];
        if (o.Y) o.Y[(size_t)ev * DO + j] = S.rows[c] >= 0 ? S.y[j * 16 + c] : S.ybj[j * 16 + c];
      }
      for (int c = 0; c < nv; ++c) {
        if (evv[c] < 0 || alive[c]) continue;
        const size_t lo = (size_t)evv[c] * DO;
        const int cnt = (endv[c] - evv[c]) * DO;
        for (int e = tid; e < cnt; e += nth) {
          if (o.Y_before) o.Y_before[lo + e] = qnan;
          if (o.Y) o.Y[lo + e] = qnan;
        }
      }
      if (tid < 16 && evv[tid] >= 0 && alive[tid]) ++ev_cur;
      __syncthreads();
    }
    if (tid < nv && sidv[tid] >= 0) o.n_done[r0 + tid] = ev_cur - (ev_end - lenv[tid]);
  } else {
    walk(0);
  }
  if (mode == ONLINE_OBSERVE) {
    // ---- the chains that arrived take part
    if (tid < 16) S.rows[tid] = alive[tid] ? r0 + tid : -1;
    __syncthreads();
    bool any = false;
#pragma unroll
    for (int c = 0; c < 16; ++c) any |= S.rows[c] >= 0;
    if (any) {
      readout_before();
      jump();
    }
    write_y(o.Y_before, (size_t)DO, 0, S.ybj);
    write_y(o.Y, (size_t)DO, 0, S.y);
  }
  // ---- the state every listed series has reached, stopped ones included
  for (int e = tid; e < nv * H; e += nth) {
    const int c = e / H, j = e - c * H, sid = sidv[c];
    if (sid >= 0) o.h[(size_t)sid * H + j] = S.h[j * 16 + c];
  }
  if (tid < nv && sidv[tid] >= 0) {
    o.now[sidv[tid]] = nowv[tid];
    o.status[r0 + tid] = alive[tid] ? 0 : 1;
  }
}

}  // namespace gen
}  // namespace njode
