// njode_cfg.hip -- one model shape, compiled once per entry of the build table
// (njode_amd/build.py) and per NJ_PART (0 segment forward + registration,
// 1 segment backward, 2 lockstep forward, 3 lockstep backward, 4 / 5 the wave-per-path lockstep
// forward / adjoint sweep of njode_chain.h, 6 the online kernel of njode_online.h) with
//   -DNJ_ID=.. -DNJ_D=.. -DNJ_H=.. -DNJ_DO=.. -DNJ_NH=.. -DNJ_W=.. -DNJ_ACT=..
//   -DNJ_MASKED=.. -DNJ_CURT=.. -DNJ_RES=.. -DNJ_PART=..
// Every launcher here takes the call's Route (njode_route.h) and switches on it: which kernel runs is
// decided there, once, and nothing in this file reads a switch or derives a route of its own.  Launch
// errors: the helpers return nothing; HIP keeps the last error of the thread until it is read, and the
// one hipGetLastError() at the end of each entry point (njode_seg_forward_ ...) reads it.
#include <type_traits>

#include "njode_route.h"
#if NJ_PART >= 4
#include "njode_chain.h"
#include "njode_chain_seg.h"
#include "njode_chain_dw.h"
#endif
#if NJ_PART == 6
#include "njode_online.h"
#endif

#define NJ_CAT_(a, b) a##b
#define NJ_CAT(a, b) NJ_CAT_(a, b)

namespace njode {

#ifndef NJ_RNN
#define NJ_RNN 0
#endif
using C = Cfg<NJ_D, NJ_H, NJ_DO, NJ_NH, NJ_W, NJ_ACT, (NJ_MASKED != 0), (NJ_CURT != 0),
              (NJ_RES != 0), (NJ_RNN != 0)>;

hipError_t NJ_CAT(njode_seg_forward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st);
hipError_t NJ_CAT(njode_seg_backward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st);
constexpr bool HAS_MFMA = C::NH == 2 && !C::MASKED && !C::RNN && C::DO <= 16 && C::W < 64;
// the lockstep forward on the matrix cores also covers masked shapes
constexpr bool HAS_MFMA_LOCK = C::NH == 2 && !C::RNN && C::W < 64 && C::H <= 64 && C::DO <= 64;
// ... and so does its adjoint sweep, unless the encoder's identity path folds units
constexpr bool HAS_MFMA_SWEEP =
    HAS_MFMA_LOCK && (!C::MASKED || C::ENC_CASE == 0 || (C::ENC_CASE == 1 && C::D == C::H));
constexpr bool HAS_SPLIT = HAS_MFMA && SplitOk<C>::value;
// masked shapes: one tile over the four waves of a block (njode_mfma_lock4.h; Route: LOCK_TILE4)
constexpr bool HAS_Q4 = HAS_MFMA_SWEEP && Q4Ok<C>::value;
// ... or one wave per path (njode_chain.h; Route: LOCK_CHAIN)
constexpr bool HAS_CHAIN = HAS_Q4 && ChainOk<C>::value;
void NJ_CAT(njode_chain_forward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st);
void NJ_CAT(njode_chain_sweep_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st);
// dW of the ODE network from the wave-per-chain sweeps' records (njode_chain_dw.h; part 5; Route::dw_stored)
void NJ_CAT(njode_chain_dw_, NJ_ID)(const KArgs& a, hipStream_t st);
// the segment plan's ODE kernels with one wave per item (njode_chain_seg.h; Route::seg_chain)
constexpr bool HAS_SEG_CHAIN = HAS_SPLIT && HAS_MFMA_SWEEP && SegChainOk<C>::value;
void NJ_CAT(njode_seg_chain_forward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st);
void NJ_CAT(njode_seg_chain_backward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st);

// f(std::true_type) when the call draws dropout masks, else f(std::false_type): the kernels take it as a
// template argument
template <class F> static auto with_drop(bool drop, F f) {
  return drop ? f(std::true_type{}) : f(std::false_type{});
}
// Profile scope names of the ODE kernels a route runs: the launched kernels', as rocprofv3 lists them
static inline const char* seg_fwd_name(const Route& r, bool tails) {
  if (r.seg_ode != ODE_MFMA) return tails ? "k_ode_fwd_items.tails" : "k_ode_fwd_items";
  if (r.seg_chain) return "k_seg_fwd_chain";   // (the tails ride)
  if (r.ode_split) return tails ? "k_ode_fwd_split.tails" : "k_ode_fwd_mixed";
  return tails ? "k_ode_fwd_mfma.tails" : "k_ode_fwd_mfma";
}
static inline const char* lock_name(int kind, bool bwd) {
  if (kind == LOCK_VALU) return bwd ? "k_paths_bwd_adj" : "k_paths_fwd";
  if (kind == LOCK_CHAIN) return bwd ? "k_paths_bwd_adj_chain" : "k_paths_fwd_chain";
  return bwd ? "k_paths_bwd_adj_mfma" : "k_paths_fwd_mfma";
}
template <bool ON, class CC> struct FragSize {
  static constexpr int ode = 0, enc = 0, dec = 0;
};
template <class CC> struct FragSize<true, CC> {
  static constexpr int ode = MF<CC>::NALL * 64;
  static constexpr int enc = EncS<CC>::type::NALL * 64;
  static constexpr int dec = DecS<CC>::type::NALL * 64;
};
using FS = FragSize<(HAS_MFMA || HAS_MFMA_LOCK), C>;
constexpr int MF_FLOATS = FS::ode + FS::enc + FS::dec + FS::ode;   // + the scaled ODE table (frag2)
constexpr int FRAG2_OFF = FS::ode + FS::enc + FS::dec;
template <bool ON, class CC> struct ActSize { static constexpr int value = 0; };
template <class CC> struct ActSize<true, CC> { static constexpr int value = StepRec<CC>::PER_CHAIN; };
constexpr int ACT_FLOATS = ActSize<HAS_SPLIT, C>::value;   // stored activations: demo-family shapes

// All fragment tables of the three networks in ONE launch instead of three in
// front of the encoder rows (each of these launches costs ~5 us of a chain that sits on the
// step's critical path once the plan is built ahead)
template <class C, class ES, class DS>
__global__ void k_pack_all(const float* __restrict__ P, float* __restrict__ frag, float* __restrict__ frag2,
                           float* __restrict__ frag_enc, float* __restrict__ frag_dec, float ik,
                           unsigned* __restrict__ zero8) {
  constexpr int N = MF<C>::NALL * 64, NE = ES::NALL * 64, ND = DS::NALL * 64;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (zero8 && idx < 8) zero8[idx] = 0;   // (KArgs::plan_sync_zero)
  if (idx < N) frag[idx] = ode_frag_value<C>(P, idx, 1.0f, 1.0f);
  else if (idx < 2 * N) frag2[idx - N] = ode_frag_value<C>(P, idx - N, Ode2Scale<C>::S, ik);
  else if (idx < 2 * N + NE) pack_net_value<typename C::Enc, ES>(P + C::OFF_ENC, frag_enc, idx - 2 * N);
  else if (idx < 2 * N + NE + ND) pack_net_value<typename C::Dec, DS>(P + C::OFF_DEC, frag_dec, idx - 2 * N - NE);
}
// ... and, in the same launch, the keep bits of the ODE forward's four-wave role (blocks behind the
// n_pack packing blocks: njode_mfma_split.h, drop_bits_tile_steps): no launch, no stream hop of
// their own, parallel over the chip, before the forward kernel starts
template <class C, class ES, class DS>
__global__ void k_pack_all_bits(KArgs a, int n_pack) {
  if ((int)blockIdx.x < n_pack) {
    constexpr int N = MF<C>::NALL * 64, NE = ES::NALL * 64, ND = DS::NALL * 64;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (a.plan_sync_zero && idx < 8) a.plan_sync_zero[idx] = 0;
    if (idx < N) a.frag[idx] = ode_frag_value<C>(a.P, idx, 1.0f, 1.0f);
    else if (idx < 2 * N) a.frag2[idx - N] = ode_frag_value<C>(a.P, idx - N, Ode2Scale<C>::S, a.dc.inv_keep);
    else if (idx < 2 * N + NE) pack_net_value<typename C::Enc, ES>(a.P + C::OFF_ENC, a.frag_enc, idx - 2 * N);
    else if (idx < 2 * N + NE + ND) pack_net_value<typename C::Dec, DS>(a.P + C::OFF_DEC, a.frag_dec, idx - 2 * N - NE);
  } else {
    if constexpr (SegChainOk<C>::value) {
      if (a.seg_chain) {   // (the wave-per-item forward's lane masks: njode_chain_seg.h)
        seg_chain_bits_body<C>(a, (int)blockIdx.x - n_pack, (int)gridDim.x - n_pack);
        return;
      }
    }
    if constexpr (HAS_SPLIT) {
      const int nb = (int)gridDim.x - n_pack;
      drop_bits_tile_steps<C>(a, ((int)blockIdx.x - n_pack) * 4 + (threadIdx.x >> 6), nb * 4);
    }
  }
}

// MFMA launches live in templates on the configuration so that `if constexpr` really
// discards them for shapes the matrix-core kernels are not written for
// (bits: the plan is complete on this stream -- the call has no helper stream -- and the forward
// will draw dropout masks: KArgs::dbits_ready)
template <class CC> static void launch_pack_frags(const KArgs& a, hipStream_t st, bool bits = false) {
  if constexpr (HAS_MFMA) {
    using ES = typename EncS<CC>::type;
    using DS = typename DecS<CC>::type;
    const int n_pack = cdiv((2 * MF<CC>::NALL + ES::NALL + DS::NALL) * 64, 256);
    if (bits) {
      // one wave per 8 Euler steps of a four-wide tile; the number of such tiles is known on the
      // device only: enough waves for the small plans (every tile four-wide), a persistent
      // grid for the large ones
      const long long work = a.seg_chain ? (long long)a.K * a.B / 64 + 1   // (256 (path, step) pairs per block)
                                         : (long long)cdiv(a.n_obs, 16) * cdiv(a.K > 0 ? a.K : 1, 8);
      const int nb = (int)(work / 4 + 1 < 1024 ? work / 4 + 1 : 1024);
      k_pack_all_bits<CC, ES, DS><<<n_pack + nb, 256, 0, st>>>(a, n_pack);
    } else {
      k_pack_all<CC, ES, DS><<<n_pack, 256, 0, st>>>(a.P, a.frag, a.frag2, a.frag_enc, a.frag_dec, a.dc.inv_keep,
                                                  a.plan_sync_zero);
    }
  }
}
template <class CC, bool DROP> static void launch_mfma_enc(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (HAS_MFMA) {
    const int n_tiles = cdiv(a.n_obs + a.B, 16);
    // one-wave blocks, 64 VGPRs: four waves per SIMD hide the row gathers (obs_idx -> path,
    // t_of_row -> k_jump, X) each tile starts with: 51 -> 37 us for 219 470 rows (the step time
    // does not move: the plan on the helper stream is the critical path beside this kernel);
    // Route::enc_blocks: 4 096, NJODE_ENC_BLOCKS overrides (A/B)
    k_encode_rows_mfma<CC, DROP><<<n_tiles < r.enc_blocks ? n_tiles : r.enc_blocks, 64, 0, st>>>(a);
  }
}
// the three fragment tables of the lockstep plan's matrix-core kernels (parts 2 and 3)
template <class CC> static void lock_pack_frags(const KArgs& a, hipStream_t st) {
  if constexpr (HAS_MFMA_LOCK) {
    using ES = typename EncS<CC>::type;
    using DS = typename DecS<CC>::type;
    k_pack_frags<CC><<<cdiv(MF<CC>::NALL * 64, 256), 256, 0, st>>>(a.P, a.frag);
    k_pack_net<typename CC::Enc, ES><<<cdiv(ES::NALL * 64, 256), 256, 0, st>>>(a.P + CC::OFF_ENC,
                                                                             a.frag_enc);
    k_pack_net<typename CC::Dec, DS><<<cdiv(DS::NALL * 64, 256), 256, 0, st>>>(a.P + CC::OFF_DEC,
                                                                             a.frag_dec);
  }
}
template <class CC, bool DROP> static void launch_mfma_jump(const KArgs& a, hipStream_t st) {
  if constexpr (HAS_MFMA) {
    const int n_tiles = cdiv(a.n_obs, 16);
    k_jump_rows_mfma<CC, DROP><<<n_tiles < 2048 ? n_tiles : 2048, 64, 0, st>>>(a);
  }
}
template <class CC, bool DROP> static void launch_ode_bwd_mfma(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (HAS_MFMA) {
    if constexpr (HAS_SPLIT) {
      if (r.ode_split) {
        ProfScope ps("k_ode_bwd_mixed", st);
        k_ode_bwd_mixed<CC, DROP><<<a.n_blocks_bwd, 256, 0, st>>>(a);
        return;
      }
    }
    ProfScope ps("k_ode_bwd_mfma", st);
    k_ode_bwd_mfma<CC, DROP><<<a.n_waves_ode / 4, 256, 0, st>>>(a);
  }
}
template <class CC, bool DROP> static void launch_jump_rows_bwd(const KArgs& a, hipStream_t st) {
  if constexpr (HAS_MFMA) {
    ProfScope ps("k_jump_rows_bwd_mfma", st);
    k_jump_rows_bwd_mfma<CC, DROP><<<a.n_waves_rows / 4, 256, 0, st>>>(a);
  }
}
template <class CC, bool DROP>
static void launch_mfma_rows_bwd(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (HAS_MFMA) {
    // (defer_loss == 2, NJODE_C_ROWS_IN_FWD: the forward call already ran this pass)
    if (r.defer_loss != 2) launch_jump_rows_bwd<CC, DROP>(a, st);
    if (r.seg_chain) NJ_CAT(njode_seg_chain_backward_, NJ_ID)(a, r, st);
    else launch_ode_bwd_mfma<CC, DROP>(a, r, st);
    if (!r.dw_enc_fused) {   // (else a role of k_ode_dw_stored_enc's launch)
      ProfScope ps("k_encode_rows_bwd_mfma", st);
      k_encode_rows_bwd_mfma<CC, DROP><<<a.n_waves_rows / 4, 256, 0, st>>>(a);
    }
  }
}
template <class CC, bool DROP, bool TAIL>
static void launch_mfma_fwd(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (HAS_MFMA) {
    const int n_tiles = cdiv(TAIL ? a.B : a.n_obs, 16);
    if constexpr (HAS_SPLIT) {
      if (r.ode_split) {
        if constexpr (TAIL) {
          // (the four-wave form for every plan: one wave per tile for the large ones was measured
          // beside the items' forward on the autograd route and slower, 1.121 against 1.075 ms per
          // step -- profiles/r05_rejected_experiments.txt, item 2)
          k_ode_fwd_split<CC, DROP, true><<<n_tiles < 1024 ? n_tiles : 1024, 256, 0, st>>>(a);
        }
        else if (a.plan_job) {
          // the next batch's plan rides in front of this launch's own blocks (njode_plan.h)
          const PlanJob job = *(const PlanJob*)a.plan_job;
          k_ode_fwd_mixed_plan<CC, DROP><<<a.n_blocks_fwd + job.P, 256, 0, st>>>(a, job);
        }
        else k_ode_fwd_mixed<CC, DROP><<<a.n_blocks_fwd, 256, 0, st>>>(a);
        return;
      }
    }
    k_ode_fwd_mfma<CC, DROP, TAIL><<<n_tiles < 4096 ? n_tiles : 4096, 64, 0, st>>>(a);
  }
}

hipError_t NJ_CAT(njode_lock_forward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st);
hipError_t NJ_CAT(njode_lock_backward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st);

#if NJ_PART == 0
template <bool DROP, bool TAIL, int ODE> static void launch_ode_fwd(const KArgs& a, const Route& r, hipStream_t st) {
  const int n_items = TAIL ? a.B : a.n_obs;
  if constexpr (ODE == ODE_MFMA) {
    launch_mfma_fwd<C, DROP, TAIL>(a, r, st);
  } else {
    k_ode_fwd_items<C, DROP, TAIL><<<cdiv(n_items, 64), 64, 0, st>>>(a);
  }
}
template <bool DROP, int ODE>
static hipError_t seg_forward_t(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (C::MASKED || C::RNN) {
    return hipErrorNotSupported;
  } else {
    // pack + encoder rows: on the call's helper stream when there is one (they only need
    // t_of_row; the plan kernels already sit on `st`), else in line
    const SideInfo* side = r.side ? (const SideInfo*)a.plan_ready : nullptr;
    hipStream_t s2 = side ? side->st : st;
    if (side) (void)hipStreamWaitEvent(s2, side->e0, 0);
    KArgs ab = a;   // (a copy of the arguments: dbits_ready, plan_sync_zero)
    if constexpr (ODE == ODE_MFMA) {
      ab.dbits_ready = r.seg_bits_ahead ? 1 : 0;
      if (ab.plan_sync_zero && s2 != st) {   // (the pack launch is not on the hosting launch's stream)
        (void)hipMemsetAsync(ab.plan_sync_zero, 0, 8 * sizeof(unsigned), st);
        ab.plan_sync_zero = nullptr;
      }
      ProfScope ps("k_pack_all", s2);
      launch_pack_frags<C>(ab, s2, r.seg_bits_ahead);
    }
    {
      ProfScope ps(ODE == ODE_MFMA ? "k_encode_rows_mfma" : "k_encode_rows", s2);
      if constexpr (ODE == ODE_MFMA) launch_mfma_enc<C, DROP>(a, r, s2);
      else k_encode_rows<C, DROP><<<cdiv(a.n_obs + a.B, 64), 64, 0, s2>>>(a);
    }
    if (side) {
      (void)hipEventRecord(side->e1, s2);
      (void)hipStreamWaitEvent(st, side->e1, 0);
    }
    // the tails (hT: every path from its last observation to the end) need the encoder's outputs
    // and nothing else of this call: with helper streams they start TOGETHER with the items' ODE
    // forward, on a stream of their own, and share the chip with it
    if (r.tails_side) {
      // the tails' stream waits for the encoder rows and for the plan's tail order: the latter is
      // on that stream itself (njode_planner.hip, build_plan) or, failing that, on `st` -- then e0,
      // which the helper stream consumed above, is recorded again here to stand for "everything
      // `st` has enqueued by now"
      (void)hipStreamWaitEvent(side->st2, side->e1, 0);
      if (!side->tails_sorted_on_st2) {
        (void)hipEventRecord(side->e0, st);
        (void)hipStreamWaitEvent(side->st2, side->e0, 0);
      }
    }
    {
      ProfScope ps(seg_fwd_name(r, false), st);
      if (r.seg_chain) NJ_CAT(njode_seg_chain_forward_, NJ_ID)(ab, r, st);
      else launch_ode_fwd<DROP, false, ODE>(ab, r, st);
    }
    if (r.tails_side) {
      // (queued behind the forward's launch only so that the items' kernel is dispatched first)
      ProfScope ps(seg_fwd_name(r, true), side->st2);
      launch_ode_fwd<DROP, true, ODE>(a, r, side->st2);
      (void)hipEventRecord(side->e2, side->st2);
    } else if (r.tails && !r.tails_ride) {
      ProfScope ps(seg_fwd_name(r, true), st);
      launch_ode_fwd<DROP, true, ODE>(a, r, st);
    }
    if (r.defer_loss == 2) {
      // NJODE_C_ROWS_IN_FWD: the backward's row pass here (loss terms, readout gradients, adjoints
      // at the segment ends) instead of the forward-only pass
      launch_jump_rows_bwd<C, DROP>(a, st);
    } else if (!r.defer_loss) {
      ProfScope ps(ODE == ODE_MFMA ? "k_jump_rows_mfma" : "k_jump_rows", st);
      if constexpr (ODE == ODE_MFMA) launch_mfma_jump<C, DROP>(a, st);
      else k_jump_rows<C, DROP><<<cdiv(a.n_obs, 64), 64, 0, st>>>(a);
    }
    if (r.tails_side) (void)hipStreamWaitEvent(st, side->e2, 0);
    return hipGetLastError();
  }
}
hipError_t NJ_CAT(njode_seg_forward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st) {
  return with_drop(r.drop, [&](auto D) {
    constexpr bool DROP = decltype(D)::value;
    return r.seg_ode == ODE_MFMA ? seg_forward_t<DROP, ODE_MFMA>(a, r, st) : seg_forward_t<DROP, ODE_VALU>(a, r, st);
  });
}

const CfgOps* NJ_CAT(njode_cfg_ops_, NJ_ID)() {
  static const CfgOps ops = {
      {NJ_D, NJ_H, NJ_DO, NJ_NH, (NJ_NH > 0 ? NJ_W : 0), NJ_ACT,
       (NJ_MASKED ? NJODE_F_MASKED : 0) | (NJ_CURT ? NJODE_F_INPUT_CURRENT_T : 0) |
           (NJ_RES ? NJODE_F_RESIDUAL : 0) | (NJ_RNN ? NJODE_F_USE_RNN : 0)},
      C::P,
      C::ODE_IN,
      C::ENC_IN,
      C::OFF_ENC,
      C::OFF_DEC,
      NJ_CAT(njode_seg_forward_, NJ_ID),
      NJ_CAT(njode_seg_backward_, NJ_ID),
      NJ_CAT(njode_lock_forward_, NJ_ID),
      NJ_CAT(njode_lock_backward_, NJ_ID),
      MF_FLOATS,
      FS::ode,
      FS::ode + FS::enc,
      FRAG2_OFF,
      ACT_FLOATS,
      HAS_Q4 ? Q4_ACT_FLOATS : 0,
      HAS_MFMA_LOCK ? 1 : 0,
      HAS_MFMA_SWEEP ? 1 : 0,
      HAS_CHAIN ? 1 : 0,
      HAS_SEG_CHAIN ? 1 : 0,
      HAS_SPLIT ? 1 : 0,
      HAS_MFMA ? 1 : 0};
  return &ops;
}
#endif

#if NJ_PART == 1
template <bool DROP, int ODE> static hipError_t seg_backward_t(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (C::MASKED || C::RNN) {
    return hipErrorNotSupported;
  } else if constexpr (ODE == ODE_MFMA) {
    launch_mfma_rows_bwd<C, DROP>(a, r, st);
    return hipGetLastError();
  } else {
    {
      ProfScope ps("k_jump_rows_bwd", st);
      k_jump_rows_bwd<C, DROP><<<a.n_waves, 64, 0, st>>>(a);
    }
    {
      ProfScope ps("k_ode_bwd_items", st);
      k_ode_bwd_items<C, DROP><<<a.n_waves, 64, 0, st>>>(a);
    }
    {
      ProfScope ps("k_encode_rows_bwd", st);
      k_encode_rows_bwd<C, DROP><<<a.n_waves, 64, 0, st>>>(a);
    }
    return hipGetLastError();
  }
}
hipError_t NJ_CAT(njode_seg_backward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st) {
  return with_drop(r.drop, [&](auto D) {
    constexpr bool DROP = decltype(D)::value;
    return r.seg_ode == ODE_MFMA ? seg_backward_t<DROP, ODE_MFMA>(a, r, st) : seg_backward_t<DROP, ODE_VALU>(a, r, st);
  });
}
#endif

#if NJ_PART == 2
template <class CC, bool DROP> static void lock_launch_mfma(const KArgs& a, const Route& r, hipStream_t st) {
  if (r.lock_fwd_kind == LOCK_CHAIN) {
    NJ_CAT(njode_chain_forward_, NJ_ID)(a, r, st);
  } else if (r.lock_fwd_kind == LOCK_TILE4) {
    if constexpr (HAS_Q4) {
      const int n_tiles = cdiv(a.B, a.q4_pt);
      KArgs ab = a;
      if (r.lock_bits_ahead) {
        // the keep bits of every evaluation of the forward, drawn ahead in parallel over the chip
        const long long items = (long long)a.K * n_tiles;
        const int nb = (int)(items / 4 + 1 < 2048 ? items / 4 + 1 : 2048);
        k_q4_bits<CC><<<nb, 256, 0, st>>>(a, n_tiles);
        ab.dbits_ready = 1;
      }
      k_paths_fwd_q4<CC, DROP><<<n_tiles, 256, 0, st>>>(ab);
    }
  } else {
    if constexpr (HAS_MFMA_LOCK) k_paths_fwd_mfma<CC, DROP><<<cdiv(a.B, 32), 128, 0, st>>>(a);
  }
}
template <bool DROP> static hipError_t lock_t(KArgs a, const Route& r, hipStream_t st) {
  a.want_path = r.want_path ? 1 : 0;
  a.want_loss = r.want_loss ? 1 : 0;
  // (the wave-per-path kernels read the flat parameter vector themselves)
  if (r.lock_fwd_kind == LOCK_WAVE1 || r.lock_fwd_kind == LOCK_TILE4) lock_pack_frags<C>(a, st);
  ProfScope ps(lock_name(r.lock_fwd_kind, false), st);
  if (r.lock_fwd_kind == LOCK_VALU) k_paths_fwd<C, DROP><<<cdiv(a.B, 64), 64, 0, st>>>(a);
  else lock_launch_mfma<C, DROP>(a, r, st);
  return hipGetLastError();
}
hipError_t NJ_CAT(njode_lock_forward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st) {
  return with_drop(r.drop, [&](auto D) { return lock_t<decltype(D)::value>(a, r, st); });
}
#endif

#if NJ_PART == 3
template <class CC, bool DROP> static void lock_bwd_mfma(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (HAS_MFMA_SWEEP) {
    lock_pack_frags<CC>(a, st);
    {
      // (the family whose records the saving forward wrote: Route::lock_bwd_kind)
      ProfScope ps(lock_name(r.lock_bwd_kind, true), st);
      if (r.lock_bwd_kind == LOCK_CHAIN) {
        NJ_CAT(njode_chain_sweep_, NJ_ID)(a, r, st);
      } else if (r.lock_bwd_kind == LOCK_TILE4) {
        if constexpr (HAS_Q4) k_paths_bwd_adj_q4<CC, DROP><<<cdiv(a.B, a.q4_pt), 256, 0, st>>>(a);
      } else {
        k_paths_bwd_adj_mfma<CC, DROP><<<cdiv(a.B, 16), 64, 0, st>>>(a);
      }
    }
    if (r.dw_stored) {
      NJ_CAT(njode_chain_dw_, NJ_ID)(a, st);
    } else {
      ProfScope ps("k_ode_dw_pairs_mfma", st);
      k_ode_dw_pairs_mfma<CC, DROP><<<a.n_waves_rows / 4, 256, 0, st>>>(a);
    }
    {
      ProfScope ps("k_dec_dw_rows_mfma", st);
      k_dec_dw_rows_mfma<CC, DROP><<<a.n_waves_rows / 4, 256, 0, st>>>(a);
    }
    {
      ProfScope ps("k_enc_dw_rows_mfma", st);
      k_enc_dw_rows_mfma<CC, DROP><<<a.n_waves_rows / 4, 256, 0, st>>>(a);
    }
  }
}
// The one-lane-per-path sweep holds a path's whole state in registers: fine for the small
// unmasked shapes, but the 41-dimensional masked ones spill thousands of registers, so
// masked shapes are only differentiated on the matrix cores.
template <class CC, bool DROP> static hipError_t lock_bwd_valu(const KArgs& a, hipStream_t st) {
  if constexpr (CC::MASKED) {
    return hipErrorNotSupported;
  } else {
    {
      ProfScope ps(lock_name(LOCK_VALU, true), st);
      k_paths_bwd_adj<CC, DROP><<<cdiv(a.B, 64), 64, 0, st>>>(a);
    }
    {
      ProfScope ps("k_ode_dw_pairs", st);
      k_ode_dw_pairs<CC, DROP><<<a.n_waves, 64, 0, st>>>(a);
    }
    {
      ProfScope ps("k_dec_dw_rows", st);
      k_dec_dw_rows<CC, DROP><<<a.n_waves, 64, 0, st>>>(a);
    }
    {
      ProfScope ps("k_enc_dw_rows", st);
      k_enc_dw_rows<CC, DROP><<<a.n_waves, 64, 0, st>>>(a);
    }
    if constexpr (CC::RNN) {
      ProfScope ps("k_gru_dw_rows", st);
      k_gru_dw_rows<CC><<<a.n_waves, 64, 0, st>>>(a);
    }
    return hipGetLastError();
  }
}
template <bool DROP> static hipError_t lock_bwd_t(const KArgs& a, const Route& r, hipStream_t st) {
  if (r.lock_bwd_kind == LOCK_VALU) return lock_bwd_valu<C, DROP>(a, st);
  lock_bwd_mfma<C, DROP>(a, r, st);
  return hipGetLastError();
}
hipError_t NJ_CAT(njode_lock_backward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st) {
  return with_drop(r.drop, [&](auto D) { return lock_bwd_t<decltype(D)::value>(a, r, st); });
}
#endif

// Parts 4 and 5, the wave-per-chain kernels.  Their launches too live in templates on the configuration
// (`if constexpr` then discards them for the other shapes); the functions the other parts call wrap them.
#if NJ_PART == 4
template <class CC> static void chain_forward(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (HAS_CHAIN) {
    const int wpb = r.chain_wpb;
    if (r.drop) {
      const long long items = (long long)a.K * a.B + (long long)a.n_obs * 3 + a.B;
      const int nb = (int)(items / 256 + 1 < 4096 ? items / 256 + 1 : 4096);
      k_chain_bits<CC><<<nb, 256, 0, st>>>(a);
    }
    with_drop(r.drop, [&](auto D) {
      k_paths_fwd_chain<CC, decltype(D)::value><<<cdiv(a.B, wpb), 64 * wpb, 0, st>>>(a);
    });
  }
}
template <class CC> static void seg_chain_forward(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (HAS_SEG_CHAIN) {
    const int nb = cdiv(a.n_obs + a.B, 4), tails = r.tails_ride ? 1 : 0;
    if (r.drop && !a.dbits_ready) {
      const long long items = (long long)a.K * a.B;
      k_seg_chain_bits<CC><<<(int)(items / 256 + 1 < 2048 ? items / 256 + 1 : 2048), 256, 0, st>>>(a);
    }
    with_drop(r.drop, [&](auto D) {
      if (a.plan_job) {
        // the next batch's plan rides in front of this launch's own blocks (njode_plan.h)
        const PlanJob job = *(const PlanJob*)a.plan_job;
        k_seg_fwd_chain_plan<CC, decltype(D)::value><<<nb + job.P, 256, 0, st>>>(a, tails, job);
      } else {
        k_seg_fwd_chain<CC, decltype(D)::value><<<nb, 256, 0, st>>>(a, tails);
      }
    });
  }
}
void NJ_CAT(njode_chain_forward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st) { chain_forward<C>(a, r, st); }
void NJ_CAT(njode_seg_chain_forward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st) {
  seg_chain_forward<C>(a, r, st);
}
#endif

#if NJ_PART == 5
template <class CC> static void chain_dw(const KArgs& a, hipStream_t st) {
  if constexpr ((HAS_CHAIN || HAS_SEG_CHAIN) && C::W < 64) {
    ProfScope ps("k_ode_dw_stored", st);
    k_ode_dw_stored<CC><<<a.dw_pair_blocks + a.dw_seg_blocks, 256, 0, st>>>(a, a.dw_pair_blocks);
  }
}
template <class CC> static void chain_dw_enc(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (HAS_SEG_CHAIN && C::W < 64) {
    ProfScope ps("k_ode_dw_stored_enc", st);
    const int nb = a.dw_pair_blocks + a.dw_seg_blocks + a.n_waves_rows / 4;
    with_drop(r.drop, [&](auto D) {
      k_ode_dw_stored_enc<CC, decltype(D)::value><<<nb, 256, 0, st>>>(a, a.dw_pair_blocks, a.dw_seg_blocks);
    });
  }
}
template <class CC> static void seg_chain_backward(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (HAS_SEG_CHAIN) {
    {
      ProfScope ps("k_seg_bwd_chain", st);
      with_drop(r.drop, [&](auto D) { k_seg_bwd_chain<CC, decltype(D)::value><<<cdiv(a.n_obs, 4), 256, 0, st>>>(a); });
    }
    // d loss / d ODE parameters: from the sweep's records (with the encoder's pass in the same launch),
    // else the lockstep plan's pair kernel on the stored adjoints
    if (r.dw_enc_fused) {
      chain_dw_enc<CC>(a, r, st);
    } else if (r.dw_stored) {
      chain_dw<CC>(a, st);
    } else {
      ProfScope ps("k_ode_dw_pairs_mfma", st);
      with_drop(r.drop, [&](auto D) {
        k_ode_dw_pairs_mfma<CC, decltype(D)::value><<<a.n_waves_rows / 4, 256, 0, st>>>(a);
      });
    }
  }
}
template <class CC> static void chain_sweep(const KArgs& a, const Route& r, hipStream_t st) {
  if constexpr (HAS_CHAIN) {
    const int wpb = r.chain_wpb;
    with_drop(r.drop, [&](auto D) {
      k_paths_bwd_adj_chain<CC, decltype(D)::value><<<cdiv(a.B, wpb), 64 * wpb, 0, st>>>(a);
    });
  }
}
void NJ_CAT(njode_seg_chain_backward_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st) {
  seg_chain_backward<C>(a, r, st);
}
void NJ_CAT(njode_chain_dw_, NJ_ID)(const KArgs& a, hipStream_t st) { chain_dw<C>(a, st); }
void NJ_CAT(njode_chain_sweep_, NJ_ID)(const KArgs& a, const Route& r, hipStream_t st) { chain_sweep<C>(a, r, st); }
#endif

// Part 6, the online kernel (njode_online.hip finds the shape's entry by name: njode_online_ops_<id>)
#if NJ_PART == 6
template <class CC> static hipError_t online_launch(const OnlineArgs& a, int mode, hipStream_t st) {
  if constexpr (OnlineOk<CC>::value) {
    const dim3 grid(cdiv(a.n, a.spb)), block(64 * ONLINE_WAVES);
    ProfScope ps("k_online", st);
    if (mode == ONLINE_ADVANCE) k_online<CC, ONLINE_ADVANCE><<<grid, block, 0, st>>>(a);
    else if (mode == ONLINE_OBSERVE) k_online<CC, ONLINE_OBSERVE><<<grid, block, 0, st>>>(a);
    else if (mode == ONLINE_PREDICT) k_online<CC, ONLINE_PREDICT><<<grid, block, 0, st>>>(a);
    else if (mode == ONLINE_RUN) k_online<CC, ONLINE_RUN><<<grid, block, 0, st>>>(a);
    else k_online<CC, ONLINE_RESET><<<grid, block, 0, st>>>(a);
    return hipGetLastError();
  } else {
    return hipErrorNotSupported;
  }
}
static hipError_t online_launch_c(const OnlineArgs& a, int mode, hipStream_t st) { return online_launch<C>(a, mode, st); }
const OnlineOps* NJ_CAT(njode_online_ops_, NJ_ID)() {
  static const OnlineOps ops = {
      {NJ_D, NJ_H, NJ_DO, NJ_NH, (NJ_NH > 0 ? NJ_W : 0), NJ_ACT,
       (NJ_MASKED ? NJODE_F_MASKED : 0) | (NJ_CURT ? NJODE_F_INPUT_CURRENT_T : 0) |
           (NJ_RES ? NJODE_F_RESIDUAL : 0) | (NJ_RNN ? NJODE_F_USE_RNN : 0)},
      OnlineOk<C>::value ? 1 : 0,
      online_launch_c};
  return &ops;
}
#endif

}  // namespace njode

#if defined(NJ_BWD_STAMPS) && NJ_PART == 1
// diagnostic build only (tools/ubench/bwd_stamps.sh): the per-wave stamps of k_ode_bwd_mixed
extern "C" int njode_debug_bwd_stamps(unsigned long long* dst, unsigned long long n_words) {
  const size_t cap = sizeof(njode::g_bwd_stamps) / 8;
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(njode::g_bwd_stamps),
                                  (n_words < cap ? n_words : cap) * 8);
}
#endif
