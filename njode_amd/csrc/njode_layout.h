// njode_layout.h -- the workspace of a call of the compiled shapes: which buffers it holds and
// where (Layout, make_layout), and the call itself as njode_api.hip prepares it and
// njode_planner.hip plans it (Call).  Host code only.
#pragma once
#include "njode_hostlib.h"
#include "njode_plan.h"
#include "njode_planner.h"
#include "njode_route.h"

namespace njode {

constexpr int SUM_BLOCKS = 64;  // k_sum_stage1 blocks
constexpr int RED_SPLIT = 32;   // k_reduce_slabs_stage1 wave subsets

constexpr int PLAN_CS_SMALL_BLOCKS = 32;   // row blocks of the one-launch plan's count table below 16 384 rows
struct Layout : Arena {
  size_t len_hist = 0, dense = 0;
  size_t sched, PT, frag, trash, t_of_row, iota, path_sorted, row_by_path, first3, item4, sort_key,
      key_sorted, order, tail4, base_s, h0row, h0start, h_end, lam_end, g_h0, lam_start, loss_terms,
      traj, slab, red_partial, sum_partial, sort_tmp, lk_lam, lk_src, lk_rows, lk_hstart, base16, act, dbits, dbits_row, lk_act, lk_jact, lk_delta, lk_seg, item_pack, tile_last, vflag, cs_small, plan_end;
  size_t sort_tmp_bytes = 0;
};

// (z: the sizing part of the call's route, njode_route.h -- every "is this buffer needed" is decided there)
inline Layout make_layout(const CfgOps* o, const Sizing& z, int B, int n_obs, int n_times, int K) {
  Layout L{};   // (every offset 0: not taken)
  const int H = o->dims.hidden_size, D = o->dims.input_size, DO = o->dims.output_size;
  const size_t nr = (size_t)(n_obs > 0 ? n_obs : 1), nb = (size_t)(B > 0 ? B : 1);
  const size_t steps = (size_t)(K > 0 ? K : 1);
  const int mx = H > D ? (H > DO ? H : DO) : (D > DO ? D : DO);
  // ---- the PLAN PREFIX: everything upload_schedule and build_plan write and nothing else, so
  // that a plan can also be built ahead of its forward into a buffer of its own
  // (njode_plan_f32: the same offsets, relative to that buffer)
  L.sched = L.take(((size_t)2 * K + 3 * (size_t)n_times + 1) * 4 + 64);
  L.t_of_row = L.take(nr * 4);
  L.iota = L.take(nr * 4);
  L.path_sorted = L.take(nr * 4);
  L.row_by_path = L.take(nr * 4);
  L.first3 = L.take(nb * 4 * 3);
  L.item4 = L.take(nr * 4 * 4);
  L.sort_key = L.take(nr * 4);
  L.key_sorted = L.take(nr * 4);
  L.order = L.take(nr * 4);
  L.tail4 = L.take(nb * 4 * 4);  // tail sort: key, key_sorted, iota, t_order
  L.base_s = L.take(((size_t)K + 4) * 8);   // + split points of the mixed ODE kernels
  L.base16 = L.take(((size_t)K + 2) * 8);
  L.len_hist = L.take(((size_t)K + 2) * 4);
  // segment plan: dense [time slice][path] -> row matrix that links the rows of a path
  // without sorting them
  L.dense = L.take((z.dense_cells ? z.dense_cells : 1) * 4);
  L.sort_tmp_bytes = plan_sort_temp_bytes(n_obs, B, K);
  L.sort_tmp = L.take(L.sort_tmp_bytes);
  L.vflag = L.take(256);
  L.cs_small = L.take((size_t)PLAN_KEYS * PLAN_CS_SMALL_BLOCKS * 4);   // count table of the one-launch plan (n_obs < 16 384)
  L.plan_end = L.total;
  // ---- per-call scratch
  L.PT = L.take((size_t)o->P * 4);
  L.frag = L.take((size_t)(o->frag_floats > 0 ? o->frag_floats : 1) * 4);
  // (also the target of the step-record stores a wave of the four-wave ODE role does not own:
  // one whole record block, StepRec::FLOATS <= 2304 floats)
  L.trash = L.take((size_t)(256 * mx > 4096 ? 256 * mx : 4096) * 4);
  // dropout keep bits of the ODE forward's FOUR-WAVE role, one dword per lane and tile-step,
  // written ahead of the kernel by spare blocks of the fragment-pack launch (njode_mfma_split.h)
  if (z.seg_bits) L.dbits = L.take(((size_t)B * K / 16 + (size_t)K + 2) * 256);
  L.h0row = L.take(nr * H * 4);
  L.h0start = L.take(nb * H * 4);
  L.h_end = L.take(nr * H * 4);
  L.lam_end = L.take(nr * H * 4);
  L.g_h0 = L.take(nr * H * 4);
  L.lam_start = L.take(nr * H * 4);
  L.loss_terms = L.take((nr > nb ? nr : nb) * 4);
  L.sum_partial = L.take(SUM_BLOCKS * 4);
  if (z.chain && z.lock_bits) {
    // keep masks of the wave-per-path forward, drawn ahead (k_chain_bits): two 64-bit words per
    // (Euler step, path), per (row, evaluation) and per start encoder
    L.dbits = L.take(((size_t)B * steps + 1) * 16);
    L.dbits_row = L.take((nr * 3 + nb) * 16);
  }
  if (!z.save) return L;
  // segment plan: checkpoints [sum len <= B K][H]; lockstep plan: states [K+1][B][H]
  L.traj = L.take(((size_t)B * (K + 1) + 1) * H * 4);
  L.lk_lam = L.take(((size_t)B * K + 1) * H * 4);
  L.lk_src = L.take(((size_t)B * K + 1) * 4);
  L.lk_rows = L.take(nr * (size_t)(4 * DO + H) * 4);   // y, y_bj, g_y, g_ybj, g_hnew
  L.lk_hstart = L.take(nb * H * 4);
  L.slab = L.take((size_t)z.slab_rows * o->P * 4);
  L.red_partial = L.take((size_t)RED_SPLIT * o->P * 4);
  // segment plan on the matrix cores: the hidden activations of every Euler step are stored
  // by the forward and read by the backward instead of being recomputed (HBM is idle while
  // the f32 pipe is the bound): [sum_s ceil16(cnt_s) <= B K + 16 (K + 1)] chain records
  // (the wave-per-item kernels keep 2 x 64 floats per chain-step: njode_chain_seg.h)
  const size_t act_fl = z.seg_items && CHAIN_ACT_FLOATS > o->act_floats ? CHAIN_ACT_FLOATS : o->act_floats;
  if (z.seg_act) L.act = L.take(((size_t)B * K + 16 * ((size_t)K + 1)) * act_fl * 4);
  // ... and what the ODE backward needs of every item, packed by the saving forward per position of the
  // item order (Item::store_pack: its tile prologue is one load deep), + per tile the record base of
  // its last Euler step
  if (z.pack) {
    const size_t packf = 4 + 4 * (size_t)((1 + D + 3) / 4);
    L.item_pack = L.take((size_t)cdiv((int)nr, 16) * 16 * packf * 4);
    L.tile_last = L.take((size_t)cdiv((int)nr, 16) * 8);
  }
  // masked models (lockstep plan): the same for their Euler steps
  if (z.chain) {
    // (njode_chain.h's own records: [Euler step][path][layer][64 lanes], [row][evaluation][layer][64])
    L.lk_act = L.take((size_t)B * steps * CHAIN_ACT_FLOATS * 4);
    L.lk_jact = L.take(nr * (size_t)CHAIN_JACT_FLOATS * 4);
  } else if (z.lock_act) {
    // (four waves per tile of q4_pt paths)
    static_assert(Q4_JACT_FLOATS == 3 * 2 * 4 * 4, "jump-activation record: 3 evaluations x 2 layers x 4 registers x 4 lane groups");
    L.lk_act = L.take((size_t)cdiv(B, z.q4_pt) * steps * o->lock_act_floats * 4);
    L.lk_jact = L.take(nr * 4 * (size_t)Q4_JACT_FLOATS * 4);   // per row: 4 waves x Q4_JACT_FLOATS floats
    // ... and the keep bits of their forward, drawn ahead of the kernel (k_q4_bits)
    if (z.lock_bits) {
      L.dbits = L.take((size_t)cdiv(B, z.q4_pt) * steps * 256);
      L.dbits_row = L.take(nr * 3 * 4 * 4);
    }
  }
  // the wave-per-chain sweeps' delta1 | delta2 of every (step, path) pair for the pair dW kernel
  if (z.delta) L.lk_delta = L.take((size_t)B * steps * CHAIN_ACT_FLOATS * 4);
  // ... and their per-segment sums of delta1 (the x / tau / time columns of dW1: njode_chain_dw.h)
  if (z.delta_seg) L.lk_seg = L.take((nr + nb) * (size_t)CHAIN_ACT_FLOATS * 4);
  return L;
}

struct Call {
  const CfgOps* o;
  Route route;     // what this call runs (njode_route.h); route.size: what its workspace is laid out for
  Layout L;
  KArgs a;
  SideInfo side;
  char* pw;        // base of the plan prefix: the workspace, or the caller's prebuilt plan
  bool planned;    // NJODE_C_PLAN_READY: schedule copy and plan already sit at pw
  bool plan_only;  // njode_plan_f32: only the plan prefix exists behind `ws`
};

}  // namespace njode
