// njode_route.h -- which kernel family a call of the compiled shapes runs on, decided ONCE from the NJODE_*
// switches (Env, njode_env.h): what the workspace is sized for (Sizing) and what is launched (Route).  Host
// only; included by njode_api.hip and njode_planner.hip, which size (make_layout, njode_layout.h), plan
// (build_plan) and call the launchers (njode_forward_f32 / backward_impl) from these fields, and by
// njode_cfg.hip, whose launchers switch on the Route they are handed; none derives anything of its own.
#pragma once
#include <algorithm>

#include "njode_env.h"
#include "njode_host.h"
#include "njode_hostlib.h"

namespace njode {

constexpr int SLAB_ROWS_MAX = 3072;   // >= every backward's worker count (<= 2048 by default)
constexpr size_t DENSE_CELLS_MAX = (size_t)64 << 20;   // 256 MB of row indices

// ---- the SIZING part: what njode_workspace_bytes / njode_plan_bytes can know -- shape, sizes,
// call flags, switches; no schedule contents, no pointers.  make_layout() takes buffers by these
// fields and holds no predicate of its own.
struct Sizing {
  bool train, save;       // NJODE_C_TRAIN, NJODE_C_SAVE_BWD
  // the call MAY run the segment plan: unmasked, no GRU, loss requested, no path output ...
  bool seg_any;           // ... whatever its schedule turns out to be (dense matrix, keep bits drawn ahead)
  bool seg_untailed;      // ... and its flags do not already say that the schedule has a tail (stored activations)
  // the wave-per-item segment kernels (njode_chain_seg.h) MAY run: up to NJODE_SEG_CHAIN_MAX waves (0 switches
  // the kernels off, A/B).  Default 16 384 = B = 1 400 of the demo data: ms per step against the 16-chain tiles
  // at B = 400 / 700 / 1 000 / 1 500 / 2 000: 0.176 / 0.201 / 0.231 / 0.290 / 0.364 against 0.271 / 0.290 /
  // 0.262 / 0.295 / 0.325 (round 6); beyond that the tiles' throughput wins. Besides the wave
  // count: K <= SPLIT_KMAX and NJODE_ODE = mfma (the split kernels they belong to), and for saving calls the
  // records (512 B per (path, step)) within the record budget.
  bool seg_items;
  // the wave-per-path lockstep kernels (njode_chain.h: a lane is a unit of the layer) run.  Built for
  // the latency regime (B = 50 .. 1 000: every path a SIMD of its own), they also win on throughput:
  // eight waves per CU take 1 350 cycles per Euler step each, a tile of 16 paths over four waves 4 300
  // (B = 4 096: 21.4 against 37.8 ms per step, B = 8 192: 41.9 against 73.5; round 6) -- so they
  // run whenever their training records (512 B per path and Euler step) fit the record budget.
  // (prediction calls -- return_path -- too, unless they draw dropout masks: a train-mode call)
  bool chain;
  // Masked lockstep kernels (njode_mfma_lock4.h: one tile of 16 lanes over the four waves of a block): paths
  // per tile.  A tile runs the three network evaluations of a jump for ALL its lanes whenever ANY of its paths
  // has an observation at that time, so a tile of 16 PhysioNet-shaped paths (~65 observation times each) goes
  // through ~740 jump events, a tile of one path through 65 -- and with B = 50 (physionet_train.py) sixteen
  // paths per tile use 4 of the chip's 256 CUs. Fewer paths per tile (the other lanes idle: the matrix
  // instruction's width is 16 either way) trade arithmetic that nobody was waiting for against the serial
  // chain: the smallest power of two that still gives every tile a CU of its own, and more where the tiles'
  // training records (lock_act_floats per tile-step + one keep-bit dword per lane) would exceed the record
  // budget.
  int q4_pt;
  size_t dense_cells;     // cells of the dense [time slice][path] -> row matrix (0: the rows are sorted)
  bool seg_bits;          // keep bits of the segment plan's ODE forward are drawn ahead of it
  bool seg_act;           // the segment plan's forward stores its hidden activations (KArgs::act)
  bool pack;              // ... and the items packed for the backward (KArgs::item_pack, tile_last)
  bool lock_act;          // the lockstep forward stores its activations (KArgs::lact, jact)
  bool lock_bits;         // ... and has buffers for keep bits drawn ahead of it (KArgs::dbits, dbits_row)
  bool delta, delta_seg;  // the wave-per-chain sweeps store delta1 | delta2 (KArgs::cdelta), and their segment sums (cseg)
  int n_waves;            // one wave per tile of 16 rows until the chip is full (+ the split blocks' slab rows)
  int n_waves_lock;       // waves (= slab rows) of the lockstep plan's matrix-core dW kernels
  int slab_rows;          // one per gradient worker of whichever backward runs
};

inline Sizing size_call(const CfgOps& o, int B, int n_obs, int n_times, int K, int call_flags,
                        double rec_budget, const Env& e) {
  Sizing z;
  const bool want_path = (call_flags & NJODE_C_RETURN_PATH) != 0;
  const int steps = K > 0 ? K : 1;
  z.train = (call_flags & NJODE_C_TRAIN) != 0;
  z.save = (call_flags & NJODE_C_SAVE_BWD) != 0;
  z.seg_any = !(o.dims.flags & (NJODE_F_MASKED | NJODE_F_USE_RNN)) && (call_flags & NJODE_C_GET_LOSS) && !want_path;
  z.seg_untailed = z.seg_any && !((call_flags & NJODE_C_SCHED_KNOWN) && (call_flags & NJODE_C_SCHED_TAIL));
  const bool chain_rec_fit = !z.save || (double)B * steps * (CHAIN_ACT_FLOATS * 4.0 + 16.0) <= rec_budget;
  z.seg_items = o.seg_chain && e.ode == ODE_MFMA && !e.ode_one_wave && n_obs > 0 &&
                n_obs + B <= e.seg_chain_max && K <= SPLIT_KMAX && chain_rec_fit;
  z.chain = o.lock_chain && B <= e.chain_max && !(want_path && z.train) && chain_rec_fit;
  if (e.lock4_pt == 1 || e.lock4_pt == 2 || e.lock4_pt == 4 || e.lock4_pt == 8 || e.lock4_pt == 16) {
    z.q4_pt = e.lock4_pt;
  } else {
    z.q4_pt = 1;
    while (z.q4_pt < 16 && cdiv(B, z.q4_pt) > 256) z.q4_pt *= 2;
    if (o.lock_act_floats > 0 && z.save && !want_path) {
      const double per_tile = (double)steps * ((double)o.lock_act_floats * 4.0 + 256.0);
      while (z.q4_pt < 16 && (double)cdiv(B, z.q4_pt) * per_tile > rec_budget) z.q4_pt *= 2;
    }
  }
  // (only when the plan can be the segment plan, and not for huge grids)
  const size_t cells = (size_t)(n_times > 0 ? n_times : 1) * (size_t)(B > 0 ? B : 1);
  z.dense_cells = (z.seg_any && n_obs > 0 && cells <= DENSE_CELLS_MAX) ? cells : 0;
  // (only plans whose every tile runs four waves wide read the bits: cdiv(n_obs, 16) <= 768, the
  // condition under which the forward is all-split; larger plans draw in the kernel)
  // (... and the wave-per-item forward its lane masks, 16 bytes per (path, step): njode_chain_seg.h)
  z.seg_bits = o.act_floats > 0 && z.seg_any && n_obs > 0 && z.train && (cdiv(n_obs, 16) <= 768 || z.seg_items);
  z.seg_act = z.save && o.act_floats > 0 && z.seg_untailed && n_obs > 0;
  z.pack = z.seg_act && e.item_pack;
  z.lock_act = z.save && (z.chain || (o.lock_act_floats > 0 && !want_path));
  z.lock_bits = z.train && (z.chain || z.lock_act);
  // ... where they fit the record budget beside the activations (else the pair dW kernel recomputes them)
  z.delta = z.save && e.chain_delta && (z.chain || (z.seg_act && z.seg_items)) &&
            (double)B * steps * (2.0 * CHAIN_ACT_FLOATS * 4.0 + 16.0) <= rec_budget;
  z.delta_seg = z.delta && o.dims.width < 64;
  const int row_tiles = cdiv(n_obs + B, 16) + 128;
  z.n_waves = std::max(4, (std::min(row_tiles, MAX_WAVES) + 3) & ~3);   // (whole 256-thread blocks)
  // weight-gradient kernels of the lockstep backward: ~8 tiles of 16 (step, path) pairs per wave
  const long long w = ((long long)B * K / 16 + 7) / 8;
  z.n_waves_lock = ((int)std::min<long long>(1024, std::max<long long>(w, z.n_waves)) + 3) & ~3;
  // (576: k_ode_dw_stored runs up to 512 + 64 blocks, a row each)
  z.slab_rows = std::max({std::min(row_tiles, SLAB_ROWS_MAX), z.n_waves, z.n_waves_lock, 576});
  return z;
}

// ---- the DISPATCH part: what a real call runs, from the sizing part plus the three things only a call knows
// -- whether its schedule has a tail, whether it draws dropout masks, whether hT is wanted.  prepare() copies
// these fields into KArgs; build_plan, the forward and the backward read them. The sizing part may
// OVER-provision relative to dispatch (it admits seg_items for a call whose schedule then has a tail, or whose
// NJODE_ODE leaves the split kernels, and sizes `act` for the wave-per-item records all the same); it must
// never under-provision: prepare() checks route_admitted() before anything is launched.
// Kernel family of the lockstep plan's forward / adjoint sweep: VALU, one wave per tile of 16 or 32 paths
// (njode_mfma_lockstep.h), one tile over the four waves of a block (njode_mfma_lock4.h; NJODE_LOCK4=0
// keeps the one-wave kernels), one wave per path (njode_chain.h)
enum LockKind { LOCK_VALU, LOCK_WAVE1, LOCK_TILE4, LOCK_CHAIN };
struct Route {
  Sizing size;
  bool drop;            // dropout masks are drawn
  bool want_path, want_loss;   // NJODE_C_RETURN_PATH, NJODE_C_GET_LOSS (the lockstep forward's outputs)
  bool seg;             // segment plan (else lockstep): unmasked, loss requested, no path output, schedule ends at its last jump
  bool tails;           // ... which also evolves every path from its last observation to the end (hT)
  int ode;              // implementation of the ODE-evolve kernels (ODE_*)
  bool seg_mfma;        // the segment plan runs on the matrix cores
  // Implementations of the lockstep plan's adjoint sweep and of its forward.  The backward
  // regenerates the dropout masks, so a forward that saves for it must key them as the sweep
  // does: the matrix-core keying where the shape has a matrix-core sweep, the VALU keying otherwise.
  int lock_sweep, lock_fwd;
  // ... and the kernel family of each.  The sweep reads the records of the family that saved them (lact /
  // jact of the four-wave tiles or of the wave-per-path kernels): both kinds come from lock_kind() on the
  // call's sizing and flags, so the two calls of a step agree.
  int lock_fwd_kind, lock_bwd_kind;
  bool lock_bits_ahead; // the four-wave tiles' forward reads keep bits drawn ahead of it (k_q4_bits)
  int chain_wpb;        // waves (= paths) per block of the wave-per-path kernels
  bool lock_mfma;       // the lockstep backward runs on the matrix cores
  int seg_ode;          // ODE-evolve implementation of the segment plan: `ode` where the shape has it
  int ode_split;        // the mixed ODE kernels (njode_mfma_split.h)
  int seg_chain;        // the wave-per-item ODE kernels (njode_chain_seg.h)
  int enc_blocks;       // grid cap of k_encode_rows_mfma
  bool tails_ride;      // the tails ride in the items' launch (k_seg_fwd_chain), else in one of their own
  // keep bits of the segment plan's ODE forward are drawn ahead, by spare blocks of the fragment-pack launch
  bool seg_bits_ahead;
  bool side, tails_side;   // the call has helper streams (route_side), and the tails run on the second one
  int defer_loss;       // 1: the loss is summed by the backward call (fused step), 2: rows in the forward call
  int dw_enc_fused;     // the encoder's weight-gradient pass rides in k_ode_dw_stored's launch
  int n_split_blocks, n_blocks_bwd, n_split_fwd, n_blocks_fwd;   // four-wave / all blocks of the mixed kernels
  int dw_pair_blocks, dw_seg_blocks;   // k_ode_dw_stored's roles
  bool chain_dw;        // the wave-per-chain sweeps' own weight-gradient kernel runs (njode_chain_dw.h)
  bool dw_stored;       // ... as k_ode_dw_stored, a launch of its own (no (step, path) pairs at K = 0: the pair kernel)
  bool hosts_plan;      // this forward's ODE launch can carry a deferred plan in front of its blocks
  bool needs_PT;        // the backward reads the transposed parameter copy (VALU kernels only)
};

// (z.chain already excludes prediction calls that draw dropout masks; the four-wave tiles neither
// return paths nor save without their records)
inline int lock_kind(const CfgOps& o, const Sizing& z, const Env& e, bool mfma, bool want_path) {
  if (!mfma) return LOCK_VALU;
  if (z.chain) return LOCK_CHAIN;
  if (o.lock_act_floats > 0 && !want_path && e.lock4 && (!z.save || z.lock_act)) return LOCK_TILE4;
  return LOCK_WAVE1;
}

inline Route route_call(const CfgOps& o, const Sizing& z, int B, int n_obs, int K, int call_flags,
                        const Env& e, bool tail, bool drop, bool want_hT) {
  Route r;
  r.size = z;
  r.drop = drop;
  r.want_path = (call_flags & NJODE_C_RETURN_PATH) != 0;
  r.want_loss = (call_flags & NJODE_C_GET_LOSS) != 0;
  r.seg = z.seg_any && n_obs > 0 && !tail && !(call_flags & NJODE_C_GEN_LOCKSTEP);
  r.tails = r.seg && want_hT;
  r.ode = e.ode;
  r.seg_mfma = r.seg && r.ode == ODE_MFMA && o.seg_mfma;
  // (masked shapes have no VALU backward -- register pressure: always the matrix cores)
  r.lock_sweep = !o.lock_sweep_mfma ? ODE_VALU
                 : (o.dims.flags & NJODE_F_MASKED) ? ODE_MFMA
                 : (r.ode == ODE_MFMA && !e.lock_sweep_valu) ? ODE_MFMA : ODE_VALU;
  // the keying must not depend on whether this call saves for a backward: a loss-only
  // forward in train mode has to see the masks of the training forward
  // ... and a forward that saves for a sweep which reads its stored activations (masked shapes,
  // njode_mfma_lock4.h) has to be the implementation that stores them
  r.lock_fwd = (z.lock_act || drop) ? r.lock_sweep : r.ode;
  r.lock_fwd_kind = lock_kind(o, z, e, r.lock_fwd == ODE_MFMA && o.lock_fwd_mfma, r.want_path);
  r.lock_bwd_kind = lock_kind(o, z, e, r.lock_sweep == ODE_MFMA, r.want_path);
  r.lock_bits_ahead = r.lock_fwd_kind == LOCK_TILE4 && drop && z.lock_bits && e.drop_bits_ahead;
  // as few waves per block as still give every path a SIMD of its own
  r.chain_wpb = 1;
  if (e.chain_wpb >= 1 && e.chain_wpb <= CHAIN_MAX_WAVES) r.chain_wpb = e.chain_wpb;
  else while (r.chain_wpb < CHAIN_MAX_WAVES && cdiv(B, r.chain_wpb) > 256) r.chain_wpb *= 2;
  r.lock_mfma = !r.seg && r.lock_sweep == ODE_MFMA;
  r.seg_ode = (r.ode == ODE_MFMA && !o.seg_mfma) ? ODE_VALU : r.ode;
  r.ode_split = (r.ode == ODE_MFMA && o.ode_split && !e.ode_one_wave && K <= SPLIT_KMAX) ? 1 : 0;
  // fused step: the matrix-core row kernel of the backward evaluates every readout anyway
  // ... or in the forward call, which then skips its forward-only row pass (NJODE_C_ROWS_IN_FWD)
  r.defer_loss = !(z.save && r.seg_mfma) ? 0
                 : (call_flags & NJODE_C_LOSS_IN_BWD) ? 1 : (call_flags & NJODE_C_ROWS_IN_FWD) ? 2 : 0;
  // mixed ODE kernels: a plan with fewer tiles than resident blocks runs every tile four waves per tile
  const int n_tiles = cdiv(n_obs > 0 ? n_obs : 1, 16);
  if (n_tiles <= 384) {
    r.n_split_blocks = r.n_blocks_bwd = n_tiles;
  } else {
    const int tot_b = e.bwd_blocks > 0 ? e.bwd_blocks : 1024;
    r.n_split_blocks = e.split_bwd_blocks;
    int nsb = tot_b - e.split_bwd_blocks;
    if (nsb > cdiv(n_tiles, 4)) nsb = cdiv(n_tiles, 4);
    if (r.n_split_blocks + nsb > z.slab_rows) nsb = z.slab_rows - r.n_split_blocks;
    r.n_blocks_bwd = r.n_split_blocks + nsb;
  }
  if (n_tiles <= 768) {
    r.n_split_fwd = r.n_blocks_fwd = n_tiles;
  } else {
    r.n_split_fwd = e.split_fwd_blocks;
    int nsb = e.fwd_blocks - e.split_fwd_blocks;
    if (nsb > cdiv(n_tiles, 4)) nsb = cdiv(n_tiles, 4);
    r.n_blocks_fwd = r.n_split_fwd + nsb;
  }
  r.seg_chain = (r.seg_mfma && r.ode_split && z.seg_items) ? 1 : 0;
  r.enc_blocks = e.enc_blocks;
  r.tails_ride = r.tails && r.seg_chain;
  // (plans whose every tile runs four waves wide, i.e. small batches: there the forward IS the chain of its
  // longest tile; in the mixed kernel of a large plan the four-wave blocks are ~10 % of the work and the
  // extra blocks of the pack launch cost more than they save: 20 000 paths, k_pack_all 7.5 -> 12.3 us for
  // ~1.5 us off k_ode_fwd_mixed) ... and the wave-per-item forward's lane masks
  r.seg_bits_ahead = r.seg_mfma && drop && z.seg_bits &&
                     (r.seg_chain || (r.ode_split && e.drop_bits_ahead && r.n_split_fwd == r.n_blocks_fwd));
  r.side = r.tails_side = false;
  {
    // k_ode_dw_stored: a wave per tile of 16 (step, path) pairs until every SIMD has one (one block per
    // CU: a wave holds all accumulator tiles and the next tile's operands), a few blocks for the segments
    // (hidden_size <= 16: the kernel is built for two blocks per CU, ChainDw::BLOCKS_PER_CU)
    const long long tiles = ((long long)B * (K > 0 ? K : 0) + 15) / 16, seg_tiles = ((long long)n_obs + B + 15) / 16;
    r.dw_pair_blocks = (int)std::min<long long>((tiles + 3) / 4, o.dims.hidden_size <= 16 ? 512 : 256);
    r.dw_seg_blocks = (int)std::min<long long>(std::max<long long>((seg_tiles + 3) / 4, 1), 64);
  }
  r.chain_dw = (z.chain || r.seg_chain) && z.delta && z.delta_seg;
  r.dw_stored = r.chain_dw && r.dw_pair_blocks > 0;
  r.dw_enc_fused = (e.dw_enc_fused && r.seg_chain && r.dw_stored) ? 1 : 0;
  r.hosts_plan = r.seg_mfma && r.ode_split;
  r.needs_PT = !(r.lock_mfma || r.seg_mfma);
  return r;
}

// The one input known only after the plan is built: whether the call has helper streams (build_plan).
// The tile kernels' keep bits need the complete plan on the pack launch's stream -- the wave-per-item
// forward's lane masks need nothing of it -- and the tails, unless they ride, take the second stream.
inline void route_side(Route& r, bool side) {
  r.side = side;
  r.tails_side = r.tails && side && !r.tails_ride;
  r.seg_bits_ahead = r.seg_bits_ahead && (r.seg_chain || !side);
}

// A kernel must never run on records sized for another: what the dispatch part chose against what the
// sizing part provided.
inline bool route_admitted(const Route& r) {
  const Sizing& z = r.size;
  const bool chain = r.lock_fwd_kind == LOCK_CHAIN || r.lock_bwd_kind == LOCK_CHAIN;
  const bool tile4 = r.lock_fwd_kind == LOCK_TILE4 || r.lock_bwd_kind == LOCK_TILE4;
  return !(r.seg_chain && !z.seg_items) && !(chain && !z.chain) && !(tile4 && z.save && !z.lock_act) &&
         !(r.seg_bits_ahead && !z.seg_bits) && !(r.lock_bits_ahead && !z.lock_bits) &&
         !(r.lock_fwd_kind == LOCK_CHAIN && r.drop && !z.lock_bits);
}

// Slab rows the backward's kernels wrote, per parameter slice (ODE / encoder / readout): what the
// gradient's reduction sums.
struct SlabRows { int ode, enc, dec; };
inline SlabRows slab_rows_written(const Route& r) {
  const Sizing& z = r.size;
  const int rows = r.seg_mfma ? z.n_waves / 4 : z.n_waves;   // (matrix-core kernels of the segment plan: a row per 256-thread block)
  SlabRows s{!r.seg || r.seg_chain ? z.n_waves : r.ode_split ? r.n_blocks_bwd : rows, rows, rows};
  if (r.lock_mfma) s.ode = s.enc = s.dec = z.n_waves_lock;
  // (the wave-per-chain sweeps' own weight-gradient kernel: one slab row per block)
  if (r.chain_dw) s.ode = r.dw_pair_blocks + r.dw_seg_blocks;
  return s;
}

}  // namespace njode
