// njode_env.h -- the switches: every NJODE_* variable the library's C++ acts on, parsed once per
// process by parse_env(), which states each one's values, default and effect (DESIGN.md section 4g
// mirrors it).  No other file under csrc reads the environment.  Host code only.
#pragma once
#include <cstdlib>
#include <cstring>

namespace njode {

// ODE-evolve implementations: matrix cores (default where compiled), VALU with weights
// through the scalar cache
constexpr int ODE_MFMA = 0, ODE_VALU = 1;
// (NJODE_ODE=mfma1 keeps ODE_MFMA but with one wave per tile, njode_mfma.h, where the default
// picks the mixed kernels of njode_mfma_split.h: A/B baseline)

struct Env {
  bool lock4, drop_bits_ahead, generic, ode_one_wave, sort_merge, sort_rocprim, item_pack, chain_delta, lock_sweep_valu,
      dw_enc_fused, tail_sort_rocprim, validate, plan_sort, plan_grid, plan_stamps, plan_stream, plan_grid_tail;
  int lock4_pt, chain_max, seg_chain_max, ode, split_bwd_blocks, split_fwd_blocks, bwd_blocks, fwd_blocks,
      plan_blocks, cs_shift, plan_inline_max, plan_inline_blocks, enc_blocks, chain_wpb,
      gen_nw, gen_pt, gen_dbg;
  float split_r_bwd, split_r_fwd;
  double rec_budget_gb;
};

inline Env parse_env() {
  const auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
  const auto real = [](const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; };
  const auto on = [](const char* name) { const char* e = getenv(name); return e && atoi(e) != 0; };         // default off
  const auto not_off = [](const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); };  // default on
  const auto is = [](const char* e, const char* v) { return e && strcmp(e, v) == 0; };
  const char *ode = getenv("NJODE_ODE"), *sort = getenv("NJODE_SORT"), *lock4 = getenv("NJODE_LOCK4");
  Env e;
  e.lock4 = !(lock4 && lock4[0] == '0');                // =0: masked shapes keep the one-wave lockstep kernels (A/B)
  e.drop_bits_ahead = not_off("NJODE_DROP_BITS_AHEAD"); // =0: the four-wave forwards draw their keep bits themselves (A/B)
  e.enc_blocks = num("NJODE_ENC_BLOCKS", 4096);         // grid cap of k_encode_rows_mfma (A/B)
  e.chain_wpb = num("NJODE_CHAIN_WPB", 0);              // =1..8: waves (= paths) per block of the wave-per-path kernels (else: by batch size)
  e.generic = on("NJODE_GENERIC");                      // =1: every model runs the shape-generic kernels (njode_gen.h; A/B, parity tests)
  e.rec_budget_gb = real("NJODE_REC_BUDGET_GB", 16.0);  // bound of the training records, see record_budget_bytes()
  e.lock4_pt = num("NJODE_LOCK4_PT", 0);                // =1|2|4|8|16: paths per tile of the masked lockstep kernels (else: by batch size)
  e.chain_max = num("NJODE_CHAIN_MAX", 1 << 30);        // paths up to which the wave-per-path lockstep kernels run; 0: off (A/B)
  e.seg_chain_max = num("NJODE_SEG_CHAIN_MAX", 16384);  // waves up to which the wave-per-item segment kernels run; 0: off (A/B)
  // implementation of the ODE-evolve kernels: valu; mfma1 and anything else: the matrix cores, with
  // mfma1 one wave per tile (njode_mfma.h) instead of the mixed kernels (A/B baseline)
  e.ode = is(ode, "valu") ? ODE_VALU : ODE_MFMA;
  e.ode_one_wave = is(ode, "mfma1");
  // =merge: rocPRIM's default dispatch instead of Onesweep (whose decoupled look-back spins between
  // workgroups and did not terminate under rocprofv3's FETCH_SIZE / WRITE_SIZE collection)
  e.sort_merge = is(sort, "merge");
  e.sort_rocprim = is(sort, "rocprim");                 // no counting sort of the rows by segment length
  e.item_pack = not_off("NJODE_ITEM_PACK");             // =0: the ODE backward walks the plan's arrays (A/B)
  e.chain_delta = not_off("NJODE_CHAIN_DELTA");         // =0: the pair dW kernel recomputes delta1 | delta2 (A/B)
  // speed of a four-wave block relative to one wave, per tile-step (backward, forward), with the chip full of
  // both kinds (profiles/r01_mixed_sweep.txt; a lone block is ~2.3x / ~2.1x faster) (backward, round 5,
  // per-role stamps: 4.4 - 4.9 us per Euler step of a bulk wave against 2.3 - 2.5 us of a four-wave block = 1.9
  // - 2.0; the static rounds do best with the slightly larger 2.25 found by the sweep of round 4 -- more tiles
  // in the four-wave role shorten the tail of the bulk's second round)
  e.split_r_bwd = (float)real("NJODE_SPLIT_R_BWD", 2.25);
  e.split_r_fwd = (float)real("NJODE_SPLIT_R_FWD", 2.0);
  e.lock_sweep_valu = is(getenv("NJODE_LOCK_SWEEP"), "valu");   // the VALU adjoint sweep of the lockstep plan (A/B)
  // mixed ODE kernels: 1024 blocks backward (one slab row each; two rounds of the 512 resident ones -- with the
  // stored activations 1024 beats 1536 by 2.4 %, profiles/r02_mixed_sweep.jsonl), 3072 forward -- more than fit
  // at once: the dispatcher then hands out the length-sorted tiles as blocks retire, longest first (round 4: 32
  // four-wave blocks backward -- with two barriers per step the role needs fewer blocks for the same tail; 64
  // -> 32: k_ode_bwd_mixed 0.436 -> 0.427 ms)
  e.split_bwd_blocks = num("NJODE_SPLIT_BWD_BLOCKS", 32);
  e.split_fwd_blocks = num("NJODE_SPLIT_FWD_BLOCKS", 96);
  e.bwd_blocks = num("NJODE_BWD_BLOCKS", 0);            // all blocks of the backward (0: 1024)
  e.fwd_blocks = num("NJODE_FWD_BLOCKS", 3072);
  e.dw_enc_fused = not_off("NJODE_DW_ENC_FUSED");       // =0: the encoder's weight-gradient pass as a launch of its own (A/B)
  e.tail_sort_rocprim = is(getenv("NJODE_TAIL_SORT"), "rocprim");   // k_tail_keys + radix sort instead of k_tail_order
  e.plan_blocks = num("NJODE_PLAN_BLOCKS", 0);          // blocks of the one-launch plan (0: by row count)
  e.validate = on("NJODE_VALIDATE");                    // =1: check the batch layout's preconditions on the device (synchronises)
  e.plan_sort = is(getenv("NJODE_PLAN"), "sort");       // link the rows by a (path, time) sort, no dense matrix
  e.plan_grid = not_off("NJODE_PLAN_GRID");             // =0: never the one-launch plan
  e.cs_shift = num("NJODE_CS_SHIFT", 8);                // log2 of the counting sort's smallest row block (A/B: 256-row blocks)
  e.plan_stamps = on("NJODE_PLAN_STAMPS");              // =1: stage stamps of the one-launch plan (njode_debug_plan_stamps)
  e.plan_inline_max = num("NJODE_PLAN_INLINE_MAX", 16384);   // rows up to which an in-line plan is ONE launch
  e.plan_stream = not_off("NJODE_PLAN_STREAM");         // =0: everything on the caller's stream, no helper streams
  e.plan_grid_tail = not_off("NJODE_PLAN_GRID_TAIL");   // =0: large in-line plans keep their five launches
  e.plan_inline_blocks = num("NJODE_PLAN_INLINE_BLOCKS", 128);   // blocks of a large in-line plan's one launch
  // the shape-generic family (njode_gen.hip)
  e.gen_nw = num("NJODE_GEN_NW", -1);                   // =1..16: waves per workgroup of its forward / sweep kernels (-1, unset: by layer width and grid; A/B)
  e.gen_pt = num("NJODE_GEN_PT", 0);                    // =1|2|4|8|16: paths per tile of its lockstep plan (else: by batch size; A/B)
  e.gen_dbg = num("NJODE_GEN_DBG", 0);                  // ablation mask of a -DNJ_GEN_ABL diagnostic build (ignored otherwise)
  return e;
}
inline const Env& env() {
  static const Env e = parse_env();
  return e;
}

}  // namespace njode
