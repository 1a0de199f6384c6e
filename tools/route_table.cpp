// route_table.cpp -- what njode_route.h decides, as a table, without a GPU: Sizing and Route of a grid of
// calls for every capability row on stdin.  Host code only:
//   hipcc --cuda-host-only -std=c++17 -O0 tools/route_table.cpp -o route_table
//   printf '10 50 0  1 1 1 1 0 0 1\n' | NJODE_LOCK4=0 ./route_table
// A row is: hidden_size width flags  HAS_MFMA HAS_SPLIT HAS_MFMA_LOCK HAS_MFMA_SWEEP HAS_Q4 HAS_CHAIN
// HAS_SEG_CHAIN (njode_cfg.hip, as njode_cfg_ops_ fills CfgOps from them).  The NJODE_* switches are read
// from the environment once, as in the library.  tests/test_route_table.py compares the output with
// tests/golden/route_table.txt and checks the route's invariants on every line.
#include <cstdio>

#include "../njode_amd/csrc/njode_route.h"

using namespace njode;

#define SIZING_FIELDS(X)                                                                                     \
  X(train) X(save) X(seg_any) X(seg_untailed) X(seg_items) X(chain) X(q4_pt) X(dense_cells) X(seg_bits)      \
  X(seg_act) X(pack) X(lock_act) X(lock_bits) X(delta) X(delta_seg) X(n_waves) X(n_waves_lock) X(slab_rows)
#define ROUTE_FIELDS(X)                                                                                      \
  X(drop) X(want_path) X(want_loss) X(seg) X(tails) X(ode) X(seg_mfma) X(lock_sweep) X(lock_fwd)             \
  X(lock_fwd_kind) X(lock_bwd_kind) X(lock_bits_ahead) X(chain_wpb) X(lock_mfma) X(seg_ode) X(ode_split)     \
  X(seg_chain) X(enc_blocks) X(tails_ride) X(seg_bits_ahead) X(defer_loss) X(dw_enc_fused) X(n_split_blocks) \
  X(n_blocks_bwd) X(n_split_fwd) X(n_blocks_fwd) X(dw_pair_blocks) X(dw_seg_blocks) X(chain_dw) X(dw_stored) \
  X(hosts_plan) X(needs_PT)

struct Size { int B, n_obs, K, n_times, budget; };   // budget: 0 default, 1 the activations fit but not the deltas, 2 nothing fits
struct Inputs { int tail, drop, want_hT; };

static void print_call(int row, const CfgOps& o, const Size& s, int flags, const Inputs& in) {
  const double steps = s.K > 0 ? s.K : 1;
  const double budget = s.budget == 0 ? 16e9 : s.budget == 1 ? s.B * steps * (CHAIN_ACT_FLOATS * 4.0 + 16.0) : 1e3;
  const Sizing z = size_call(o, s.B, s.n_obs, s.n_times, s.K, flags, budget, env());
  const Route r = route_call(o, z, s.B, s.n_obs, s.K, flags, env(), in.tail != 0, in.drop != 0, in.want_hT != 0);
  Route rs = r;
  route_side(rs, true);   // ... had build_plan taken helper streams
  const SlabRows w = slab_rows_written(r);
  printf("%d %d %d %d %d %d %d %d %d %d", row, s.B, s.n_obs, s.K, s.n_times, s.budget, flags, in.tail, in.drop, in.want_hT);
#define X(f) printf(" %lld", (long long)z.f);
  SIZING_FIELDS(X)
#undef X
#define X(f) printf(" %lld", (long long)r.f);
  ROUTE_FIELDS(X)
#undef X
  printf(" %d %d %d %d %d %d\n", (int)rs.seg_bits_ahead, (int)rs.tails_side, w.ode, w.enc, w.dec, (int)route_admitted(r));
}

int main() {
  // both sides of every threshold of size_call / route_call, one axis at a time around a small call
  const int Kmax = SPLIT_KMAX;
  const Size sizes[] = {
      {24, 100, 100, 64, 0},
      {24, 0, 100, 64, 0},                                               // no rows
      {24, 384 * 16, 100, 64, 0},     {24, 384 * 16 + 1, 100, 64, 0},    // cdiv(n_obs, 16): 384 | 385
      {24, 768 * 16, 100, 64, 0},     {24, 768 * 16 + 1, 100, 64, 0},    // 768 | 769
      {24, 16384 - 24, 100, 64, 0},   {24, 16385 - 24, 100, 64, 0},      // n_obs + B: NJODE_SEG_CHAIN_MAX
      {256, 100, 100, 64, 0},         {257, 100, 100, 64, 0},            // cdiv(B, q4_pt) (and B over chain_wpb): 256 | 257
      {4096, 100, 100, 64, 0},        {4097, 100, 100, 64, 0},           // ... at sixteen paths per tile
      {24, 100, 0, 1, 0},             {24, 100, Kmax, 64, 0},            {24, 100, Kmax + 1, 64, 0},
      {1024, 100, 100, 65536, 0},     {1024, 100, 100, 65537, 0},        // DENSE_CELLS_MAX
      {24, 100, 100, 64, 1},          {24, 100, 100, 64, 2},             // record budget
      {300, 2000, 60, 60, 2},                                            // ... which raises the paths per tile
  };
  // the flag sets of the Python wrapper (njode_amd/models.py)
  const int L = NJODE_C_GET_LOSS, T = NJODE_C_TRAIN, S = NJODE_C_SAVE_BWD;
  const int flag_sets[] = {L,                                    // eval loss
                           L | T | S,                            // train + save
                           L | T | S | NJODE_C_LOSS_IN_BWD,      // fused step
                           L | T | S | NJODE_C_ROWS_IN_FWD,
                           NJODE_C_RETURN_PATH,                  // prediction
                           NJODE_C_RETURN_PATH | L | T,
                           L | T | S | NJODE_C_GEN_LOCKSTEP,     // a step that differentiates through hT
                           L | T | S | NJODE_C_SCHED_KNOWN | NJODE_C_SCHED_TAIL};
  const int SAVE = 1;   // (index of the saving set the sizes are walked with, dropout on, hT wanted)
  const Inputs inputs[] = {{0, 1, 1}, {0, 0, 1}, {1, 0, 1}, {1, 1, 0}};

  printf("row B n_obs K n_times budget flags tail drop want_hT");
#define X(f) printf(" z." #f);
  SIZING_FIELDS(X)
#undef X
#define X(f) printf(" " #f);
  ROUTE_FIELDS(X)
#undef X
  printf(" side.seg_bits_ahead side.tails_side rows.ode rows.enc rows.dec admitted\n");

  int row = 0, H, W, flags, mfma, split, mfma_lock, mfma_sweep, q4, chain, seg_chain;
  while (scanf("%d %d %d %d %d %d %d %d %d %d", &H, &W, &flags, &mfma, &split, &mfma_lock, &mfma_sweep, &q4, &chain,
               &seg_chain) == 10) {
    CfgOps o{};
    o.dims.hidden_size = H;
    o.dims.width = W;
    o.dims.flags = flags;
    o.act_floats = split;   // (only "> 0" is read)
    o.lock_act_floats = q4 ? Q4_ACT_FLOATS : 0;
    o.lock_fwd_mfma = mfma_lock, o.lock_sweep_mfma = mfma_sweep, o.lock_chain = chain;
    o.seg_chain = seg_chain, o.ode_split = split, o.seg_mfma = mfma;
    for (const Size& s : sizes) print_call(row, o, s, flag_sets[SAVE], inputs[0]);
    for (int f : flag_sets)
      for (const Inputs& in : inputs)
        if (!in.drop || (f & NJODE_C_TRAIN)) print_call(row, o, sizes[0], f, in);   // (masks are drawn by training calls only)
    ++row;
  }
  return 0;
}
