// njode_planner.h -- the batch planner of the compiled shapes (njode_planner.hip: CSR-by-time ->
// per-path links -> length-sorted segment items, tail order, trajectory layout), as far as the
// C ABI unit (njode_api.hip) calls it.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/njode_hip.h"
#include "../../include/njode_selftest.h"
#include "njode_plan.h"

namespace njode {

struct Call;   // njode_layout.h

// Temporary storage of the plan's radix sorts (rows by path, rows by length, tails by length), the
// largest of the three: part of the plan prefix make_layout() lays out.
size_t plan_sort_temp_bytes(int n_obs, int B, int K);

// The plan of the prepared call `c` into the prefix at `ws`, whose schedule block is uploaded, on `st`.
int build_plan(Call& c, void* ws, hipStream_t st);
// njode_plan_f32 behind prepare(): schedule upload and plan into c.pw -- at once, or
// (NJODE_C_PLAN_DEFER, where the one-launch plan can build it) left pending for the next forward.
int plan_call(Call& c, const NjodeSchedule* sched, int call_flags, hipStream_t st);

// A plan whose launch was deferred (njode_plan_f32 with NJODE_C_PLAN_DEFER): it rides in front of the
// ODE-forward launch of the next njode_forward_f32 call this thread makes on the same stream, or is
// launched as a kernel of its own in front of that call when it cannot host it.
struct PendingPlan {
  bool on = false;
  PlanJob job;
  hipStream_t st = nullptr;
  bool tails = false;         // ... then the tail order (hT) behind it: k_tail_order's arguments
  int tB = 0, tK = 0;
  const int *t_last_row = nullptr, *t_t_of_row = nullptr, *t_k_jump = nullptr;
  int* t_order = nullptr;
};
// Launches this thread's pending plan, if any, as a kernel of its own; false: there was none.
bool pending_flush();
// njode_forward_f32, once the call's own plan is in place: this thread's pending plan moves into
// `hosted` and rides in the call's ODE-forward launch on `st` (c.a.plan_job), or is flushed when
// the call cannot host it.  pending_tails(hosted) goes behind that launch.
void pending_host_or_flush(Call& c, hipStream_t st, PendingPlan& hosted);
void pending_tails(const PendingPlan& p);

// njode_debug_plan_view behind prepare(): which builder build_plan / plan_call would take for the
// prepared call `c` in this process, and what that builder defines.  Launches nothing.
void describe_plan(const Call& c, int call_flags, NjodePlanView* v);

}  // namespace njode
