// njode_hostlib.h -- what every host-side unit of the library needs and none owns: the error
// message, the HIP call guard, the profile scope, integer helpers, the workspace arena and the
// per-device state.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stddef.h>
#include <mutex>

#include "../../include/njode_hip.h"

namespace njode {

// ---- errors: the thread-local message njode_last_error() returns is owned by njode_api.hip
int set_error_v(int code, const char* fmt, va_list ap);
inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  set_error_v(code, fmt, ap);
  va_end(ap);
  return code;
}
#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return ::njode::fail(NJODE_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
  } while (0)

// a kernel that asks for more dynamic LDS than the 48 KB a launch gets without saying so (static:
// every unit has its own, the library exports none)
static inline int set_lds(const void* fn, int bytes) {
  if (bytes > 48 * 1024) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return NJODE_OK;
}

// ---- optional per-kernel timing (njode_profile_enable / njode_profile_read, njode_prof.hip):
// HIP events recorded on the launch stream around each kernel
void prof_mark(const char* name, hipStream_t st, bool begin);
struct ProfScope {
  const char* name;
  hipStream_t st;
  ProfScope(const char* n, hipStream_t s) : name(n), st(s) { prof_mark(name, st, true); }
  ~ProfScope() { prof_mark(name, st, false); }
};

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
inline int bits_for(unsigned v) {  // radix bits needed for keys in [0, v]
  int b = 1;
  while (b < 32 && (v >> b)) ++b;
  return b;
}

// Offsets of a workspace, taken in order, each a multiple of 256 bytes
struct Arena {
  size_t total = 0;
  size_t take(size_t bytes) {
    size_t off = total;
    total += (bytes + 255) & ~(size_t)255;
    return off;
  }
};

// ---- what the library keeps per device, for the life of the process (with the profiler's events
// the only state it has).  Every member is created on first use by the one function that reads it
// (named beside it), under the lock device_state() returns with.
struct DeviceState {
  double total_mem = 0.0;                  // record_budget_bytes()
  int n_cu = 0;                            // device_cu_count()
  // helper streams of a forward call and a ring of their events (side_streams(), njode_planner.hip)
  hipStream_t st = nullptr, st2 = nullptr;
  hipEvent_t ev[8][3] = {};
  unsigned next = 0;
  // one-launch plan: [0] the word a grid barrier sets when it gives up waiting, then the stage
  // stamps of the last job (plan_sync_mem(), njode_planner.hip)
  unsigned* plan_mem = nullptr;
};
struct DeviceLock {
  std::unique_lock<std::mutex> lk;
  DeviceState* d = nullptr;   // null: no current device, or one beyond the 64 the library keeps state for
  int dev = 0;
};
DeviceLock device_state();     // njode_api.hip
// Budget of the per-(tile, Euler step) TRAINING RECORDS of the masked lockstep kernels, which grow
// up to 16x when a tile holds fewer than 16 paths (q4_pt of njode_route.h, gen_paths_per_tile): the
// smaller of NJODE_REC_BUDGET_GB (default 16) and 1/8 of the device's TOTAL memory.  Total, not
// free: the layout is computed twice per call (njode_workspace_bytes, then the call itself, after
// the caller has allocated the workspace) and must come out the same both times.
double record_budget_bytes();  // njode_api.hip
int device_cu_count();         // njode_api.hip (256 when the device does not say)

}  // namespace njode
