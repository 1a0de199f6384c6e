// njode_prof.hip -- optional per-kernel timing (njode_profile_enable / njode_profile_read of
// include/njode_hip.h): HIP events recorded on the launch stream around each kernel by the
// ProfScope of njode_hostlib.h.  A measurement aid, process-global.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "njode_hostlib.h"

using namespace njode;

namespace {
struct ProfRec { const char* name; hipEvent_t e0, e1; };
struct Prof {
  std::mutex mu;
  bool on = false;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
  int mode = 1;
} g_prof;
}  // namespace
namespace njode {
void prof_mark(const char* name, hipStream_t st, bool begin) {
  if (!g_prof.on) return;
  // mode 2: the ODE backward only (two events per step instead of twelve: the events of a full
  // profile cost ~3.5 % of a 1.1 ms step)
  if (g_prof.mode == 2 && strncmp(name, "k_ode_bwd", 9) != 0) return;
  std::lock_guard<std::mutex> lk(g_prof.mu);
  if (begin) {
    if (g_prof.recs.size() >= (1u << 18)) return;
    ProfRec r{name, g_prof.get(), g_prof.get()};
    if (!r.e0 || !r.e1) return;
    (void)hipEventRecord(r.e0, st);
    g_prof.recs.push_back(r);
  } else {
    for (size_t i = g_prof.recs.size(); i-- > 0;) {
      if (g_prof.recs[i].name == name) { (void)hipEventRecord(g_prof.recs[i].e1, st); break; }
    }
  }
}
}  // namespace njode

extern "C" int njode_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  g_prof.on = on != 0;
  g_prof.mode = on;
  return NJODE_OK;
}

extern "C" int njode_profile_read(char* out, size_t cap) {
  if (!out || cap == 0) return fail(NJODE_E_BADARG, "null buffer");
  std::lock_guard<std::mutex> lk(g_prof.mu);
  if (hipDeviceSynchronize() != hipSuccess) return fail(NJODE_E_HIP, "synchronize failed");
  std::map<std::string, std::pair<int, double>> acc;
  for (const ProfRec& r : g_prof.recs) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
      auto& a = acc[r.name];
      a.first += 1;
      a.second += ms;
    }
    g_prof.pool.push_back(r.e0);
    g_prof.pool.push_back(r.e1);
  }
  g_prof.recs.clear();
  size_t n = 0;
  out[0] = 0;
  for (const auto& kv : acc) {
    int w = snprintf(out + n, cap - n, "%s %d %.6f\n", kv.first.c_str(), kv.second.first,
                     kv.second.second);
    if (w < 0 || (size_t)w >= cap - n) break;
    n += (size_t)w;
  }
  return NJODE_OK;
}
