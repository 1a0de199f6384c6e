// njode_online_args.h -- what the online entry points (njode_online.hip) hand to the per-shape
// kernel unit (njode_cfg.hip, part 6: njode_online.h), and those of njode_gen.hip to k_gen_online
// (njode_gen_online.h; it ignores spb).  Plain data, host and device.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/njode_hip.h"

namespace njode {

enum OnlineMode { ONLINE_ADVANCE = 0, ONLINE_OBSERVE = 1, ONLINE_PREDICT = 2, ONLINE_RESET = 3, ONLINE_RUN = 4 };
constexpr int ONLINE_WAVES = 8;   // waves per block; the first `spb` of them own a series each

struct OnlineArgs {
  const float* P;         // flat parameter vector
  // the resident state, row i = series i (predict reads it only)
  float* h;               // [n_series][H]
  float* last_X;          // [n_series][D]
  float* tau;             // [n_series]
  double* now;            // [n_series]
  int n_series;
  const int* ids;         // [n] series of the call's rows, or null: 0 .. n-1
  int n;
  const double* t;        // [n][Q] targets (Q = 1 but for predict)
  int Q;
  const float* X;         // [n][D] observe: the observation; reset: start_X
  const float* M;         // [n][D] masked models
  double delta_t, eps_dt; // eps_dt = 1e-10 * delta_t, multiplied on the host (no contraction)
  int max_steps;          // bound of the step loop in front of ONE target
  float* Y_before;        // [n][DO] observe, nullable
  float* Y;               // [n][DO] observe (nullable) | [n][Q][DO] predict
  int* status;            // [n]: 0 reached, 1 the bound stopped it, 2 id outside the state, 3 bad event range
  // run: events by series (CSR); t, X, M, Y_before, Y are then [n_events] rows, indexed by event
  const int* ev_ptr;      // [n + 1] row r owns events ev_ptr[r] .. ev_ptr[r + 1] - 1
  int n_events;
  const int* kind;        // [n_events] 1 observation, 0 empty slice; null: all observations
  int* n_done;            // [n] events of the row that were applied
  int spb;                // series per block, 1 .. ONLINE_WAVES
};

struct OnlineOps {
  NjodeDims dims;
  int ok;                 // the shape has the kernel (OnlineOk, njode_online.h)
  hipError_t (*launch)(const OnlineArgs&, int mode, hipStream_t);
};

}  // namespace njode
