// njode_online_check.h -- the argument checks both online families share (njode_online.hip: one wave
// per series; njode_gen.hip: a tile of series per workgroup).  Host code.
#pragma once
#include <cmath>

#include "../../include/njode_online.h"
#include "njode_hostlib.h"
#include "njode_online_args.h"

namespace njode {

// params, the state and the rows of a call; fills the common part of the arguments
inline int online_state(const float* params, const NjodeOnlineState* s, const int32_t* ids, int32_t n, OnlineArgs* a) {
  if (!params) return fail(NJODE_E_BADARG, "online: null params");
  if (!s || !s->h || !s->last_X || !s->tau || !s->now) return fail(NJODE_E_BADARG, "online: null state or state array");
  if (s->n_series <= 0) return fail(NJODE_E_BADARG, "online: n_series = %d", s->n_series);
  if (n < 0) return fail(NJODE_E_BADARG, "online: n = %d", n);
  if (!ids && n > s->n_series) return fail(NJODE_E_BADARG, "online: n = %d rows without ids, n_series = %d", n, s->n_series);
  *a = OnlineArgs{};
  a->P = params;
  a->h = s->h;
  a->last_X = s->last_X;
  a->tau = s->tau;
  a->now = s->now;
  a->n_series = s->n_series;
  a->ids = ids;
  a->n = n;
  a->Q = 1;
  a->max_steps = 1;
  // as few series per block as still give every block a CU of its own: a lone wave is
  // latency-bound, and the block's other waves only help to fill the tables
  a->spb = 1;
  while (a->spb < ONLINE_WAVES && cdiv(n, a->spb) > 256) a->spb *= 2;
  return NJODE_OK;
}
// the clock of advance / observe / predict
inline int online_clock(double delta_t, int32_t max_steps, const double* t, const int32_t* status, OnlineArgs* a) {
  if (!(delta_t > 0.0) || !std::isfinite(delta_t))
    return fail(NJODE_E_BADARG, "online: delta_t = %g must be positive and finite", delta_t);
  if (max_steps <= 0) return fail(NJODE_E_BADARG, "online: max_steps = %d", max_steps);
  if (!t || !status) return fail(NJODE_E_BADARG, "online: null t or status");
  a->t = t;
  a->delta_t = delta_t;
  a->eps_dt = 1e-10 * delta_t;
  a->max_steps = max_steps;
  return NJODE_OK;
}
// the clock and the events of a run: t, X, M, kind and the outputs are rows by EVENT, and with
// n_events = 0 nobody reads them
inline int online_events(double delta_t, int32_t max_steps, bool masked, const int32_t* ev_ptr, int32_t n_events,
                         const double* t, const float* X, const float* M, const int32_t* kind, float* Y_before,
                         float* Y, int32_t* status, int32_t* n_done, OnlineArgs* a) {
  if (!(delta_t > 0.0) || !std::isfinite(delta_t))
    return fail(NJODE_E_BADARG, "online: delta_t = %g must be positive and finite", delta_t);
  if (max_steps <= 0) return fail(NJODE_E_BADARG, "online: max_steps = %d", max_steps);
  if (!ev_ptr || !status || !n_done) return fail(NJODE_E_BADARG, "online: null ev_ptr, status or n_done");
  if (n_events < 0) return fail(NJODE_E_BADARG, "online: n_events = %d", n_events);
  if (n_events > 0 && (!t || !X)) return fail(NJODE_E_BADARG, "online: null t or X with n_events = %d", n_events);
  if (masked && n_events > 0 && !M) return fail(NJODE_E_BADARG, "online: a masked model needs M");
  if (!masked && M) return fail(NJODE_E_BADARG, "online: M given to an unmasked model");
  a->t = t;
  a->delta_t = delta_t;
  a->eps_dt = 1e-10 * delta_t;
  a->max_steps = max_steps;
  a->ev_ptr = ev_ptr;
  a->n_events = n_events;
  a->kind = kind;
  a->X = X;
  a->M = M;
  a->Y_before = Y_before;
  a->Y = Y;
  a->status = status;
  a->n_done = n_done;
  return NJODE_OK;
}

}  // namespace njode
