// gls_time_control.cpp — the transient simulation control (host only): the reference's
// SimulationControlTransient and SimulationControlTransientDynamicOutput (source/core/simulation_control.cc:
// 84-147, 173-218) restated behind the C ABI. The controller owns the iteration number, the time, the
// step and the four most recent steps (newest first: what gls_set_time / gls_bdf_coefficients take).
#include <cmath>

#include "../../include/gls_native.h"
#include "gls_error.hpp"

struct gls_time_control {
  gls_time_control_params prm;
  double time = 0.0, time_step = 0.0, cfl = 0.0;
  int iteration = 0;
  double steps[4] = {0, 0, 0, 0};  // time_step_vector (simulation_control.cc:24-25)
  bool forced_output = false;      // SimulationControlTransientDynamicOutput::time_step_forced_output
  double last_output_time = 0.0;
};

namespace {

bool at_end(const gls_time_control *t) {  // is_at_end (simulation_control.cc:126-130)
  return t->time >= t->prm.time_end - 1e-12 * t->time_step;
}

// calculate_time_step (simulation_control.cc:132-147; the time-output variant :180-206, which scales the
// step whatever `adapt` says, as the reference's class does)
double next_step(gls_time_control *t) {
  const gls_time_control_params &p = t->prm;
  const bool by_time = p.output_control == GLS_OUTPUT_TIME;
  double dt = t->time_step;
  if (by_time && t->forced_output) {
    dt = t->steps[1];
    t->forced_output = false;
  } else if ((by_time || p.adapt) && t->iteration > 1) {
    dt = t->time_step * p.scaling;
    if (t->cfl > 0 && p.max_cfl / t->cfl < p.scaling) dt = t->time_step * p.max_cfl / t->cfl;
  }
  if (t->time + dt > p.time_end) dt = p.time_end - t->time;
  if (by_time && t->time + dt > t->last_output_time + p.output_time) {
    dt = t->last_output_time + p.output_time - t->time;
    t->forced_output = true;
  }
  return dt;
}

}  // namespace

extern "C" {

int gls_time_control_create(const gls_time_control_params *prm, gls_time_control **out) {
  if (!prm || !out) return gls_internal_set_err(GLS_EINVAL, "gls_time_control_create: null argument");
  *out = nullptr;
  if (!(prm->dt > 0) || !std::isfinite(prm->dt) || !std::isfinite(prm->time_end))
    return gls_internal_set_err(GLS_EINVAL, "gls_time_control_create: dt must be positive and finite");
  if (prm->output_control != GLS_OUTPUT_ITERATION && prm->output_control != GLS_OUTPUT_TIME)
    return gls_internal_set_err(GLS_EINVAL, "gls_time_control_create: output control is iteration (0) or time (1)");
  if (prm->output_control == GLS_OUTPUT_ITERATION && prm->output_frequency < 1)
    return gls_internal_set_err(GLS_EINVAL, "gls_time_control_create: output frequency must be >= 1");
  if (prm->output_control == GLS_OUTPUT_TIME && !(prm->output_time > 0))
    return gls_internal_set_err(GLS_EINVAL, "gls_time_control_create: output time must be positive");
  if ((prm->adapt || prm->output_control == GLS_OUTPUT_TIME) && (!(prm->scaling > 0) || !(prm->max_cfl > 0)))
    return gls_internal_set_err(GLS_EINVAL,
                                "gls_time_control_create: adaptive stepping needs max cfl > 0 and a scaling > 0");
  gls_time_control *t = new gls_time_control;
  t->prm = *prm;
  t->time_step = prm->dt;
  t->steps[0] = prm->dt;
  *out = t;
  return GLS_OK;
}

void gls_time_control_destroy(gls_time_control *t) { delete t; }

int gls_time_control_integrate(gls_time_control *t) {  // integrate + add_time_step (simulation_control.cc:28-38, 109-122)
  if (!t) return gls_internal_set_err(GLS_EINVAL, "gls_time_control_integrate: null controller");
  if (at_end(t)) return 0;
  ++t->iteration;
  const double dt = next_step(t);
  t->time_step = dt;
  for (int i = 3; i > 0; --i) t->steps[i] = t->steps[i - 1];
  t->steps[0] = dt;
  t->time += dt;
  return 1;
}

int gls_time_control_set_cfl(gls_time_control *t, double cfl) {
  if (!t) return gls_internal_set_err(GLS_EINVAL, "gls_time_control_set_cfl: null controller");
  t->cfl = cfl;
  return GLS_OK;
}

int gls_time_control_get(const gls_time_control *t, int *iteration, double *time, double *time_step, double steps[4]) {
  if (!t) return gls_internal_set_err(GLS_EINVAL, "gls_time_control_get: null controller");
  if (iteration) *iteration = t->iteration;
  if (time) *time = t->time;
  if (time_step) *time_step = t->time_step;
  if (steps)
    for (int i = 0; i < 4; ++i) steps[i] = t->steps[i];
  return GLS_OK;
}

int gls_time_control_is_output_iteration(gls_time_control *t) {
  if (!t) return gls_internal_set_err(GLS_EINVAL, "gls_time_control_is_output_iteration: null controller");
  if (t->prm.output_control == GLS_OUTPUT_ITERATION)  // simulation_control.cc:40-44
    return t->iteration % t->prm.output_frequency == 0 ? 1 : 0;
  const double f = t->prm.output_time;  // simulation_control.cc:208-218
  const bool is_output_time = (t->time - t->last_output_time) - f > -1e-12 * f;
  if (is_output_time) t->last_output_time = t->time;
  return is_output_time ? 1 : 0;
}

}  // extern "C"
