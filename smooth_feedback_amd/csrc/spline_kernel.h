// Host<->kernel interface of the batched Lie-group spline kernels (fit, evaluation, PID rollout along a spline).  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pid_kernel.h"

namespace sfb {

// a batch of cubic splines in the flat layout of include/sfb.h: per agent tk [S+1], gk [S+1][elem], V [S][3][dof];
// shared != 0: one spline for every agent; ts0 [batch] nullable: the agent's time origin
struct SplineRef {
  int64_t S;
  int shared;
  const double *tk, *gk, *V, *ts0;
};

struct SplineFitArgs {
  PidGroup grp;
  int64_t batch, S;
  int tk_shared;
  const double *tk, *gk;
  double *V;
};

struct SplineEvalArgs {
  PidGroup grp;
  int64_t batch, nt;
  SplineRef c;
  int t_shared;
  const double *t;
  double *g, *vel, *acc;
};

// the rollout's arguments with the spline in place of g_des / v_des (unused here)
struct PidSplineArgs {
  PidArgs p;
  SplineRef c;
};

hipError_t spline_fit_launch(const SplineFitArgs &a, hipStream_t stream);
hipError_t spline_eval_launch(const SplineEvalArgs &a, hipStream_t stream);
hipError_t pid_rollout_spline_launch(const PidSplineArgs &a, hipStream_t stream);

}  // namespace sfb
