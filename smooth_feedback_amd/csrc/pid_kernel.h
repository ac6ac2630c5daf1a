// Host<->kernel interface of the batched Lie-group PID kernels.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sfb.h"

namespace sfb {

// the group of sfb_pid_group, checked and copied (travels to the kernel by value)
struct PidGroup {
  int32_t nparts;
  int32_t kind[SFB_PID_MAX_PARTS], dof[SFB_PID_MAX_PARTS];
  int32_t elem, dofs;  // doubles per element / per tangent of the whole bundle
};

struct PidArgs {
  PidGroup grp;
  int64_t batch;
  double t, dt;  // step: t; rollout: t0 and the tick length
  int64_t steps;
  double windup_limit;
  int des_shared, gains_shared;
  const double *g_des, *v_des, *a_des;  // rollout: g_des0, v_des, a_des unused
  const double *kp, *kd, *ki;
  const double *u_max;  // rollout, nullable
  double *x, *v;        // step: read only
  double *i_err, *t_last;
  double *u, *cost;  // step: u; rollout: u_last and cost
};

// false with a message for a bad descriptor (kinds outside sfb_lie_kind, dof inconsistent with the kind, part count)
bool pid_group_from(const sfb_pid_group *g, PidGroup &out, const char **why);
hipError_t pid_step_launch(const PidArgs &a, hipStream_t stream);
hipError_t pid_rollout_launch(const PidArgs &a, hipStream_t stream);

}  // namespace sfb
