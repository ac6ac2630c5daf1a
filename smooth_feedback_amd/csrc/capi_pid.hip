// C-ABI for the batched Lie-group PID path (include/sfb.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/sfb.h"
#include "capi_common.h"
#include "pid_kernel.h"

namespace {

// everything that can be refused without a device; fills the kernel arguments' group
sfb_status pid_check(const sfb_pid_group *group, int64_t batch, double windup_limit, sfb::PidGroup &grp)
{
  const char *why = nullptr;
  if (!sfb::pid_group_from(group, grp, &why)) return sfb::fail(SFB_ERR_INVALID_ARG, why);
  if (batch < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "batch < 0");
  if (!(windup_limit >= 0.0)) return sfb::fail(SFB_ERR_INVALID_ARG, "windup_limit must be >= 0 (+inf: no clamp)");
  return SFB_OK;
}

}  // namespace

extern "C" {

int64_t sfb_pid_elem_doubles(const sfb_pid_group *group)
{
  sfb::PidGroup g;
  const char *why = nullptr;
  return sfb::pid_group_from(group, g, &why) ? g.elem : -1;
}

int64_t sfb_pid_dof(const sfb_pid_group *group)
{
  sfb::PidGroup g;
  const char *why = nullptr;
  return sfb::pid_group_from(group, g, &why) ? g.dofs : -1;
}

sfb_status sfb_pid_step_batch(const sfb_pid_group *group, int64_t batch, double t, const double *x, const double *v,
                              const double *g_des, const double *v_des, const double *a_des, int des_shared,
                              const double *kp, const double *kd, const double *ki, int gains_shared,
                              double windup_limit, double *i_err, double *t_last, double *u, void *stream)
{
  sfb::PidArgs a{};
  sfb_status st = pid_check(group, batch, windup_limit, a.grp);
  if (st != SFB_OK) return st;
  if (!std::isfinite(t)) return sfb::fail(SFB_ERR_INVALID_ARG, "t is not finite");
  if (batch > 0 && (!x || !v || !g_des || !v_des || !a_des || !kp || !kd || !ki || !i_err || !t_last || !u))
    return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  a.batch = batch; a.t = t; a.windup_limit = windup_limit; a.des_shared = des_shared; a.gains_shared = gains_shared;
  a.g_des = g_des; a.v_des = v_des; a.a_des = a_des; a.kp = kp; a.kd = kd; a.ki = ki;
  a.x = const_cast<double *>(x); a.v = const_cast<double *>(v);  // read only in the step kernel
  a.i_err = i_err; a.t_last = t_last; a.u = u;
  hipError_t e = sfb::pid_step_launch(a, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return sfb::hip_fail(e, "pid_step_kernel launch");
  return SFB_OK;
}

sfb_status sfb_pid_rollout_batch(const sfb_pid_group *group, int64_t batch, double t0, double dt, int64_t steps,
                                 double *x, double *v, const double *g_des0, const double *v_des, int des_shared,
                                 const double *kp, const double *kd, const double *ki, int gains_shared,
                                 double windup_limit, const double *u_max, double *i_err, double *t_last,
                                 double *u_last, double *cost, void *stream)
{
  sfb::PidArgs a{};
  sfb_status st = pid_check(group, batch, windup_limit, a.grp);
  if (st != SFB_OK) return st;
  if (steps < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "steps < 0");
  if (!std::isfinite(dt) || !std::isfinite(t0)) return sfb::fail(SFB_ERR_INVALID_ARG, "t0 / dt is not finite");
  if (batch > 0 && (!x || !v || !g_des0 || !v_des || !kp || !kd || !ki || !i_err || !t_last || !u_last || !cost))
    return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0 || steps == 0) return SFB_OK;
  a.batch = batch; a.t = t0; a.dt = dt; a.steps = steps; a.windup_limit = windup_limit;
  a.des_shared = des_shared; a.gains_shared = gains_shared;
  a.g_des = g_des0; a.v_des = v_des; a.kp = kp; a.kd = kd; a.ki = ki; a.u_max = u_max;
  a.x = x; a.v = v; a.i_err = i_err; a.t_last = t_last; a.u = u_last; a.cost = cost;
  hipError_t e = sfb::pid_rollout_launch(a, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return sfb::hip_fail(e, "pid_rollout_kernel launch");
  return SFB_OK;
}

sfb_status sfb_pid_step_batch_host(const sfb_pid_group *group, int64_t batch, double t, const double *x,
                                   const double *v, const double *g_des, const double *v_des, const double *a_des,
                                   int des_shared, const double *kp, const double *kd, const double *ki,
                                   int gains_shared, double windup_limit, double *i_err, double *t_last, double *u)
{
  // the device entry point's checks with NULL device work: same order, same messages
  sfb::PidGroup grp;
  sfb_status st = pid_check(group, batch, windup_limit, grp);
  if (st != SFB_OK) return st;
  if (!std::isfinite(t)) return sfb::fail(SFB_ERR_INVALID_ARG, "t is not finite");
  if (batch > 0 && (!x || !v || !g_des || !v_des || !a_des || !kp || !kd || !ki || !i_err || !t_last || !u))
    return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  const size_t B = (size_t)batch, E = (size_t)grp.elem, D = (size_t)grp.dofs, Bd = des_shared ? 1 : B, Bg = gains_shared ? 1 : B;
  using S = sfb::Staging;
  S s;
  double *dx, *dv, *dg, *dvd, *dad, *dkp, *dkd, *dki, *die, *dtl, *du;
  s.add(&dx, B * E, S::In, x); s.add(&dv, B * D, S::In, v);
  s.add(&dg, Bd * E, S::In, g_des); s.add(&dvd, Bd * D, S::In, v_des); s.add(&dad, Bd * D, S::In, a_des);
  s.add(&dkp, Bg * D, S::In, kp); s.add(&dkd, Bg * D, S::In, kd); s.add(&dki, Bg * D, S::In, ki);
  s.add(&die, B * D, S::InOut, i_err); s.add(&dtl, B, S::InOut, t_last); s.add(&du, B * D, S::Out, u);
  return sfb::staged_call(s, "sfb_pid_step_batch_host", [&] {
    return sfb_pid_step_batch(group, batch, t, dx, dv, dg, dvd, dad, des_shared, dkp, dkd, dki, gains_shared, windup_limit, die, dtl, du, nullptr);
  });
}

sfb_status sfb_pid_rollout_batch_host(const sfb_pid_group *group, int64_t batch, double t0, double dt, int64_t steps,
                                      double *x, double *v, const double *g_des0, const double *v_des, int des_shared,
                                      const double *kp, const double *kd, const double *ki, int gains_shared,
                                      double windup_limit, const double *u_max, double *i_err, double *t_last,
                                      double *u_last, double *cost)
{
  sfb::PidGroup grp;
  sfb_status st = pid_check(group, batch, windup_limit, grp);
  if (st != SFB_OK) return st;
  if (steps < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "steps < 0");
  if (!std::isfinite(dt) || !std::isfinite(t0)) return sfb::fail(SFB_ERR_INVALID_ARG, "t0 / dt is not finite");
  if (batch > 0 && (!x || !v || !g_des0 || !v_des || !kp || !kd || !ki || !i_err || !t_last || !u_last || !cost))
    return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0 || steps == 0) return SFB_OK;
  const size_t B = (size_t)batch, E = (size_t)grp.elem, D = (size_t)grp.dofs, Bd = des_shared ? 1 : B, Bg = gains_shared ? 1 : B;
  using S = sfb::Staging;
  S s;
  double *dx, *dv, *dg, *dvd, *dkp, *dkd, *dki, *dum, *die, *dtl, *du, *dc;
  s.add(&dx, B * E, S::InOut, x); s.add(&dv, B * D, S::InOut, v);
  s.add(&dg, Bd * E, S::In, g_des0); s.add(&dvd, Bd * D, S::In, v_des);
  s.add(&dkp, Bg * D, S::In, kp); s.add(&dkd, Bg * D, S::In, kd); s.add(&dki, Bg * D, S::In, ki); s.add_opt(&dum, D, S::In, u_max);
  s.add(&die, B * D, S::InOut, i_err); s.add(&dtl, B, S::InOut, t_last); s.add(&du, B * D, S::Out, u_last); s.add(&dc, B, S::Out, cost);
  return sfb::staged_call(s, "sfb_pid_rollout_batch_host", [&] {
    return sfb_pid_rollout_batch(group, batch, t0, dt, steps, dx, dv, dg, dvd, des_shared, dkp, dkd, dki, gains_shared, windup_limit, dum, die, dtl,
                                 du, dc, nullptr);
  });
}

}  // extern "C"
