// C-ABI for the batched Lie-group spline path (include/sfb.h): cubic fit, evaluation, PID rollout along a spline.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sfb.h"
#include "capi_common.h"
#include "spline_kernel.h"

namespace {

// what every entry point refuses first, in this order: descriptor, batch, knot count
sfb_status spline_check(const sfb_pid_group *group, int64_t batch, int64_t nknots, sfb::PidGroup &grp)
{
  const char *why = nullptr;
  if (!sfb::pid_group_from(group, grp, &why)) return sfb::fail(SFB_ERR_INVALID_ARG, why);
  if (batch < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "batch < 0");
  if (nknots < 2) return sfb::fail(SFB_ERR_INVALID_ARG, "nknots < 2");
  return SFB_OK;
}

// the _host entries see the knot times: `count` rows of nknots, each finite and strictly increasing
sfb_status knot_times_check(const double *tk, int64_t count, int64_t nknots)
{
  for (int64_t b = 0; b < count; ++b)
    for (int64_t i = 0; i < nknots; ++i) {
      const double t = tk[b * nknots + i];
      if (!std::isfinite(t) || (i > 0 && !(t > tk[b * nknots + i - 1])))
        return sfb::fail(SFB_ERR_INVALID_ARG, "knot times must be finite and strictly increasing");
    }
  return SFB_OK;
}

sfb_status fit_check(const sfb_pid_group *group, int64_t batch, int64_t nknots, const double *tk, const double *gk, double *V, sfb::PidGroup &grp)
{
  const sfb_status st = spline_check(group, batch, nknots, grp);
  if (st != SFB_OK) return st;
  if (batch > 0 && (!tk || !gk || !V)) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  return SFB_OK;
}

sfb_status eval_check(const sfb_pid_group *group, int64_t batch, int64_t nknots, int64_t nt, const double *tk, const double *gk, const double *V,
                      const double *t, double *g, double *vel, double *acc, sfb::PidGroup &grp)
{
  const sfb_status st = spline_check(group, batch, nknots, grp);
  if (st != SFB_OK) return st;
  if (nt < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "nt < 0");
  if (batch > 0 && nt > 0 && (!tk || !gk || !V || !t || !g || !vel || !acc)) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  return SFB_OK;
}

sfb_status rollout_check(const sfb_pid_group *group, int64_t batch, int64_t nknots, double t0, double dt, int64_t steps, double windup_limit,
                         bool arrays, sfb::PidGroup &grp)
{
  const sfb_status st = spline_check(group, batch, nknots, grp);
  if (st != SFB_OK) return st;
  if (steps < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "steps < 0");
  if (!std::isfinite(dt) || !std::isfinite(t0)) return sfb::fail(SFB_ERR_INVALID_ARG, "t0 / dt is not finite");
  if (!(windup_limit >= 0.0)) return sfb::fail(SFB_ERR_INVALID_ARG, "windup_limit must be >= 0 (+inf: no clamp)");
  if (batch > 0 && !arrays) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  return SFB_OK;
}

}  // namespace

extern "C" {

sfb_status sfb_spline_fit_cubic_batch(const sfb_pid_group *group, int64_t batch, int64_t nknots, const double *tk, int tk_shared,
                                      const double *gk, double *V, void *stream)
{
  sfb::SplineFitArgs a{};
  sfb_status st = fit_check(group, batch, nknots, tk, gk, V, a.grp);
  if (st != SFB_OK) return st;
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  a.batch = batch; a.S = nknots - 1; a.tk_shared = tk_shared; a.tk = tk; a.gk = gk; a.V = V;
  hipError_t e = sfb::spline_fit_launch(a, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return sfb::hip_fail(e, "spline_fit_kernel launch");
  return SFB_OK;
}

sfb_status sfb_spline_eval_batch(const sfb_pid_group *group, int64_t batch, int64_t nknots, const double *tk, const double *gk,
                                 const double *V, int spline_shared, const double *ts0, int64_t nt, const double *t, int t_shared,
                                 double *g, double *vel, double *acc, void *stream)
{
  sfb::SplineEvalArgs a{};
  sfb_status st = eval_check(group, batch, nknots, nt, tk, gk, V, t, g, vel, acc, a.grp);
  if (st != SFB_OK) return st;
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0 || nt == 0) return SFB_OK;
  a.batch = batch; a.nt = nt; a.c = sfb::SplineRef{nknots - 1, spline_shared, tk, gk, V, ts0};
  a.t_shared = t_shared; a.t = t; a.g = g; a.vel = vel; a.acc = acc;
  hipError_t e = sfb::spline_eval_launch(a, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return sfb::hip_fail(e, "spline_eval_kernel launch");
  return SFB_OK;
}

sfb_status sfb_pid_rollout_spline_batch(const sfb_pid_group *group, int64_t batch, double t0, double dt, int64_t steps, double *x,
                                        double *v, int64_t nknots, const double *tk, const double *gk, const double *V,
                                        int spline_shared, const double *ts0, const double *kp, const double *kd, const double *ki,
                                        int gains_shared, double windup_limit, const double *u_max, double *i_err, double *t_last,
                                        double *u_last, double *cost, void *stream)
{
  sfb::PidSplineArgs s{};
  sfb::PidArgs &a = s.p;
  sfb_status st   = rollout_check(group, batch, nknots, t0, dt, steps, windup_limit,
                                  x && v && tk && gk && V && kp && kd && ki && i_err && t_last && u_last && cost, a.grp);
  if (st != SFB_OK) return st;
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0 || steps == 0) return SFB_OK;
  a.batch = batch; a.t = t0; a.dt = dt; a.steps = steps; a.windup_limit = windup_limit; a.gains_shared = gains_shared;
  a.kp = kp; a.kd = kd; a.ki = ki; a.u_max = u_max;
  a.x = x; a.v = v; a.i_err = i_err; a.t_last = t_last; a.u = u_last; a.cost = cost;
  s.c = sfb::SplineRef{nknots - 1, spline_shared, tk, gk, V, ts0};
  hipError_t e = sfb::pid_rollout_spline_launch(s, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return sfb::hip_fail(e, "pid_rollout_spline_kernel launch");
  return SFB_OK;
}

sfb_status sfb_spline_fit_cubic_batch_host(const sfb_pid_group *group, int64_t batch, int64_t nknots, const double *tk, int tk_shared,
                                           const double *gk, double *V)
{
  // the device entry point's checks: same order, same messages; then what only a host entry can see
  sfb::PidGroup grp;
  sfb_status st = fit_check(group, batch, nknots, tk, gk, V, grp);
  if (st != SFB_OK) return st;
  if (batch > 0 && (st = knot_times_check(tk, tk_shared ? 1 : batch, nknots)) != SFB_OK) return st;
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  const size_t B = (size_t)batch, E = (size_t)grp.elem, D = (size_t)grp.dofs, K = (size_t)nknots;
  using S = sfb::Staging;
  S s;
  double *dtk, *dgk, *dV;
  s.add(&dtk, (tk_shared ? 1 : B) * K, S::In, tk); s.add(&dgk, B * K * E, S::In, gk); s.add(&dV, B * (K - 1) * 3 * D, S::Out, V);
  return sfb::staged_call(s, "sfb_spline_fit_cubic_batch_host",
                          [&] { return sfb_spline_fit_cubic_batch(group, batch, nknots, dtk, tk_shared, dgk, dV, nullptr); });
}

sfb_status sfb_spline_eval_batch_host(const sfb_pid_group *group, int64_t batch, int64_t nknots, const double *tk, const double *gk,
                                      const double *V, int spline_shared, const double *ts0, int64_t nt, const double *t,
                                      int t_shared, double *g, double *vel, double *acc)
{
  sfb::PidGroup grp;
  sfb_status st = eval_check(group, batch, nknots, nt, tk, gk, V, t, g, vel, acc, grp);
  if (st != SFB_OK) return st;
  if (batch > 0 && nt > 0 && (st = knot_times_check(tk, spline_shared ? 1 : batch, nknots)) != SFB_OK) return st;
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0 || nt == 0) return SFB_OK;
  const size_t B = (size_t)batch, E = (size_t)grp.elem, D = (size_t)grp.dofs, K = (size_t)nknots, Bs = spline_shared ? 1 : B, T = (size_t)nt;
  using S = sfb::Staging;
  S s;
  double *dtk, *dgk, *dV, *dts, *dt, *dg, *dvel, *dacc;
  s.add(&dtk, Bs * K, S::In, tk); s.add(&dgk, Bs * K * E, S::In, gk); s.add(&dV, Bs * (K - 1) * 3 * D, S::In, V);
  s.add_opt(&dts, B, S::In, ts0); s.add(&dt, (t_shared ? 1 : B) * T, S::In, t);
  s.add(&dg, B * T * E, S::Out, g); s.add(&dvel, B * T * D, S::Out, vel); s.add(&dacc, B * T * D, S::Out, acc);
  return sfb::staged_call(s, "sfb_spline_eval_batch_host", [&] {
    return sfb_spline_eval_batch(group, batch, nknots, dtk, dgk, dV, spline_shared, dts, nt, dt, t_shared, dg, dvel, dacc, nullptr);
  });
}

sfb_status sfb_pid_rollout_spline_batch_host(const sfb_pid_group *group, int64_t batch, double t0, double dt, int64_t steps, double *x,
                                             double *v, int64_t nknots, const double *tk, const double *gk, const double *V,
                                             int spline_shared, const double *ts0, const double *kp, const double *kd,
                                             const double *ki, int gains_shared, double windup_limit, const double *u_max,
                                             double *i_err, double *t_last, double *u_last, double *cost)
{
  sfb::PidGroup grp;
  sfb_status st = rollout_check(group, batch, nknots, t0, dt, steps, windup_limit,
                                x && v && tk && gk && V && kp && kd && ki && i_err && t_last && u_last && cost, grp);
  if (st != SFB_OK) return st;
  if (batch > 0 && steps > 0 && (st = knot_times_check(tk, spline_shared ? 1 : batch, nknots)) != SFB_OK) return st;  // as eval: only with work to do
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0 || steps == 0) return SFB_OK;
  const size_t B = (size_t)batch, E = (size_t)grp.elem, D = (size_t)grp.dofs, K = (size_t)nknots, Bs = spline_shared ? 1 : B,
               Bg = gains_shared ? 1 : B;
  using S = sfb::Staging;
  S s;
  double *dx, *dv, *dtk, *dgk, *dV, *dts, *dkp, *dkd, *dki, *dum, *die, *dtl, *du, *dc;
  s.add(&dx, B * E, S::InOut, x); s.add(&dv, B * D, S::InOut, v);
  s.add(&dtk, Bs * K, S::In, tk); s.add(&dgk, Bs * K * E, S::In, gk); s.add(&dV, Bs * (K - 1) * 3 * D, S::In, V);
  s.add_opt(&dts, B, S::In, ts0);
  s.add(&dkp, Bg * D, S::In, kp); s.add(&dkd, Bg * D, S::In, kd); s.add(&dki, Bg * D, S::In, ki); s.add_opt(&dum, D, S::In, u_max);
  s.add(&die, B * D, S::InOut, i_err); s.add(&dtl, B, S::InOut, t_last); s.add(&du, B * D, S::Out, u_last); s.add(&dc, B, S::Out, cost);
  return sfb::staged_call(s, "sfb_pid_rollout_spline_batch_host", [&] {
    return sfb_pid_rollout_spline_batch(group, batch, t0, dt, steps, dx, dv, nknots, dtk, dgk, dV, spline_shared, dts, dkp, dkd, dki, gains_shared,
                                        windup_limit, dum, die, dtl, du, dc, nullptr);
  });
}

}  // extern "C"
