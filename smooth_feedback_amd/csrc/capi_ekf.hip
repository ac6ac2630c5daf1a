// C-ABI for the batched EKF path (include/sfb.h).
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/sfb.h"
#include "capi_common.h"
#include "ekf_kernel.h"

namespace {

sfb_status ekf_common(int64_t batch, int dof, int ny, const double *A, const double *Q, int q_shared, const double *dt,
                      int dt_shared, const double *H, const double *R, int r_shared, const double *r, double *P,
                      double *delta, int32_t *info, bool predict, bool update, void *stream)
{
  if (batch < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "batch < 0");
  if (!predict && !update) return sfb::fail(SFB_ERR_INVALID_ARG, "nothing to do");
  if (batch > 0 && !P) return sfb::fail(SFB_ERR_INVALID_ARG, "P is NULL");
  if (predict && batch > 0 && (!A || !Q || !dt)) return sfb::fail(SFB_ERR_INVALID_ARG, "predict needs A, Q, dt");
  if (update && batch > 0 && (!H || !R || !r || !delta)) return sfb::fail(SFB_ERR_INVALID_ARG, "update needs H, R, r, delta");
  if (!sfb::ekf_supported(dof, ny, update))
    return sfb::fail(SFB_ERR_UNSUPPORTED, "EKF kernels support dof and ny up to 16");
  sfb_status st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  sfb::EkfArgs a{};
  a.batch = batch; a.A = A; a.Q = Q; a.dt = dt; a.q_shared = q_shared; a.dt_shared = dt_shared;
  a.H = H; a.R = R; a.r = r; a.r_shared = r_shared; a.delta = delta; a.info = info; a.P = P;
  hipError_t e = sfb::ekf_launch(a, dof, ny, predict, update, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return sfb::hip_fail(e, "ekf_kernel launch");
  return SFB_OK;
}

}  // namespace

extern "C" {

sfb_status sfb_ekf_predict_batch(int64_t batch, int dof, const double *A, const double *Q, int q_shared,
                                 const double *dt, int dt_shared, double *P, void *stream)
{
  return ekf_common(batch, dof, 1, A, Q, q_shared, dt, dt_shared, nullptr, nullptr, 0, nullptr, P, nullptr, nullptr,
                    true, false, stream);
}

sfb_status sfb_ekf_predict_stepper_batch(int stepper, int64_t batch, int dof, const double *A, const double *Q,
                                         int q_shared, const double *dt, int dt_shared, double *P, void *stream)
{
  if (stepper == SFB_EKF_EULER) return sfb_ekf_predict_batch(batch, dof, A, Q, q_shared, dt, dt_shared, P, stream);
  if (stepper != SFB_EKF_RK4) return sfb::fail(SFB_ERR_INVALID_ARG, "unknown stepper");
  return sfb_ekf_predict_rk4_batch(batch, dof, A, nullptr, nullptr, Q, q_shared, dt, dt_shared, P, stream);
}

sfb_status sfb_ekf_predict_rk4_batch(int64_t batch, int dof, const double *A, const double *A_mid, const double *A_end,
                                     const double *Q, int q_shared, const double *dt, int dt_shared, double *P,
                                     void *stream)
{
  if (batch < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "batch < 0");
  if (batch > 0 && (!A || !Q || !dt || !P)) return sfb::fail(SFB_ERR_INVALID_ARG, "predict needs A, Q, dt, P");
  if ((A_mid == nullptr) != (A_end == nullptr)) return sfb::fail(SFB_ERR_INVALID_ARG, "A_mid and A_end must both be given or both be NULL");
  if (!sfb::ekf_supported(dof, 1, false)) return sfb::fail(SFB_ERR_UNSUPPORTED, "EKF kernels support dof up to 16");
  sfb_status st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  sfb::EkfArgs a{};
  a.batch = batch; a.A = A; a.A_mid = A_mid; a.A_end = A_end; a.Q = Q; a.dt = dt; a.q_shared = q_shared;
  a.dt_shared = dt_shared; a.P = P;
  hipError_t e = sfb::ekf_rk4_launch(a, dof, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return sfb::hip_fail(e, "ekf_rk4_kernel launch");
  return SFB_OK;
}

sfb_status sfb_ekf_predict_rk4_batch_host(int64_t batch, int dof, const double *A, const double *A_mid, const double *A_end,
                                          const double *Q, int q_shared, const double *dt, int dt_shared, double *P)
{
  if (batch < 0 || (batch > 0 && (!A || !Q || !dt || !P))) return sfb::fail(SFB_ERR_INVALID_ARG, "bad arguments");
  if ((A_mid == nullptr) != (A_end == nullptr)) return sfb::fail(SFB_ERR_INVALID_ARG, "A_mid and A_end must both be given or both be NULL");
  if (!sfb::ekf_supported(dof, 1, false)) return sfb::fail(SFB_ERR_UNSUPPORTED, "EKF kernels support dof up to 16");
  sfb_status st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  const size_t B = (size_t)batch, nn = (size_t)dof * dof;
  const size_t nQ = q_shared ? nn : B * nn, nT = dt_shared ? 1 : B;
  using S = sfb::Staging;
  S s;
  double *dP, *dA, *dAm, *dAe, *dQ, *ddt;
  s.add(&dP, B * nn, S::InOut, P); s.add(&dA, B * nn, S::In, A);
  s.add_opt(&dAm, B * nn, S::In, A_mid); s.add_opt(&dAe, B * nn, S::In, A_end);
  s.add(&dQ, nQ, S::In, Q); s.add(&ddt, nT, S::In, dt);
  return sfb::staged_call(s, "sfb_ekf_predict_rk4_batch_host",
                          [&] { return sfb_ekf_predict_rk4_batch(batch, dof, dA, dAm, dAe, dQ, q_shared, ddt, dt_shared, dP, nullptr); });
}

sfb_status sfb_ekf_predict_stepper_batch_host(int stepper, int64_t batch, int dof, const double *A, const double *Q,
                                              int q_shared, const double *dt, int dt_shared, double *P)
{
  if (stepper == SFB_EKF_EULER)
    return sfb_ekf_step_batch_host(batch, dof, 1, A, Q, q_shared, dt, dt_shared, nullptr, nullptr, 0, nullptr, P,
                                   nullptr, nullptr);
  if (stepper != SFB_EKF_RK4) return sfb::fail(SFB_ERR_INVALID_ARG, "unknown stepper");
  return sfb_ekf_predict_rk4_batch_host(batch, dof, A, nullptr, nullptr, Q, q_shared, dt, dt_shared, P);
}

sfb_status sfb_ekf_update_batch(int64_t batch, int dof, int ny, const double *H, const double *R, int r_shared,
                                const double *r, double *P, double *delta, int32_t *info, void *stream)
{
  return ekf_common(batch, dof, ny, nullptr, nullptr, 0, nullptr, 0, H, R, r_shared, r, P, delta, info, false, true,
                    stream);
}

sfb_status sfb_ekf_predict_update_batch(int64_t batch, int dof, int ny, const double *A, const double *Q, int q_shared,
                                        const double *dt, int dt_shared, const double *H, const double *R,
                                        int r_shared, const double *r, double *P, double *delta, int32_t *info,
                                        void *stream)
{
  return ekf_common(batch, dof, ny, A, Q, q_shared, dt, dt_shared, H, R, r_shared, r, P, delta, info, true, true,
                    stream);
}

sfb_status sfb_ekf_step_batch_host(int64_t batch, int dof, int ny, const double *A, const double *Q, int q_shared,
                                   const double *dt, int dt_shared, const double *H, const double *R, int r_shared,
                                   const double *r, double *P, double *delta, int32_t *info)
{
  const bool predict = A != nullptr, update = H != nullptr;
  if (batch < 0 || (!predict && !update) || (batch > 0 && !P)) return sfb::fail(SFB_ERR_INVALID_ARG, "bad arguments");
  if (!sfb::ekf_supported(dof, ny, update))
    return sfb::fail(SFB_ERR_UNSUPPORTED, "EKF kernels support dof and ny up to 16");
  sfb_status st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  const size_t B = (size_t)batch, nn = (size_t)dof * dof, mn = (size_t)ny * dof, mm = (size_t)ny * ny;
  using S = sfb::Staging;
  S s;  // (the arrays of a half that is not asked for take no space; ekf_common refuses what the caller left out of the other)
  double *dP, *dA, *dQ, *ddt, *dH, *dR, *dr, *ddelta;
  int32_t *dinfo;
  s.add(&dP, B * nn, S::InOut, P);
  s.add_opt(&dA, predict ? B * nn : 0, S::In, A); s.add_opt(&dQ, predict ? (q_shared ? nn : B * nn) : 0, S::In, Q);
  s.add_opt(&ddt, predict ? (dt_shared ? 1 : B) : 0, S::In, dt);
  s.add_opt(&dH, update ? B * mn : 0, S::In, H); s.add_opt(&dR, update ? (r_shared ? mm : B * mm) : 0, S::In, R);
  s.add_opt(&dr, update ? B * ny : 0, S::In, r); s.add_opt(&ddelta, update ? B * dof : 0, S::Out, delta);
  s.add_opt(&dinfo, update ? B : 0, S::Out, info);
  return sfb::staged_call(s, "sfb_ekf_step_batch_host", [&] {
    return ekf_common(batch, dof, ny, dA, dQ, q_shared, ddt, dt_shared, dH, dR, r_shared, dr, dP, ddelta, dinfo, predict, update, nullptr);
  });
}

}  // extern "C"
