// Device-side harness of the collocation layer (part of libsfb_models_dev.so): the fused dynamics-error audit of
// include/smooth_feedback_amd/mesh_device.hpp on GIVEN plans, for the example MPC models.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include <smooth_feedback_amd/detail/device_arena.hpp>
#include <smooth_feedback_amd/mesh_device.hpp>
#include <smooth_feedback_amd/mpc_device.hpp>

#include "rigid_body_model.h"
#include "vehicle_model.h"

using namespace smooth_feedback_amd;

namespace {

template<class MPCT, class Model>
int audit(MPCT mpc, int64_t B, const double * t, const double * primal, const int32_t * code, double * errs, double * agent_max, double * ival_max,
          int32_t * skipped)
{
  const int nivals = mpc.mesh().N_ivals();
  const size_t n   = (size_t)MPCT::Nx * (mpc.N() + 1) + (size_t)MPCT::Nu * mpc.N();
  double *dt, *dp, *de, *da, *di;
  int32_t *dc, *ds;
  detail::DeviceArena a;
  a.add(&dt, (size_t)B); a.add(&dp, (size_t)B * n); a.add(&de, (size_t)B * nivals); a.add(&da, (size_t)B); a.add(&di, (size_t)nivals);
  a.add(&dc, (size_t)B); a.add(&ds, 1);
  detail::DeviceBlock blk(a, "sfbx_mpc_audit_device");
  const auto ok = [](hipError_t e, const char * what) { detail::hip_check(e, "sfbx_mpc_audit_device", what); };
  ok(detail::upload(dt, t, (size_t)B), "upload t");
  ok(detail::upload(dp, primal, (size_t)B * n), "upload primal");
  if (code) ok(detail::upload(dc, code, (size_t)B), "upload code");
  ok(mpc_dyn_error_device(mpc, Model{}, B, dt, dp, code ? dc : nullptr, de, da, di, ds, nullptr), "launch");
  ok(hipDeviceSynchronize(), "synchronise");
  ok(detail::download(errs, de, (size_t)B * nivals), "download errs");
  ok(detail::download(agent_max, da, (size_t)B), "download agent_max");
  ok(detail::download(ival_max, di, (size_t)nivals), "download ival_max");
  ok(detail::download(skipped, ds, 1), "download skipped");
  return 0;
}

template<class MPCT, class Model>
int tick_then_audit(int K, double tf, int64_t B, const double * t, const double * dx0, int do_audit, double target, double * primal, int32_t * code,
                    double * errs, double * agent_max, double * ival_max, int32_t * skipped, int32_t * refined_ivals, double * u_next, double * seconds)
{
  using X = decltype(std::declval<const Model &>().xdes(0.0));
  using U = decltype(std::declval<const Model &>().udes(0.0));
  const Model mdl{};
  MPCT mpc = [&] {
    if constexpr (std::is_same_v<Model, sfbx::RigidBodyModel>) return sfbx::make_rigid_body_mpc(K, tf);
    else return sfbx::make_vehicle_mpc<MPCT, Model>(K, tf);
  }();
  MPCSwarmDeviceLin<MPCT, Model> swarm(mpc, mdl, B);
  std::vector<double> ts(t, t + B);
  std::vector<X> xs((size_t)B);
  for (int64_t b = 0; b < B; ++b) {
    typename X::Tangent a{};
    for (int i = 0; i < X::Dof; ++i) a[i] = dx0[b * X::Dof + i];
    xs[(size_t)b] = rplus(mdl.xdes(t[b]), a);
  }
  std::vector<U> us;
  std::vector<QPSolutionStatus> cs;
  swarm.step(ts, xs, us, cs);
  swarm.copy_solution(primal, code);
  if (do_audit) {
    std::vector<double> all;
    const auto r = swarm.audit(t, &all);
    std::copy(all.begin(), all.end(), errs);
    std::copy(r.agent_max.begin(), r.agent_max.end(), agent_max);
    std::copy(r.ival_max.begin(), r.ival_max.end(), ival_max);
    *skipped       = r.skipped;
    *refined_ivals = (int32_t)swarm.refined_mesh(r.ival_max, target).N_ivals();
    if (seconds) {
      // the two launches alone, warmed, between device events (outputs in a block of their own; t is on the device already)
      const auto ok = [](hipError_t e, const char * what) { detail::hip_check(e, "sfbx_mpc_swarm_devlin_audit", what); };
      const int nivals = mpc.mesh().N_ivals();
      double *dt, *de, *da, *di;
      int32_t * ds;
      detail::DeviceArena a;
      a.add(&dt, (size_t)B); a.add(&de, (size_t)B * nivals); a.add(&da, (size_t)B); a.add(&di, (size_t)nivals); a.add(&ds, 1);
      detail::DeviceBlock blk(a, "sfbx_mpc_swarm_devlin_audit");
      ok(detail::upload(dt, t, (size_t)B), "upload t");
      const double * dprimal = nullptr;
      const int32_t * dcode  = nullptr;
      swarm.device_solution(&dprimal, &dcode);
      hipEvent_t e0, e1;
      ok(hipEventCreate(&e0), "event"); ok(hipEventCreate(&e1), "event");
      float best = 1e30f;
      for (int rep = 0; rep < 6; ++rep) {  // the first is the warm-up
        ok(hipEventRecord(e0, nullptr), "record");
        ok(mpc_dyn_error_device(mpc, mdl, B, dt, dprimal, dcode, de, da, di, ds, nullptr), "launch");
        ok(hipEventRecord(e1, nullptr), "record");
        ok(hipEventSynchronize(e1), "synchronise");
        float ms = 0;
        ok(hipEventElapsedTime(&ms, e0, e1), "elapsed");
        if (rep > 0 && ms < best) best = ms;
      }
      ok(hipEventDestroy(e0), "event"); ok(hipEventDestroy(e1), "event");
      seconds[2] = 1e-3 * best;
      // ... and the whole audit() call, warmed: upload of t, launches, summary download (8 bytes per agent)
      const auto t0 = std::chrono::steady_clock::now();
      (void)swarm.audit(t);
      seconds[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
  }
  const auto t0 = std::chrono::steady_clock::now();
  swarm.step(ts, xs, us, cs);  // the tick after: the same with and without an audit in between
  if (seconds) seconds[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (int64_t b = 0; b < B; ++b)
    for (int i = 0; i < U::Dof; ++i) u_next[b * U::Dof + i] = us[(size_t)b].v[i];
  return 0;
}

}  // namespace

extern "C" {

/* One tick of MPCSwarmDeviceLin from the states xdes(t[b]) (+) dx0[b], the solution it left (primal [agents][n], code), with
 * do_audit != 0 its audit() (errs [agents][nivals], agent_max, ival_max, skipped, and the interval count of
 * refined_mesh(ival_max, target)), then the same tick again: u_next [agents][Nu].  seconds (nullable) [3]: wall clock of that second
 * tick, wall clock of a second, warmed audit() call, and the least of five warmed runs of the audit's two launches between device events. */
int sfbx_mpc_swarm_devlin_audit(int variant, int K, double tf, int64_t agents, const double * t, const double * dx0, int do_audit, double target,
                                double * primal, int32_t * code, double * errs, double * agent_max, double * ival_max, int32_t * skipped,
                                int32_t * refined_ivals, double * u_next, double * seconds)
{
  try {
    if (variant == 6)
      return tick_then_audit<sfbx::MPC6, sfbx::VehicleModel6>(K, tf, agents, t, dx0, do_audit, target, primal, code, errs, agent_max, ival_max,
                                                               skipped, refined_ivals, u_next, seconds);
    if (variant == 12)
      return tick_then_audit<sfbx::MPC12, sfbx::VehicleModel12>(K, tf, agents, t, dx0, do_audit, target, primal, code, errs, agent_max, ival_max,
                                                                 skipped, refined_ivals, u_next, seconds);
    if (variant == 13)
      return tick_then_audit<sfbx::MPC12B, sfbx::RigidBodyModel>(K, tf, agents, t, dx0, do_audit, target, primal, code, errs, agent_max, ival_max,
                                                                  skipped, refined_ivals, u_next, seconds);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_mpc_swarm_devlin_audit: %s\n", e.what());
    return -2;
  }
  return -1;
}

/* mpc_dyn_error_device on GIVEN plans: variant 6 / 12 the vehicles, 13 the rigid body (-1 otherwise); t [agents], primal
 * [agents][n], code [agents] or NULL.  Out: errs [agents][ceil(K / 4)], agent_max [agents], ival_max [ceil(K / 4)], skipped [1]. */
int sfbx_mpc_audit_device(int variant, int K, double tf, int64_t agents, const double * t, const double * primal, const int32_t * code,
                          double * errs, double * agent_max, double * ival_max, int32_t * skipped)
{
  try {
    if (variant == 6)
      return audit<sfbx::MPC6, sfbx::VehicleModel6>(sfbx::make_vehicle_mpc<sfbx::MPC6, sfbx::VehicleModel6>(K, tf), agents, t, primal, code, errs,
                                                     agent_max, ival_max, skipped);
    if (variant == 12)
      return audit<sfbx::MPC12, sfbx::VehicleModel12>(sfbx::make_vehicle_mpc<sfbx::MPC12, sfbx::VehicleModel12>(K, tf), agents, t, primal, code,
                                                       errs, agent_max, ival_max, skipped);
    if (variant == 13)
      return audit<sfbx::MPC12B, sfbx::RigidBodyModel>(sfbx::make_rigid_body_mpc(K, tf), agents, t, primal, code, errs, agent_max, ival_max, skipped);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_mpc_audit_device: %s\n", e.what());
    return -2;
  }
  return -1;
}

}  // extern "C"
