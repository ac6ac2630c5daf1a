// Device harness of the re-linearisation passes (mpc_device.hpp: mpc_relinearise_kernel, MPCSwarmDeviceLin::step(.., passes)
// -> sfb_mpc_swarm_step_resident_flat), compiled by hipcc into libsfb_models_dev.so: the planar vehicle of vehicle_model.h.
// A translation unit of its own: the kernels of models_device.hip and collocation_device.hip are compiled as before.
#include <cstdint>
#include <cstdio>
#include <vector>

#include <smooth_feedback_amd/mpc_device.hpp>
#include <smooth_feedback_amd/multi_device.hpp>

#include "mpc_relin.h"

using namespace smooth_feedback_amd;

namespace {
using MPCT  = sfbx::MPC6;
using Model = sfbx::VehicleModel6;
using Swarm = MPCSwarmDeviceLin<MPCT, Model>;

void ok(hipError_t e, const char * what) { detail::hip_check(e, "mpc_relin harness", what); }

// prune: 0 = the swarm's own probe (probe_default), 1 = the mask of MPC::probe_relin, 2 = the whole pattern
MPCT make(int K, double tf, int prune)
{
  MPCT mpc = sfbx::make_relin_mpc<MPCT, Model>(K, tf, 0, prune != 2);
  if (prune == 1) {
    std::vector<uint8_t> keep;
    mpc.probe_relin(0.0, keep);
    mpc.analyze_solver(&keep);
  }
  return mpc;
}
}  // namespace

extern "C" {

/* `ticks` times MPCSwarmDeviceLin::step(t, xs, us, codes, passes) from the states xdes(t[b]) (+) dx0[b] (the same every tick; the
 * warm starts carry over).  Out, of the last tick: primal [B][n], code, iter [B], u0 [B][2], agent_max [B] of audit(), the flat
 * records of its last pass (flat_rec [B][record_doubles], nullable; passes >= 1) and the A it assembled (Ax [B][nnzA], nullable).
 * info [6]: free device memory before and after the last tick (ticks >= 2: nothing may be allocated by then), nnzA_kept and
 * nnzL_fallback of sfb_sparse_qp_plan_pruned_info, nnzA, packed_records().  seconds (nullable) [1]: the last tick between device events. */
int sfbx_mpc_relin_swarm(int K, double tf, int64_t B, const double * t, const double * dx0, int passes, int prune, int ticks, double * primal,
                         int32_t * code, uint32_t * iter, double * u0, double * agent_max, double * flat_rec, double * Ax, int64_t * info,
                         double * seconds)
{
  if (B < 1 || ticks < 1 || passes < 0) return -1;
  try {
    const Model mdl{};
    MPCT mpc = make(K, tf, prune);
    Swarm swarm(mpc, mdl, B);
    const std::vector<double> ts(t, t + B);
    const auto xs = sfbx::relin_states(mdl, B, t, dx0);
    std::vector<sfbx::U2> us;
    std::vector<QPSolutionStatus> cs;
    size_t free0 = 0, free1 = 0, total = 0;
    hipEvent_t e0, e1;
    ok(hipEventCreate(&e0), "event"); ok(hipEventCreate(&e1), "event");
    for (int k = 0; k < ticks; ++k) {
      if (k == ticks - 1) {
        ok(hipMemGetInfo(&free0, &total), "hipMemGetInfo");
        ok(hipEventRecord(e0, nullptr), "record");
      }
      swarm.step(ts, xs, us, cs, passes);
    }
    ok(hipEventRecord(e1, nullptr), "record");
    ok(hipEventSynchronize(e1), "synchronise");
    float ms = 0;
    ok(hipEventElapsedTime(&ms, e0, e1), "elapsed");
    ok(hipEventDestroy(e0), "event"); ok(hipEventDestroy(e1), "event");
    if (seconds) seconds[0] = 1e-3 * ms;
    ok(hipMemGetInfo(&free1, &total), "hipMemGetInfo");
    swarm.copy_solution(primal, code);
    for (int64_t b = 0; b < B; ++b) {
      iter[b]       = swarm.iterations()[(size_t)b];
      u0[2 * b]     = us[(size_t)b].v[0];
      u0[2 * b + 1] = us[(size_t)b].v[1];
      if ((int32_t)cs[(size_t)b] != code[b]) return -4;  // the codes step() returns are those of the plans the swarm holds
    }
    if (flat_rec && passes > 0) swarm.copy_flat_records(flat_rec);
    if (Ax) {
      const double * dAx = nullptr;
      sfb_check(sfb_mpc_swarm_debug_buffers(swarm.handle(), &dAx, nullptr, nullptr));
      ok(detail::download(Ax, dAx, (size_t)B * mpc.qp().A_val.size()), "download Ax");
    }
    if (info) {
      int64_t kept = 0, fallback = 0;
      sfb_check(sfb_sparse_qp_plan_pruned_info(mpc.solver().plan(), &kept, &fallback));
      info[0] = (int64_t)free0, info[1] = (int64_t)free1, info[2] = kept, info[3] = fallback, info[4] = (int64_t)mpc.qp().A_val.size();
      info[5] = swarm.packed_records() ? 1 : 0;
    }
    if (agent_max) {
      const auto r = swarm.audit(t);
      std::copy(r.agent_max.begin(), r.agent_max.end(), agent_max);
    }
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_mpc_relin_swarm: %s\n", e.what());
    return -2;
  }
}

/* One tick with `passes` passes through MPCSwarmMultiDeviceLin (multi_device.hpp), the agents sharded over `devices` (an ordinal
 * may repeat).  Out: u0 [B][2], code, iter [B]. */
int sfbx_mpc_relin_swarm_multi(int K, double tf, int64_t B, const double * t, const double * dx0, int passes, const int * devices, int ndev,
                               double * u0, int32_t * code, uint32_t * iter)
{
  if (B < 1 || passes < 0 || ndev < 1) return -1;
  try {
    const Model mdl{};
    MPCT mpc = make(K, tf, 0);
    MPCSwarmMultiDeviceLin<MPCT, Model> swarm(mpc, mdl, B, std::vector<int>(devices, devices + ndev));
    std::vector<sfbx::U2> us;
    std::vector<QPSolutionStatus> cs;
    swarm.step(std::vector<double>(t, t + B), sfbx::relin_states(mdl, B, t, dx0), us, cs, passes);
    for (int64_t b = 0; b < B; ++b) {
      u0[2 * b] = us[(size_t)b].v[0], u0[2 * b + 1] = us[(size_t)b].v[1];
      code[b] = (int32_t)cs[(size_t)b];
      iter[b] = swarm.iterations()[(size_t)b];
    }
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_mpc_relin_swarm_multi: %s\n", e.what());
    return -2;
  }
}

/* mpc_relinearise_kernel alone.  One tick of the swarm (so that it holds times, states and a solution), then -- plan_in [B][n] and
 * code_in [B] given -- the swarm's device solution is overwritten with them, and the kernel writes rec [B][record_doubles] on the null
 * stream.  plan_out [B][n] / code_out [B]: the plan the kernel read.  side != 0: the record buffer is filled with NaN and the kernel
 * runs once more on a non-blocking stream behind a queue of large memsets -> rec_side.  reps > 0: seconds [1] = the least time of the
 * kernel between device events over reps warmed runs.  Also the argument errors of sfb_mpc_swarm_step_resident_flat on the live swarm:
 * status [3] = its result for prm = NULL, du0 = NULL, code = NULL. */
int sfbx_mpc_relin_kernel(int K, double tf, int64_t B, const double * t, const double * dx0, const double * plan_in, const int32_t * code_in,
                          int side, int reps, double * plan_out, int32_t * code_out, double * rec, double * rec_side, int32_t * status,
                          double * seconds)
{
  if (B < 1) return -1;
  try {
    const Model mdl{};
    MPCT mpc = make(K, tf, 0);
    Swarm swarm(mpc, mdl, B);
    const std::vector<double> ts(t, t + B);
    const auto xs = sfbx::relin_states(mdl, B, t, dx0);
    std::vector<sfbx::U2> us;
    std::vector<QPSolutionStatus> cs;
    swarm.step(ts, xs, us, cs);
    const double * dprimal = nullptr;
    const int32_t * dcode  = nullptr;
    swarm.device_solution(&dprimal, &dcode);
    const size_t n = (size_t)mpc.qp().n, rd = (size_t)MPCT::record_doubles(mpc.N());
    if (plan_in) ok(detail::upload(const_cast<double *>(dprimal), plan_in, (size_t)B * n), "upload plan");
    if (code_in) ok(detail::upload(const_cast<int32_t *>(dcode), code_in, (size_t)B), "upload code");
    swarm.relinearise(nullptr);
    ok(hipDeviceSynchronize(), "synchronise");
    swarm.copy_flat_records(rec);
    swarm.copy_solution(plan_out, code_out);
    double * drec = nullptr;
    sfb_check(sfb_mpc_swarm_device_records(swarm.handle(), &drec, nullptr));
    if (side) {
      hipStream_t st;
      double * spin        = nullptr;
      const size_t spin_len = (size_t)8 << 20;  // 64 MB
      ok(hipMalloc(reinterpret_cast<void **>(&spin), spin_len * sizeof(double)), "hipMalloc");
      ok(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreateWithFlags");
      ok(hipMemset(drec, 0xFF, (size_t)B * rd * sizeof(double)), "poison records");
      ok(hipDeviceSynchronize(), "synchronise");
      for (int k = 0; k < 8; ++k) ok(hipMemsetAsync(spin, k, spin_len * sizeof(double), st), "hipMemsetAsync");
      swarm.relinearise(st);
      ok(hipStreamSynchronize(st), "hipStreamSynchronize");
      swarm.copy_flat_records(rec_side);
      ok(hipStreamDestroy(st), "hipStreamDestroy");
      ok(hipFree(spin), "hipFree");
    }
    if (reps > 0 && seconds) {
      hipEvent_t e0, e1;
      ok(hipEventCreate(&e0), "event"); ok(hipEventCreate(&e1), "event");
      float best = 1e30f;
      for (int rep = 0; rep <= reps; ++rep) {  // the first is the warm-up
        ok(hipEventRecord(e0, nullptr), "record");
        swarm.relinearise(nullptr);
        ok(hipEventRecord(e1, nullptr), "record");
        ok(hipEventSynchronize(e1), "synchronise");
        float ms = 0;
        ok(hipEventElapsedTime(&ms, e0, e1), "elapsed");
        if (rep > 0 && ms < best) best = ms;
      }
      ok(hipEventDestroy(e0), "event"); ok(hipEventDestroy(e1), "event");
      seconds[0] = 1e-3 * best;
    }
    if (status) {
      const sfb_qp_params c = mpc.solver().params().to_c();
      std::vector<double> du0((size_t)B * 2);
      std::vector<int32_t> cd((size_t)B);
      status[0] = (int32_t)sfb_mpc_swarm_step_resident_flat(swarm.handle(), nullptr, du0.data(), nullptr, cd.data(), nullptr, nullptr);
      status[1] = (int32_t)sfb_mpc_swarm_step_resident_flat(swarm.handle(), &c, nullptr, nullptr, cd.data(), nullptr, nullptr);
      status[2] = (int32_t)sfb_mpc_swarm_step_resident_flat(swarm.handle(), &c, du0.data(), nullptr, nullptr, nullptr, nullptr);
    }
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_mpc_relin_kernel: %s\n", e.what());
    return -2;
  }
}

}  // extern "C"
