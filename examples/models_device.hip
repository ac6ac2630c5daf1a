// Example / test harness of the device-side fronts (compiled by hipcc into libsfb_models_dev.so): the vehicle safety
// filter of examples/mpc_asif_vehicle.cpp for a swarm, assembled AND solved on the GPU (ASIFSwarmDevice), and the vehicle
// MPC swarm linearised on the GPU (MPCSwarmDeviceLin).
#include <cstdint>
#include <cstdio>
#include <vector>

#include <chrono>
#include <random>

#include <smooth_feedback_amd/asif_device.hpp>
#include <smooth_feedback_amd/ekf_device.hpp>
#include <smooth_feedback_amd/mpc_device.hpp>
#include <smooth_feedback_amd/multi_device.hpp>
#include <smooth_feedback_amd/ocp_flatten_device.hpp>
#include <smooth_feedback_amd/pid_device.hpp>

#include "flat_ocp_harness.h"
#include "lie_eval.h"
#include "rigid_body_model.h"
#include "vehicle_model.h"

using namespace smooth_feedback_amd;
using sfbx::U2;
using sfbx::X6;

namespace {
// the swarm of sfbx_mpc_swarm_step (models.cpp): agent b at time 0.025 (b mod 400), its state off the desired one
template<class X>
X perturbed(const X & x0, uint64_t seed)
{
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> d(-0.5, 0.5);
  typename X::Tangent xi{};
  for (auto & v : xi) v = d(rng);
  return rplus(x0, xi);
}

// the host MPC object of a model: the vehicles, or the rigid body on SE3 x R^6 (rigid_body_model.h, variant 13)
template<class MPCT, class Model>
MPCT make_mpc(int K, double tf)
{
  if constexpr (std::is_same_v<Model, sfbx::RigidBodyModel>) return sfbx::make_rigid_body_mpc(K, tf);
  else return sfbx::make_vehicle_mpc<MPCT, Model>(K, tf);
}

// `ticks` closed-loop ticks of the swarm of sfbx_mpc_swarm_step through any swarm type with MPCSwarmDeviceLin's step()
template<class Model, class Swarm>
void devlin_loop(Swarm & swarm, const Model & mdl, int64_t batch, uint64_t seed, int ticks, double * u0, int32_t * codes, uint32_t * iters,
                 double * seconds)
{
  using X = decltype(std::declval<const Model &>().xdes(0.0));
  using U = decltype(std::declval<const Model &>().udes(0.0));
  std::vector<double> t((size_t)batch);
  std::vector<X> xs((size_t)batch);
  for (int64_t b = 0; b < batch; ++b) {
    t[b]  = 0.025 * double(b % 400);
    xs[b] = perturbed(mdl.xdes(t[b]), seed + (uint64_t)b);
  }
  std::vector<U> us;
  std::vector<QPSolutionStatus> cs;
  for (int k = 0; k < ticks; ++k) {
    if (k > 0)
      for (int64_t b = 0; b < batch; ++b) {  // crude closed loop, as in models.cpp
        auto f = mdl.f(xs[b], us[b]);
        for (auto & v : f) v *= 0.025;
        xs[b] = rplus(xs[b], f);
        t[b] += 0.025;
      }
    const auto t0 = std::chrono::steady_clock::now();
    swarm.step(t, xs, us, cs);
    if (seconds) seconds[k] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  for (int64_t b = 0; b < batch; ++b) {
    for (int i = 0; i < U::Dof; ++i) u0[U::Dof * b + i] = us[b].v[i];
    codes[b] = (int32_t)cs[b];
    iters[b] = swarm.iterations()[b];
  }
}

template<class MPCT, class Model>
int devlin_step(int K, double tf, int64_t batch, uint64_t seed, int ticks, int probe_empty, double * u0, int32_t * codes, uint32_t * iters,
                double * records, int64_t * record_doubles, int32_t * packed, double * seconds)
{
  const Model mdl{};
  auto mpc = make_mpc<MPCT, Model>(K, tf);
  MPCSwarmDeviceLin<MPCT, Model> swarm(mpc, mdl, batch, 0.0, probe_empty != 0);
  devlin_loop(swarm, mdl, batch, seed, ticks, u0, codes, iters, seconds);
  if (record_doubles) *record_doubles = swarm.record_doubles();
  if (packed) *packed = swarm.packed_records() ? 1 : 0;
  if (records) swarm.copy_records(records);
  return 0;
}

template<class MPCT, class Model>
int devlin_step_multi(int K, double tf, int64_t batch, uint64_t seed, int ticks, const int * devices, int ndev, int thread_per_shard, double * u0,
                      int32_t * codes, uint32_t * iters, double * seconds)
{
  const Model mdl{};
  auto mpc = make_mpc<MPCT, Model>(K, tf);
  MPCSwarmMultiDeviceLin<MPCT, Model> swarm(mpc, mdl, batch, std::vector<int>(devices, devices + ndev));
  swarm.shards().thread_per_shard(thread_per_shard != 0);
  devlin_loop(swarm, mdl, batch, seed, ticks, u0, codes, iters, seconds);
  return 0;
}

// the same rounds through EKFSwarmMultiDevice (fused: 0 = predict + update, 1 = step())
template<EKFStepper Stp>
int ekf_swarm_multi(int64_t batch, int steps, int fused, double tau, double dt, const int * devices, int ndev, int thread_per_shard,
                    const double * states, const double * P0, const double * y, double * states_out, double * P_out, int32_t * info)
{
  EKFSwarmMultiDevice<X6, sfbx::VehicleEkfDyn, sfbx::VehicleEkfMeas, 3, Stp> swarm(sfbx::VehicleEkfDyn{}, sfbx::VehicleEkfMeas{}, batch,
                                                                                  std::vector<int>(devices, devices + ndev));
  swarm.shards().thread_per_shard(thread_per_shard != 0);
  std::vector<X6> g((size_t)batch);
  std::vector<Mat<6, 6>> P((size_t)batch);
  for (int64_t b = 0; b < batch; ++b) {
    g[b] = sfbx::vehicle_state(states + 7 * b);
    std::copy(P0 + 36 * b, P0 + 36 * (b + 1), P[b].a.begin());
  }
  swarm.reset(g, P);
  const auto Q = sfbx::vehicle_ekf_Q();
  const auto R = sfbx::vehicle_ekf_R();
  std::vector<Vec<3>> ys((size_t)batch);
  for (int k = 0; k < steps; ++k) {
    for (int64_t b = 0; b < batch; ++b) ys[b] = {y[((size_t)k * batch + b) * 3], y[((size_t)k * batch + b) * 3 + 1], y[((size_t)k * batch + b) * 3 + 2]};
    if (fused) {
      swarm.step(Q, tau, ys, R);
    } else {
      swarm.predict(Q, tau, dt > 0 ? std::optional<double>(dt) : std::nullopt);
      swarm.update(ys, R);
    }
  }
  g = swarm.estimates();
  P = swarm.covariances();
  const auto inf = swarm.update_info();
  for (int64_t b = 0; b < batch; ++b) {
    sfbx::vehicle_state_out(g[b], states_out + 7 * b);
    std::copy(P[b].a.begin(), P[b].a.end(), P_out + 36 * b);
    info[b] = inf[b];
  }
  return 0;
}

template<EKFStepper Stp>
int ekf_swarm(int64_t batch, int steps, int fused, double tau, double dt, const double * states, const double * P0, const double * y,
              double * states_out, double * P_out, int32_t * info, double * seconds)
{
  EKFSwarmDevice<X6, sfbx::VehicleEkfDyn, sfbx::VehicleEkfMeas, 3, Stp> swarm(sfbx::VehicleEkfDyn{}, sfbx::VehicleEkfMeas{}, batch);
  std::vector<X6> g((size_t)batch);
  std::vector<Mat<6, 6>> P((size_t)batch);
  for (int64_t b = 0; b < batch; ++b) {
    g[b] = sfbx::vehicle_state(states + 7 * b);
    std::copy(P0 + 36 * b, P0 + 36 * (b + 1), P[b].a.begin());
  }
  swarm.reset(g, P);
  swarm.one_launch(fused != 2);  // fused: 1 = step() in one launch, 2 = step() as separate launches, 3 = 1 with resident measurements
  double * dy = nullptr;
  if (fused == 3) {
    if (hipMalloc(reinterpret_cast<void **>(&dy), (size_t)steps * batch * 24) != hipSuccess) return -3;
    (void)hipMemcpy(dy, y, (size_t)steps * batch * 24, hipMemcpyHostToDevice);
  }
  const auto Q = sfbx::vehicle_ekf_Q();
  const auto R = sfbx::vehicle_ekf_R();
  std::vector<Vec<3>> ys((size_t)batch);
  for (int k = 0; k < steps; ++k) {
    for (int64_t b = 0; b < batch; ++b) ys[b] = {y[((size_t)k * batch + b) * 3], y[((size_t)k * batch + b) * 3 + 1], y[((size_t)k * batch + b) * 3 + 2]};
    const auto t0 = std::chrono::steady_clock::now();
    if (fused == 3) {  // measurements already on the device: copied device-to-device into the swarm's buffer
      (void)hipMemcpy(swarm.device_measurements(), dy + (size_t)k * batch * 3, (size_t)batch * 24, hipMemcpyDeviceToDevice);
      swarm.step_resident(Q, tau, R);
    } else if (fused) {
      swarm.step(Q, tau, ys, R);
    } else {
      swarm.predict(Q, tau, dt > 0 ? std::optional<double>(dt) : std::nullopt);
      swarm.update(ys, R);
    }
    (void)hipDeviceSynchronize();
    if (seconds) seconds[k] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  if (dy) (void)hipFree(dy);
  g = swarm.estimates();
  P = swarm.covariances();
  const auto inf = swarm.update_info();
  for (int64_t b = 0; b < batch; ++b) {
    sfbx::vehicle_state_out(g[b], states_out + 7 * b);
    std::copy(P[b].a.begin(), P[b].a.end(), P_out + 36 * b);
    info[b] = inf[b];
  }
  return 0;
}

// the pose filter of rigid_body_model.h (G = SE3) through EKFSwarmDevice: the rounds of ekf_swarm, fused as there
template<EKFStepper Stp>
int pose_ekf_swarm(int64_t batch, int steps, int fused, double tau, double dt, const double * states, const double * P0, const double * y,
                   double * states_out, double * P_out, int32_t * info)
{
  EKFSwarmDevice<SE3, sfbx::PoseEkfDyn, sfbx::PoseEkfMeas, 3, Stp> swarm(sfbx::PoseEkfDyn{}, sfbx::PoseEkfMeas{}, batch);
  std::vector<SE3> g((size_t)batch);
  std::vector<Mat<6, 6>> P((size_t)batch);
  for (int64_t b = 0; b < batch; ++b) {
    g[b] = sfbx::pose_state(states + 7 * b);
    std::copy(P0 + 36 * b, P0 + 36 * (b + 1), P[b].a.begin());
  }
  swarm.reset(g, P);
  swarm.one_launch(fused != 2);
  double * dy = nullptr;
  if (fused == 3) {
    if (hipMalloc(reinterpret_cast<void **>(&dy), (size_t)steps * batch * 24) != hipSuccess) return -3;
    (void)hipMemcpy(dy, y, (size_t)steps * batch * 24, hipMemcpyHostToDevice);
  }
  const auto Q = sfbx::pose_ekf_Q();
  const auto R = sfbx::pose_ekf_R();
  std::vector<Vec<3>> ys((size_t)batch);
  for (int k = 0; k < steps; ++k) {
    for (int64_t b = 0; b < batch; ++b) ys[b] = {y[((size_t)k * batch + b) * 3], y[((size_t)k * batch + b) * 3 + 1], y[((size_t)k * batch + b) * 3 + 2]};
    if (fused == 3) {
      (void)hipMemcpy(swarm.device_measurements(), dy + (size_t)k * batch * 3, (size_t)batch * 24, hipMemcpyDeviceToDevice);
      swarm.step_resident(Q, tau, R);
    } else if (fused) {
      swarm.step(Q, tau, ys, R);
    } else {
      swarm.predict(Q, tau, dt > 0 ? std::optional<double>(dt) : std::nullopt);
      swarm.update(ys, R);
    }
  }
  if (dy) (void)hipFree(dy);
  g = swarm.estimates();
  P = swarm.covariances();
  const auto inf = swarm.update_info();
  for (int64_t b = 0; b < batch; ++b) {
    sfbx::pose_state_out(g[b], states_out + 7 * b);
    std::copy(P[b].a.begin(), P[b].a.end(), P_out + 36 * b);
    info[b] = inf[b];
  }
  return 0;
}

// one thread per item through sfbx::lie_eval_item, the function sfbx_lie_eval (models.cpp) runs on the host
template<class G>
__global__ void __launch_bounds__(64) lie_eval_kernel(const int op, const int64_t count, const int win, const int wout, const double * __restrict__ in,
                                                      double * __restrict__ out)
{
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= count) return;
  sfbx::lie_eval_item<G>(op, in + b * win, out + b * wout);
}
}  // namespace

extern "C" {

/* A swarm of vehicle EKFs on the GPU (EKFSwarmDevice; model: vehicle_model.h VehicleEkfDyn / VehicleEkfMeas): `steps` times
 * predict(Q, tau, dt) + update(y[step], R) -- or the fused step() (fused != 0, Euler, one substep) -- from states [batch][7]
 * and covariances P0 [batch][36]; y [steps][batch][3].  dt <= 0: the default single substep.  Out: states, covariances, the
 * last update's info, seconds[steps].  sfbx_ekf_swarm_host (models.h) does the same with one host EKF<> object per filter. */
int sfbx_ekf_swarm_device(int64_t batch, int steps, int rk4, int fused, double tau, double dt, const double * states, const double * P0,
                          const double * y, double * states_out, double * P_out, int32_t * info, double * seconds)
{
  try {
    return rk4 ? ekf_swarm<EKFStepper::RK4>(batch, steps, fused, tau, dt, states, P0, y, states_out, P_out, info, seconds)
               : ekf_swarm<EKFStepper::Euler>(batch, steps, fused, tau, dt, states, P0, y, states_out, P_out, info, seconds);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_ekf_swarm_device: %s\n", e.what());
    return -2;
  }
}

/* sfbx_ekf_swarm_device for the pose filter on SE3 (rigid_body_model.h: PoseEkfDyn / PoseEkfMeas): states [batch][7] =
 * (px, py, pz, w, x, y, z), P0 [batch][36], y [steps][batch][3].  sfbx_pose_ekf_swarm_host (models.cpp) is its host twin. */
int sfbx_pose_ekf_swarm_device(int64_t batch, int steps, int rk4, int fused, double tau, double dt, const double * states, const double * P0,
                               const double * y, double * states_out, double * P_out, int32_t * info)
{
  try {
    return rk4 ? pose_ekf_swarm<EKFStepper::RK4>(batch, steps, fused, tau, dt, states, P0, y, states_out, P_out, info)
               : pose_ekf_swarm<EKFStepper::Euler>(batch, steps, fused, tau, dt, states, P0, y, states_out, P_out, info);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_pose_ekf_swarm_device: %s\n", e.what());
    return -2;
  }
}

/* sfbx_ekf_swarm_device through EKFSwarmMultiDevice (multi_device.hpp): the filters sharded over `devices` (an ordinal may repeat),
 * one resident swarm per shard.  thread_per_shard != 0: a host thread per shard even on one device (test hook). */
int sfbx_ekf_swarm_device_multi(int64_t batch, int steps, int rk4, int fused, double tau, double dt, const int * devices, int ndev,
                                int thread_per_shard, const double * states, const double * P0, const double * y, double * states_out,
                                double * P_out, int32_t * info)
{
  try {
    return rk4 ? ekf_swarm_multi<EKFStepper::RK4>(batch, steps, fused, tau, dt, devices, ndev, thread_per_shard, states, P0, y, states_out, P_out, info)
               : ekf_swarm_multi<EKFStepper::Euler>(batch, steps, fused, tau, dt, devices, ndev, thread_per_shard, states, P0, y, states_out, P_out,
                                                    info);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_ekf_swarm_device_multi: %s\n", e.what());
    return -2;
  }
}

/* sfbx_mpc_swarm_devlin_step through MPCSwarmMultiDeviceLin (multi_device.hpp): the agents sharded over `devices`. */
int sfbx_mpc_swarm_devlin_step_multi(int variant, int K, double tf, int64_t batch, uint64_t seed, int ticks, const int * devices, int ndev,
                                     int thread_per_shard, double * u0, int32_t * codes, uint32_t * iters, double * seconds)
{
  try {
    if (variant == 6)
      return devlin_step_multi<sfbx::MPC6, sfbx::VehicleModel6>(K, tf, batch, seed, ticks, devices, ndev, thread_per_shard, u0, codes, iters, seconds);
    if (variant == 12)
      return devlin_step_multi<sfbx::MPC12, sfbx::VehicleModel12>(K, tf, batch, seed, ticks, devices, ndev, thread_per_shard, u0, codes, iters, seconds);
    if (variant == 13)
      return devlin_step_multi<sfbx::MPC12B, sfbx::RigidBodyModel>(K, tf, batch, seed, ticks, devices, ndev, thread_per_shard, u0, codes, iters, seconds);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_mpc_swarm_devlin_step_multi: %s\n", e.what());
    return -2;
  }
  return -1;
}

/* examples/mpc_asif_vehicle.cpp:151-175 for a swarm, both controllers on the GPU: per 25 ms tick the MPC input of every vehicle
 * (MPCSwarmDeviceLin, K_mpc), filtered by the ASI filter (ASIFSwarmDevice, K_asif), then one runge_kutta4 step of the
 * closed loop.  Vehicle 0 starts at the identity like the example, the others off it by xi ~ U(-0.3, 0.3)^6 (mt19937_64(seed + b)).
 * Out per tick: positions xy [ticks][batch][2], u_mpc / u_asif [ticks][batch][2], the number of non-Optimal MPC / ASIF
 * solves, the smallest barrier value h(x) over the swarm, seconds [ticks][2] (MPC, ASIF). */
static int vehicle_swarm_sim_impl(int64_t batch, int K_mpc, int K_asif, int ticks, uint64_t seed, double * xy, double * u_mpc, double * u_asif,
                                  int32_t * mpc_bad, int32_t * asif_bad, double * hmin, double * seconds, const bool reduced_kkt)
{
  try {
    auto fprm        = sfbx::vehicle_asif_params(K_asif);
    fprm.reduced_kkt = reduced_kkt;
    const sfbx::VehicleModel6 mdl{};
    auto mpc = sfbx::make_vehicle_mpc<sfbx::MPC6, sfbx::VehicleModel6>(K_mpc, 5.0);
    MPCSwarmDeviceLin<sfbx::MPC6, sfbx::VehicleModel6> ctrl(mpc, mdl, batch);
    ASIFSwarmDevice<X6, U2, sfbx::VehicleDyn6, sfbx::VehicleH, sfbx::VehicleBU> filt(sfbx::VehicleDyn6{}, sfbx::VehicleH{}, sfbx::VehicleBU{},
                                                                                    (size_t)batch, fprm);
    std::vector<X6> x((size_t)batch);
    for (int64_t b = 1; b < batch; ++b) {
      std::mt19937_64 rng(seed + (uint64_t)b);
      std::uniform_real_distribution<double> d(-0.3, 0.3);
      X6::Tangent xi{};
      for (auto & v : xi) v = d(rng);
      x[b] = rplus(X6::Identity(), xi);
    }
    std::vector<double> t((size_t)batch, 0.0);
    std::vector<U2> um, ua;
    std::vector<QPSolutionStatus> cs;
    const double dt = 0.025;
    for (int k = 0; k < ticks; ++k) {
      auto t0 = std::chrono::steady_clock::now();
      ctrl.step(t, x, um, cs);
      auto t1 = std::chrono::steady_clock::now();
      ua = filt(x, um);
      auto t2 = std::chrono::steady_clock::now();
      seconds[2 * k]     = std::chrono::duration<double>(t1 - t0).count();
      seconds[2 * k + 1] = std::chrono::duration<double>(t2 - t1).count();
      mpc_bad[k] = asif_bad[k] = 0;
      hmin[k]    = 1e300;
      for (int64_t b = 0; b < batch; ++b) {
        mpc_bad[k] += cs[b] != QPSolutionStatus::Optimal;
        asif_bad[k] += filt.codes()[b] != 0;
        double * o = xy + ((size_t)k * batch + b) * 2;
        o[0] = x[b].part<0>().x; o[1] = x[b].part<0>().y;
        double * pm = u_mpc + ((size_t)k * batch + b) * 2, *pa = u_asif + ((size_t)k * batch + b) * 2;
        pm[0] = um[b].v[0]; pm[1] = um[b].v[1]; pa[0] = ua[b].v[0]; pa[1] = ua[b].v[1];
        hmin[k] = std::min(hmin[k], sfbx::VehicleH{}(0.0, x[b])[0]);
        const U2 u = ua[b];
        auto f     = [&](double, const X6 & g) { return sfbx::VehicleDyn6{}(g, u); };
        x[b]       = detail::ekf_rk4_state(f, 0.0, dt, x[b], f(0.0, x[b]));  // runge_kutta4 on the group (:146-147)
        t[b] += dt;
      }
    }
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_vehicle_swarm_sim: %s\n", e.what());
    return -2;
  }
}
int sfbx_vehicle_swarm_sim(int64_t batch, int K_mpc, int K_asif, int ticks, uint64_t seed, double * xy, double * u_mpc, double * u_asif,
                           int32_t * mpc_bad, int32_t * asif_bad, double * hmin, double * seconds)
{
  return vehicle_swarm_sim_impl(batch, K_mpc, K_asif, ticks, seed, xy, u_mpc, u_asif, mpc_bad, asif_bad, hmin, seconds, false);
}
/* ... with the filter's QPs on the reduced-KKT route for tall problems (ASIFilterParams::reduced_kkt) */
int sfbx_vehicle_swarm_sim_tall(int64_t batch, int K_mpc, int K_asif, int ticks, uint64_t seed, double * xy, double * u_mpc, double * u_asif,
                                int32_t * mpc_bad, int32_t * asif_bad, double * hmin, double * seconds)
{
  return vehicle_swarm_sim_impl(batch, K_mpc, K_asif, ticks, seed, xy, u_mpc, u_asif, mpc_bad, asif_bad, hmin, seconds, true);
}

/* sfbx_mpc_swarm_device_step (models.h) with the linearisation on the GPU as well (MPCSwarmDeviceLin): same agents, same
 * closed loop.  Also out: the records of the LAST tick as the device wrote them ([batch][*record_doubles], room for the
 * unpacked size; NULL to skip), whether they are packed, seconds[ticks].  probe_empty != 0: start from an empty packing
 * (every non-zero Jacobian entry is then a misfit -> the unpacked fallback runs). */
int sfbx_mpc_swarm_devlin_step(int variant, int K, double tf, int64_t batch, uint64_t seed, int ticks, int probe_empty, double * u0,
                               int32_t * codes, uint32_t * iters, double * records, int64_t * record_doubles, int32_t * packed,
                               double * seconds)
{
  try {
    if (variant == 6)
      return devlin_step<sfbx::MPC6, sfbx::VehicleModel6>(K, tf, batch, seed, ticks, probe_empty, u0, codes, iters, records, record_doubles,
                                                          packed, seconds);
    if (variant == 12)
      return devlin_step<sfbx::MPC12, sfbx::VehicleModel12>(K, tf, batch, seed, ticks, probe_empty, u0, codes, iters, records,
                                                            record_doubles, packed, seconds);
    if (variant == 13)
      return devlin_step<sfbx::MPC12B, sfbx::RigidBodyModel>(K, tf, batch, seed, ticks, probe_empty, u0, codes, iters, records,
                                                             record_doubles, packed, seconds);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_mpc_swarm_devlin_step: %s\n", e.what());
    return -2;
  }
  return -1;
}

/* Like sfbx_asif_swarm_step (models.h) from given states [batch][7] = (x, y, cos, sin, v0, v1, v2) and desired inputs
 * [batch][2]: `ticks` consecutive filter calls, the vehicles moved 25 ms along their filtered inputs in between.  Out for
 * the LAST tick: u [batch][2], codes, iters, the QPs (n = 3, m = K + 3), their primal / dual and the warm start used;
 * seconds[ticks]: wall time of every filter call. */
static int asif_swarm_device_step_impl(int64_t batch, int K, int ticks, const double * states, const double * udes, double * u_out,
                                       int32_t * codes, uint32_t * iters, double * P, double * q, double * A, double * l, double * u,
                                       double * x, double * y, double * wx, double * wy, double * seconds, const bool reduced_kkt)
{
  try {
    auto fprm        = sfbx::vehicle_asif_params(K);
    fprm.reduced_kkt = reduced_kkt;
    ASIFSwarmDevice<X6, U2, sfbx::VehicleDyn6, sfbx::VehicleH, sfbx::VehicleBU> swarm(sfbx::VehicleDyn6{}, sfbx::VehicleH{}, sfbx::VehicleBU{},
                                                                                     (size_t)batch, fprm);
    std::vector<X6> g((size_t)batch);
    std::vector<U2> ud((size_t)batch);
    for (int64_t b = 0; b < batch; ++b) {
      const double * s = states + 7 * b;
      g[b].part<0>()   = SE2{s[0], s[1], s[2], s[3]};
      g[b].part<1>().v = {s[4], s[5], s[6]};
      ud[b].v          = {udes[2 * b], udes[2 * b + 1]};
    }
    std::vector<U2> out;
    for (int tick = 0; tick < ticks; ++tick) {
      if (tick > 0) {
        for (int64_t b = 0; b < batch; ++b) {
          auto dx = sfbx::VehicleDyn6{}(g[b], out[b]);
          for (auto & v : dx) v *= 0.025;
          g[b] = rplus(g[b], dx);
        }
      }
      if (tick == ticks - 1) swarm.copy_warm_start(wx, wy);
      const auto t0 = std::chrono::steady_clock::now();
      out = swarm(g, ud);
      if (seconds) seconds[tick] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    for (int64_t b = 0; b < batch; ++b) { u_out[2 * b] = out[b].v[0]; u_out[2 * b + 1] = out[b].v[1]; }
    std::copy(swarm.codes().begin(), swarm.codes().end(), codes);
    std::copy(swarm.iterations().begin(), swarm.iterations().end(), iters);
    swarm.copy_problem(P, q, A, l, u, x, y);
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_asif_swarm_device_step: %s\n", e.what());
    return 1;
  }
}
int sfbx_asif_swarm_device_step(int64_t batch, int K, int ticks, const double * states, const double * udes, double * u_out,
                                int32_t * codes, uint32_t * iters, double * P, double * q, double * A, double * l, double * u,
                                double * x, double * y, double * wx, double * wy, double * seconds)
{
  return asif_swarm_device_step_impl(batch, K, ticks, states, udes, u_out, codes, iters, P, q, A, l, u, x, y, wx, wy, seconds, false);
}
/* ... with the QPs on the reduced-KKT route for tall problems (ASIFilterParams::reduced_kkt) */
int sfbx_asif_swarm_device_step_tall(int64_t batch, int K, int ticks, const double * states, const double * udes, double * u_out,
                                     int32_t * codes, uint32_t * iters, double * P, double * q, double * A, double * l, double * u,
                                     double * x, double * y, double * wx, double * wy, double * seconds)
{
  return asif_swarm_device_step_impl(batch, K, ticks, states, udes, u_out, codes, iters, P, q, A, l, u, x, y, wx, wy, seconds, true);
}

/* ASIFSwarmDevice on the rigid body (rigid_body_model.h): the agents of sfbx_test_asif_rigid_body (models.cpp), one filter call.
 * Out: u [batch][6], codes. */
int sfbx_asif_rigid_body_swarm_device(int64_t batch, double * u_out, int32_t * codes)
{
  try {
    ASIFSwarmDevice<sfbx::X12B, sfbx::U6, sfbx::RigidBodyDyn, sfbx::RigidBodyH, sfbx::RigidBodyBU> swarm(
      sfbx::RigidBodyDyn{}, sfbx::RigidBodyH{}, sfbx::RigidBodyBU{}, (size_t)batch, sfbx::rigid_body_asif_params(20));
    std::vector<sfbx::X12B> g((size_t)batch);
    std::vector<sfbx::U6> ud((size_t)batch, sfbx::rigid_body_asif_udes());
    for (int64_t b = 0; b < batch; ++b) g[b] = sfbx::rigid_body_asif_state(b);
    const auto out = swarm(g, ud);
    for (int64_t b = 0; b < batch; ++b)
      for (int i = 0; i < 6; ++i) u_out[6 * b + i] = out[b].v[i];
    std::copy(swarm.codes().begin(), swarm.codes().end(), codes);
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_asif_rigid_body_swarm_device: %s\n", e.what());
    return 1;
  }
}

/* sfbx_lie_eval (models.h) on the GPU: in [count][win] is copied to a plain device buffer, one thread per item runs the
 * item function of examples/lie_eval.h (the lie.hpp operations with the device maths library), out [count][wout] comes back. */
int sfbx_lie_eval_device(int group, int op, int64_t count, const double * in, double * out)
{
  int win = 0, wout = 0;
  if (count < 0 || !sfbx::lie_eval_widths(group, op, &win, &wout)) return -1;
  if (count == 0) return 0;
  const size_t nin = (size_t)count * win * sizeof(double), nout = (size_t)count * wout * sizeof(double);
  double *din = nullptr, *dout = nullptr;
  if (hipMalloc(reinterpret_cast<void **>(&din), nin) != hipSuccess) return -3;
  if (hipMalloc(reinterpret_cast<void **>(&dout), nout) != hipSuccess) { (void)hipFree(din); return -3; }
  hipError_t e = hipMemcpy(din, in, nin, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    sfbx::lie_dispatch_group(group, [&]<class G>() {
      hipLaunchKernelGGL((lie_eval_kernel<G>), dim3((unsigned)((count + 63) / 64)), dim3(64), 0, nullptr, op, count, win, wout, din, dout);
    });
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, nout, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  (void)hipFree(dout);
  if (e != hipSuccess) {
    std::fprintf(stderr, "sfbx_lie_eval_device: %s\n", hipGetErrorString(e));
    return -2;
  }
  return 0;
}

}  // extern "C"

namespace {
// The trajectory functor of sfbx_pid_swarm_device: per agent a start pose g0 and a twist direction w (device arrays).
// kind 0: constant twist, what PIDConstantTwist (the family of sfb_pid_rollout_batch) returns; kind 1: the twist keeps its
// direction and changes its size, s(t) = 1 + 0.3 t:  g_des = rplus(g0, S(t) w), v_des = s(t) w, a_des = s'(t) w with
// S(t) = t + 0.15 t^2 -- dynamically consistent (pid.hpp:170-176), since twists of one direction commute.
struct PidSwarmTraj {
  const SE3 * g0;
  const double * w;  // [agents][6]
  const int32_t * kind;
  __host__ __device__ PIDDesired<SE3> operator()(int64_t agent, double t) const
  {
    SE3::Tangent wa{};
    for (int i = 0; i < 6; ++i) wa[i] = w[agent * 6 + i];
    if (kind[agent] == 0) return PIDConstantTwist<SE3>{g0[agent], wa}(t);
    const double s = 1.0 + 0.3 * t, S = t + 0.15 * t * t;
    PIDDesired<SE3> d;
    SE3::Tangent Sw{};
    for (int i = 0; i < 6; ++i) {
      Sw[i]  = S * wa[i];
      d.v[i] = s * wa[i];
      d.a[i] = 0.3 * wa[i];
    }
    d.g = rplus(g0[agent], Sw);
    return d;
  }
};
}  // namespace

extern "C" {

/* PIDSwarmDevice<SE3, functor> (pid_device.hpp): agents with states x [batch][7], v [batch][6], controllers' state ie
 * [batch][6] and t_last [batch], gains [batch][6], trajectory g0 [batch][7], w [batch][6], kind [batch] (0: constant twist,
 * 1: a twist of changing size).  steps > 0: rollout(t0, dt, steps); steps == 0: one step(t0).  u_max [6] nullable.
 * Out: x, v, ie, u [batch][...], cost [batch] (rollout only). */
int sfbx_pid_swarm_device(int64_t batch, double t0, double dt, int64_t steps, const double * x, const double * v, const double * ie,
                          const double * t_last, const double * kp, const double * kd, const double * ki, const double * g0, const double * w,
                          const int32_t * kind, double windup, const double * u_max, double * x_out, double * v_out, double * ie_out,
                          double * u_out, double * cost_out)
{
  if (batch < 1 || steps < 0) return -1;
  SE3 * dg0;
  double * dw;
  int32_t * dkind;
  int rc = 0;
  try {
    const size_t B = (size_t)batch;
    using T6       = SE3::Tangent;
    const auto tangents = [&](const double * p) {
      std::vector<T6> out(B);
      for (size_t b = 0; b < B; ++b)
        for (int i = 0; i < 6; ++i) out[b][i] = p[6 * b + i];
      return out;
    };
    const auto poses = [&](const double * p) {
      std::vector<SE3> out(B);
      for (size_t b = 0; b < B; ++b) out[b] = PIDFlat<SE3>::load(p + 7 * b);
      return out;
    };
    const std::vector<SE3> hg0 = poses(g0);
    detail::DeviceArena a;
    a.add(&dg0, B); a.add(&dw, B * 6); a.add(&dkind, B);
    const detail::DeviceBlock traj(a, "pid_device");
    detail::hip_check(detail::upload(dg0, hg0.data(), B), "pid_device", "hipMemcpy");
    detail::hip_check(detail::upload(dw, w, B * 6), "pid_device", "hipMemcpy");
    detail::hip_check(detail::upload(dkind, kind, B), "pid_device", "hipMemcpy");
    PIDSwarmDevice<SE3, PidSwarmTraj> swarm(PidSwarmTraj{dg0, dw, dkind}, batch, PIDParams{windup});
    swarm.set_state(poses(x), tangents(v));
    swarm.set_gains(tangents(kp), tangents(kd), tangents(ki));
    swarm.set_integral(tangents(ie), std::vector<double>(t_last, t_last + B));
    if (u_max) {
      T6 um{};
      for (int i = 0; i < 6; ++i) um[i] = u_max[i];
      swarm.set_u_max(um);
    }
    if (steps > 0) swarm.rollout(t0, dt, steps);
    else swarm.step(t0);
    const auto xs = swarm.states();
    const auto vs = swarm.velocities(), is = swarm.integrals(), us = swarm.inputs();
    const auto cs = swarm.costs();
    for (size_t b = 0; b < B; ++b) {
      PIDFlat<SE3>::store(xs[b], x_out + 7 * b);
      for (int i = 0; i < 6; ++i) {
        v_out[6 * b + i]  = vs[b][i];
        ie_out[6 * b + i] = is[b][i];
        u_out[6 * b + i]  = us[b][i];
      }
      cost_out[b] = steps > 0 ? cs[b] : 0.0;
    }
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_pid_swarm_device: %s\n", e.what());
    rc = -2;
  }
  return rc;
}

/* PIDSwarmDevice<SE3, SplineTrajectory<3, SE3>> (pid_device.hpp, spline.hpp): the swarm of sfbx_pid_swarm_device following
 * cubic splines -- tk [nknots], gk [nknots][7], V [nknots-1][3][6] per agent, or ONE of each with spline_shared != 0 -- at
 * t - ts0[agent] (ts0 [batch] nullable).  rollout(t0, dt, steps), steps >= 1.  Out as sfbx_pid_swarm_device. */
int sfbx_pid_swarm_spline_device(int64_t batch, double t0, double dt, int64_t steps, const double * x, const double * v, const double * ie,
                                 const double * t_last, const double * kp, const double * kd, const double * ki, int64_t nknots, const double * tk,
                                 const double * gk, const double * V, int spline_shared, const double * ts0, double windup, const double * u_max,
                                 double * x_out, double * v_out, double * ie_out, double * u_out, double * cost_out)
{
  if (batch < 1 || steps < 1 || nknots < 2) return -1;
  double *dtk, *dgk, *dV, *dts;
  int rc = 0;
  try {
    const size_t B = (size_t)batch, K = (size_t)nknots, Bs = spline_shared ? 1 : B;
    using T6       = SE3::Tangent;
    const auto tangents = [&](const double * p) {
      std::vector<T6> out(B);
      for (size_t b = 0; b < B; ++b)
        for (int i = 0; i < 6; ++i) out[b][i] = p[6 * b + i];
      return out;
    };
    const auto poses = [&](const double * p) {
      std::vector<SE3> out(B);
      for (size_t b = 0; b < B; ++b) out[b] = PIDFlat<SE3>::load(p + 7 * b);
      return out;
    };
    detail::DeviceArena a;
    a.add(&dtk, Bs * K); a.add(&dgk, Bs * K * 7); a.add(&dV, Bs * (K - 1) * 18); a.add(&dts, ts0 ? B : 0);
    const detail::DeviceBlock mem(a, "pid_device");
    detail::hip_check(detail::upload(dtk, tk, Bs * K), "pid_device", "hipMemcpy");
    detail::hip_check(detail::upload(dgk, gk, Bs * K * 7), "pid_device", "hipMemcpy");
    detail::hip_check(detail::upload(dV, V, Bs * (K - 1) * 18), "pid_device", "hipMemcpy");
    if (ts0) detail::hip_check(detail::upload(dts, ts0, B), "pid_device", "hipMemcpy");
    using Traj = SplineTrajectory<3, SE3>;
    PIDSwarmDevice<SE3, Traj> swarm(Traj{nknots - 1, dtk, dgk, dV, spline_shared != 0, ts0 ? dts : nullptr}, batch, PIDParams{windup});
    swarm.set_state(poses(x), tangents(v));
    swarm.set_gains(tangents(kp), tangents(kd), tangents(ki));
    swarm.set_integral(tangents(ie), std::vector<double>(t_last, t_last + B));
    if (u_max) {
      T6 um{};
      for (int i = 0; i < 6; ++i) um[i] = u_max[i];
      swarm.set_u_max(um);
    }
    swarm.rollout(t0, dt, steps);
    const auto xs = swarm.states();
    const auto vs = swarm.velocities(), is = swarm.integrals(), us = swarm.inputs();
    const auto cs = swarm.costs();
    for (size_t b = 0; b < B; ++b) {
      PIDFlat<SE3>::store(xs[b], x_out + 7 * b);
      for (int i = 0; i < 6; ++i) {
        v_out[6 * b + i]  = vs[b][i];
        ie_out[6 * b + i] = is[b][i];
        u_out[6 * b + i]  = us[b][i];
      }
      cost_out[b] = cs[b];
    }
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_pid_swarm_spline_device: %s\n", e.what());
    rc = -2;
  }
  return rc;
}

}  // extern "C"

// ---- flatten_ocp on the device (ocp_flatten_device.hpp; harness: flat_ocp_harness.h) ----
namespace {
template<class G>
__global__ void __launch_bounds__(64) flat_lie_kernel(const int op, const int64_t count, const double * __restrict__ in, double * __restrict__ out)
{
  constexpr int T   = G::Dof;
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  sfbx::flat_lie_item<G>(op, in + k * (op == 0 ? T : 2 * T), out + k * T * T);
}

void flat_ok(hipError_t e, const char * what) { detail::hip_check(e, "flat_ocp_device", what); }

// the ten node arrays of `agents` agents on N nodes in one block, and their sizes in the order of FlatNodeArrays
template<class Ocp>
struct FlatNodeBlock {
  using S = sfbx::FlatSizes<Ocp>;
  size_t len[10];
  FlatNodeArrays arr{};
  FlatNodeBlock(detail::DeviceArena & a, size_t B, size_t N)
  {
    const size_t l[10] = {B * N * S::Nx, B * N * S::Nx * S::nz, B * N * S::Nq, B * N * S::Nq * S::nz, B * N * S::Ncr, B * N * S::Ncr * S::nz,
                          B * S::Nce,    B * S::Nce * S::ne,    B,             B * S::ne};
    double ** slot[10] = {&arr.Ff, &arr.dFf, &arr.Fg, &arr.dFg, &arr.Fcr, &arr.dFcr, &arr.ce, &arr.dce, &arr.theta, &arr.dtheta};
    for (int k = 0; k < 10; ++k) len[k] = l[k], a.add(slot[k], l[k]);
  }
  void download(double * const * host) const
  {
    const double * dev[10] = {arr.Ff, arr.dFf, arr.Fg, arr.dFg, arr.Fcr, arr.dFcr, arr.ce, arr.dce, arr.theta, arr.dtheta};
    for (int k = 0; k < 10; ++k)
      if (host[k]) flat_ok(detail::download(host[k], dev[k], len[k]), "download node arrays");
  }
};
}  // namespace

extern "C" {

/* sfbx_flat_lie_eval (models.h) on the GPU: one thread per item runs the same item function. */
int sfbx_flat_lie_eval_device(int group, int op, int64_t count, const double * in, double * out)
{
  if (count < 0 || op < 0 || op > 1) return -1;
  try {
    const bool ok = sfbx::flat_lie_dispatch(group, [&]<class G>() {
      constexpr size_t T = G::Dof;
      if (count == 0) return;
      double *din, *dout;
      detail::DeviceArena a;
      a.add(&din, (size_t)count * (op == 0 ? T : 2 * T)); a.add(&dout, (size_t)count * T * T);
      const detail::DeviceBlock blk(a, "flat_ocp_device");
      flat_ok(detail::upload(din, in, (size_t)count * (op == 0 ? T : 2 * T)), "upload");
      hipLaunchKernelGGL((flat_lie_kernel<G>), detail::lane_grid(count), dim3(64), 0, nullptr, op, count, din, dout);
      flat_ok(hipGetLastError(), "flat_lie_kernel");
      flat_ok(hipDeviceSynchronize(), "synchronise");
      flat_ok(detail::download(out, dout, (size_t)count * T * T), "download");
    });
    return ok ? 0 : -1;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_flat_lie_eval_device: %s\n", e.what());
    return -2;
  }
}

/* sfbx_flat_ocp_nodes_host (models.h) on the GPU: flat_ocp_nodes_kernel alone over the nodes tau [N]; out arrays nullable. */
int sfbx_flat_ocp_nodes_device(int problem, int64_t agents, int32_t N, const double * tau, const double * x, const double * traj, double * Ff,
                               double * dFf, double * Fg, double * dFg, double * Fcr, double * dFcr, double * ce, double * dce, double * theta,
                               double * dtheta)
{
  if (agents < 1 || N < 1) return -1;
  try {
    const bool ok = sfbx::flat_dispatch_problem(problem, [&]<class Ocp>() {
      using S = sfbx::FlatSizes<Ocp>;
      const size_t B = (size_t)agents, n = (size_t)S::n(N);
      double *dtau, *dx, *dtraj;
      detail::DeviceArena a;
      a.add(&dtau, (size_t)N); a.add(&dx, B * n); a.add(&dtraj, B * S::stride);
      FlatNodeBlock<Ocp> nodes(a, B, (size_t)N);
      const detail::DeviceBlock blk(a, "flat_ocp_device");
      flat_ok(detail::upload(dtau, tau, (size_t)N), "upload tau");
      flat_ok(detail::upload(dx, x, B * n), "upload x");
      flat_ok(detail::upload(dtraj, traj, B * S::stride), "upload traj");
      const auto model = sfbx::flat_swarm_model<Ocp>(dtraj);
      flat_ok(flat_ocp_nodes_launch<Ocp>(model, agents, N, dtau, dx, nodes.arr, nullptr), "flat_ocp_nodes_kernel");
      flat_ok(hipDeviceSynchronize(), "synchronise");
      double * const host[10] = {Ff, dFf, Fg, dFg, Fcr, dFcr, ce, dce, theta, dtheta};
      nodes.download(host);
    });
    return ok ? 0 : -1;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_flat_ocp_nodes_device: %s\n", e.what());
    return -2;
  }
}

/* FlatOCPSwarmDevice on the mesh of sfbx_flat_ocp_nlp_host (models.h): eval() on the null stream -> g [agents][m], dg
 * [agents][nnz], f [agents], df [agents][1 + 2 nx + nq], and the front's node arrays (nodes [10] host pointers in the order of
 * FlatNodeArrays, each nullable).  side != 0: then once more on a non-blocking stream, behind a queue of large memsets and the
 * upload of x on that stream (x on the device is NaN until that upload lands) -> g2, dg2, f2, df2.  info [4]: free device
 * memory before and after a further eval(), the front's bytes, its n.  reps > 0: seconds [2] = the least time between device
 * events of the node kernel and of sfb_ocp_nlp_batch over reps warmed runs each. */
int sfbx_flat_ocp_front_device(int problem, int mesh_kind, int64_t agents, const double * x, const double * traj, int side, int reps, double * g,
                               double * dg, double * f, double * df, double * const * nodes, double * g2, double * dg2, double * f2, double * df2,
                               int64_t * info, double * seconds)
{
  if (agents < 1) return -1;
  try {
    const auto mesh = sfbx::flat_mesh(mesh_kind);
    const bool ok   = sfbx::flat_dispatch_problem(problem, [&]<class Ocp>() {
      using S     = sfbx::FlatSizes<Ocp>;
      using Model = sfbx::FlatSwarmModel<Ocp>;
      const size_t B = (size_t)agents;
      double * dtraj;
      detail::DeviceArena at;
      at.add(&dtraj, B * S::stride);
      const detail::DeviceBlock tblk(at, "flat_ocp_device");
      flat_ok(detail::upload(dtraj, traj, B * S::stride), "upload traj");
      FlatOCPSwarmDevice<Ocp, Model, sfbx::FlatMesh> front(Ocp{}, sfbx::flat_swarm_model<Ocp>(dtraj), mesh, agents);
      const size_t n = (size_t)front.n(), m = (size_t)front.m(), nnz = (size_t)front.nnz();
      double *dx, *dg_, *ddg, *df_, *ddf, *spin;
      const size_t spin_len = side ? (size_t)8 << 20 : 0;  // 64 MB
      detail::DeviceArena a;
      a.add(&dx, B * n); a.add(&dg_, B * m); a.add(&ddg, B * nnz); a.add(&df_, B); a.add(&ddf, B * S::ne); a.add(&spin, spin_len);
      const detail::DeviceBlock blk(a, "flat_ocp_device");
      flat_ok(detail::upload(dx, x, B * n), "upload x");
      front.eval(dx, dg_, ddg, df_, ddf, nullptr);
      flat_ok(hipDeviceSynchronize(), "synchronise");
      const auto fetch = [&](double * hg, double * hdg, double * hf, double * hdf) {
        if (hg) flat_ok(detail::download(hg, dg_, B * m), "download g");
        if (hdg) flat_ok(detail::download(hdg, ddg, B * nnz), "download dg");
        if (hf) flat_ok(detail::download(hf, df_, B), "download f");
        if (hdf) flat_ok(detail::download(hdf, ddf, B * S::ne), "download df");
      };
      fetch(g, dg, f, df);
      if (nodes) {
        const FlatNodeArrays & arr = front.node_arrays();
        const size_t N             = (size_t)front.N_colloc();
        const size_t len[8]    = {B * N * S::Nx, B * N * S::Nx * S::nz, B * N * S::Nq, B * N * S::Nq * S::nz, B * N * S::Ncr, B * N * S::Ncr * S::nz, B * S::Nce, B * S::Nce * S::ne};
        const double * dev[8]  = {arr.Ff, arr.dFf, arr.Fg, arr.dFg, arr.Fcr, arr.dFcr, arr.ce, arr.dce};
        for (int k = 0; k < 8; ++k)
          if (nodes[k]) flat_ok(detail::download(nodes[k], dev[k], len[k]), "download node arrays");
      }
      if (info) {
        size_t free0 = 0, free1 = 0, total = 0;
        flat_ok(hipMemGetInfo(&free0, &total), "hipMemGetInfo");
        front.eval(dx, dg_, ddg, df_, ddf, nullptr);
        flat_ok(hipDeviceSynchronize(), "synchronise");
        flat_ok(hipMemGetInfo(&free1, &total), "hipMemGetInfo");
        info[0] = (int64_t)free0, info[1] = (int64_t)free1, info[2] = (int64_t)front.device_bytes(), info[3] = (int64_t)n;
      }
      if (side) {
        hipStream_t st;
        flat_ok(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreateWithFlags");
        flat_ok(hipMemset(dx, 0xFF, B * n * sizeof(double)), "poison x");  // NaN until the upload below lands
        flat_ok(hipMemset(dg_, 0, B * m * sizeof(double)), "clear g");
        flat_ok(hipMemset(ddg, 0, B * nnz * sizeof(double)), "clear dg");
        flat_ok(hipMemset(df_, 0, B * sizeof(double)), "clear f");
        flat_ok(hipMemset(ddf, 0, B * S::ne * sizeof(double)), "clear df");
        flat_ok(hipDeviceSynchronize(), "synchronise");
        for (int k = 0; k < 8; ++k) flat_ok(hipMemsetAsync(spin, k, spin_len * sizeof(double), st), "hipMemsetAsync");
        flat_ok(hipMemcpyAsync(dx, x, B * n * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
        front.eval(dx, dg_, ddg, df_, ddf, st);
        flat_ok(hipStreamSynchronize(st), "hipStreamSynchronize");
        fetch(g2, dg2, f2, df2);
        flat_ok(hipStreamDestroy(st), "hipStreamDestroy");
      }
      if (reps > 0 && seconds) {
        hipEvent_t e0, e1;
        flat_ok(hipEventCreate(&e0), "event"); flat_ok(hipEventCreate(&e1), "event");
        float best[2] = {1e30f, 1e30f};
        for (int rep = 0; rep <= reps; ++rep)  // the first is the warm-up
          for (int half = 0; half < 2; ++half) {
            flat_ok(hipEventRecord(e0, nullptr), "record");
            if (half == 0) flat_ok(front.nodes(dx, df_, ddf, nullptr), "flat_ocp_nodes_kernel");
            else if (front.assemble(dx, dg_, ddg, nullptr) != SFB_OK) throw std::runtime_error(sfb_last_error());
            flat_ok(hipEventRecord(e1, nullptr), "record");
            flat_ok(hipEventSynchronize(e1), "synchronise");
            float ms = 0;
            flat_ok(hipEventElapsedTime(&ms, e0, e1), "elapsed");
            if (rep > 0 && ms < best[half]) best[half] = ms;
          }
        flat_ok(hipEventDestroy(e0), "event"); flat_ok(hipEventDestroy(e1), "event");
        seconds[0] = 1e-3 * best[0], seconds[1] = 1e-3 * best[1];
      }
    });
    return ok ? 0 : -1;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "sfbx_flat_ocp_front_device: %s\n", e.what());
    return -2;
  }
}

}  // extern "C"
