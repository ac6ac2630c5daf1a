// A swarm of Lie-group PID controllers that lives on the GPU (HIP only: include from a translation unit compiled by
// hipcc), for desired trajectories given as a device-callable functor.  The batched C-ABI (sfb_pid_step_batch,
// sfb_pid_rollout_batch) takes the desired triple as data -- arrays for a step, a constant body twist for a rollout; here
//   Traj: PIDDesired<G> operator()(int64_t agent, double t) const          __host__ __device__
// is evaluated per agent and tick inside the kernel.  States x, body velocities v, the controllers' state (i_err, t_last)
// and the gains stay resident; step(t) is PID::operator() (pid.hpp:74-87) for every agent, rollout(t0, dt, steps) the closed
// loop on d^r x = v, dv/dt = u in ONE launch.  One agent per lane, the per-lane arithmetic is pid_law / pid_rollout of
// pid.hpp -- the functions the host front and the kernels of libsfb.so call: a functor that returns what
// PIDConstantTwist<G> returns gives the bits sfb_pid_rollout_batch gives (G not a Bundle: the C-ABI sums a bundle's cost
// part by part).
#pragma once
#ifndef __HIPCC__
#error "pid_device.hpp needs hipcc"
#endif
#include <hip/hip_runtime.h>

#include <limits>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "detail/device_arena.hpp"
#include "pid.hpp"

namespace smooth_feedback_amd {

namespace detail {

template<class G>
struct PIDSwarmBuffers {
  G * x;
  double *v, *i_err, *t_last, *kp, *kd, *ki, *u, *cost;  // [B][Dof] each, t_last and cost [B]
};

template<int N>
__device__ inline Vec<N> pid_load_tangent(const double * __restrict__ p)
{
  Vec<N> t{};
#pragma unroll
  for (int i = 0; i < N; ++i) t[i] = p[i];
  return t;
}
template<int N>
__device__ inline void pid_store_tangent(const Vec<N> & t, double * __restrict__ p)
{
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = t[i];
}

template<class G, class Traj>
__global__ void __launch_bounds__(64) pid_swarm_step_kernel(const int64_t B, const Traj traj, const double t, const double windup,
                                                            const PIDSwarmBuffers<G> m)
{
  constexpr int N = G::Dof;
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const PIDDesired<G> d = traj(b, t);
  auto ie               = pid_load_tangent<N>(m.i_err + b * N);
  double tl             = m.t_last[b];
  typename G::Tangent e{};
  const auto u = pid_law<G>(t, m.x[b], pid_load_tangent<N>(m.v + b * N), d.g, d.v, d.a, pid_load_tangent<N>(m.kp + b * N),
                            pid_load_tangent<N>(m.kd + b * N), pid_load_tangent<N>(m.ki + b * N), windup, tl, ie, e);
  pid_store_tangent<N>(ie, m.i_err + b * N);
  pid_store_tangent<N>(u, m.u + b * N);
  m.t_last[b] = tl;
}

template<class G, class Traj>
__global__ void __launch_bounds__(64) pid_swarm_rollout_kernel(const int64_t B, const Traj traj, const double t0, const double dt, const int64_t steps,
                                                               const double windup, const bool clamp, const typename G::Tangent u_max,
                                                               const PIDSwarmBuffers<G> m)
{
  constexpr int N = G::Dof;
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  G x       = m.x[b];
  auto v    = pid_load_tangent<N>(m.v + b * N);
  auto ie   = pid_load_tangent<N>(m.i_err + b * N);
  double tl = m.t_last[b];
  typename G::Tangent ul{};
  const double cost = pid_rollout<G>([&](const double t) { return traj(b, t); }, t0, dt, steps, x, v, pid_load_tangent<N>(m.kp + b * N),
                                     pid_load_tangent<N>(m.kd + b * N), pid_load_tangent<N>(m.ki + b * N), windup, clamp, u_max, tl, ie, ul);
  m.x[b] = x;
  pid_store_tangent<N>(v, m.v + b * N);
  pid_store_tangent<N>(ie, m.i_err + b * N);
  pid_store_tangent<N>(ul, m.u + b * N);
  m.t_last[b] = tl;
  m.cost[b]   = cost;
}

}  // namespace detail

template<class G, class Traj>
class PIDSwarmDevice {
public:
  static constexpr int N = G::Dof;
  using Tangent          = typename G::Tangent;

  /// `agents` controllers at the identity and at rest, gains kp = kd = 1, ki = 0 (pid.hpp:50-53), integral unset
  PIDSwarmDevice(Traj traj, int64_t agents, const PIDParams & prm = PIDParams{}) : traj_(traj), B_(agents), prm_(prm)
  {
    if (B_ < 1) throw std::invalid_argument("PIDSwarmDevice: at least one agent");
    if (!(prm_.windup_limit >= 0.0)) throw std::invalid_argument("PIDSwarmDevice: windup_limit must be >= 0");
    const size_t B = (size_t)B_;
    detail::DeviceArena a;
    a.add(&m_.v, B * N); a.add(&m_.i_err, B * N); a.add(&m_.kp, B * N); a.add(&m_.kd, B * N); a.add(&m_.ki, B * N);
    a.add(&m_.u, B * N); a.add(&m_.t_last, B); a.add(&m_.cost, B); a.add(&m_.x, B);
    mem_ = detail::DeviceBlock(a, "pid_device");
    Tangent one{}, zero{};
    one.fill(1.0);
    set_state(std::vector<G>(B, G::Identity()), std::vector<Tangent>(B, zero));
    set_gains(one, one, zero);
    reset();
  }
  PIDSwarmDevice(const PIDSwarmDevice &)             = delete;
  PIDSwarmDevice & operator=(const PIDSwarmDevice &) = delete;

  int64_t size() const { return B_; }

  void set_state(const std::vector<G> & x, const std::vector<Tangent> & v)
  {
    need(x.size(), "state");
    need(v.size(), "velocity");
    check(detail::upload(m_.x, x.data(), (size_t)B_), "hipMemcpy(states)");
    up(m_.v, v);
  }
  /// gains per agent, or one set for the whole swarm (set_kp / set_kd / set_ki of every controller)
  void set_gains(const std::vector<Tangent> & kp, const std::vector<Tangent> & kd, const std::vector<Tangent> & ki)
  {
    up(m_.kp, kp);
    up(m_.kd, kd);
    up(m_.ki, ki);
  }
  void set_gains(const Tangent & kp, const Tangent & kd, const Tangent & ki)
  {
    set_gains(std::vector<Tangent>((size_t)B_, kp), std::vector<Tangent>((size_t)B_, kd), std::vector<Tangent>((size_t)B_, ki));
  }
  /// the controllers' state: integral (reset_integral of every controller with zeros) and time of the last call (NaN: unset)
  void set_integral(const std::vector<Tangent> & i_err, const std::vector<double> & t_last)
  {
    need(t_last.size(), "t_last");
    up(m_.i_err, i_err);
    check(detail::upload(m_.t_last, t_last.data(), (size_t)B_), "hipMemcpy(t_last)");
  }
  void reset_integral() { up(m_.i_err, std::vector<Tangent>((size_t)B_, Tangent{})); }
  /// fresh controllers: zero integral, no last call
  void reset() { set_integral(std::vector<Tangent>((size_t)B_, Tangent{}), std::vector<double>((size_t)B_, std::numeric_limits<double>::quiet_NaN())); }
  /// componentwise input clamp of rollout(); nullopt: none
  void set_u_max(const std::optional<Tangent> & u_max) { u_max_ = u_max; }

  /// PID::operator() at time t for every agent, on the resident states: writes inputs()
  void step(double t)
  {
    hipLaunchKernelGGL((detail::pid_swarm_step_kernel<G, Traj>), detail::lane_grid(B_), dim3(64), 0, nullptr, B_, traj_, t, prm_.windup_limit, m_);
    check(hipGetLastError(), "pid_swarm_step_kernel");
  }
  /// `steps` closed-loop ticks of length dt from t0 (tick k at t0 + k dt: law, clamp, double-integrator step) in one launch:
  /// updates the states, velocities and the controllers' state, writes inputs() (last tick) and costs()
  void rollout(double t0, double dt, int64_t steps)
  {
    if (steps < 0 || !(dt == dt) || dt - dt != 0.0) throw std::invalid_argument("PIDSwarmDevice: steps >= 0 and a finite dt");
    if (steps == 0) return;
    hipLaunchKernelGGL((detail::pid_swarm_rollout_kernel<G, Traj>), detail::lane_grid(B_), dim3(64), 0, nullptr, B_, traj_, t0, dt, steps, prm_.windup_limit,
                       u_max_.has_value(), u_max_.value_or(Tangent{}), m_);
    check(hipGetLastError(), "pid_swarm_rollout_kernel");
  }

  /// device -> host (synchronises with the launches above: null stream)
  std::vector<G> states() const
  {
    std::vector<G> out((size_t)B_);
    check(detail::download(out.data(), m_.x, (size_t)B_), "hipMemcpy(states)");
    return out;
  }
  std::vector<Tangent> velocities() const { return down(m_.v); }
  std::vector<Tangent> integrals() const { return down(m_.i_err); }
  std::vector<Tangent> inputs() const { return down(m_.u); }
  std::vector<double> costs() const
  {
    std::vector<double> out((size_t)B_);
    check(detail::download(out.data(), m_.cost, (size_t)B_), "hipMemcpy(costs)");
    return out;
  }
  /// resident buffers, for callers that produce states or consume inputs on the device
  G * device_states() { return m_.x; }
  double * device_velocities() { return m_.v; }
  double * device_inputs() { return m_.u; }

private:
  void need(size_t n, const char * what) const
  {
    if ((int64_t)n != B_) throw std::invalid_argument(std::string("PIDSwarmDevice: one ") + what + " per agent");
  }
  void up(double * dst, const std::vector<Tangent> & src)
  {
    need(src.size(), "tangent");
    static_assert(sizeof(Tangent) == N * sizeof(double));
    check(detail::upload(dst, src.data()->data(), (size_t)B_ * N), "hipMemcpy");
  }
  std::vector<Tangent> down(const double * src) const
  {
    std::vector<Tangent> out((size_t)B_);
    check(detail::download(out.data()->data(), src, (size_t)B_ * N), "hipMemcpy");
    return out;
  }
  static void check(hipError_t e, const char * what) { detail::hip_check(e, "pid_device", what); }

  Traj traj_;
  int64_t B_;
  PIDParams prm_;
  std::optional<Tangent> u_max_;
  detail::DeviceBlock mem_;
  detail::PIDSwarmBuffers<G> m_{};
};

}  // namespace smooth_feedback_amd
