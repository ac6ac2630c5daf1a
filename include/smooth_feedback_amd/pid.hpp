// Lie-group PID controller: mirrors smooth::feedback::PID (pid.hpp:37-204) for the system the reference designs it for,
//   d^r x_t = v,  dv/dt = u,   x in G, v and u in R^dim(G)                                        (pid.hpp:29-35)
//   u = a_des + kp o (g_des (-) x) + kd o (v_des - v) + ki o i_err                                 (pid.hpp:74-87)
// The control law is written ONCE, as a __host__ __device__ function on the groups of lie.hpp: the host front PID<T, G>
// below calls it for one controller on the CPU (one controller has nothing to send to a GPU: O(dim) arithmetic), the
// batched kernels of libsfb.so (csrc/pid.hip, sfb_pid_step_batch / sfb_pid_rollout_batch) and the device swarm front
// (pid_device.hpp) call it for one agent per GPU lane.  Next to it: the double-integrator step that closes the loop on
// that system, and the flat storage of a group element the C-ABI uses.  The Spline overloads of set_xdes (pid.hpp:142-159)
// take the Spline<K, G> of spline.hpp, which this header includes at its end.
#pragma once
#include <cmath>
#include <functional>
#include <limits>
#include <optional>
#include <tuple>
#include <utility>

#include "lie.hpp"
#include "time.hpp"

namespace smooth_feedback_amd {

template<int K, class G>
  requires(K >= 1 && K <= 5)
class Spline;  // spline.hpp

/// pid.hpp:17-21
struct PIDParams {
  /// Maximal absolute value for integral states
  double windup_limit = std::numeric_limits<double>::infinity();
};

/// what a desired trajectory returns at one time: position, body velocity, body acceleration (a plain struct: the
/// device-side twin of PID::TrajectoryReturnT)
template<class G>
struct PIDDesired {
  G g{};
  typename G::Tangent v{}, a{};
};

/// PID::operator() (pid.hpp:74-87) on plain values.  t_last is NaN while unset (first call); i_err and t_last are the
/// controller's state and are updated.  g_err receives g_des (-) x.  Returns u.
template<class G>
SFB_LIE_HD typename G::Tangent pid_law(double t, const G & x, const typename G::Tangent & v, const G & g_des, const typename G::Tangent & v_des,
                                       const typename G::Tangent & a_des, const typename G::Tangent & kp, const typename G::Tangent & kd,
                                       const typename G::Tangent & ki, double windup_limit, double & t_last, typename G::Tangent & i_err,
                                       typename G::Tangent & g_err)
{
  g_err = rminus(g_des, x);
  if (!(t_last != t_last) && t > t_last) {  // pid.hpp:79-83: integrate, then clamp (+inf: no clamp)
    const double h = t - t_last;
    for (int i = 0; i < G::Dof; ++i) {
      double e = i_err[i] + h * g_err[i];
      e        = (e < -windup_limit) ? -windup_limit : e;
      e        = (e > windup_limit) ? windup_limit : e;
      i_err[i] = e;
    }
  }
  t_last = t;
  typename G::Tangent u{};
  for (int i = 0; i < G::Dof; ++i) u[i] = a_des[i] + kp[i] * g_err[i] + kd[i] * (v_des[i] - v[i]) + ki[i] * i_err[i];
  return u;
}

/// u <- clamp(u, -u_max, u_max), componentwise
template<int N>
SFB_LIE_HD void pid_clamp_input(Vec<N> & u, const Vec<N> & u_max)
{
  for (int i = 0; i < N; ++i) {
    u[i] = (u[i] < -u_max[i]) ? -u_max[i] : u[i];
    u[i] = (u[i] > u_max[i]) ? u_max[i] : u[i];
  }
}

/// One step of length h of  d^r x = v, dv/dt = u  with u held.  Classical RK4 on Bundle<G, Rn<Dof>> has the stages
/// k1 = (v, u), k2 = k3 = (v + h/2 u, u), k4 = (v + h u, u) -- the right-hand side does not depend on x -- whose weighted
/// mean is (v + h/2 u, u): the step reduces exactly to this closed form, which is what is computed.
template<class G>
SFB_LIE_HD void pid_double_integrator_step(G & x, typename G::Tangent & v, const typename G::Tangent & u, double h)
{
  typename G::Tangent d{};
  const double h2 = 0.5 * h * h;
  for (int i = 0; i < G::Dof; ++i) d[i] = h * v[i] + h2 * u[i];
  x = rplus(x, d);
  for (int i = 0; i < G::Dof; ++i) v[i] = v[i] + h * u[i];
}

/// The trajectory family of the batched rollout (and of the reference's examples/pid_se2.cpp): constant body twist,
///   g_des(t) = rplus(g0, t v),  v_des = v,  a_des = 0  -- dynamically consistent, as pid.hpp:170-176 asks.
/// The pose is computed from t each time, not accumulated: its rounding does not depend on how many ticks came before.
template<class G>
struct PIDConstantTwist {
  G g0{};
  typename G::Tangent v{};
  SFB_LIE_HD PIDDesired<G> operator()(double t) const
  {
    typename G::Tangent tv{};
    for (int i = 0; i < G::Dof; ++i) tv[i] = t * v[i];
    return PIDDesired<G>{rplus(g0, tv), v, typename G::Tangent{}};
  }
};

/// `steps` closed-loop ticks of length dt from t0 on the double integrator: per tick k at t_k = t0 + k dt the law, the
/// optional input clamp (clamp != false: by u_max; a flag and a value, not a nullable pointer, so that u_max stays in
/// registers on the GPU), the step.  traj(t) -> PIDDesired<G>.  x, v, i_err, t_last are updated, u_last receives the last
/// tick's (clamped) input.  Returns cost + sum_k dt |g_err_k|^2, summed in tick order.
template<class G, class Traj>
SFB_LIE_HD double pid_rollout(const Traj & traj, double t0, double dt, int64_t steps, G & x, typename G::Tangent & v,
                              const typename G::Tangent & kp, const typename G::Tangent & kd, const typename G::Tangent & ki, double windup_limit,
                              bool clamp, const typename G::Tangent & u_max, double & t_last, typename G::Tangent & i_err, typename G::Tangent & u_last,
                              double cost = 0.0)
{
  for (int64_t k = 0; k < steps; ++k) {
    const double t         = t0 + (double)k * dt;
    const PIDDesired<G> d  = traj(t);
    typename G::Tangent e{};
    typename G::Tangent u = pid_law<G>(t, x, v, d.g, d.v, d.a, kp, kd, ki, windup_limit, t_last, i_err, e);
    if (clamp) pid_clamp_input<G::Dof>(u, u_max);
    pid_double_integrator_step<G>(x, v, u, dt);
    double e2 = 0.0;
    for (int i = 0; i < G::Dof; ++i) e2 += e[i] * e[i];
    cost += dt * e2;
    u_last = u;
  }
  return cost;
}

// ---- flat storage of an element, as the C-ABI (sfb_pid_*) lays it out: Rn N values; SE2 (x, y, c, s); SO3 (w, x, y, z);
// SE3 (p, w, x, y, z); a Bundle is its parts one after the other ----
template<class G>
struct PIDFlat;
template<int N>
struct PIDFlat<Rn<N>> {
  static constexpr int E = N;
  SFB_LIE_HD static Rn<N> load(const double * p)
  {
    Rn<N> g;
    for (int i = 0; i < N; ++i) g.v[i] = p[i];
    return g;
  }
  SFB_LIE_HD static void store(const Rn<N> & g, double * p)
  {
    for (int i = 0; i < N; ++i) p[i] = g.v[i];
  }
};
template<>
struct PIDFlat<SE2> {
  static constexpr int E = 4;
  SFB_LIE_HD static SE2 load(const double * p) { return SE2{p[0], p[1], p[2], p[3]}; }
  SFB_LIE_HD static void store(const SE2 & g, double * p) { p[0] = g.x; p[1] = g.y; p[2] = g.c; p[3] = g.s; }
};
template<>
struct PIDFlat<SO3> {
  static constexpr int E = 4;
  SFB_LIE_HD static SO3 load(const double * p) { return SO3{p[0], p[1], p[2], p[3]}; }
  SFB_LIE_HD static void store(const SO3 & g, double * p) { p[0] = g.w; p[1] = g.x; p[2] = g.y; p[3] = g.z; }
};
template<>
struct PIDFlat<SE3> {
  static constexpr int E = 7;
  SFB_LIE_HD static SE3 load(const double * p) { return SE3{{p[0], p[1], p[2]}, SO3{p[3], p[4], p[5], p[6]}}; }
  SFB_LIE_HD static void store(const SE3 & g, double * p)
  {
    p[0] = g.p[0]; p[1] = g.p[1]; p[2] = g.p[2]; p[3] = g.q.w; p[4] = g.q.x; p[5] = g.q.y; p[6] = g.q.z;
  }
};
template<class... Gs>
struct PIDFlat<Bundle<Gs...>> {
  static constexpr int E = (PIDFlat<Gs>::E + ...);
  SFB_LIE_HD static Bundle<Gs...> load(const double * p)
  {
    Bundle<Gs...> g;
    load_parts(g, p, std::index_sequence_for<Gs...>{});
    return g;
  }
  SFB_LIE_HD static void store(const Bundle<Gs...> & g, double * p) { store_parts(g, p, std::index_sequence_for<Gs...>{}); }

private:
  template<size_t... I>
  SFB_LIE_HD static void load_parts(Bundle<Gs...> & g, const double * p, std::index_sequence<I...>)
  {
    int off = 0;
    ((g.template part<I>() = PIDFlat<Gs>::load(p + off), off += PIDFlat<Gs>::E), ...);
  }
  template<size_t... I>
  SFB_LIE_HD static void store_parts(const Bundle<Gs...> & g, double * p, std::index_sequence<I...>)
  {
    int off = 0;
    ((PIDFlat<Gs>::store(g.template part<I>(), p + off), off += PIDFlat<Gs>::E), ...);
  }
};

/// Host front: smooth::feedback::PID<T, G> (pid.hpp:37-204).  Plain CPU arithmetic through pid_law.
template<Time T, class G>
  requires(G::Dof > 0)
class PID {
public:
  using Tangent = typename G::Tangent;
  /// Desired trajectory consists of position, velocity, and acceleration
  using TrajectoryReturnT = std::tuple<G, Tangent, Tangent>;

  /// proportional and derivative gains 1, integral gains 0 (pid.hpp:50-53)
  PID(const PIDParams & prm = PIDParams{}) noexcept : prm_(prm)
  {
    kp_.fill(1.0);
    kd_.fill(1.0);
    ki_.fill(0.0);
  }

  /// pid.hpp:74-87
  Tangent operator()(const T & t, const G & x, const Tangent & v)
  {
    const auto [g_des, v_des, a_des] = x_des_(t);
    // the law sees seconds since the last call: (t - t_last) - 0 is the reference's time_trait<T>::minus(t, t_last)
    double t_last   = t_last_ ? 0.0 : std::numeric_limits<double>::quiet_NaN();
    const double tt = t_last_ ? time_trait<T>::minus(t, *t_last_) : 0.0;
    Tangent g_err{};
    const Tangent u = pid_law<G>(tt, x, v, g_des, v_des, a_des, kp_, kd_, ki_, prm_.windup_limit, t_last, i_err_, g_err);
    t_last_ = t;
    return u;
  }

  void set_kp(double kp) { kp_.fill(kp); }
  void set_kp(const Tangent & kp) { kp_ = kp; }
  void set_kd(double kd) { kd_.fill(kd); }
  void set_kd(const Tangent & kd) { kd_ = kd; }
  void set_ki(double ki) { ki_.fill(ki); }
  void set_ki(const Tangent & ki) { ki_ = ki; }

  /// pid.hpp:134
  void reset_integral() { i_err_.fill(0.0); }

  /// pid.hpp:142-159: track a spline whose time 0 is t0 -- the desired triple at t is the spline at
  /// time_trait<T>::minus(t, t0) (held pose at rest outside its knots)
  template<int K>
  void set_xdes(T t0, const Spline<K, G> & c)
  {
    set_xdes(t0, Spline<K, G>(c));
  }
  template<int K>
  void set_xdes(T t0, Spline<K, G> && c)
  {
    x_des_ = [t0 = std::move(t0), c = std::move(c)](T t) -> TrajectoryReturnT {
      Tangent vel{}, acc{};
      G g = c(time_trait<T>::minus(t, t0), vel, acc);
      return TrajectoryReturnT(std::move(g), std::move(vel), std::move(acc));
    };
  }

  /// pid.hpp:177-186
  void set_xdes(const std::function<TrajectoryReturnT(T)> & f)
  {
    auto f_copy = f;
    set_xdes(std::move(f_copy));
  }
  void set_xdes(std::function<TrajectoryReturnT(T)> && f) { x_des_ = std::move(f); }

  /// the controller's state, for callers that move it to or from the batched entry points
  const Tangent & integral() const { return i_err_; }
  const Tangent & kp() const { return kp_; }
  const Tangent & kd() const { return kd_; }
  const Tangent & ki() const { return ki_; }

private:
  PIDParams prm_;
  Tangent kd_{}, kp_{}, ki_{};
  std::optional<T> t_last_;
  Tangent i_err_{};
  std::function<TrajectoryReturnT(T)> x_des_ = [](T) -> TrajectoryReturnT { return TrajectoryReturnT(G::Identity(), Tangent{}, Tangent{}); };
};

}  // namespace smooth_feedback_amd

#include "spline.hpp"
