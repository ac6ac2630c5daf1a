// Batched Lie-group splines (include/sfb.h: sfb_spline_fit_cubic_batch, sfb_spline_eval_batch,
// sfb_pid_rollout_spline_batch): one agent per lane, 64-lane blocks, cubic.
//
// As in pid.hip a bundle decouples exactly into its parts -- exp, log, Ad and ad of a product group act per part, and the
// fit's tridiagonal system is solved per tangent coordinate -- so the kernels loop over the parts (wave-uniform) and
// dispatch on the kind to a routine templated on the lie.hpp type; an RN part of run-time dof is a loop over Rn<1>.  The
// per-lane arithmetic is spline_fit_cubic_flat / spline_eval of include/smooth_feedback_amd/spline.hpp and pid_rollout of
// pid.hpp: the functions the host fronts and SplineTrajectory (for PIDSwarmDevice) call.  The fit's Thomas sweeps run in
// the agent's own V (no workspace).  Evaluation and rollout walk their times with a SplineSegment in registers: the
// segment's element and control differences are loaded again only when the segment index moves; with a shared spline and
// no ts0 that index is wave-uniform.  Plain loads and stores.
#include "spline_kernel.h"

#include "../../include/smooth_feedback_amd/spline.hpp"

namespace sfb {

namespace {

namespace L = smooth_feedback_amd;

template<int N>
__device__ inline L::Vec<N> load_tangent(const double *__restrict__ p)
{
  L::Vec<N> t{};
#pragma unroll
  for (int i = 0; i < N; ++i) t[i] = p[i];
  return t;
}
template<int N>
__device__ inline void store_tangent(const L::Vec<N> &t, double *__restrict__ p)
{
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = t[i];
}

// the part at element offset eo / tangent offset to of agent b's spline
template<class G>
__device__ inline L::SplineView<3, G> part_view(const SplineRef &c, const PidGroup &grp, const int64_t b, const int eo, const int to)
{
  const int64_t E = grp.elem, D = grp.dofs, sb = c.shared ? 0 : b;
  return L::SplineView<3, G>{c.S, c.tk + sb * (c.S + 1), c.gk + sb * (c.S + 1) * E + eo, c.V + sb * c.S * 3 * D + to, E, D};
}

template<class G>
__device__ inline void fit_part(const SplineFitArgs &a, const int64_t b, const int eo, const int to)
{
  const int64_t E = a.grp.elem, D = a.grp.dofs;
  L::spline_fit_cubic_flat<G>(a.S, a.tk + (a.tk_shared ? 0 : b) * (a.S + 1), a.gk + b * (a.S + 1) * E + eo, E, a.V + b * a.S * 3 * D + to, D);
}

template<class G>
__device__ inline void eval_part(const SplineEvalArgs &a, const int64_t b, const int eo, const int to)
{
  constexpr int N = G::Dof;
  const int64_t E = a.grp.elem, D = a.grp.dofs;
  const L::SplineView<3, G> view = part_view<G>(a.c, a.grp, b, eo, to);
  const double ts0               = a.c.ts0 ? a.c.ts0[b] : 0.0;
  const double *t                = a.t + (a.t_shared ? 0 : b) * a.nt;
  L::SplineSegment<3, G> seg;
  for (int64_t k = 0; k < a.nt; ++k) {
    G g;
    typename G::Tangent vel, acc;
    L::spline_eval<3, G>(view, t[k] - ts0, seg, g, vel, acc);
    const int64_t r = b * a.nt + k;
    L::PIDFlat<G>::store(g, a.g + r * E + eo);
    store_tangent<N>(vel, a.vel + r * D + to);
    store_tangent<N>(acc, a.acc + r * D + to);
  }
}

// one part of one agent, all ticks (rollout_part of pid.hip with the spline as the trajectory)
template<class G>
__device__ inline double rollout_part(const PidSplineArgs &s, const int64_t b, const int eo, const int to, const double t_last_in, double &t_last_out,
                                      const double cost)
{
  constexpr int N  = G::Dof;
  using Flat       = L::PIDFlat<G>;
  const PidArgs &a = s.p;
  const int64_t E = a.grp.elem, D = a.grp.dofs, gb = a.gains_shared ? 0 : b;
  G x    = Flat::load(a.x + b * E + eo);
  auto v = load_tangent<N>(a.v + b * D + to);
  const L::SplineView<3, G> view = part_view<G>(s.c, a.grp, b, eo, to);
  const double ts0               = s.c.ts0 ? s.c.ts0[b] : 0.0;
  L::SplineSegment<3, G> seg;
  const auto traj = [&](const double t) {
    L::PIDDesired<G> d;
    L::spline_eval<3, G>(view, t - ts0, seg, d.g, d.v, d.a);
    return d;
  };
  const auto kp = load_tangent<N>(a.kp + gb * D + to), kd = load_tangent<N>(a.kd + gb * D + to), ki = load_tangent<N>(a.ki + gb * D + to);
  auto ie       = load_tangent<N>(a.i_err + b * D + to);
  typename G::Tangent umax{}, ul{};
  if (a.u_max) umax = load_tangent<N>(a.u_max + to);
  double tl      = t_last_in;
  const double c = L::pid_rollout<G>(traj, a.t, a.dt, a.steps, x, v, kp, kd, ki, a.windup_limit, a.u_max != nullptr, umax, tl, ie, ul, cost);
  Flat::store(x, a.x + b * E + eo);
  store_tangent<N>(v, a.v + b * D + to);
  store_tangent<N>(ie, a.i_err + b * D + to);
  store_tangent<N>(ul, a.u + b * D + to);
  t_last_out = tl;
  return c;
}

__global__ void __launch_bounds__(64) spline_fit_kernel(const SplineFitArgs a)
{
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.batch) return;
  int eo = 0, to = 0;
  for (int p = 0; p < a.grp.nparts; ++p) {
    const int dof = a.grp.dof[p];
    switch (a.grp.kind[p]) {
    case SFB_LIE_SE2: fit_part<L::SE2>(a, b, eo, to); eo += 4; break;
    case SFB_LIE_SO3: fit_part<L::SO3>(a, b, eo, to); eo += 4; break;
    case SFB_LIE_SE3: fit_part<L::SE3>(a, b, eo, to); eo += 7; break;
    default:
      for (int i = 0; i < dof; ++i) fit_part<L::Rn<1>>(a, b, eo + i, to + i);
      eo += dof;
      break;
    }
    to += dof;
  }
}

__global__ void __launch_bounds__(64) spline_eval_kernel(const SplineEvalArgs a)
{
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.batch) return;
  int eo = 0, to = 0;
  for (int p = 0; p < a.grp.nparts; ++p) {
    const int dof = a.grp.dof[p];
    switch (a.grp.kind[p]) {
    case SFB_LIE_SE2: eval_part<L::SE2>(a, b, eo, to); eo += 4; break;
    case SFB_LIE_SO3: eval_part<L::SO3>(a, b, eo, to); eo += 4; break;
    case SFB_LIE_SE3: eval_part<L::SE3>(a, b, eo, to); eo += 7; break;
    default:
      for (int i = 0; i < dof; ++i) eval_part<L::Rn<1>>(a, b, eo + i, to + i);
      eo += dof;
      break;
    }
    to += dof;
  }
}

__global__ void __launch_bounds__(64) pid_rollout_spline_kernel(const PidSplineArgs s)
{
  const PidArgs &a = s.p;
  const int64_t b  = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.batch) return;
  const double tl = a.t_last[b];
  double tl_out = tl, cost = 0.0;
  int eo = 0, to = 0;
  for (int p = 0; p < a.grp.nparts; ++p) {
    const int dof = a.grp.dof[p];
    switch (a.grp.kind[p]) {
    case SFB_LIE_SE2: cost = rollout_part<L::SE2>(s, b, eo, to, tl, tl_out, cost); eo += 4; break;
    case SFB_LIE_SO3: cost = rollout_part<L::SO3>(s, b, eo, to, tl, tl_out, cost); eo += 4; break;
    case SFB_LIE_SE3: cost = rollout_part<L::SE3>(s, b, eo, to, tl, tl_out, cost); eo += 7; break;
    default:
      for (int i = 0; i < dof; ++i) cost = rollout_part<L::Rn<1>>(s, b, eo + i, to + i, tl, tl_out, cost);
      eo += dof;
      break;
    }
    to += dof;
  }
  a.t_last[b] = tl_out;
  a.cost[b]   = cost;
}

template<class Args>
hipError_t launch(void (*kernel)(const Args), const Args &a, int64_t batch, hipStream_t stream)
{
  const int64_t blocks = (batch + 63) / 64;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t spline_fit_launch(const SplineFitArgs &a, hipStream_t stream) { return launch(spline_fit_kernel, a, a.batch, stream); }
hipError_t spline_eval_launch(const SplineEvalArgs &a, hipStream_t stream) { return launch(spline_eval_kernel, a, a.batch, stream); }
hipError_t pid_rollout_spline_launch(const PidSplineArgs &a, hipStream_t stream) { return launch(pid_rollout_spline_kernel, a, a.p.batch, stream); }

}  // namespace sfb
