// Batched Lie-group PID (include/sfb.h: sfb_pid_step_batch, sfb_pid_rollout_batch): one agent per lane, 64-lane blocks.
//
// The law, the input clamp and the double-integrator step are componentwise in the tangent, and rplus / rminus of a bundle
// act per part: a bundle decouples EXACTLY into its parts.  So the kernels loop over the parts (wave-uniform: the descriptor
// is a kernel argument) and dispatch on the kind to a routine templated on the lie.hpp type, which keeps its element,
// tangents, gains and integral in registers with compile-time sizes -- no per-lane array is indexed by a run-time value.
// An RN part of run-time dof is a loop over scalars (Rn<1>).  In the rollout a part runs all its ticks before the next
// part starts; the reference pose is recomputed from t_k each tick (PIDConstantTwist, pid.hpp).  The per-lane arithmetic
// is pid_law / pid_clamp_input / pid_double_integrator_step / pid_rollout of include/smooth_feedback_amd/pid.hpp, the
// functions the host front and the device swarm front call.  Plain loads and stores.
#include "pid_kernel.h"

#include "../../include/smooth_feedback_amd/pid.hpp"

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

// one part of one agent, one controller call; eo / to: the part's offset in the element / the tangent
template<class G>
__device__ inline void step_part(const PidArgs &a, const int64_t b, const int eo, const int to, const double t_last_in)
{
  constexpr int N = G::Dof;
  using Flat      = L::PIDFlat<G>;
  const int64_t E = a.grp.elem, D = a.grp.dofs;
  const int64_t db = a.des_shared ? 0 : b, gb = a.gains_shared ? 0 : b;
  const G x        = Flat::load(a.x + b * E + eo);
  const G gd       = Flat::load(a.g_des + db * E + eo);
  const auto v = load_tangent<N>(a.v + b * D + to), vd = load_tangent<N>(a.v_des + db * D + to), ad = load_tangent<N>(a.a_des + db * D + to);
  const auto kp = load_tangent<N>(a.kp + gb * D + to), kd = load_tangent<N>(a.kd + gb * D + to), ki = load_tangent<N>(a.ki + gb * D + to);
  auto ie       = load_tangent<N>(a.i_err + b * D + to);
  double tl     = t_last_in;
  typename G::Tangent e{};
  const auto u = L::pid_law<G>(a.t, x, v, gd, vd, ad, kp, kd, ki, a.windup_limit, tl, ie, e);
  store_tangent<N>(ie, a.i_err + b * D + to);
  store_tangent<N>(u, a.u + b * D + to);
}

// one part of one agent, all ticks; returns the cost so far plus this part's, t_last receives the last tick's time
template<class G>
__device__ inline double rollout_part(const PidArgs &a, const int64_t b, const int eo, const int to, const double t_last_in, double &t_last_out,
                                      const double cost)
{
  constexpr int N = G::Dof;
  using Flat      = L::PIDFlat<G>;
  const int64_t E = a.grp.elem, D = a.grp.dofs;
  const int64_t db = a.des_shared ? 0 : b, gb = a.gains_shared ? 0 : b;
  G x              = Flat::load(a.x + b * E + eo);
  auto v           = load_tangent<N>(a.v + b * D + to);
  const L::PIDConstantTwist<G> traj{Flat::load(a.g_des + db * E + eo), load_tangent<N>(a.v_des + db * D + to)};
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

__global__ void __launch_bounds__(64) pid_step_kernel(const PidArgs a)
{
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.batch) return;
  const double tl = a.t_last[b];
  int eo = 0, to = 0;
  for (int p = 0; p < a.grp.nparts; ++p) {
    const int dof = a.grp.dof[p];
    switch (a.grp.kind[p]) {
    case SFB_LIE_SE2: step_part<L::SE2>(a, b, eo, to, tl); eo += 4; break;
    case SFB_LIE_SO3: step_part<L::SO3>(a, b, eo, to, tl); eo += 4; break;
    case SFB_LIE_SE3: step_part<L::SE3>(a, b, eo, to, tl); eo += 7; break;
    default:
      for (int i = 0; i < dof; ++i) step_part<L::Rn<1>>(a, b, eo + i, to + i, tl);
      eo += dof;
      break;
    }
    to += dof;
  }
  a.t_last[b] = a.t;  // pid.hpp:84: always
}

__global__ void __launch_bounds__(64) pid_rollout_kernel(const PidArgs a)
{
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.batch) return;
  const double tl = a.t_last[b];
  double tl_out = tl, cost = 0.0;
  int eo = 0, to = 0;
  for (int p = 0; p < a.grp.nparts; ++p) {
    const int dof = a.grp.dof[p];
    switch (a.grp.kind[p]) {
    case SFB_LIE_SE2: cost = rollout_part<L::SE2>(a, b, eo, to, tl, tl_out, cost); eo += 4; break;
    case SFB_LIE_SO3: cost = rollout_part<L::SO3>(a, b, eo, to, tl, tl_out, cost); eo += 4; break;
    case SFB_LIE_SE3: cost = rollout_part<L::SE3>(a, b, eo, to, tl, tl_out, cost); eo += 7; break;
    default:
      for (int i = 0; i < dof; ++i) cost = rollout_part<L::Rn<1>>(a, b, eo + i, to + i, tl, tl_out, cost);
      eo += dof;
      break;
    }
    to += dof;
  }
  a.t_last[b] = tl_out;
  a.cost[b]   = cost;
}

hipError_t launch(void (*kernel)(const PidArgs), const PidArgs &a, hipStream_t stream)
{
  const int64_t blocks = (a.batch + 63) / 64;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

bool pid_group_from(const sfb_pid_group *g, PidGroup &out, const char **why)
{
  out = PidGroup{};
  if (!g || !g->part_kind || !g->part_dof) { *why = "group descriptor or its arrays are NULL"; return false; }
  if (g->nparts < 1 || g->nparts > SFB_PID_MAX_PARTS) { *why = "nparts outside 1 .. SFB_PID_MAX_PARTS"; return false; }
  out.nparts = g->nparts;
  for (int p = 0; p < g->nparts; ++p) {
    const int32_t kind = g->part_kind[p], dof = g->part_dof[p];
    int elem = 0;
    switch (kind) {
    case SFB_LIE_RN: elem = dof; if (dof < 1 || dof > 4096) { *why = "RN part: dof outside 1 .. 4096"; return false; } break;
    case SFB_LIE_SE2: elem = 4; if (dof != 3) { *why = "SE2 part: dof must be 3"; return false; } break;
    case SFB_LIE_SO3: elem = 4; if (dof != 3) { *why = "SO3 part: dof must be 3"; return false; } break;
    case SFB_LIE_SE3: elem = 7; if (dof != 6) { *why = "SE3 part: dof must be 6"; return false; } break;
    default: *why = "part kind outside sfb_lie_kind"; return false;
    }
    out.kind[p] = kind;
    out.dof[p]  = dof;
    out.elem += elem;
    out.dofs += dof;
  }
  return true;
}

hipError_t pid_step_launch(const PidArgs &a, hipStream_t stream) { return launch(pid_step_kernel, a, stream); }
hipError_t pid_rollout_launch(const PidArgs &a, hipStream_t stream) { return launch(pid_rollout_kernel, a, stream); }

}  // namespace sfb
