// Fused dynamics-error audit of MPC plans on the GPU (HIP only: include from a translation unit compiled by hipcc).
// For a swarm whose plans already lie in device memory, one launch tells how well every plan -- a solution of the
// dynamics LINEARISED around the desired trajectory -- obeys the true dynamics: MPC::dyn_error (mpc.hpp; reference
// collocation/dyn_error.hpp:28-73 on the flattened dynamics of ocp_flatten.hpp:166-177) per (agent, mesh interval),
// without the plan leaving the device.  Only the summaries need to come back: one error per agent, one per interval.
//
// Mapping: one lane per (agent, interval, audit point).  An interval of Kmesh points is audited at the Kmesh + 2 points
// of the degree-raised interval; these sit in a slot of W lanes, W the next power of two (Kmesh = 4: 6 points in a slot
// of 8, eight intervals to a wave).  Every lane resamples the interval's node values of dx / du to its own point
// (weights chosen by compile-time unrolled selects from the kernel arguments: no table in memory, no run-time indexed
// array), forms xl (+) e, ul (+) v and evaluates flat_dynamics there; the slot then exchanges F and X_0 with cross-lane
// moves, every lane j >= 1 integrates to its own point with its column of the integration matrix, and the maxima are
// taken across the slot.  No LDS, no scratch; every loop over vector or matrix entries is unrolled.  A second, tiny
// launch reduces errs to the per-agent and per-interval maxima.
//
// Model: as for mpc_device.hpp (xdes, dxdes, udes, f -- `__host__ __device__`).
#pragma once
#ifndef __HIPCC__
#error "mesh_device.hpp needs hipcc"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dyn_error.hpp"
#include "mesh.hpp"
#include "mpc.hpp"

namespace smooth_feedback_amd {

namespace detail {

/// the per-degree tables of one audit, by value in the kernel arguments ([-1, 1] scale)
template<int K>
struct AuditTables {
  double tau[K + 2];           // raised points, the end point +1 included
  double Wc[K + 2][K + 1];     // resampling weights from the K + 1 points of a closed interval
  double Wo[K + 2][K];         // ... from the K collocation points alone (inputs, last interval)
  double I[K + 1][K + 1];      // I[j][i] = integration matrix entry (i, j) of the raised interval
};

template<int K>
inline AuditTables<K> make_audit_tables()
{
  AuditTables<K> t{};
  const MeshMat wc = resample_weights(K, true), wo = resample_weights(K, false);
  const LgrTable & up = lgr_table(K + 1);
  for (int j = 0; j < K + 2; ++j) {
    t.tau[j] = up.tau[(std::size_t)j];
    for (int i = 0; i <= K; ++i) t.Wc[j][i] = wc(j, i);
    for (int i = 0; i < K; ++i) t.Wo[j][i] = wo(j, i);
  }
  for (int j = 0; j <= K; ++j)
    for (int i = 0; i <= K; ++i) t.I[j][i] = up.Ius(i, j);
  return t;
}

constexpr int audit_slot(int points)
{
  int w = 1;
  while (w < points) w *= 2;
  return w;
}

template<class X, class U, int K, class Model>
__global__ void __launch_bounds__(64) mpc_audit_kernel(const int64_t B, const int nivals, const double tf, const Model model, const AuditTables<K> tab,
                                                       const double * __restrict__ t, const double * __restrict__ primal,
                                                       double * __restrict__ errs)
{
  constexpr int Nx = X::Dof, Nu = U::Dof, Ke = K + 1, W = audit_slot(K + 2);
  static_assert(W <= 64, "an interval's audit points fit a wave");
  const int64_t gid  = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t pair = gid / W;  // (agent, interval)
  const int p        = (int)(gid - pair * W);
  const bool live    = pair < B * nivals;
  const int64_t b    = live ? pair / nivals : 0;  // (lanes without work run along on agent 0: the cross-lane moves need them)
  const int s        = live ? (int)(pair - b * nivals) : 0;
  const bool closed  = s + 1 < nivals;
  const int N        = nivals * K;
  const int64_t n    = (int64_t)Nx * (N + 1) + (int64_t)Nu * N;
  const double * dx  = primal + b * n + (int64_t)s * K * Nx;
  const double * du  = primal + b * n + (int64_t)Nx * (N + 1) + (int64_t)s * K * Nu;

  // this lane's point: weights, node, integration column -- selected with compile-time indices
  double wx[K + 1], wu[K + 1], icol[Ke], taup = 0.0;
#pragma unroll
  for (int i = 0; i <= K; ++i) wx[i] = wu[i] = 0.0;
#pragma unroll
  for (int i = 0; i < Ke; ++i) icol[i] = 0.0;
#pragma unroll
  for (int q = 0; q < K + 2; ++q) {
    if (p == q || (q == K + 1 && p > q)) {
      taup = tab.tau[q];
#pragma unroll
      for (int i = 0; i <= K; ++i) {
        wx[i] = tab.Wc[q][i];
        wu[i] = closed ? tab.Wc[q][i] : (i < K ? tab.Wo[q][i < K ? i : 0] : 0.0);
      }
    }
    if (q >= 1 && (p == q || (q == 1 && p == 0) || (q == K + 1 && p > q))) {
#pragma unroll
      for (int i = 0; i < Ke; ++i) icol[i] = tab.I[q - 1][i];
    }
  }

  // resample the plan to this point
  Vec<Nx> e{};
  Vec<Nu> v{};
#pragma unroll
  for (int i = 0; i <= K; ++i) {
#pragma unroll
    for (int d = 0; d < Nx; ++d) e[d] += wx[i] * dx[i * Nx + d];
    if (i < K || closed) {
#pragma unroll
      for (int d = 0; d < Nu; ++d) v[d] += wu[i] * du[i * Nu + d];
    }
  }

  // the true dynamics of the deviation at this point
  const double half = 0.5 / (double)nivals;
  const double ti   = t[b] + tf * ((double)s / (double)nivals + half * (taup + 1.0));
  const Vec<Nx> F   = flat_dynamics(model.f, model.xdes(ti), model.dxdes(ti), model.udes(ti), e, v);

  // integrate through the interval to this lane's point j = p, compare
  const double h = tf * half;
  double e2 = 0.0, x2 = 0.0;
#pragma unroll
  for (int d = 0; d < Nx; ++d) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < Ke; ++i) acc += __shfl(F[d], i, W) * icol[i];
    const double x0 = __shfl(e[d], 0, W);
    const double r  = (x0 + h * acc) - e[d];
    e2 += r * r;
    x2 += e[d] * e[d];
  }
  bool bad = e2 != e2 || x2 != x2;
  if (!(live && p >= 1 && p <= Ke)) e2 = x2 = 0.0, bad = false;
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) {
    const double oe = __shfl_xor(e2, off, W), ox = __shfl_xor(x2, off, W);
    const int ob    = __shfl_xor((int)bad, off, W);
    e2  = oe > e2 ? oe : e2;
    x2  = ox > x2 ? ox : x2;
    bad = bad || ob;
  }
  if (live && p == 0) errs[pair] = dyn_error_combine(e2, x2, bad);
}

/// blocks 0 .. nivals - 1: ival_max[s] over the agents whose plan the swarm keeps (code Optimal, MaxTime or MaxIterations:
/// mpc.hpp:510-516) and whose errs row has no NaN; block nivals: agent_max[b] (NaN if the row has one) and the number of
/// agents left out of ival_max.
template<int Threads = 256>
__global__ void __launch_bounds__(Threads) mpc_audit_reduce_kernel(const int64_t B, const int nivals, const int32_t * __restrict__ code,
                                                               const double * __restrict__ errs, double * __restrict__ agent_max,
                                                               double * __restrict__ ival_max, int32_t * __restrict__ skipped)
{
  __shared__ double smax[Threads];
  __shared__ int scount[Threads];
  const int s = blockIdx.x;
  double mx   = 0.0;
  int count   = 0;
  for (int64_t b = threadIdx.x; b < B; b += Threads) {
    const double * row = errs + b * nivals;
    double am = 0.0;
    bool nan  = false;
    for (int k = 0; k < nivals; ++k) {
      const double ev = row[k];
      nan = nan || ev != ev;
      am  = ev > am ? ev : am;
    }
    const int32_t c = code ? code[b] : 0;
    const bool keep = !nan && (c == 0 || c == 4 || c == 5);  // QPSolutionStatus::Optimal, MaxIterations, MaxTime
    if (s == nivals) {
      agent_max[b] = nan ? NAN : am;
      count += keep ? 0 : 1;
    } else if (keep) {
      const double ev = row[s];
      mx = ev > mx ? ev : mx;
    }
  }
  smax[threadIdx.x]   = mx;
  scount[threadIdx.x] = count;
  __syncthreads();
  for (int off = Threads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      smax[threadIdx.x] = smax[threadIdx.x + off] > smax[threadIdx.x] ? smax[threadIdx.x + off] : smax[threadIdx.x];
      scount[threadIdx.x] += scount[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (s == nivals) *skipped = scount[0];
    else ival_max[s] = smax[0];
  }
}

}  // namespace detail

/// Audit B plans in device memory.  `proto`: the host MPC object the plans belong to (mesh, horizon); `model`: its
/// device-callable twin.  d_t [B] tick times, d_primal [B][n] plans ([dx_0 .. dx_N | du_0 .. du_{N-1}]), d_code [B]
/// solver status per agent (NULL: all kept).  Out, all device pointers: d_errs [B][nivals]; d_agent_max [B] the largest
/// interval error of each agent (NaN for a plan with a NaN: it stays in that agent's row); d_ival_max [nivals] the
/// largest error per interval over the agents whose plan a swarm keeps (status Optimal, MaxTime, MaxIterations) and
/// that have no NaN; d_skipped [1] how many agents that leaves out.  Two launches on `stream`, asynchronous.
template<class MPCT, class Model>
hipError_t mpc_dyn_error_device(const MPCT & proto, const Model & model, const int64_t B, const double * d_t, const double * d_primal,
                                const int32_t * d_code, double * d_errs, double * d_agent_max, double * d_ival_max, int32_t * d_skipped,
                                hipStream_t stream = nullptr)
{
  using X = decltype(model.xdes(0.0));
  using U = decltype(model.udes(0.0));
  constexpr int K = MPCT::Kmesh;
  // the tables travel by value in the kernel arguments: 85 doubles at Kmesh = 4 (the degree every model here uses, and
  // the one that is tested), 161 at 6; larger degrees would want them in device memory
  static_assert(K <= 6, "mpc_dyn_error_device: tables by value in the kernel arguments, built for Kmesh <= 6");
  static_assert(std::is_same_v<typename MPCT::TimeT, double>, "the device-side audit takes time as double seconds");
  const int nivals = proto.mesh().N_ivals();
  if (B <= 0) return hipSuccess;
  constexpr int W      = detail::audit_slot(K + 2);
  const int64_t blocks = (B * nivals * W + 63) / 64;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const detail::AuditTables<K> tab = detail::make_audit_tables<K>();
  hipLaunchKernelGGL((detail::mpc_audit_kernel<X, U, K, Model>), dim3((unsigned)blocks), dim3(64), 0, stream, B, nivals, proto.params().tf, model, tab,
                     d_t, d_primal, d_errs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(detail::mpc_audit_reduce_kernel<256>, dim3((unsigned)nivals + 1), dim3(256), 0, stream, B, nivals, d_code, d_errs, d_agent_max,
                     d_ival_max, d_skipped);
  return hipGetLastError();
}

}  // namespace smooth_feedback_amd
