// A swarm of flattened Lie-group problems whose MODEL runs on the GPU as well (HIP only: include from a translation unit
// compiled by hipcc).  The fused kernels behind sfb_ocp_nlp_batch / sfb_ocp_nlp_hess_batch are model-free: they take the
// model at the collocation nodes as arrays.  For a problem on a group those arrays are the flattened functions of
// ocp_flatten.hpp -- the model and the whole change of variables, N (nx + nq + ncr) (2 + nx + nu) doubles per agent -- and
// without this front they are evaluated on the host and go up over PCIe on every call.  Here one GPU lane per (agent, node),
// and one per agent for the end functions, evaluates them where the NLP kernel reads them.
//
// Model: a struct with `__host__ __device__` members
//   theta, f, g, cr, ce                                   the functors of the problem on the groups X, U (optionally with
//                                                         jacobian members, ocp_flatten.hpp)
//   X xl(int64_t b, double t),  X::Tangent dxl(b, t)      agent b's linearisation trajectory and its body velocity
//   U ul(int64_t b, double t),  U::Tangent dul(b, t)
// Ocp names the sizes and the groups (Ocp::X, Ocp::U, Nq, Ncr, Nce, and crl, cru, cel, ceu for bounds()).  The law is
// the one of ocp_flatten.hpp: the kernel builds agent b's FlatDyn / FlatInnerFun / FlatEndptFun and calls their eval().
#pragma once
#ifndef __HIPCC__
#error "ocp_flatten_device.hpp needs hipcc"
#endif
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../sfb.h"
#include "detail/device_arena.hpp"
#include "ocp_flatten.hpp"

namespace smooth_feedback_amd {

/// the model at the nodes as sfb_ocp_nlp_batch takes it, and the objective: device arrays, agent-major
struct FlatNodeArrays {
  double *Ff, *dFf;      // [B][N][nx], [B][N][nx][1 + nx + nu]
  double *Fg, *dFg;      // [B][N][nq], ...
  double *Fcr, *dFcr;    // [B][N][ncr], ...
  double *ce, *dce;      // [B][nce], [B][nce][1 + 2 nx + nq], columns (tf | e0 | ef | q)
  double *theta, *dtheta;  // [B], [B][1 + 2 nx + nq]
};

namespace detail {

/// One lane per (agent, collocation node) and one per agent for the end functions.  x [B][n] in the layout of the NLP,
/// [tf | q | e_0 .. e_N | v_0 .. v_{N-1}]; tau [N] the nodes on [0, 1].  Every loop over matrix entries has compile-time
/// bounds and is unrolled: with run-time indices the matrices would live in scratch memory (see mpc_linearise_kernel).
template<class Ocp, class Model>
__global__ void __launch_bounds__(64) flat_ocp_nodes_kernel(const int64_t B, const int32_t N, const int64_t n, const Model model,
                                                            const double * __restrict__ tau, const double * __restrict__ x, const FlatNodeArrays out)
{
  using X = typename Ocp::X;
  using U = typename Ocp::U;
  constexpr int Nx = X::Dof, Nu = U::Dof, Nq = Ocp::Nq, Ncr = Ocp::Ncr, Nce = Ocp::Nce, nz = 1 + Nx + Nu, ne = 1 + 2 * Nx + Nq;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t b   = gid / (N + 1);
  const int i       = (int)(gid - b * (N + 1));
  if (b >= B) return;
  const double * xa = x + b * n;
  const double tf   = xa[0];
  const AgentStateTrajectory<Model> xl{&model, b};
  const AgentInputTrajectory<Model> ul{&model, b};
  using XlT = AgentStateTrajectory<Model>;
  using UlT = AgentInputTrajectory<Model>;
  if (i < N) {
    const double t    = tf * tau[i];
    const double * xe = xa + 1 + Nq + (int64_t)i * Nx;
    const double * xv = xa + 1 + Nq + (int64_t)(N + 1) * Nx + (int64_t)i * Nu;
    Rn<Nx> e;
    Rn<Nu> v;
#pragma unroll
    for (int d = 0; d < Nx; ++d) e.v[d] = xe[d];
#pragma unroll
    for (int d = 0; d < Nu; ++d) v.v[d] = xv[d];
    const int64_t node = b * N + i;
    {
      Vec<Nx> val;
      Mat<Nx, nz> J;
      FlatDyn<X, U, decltype(model.f), XlT, UlT>{model.f, xl, ul}.eval(t, e, v, val, J);
#pragma unroll
      for (int r = 0; r < Nx; ++r) {
        out.Ff[node * Nx + r] = val[r];
#pragma unroll
        for (int c = 0; c < nz; ++c) out.dFf[(node * Nx + r) * nz + c] = J(r, c);
      }
    }
    {
      Vec<Nq> val;
      Mat<Nq, nz> J;
      FlatInnerFun<X, U, Nq, decltype(model.g), XlT, UlT>{model.g, xl, ul}.eval(t, e, v, val, J);
#pragma unroll
      for (int r = 0; r < Nq; ++r) {
        out.Fg[node * Nq + r] = val[r];
#pragma unroll
        for (int c = 0; c < nz; ++c) out.dFg[(node * Nq + r) * nz + c] = J(r, c);
      }
    }
    {
      Vec<Ncr> val;
      Mat<Ncr, nz> J;
      FlatInnerFun<X, U, Ncr, decltype(model.cr), XlT, UlT>{model.cr, xl, ul}.eval(t, e, v, val, J);
#pragma unroll
      for (int r = 0; r < Ncr; ++r) {
        out.Fcr[node * Ncr + r] = val[r];
#pragma unroll
        for (int c = 0; c < nz; ++c) out.dFcr[(node * Ncr + r) * nz + c] = J(r, c);
      }
    }
  } else {
    Rn<Nx> e0, ef;
    Vec<Nq> q;
#pragma unroll
    for (int d = 0; d < Nx; ++d) e0.v[d] = xa[1 + Nq + d], ef.v[d] = xa[1 + Nq + (int64_t)N * Nx + d];
#pragma unroll
    for (int d = 0; d < Nq; ++d) q[d] = xa[1 + d];
    {
      Vec<Nce> val;
      Mat<Nce, ne> J;
      FlatEndptFun<X, Nq, Nce, false, decltype(model.ce), XlT>{model.ce, xl}.eval(tf, e0, ef, q, val, J);
#pragma unroll
      for (int r = 0; r < Nce; ++r) {
        out.ce[b * Nce + r] = val[r];
#pragma unroll
        for (int c = 0; c < ne; ++c) out.dce[(b * Nce + r) * ne + c] = J(r, c);
      }
    }
    {
      Vec<1> val;
      Mat<1, ne> J;
      FlatEndptFun<X, Nq, 1, true, decltype(model.theta), XlT>{model.theta, xl}.eval(tf, e0, ef, q, val, J);
      out.theta[b] = val[0];
#pragma unroll
      for (int c = 0; c < ne; ++c) out.dtheta[b * ne + c] = J(0, c);
    }
  }
}

}  // namespace detail

/// the launch alone: `agents` problems over the nodes tau_dev [N] (device), x_dev [agents][n]; asynchronous on `stream`
template<class Ocp, class Model>
hipError_t flat_ocp_nodes_launch(const Model & model, int64_t agents, int32_t N, const double * tau_dev, const double * x_dev,
                                 const FlatNodeArrays & out, hipStream_t stream)
{
  if (agents <= 0) return hipSuccess;
  const int64_t n = 1 + Ocp::Nq + (int64_t)(N + 1) * Ocp::X::Dof + (int64_t)N * Ocp::U::Dof;
  hipLaunchKernelGGL((detail::flat_ocp_nodes_kernel<Ocp, Model>), detail::lane_grid(agents * (N + 1)), dim3(64), 0, stream, agents, N, n, model,
                     tau_dev, x_dev, out);
  return hipGetLastError();
}

/// g, dg_dx (values), f and df of the collocation NLPs of a swarm of flattened problems, model included, on the device.
/// Owns the node arrays (one allocation, detail/device_arena.hpp), the mesh and the dims.
template<class Ocp, class Model, class MeshT>
class FlatOCPSwarmDevice {
public:
  static constexpr int Nx = Ocp::X::Dof, Nu = Ocp::U::Dof, Nq = Ocp::Nq, Ncr = Ocp::Ncr, Nce = Ocp::Nce, nz = 1 + Nx + Nu, ne = 1 + 2 * Nx + Nq;

  FlatOCPSwarmDevice(Ocp ocp, Model model, const MeshT & mesh, int64_t agents)
      : ocp_(ocp), model_(model), B_(agents), N_((int32_t)mesh.N_colloc()), dims_{Nx, Nu, Nq, Ncr, Nce}
  {
    if (agents < 1) throw std::invalid_argument("FlatOCPSwarmDevice: agents >= 1");
    for (std::size_t s = 0; s < mesh.N_ivals(); ++s) K_.push_back((int32_t)mesh.N_colloc_ival(s)), tau0_.push_back(mesh.interval_start(s));
    cmesh_ = sfb_mesh{(int32_t)K_.size(), K_.data(), tau0_.data()};
    sfb_check(sfb_ocp_nlp_structure(&cmesh_, &dims_, vb_, cb_));
    sfb_check(sfb_ocp_nlp_pattern(&cmesh_, &dims_, nullptr, nullptr, &nnz_));
    const std::vector<double> taus = mesh.all_nodes();
    const size_t B = (size_t)B_, N = (size_t)N_;
    detail::DeviceArena a;
    a.add(&tau_, N);
    a.add(&arr_.Ff, B * N * Nx); a.add(&arr_.dFf, B * N * Nx * nz);
    a.add(&arr_.Fg, B * N * Nq); a.add(&arr_.dFg, B * N * Nq * nz);
    a.add(&arr_.Fcr, B * N * Ncr); a.add(&arr_.dFcr, B * N * Ncr * nz);
    a.add(&arr_.ce, B * Nce); a.add(&arr_.dce, B * Nce * ne);
    a.add(&arr_.theta, B); a.add(&arr_.dtheta, B * ne);
    bytes_ = a.bytes();
    mem_   = detail::DeviceBlock(a, "ocp_flatten_device");
    detail::hip_check(detail::upload(tau_, taus.data(), N), "ocp_flatten_device", "hipMemcpy(tau)");
  }
  FlatOCPSwarmDevice(const FlatOCPSwarmDevice &)             = delete;
  FlatOCPSwarmDevice & operator=(const FlatOCPSwarmDevice &) = delete;

  /// x_dev [agents][n] -> g_dev [agents][m], dg_val_dev [agents][nnz] (nullable: values only), f_dev [agents], df_dev
  /// [agents][1 + 2 nx + nq] over the columns df_columns() (both nullable: node_arrays().theta / .dtheta then).  The node
  /// kernel and sfb_ocp_nlp_batch run on `stream`, in that order; nothing waits on the host and nothing is allocated (the
  /// library uploads the tables of a (mesh, dims) pair once, on the first call that meets it).
  void eval(const double * x_dev, double * g_dev, double * dg_val_dev, double * f_dev, double * df_dev, hipStream_t stream)
  {
    detail::hip_check(nodes(x_dev, f_dev, df_dev, stream), "ocp_flatten_device", "flat_ocp_nodes_kernel");
    sfb_check(assemble(x_dev, g_dev, dg_val_dev, stream));
  }
  /// the two halves of eval()
  hipError_t nodes(const double * x_dev, double * f_dev, double * df_dev, hipStream_t stream)
  {
    FlatNodeArrays out = arr_;
    if (f_dev) out.theta = f_dev;
    if (df_dev) out.dtheta = df_dev;
    return flat_ocp_nodes_launch<Ocp, Model>(model_, B_, N_, tau_, x_dev, out, stream);
  }
  sfb_status assemble(const double * x_dev, double * g_dev, double * dg_val_dev, hipStream_t stream)
  {
    return sfb_ocp_nlp_batch(&cmesh_, &dims_, B_, x_dev, arr_.Ff, arr_.dFf, arr_.Fg, arr_.dFg, arr_.Fcr, arr_.dFcr, arr_.ce, arr_.dce, g_dev,
                             dg_val_dev, stream);
  }

  /// the device buffers of the last eval(): what sfb_ocp_nlp_batch was given, and what sfb_ocp_nlp_hess_batch takes as dFf, dFg, dFcr
  const FlatNodeArrays & node_arrays() const { return arr_; }
  int64_t size() const { return B_; }
  int64_t n() const { return vb_[4]; }
  int64_t m() const { return cb_[4]; }
  int64_t nnz() const { return nnz_; }
  int32_t N_colloc() const { return N_; }
  std::size_t device_bytes() const { return bytes_; }
  const sfb_mesh & mesh() const { return cmesh_; }
  const sfb_ocp_dims & dims() const { return dims_; }
  /// forwarded from the host entries of the model-free NLP: layout, pattern of dg_dx, bounds
  void structure(int64_t var_beg[5], int64_t con_beg[5]) const
  {
    for (int k = 0; k < 5; ++k) var_beg[k] = vb_[k], con_beg[k] = cb_[k];
  }
  void dg_pattern(int32_t * rowptr, int32_t * colind) const { sfb_check(sfb_ocp_nlp_pattern(&cmesh_, &dims_, rowptr, colind, nullptr)); }
  void bounds(double * xl, double * xu, double * gl, double * gu, double * w_scaling) const
  {
    sfb_check(sfb_ocp_nlp_bounds(&cmesh_, &dims_, ocp_.crl.data(), ocp_.cru.data(), ocp_.cel.data(), ocp_.ceu.data(), xl, xu, gl, gu, w_scaling));
  }
  /// the NLP column of entry a of df (tf | e0 | ef | q)
  std::vector<int32_t> df_columns() const
  {
    std::vector<int32_t> c((size_t)ne);
    for (int a = 0; a < ne; ++a)
      c[(size_t)a] = a == 0 ? 0 : a <= Nx ? (int32_t)vb_[2] + a - 1 : a <= 2 * Nx ? (int32_t)(vb_[2] + (int64_t)N_ * Nx) + a - 1 - Nx : (int32_t)vb_[1] + a - 1 - 2 * Nx;
    return c;
  }

private:
  static void sfb_check(sfb_status s)
  {
    if (s != SFB_OK) throw std::runtime_error(std::string("ocp_flatten_device: ") + sfb_last_error());
  }
  Ocp ocp_;
  Model model_;
  int64_t B_;
  int32_t N_;
  sfb_ocp_dims dims_;
  std::vector<int32_t> K_;
  std::vector<double> tau0_;
  sfb_mesh cmesh_{};
  int64_t vb_[5], cb_[5], nnz_ = 0;
  std::size_t bytes_ = 0;
  detail::DeviceBlock mem_;
  double * tau_ = nullptr;
  FlatNodeArrays arr_{};
};

}  // namespace smooth_feedback_amd
