// Optimal control problem -> nonlinear program by collocation on a ph mesh (reference ocp_to_nlp.hpp: ocp_to_nlp(),
// detail::OCPNLP, detail::ocp_nlp_structure, nlpsol_to_ocpsol, ocpsol_to_nlpsol), on plain arrays over nlp.hpp.
//
// t0 = 0.  Variables [tf | q (Nq) | x_0 .. x_N | u_0 .. u_{N-1}], constraints [dyn Nx N | integrals Nq | running Ncr N |
// end Nce], and with ws = 1 / max(1e-6, max_i w_i)
//   g = [ws mesh_dyn.F | ws (mesh_integrate.F - q) | ws mesh_eval(cr, scaled by the weights).F | ce(tf, x0, xf, q)],
// dg_dx the mesh functions' dF without the t0 column, scaled by ws, with -ws I at (integral r, q_r) and the unscaled
// Jacobian of ce; f, df_dx, d2f_dx2 from theta(tf, x0, xf, q) (reference :121-155, :251-331).
//
// One law: g and dg_dx are written by meshfn::ocp_nlp_value (mesh_function.hpp) item by item over the decode records of
// meshfn::ocp_nlp_pattern -- the function and the records the fused kernel of smooth_feedback_amd/csrc/mesh.hip uses
// (sfb_ocp_nlp_batch).  The front evaluates the model at the nodes into the arrays that entry takes and runs the same loop.
//
// Patterns depend on (mesh, dims) only and every reserved entry is stored: dg_dx in CSR as described at
// meshfn::ocp_nlp_pattern; d2f_dx2 and d2g_dx2 share ONE upper-triangle CSC pattern, so sigma d2f + d2g is a sum value by
// value: the image of meshfn::d2_pattern under the variable map, united with the (tf, q, x0, xf)^2 block.
// Differences from the reference, stated once:
//   * the Hessian is the mathematical one.  In the NLP order q comes before x, and the reference's
//     block_add(.., x0var_B, qvar_B, .., upper_only = true) (and the same for xf) tests row <= col on a block that lies
//     wholly below the diagonal, so it drops the x0-q and xf-q cross terms of theta and ce.  Here those blocks are stored
//     transposed, at (q, x0) and (q, xf).
//   * derivatives: a functor may carry analytic derivatives; otherwise differences (diff::Type as in mesh_function.hpp).
//     f, g, cr: jacobian(t, x, u, J) / hessian(t, x, u, H) as there.  theta, ce: jacobian(tf, x0, xf, q, J) with
//     J (rows x (1 + 2 Nx + Nq)), columns (tf | x0 | xf | q), and hessian(tf, x0, xf, q, H) with the rows' Hessians side by
//     side.  (detail::jac_end / hess_end of ocp_to_qp.hpp hold tf fixed and carry no q blocks, which the NLP needs.)
//   * Ocp is any type with the members of OCP<...> of ocp_to_qp.hpp (that type asks every size to be positive; a problem
//     without integrals or constraints brings a struct of its own).  X and U must be Rn<.> (flatten_ocp of ocp_flatten.hpp makes them so).
// The Lagrangian Hessian sigma d2f + d2g(lambda) in one pass is d2l_dx2(x, sigma, lambda): the same pattern, its values written by
// meshfn::ocp_nlp_hess_value entry by entry over the records of meshfn::ocp_nlp_hess_pattern -- the function and the records the
// kernel behind sfb_ocp_nlp_hess_batch uses.  d2f_dx2 and d2g_dx2 keep their own code.
// A problem on Lie groups comes here through flatten_ocp (ocp_flatten.hpp).  The solver is apart: the swarm SQP solver sfb_nlp_sqp_*
// of sfb.h consumes g, dg_dx and the Lagrangian Hessian of a swarm where sfb_ocp_nlp_batch / _hess_batch leave them.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <functional>
#include <limits>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

#include "lie.hpp"
#include "mesh.hpp"
#include "mesh_function.hpp"
#include "nlp.hpp"
#include "ocp_to_qp.hpp"

namespace smooth_feedback_amd {

/// the solution of an OCP as the NLP side carries it (reference ocp.hpp:124-166 with the multipliers)
template<class X, class U, int Nq, int Ncr, int Nce>
struct OCPNLPSolution {
  double t0 = 0., tf = 1.;
  Vec<Nq> Q{};
  std::function<U(double)> u;
  std::function<X(double)> x;
  Vec<Nq> lambda_q{};
  Vec<Nce> lambda_ce{};
  std::function<Vec<X::Dof>(double)> lambda_dyn;
  std::function<Vec<Ncr>(double)> lambda_cr;
};

namespace detail {

template<class Ocp>
meshfn::OcpDims ocp_dims(const Ocp &)
{
  return meshfn::OcpDims{Ocp::Nx, Ocp::Nu, Ocp::Nq, Ocp::Ncr, Ocp::Nce};
}

/// (var_beg[5], var_len[4], con_beg[5], con_len[4]) (:24-51)
template<class Ocp, class Mesh>
auto ocp_nlp_structure(const Ocp & ocp, const Mesh & mesh)
{
  int64_t vb[5], cb[5];
  meshfn::ocp_nlp_structure((int64_t)mesh.N_colloc(), ocp_dims(ocp), vb, cb);
  std::array<std::size_t, 5> var_beg{}, con_beg{};
  std::array<std::size_t, 4> var_len{}, con_len{};
  for (int k = 0; k < 5; ++k) var_beg[k] = (std::size_t)vb[k], con_beg[k] = (std::size_t)cb[k];
  for (int k = 0; k < 4; ++k) var_len[k] = var_beg[k + 1] - var_beg[k], con_len[k] = con_beg[k + 1] - con_beg[k];
  return std::make_tuple(var_beg, var_len, con_beg, con_len);
}

/// theta or ce at z = (tf | x0 | xf | q): value val [R], Jacobian J (R x ne), Hessians H (ne x R ne, side by side)
template<uint8_t Deriv, diff::Type DT, int R, bool Scalar, class Fn, int Nx, int Nq>
struct EndEval {
  static constexpr int ne = 1 + 2 * Nx + Nq;
  using JMat = Mat<R, ne>;
  using HMat = Mat<ne, R * ne>;
  static constexpr bool has_jacobian =
    requires(const Fn & f, const Rn<Nx> & x, const Vec<Nq> & q, JMat & J) { f.jacobian(0.0, x, x, q, J); };
  static constexpr bool has_hessian = requires(const Fn & f, const Rn<Nx> & x, const Vec<Nq> & q, HMat & H) { f.hessian(0.0, x, x, q, H); };
  static_assert(DT != diff::Type::Analytic || Deriv < 1 || has_jacobian, "diff::Type::Analytic: theta / ce need jacobian(tf, x0, xf, q, J)");
  static_assert(DT != diff::Type::Analytic || Deriv < 2 || has_hessian, "diff::Type::Analytic: theta / ce need hessian(tf, x0, xf, q, H)");
  Vec<R> val{};
  JMat J{};
  HMat H{};

  static Vec<R> at(const Fn & fn, std::array<double, ne> z)
  {
    Rn<Nx> x0, xf;
    Vec<Nq> q{};
    for (int d = 0; d < Nx; ++d) x0.v[d] = z[1 + d], xf.v[d] = z[1 + Nx + d];
    for (int d = 0; d < Nq; ++d) q[d] = z[1 + 2 * Nx + d];
    Vec<R> v{};
    if constexpr (Scalar) v[0] = fn(z[0], x0, xf, q);
    else v = fn(z[0], x0, xf, q);
    return v;
  }
  void operator()(const Fn & fn, double tf, const Rn<Nx> & x0, const Rn<Nx> & xf, const Vec<Nq> & q)
  {
    std::array<double, ne> z{};
    z[0] = tf;
    for (int d = 0; d < Nx; ++d) z[1 + d] = x0.v[d], z[1 + Nx + d] = xf.v[d];
    for (int d = 0; d < Nq; ++d) z[1 + 2 * Nx + d] = q[d];
    val = at(fn, z);
    if constexpr (Deriv >= 1) {
      if constexpr (DT != diff::Type::Numerical && has_jacobian) {
        fn.jacobian(tf, x0, xf, q, J);
      } else {
        const double h = meshfn_fd_step();
        for (int a = 0; a < ne; ++a) {
          auto za = z;
          za[a] += h;
          const Vec<R> fa = at(fn, za);
          for (int r = 0; r < R; ++r) J(r, a) = (fa[r] - val[r]) / h;
        }
      }
    }
    if constexpr (Deriv >= 2) {
      if constexpr (DT != diff::Type::Numerical && has_hessian) {
        fn.hessian(tf, x0, xf, q, H);
      } else {
        const double h = std::sqrt(meshfn_fd_step());
        for (int a = 0; a < ne; ++a)
          for (int b = a; b < ne; ++b) {
            auto pp = z, pm = z, mp = z, mm = z;
            pp[a] += h, pp[b] += h, pm[a] += h, pm[b] -= h, mp[a] -= h, mp[b] += h, mm[a] -= h, mm[b] -= h;
            const Vec<R> fpp = at(fn, pp), fpm = at(fn, pm), fmp = at(fn, mp), fmm = at(fn, mm);
            for (int r = 0; r < R; ++r) H(a, r * ne + b) = H(b, r * ne + a) = ((fpp[r] - fpm[r]) - (fmp[r] - fmm[r])) / (4 * h * h);
          }
      }
    }
  }
};

/// NLP of an OCP over a mesh (:58-417).  Results are returned by const reference to members allocated by the
/// constructor: no output array moves afterwards.
template<class Ocp, class Mesh, diff::Type DT = diff::Type::Default>
class OCPNLP {
public:
  using X = typename Ocp::X;
  using U = typename Ocp::U;
  static constexpr int Nx = Ocp::Nx, Nu = Ocp::Nu, Nq = Ocp::Nq, Ncr = Ocp::Ncr, Nce = Ocp::Nce, nz = 1 + Nx + Nu, ne = 1 + 2 * Nx + Nq;
  static_assert(is_rn<X>::value && is_rn<U>::value,
                "ocp_to_nlp: X and U must be Rn<.>; a problem on a Lie group goes through flatten_ocp (ocp_flatten.hpp) first");
  static_assert(Nx >= 1, "ocp_to_nlp: Nx >= 1");

  OCPNLP(Ocp ocp, Mesh mesh) : ocp_(std::move(ocp)), mesh_(std::move(mesh)), N_(mesh_.N_colloc()), dims_(ocp_dims(ocp_))
  {
    meshfn::ocp_nlp_structure((int64_t)N_, dims_, vb_, cb_);
    const std::size_t S = mesh_.N_ivals(), n = (std::size_t)vb_[4], m = (std::size_t)cb_[4];
    const std::vector<double> taus = mesh_.all_nodes(), wts = mesh_.all_weights();
    std::vector<int32_t> K(S);
    double wmax = 0.0;
    for (std::size_t s = 0, i = 0; s < S; ++s) {
      K[s]                    = (int32_t)mesh_.N_colloc_ival(s);
      const auto [alpha, Dus] = mesh_.interval_diffmat_unscaled(s);
      for (int32_t j = 0; j < K[s]; ++j, ++i) {
        nodes_.push_back(meshfn::OcpNlpNode{taus[i], wts[i], alpha, K[s], (int32_t)(i - j)});
        wmax = std::max(wmax, wts[i]);
      }
      D_.insert(D_.end(), Dus.a.begin(), Dus.a.begin() + (std::ptrdiff_t)(K[s] + 1) * K[s]);
    }
    ws_ = meshfn::ocp_nlp_w_scaling(wmax);
    // constraint Jacobian and the decode records
    const int64_t nnz = meshfn::ocp_nlp_pattern((int)S, K.data(), dims_, nullptr, nullptr, nullptr);
    dg_.rows = (int32_t)m, dg_.cols = (int32_t)n;
    dg_.rowptr.assign(m + 1, 0), dg_.colind.assign((std::size_t)nnz, 0), dg_.val.assign((std::size_t)nnz, 0.0);
    items_.resize(m + (std::size_t)nnz);
    meshfn::ocp_nlp_pattern((int)S, K.data(), dims_, dg_.rowptr.data(), dg_.colind.data(), items_.data());
    g_.assign(m, 0.0);
    // bounds
    xl_.assign(n, 0.0), xu_.assign(n, 0.0), gl_.assign(m, 0.0), gu_.assign(m, 0.0);
    meshfn::ocp_nlp_bounds(dims_, (int64_t)N_, nodes_.data(), ws_, ocp_.crl.data(), ocp_.cru.data(), ocp_.cel.data(), ocp_.ceu.data(), xl_.data(),
                           xu_.data(), gl_.data(), gu_.data());
    // objective gradient: columns tf | q | x0 | xf
    for (int a = 0; a < ne; ++a) end_col_[a] = a == 0 ? 0 : a <= Nx ? (int)vb_[2] + a - 1 : a <= 2 * Nx ? (int)(vb_[2] + N_ * Nx) + a - 1 - Nx : (int)vb_[1] + a - 1 - 2 * Nx;
    std::vector<std::pair<int, int>> ord;  // (column, position in the (tf | x0 | xf | q) order)
    for (int a = 0; a < ne; ++a) ord.push_back({end_col_[a], a});
    std::sort(ord.begin(), ord.end());
    df_.rows = 1, df_.cols = (int32_t)n;
    df_.rowptr = {0, ne};
    for (const auto & [c, a] : ord) df_.colind.push_back(c), df_src_.push_back(a);
    df_.val.assign(ne, 0.0);
    // the shared upper-triangle pattern: the image of the mesh functions' d2 pattern, united with the end block
    meshfn::d2_pattern((int64_t)N_, Nx, Nu, d2old_);
    std::map<std::pair<int, int>, int> pos;  // (col, row) -> index
    const auto to_new = [&](int c) { return c == 1 ? 0 : c < 2 + Nx * (int)(N_ + 1) ? (int)vb_[2] + c - 2 : (int)vb_[3] + c - 2 - Nx * (int)(N_ + 1); };
    for (int c = 1; c < d2old_.cols; ++c)
      for (int p = d2old_.colptr[c]; p < d2old_.colptr[c + 1]; ++p)
        if (d2old_.rowind[p] > 0) pos[{to_new(c), to_new(d2old_.rowind[p])}] = 0;
    for (int a = 0; a < ne; ++a)
      for (int b = 0; b < ne; ++b)
        if (end_col_[a] <= end_col_[b]) pos[{end_col_[b], end_col_[a]}] = 0;
    d2f_.rows = d2f_.cols = (int32_t)n;
    d2f_.colptr.assign(n + 1, 0);
    int at = 0;
    for (auto & [cr, idx] : pos) idx = at++, d2f_.rowind.push_back(cr.second), ++d2f_.colptr[(std::size_t)cr.first + 1];
    for (std::size_t c = 0; c < n; ++c) d2f_.colptr[c + 1] += d2f_.colptr[c];
    d2f_.val.assign(d2f_.rowind.size(), 0.0);
    d2g_ = d2f_;
    d2_map_.assign(d2old_.rowind.size(), -1);
    for (int c = 1; c < d2old_.cols; ++c)
      for (int p = d2old_.colptr[c]; p < d2old_.colptr[c + 1]; ++p)
        if (d2old_.rowind[p] > 0) d2_map_[(std::size_t)p] = pos[{to_new(c), to_new(d2old_.rowind[p])}];
    for (int a = 0; a < ne; ++a)
      for (int b = 0; b < ne; ++b) end_map_[a][b] = end_col_[a] <= end_col_[b] ? pos[{end_col_[b], end_col_[a]}] : -1;
    // model values at the nodes, in the layout of the model-free entry
    Ff_.assign(N_ * Nx, 0.0), dFf_.assign(N_ * Nx * nz, 0.0), Fg_.assign(N_ * Nq, 0.0), dFg_.assign(N_ * Nq * nz, 0.0);
    Fcr_.assign(N_ * Ncr, 0.0), dFcr_.assign(N_ * Ncr * nz, 0.0), ce_.assign(Nce, 0.0), dce_.assign((std::size_t)Nce * ne, 0.0);
    X_.resize(N_ + 1), U_.resize(N_);
    // the Lagrangian Hessian: the records of the model-free entry (the same pattern, built by the shared builder) and its contracted inputs
    const int64_t nnzh = meshfn::ocp_nlp_hess_pattern((int)S, K.data(), dims_, nullptr, nullptr, nullptr);
    d2l_.rows = d2l_.cols = (int32_t)n;
    d2l_.colptr.assign(n + 1, 0), d2l_.rowind.assign((std::size_t)nnzh, 0), d2l_.val.assign((std::size_t)nnzh, 0.0);
    hitems_.resize((std::size_t)nnzh);
    meshfn::ocp_nlp_hess_pattern((int)S, K.data(), dims_, d2l_.colptr.data(), d2l_.rowind.data(), hitems_.data());
    HLf_.assign(N_ * nz * nz, 0.0), HLg_.assign(Nq > 0 ? N_ * nz * nz : 0, 0.0), HLcr_.assign(Ncr > 0 ? N_ * nz * nz : 0, 0.0);
    d2theta_.assign((std::size_t)ne * ne, 0.0), d2ce_l_.assign(Nce > 0 ? (std::size_t)ne * ne : 0, 0.0);
    dyn2_.lambda.assign(N_ * Nx, 0.0), int2_.lambda.assign(Nq, 0.0), cr2_.lambda.assign(N_ * Ncr, 0.0);
  }

  std::size_t n() const { return (std::size_t)vb_[4]; }
  std::size_t m() const { return (std::size_t)cb_[4]; }
  const std::vector<double> & xl() const { return xl_; }
  const std::vector<double> & xu() const { return xu_; }
  const std::vector<double> & gl() const { return gl_; }
  const std::vector<double> & gu() const { return gu_; }
  double w_scaling() const { return ws_; }
  /// what the fused kernel is given for this (mesh, dims); valid while this object lives and is not moved from
  meshfn::OcpNlpTables tables() const
  {
    return meshfn::OcpNlpTables{dims_, (int32_t)N_, cb_[4], (int64_t)dg_.val.size(), ws_, nodes_.data(), D_.data(), items_.data()};
  }

  /// the same for the Lagrangian Hessian (sfb_ocp_nlp_hess_batch), and one agent's arrays as d2l_dx2 last filled them
  meshfn::OcpNlpHessTables hess_tables() const
  {
    return meshfn::OcpNlpHessTables{dims_, (int32_t)N_, cb_[4], (int64_t)d2l_.val.size(), ws_, nodes_.data(), hitems_.data()};
  }
  meshfn::OcpNlpHessAgent hess_agent(const std::vector<double> & x, const std::vector<double> & lambda, double sigma) const
  {
    return meshfn::OcpNlpHessAgent{x.data(), lambda.data(), sigma, dFf_.data(), HLf_.data(), dFg_.data(), HLg_.data(), HLcr_.data(), d2theta_.data(), d2ce_l_.data()};
  }

  double f(const std::vector<double> & x)
  {
    EndEval<0, DT, 1, true, decltype(ocp_.theta), Nx, Nq> ev;
    end_args(x);
    ev(ocp_.theta, x[0], x0_, xf_, q_);
    return ev.val[0];
  }
  const MeshCsr & df_dx(const std::vector<double> & x)
  {
    EndEval<1, DT, 1, true, decltype(ocp_.theta), Nx, Nq> ev;
    end_args(x);
    ev(ocp_.theta, x[0], x0_, xf_, q_);
    for (int k = 0; k < ne; ++k) df_.val[(std::size_t)k] = ev.J(0, df_src_[(std::size_t)k]);
    return df_;
  }
  const MeshCsc & d2f_dx2(const std::vector<double> & x)
  {
    EndEval<2, DT, 1, true, decltype(ocp_.theta), Nx, Nq> ev;
    end_args(x);
    ev(ocp_.theta, x[0], x0_, xf_, q_);
    for (double & v : d2f_.val) v = 0.0;
    add_end_hessian(d2f_, 1.0, [&](int a, int b) { return ev.H(a, b); });
    return d2f_;
  }
  const std::vector<double> & g(const std::vector<double> & x)
  {
    evaluate<0>(x);
    meshfn::ocp_nlp_assemble(tables(), agent(x), g_.data(), nullptr);
    return g_;
  }
  const MeshCsr & dg_dx(const std::vector<double> & x)
  {
    evaluate<1>(x);
    meshfn::ocp_nlp_assemble(tables(), agent(x), g_.data(), dg_.val.data());
    return dg_;
  }
  const MeshCsc & d2g_dx2(const std::vector<double> & x, const std::vector<double> & lambda)
  {
    states(x);
    const double tf = x[0];
    for (double & v : d2g_.val) v = 0.0;
    const auto add_mesh = [&](const MeshCsc & H) {
      for (std::size_t p = 0; p < H.val.size(); ++p)
        if (d2_map_[p] >= 0) d2g_.val[(std::size_t)d2_map_[p]] += ws_ * H.val[p];
    };
    std::copy(lambda.begin() + cb_[0], lambda.begin() + cb_[1], dyn2_.lambda.begin());
    mesh_dyn<2, DT>(dyn2_, mesh_, ocp_.f, 0.0, tf, X_, U_);
    add_mesh(dyn2_.d2F);
    if constexpr (Nq > 0) {
      std::copy(lambda.begin() + cb_[1], lambda.begin() + cb_[2], int2_.lambda.begin());
      mesh_integrate<2, DT>(int2_, mesh_, ocp_.g, 0.0, tf, X_, U_);
      add_mesh(int2_.d2F);
    }
    if constexpr (Ncr > 0) {
      std::copy(lambda.begin() + cb_[2], lambda.begin() + cb_[3], cr2_.lambda.begin());
      mesh_eval<2, DT>(cr2_, mesh_, ocp_.cr, 0.0, tf, X_, U_, true);
      add_mesh(cr2_.d2F);
    }
    if constexpr (Nce > 0) {
      EndEval<2, DT, Nce, false, decltype(ocp_.ce), Nx, Nq> ev;
      end_args(x);
      ev(ocp_.ce, tf, x0_, xf_, q_);
      for (int j = 0; j < Nce; ++j) add_end_hessian(d2g_, lambda[(std::size_t)cb_[3] + j], [&](int a, int b) { return ev.H(a, j * ne + b); });
    }
    return d2g_;
  }
  /// sigma d2f_dx2 + d2g_dx2(lambda) in one pass: the model at the nodes (order 2) contracted with the multipliers into the
  /// arrays of the model-free entry, then meshfn::ocp_nlp_hess_assemble -- the loop the kernel of sfb_ocp_nlp_hess_batch runs
  const MeshCsc & d2l_dx2(const std::vector<double> & x, double sigma, const std::vector<double> & lambda)
  {
    states(x);
    const double tf = x[0];
    for (std::size_t i = 0; i < N_; ++i) {
      const double t = 0.0 + (tf - 0.0) * nodes_[i].tau;
      node_hessian<Nx>(ocp_.f, t, i, lambda.data() + cb_[0] + i * Nx, dFf_.data(), HLf_.data());
      node_hessian<Nq>(ocp_.g, t, i, lambda.data() + cb_[1], dFg_.data(), HLg_.data());
      node_hessian<Ncr>(ocp_.cr, t, i, lambda.data() + cb_[2] + i * Ncr, dFcr_.data(), HLcr_.data());
    }
    end_args(x);
    {
      EndEval<2, DT, 1, true, decltype(ocp_.theta), Nx, Nq> ev;
      ev(ocp_.theta, tf, x0_, xf_, q_);
      for (int a = 0; a < ne; ++a)
        for (int b = 0; b < ne; ++b) d2theta_[(std::size_t)a * ne + b] = ev.H(a, b);
    }
    if constexpr (Nce > 0) {
      EndEval<2, DT, Nce, false, decltype(ocp_.ce), Nx, Nq> ev;
      ev(ocp_.ce, tf, x0_, xf_, q_);
      for (int a = 0; a < ne; ++a)
        for (int b = 0; b < ne; ++b) {
          double acc = 0.0;
          for (int r = 0; r < Nce; ++r) acc += lambda[(std::size_t)cb_[3] + r] * ev.H(a, r * ne + b);
          d2ce_l_[(std::size_t)a * ne + b] = acc;
        }
    }
    meshfn::ocp_nlp_hess_assemble(hess_tables(), hess_agent(x, lambda, sigma), sigma, d2l_.val.data());
    return d2l_;
  }

private:
  void end_args(const std::vector<double> & x)
  {
    for (int d = 0; d < Nx; ++d) x0_.v[d] = x[(std::size_t)vb_[2] + d], xf_.v[d] = x[(std::size_t)vb_[2] + N_ * Nx + d];
    for (int d = 0; d < Nq; ++d) q_[d] = x[(std::size_t)vb_[1] + d];
  }
  void states(const std::vector<double> & x)
  {
    for (std::size_t i = 0; i <= N_; ++i)
      for (int d = 0; d < Nx; ++d) X_[i].v[d] = x[(std::size_t)vb_[2] + i * Nx + d];
    for (std::size_t i = 0; i < N_; ++i)
      for (int d = 0; d < Nu; ++d) U_[i].v[d] = x[(std::size_t)vb_[3] + i * Nu + d];
  }
  template<class H>
  void add_end_hessian(MeshCsc & out, double scale, H && h)
  {
    for (int a = 0; a < ne; ++a)
      for (int b = 0; b < ne; ++b)
        if (end_map_[a][b] >= 0 && (end_col_[a] < end_col_[b] || a == b)) out.val[(std::size_t)end_map_[a][b]] += scale * h(a, b);
  }
  template<uint8_t Deriv, int NF, class Fn>
  void node_model(Fn & fn, double t, std::size_t i, double * F, double * dF)
  {
    if constexpr (NF > 0) {
      MeshModelEval<Deriv, DT, Fn, X, U> ev;
      ev(fn, t, X_[i], U_[i]);
      for (int r = 0; r < NF; ++r) {
        F[i * NF + r] = ev.f[r];
        if constexpr (Deriv >= 1)
          for (int c = 0; c < nz; ++c) dF[(i * NF + r) * nz + c] = ev.J(r, c);
      }
    }
  }
  /// node i of one model at order 2: its Jacobian into dF, and its Hessians contracted with lam [NF] into HL [i][nz][nz]
  template<int NF, class Fn>
  void node_hessian(Fn & fn, double t, std::size_t i, const double * lam, double * dF, double * HL)
  {
    if constexpr (NF > 0) {
      MeshModelEval<2, DT, Fn, X, U> ev;
      ev(fn, t, X_[i], U_[i]);
      for (int r = 0; r < NF; ++r)
        for (int c = 0; c < nz; ++c) dF[(i * NF + r) * nz + c] = ev.J(r, c);
      for (int a = 0; a < nz; ++a)
        for (int b = 0; b < nz; ++b) {
          double acc = 0.0;
          for (int r = 0; r < NF; ++r) acc += lam[r] * ev.H(a, r * nz + b);
          HL[(i * nz + a) * nz + b] = acc;
        }
    }
  }
  /// the model at the nodes (times tf tau_i) and the end constraint, into the arrays of the model-free entry
  template<uint8_t Deriv>
  void evaluate(const std::vector<double> & x)
  {
    states(x);
    const double tf = x[0];
    for (std::size_t i = 0; i < N_; ++i) {
      const double t = 0.0 + (tf - 0.0) * nodes_[i].tau;
      node_model<Deriv, Nx>(ocp_.f, t, i, Ff_.data(), dFf_.data());
      node_model<Deriv, Nq>(ocp_.g, t, i, Fg_.data(), dFg_.data());
      node_model<Deriv, Ncr>(ocp_.cr, t, i, Fcr_.data(), dFcr_.data());
    }
    if constexpr (Nce > 0) {
      EndEval<Deriv, DT, Nce, false, decltype(ocp_.ce), Nx, Nq> ev;
      end_args(x);
      ev(ocp_.ce, tf, x0_, xf_, q_);
      for (int r = 0; r < Nce; ++r) {
        ce_[(std::size_t)r] = ev.val[r];
        if constexpr (Deriv >= 1)
          for (int c = 0; c < ne; ++c) dce_[(std::size_t)r * ne + c] = ev.J(r, c);
      }
    }
  }
  meshfn::OcpNlpAgent agent(const std::vector<double> & x) const
  {
    return meshfn::OcpNlpAgent{x.data(), Ff_.data(), dFf_.data(), Fg_.data(), dFg_.data(), Fcr_.data(), dFcr_.data(), ce_.data(), dce_.data()};
  }

  Ocp ocp_;
  Mesh mesh_;
  std::size_t N_;
  meshfn::OcpDims dims_;
  int64_t vb_[5], cb_[5];
  double ws_{1};
  std::vector<meshfn::OcpNlpNode> nodes_;
  std::vector<double> D_;
  std::vector<meshfn::OcpNlpItem> items_;
  std::vector<double> xl_, xu_, gl_, gu_, g_;
  MeshCsr df_, dg_;
  MeshCsc d2f_, d2g_, d2old_, d2l_;
  std::vector<meshfn::OcpNlpHessItem> hitems_;
  std::vector<double> HLf_, HLg_, HLcr_, d2theta_, d2ce_l_;
  std::vector<int> df_src_, d2_map_;
  int end_col_[ne], end_map_[ne][ne];
  std::vector<double> Ff_, dFf_, Fg_, dFg_, Fcr_, dFcr_, ce_, dce_;
  std::vector<X> X_;
  std::vector<U> U_;
  X x0_, xf_;
  Vec<Nq> q_{};
  MeshValue<2> dyn2_, int2_, cr2_;
};

}  // namespace detail

/// the OCP as an NLP by collocation on the mesh (:431-437)
template<diff::Type DT = diff::Type::Default, class Ocp, class Mesh>
auto ocp_to_nlp(Ocp && ocp, Mesh && mesh) -> detail::OCPNLP<std::decay_t<Ocp>, std::decay_t<Mesh>, DT>
{
  return detail::OCPNLP<std::decay_t<Ocp>, std::decay_t<Mesh>, DT>(std::forward<Ocp>(ocp), std::forward<Mesh>(mesh));
}

/// NLP solution -> OCP solution (:442-508): x through Mesh::eval with the end point, u and the multipliers without
template<class Ocp, class Mesh>
auto nlpsol_to_ocpsol(const Ocp & ocp, const Mesh & mesh, const NLPSolution & s)
{
  using X = typename Ocp::X;
  using U = typename Ocp::U;
  constexpr int Nx = Ocp::Nx, Nu = Ocp::Nu, Nq = Ocp::Nq, Ncr = Ocp::Ncr, Nce = Ocp::Nce;
  const std::size_t N = mesh.N_colloc();
  const auto [vb, vl, cb, cl] = detail::ocp_nlp_structure(ocp, mesh);
  const double t0 = 0, tf = s.x[vb[0]];
  const auto rows = [](const std::vector<double> & v, std::size_t beg, std::size_t count, auto proto) {
    std::vector<decltype(proto)> out(count);
    constexpr std::size_t D = std::tuple_size_v<decltype(proto)>;
    for (std::size_t i = 0; i < count; ++i)
      for (std::size_t d = 0; d < D; ++d) out[i][d] = v[beg + i * D + d];
    return out;
  };
  OCPNLPSolution<X, U, Nq, Ncr, Nce> out;
  out.t0 = t0, out.tf = tf;
  for (int d = 0; d < Nq; ++d) out.Q[d] = s.x[vb[1] + d], out.lambda_q[d] = s.lambda[cb[1] + d];
  for (int d = 0; d < Nce; ++d) out.lambda_ce[d] = s.lambda[cb[3] + d];
  out.x = [=, Xv = rows(s.x, vb[2], N + 1, std::array<double, Nx>{})](double t) {
    X r;
    const auto v = mesh.template eval<Nx>((t - t0) / (tf - t0), Xv, 0, true);
    for (int d = 0; d < Nx; ++d) r.v[d] = v[d];
    return r;
  };
  out.u = [=, Uv = rows(s.x, vb[3], Nu > 0 ? N : 0, std::array<double, (Nu > 0 ? Nu : 1)>{})](double t) {
    U r;
    if constexpr (Nu > 0) {
      const auto v = mesh.template eval<Nu>((t - t0) / (tf - t0), Uv, 0, false);
      for (int d = 0; d < Nu; ++d) r.v[d] = v[d];
    }
    return r;
  };
  out.lambda_dyn = [=, Lv = rows(s.lambda, cb[0], N, std::array<double, Nx>{})](double t) -> Vec<Nx> {
    return mesh.template eval<Nx>((t - t0) / (tf - t0), Lv, 0, false);
  };
  out.lambda_cr = [=, Lv = rows(s.lambda, cb[2], Ncr > 0 ? N : 0, std::array<double, (Ncr > 0 ? Ncr : 1)>{})](double t) -> Vec<Ncr> {
    if constexpr (Ncr > 0) return mesh.template eval<Ncr>((t - t0) / (tf - t0), Lv, 0, false);
    else return Vec<Ncr>{};
  };
  return out;
}

/// OCP solution -> NLP solution (:515-554): sampled at all_nodes(); status Unknown, zl = zu = 0
template<class Ocp, class Mesh, class Sol>
NLPSolution ocpsol_to_nlpsol(const Ocp & ocp, const Mesh & mesh, const Sol & sol)
{
  constexpr int Nx = Ocp::Nx, Nu = Ocp::Nu, Nq = Ocp::Nq, Ncr = Ocp::Ncr, Nce = Ocp::Nce;
  const std::size_t N = mesh.N_colloc();
  const auto [vb, vl, cb, cl] = detail::ocp_nlp_structure(ocp, mesh);
  const double t0 = 0, tf = sol.tf;
  NLPSolution out;
  out.status = NLPSolution::Status::Unknown;
  out.x.assign(vb[4], 0.0), out.zl.assign(vb[4], 0.0), out.zu.assign(vb[4], 0.0), out.lambda.assign(cb[4], 0.0);
  out.x[vb[0]] = sol.tf;
  for (int d = 0; d < Nq; ++d) out.x[vb[1] + d] = sol.Q[d], out.lambda[cb[1] + d] = sol.lambda_q[d];
  for (int d = 0; d < Nce; ++d) out.lambda[cb[3] + d] = sol.lambda_ce[d];
  const std::vector<double> taus = mesh.all_nodes();
  for (std::size_t i = 0; i <= N; ++i) {
    const double t = t0 + taus[i] * (tf - t0);
    const auto x   = sol.x(t);
    for (int d = 0; d < Nx; ++d) out.x[vb[2] + i * Nx + d] = x.v[d];
    if (i < N) {
      const auto u = sol.u(t);
      for (int d = 0; d < Nu; ++d) out.x[vb[3] + i * Nu + d] = u.v[d];
      const auto ld = sol.lambda_dyn(t);
      for (int d = 0; d < Nx; ++d) out.lambda[cb[0] + i * Nx + d] = ld[d];
      const auto lc = sol.lambda_cr(t);
      for (int d = 0; d < Ncr; ++d) out.lambda[cb[2] + i * Ncr + d] = lc[d];
    }
  }
  return out;
}

}  // namespace smooth_feedback_amd
