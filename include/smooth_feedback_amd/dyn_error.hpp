// Collocation dynamics-error estimate (reference collocation/dyn_error.hpp:28-73) and the flattened dynamics of a
// group-valued problem (reference ocp_flatten.hpp:166-177), on plain arrays.  The interval estimate and the flattened
// dynamics are written once for host and device (SFB_LIE_HD): the host function mesh_dyn_error below and the batched
// kernel of smooth_feedback_amd/csrc/mesh.hip both call dyn_error_point.
#pragma once
#include <cmath>
#include <cstdint>
#include <tuple>
#include <vector>

#include "lie.hpp"
#include "mesh.hpp"

namespace smooth_feedback_amd {

/// One estimate point j in 1 .. Ke of one interval (dyn_error.hpp:62-67), over the `nx` state coordinates given:
///   Xest_j = X_0 + h sum_{i < Ke} F_i I(i, j - 1),  e2 += |Xest_j - X_j|^2,  x2 += |X_j|^2.
/// X holds the samples at the interval's Ke + 1 points (row p at X + p ldx), F the dynamics at the first Ke (row i at
/// F + i ldf; the end point's is never read), I the Ke x Ke integration matrix, column-major, columns ldi apart.  The
/// sums of squares are accumulated, so a caller may pass the coordinates in several pieces.
SFB_LIE_HD inline void dyn_error_point(const int Ke, const int nx, const int j, const double * X, const int64_t ldx, const double * F,
                                       const int64_t ldf, const double * I, const int64_t ldi, const double h, double & e2, double & x2)
{
  const double * Icol = I + (int64_t)(j - 1) * ldi;
  for (int d = 0; d < nx; ++d) {
    double acc = 0.0;
    for (int i = 0; i < Ke; ++i) acc += F[i * ldf + d] * Icol[i];
    const double xj = X[j * ldx + d];
    const double r  = (X[d] + h * acc) - xj;
    e2 += r * r;
    x2 += xj * xj;
  }
}

/// err = max_j e_j / (1 + max_{j >= 1} |X_j|) from the per-point sums of squares (dyn_error.hpp:66-70); a NaN in any
/// point makes the interval's estimate NaN.
SFB_LIE_HD inline double dyn_error_combine(const double max_e2, const double max_x2, const bool any_nan)
{
  if (any_nan) return NAN;
  return std::sqrt(max_e2) / (1.0 + std::sqrt(max_x2));
}

/// The whole interval on one thread: X [Ke + 1][nx], F [>= Ke][nx] (rows ldx / ldf apart), I Ke x Ke column-major, dense.
SFB_LIE_HD inline double interval_dyn_error(const int Ke, const int nx, const double * X, const int64_t ldx, const double * F,
                                            const int64_t ldf, const double * I, const double h)
{
  double me = 0.0, mx = 0.0;
  bool bad = false;
  for (int j = 1; j <= Ke; ++j) {
    double e2 = 0.0, x2 = 0.0;
    dyn_error_point(Ke, nx, j, X, ldx, F, ldf, I, Ke, h, e2, x2);
    bad = bad || e2 != e2 || x2 != x2;
    me  = e2 > me ? e2 : me;
    mx  = x2 > mx ? x2 : mx;
  }
  return dyn_error_combine(me, mx, bad);
}

/// Relative dynamics error of every interval of `mesh` for the trajectory xfun(t), ufun(t) over [t0, tf] under
/// xdot = f(t, x, u) (dyn_error.hpp:28-73).  xfun returns Vec<Nx>; ufun any Vec (Vec<0> for no input).  The estimate
/// is made on the mesh as given: callers raise the degrees first (increase_degrees), as the reference's do.
template<class F, std::size_t Kmin, std::size_t Kmax, class XF, class UF>
std::vector<double> mesh_dyn_error(F && f, const Mesh<Kmin, Kmax> & mesh, const double t0, const double tf, XF && xfun, UF && ufun)
{
  constexpr int Nx = (int)std::tuple_size_v<std::decay_t<decltype(xfun(0.0))>>;
  const std::size_t N = mesh.N_ivals();
  std::vector<double> errs(N);
  std::vector<double> X, Fv;
  for (std::size_t ival = 0; ival < N; ++ival) {
    const int Ke                   = (int)mesh.N_colloc_ival(ival);
    const std::vector<double> taus = mesh.interval_nodes(ival);
    X.assign((std::size_t)(Ke + 1) * Nx, 0.0);
    Fv.assign((std::size_t)Ke * Nx, 0.0);
    for (int j = 0; j <= Ke; ++j) {
      const double tj = t0 + (tf - t0) * taus[j];
      const auto Xj   = xfun(tj);
      for (int d = 0; d < Nx; ++d) X[(std::size_t)j * Nx + d] = Xj[d];
      if (j == Ke) break;  // the dynamics at the interval's end point are not used
      const auto Fj = f(tj, Xj, ufun(tj));
      for (int d = 0; d < Nx; ++d) Fv[(std::size_t)j * Nx + d] = Fj[d];
    }
    const MeshMat I = mesh.interval_intmat(ival);
    errs[ival]      = interval_dyn_error(Ke, Nx, X.data(), Nx, Fv.data(), Nx, I.a.data(), tf - t0);
  }
  return errs;
}

namespace detail {

/// d^r exp^-1(e) d + ad(e) dxl without forming the Dof x Dof matrices of a product group: a bundle is block diagonal
/// (the full 12 x 12 pair of a two-vehicle state is 2.3 KB per GPU lane), and on R^n the result is d itself.
template<class G>
struct FlatApply {
  SFB_LIE_HD static typename G::Tangent apply(const typename G::Tangent & e, const typename G::Tangent & d, const typename G::Tangent & dxl)
  {
    const typename G::Tangent a = G::dr_expinv(e) * d, b = G::ad(e) * dxl;
    typename G::Tangent r{};
    for (int i = 0; i < G::Dof; ++i) r[i] = a[i] + b[i];
    return r;
  }
};
template<int N>
struct FlatApply<Rn<N>> {
  SFB_LIE_HD static Vec<N> apply(const Vec<N> &, const Vec<N> & d, const Vec<N> &) { return d; }
};
template<class... Gs>
struct FlatApply<Bundle<Gs...>> {
  using B = Bundle<Gs...>;
  SFB_LIE_HD static typename B::Tangent apply(const typename B::Tangent & e, const typename B::Tangent & d, const typename B::Tangent & dxl)
  {
    typename B::Tangent r{};
    B::for_parts([&](auto I, int off) {
      using G       = std::tuple_element_t<decltype(I)::value, std::tuple<Gs...>>;
      const auto ri = FlatApply<G>::apply(B::template seg<G::Dof, 0>(e, off), B::template seg<G::Dof, 0>(d, off), B::template seg<G::Dof, 0>(dxl, off));
      for (int i = 0; i < G::Dof; ++i) r[off + i] = ri[i];
    });
    return r;
  }
};

}  // namespace detail

/// FlatDyn::operator() (ocp_flatten.hpp:166-177): the dynamics of the tangent deviation e of x = xl (+) e under
/// xdot = f(x, u), u = ul (+) v, with dxl the body velocity of the linearisation trajectory:
///   d^r exp^-1(e) (f(xl (+) e, ul (+) v) - dxl) + ad(e) dxl.
template<class F, class X, class U>
SFB_LIE_HD typename X::Tangent flat_dynamics(F && f, const X & xl, const typename X::Tangent & dxl, const U & ul, const typename X::Tangent & e,
                                             const typename U::Tangent & v)
{
  typename X::Tangent d = f(rplus(xl, e), rplus(ul, v));
  for (int i = 0; i < X::Dof; ++i) d[i] -= dxl[i];
  return detail::FlatApply<X>::apply(e, d, dxl);
}

}  // namespace smooth_feedback_amd
