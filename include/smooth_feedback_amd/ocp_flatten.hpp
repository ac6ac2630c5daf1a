// Flattening of an optimal control problem on Lie groups (reference ocp_flatten.hpp: flatten_ocp, detail::FlatDyn,
// FlatInnerFun, FlatEndptFun, unflatten_ocpsol): the problem in the tangent deviations (e, v) around a trajectory
// (xl(t), ul(t)),  x = xl(t) (+) e,  u = ul(t) (+) v,  which is a problem on Rn<Nx> x Rn<Nu> and goes through ocp_to_nlp.hpp as it is.
// Plain Vec / Mat, SFB_LIE_HD throughout: ONE law for the host front and for the kernel of ocp_flatten_device.hpp.
//
// Trajectories.  A trajectory is any type with  G operator()(double t)  and  G::Tangent velocity(double t),  the body
// velocity d^r xl_t.  The velocity is GIVEN: nothing is differentiated through the trajectory (the reference differentiates
// xl automatically).  trajectory(fn, dfn) pairs two callables, spline_trajectory(spline) adapts a Spline of spline.hpp.
// As in the reference (:171), the velocity counts as constant where a function of it is differentiated in t: the
// Jacobians below are exact for trajectories of constant body velocity and leave out d2xl otherwise.
//
// The law, with z = (t | e | v), w = f(t, x, u) - dxl, and Jf the right-Jacobian of a function on the groups in (t | x | u):
//   J(+)(t, e, v), the Jacobian of (t, xl(t) (+) e, ul(t) (+) v) (:128-136): dr_exp(e), dr_exp(v) on the diagonal and the
//     time column Ad_exp(-e) dxl, Ad_exp(-v) dul.  Never formed: its three column groups are applied to Jf directly.
//   g, cr (:352-370):          value f(t, x, u),  Jacobian Jf J(+).
//   theta, ce (:455-473):      variables (tf | e0 | ef | q), x0 = xl(0) (+) e0, xf = xl(tf) (+) ef; the time column on the xf block only.
//   dynamics (:166-216):       value  dr_expinv(e) w + ad(e) dxl   (flat_dynamics of dyn_error.hpp),
//                              Jacobian  dr_expinv(e) Jf J(+)  +  [ d/de (dr_expinv(e) w) - ad(dxl) ]  in the e columns.
//     At e = 0 the e block is  df/dx - ad(f + dxl) / 2:  dr_expinv(e) w = w - ad(w) e / 2 + O(e^2) gives -ad(w) / 2, and
//     -ad(w) / 2 - ad(dxl) = -ad(f + dxl) / 2.  tests/golden/flatten_reference.npz pins it (the points with e = 0).
//   d/de (dr_expinv(e) w): closed form on SE2 and SO3, where dr_expinv = I + ad/2 + k(th^2) ad^2 and lie.hpp has k and k':
//       -ad(w)/2 + (ad_e^2 w) (k' grad th^2)' - k (ad(ad_e w) + ad_e ad(w)).
//     On SE3 the Bernoulli recursion of the reference's Hessian (:237-273), on ad as a 6 x 6 matrix:
//       v_0 = w, D_0 = 0, v_(i+1) = ad_e v_i, D_(i+1) = ad_e D_i - ad(v_i),   sum_i c_i D_i,  c_i = B_i (-1)^i / i!,
//     through i = 26.  DOMAIN: the rotation part of e at most 1 rad.  Truncation: |c_i| < 2.1 / (2 pi)^i, and with
//     ad_e = [[W, V], [0, W]], |W| = th <= 1:  |ad_e^i| <= th^i + i th^(i-1) |v|  and  |D_i| <= i |ad_e|^(i-1) |ad(w)|,  so
//     the first term left out, i = 28, is below  2.1 * 28 (1 + 27 |v_e|) / (2 pi)^28 |ad(w)| = 2.6e-21 (1 + 27 |v_e|) |ad(w)|
//     and the tail is a geometric series of ratio (1 / 2 pi)^2 after it.  A larger rotation part is OUTSIDE the guarantee:
//     at th = 2 the same bound is 4e-13 (1 + 14 |v_e|), and the series diverges at 2 pi.
//
// Inner derivatives: a wrapped functor may carry jacobian(t, x, u, J) (end functions: jacobian(tf, x0, xf, q, J)), right-
// Jacobians on the group, columns (t | x | u) / (tf | x0 | xf | q); without one, forward differences with the step of
// xu_jacobian / mesh_function.hpp (2^-26) on the group.
// Second derivatives (the reference's flat functors carry Hessians, :221-241, :373-387, :476-490; an analytic chain rule through
// d2r_exp is out of scope here).  flatten_ocp<FlatHess::None> (the default): the flat functors have NO hessian member and d2f_dx2,
// d2g_dx2, d2l_dx2 of a flattened problem go through OCPNLP's differences of the flat values, four evaluations of the whole
// change of variables per entry.  flatten_ocp<FlatHess::Differences>: they carry hessian(t, e, v, H) / hessian(tf, e0, ef, q, H)
// in the layouts MeshModelEval and EndEval expect, and OCPNLP picks them up.  The law, built on ONE primitive, "the difference
// along direction a" (flat_inner_direction / flat_end_direction below, SFB_LIE_HD like the rest of this header), used by the
// uncontracted members and by the multiplier-contracted per-direction form (flat_contract_direction) alike:
//   inner functor with a jacobian member    H_r(a, b) = (J(z + h e_a)(r, b) - J(z - h e_a)(r, b)) / (2 h),  J the closed form of
//                                           eval() above, h = flat_hess_step = 2^-17: two Jacobians per direction
//   inner functor without one               the four-point second difference of the flat VALUES at 2^-13, the rule and step of
//                                           MeshModelEval: differencing a forward-difference Jacobian would amplify its 1e-8 noise by 1 / h
//   symmetry                                computed for a <= b; the lower triangle mirrors the upper, H(b, a) = H(a, b)
//   end functions                           the same with z = (tf | e0 | ef | q)
//   time direction                          J(z +- h e_0) is the closed-form Jacobian at t +- h, so the convention above carries
//                                           over: the body velocity counts as constant, and the second derivatives are exact (up to
//                                           the difference) for trajectories of constant body velocity, as the Jacobians are
//   contraction with multipliers            acc = 0; acc += lam[r] * d(r, b), r ascending: the order of OCPNLP::node_hessian
#pragma once
#include <functional>
#include <type_traits>
#include <utility>

#include "dyn_error.hpp"
#include "lie.hpp"
#include "ocp_to_nlp.hpp"
#include "spline.hpp"

// loops over matrix entries in code that also runs in kernels: unrolled there, so that the entries stay in registers
#if defined(__HIPCC__)
#define SFB_FLAT_UNROLL _Pragma("unroll")
#else
#define SFB_FLAT_UNROLL
#endif

namespace smooth_feedback_amd {

/// a trajectory from two callables: the curve and its body velocity
template<class Fn, class DFn>
struct TrajectoryPair {
  Fn fn;
  DFn dfn;
  SFB_LIE_HD auto operator()(double t) const { return fn(t); }
  SFB_LIE_HD auto velocity(double t) const { return dfn(t); }
};
template<class Fn, class DFn>
SFB_LIE_HD TrajectoryPair<std::decay_t<Fn>, std::decay_t<DFn>> trajectory(Fn && fn, DFn && dfn)
{
  return {std::forward<Fn>(fn), std::forward<DFn>(dfn)};
}
/// a Spline of spline.hpp as a trajectory (host; the spline is shared, not copied)
template<int K, class G>
struct SplineTrajectoryAdapter {
  const Spline<K, G> * s;
  G operator()(double t) const { return (*s)(t); }
  typename G::Tangent velocity(double t) const
  {
    typename G::Tangent vel{}, acc{};
    (void)(*s)(t, vel, acc);
    return vel;
  }
};
template<int K, class G>
SplineTrajectoryAdapter<K, G> spline_trajectory(const Spline<K, G> & s)
{
  return {&s};
}

/// agent b's trajectories out of a swarm model with xl(b, t), dxl(b, t), ul(b, t), dul(b, t) (ocp_flatten_device.hpp)
template<class Model>
struct AgentStateTrajectory {
  const Model * m;
  int64_t b;
  SFB_LIE_HD auto operator()(double t) const { return m->xl(b, t); }
  SFB_LIE_HD auto velocity(double t) const { return m->dxl(b, t); }
};
template<class Model>
struct AgentInputTrajectory {
  const Model * m;
  int64_t b;
  SFB_LIE_HD auto operator()(double t) const { return m->ul(b, t); }
  SFB_LIE_HD auto velocity(double t) const { return m->dul(b, t); }
};

/// second derivatives of the flat functors: none (OCPNLP differences the flat values) or hessian members by the law at the top
enum class FlatHess { None, Differences };

namespace detail {

inline constexpr double flat_fd_step = 1.4901161193847656e-08;  // 2^-26 = sqrt(DBL_EPSILON), the step of xu_jacobian and meshfn_fd_step()

/// Ad_exp(-e) d
template<class G>
SFB_LIE_HD typename G::Tangent flat_ad_exp_neg(const typename G::Tangent & e, const typename G::Tangent & d)
{
  if constexpr (G::IsCommutative) {
    return d;
  } else {
    typename G::Tangent me{};
    for (int i = 0; i < G::Dof; ++i) me[i] = -e[i];
    return rplus(G::Identity(), me).Ad(d);
  }
}

/// d/de (dr_expinv(e) w) for a fixed w
template<class G>
struct FlatDExpinv;
template<int N>
struct FlatDExpinv<Rn<N>> {
  SFB_LIE_HD static Mat<N, N> apply(const Vec<N> &, const Vec<N> &) { return Mat<N, N>::Zero(); }
};
/// SE2 and SO3: -ad(w)/2 + (ad_e^2 w) (k' grad th^2)' - k (ad(ad_e w) + ad_e ad(w));  grad th^2 = 2 e on SO3, (0, 0, 2 e_2) on SE2
template<class G>
SFB_LIE_HD Mat<3, 3> flat_dexpinv_rot(const Vec<3> & e, const Vec<3> & w, double th2, const Vec<3> & grad)
{
  const double k = dr_expinv_coef(th2), dk = dr_expinv_dcoef(th2);
  const Mat<3, 3> Ae = G::ad(e), Aw = G::ad(w);
  const Vec<3> y = Ae * w, yy = Ae * y;
  const Mat<3, 3> Ay = G::ad(y), AeAw = Ae * Aw;
  Mat<3, 3> m{};
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) m(r, c) = -0.5 * Aw(r, c) + yy[r] * (dk * grad[c]) - k * (Ay(r, c) + AeAw(r, c));
  return m;
}
template<>
struct FlatDExpinv<SE2> {
  SFB_LIE_HD static Mat<3, 3> apply(const Vec<3> & e, const Vec<3> & w) { return flat_dexpinv_rot<SE2>(e, w, e[2] * e[2], {0.0, 0.0, 2.0 * e[2]}); }
};
template<>
struct FlatDExpinv<SO3> {
  SFB_LIE_HD static Mat<3, 3> apply(const Vec<3> & e, const Vec<3> & w)
  {
    return flat_dexpinv_rot<SO3>(e, w, e[0] * e[0] + e[1] * e[1] + e[2] * e[2], {2.0 * e[0], 2.0 * e[1], 2.0 * e[2]});
  }
};
/// c_i = B_i (-1)^i / i! for i = 2, 4, .., 26 (c_0 = 1 multiplies D_0 = 0, c_1 = 1/2, the other odd ones vanish)
SFB_LIE_HD constexpr double flat_bernoulli_coef(int half)
{
  constexpr double c[13] = {1.0 / 12.0, -1.0 / 720.0, 1.0 / 30240.0, -1.0 / 1209600.0, 1.0 / 47900160.0, -691.0 / 1307674368000.0,
                            1.0 / 74724249600.0, -3617.0 / 10670622842880000.0, 8.586062056277845e-15, -2.174868698558062e-16,
                            5.5090028283602295e-18, -1.3954464685812522e-19, 3.534707039629467e-21};
  return c[half];
}
/// SE3: the recursion (domain and truncation bound at the top of this file)
template<>
struct FlatDExpinv<SE3> {
  SFB_LIE_HD static Mat<6, 6> apply(const Vec<6> & e, const Vec<6> & w)
  {
    const Mat<6, 6> Ae = SE3::ad(e);
    Vec<6> v      = w;
    Mat<6, 6> D   = Mat<6, 6>::Zero(), out = Mat<6, 6>::Zero();
SFB_FLAT_UNROLL
    for (int i = 1; i <= 26; ++i) {
      const Mat<6, 6> Av = SE3::ad(v);
      D                  = Ae * D;
SFB_FLAT_UNROLL
      for (int k = 0; k < 36; ++k) D.a[k] -= Av.a[k];  // D_i = ad_e D_(i-1) - ad(v_(i-1))
      v = Ae * v;
      if (i == 1 || i % 2 == 0) {
        const double c = i == 1 ? 0.5 : flat_bernoulli_coef(i / 2 - 1);
SFB_FLAT_UNROLL
        for (int k = 0; k < 36; ++k) out.a[k] += c * D.a[k];
      }
    }
    return out;
  }
};
template<class... Gs>
struct FlatDExpinv<Bundle<Gs...>> {
  using B = Bundle<Gs...>;
  SFB_LIE_HD static Mat<B::Dof, B::Dof> apply(const typename B::Tangent & e, const typename B::Tangent & w)
  {
    Mat<B::Dof, B::Dof> m{};
    B::for_parts([&](auto I, int off) {
      using G      = std::tuple_element_t<decltype(I)::value, std::tuple<Gs...>>;
      const auto b = FlatDExpinv<G>::apply(B::template seg<G::Dof, 0>(e, off), B::template seg<G::Dof, 0>(w, off));
      for (int c = 0; c < G::Dof; ++c)
        for (int r = 0; r < G::Dof; ++r) m(off + r, off + c) = b(r, c);
    });
    return m;
  }
};

/// h e_c as a tangent, and column `col` of J from a forward difference -- written with compile-time indices under a run-time
/// c (a compare per entry): the loops over difference directions stay rolled in a kernel and nothing is indexed at run time
template<int N>
SFB_LIE_HD Vec<N> flat_unit(int c, double h)
{
  Vec<N> d{};
  SFB_FLAT_UNROLL
  for (int k = 0; k < N; ++k) d[k] = (k == c) ? h : 0.0;
  return d;
}
template<int NF, int C>
SFB_LIE_HD void flat_difference_column(Mat<NF, C> & J, int col, const Vec<NF> & fa, const Vec<NF> & f0, double h)
{
  SFB_FLAT_UNROLL
  for (int k = 0; k < C; ++k)
    if (k == col) {
      SFB_FLAT_UNROLL
      for (int r = 0; r < NF; ++r) J(r, k) = (fa[r] - f0[r]) / h;
    }
}

/// value [NF] and right-Jacobian (NF x (1 + nx + nu), columns t | x | u) of fn(t, x, u) on the groups: the functor's
/// jacobian(t, x, u, J), else forward differences on the group
template<int NF, class Fn, class X, class U>
SFB_LIE_HD void flat_inner_jacobian(const Fn & fn, double t, const X & x, const U & u, Vec<NF> & val, Mat<NF, 1 + X::Dof + U::Dof> & J)
{
  constexpr int nx = X::Dof, nu = U::Dof;
  val = fn(t, x, u);
  if constexpr (requires { fn.jacobian(t, x, u, J); }) {
    fn.jacobian(t, x, u, J);
  } else {
    const double h = flat_fd_step;
    flat_difference_column(J, 0, fn(t + h, x, u), val, h);
    for (int c = 0; c < nx; ++c) flat_difference_column(J, 1 + c, fn(t, rplus(x, flat_unit<nx>(c, h)), u), val, h);
    for (int c = 0; c < nu; ++c) flat_difference_column(J, 1 + nx + c, fn(t, x, rplus(u, flat_unit<nu>(c, h))), val, h);
  }
}

/// Jf J(+) for an inner function: Jf (NF x (1 + nx + nu)) on the groups -> the Jacobian in (t | e | v)
template<int NF, class X, class U>
SFB_LIE_HD Mat<NF, 1 + X::Dof + U::Dof> flat_chain_inner(const Mat<NF, 1 + X::Dof + U::Dof> & Jf, const typename X::Tangent & e,
                                                         const typename U::Tangent & v, const typename X::Tangent & dxl,
                                                         const typename U::Tangent & dul)
{
  constexpr int nx = X::Dof, nu = U::Dof;
  const typename X::Tangent ax = flat_ad_exp_neg<X>(e, dxl);
  const typename U::Tangent au = flat_ad_exp_neg<U>(v, dul);
  Mat<NF, 1 + nx + nu> J{};
  for (int r = 0; r < NF; ++r) {
    double acc = Jf(r, 0);
    for (int k = 0; k < nx; ++k) acc += Jf(r, 1 + k) * ax[k];
    for (int k = 0; k < nu; ++k) acc += Jf(r, 1 + nx + k) * au[k];
    J(r, 0) = acc;
  }
  if constexpr (X::IsCommutative) {
    for (int c = 0; c < nx; ++c)
      for (int r = 0; r < NF; ++r) J(r, 1 + c) = Jf(r, 1 + c);
  } else {
    const Mat<nx, nx> Ex = X::dr_exp(e);
    for (int c = 0; c < nx; ++c)
      for (int r = 0; r < NF; ++r) {
        double acc = 0.0;
        for (int k = 0; k < nx; ++k) acc += Jf(r, 1 + k) * Ex(k, c);
        J(r, 1 + c) = acc;
      }
  }
  if constexpr (U::IsCommutative) {
    for (int c = 0; c < nu; ++c)
      for (int r = 0; r < NF; ++r) J(r, 1 + nx + c) = Jf(r, 1 + nx + c);
  } else {
    const Mat<nu, nu> Eu = U::dr_exp(v);
    for (int c = 0; c < nu; ++c)
      for (int r = 0; r < NF; ++r) {
        double acc = 0.0;
        for (int k = 0; k < nu; ++k) acc += Jf(r, 1 + nx + k) * Eu(k, c);
        J(r, 1 + nx + c) = acc;
      }
  }
  return J;
}

// ---- second derivatives: the difference along direction a (the law at the top of this file) ----
// eps^(1/3) = 2^-17.33 balances the central difference of a Jacobian known to eps: truncation h^2 |d3J| / 6 against rounding
// eps |J| / h.  The nearest power of two, so that z + h e_a and z - h e_a are exact and 2 h divides exactly.
inline constexpr double flat_hess_step = 7.62939453125e-06;  // 2^-17
// eps^(1/4), the step of MeshModelEval's and EndEval's four-point second difference of values (sqrt of their 2^-26)
inline constexpr double flat_hess_value_step = 1.220703125e-04;  // 2^-13

/// z[c] += d as a compare-select over the entries, never a run-time index (c outside [0, N): nothing)
template<int N>
SFB_LIE_HD void flat_bump(Vec<N> & z, int c, double d)
{
  SFB_FLAT_UNROLL
  for (int k = 0; k < N; ++k) z[k] += (k == c) ? d : 0.0;
}

/// D (NF x nv) of a flat inner functor `fun` (FlatDyn, FlatInnerFun) along direction a of z = (t | e | v).  With a jacobian
/// member in the wrapped functor: D = (J(z + h e_a) - J(z - h e_a)) / (2 h), every column.  Without: columns b >= a hold the
/// four-point second difference of the values in (a, b), the others 0.  Row r of the Hessians: H_r(a, b) = D(r, b), b >= a.
template<int NF, class Fun>
SFB_LIE_HD void flat_inner_direction(const Fun & fun, double t, const Rn<Fun::Nx> & e, const Rn<Fun::Nu> & v, int a, Mat<NF, Fun::nv> & D)
{
  constexpr int Nx = Fun::Nx, Nu = Fun::Nu, nv = Fun::nv;
  if constexpr (Fun::inner_has_jacobian) {
    const double h = flat_hess_step;
    Rn<Nx> ep = e, em = e;
    Rn<Nu> vp = v, vm = v;
    const double dt = (a == 0) ? h : 0.0;
    flat_bump<Nx>(ep.v, a - 1, h), flat_bump<Nx>(em.v, a - 1, -h);
    flat_bump<Nu>(vp.v, a - 1 - Nx, h), flat_bump<Nu>(vm.v, a - 1 - Nx, -h);
    Vec<NF> val;
    Mat<NF, nv> Jm;
    fun.eval(t + dt, ep, vp, val, D);
    fun.eval(t - dt, em, vm, val, Jm);
    SFB_FLAT_UNROLL
    for (int k = 0; k < NF * nv; ++k) D.a[k] = (D.a[k] - Jm.a[k]) / (2 * h);
  } else {
    const double h = flat_hess_value_step;
    D = Mat<NF, nv>::Zero();
    const auto at = [&](double sa, double sb, int b) {
      Rn<Nx> es = e;
      Rn<Nu> vs = v;
      const double dt = ((a == 0) ? sa : 0.0) + ((b == 0) ? sb : 0.0);
      Vec<Nx> de{};
      Vec<Nu> dv{};
      flat_bump<Nx>(de, a - 1, sa), flat_bump<Nx>(de, b - 1, sb);
      flat_bump<Nu>(dv, a - 1 - Nx, sa), flat_bump<Nu>(dv, b - 1 - Nx, sb);
      SFB_FLAT_UNROLL
      for (int k = 0; k < Nx; ++k) es.v[k] += de[k];
      SFB_FLAT_UNROLL
      for (int k = 0; k < Nu; ++k) vs.v[k] += dv[k];
      return fun(t + dt, es, vs);
    };
    for (int b = 0; b < nv; ++b) {  // stays rolled in device code: the body is the flat function four times
      if (b < a) continue;
      const Vec<NF> pp = at(h, h, b), pm = at(h, -h, b), mp = at(-h, h, b), mm = at(-h, -h, b);
      SFB_FLAT_UNROLL
      for (int k = 0; k < nv; ++k)
        if (k == b) {
          SFB_FLAT_UNROLL
          for (int r = 0; r < NF; ++r) D(r, k) = ((pp[r] - pm[r]) - (mp[r] - mm[r])) / (4 * h * h);
        }
    }
  }
}

/// the same for a flat end functor (FlatEndptFun), z = (tf | e0 | ef | q)
template<int R, class Fun>
SFB_LIE_HD void flat_end_direction(const Fun & fun, double tf, const Rn<Fun::Nx> & e0, const Rn<Fun::Nx> & ef, const Vec<Fun::nq> & q, int a, Mat<R, Fun::ne> & D)
{
  constexpr int Nx = Fun::Nx, Nq = Fun::nq, ne = Fun::ne;
  if constexpr (Fun::inner_has_jacobian) {
    const double h = flat_hess_step;
    Rn<Nx> e0p = e0, e0m = e0, efp = ef, efm = ef;
    Vec<Nq> qp = q, qm = q;
    const double dt = (a == 0) ? h : 0.0;
    flat_bump<Nx>(e0p.v, a - 1, h), flat_bump<Nx>(e0m.v, a - 1, -h);
    flat_bump<Nx>(efp.v, a - 1 - Nx, h), flat_bump<Nx>(efm.v, a - 1 - Nx, -h);
    flat_bump<Nq>(qp, a - 1 - 2 * Nx, h), flat_bump<Nq>(qm, a - 1 - 2 * Nx, -h);
    Vec<R> val;
    Mat<R, ne> Jm;
    fun.eval(tf + dt, e0p, efp, qp, val, D);
    fun.eval(tf - dt, e0m, efm, qm, val, Jm);
    SFB_FLAT_UNROLL
    for (int k = 0; k < R * ne; ++k) D.a[k] = (D.a[k] - Jm.a[k]) / (2 * h);
  } else {
    const double h = flat_hess_value_step;
    D = Mat<R, ne>::Zero();
    const auto at = [&](double sa, double sb, int b) {
      Rn<Nx> e0s = e0, efs = ef;
      Vec<Nq> qs = q;
      const double dt = ((a == 0) ? sa : 0.0) + ((b == 0) ? sb : 0.0);
      Vec<Nx> d0{}, df{};
      Vec<Nq> dq{};
      flat_bump<Nx>(d0, a - 1, sa), flat_bump<Nx>(d0, b - 1, sb);
      flat_bump<Nx>(df, a - 1 - Nx, sa), flat_bump<Nx>(df, b - 1 - Nx, sb);
      flat_bump<Nq>(dq, a - 1 - 2 * Nx, sa), flat_bump<Nq>(dq, b - 1 - 2 * Nx, sb);
      SFB_FLAT_UNROLL
      for (int k = 0; k < Nx; ++k) e0s.v[k] += d0[k], efs.v[k] += df[k];
      SFB_FLAT_UNROLL
      for (int k = 0; k < Nq; ++k) qs[k] += dq[k];
      return Fun::as_vec_flat(fun, tf + dt, e0s, efs, qs);
    };
    for (int b = 0; b < ne; ++b) {
      if (b < a) continue;
      const Vec<R> pp = at(h, h, b), pm = at(h, -h, b), mp = at(-h, h, b), mm = at(-h, -h, b);
      SFB_FLAT_UNROLL
      for (int k = 0; k < ne; ++k)
        if (k == b) {
          SFB_FLAT_UNROLL
          for (int r = 0; r < R; ++r) D(r, k) = ((pp[r] - pm[r]) - (mp[r] - mm[r])) / (4 * h * h);
        }
    }
  }
}

/// row[b] = sum_r lam[r] D(r, b): acc = 0, r ascending (OCPNLP::node_hessian): row a of a contracted square, from b = a on
template<int NF, int NV>
SFB_LIE_HD void flat_contract_direction(const Mat<NF, NV> & D, const double * lam, Vec<NV> & row)
{
  SFB_FLAT_UNROLL
  for (int b = 0; b < NV; ++b) {
    double acc = 0.0;
    SFB_FLAT_UNROLL
    for (int r = 0; r < NF; ++r) acc += lam[r] * D(r, b);
    row[b] = acc;
  }
}

/// the uncontracted squares from the directions: H (NV x NF NV, side by side), upper triangle computed, lower mirrored
template<int NF, int NV, class Dir>
SFB_LIE_HD void flat_hessian_from_directions(Mat<NV, NF * NV> & H, Dir && direction)
{
  for (int a = 0; a < NV; ++a) {
    Mat<NF, NV> D;
    direction(a, D);
    for (int r = 0; r < NF; ++r)
      for (int b = a; b < NV; ++b) H(a, r * NV + b) = H(b, r * NV + a) = D(r, b);
  }
}

/// g or cr of the flattened problem (FlatInnerFun)
template<class X, class U, int NF, class Fn, class Xl, class Ul, FlatHess HM = FlatHess::None>
struct FlatInnerFun {
  static constexpr int Nx = X::Dof, Nu = U::Dof, nv = 1 + Nx + Nu;
  static constexpr bool inner_has_jacobian = requires(const Fn & fn, const X & x, const U & u, Mat<NF, nv> & J) { fn.jacobian(0.0, x, u, J); };
  Fn f;
  Xl xl;
  Ul ul;
  SFB_LIE_HD Vec<NF> operator()(double t, const Rn<Nx> & e, const Rn<Nu> & v) const { return f(t, rplus(xl(t), e.v), rplus(ul(t), v.v)); }
  SFB_LIE_HD void jacobian(double t, const Rn<Nx> & e, const Rn<Nu> & v, Mat<NF, nv> & J) const
  {
    Vec<NF> val;
    eval(t, e, v, val, J);
  }
  /// value and Jacobian in one pass (what the device kernel calls)
  SFB_LIE_HD void eval(double t, const Rn<Nx> & e, const Rn<Nu> & v, Vec<NF> & val, Mat<NF, nv> & J) const
  {
    Mat<NF, nv> Jf{};
    flat_inner_jacobian<NF>(f, t, rplus(xl(t), e.v), rplus(ul(t), v.v), val, Jf);
    J = flat_chain_inner<NF, X, U>(Jf, e.v, v.v, xl.velocity(t), ul.velocity(t));
  }
  /// the Hessians of the NF rows side by side (MeshModelEval's layout), FlatHess::Differences only
  SFB_LIE_HD void hessian(double t, const Rn<Nx> & e, const Rn<Nu> & v, Mat<nv, NF * nv> & H) const
    requires(HM == FlatHess::Differences)
  {
    flat_hessian_from_directions<NF, nv>(H, [&](int a, Mat<NF, nv> & D) { flat_inner_direction<NF>(*this, t, e, v, a, D); });
  }
};

/// the dynamics of the flattened problem (FlatDyn)
template<class X, class U, class Fn, class Xl, class Ul, FlatHess HM = FlatHess::None>
struct FlatDyn {
  static constexpr int Nx = X::Dof, Nu = U::Dof, nv = 1 + Nx + Nu;
  static constexpr bool inner_has_jacobian = requires(const Fn & fn, const X & x, const U & u, Mat<Nx, nv> & J) { fn.jacobian(0.0, x, u, J); };
  Fn f;
  Xl xl;
  Ul ul;
  SFB_LIE_HD Vec<Nx> operator()(double t, const Rn<Nx> & e, const Rn<Nu> & v) const
  {
    return flat_dynamics([&](const X & x, const U & u) { return f(t, x, u); }, xl(t), xl.velocity(t), ul(t), e.v, v.v);
  }
  SFB_LIE_HD void jacobian(double t, const Rn<Nx> & e, const Rn<Nu> & v, Mat<Nx, nv> & J) const
  {
    Vec<Nx> val;
    eval(t, e, v, val, J);
  }
  SFB_LIE_HD void eval(double t, const Rn<Nx> & e, const Rn<Nu> & v, Vec<Nx> & val, Mat<Nx, nv> & J) const
  {
    const typename X::Tangent dxl = xl.velocity(t);
    Vec<Nx> fv;
    Mat<Nx, nv> Jf{};
    flat_inner_jacobian<Nx>(f, t, rplus(xl(t), e.v), rplus(ul(t), v.v), fv, Jf);
    Vec<Nx> w = fv;
    for (int i = 0; i < Nx; ++i) w[i] -= dxl[i];
    val = FlatApply<X>::apply(e.v, w, dxl);  // the value as flat_dynamics forms it
    const Mat<Nx, nv> Jc = flat_chain_inner<Nx, X, U>(Jf, e.v, v.v, dxl, ul.velocity(t));
    if constexpr (X::IsCommutative) {
      J = Jc;
    } else {
      J = X::dr_expinv(e.v) * Jc;
      const Mat<Nx, Nx> De = FlatDExpinv<X>::apply(e.v, w), Ad = X::ad(dxl);
      for (int c = 0; c < Nx; ++c)
        for (int r = 0; r < Nx; ++r) J(r, 1 + c) += De(r, c) - Ad(r, c);
    }
  }
  SFB_LIE_HD void hessian(double t, const Rn<Nx> & e, const Rn<Nu> & v, Mat<nv, Nx * nv> & H) const
    requires(HM == FlatHess::Differences)
  {
    flat_hessian_from_directions<Nx, nv>(H, [&](int a, Mat<Nx, nv> & D) { flat_inner_direction<Nx>(*this, t, e, v, a, D); });
  }
};

/// theta (Scalar: returns double) or ce of the flattened problem (FlatEndptFun), variables (tf | e0 | ef | q)
template<class X, int Nq, int R, bool Scalar, class Fn, class Xl, FlatHess HM = FlatHess::None>
struct FlatEndptFun {
  static constexpr int Nx = X::Dof, nq = Nq, ne = 1 + 2 * Nx + Nq;
  static constexpr bool inner_has_jacobian =
    requires(const Fn & fn, const X & x, const Vec<Nq> & q, Mat<R, ne> & J) { fn.jacobian(0.0, x, x, q, J); };
  Fn f;
  Xl xl;
  SFB_LIE_HD static Vec<R> as_vec(const Fn & fn, double tf, const X & x0, const X & xf, const Vec<Nq> & q)
  {
    if constexpr (Scalar) return Vec<R>{fn(tf, x0, xf, q)};
    else return fn(tf, x0, xf, q);
  }
  SFB_LIE_HD auto operator()(double tf, const Rn<Nx> & e0, const Rn<Nx> & ef, const Vec<Nq> & q) const
  {
    return f(tf, rplus(xl(0.0), e0.v), rplus(xl(tf), ef.v), q);
  }
  /// the flat value as a vector, scalar or not
  SFB_LIE_HD static Vec<R> as_vec_flat(const FlatEndptFun & fun, double tf, const Rn<Nx> & e0, const Rn<Nx> & ef, const Vec<Nq> & q)
  {
    if constexpr (Scalar) return Vec<R>{fun(tf, e0, ef, q)};
    else return fun(tf, e0, ef, q);
  }
  SFB_LIE_HD void jacobian(double tf, const Rn<Nx> & e0, const Rn<Nx> & ef, const Vec<Nq> & q, Mat<R, ne> & J) const
  {
    Vec<R> val;
    eval(tf, e0, ef, q, val, J);
  }
  SFB_LIE_HD void eval(double tf, const Rn<Nx> & e0, const Rn<Nx> & ef, const Vec<Nq> & q, Vec<R> & val, Mat<R, ne> & J) const
  {
    const X x0 = rplus(xl(0.0), e0.v), xf = rplus(xl(tf), ef.v);
    val = as_vec(f, tf, x0, xf, q);
    Mat<R, ne> Jf{};
    if constexpr (requires { f.jacobian(tf, x0, xf, q, Jf); }) {
      f.jacobian(tf, x0, xf, q, Jf);
    } else {
      const double h = flat_fd_step;
      flat_difference_column(Jf, 0, as_vec(f, tf + h, x0, xf, q), val, h);
      for (int c = 0; c < Nx; ++c) {
        const typename X::Tangent d = flat_unit<Nx>(c, h);
        flat_difference_column(Jf, 1 + c, as_vec(f, tf, rplus(x0, d), xf, q), val, h);
        flat_difference_column(Jf, 1 + Nx + c, as_vec(f, tf, x0, rplus(xf, d), q), val, h);
      }
      for (int c = 0; c < Nq; ++c) {
        Vec<Nq> qa       = q;
        const Vec<Nq> dq = flat_unit<Nq>(c, h);
        for (int k = 0; k < Nq; ++k) qa[k] += dq[k];
        flat_difference_column(Jf, 1 + 2 * Nx + c, as_vec(f, tf, x0, xf, qa), val, h);
      }
    }
    const typename X::Tangent af = flat_ad_exp_neg<X>(ef.v, xl.velocity(tf));
    const Mat<Nx, Nx> E0 = X::dr_exp(e0.v), Ef = X::dr_exp(ef.v);
    for (int r = 0; r < R; ++r) {
      double acc = Jf(r, 0);
      for (int k = 0; k < Nx; ++k) acc += Jf(r, 1 + Nx + k) * af[k];
      J(r, 0) = acc;
      for (int c = 0; c < Nx; ++c) {
        double a0 = 0.0, a1 = 0.0;
        for (int k = 0; k < Nx; ++k) a0 += Jf(r, 1 + k) * E0(k, c), a1 += Jf(r, 1 + Nx + k) * Ef(k, c);
        J(r, 1 + c) = a0, J(r, 1 + Nx + c) = a1;
      }
      for (int c = 0; c < Nq; ++c) J(r, 1 + 2 * Nx + c) = Jf(r, 1 + 2 * Nx + c);
    }
  }
  /// the Hessians of the R rows side by side (EndEval's layout), FlatHess::Differences only
  SFB_LIE_HD void hessian(double tf, const Rn<Nx> & e0, const Rn<Nx> & ef, const Vec<Nq> & q, Mat<ne, R * ne> & H) const
    requires(HM == FlatHess::Differences)
  {
    flat_hessian_from_directions<R, ne>(H, [&](int a, Mat<R, ne> & D) { flat_end_direction<R>(*this, tf, e0, ef, q, a, D); });
  }
};

}  // namespace detail

/// the flattened problem: the members of OCP<...> of ocp_to_qp.hpp on X = Rn<Nx>, U = Rn<Nu>
template<class GX, class GU, int Nq_, int Ncr_, int Nce_, class Theta, class F, class G, class CR, class CE>
struct FlatOCP {
  using X = Rn<GX::Dof>;
  using U = Rn<GU::Dof>;
  using GroupX = GX;
  using GroupU = GU;
  static constexpr int Nx = GX::Dof, Nu = GU::Dof, Nq = Nq_, Ncr = Ncr_, Nce = Nce_;
  Theta theta;
  F f;
  G g;
  CR cr;
  Vec<Ncr> crl{}, cru{};
  CE ce;
  Vec<Nce> cel{}, ceu{};
};

/// flatten_ocp (:513-541): the problem in (e, v) around the trajectories xl, ul; sizes Nq, Ncr, Nce >= 1.
/// flatten_ocp<FlatHess::Differences>(ocp, xl, ul): the flat functors carry hessian members (the law at the top).
template<FlatHess HM = FlatHess::None, class Ocp, class Xl, class Ul>
SFB_LIE_HD auto flatten_ocp(const Ocp & ocp, const Xl & xl, const Ul & ul)
{
  using X = typename Ocp::X;
  using U = typename Ocp::U;
  constexpr int Nq = Ocp::Nq, Ncr = Ocp::Ncr, Nce = Ocp::Nce;
  static_assert(Nq >= 1 && Ncr >= 1 && Nce >= 1, "flatten_ocp: Nq, Ncr, Nce >= 1");
  using Theta = detail::FlatEndptFun<X, Nq, 1, true, std::decay_t<decltype(ocp.theta)>, Xl, HM>;
  using F     = detail::FlatDyn<X, U, std::decay_t<decltype(ocp.f)>, Xl, Ul, HM>;
  using G     = detail::FlatInnerFun<X, U, Nq, std::decay_t<decltype(ocp.g)>, Xl, Ul, HM>;
  using CR    = detail::FlatInnerFun<X, U, Ncr, std::decay_t<decltype(ocp.cr)>, Xl, Ul, HM>;
  using CE    = detail::FlatEndptFun<X, Nq, Nce, false, std::decay_t<decltype(ocp.ce)>, Xl, HM>;
  return FlatOCP<X, U, Nq, Ncr, Nce, Theta, F, G, CR, CE>{Theta{ocp.theta, xl}, F{ocp.f, xl, ul},   G{ocp.g, xl, ul}, CR{ocp.cr, xl, ul},
                                                          ocp.crl,              ocp.cru,           CE{ocp.ce, xl},   ocp.cel,
                                                          ocp.ceu};
}

/// unflatten_ocpsol (:549-573): x(t) = xl(t) (+) e(t), u(t) = ul(t) (+) v(t); everything else is carried over
template<class X, class U, int Nq, int Ncr, int Nce, class Xl, class Ul>
OCPNLPSolution<X, U, Nq, Ncr, Nce> unflatten_ocpsol(const OCPNLPSolution<Rn<X::Dof>, Rn<U::Dof>, Nq, Ncr, Nce> & flatsol, Xl xl, Ul ul)
{
  OCPNLPSolution<X, U, Nq, Ncr, Nce> out;
  out.t0 = flatsol.t0, out.tf = flatsol.tf, out.Q = flatsol.Q;
  out.u          = [ul, usol = flatsol.u](double t) -> U { return rplus(ul(t), usol(t).v); };
  out.x          = [xl, xsol = flatsol.x](double t) -> X { return rplus(xl(t), xsol(t).v); };
  out.lambda_q   = flatsol.lambda_q;
  out.lambda_ce  = flatsol.lambda_ce;
  out.lambda_dyn = flatsol.lambda_dyn;
  out.lambda_cr  = flatsol.lambda_cr;
  return out;
}

}  // namespace smooth_feedback_amd
