// Re-linearisation of an MPC problem about a PLAN instead of about the desired trajectory: the law of sequential convex
// MPC, once, for the host front (MPC::fill_flat_record, mpc.hpp) and for the kernel (mpc_relinearise_kernel,
// mpc_device.hpp).  Plain Vec / Mat, SFB_LIE_HD throughout.
//
// The unknowns of every pass stay the tangent deviations e = x (-) xdes, v = u (-) udes, so the quadratic cost is exact
// in them and P, q never change.  With the flat dynamics of ocp_flatten.hpp,
//   F(e, v) = dr_expinv(e) (f(xdes (+) e, udes (+) v) - dxdes) + ad(e) dxdes,       de/dt = F(e, v),
// and a plan (ebar_i, vbar_i) at node i, the pass solves the QP whose rows are the first-order model of F and of the
// running constraint about that plan:
//   A_i = dF/de, B_i = dF/dv at (ebar_i, vbar_i)      FlatDyn::eval with xl = xdes, dxl = dxdes, ul = udes, dul = 0
//   f0_i = F(ebar_i, vbar_i) - A_i ebar_i - B_i vbar_i
//   C_i, D_i = d cr / d(e, v) at the plan               FlatInnerFun::eval
//   c0_i = cr(xdes (+) ebar_i, udes (+) vbar_i) - C_i ebar_i - D_i vbar_i
// The time column of the flat Jacobians is not used (and MPCDes carries no dudes: zero).  These go into the record of
// sfb.h with dfdx := A, dfdu := B, f := f0, dxdes := 0, c := c0, dcdx := C, dcdu := D, assembled in the commutative
// mode (no ad(f + dxdes) term: the flat Jacobian already holds the group terms), which gives the rows
//   sum_j alpha D(j, i) e_j = tf (A_i e_i + B_i v_i + f0_i),      crl <= C_i e_i + D_i v_i + c0_i <= cru.
// The initial state is pinned exactly, e_0 = log(xdes(t)^-1 x): the x0 rows get J = I and the record's
// e = xdes(t) (-) x = -e_0 (the assembled row is J e_0 = 0 - e).
// At ebar = vbar = 0 this is the pass-one problem (the e block is df/dx - ad(f + dxdes) / 2), x0 rows apart.
//
// Summation orders are part of the law (the host loop and the kernel are compared bit for bit up to the maths
// libraries' sin / cos):  acc = F[r];  acc -= A(r, c) * ebar[c], c ascending;  then acc -= B(r, c) * vbar[c], c ascending.
#pragma once
#include "lie.hpp"
#include "ocp_flatten.hpp"

// forced inline where the law runs per lane in a kernel: an out-of-line call would hand pointers into a lane's private
// memory across a call boundary
#if defined(__HIPCC__)
#define SFB_RELIN_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define SFB_RELIN_HD inline
#endif

namespace smooth_feedback_amd {
namespace detail {

template<int NO, class Fn, class X, class U>
SFB_LIE_HD void xu_jacobian(const Fn & fn, const X & x, const U & u, Vec<NO> & val, Mat<NO, X::Dof> & dx, Mat<NO, U::Dof> & du);  // mpc.hpp

/// a time-invariant functor fn(x, u) of the MPC front as the fn(t, x, u) the flat functors wrap; its Jacobian is
/// xu_jacobian's (the functor's own, else forward differences), the time column zero
template<class Fn, class X, class U>
struct RelinInner {
  Fn fn;
  SFB_RELIN_HD auto operator()(double, const X & x, const U & u) const { return fn(x, u); }
  template<int NO>
  SFB_RELIN_HD void jacobian(double, const X & x, const U & u, Mat<NO, 1 + X::Dof + U::Dof> & J) const
  {
    Vec<NO> val;
    Mat<NO, X::Dof> dx;
    Mat<NO, U::Dof> du;
    xu_jacobian<NO>(fn, x, u, val, dx, du);
    SFB_FLAT_UNROLL
    for (int r = 0; r < NO; ++r) {
      J(r, 0) = 0.0;
      SFB_FLAT_UNROLL
      for (int c = 0; c < X::Dof; ++c) J(r, 1 + c) = dx(r, c);
      SFB_FLAT_UNROLL
      for (int c = 0; c < U::Dof; ++c) J(r, 1 + X::Dof + c) = du(r, c);
    }
  }
};

/// the linearisation point of ONE node as a trajectory: the values the caller evaluated at the node's time
template<class G>
struct RelinPoint {
  G g;
  typename G::Tangent vel;
  SFB_RELIN_HD G operator()(double) const { return g; }
  SFB_RELIN_HD typename G::Tangent velocity(double) const { return vel; }
};

/// val0 = val - Je ebar - Jv vbar in the order of the law; Je, Jv = the e and v columns of the flat Jacobian J (t | e | v)
template<int NO, int Nx, int Nu>
SFB_RELIN_HD void relin_split(const Vec<NO> & val, const Mat<NO, 1 + Nx + Nu> & J, const Vec<Nx> & ebar, const Vec<Nu> & vbar, Vec<NO> & val0,
                              Mat<NO, Nx> & Je, Mat<NO, Nu> & Jv)
{
  SFB_FLAT_UNROLL
  for (int r = 0; r < NO; ++r) {
    double acc = val[r];
    SFB_FLAT_UNROLL
    for (int c = 0; c < Nx; ++c) {
      Je(r, c) = J(r, 1 + c);
      acc -= Je(r, c) * ebar[c];
    }
    SFB_FLAT_UNROLL
    for (int c = 0; c < Nu; ++c) {
      Jv(r, c) = J(r, 1 + Nx + c);
      acc -= Jv(r, c) * vbar[c];
    }
    val0[r] = acc;
  }
}

/// dynamics of one node: A, B, f0 about (ebar, vbar) at the linearisation point (xl, dxl, ul)
template<class X, class U, class F>
SFB_RELIN_HD void relin_dyn_node(const F & f, const X & xl, const typename X::Tangent & dxl, const U & ul, const Vec<X::Dof> & ebar,
                                 const Vec<U::Dof> & vbar, Vec<X::Dof> & f0, Mat<X::Dof, X::Dof> & A, Mat<X::Dof, U::Dof> & B)
{
  constexpr int Nx = X::Dof, Nu = U::Dof;
  const FlatDyn<X, U, RelinInner<F, X, U>, RelinPoint<X>, RelinPoint<U>> fd{{f}, {xl, dxl}, {ul, typename U::Tangent{}}};
  Rn<Nx> e;
  Rn<Nu> v;
  e.v = ebar, v.v = vbar;
  Vec<Nx> val;
  Mat<Nx, 1 + Nx + Nu> J;
#if defined(__HIPCC__)
  [[clang::always_inline]] fd.eval(0.0, e, v, val, J);
#else
  fd.eval(0.0, e, v, val, J);
#endif
  relin_split<Nx, Nx, Nu>(val, J, ebar, vbar, f0, A, B);
}

/// running constraint of one node: C, D, c0 about (ebar, vbar)
template<class X, class U, int Ncr, class CR>
SFB_RELIN_HD void relin_cr_node(const CR & cr, const X & xl, const typename X::Tangent & dxl, const U & ul, const Vec<X::Dof> & ebar,
                                const Vec<U::Dof> & vbar, Vec<Ncr> & c0, Mat<Ncr, X::Dof> & C, Mat<Ncr, U::Dof> & D)
{
  constexpr int Nx = X::Dof, Nu = U::Dof;
  const FlatInnerFun<X, U, Ncr, RelinInner<CR, X, U>, RelinPoint<X>, RelinPoint<U>> fc{{cr}, {xl, dxl}, {ul, typename U::Tangent{}}};
  Rn<Nx> e;
  Rn<Nu> v;
  e.v = ebar, v.v = vbar;
  Vec<Ncr> val;
  Mat<Ncr, 1 + Nx + Nu> J;
#if defined(__HIPCC__)
  [[clang::always_inline]] fc.eval(0.0, e, v, val, J);
#else
  fc.eval(0.0, e, v, val, J);
#endif
  relin_split<Ncr, Nx, Nu>(val, J, ebar, vbar, c0, C, D);
}

/// which plans a pass re-linearises about: those the swarm keeps (Optimal, MaxTime, MaxIterations: mpc.hpp:510-516); an
/// agent with any other code is re-linearised about the desired trajectory itself (ebar = vbar = 0)
SFB_RELIN_HD bool relin_plan_kept(int code) { return code == 0 || code == 4 || code == 5; }

}  // namespace detail
}  // namespace smooth_feedback_amd
