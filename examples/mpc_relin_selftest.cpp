// Stand-alone driver of the re-linearisation law (include/smooth_feedback_amd/mpc_relin.hpp) for sanitizer builds:
//   g++ -std=c++20 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I examples examples/mpc_relin_selftest.cpp
// relin_dyn_node / relin_cr_node -- what MPC::fill_flat_record and mpc_relinearise_kernel call per node -- on the planar
// vehicle (SE2 x R^3) and on two of them, about plans with rotation parts 0, 1e-9, 0.3 and 1.0 at three node times, written
// into a record of the unpacked layout.  Checked: everything finite; f0 + A ebar + B vbar gives back flat_dynamics; A and B
// against central differences of flat_dynamics; at ebar = 0 the e block is df/dx - ad(f + dxdes) / 2; the running constraint
// likewise.  Host only, header-only: links nothing of the library.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vehicle_model.h"

using namespace smooth_feedback_amd;

namespace {

int failures = 0;
void expect(bool ok, const char * what, double figure)
{
  if (!ok) {
    std::printf("FAILED: %s (%.3e)\n", what, figure);
    ++failures;
  }
}

template<class Model>
void run(const char * name)
{
  using X = decltype(std::declval<const Model &>().xdes(0.0));
  using U = decltype(std::declval<const Model &>().udes(0.0));
  constexpr int Nx = X::Dof, Nu = U::Dof, Ncr = 2, N = 3;
  const Model mdl{};
  const double rot[4] = {0.0, 1e-9, 0.3, 1.0}, tau[N] = {0.0, 0.4, 1.7};
  // the record of sfb.h for N nodes, filled as MPC::fill_flat_record fills it
  const size_t o_f = 0, o_dx = o_f + N * Nx, o_dfdx = o_dx + N * Nx, o_dfdu = o_dfdx + N * Nx * Nx, o_c = o_dfdu + N * Nx * Nu,
               o_dcdx = o_c + N * Ncr, o_dcdu = o_dcdx + N * Ncr * Nx, o_e = o_dcdu + N * Ncr * Nu, o_J = o_e + Nx;
  double worst_split = 0, worst_fd = 0, worst_zero = 0, worst_cr = 0;
  for (int k = 0; k < 4; ++k) {
    std::vector<double> rec(o_J + Nx * Nx, std::nan(""));
    for (int node = 0; node < N; ++node) {
      const double ti = 0.3 + tau[node];
      const X xl      = mdl.xdes(ti);
      const auto dxl  = mdl.dxdes(ti);
      const U ul      = mdl.udes(ti);
      Vec<Nx> ebar{};
      Vec<Nu> vbar{};
      if (k > 0) {
        for (int d = 0; d < Nx; ++d) ebar[d] = 0.2 * std::sin(1.0 + d + node);
        for (int d = 2; d < Nx; d += 6) ebar[d] = rot[k] * ((d / 6) % 2 ? -1.0 : 1.0);  // the rotation component of every SE2 part
        for (int d = 0; d < Nu; ++d) vbar[d] = 0.3 * std::cos(2.0 + d + node);
      }
      Vec<Nx> f0;
      Mat<Nx, Nx> A;
      Mat<Nx, Nu> B;
      detail::relin_dyn_node<X, U>(mdl.f, xl, dxl, ul, ebar, vbar, f0, A, B);
      Vec<Ncr> c0;
      Mat<Ncr, Nx> C;
      Mat<Ncr, Nu> D;
      detail::relin_cr_node<X, U, Ncr>(mdl.cr, xl, dxl, ul, ebar, vbar, c0, C, D);
      for (int d = 0; d < Nx; ++d) {
        rec[o_f + node * Nx + d]  = f0[d];
        rec[o_dx + node * Nx + d] = 0.0;
        for (int c = 0; c < Nx; ++c) rec[o_dfdx + (node * Nx + d) * Nx + c] = A(d, c);
        for (int c = 0; c < Nu; ++c) rec[o_dfdu + (node * Nx + d) * Nu + c] = B(d, c);
      }
      for (int d = 0; d < Ncr; ++d) {
        rec[o_c + node * Ncr + d] = c0[d];
        for (int c = 0; c < Nx; ++c) rec[o_dcdx + (node * Ncr + d) * Nx + c] = C(d, c);
        for (int c = 0; c < Nu; ++c) rec[o_dcdu + (node * Ncr + d) * Nu + c] = D(d, c);
      }
      // f0 + A ebar + B vbar = F
      const auto F = flat_dynamics(mdl.f, xl, dxl, ul, ebar, vbar);
      for (int d = 0; d < Nx; ++d) {
        double acc = f0[d];
        for (int c = 0; c < Nx; ++c) acc += A(d, c) * ebar[c];
        for (int c = 0; c < Nu; ++c) acc += B(d, c) * vbar[c];
        worst_split = std::fmax(worst_split, std::fabs(acc - F[d]));
      }
      // central differences of the flat dynamics
      const double h = 1e-6;
      for (int c = 0; c < Nx + Nu; ++c) {
        Vec<Nx> ep = ebar, em = ebar;
        Vec<Nu> vp = vbar, vm = vbar;
        if (c < Nx) ep[c] += h, em[c] -= h;
        else vp[c - Nx] += h, vm[c - Nx] -= h;
        const auto Fp = flat_dynamics(mdl.f, xl, dxl, ul, ep, vp), Fm = flat_dynamics(mdl.f, xl, dxl, ul, em, vm);
        for (int d = 0; d < Nx; ++d) {
          const double fd = (Fp[d] - Fm[d]) / (2 * h), an = c < Nx ? A(d, c) : B(d, c - Nx);
          worst_fd = std::fmax(worst_fd, std::fabs(fd - an));
        }
      }
      if (k == 0) {  // df/dx - ad(f + dxdes) / 2, and f0 = f - dxdes
        Vec<Nx> fv;
        Mat<Nx, Nx> dfdx;
        Mat<Nx, Nu> dfdu;
        detail::xu_jacobian<Nx>(mdl.f, xl, ul, fv, dfdx, dfdu);
        Vec<Nx> s;
        for (int d = 0; d < Nx; ++d) s[d] = fv[d] + dxl[d];
        const auto adm = X::ad(s);
        for (int d = 0; d < Nx; ++d) {
          worst_zero = std::fmax(worst_zero, std::fabs(f0[d] - (fv[d] - dxl[d])));
          for (int c = 0; c < Nx; ++c) worst_zero = std::fmax(worst_zero, std::fabs(A(d, c) - (dfdx(d, c) - 0.5 * adm(d, c))));
          for (int c = 0; c < Nu; ++c) worst_zero = std::fmax(worst_zero, std::fabs(B(d, c) - dfdu(d, c)));
        }
      }
      // the input box: cr = u = udes (+) v, so C = 0, D = I, c0 = udes
      for (int d = 0; d < Ncr; ++d) {
        worst_cr = std::fmax(worst_cr, std::fabs(c0[d] - ul.v[d]));
        for (int c = 0; c < Nx; ++c) worst_cr = std::fmax(worst_cr, std::fabs(C(d, c)));
        for (int c = 0; c < Nu; ++c) worst_cr = std::fmax(worst_cr, std::fabs(D(d, c) - (c == d ? 1.0 : 0.0)));
      }
    }
    // the initial state, pinned: e = xdes(t) (-) x, J = I
    typename X::Tangent xi{};
    for (int d = 0; d < Nx; ++d) xi[d] = 0.1 * (d + 1) * (k + 1) * 0.3;
    const auto e = rminus(mdl.xdes(0.3), rplus(mdl.xdes(0.3), xi));
    for (int d = 0; d < Nx; ++d) {
      rec[o_e + d] = e[d];
      for (int c = 0; c < Nx; ++c) rec[o_J + d * Nx + c] = (c == d) ? 1.0 : 0.0;
      expect(std::fabs(e[d] + xi[d]) <= 1e-12, "e = -log(xdes^-1 x)", e[d] + xi[d]);
    }
    bool finite = true;
    for (const double v : rec) finite = finite && std::isfinite(v);
    expect(finite, "every double of the record written and finite", (double)k);
  }
  std::printf("%s: split %.2e  differences %.2e  e = 0 block %.2e  cr %.2e\n", name, worst_split, worst_fd, worst_zero, worst_cr);
  expect(worst_split <= 1e-13, "f0 + A ebar + B vbar = F", worst_split);
  expect(worst_fd <= 1e-8, "A, B against central differences", worst_fd);
  expect(worst_zero <= 1e-14, "e = 0: df/dx - ad(f + dxdes) / 2", worst_zero);
  expect(worst_cr <= 1e-15, "running constraint", worst_cr);
}

}  // namespace

int main()
{
  run<sfbx::VehicleModel6>("vehicle (SE2 x R^3)");
  run<sfbx::VehicleModel12>("two vehicles");
  std::printf(failures ? "mpc_relin_selftest: %d FAILED\n" : "mpc_relin_selftest: ok\n", failures);
  return failures ? 1 : 0;
}
