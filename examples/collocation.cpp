// Host entries of the collocation layer for the test harness (declared in models.h, part of libsfb_models.so): the ph
// mesh driven by an op script, the dynamics-error estimate for built-in dynamics, the flattened dynamics of the example
// models, and the reference's mesh / dyn-error test scenarios written as caller code against the reference's include
// paths and namespace.
#include "models.h"

#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include <smooth/feedback/collocation/dyn_error.hpp>
#include <smooth/feedback/collocation/mesh.hpp>
#include <smooth/feedback/mpc.hpp>

#include "lie_eval.h"
#include "rigid_body_model.h"
#include "vehicle_model.h"

namespace {

namespace sf = smooth::feedback;

// ops rows (code, a, b): 0 refine_ph(a, b), 1 increase_degrees, 2 decrease_degrees, 3 set_N_colloc_ival(a, b),
// 4 refine_errors with (target, errs[N_ivals]) taken from opdata
template<class M>
M run_script(int n, int k, int nops, const int32_t * ops, const double * opdata)
{
  M m = (n == 1 && k == (int)M::Kmin) ? M() : M((std::size_t)n, (std::size_t)k);
  for (int o = 0; o < nops; ++o) {
    const int32_t code = ops[3 * o], a = ops[3 * o + 1], b = ops[3 * o + 2];
    switch (code) {
    case 0: m.refine_ph((std::size_t)a, (std::size_t)b); break;
    case 1: m.increase_degrees(); break;
    case 2: m.decrease_degrees(); break;
    case 3: m.set_N_colloc_ival((std::size_t)a, (std::size_t)b); break;
    case 4: {
      const std::vector<double> errs(opdata + 1, opdata + 1 + m.N_ivals());
      m.refine_errors(errs, opdata[0]);
      opdata += 1 + errs.size();
      break;
    }
    default: throw std::invalid_argument("mesh script: unknown op");
    }
  }
  return m;
}

// run f on the instantiation <kmin, kmax> the harness carries
template<class F>
int with_mesh(int kmin, int kmax, int n, int k, int nops, const int32_t * ops, const double * opdata, F && f)
{
  try {
    if (kmin == 5 && kmax == 10) return f(run_script<sf::Mesh<5, 10>>(n, k, nops, ops, opdata));
    if (kmin == 5 && kmax == 5) return f(run_script<sf::Mesh<5, 5>>(n, k, nops, ops, opdata));
    if (kmin == 8 && kmax == 8) return f(run_script<sf::Mesh<8, 8>>(n, k, nops, ops, opdata));
    if (kmin == 3 && kmax == 6) return f(run_script<sf::Mesh<3, 6>>(n, k, nops, ops, opdata));
    if (kmin == 4 && kmax == 4) return f(run_script<sf::Mesh<4, 4>>(n, k, nops, ops, opdata));
    if (kmin == 13 && kmax == 13) return f(run_script<sf::Mesh<13, 13>>(n, k, nops, ops, opdata));  // the kernels' largest degree
  } catch (const std::exception & e) {
    std::fprintf(stderr, "collocation harness: %s\n", e.what());
    return -2;
  }
  return -1;  // no such instantiation
}

// the built-in dynamics of sfbx_mesh_dyn_error_host
template<int Nx, int Nu>
sf::Vec<Nx> builtin_f(int fid, const double * coef, double t, const sf::Vec<Nx> & x, const sf::Vec<Nu> & u)
{
  sf::Vec<Nx> f{};
  if (fid == 0) {  // time only: the derivative of sum_k coef[d][k] t^k, k < 4
    for (int d = 0; d < Nx; ++d) f[d] = coef[4 * d + 1] + t * (2 * coef[4 * d + 2] + t * 3 * coef[4 * d + 3]);
    return f;
  }
  for (int p = 0; p < Nx / 2; ++p) {
    f[2 * p] = x[2 * p + 1];
    if (fid == 1) f[2 * p + 1] = -x[2 * p];                                                  // harmonic oscillator
    else f[2 * p + 1] = -std::sin(x[2 * p]) + (Nu > 0 ? u[p % (Nu > 0 ? Nu : 1)] : 0.0);      // pendulum with input
  }
  return f;
}

template<int Nx, int Nu, class M>
int dyn_error_case(const M & base, int fid, const double * coef, double t0, double tf, const double * vals_x, const double * vals_u, double * errs)
{
  const auto xfun = [&](double t) {
    sf::Vec<Nx> x{};
    base.eval_flat((t - t0) / (tf - t0), vals_x, Nx, Nx, 0, true, x.data());
    return x;
  };
  const auto ufun = [&](double t) {
    sf::Vec<Nu> u{};
    if constexpr (Nu > 0) base.eval_flat((t - t0) / (tf - t0), vals_u, Nu, Nu, 0, false, u.data());
    return u;
  };
  const auto f = [&](double t, const sf::Vec<Nx> & x, const sf::Vec<Nu> & u) { return builtin_f<Nx, Nu>(fid, coef, t, x, u); };
  M raised = base;
  raised.increase_degrees();
  const std::vector<double> e = sf::mesh_dyn_error(f, raised, t0, tf, xfun, ufun);
  for (std::size_t i = 0; i < e.size(); ++i) errs[i] = e[i];
  return 0;
}

template<class Model, class X, class U>
void flat_dynamics_rows(int rows, const double * xl, const double * dxl, const double * ul, const double * e, const double * v, double * out)
{
  constexpr int EX = sfbx::LieIO<X>::E, EU = sfbx::LieIO<U>::E, Nx = X::Dof, Nu = U::Dof;
  const Model model{};
  for (int r = 0; r < rows; ++r) {
    typename X::Tangent d{}, ee{};
    typename U::Tangent vv{};
    for (int i = 0; i < Nx; ++i) d[i] = dxl[r * Nx + i], ee[i] = e[r * Nx + i];
    for (int i = 0; i < Nu; ++i) vv[i] = v[r * Nu + i];
    const auto fd = sf::flat_dynamics(model.f, sfbx::LieIO<X>::load(xl + r * EX), d, sfbx::LieIO<U>::load(ul + r * EU), ee, vv);
    for (int i = 0; i < Nx; ++i) out[r * Nx + i] = fd[i];
  }
}

// the harness's MPC variants: 6 / 12 the vehicles, 13 the rigid body; fn(mpc, its model)
template<class Fn>
int with_mpc(int variant, int K, double tf, Fn && fn)
{
  try {
    if (variant == 6) return fn(sfbx::make_vehicle_mpc<sfbx::MPC6, sfbx::VehicleModel6>(K, tf), sfbx::VehicleModel6{});
    if (variant == 12) return fn(sfbx::make_vehicle_mpc<sfbx::MPC12, sfbx::VehicleModel12>(K, tf), sfbx::VehicleModel12{});
    if (variant == 13) return fn(sfbx::make_rigid_body_mpc(K, tf), sfbx::RigidBodyModel{});
  } catch (const std::exception & e) {
    std::fprintf(stderr, "collocation harness: %s\n", e.what());
    return -2;
  }
  return -1;
}

}  // namespace

extern "C" {

int sfbx_mpc_dyn_error_host(int variant, int K, double tf, int64_t batch, const double * t, const double * primal, double * errs)
{
  return with_mpc(variant, K, tf, [&](const auto & mpc, const auto &) {
    const int64_t n = (int64_t)mpc.Nx * (mpc.N() + 1) + (int64_t)mpc.Nu * mpc.N();
    for (int64_t b = 0; b < batch; ++b) {
      const std::vector<double> e = mpc.dyn_error(t[b], primal + b * n);
      std::copy(e.begin(), e.end(), errs + b * (int64_t)e.size());
    }
    return 0;
  });
}

int sfbx_mpc_tick_dyn_error_host(int variant, int K, double tf, double t, const double * dx0, double * errs, int32_t * code)
{
  return with_mpc(variant, K, tf, [&](auto mpc, const auto & model) {
    using X = decltype(model.xdes(t));
    typename X::Tangent a{};
    for (int i = 0; i < X::Dof; ++i) a[i] = dx0[i];
    try {
      (void)mpc.dyn_error(t);
      return -3;  // no plan yet: this must throw
    } catch (const std::logic_error &) {
    }
    const auto [u, c] = mpc(t, rplus(model.xdes(t), a));
    (void)u;
    *code = (int32_t)c;
    const std::vector<double> e = mpc.dyn_error(t);
    std::copy(e.begin(), e.end(), errs);
    return 0;
  });
}

int sfbx_mesh_script(int kmin, int kmax, int n, int k, int nops, const int32_t * ops, const double * opdata, int cap_ivals, int32_t * nivals,
                     int32_t * K, double * tau0, double * nodes, double * weights, double * diffmat, double * intmat, int nt, const double * t,
                     int dim, const double * vals, int p, int extend, double * eval_out, int32_t * found)
{
  return with_mesh(kmin, kmax, n, k, nops, ops, opdata, [&](const auto & m) {
    const int N = (int)m.N_ivals();
    *nivals     = N;
    if (N > cap_ivals) return -3;
    for (int i = 0; i < N; ++i) {
      K[i]    = (int32_t)m.N_colloc_ival(i);
      tau0[i] = m.interval_nodes(i).front();
      const auto D = m.interval_diffmat(i);
      const auto I = m.interval_intmat(i);
      for (int r = 0; r < D.rows; ++r)  // row-major, interval after interval
        for (int c = 0; c < D.cols; ++c) *diffmat++ = D(r, c);
      for (int r = 0; r < I.rows; ++r)
        for (int c = 0; c < I.cols; ++c) *intmat++ = I(r, c);
    }
    const auto an = m.all_nodes(), aw = m.all_weights();
    if (an.size() != m.N_colloc() + 1 || aw.size() != an.size()) return -4;
    std::copy(an.begin(), an.end(), nodes);
    std::copy(aw.begin(), aw.end(), weights);
    for (int q = 0; q < nt; ++q) {
      m.eval_flat(t[q], vals, (std::size_t)dim, (std::size_t)dim, (std::size_t)p, extend != 0, eval_out + (std::size_t)q * dim);
      found[q] = (int32_t)m.interval_find(t[q]);
    }
    return 0;
  });
}

int sfbx_mesh_dyn_error_host(int kmin, int kmax, int n, int k, int nops, const int32_t * ops, const double * opdata, int fid, const double * coef,
                             int nx, int nu, double t0, double tf, const double * vals_x, const double * vals_u, double * errs)
{
  return with_mesh(kmin, kmax, n, k, nops, ops, opdata, [&](const auto & m) {
#define SFBX_CASE(NX, NU) \
  if (nx == NX && nu == NU) return dyn_error_case<NX, NU>(m, fid, coef, t0, tf, vals_x, vals_u, errs);
    SFBX_CASE(1, 0) SFBX_CASE(1, 1) SFBX_CASE(2, 0) SFBX_CASE(2, 1) SFBX_CASE(2, 2) SFBX_CASE(12, 2)
#undef SFBX_CASE
    return -5;  // no such (nx, nu)
  });
}

int sfbx_flat_dynamics_host(int model, int rows, const double * xl, const double * dxl, const double * ul, const double * e, const double * v,
                            double * out)
{
  if (model == 0) flat_dynamics_rows<sfbx::VehicleModel6, sfbx::X6, sfbx::U2>(rows, xl, dxl, ul, e, v, out);
  else if (model == 1) flat_dynamics_rows<sfbx::RigidBodyModel, sfbx::X12B, sfbx::U6>(rows, xl, dxl, ul, e, v, out);
  else return -1;
  return 0;
}

// tests/test_collocation_mesh.cpp and tests/test_collocation_dyn_error.cpp of the reference as caller code; returns 0, or
// the number of the first expectation that fails
int sfbx_test_collocation_api(void)
{
  namespace F = smooth::feedback;
  const auto near = [](double a, double b, double tol) { return std::fabs(a - b) <= tol * (1 + std::fabs(b)); };
  const auto nondecreasing = [](const std::vector<double> & v) {
    for (std::size_t i = 1; i < v.size(); ++i)
      if (v[i - 1] > v[i]) return false;
    return true;
  };
  {  // CollocationMesh.Basic (:38-77)
    F::Mesh<5, 10> m;
    m.refine_ph(0, 5 * 10);
    if (m.N_ivals() != 10) return 1;
    for (unsigned i = 0; i < 10; ++i)
      if (!near(m.interval_nodes(i).front(), i * 0.1, 1e-15)) return 2;
    m.refine_ph(1, 10);  // only raises the degree
    if (m.N_ivals() != 10 || m.N_colloc_ival(1) != 10 || !near(m.interval_nodes(1).front(), 0.1, 1e-15)) return 3;
    m.refine_ph(1, 13);  // splits
    if (m.N_ivals() != 12) return 4;
    if (!near(m.interval_nodes(1).front(), 0.1, 1e-15) || !near(m.interval_nodes(2).front(), 0.1 + 0.1 / 3, 1e-15) ||
        !near(m.interval_nodes(3).front(), 0.1 + 2 * 0.1 / 3, 1e-15))
      return 5;
    m.refine_ph(2, 27);
    m.refine_ph(7, 33);
    m.refine_ph(9, 22);
    const auto alln = m.all_nodes();
    if (alln.size() != m.N_colloc() + 1 || !nondecreasing(alln)) return 6;
  }
  {  // CollocationMesh.Constructor (:79-92)
    for (std::size_t i = 0; i < 100; ++i) {
      F::Mesh<5, 10> m(i);
      if (m.N_ivals() != std::max<std::size_t>(i, 1)) return 7;
      for (std::size_t j = 0; j < m.N_ivals(); ++j)
        if (m.N_colloc_ival(j) != 5) return 8;
    }
    for (std::size_t k = 5; k <= 10; ++k) {
      F::Mesh<5, 10> m(10, k);
      for (std::size_t j = 0; j < 10; ++j)
        if (m.N_colloc_ival(j) != k) return 9;
    }
  }
  {  // CollocationMesh.DifferentiationIntegration (:94-125)
    F::Mesh<8, 8> m;
    m.refine_ph(0, 40);
    const auto x  = [](double t) { return 1 + 2 * t + 3 * t * t + 4 * t * t * t; };
    const auto dx = [](double t) { return 2 + 3 * 2 * t + 4 * 3 * t * t; };
    for (std::size_t ival = 0; ival < m.N_ivals(); ++ival) {
      const int N     = (int)m.N_colloc_ival(ival);
      const auto taus = m.interval_nodes(ival);
      const auto D = m.interval_diffmat(ival), I = m.interval_intmat(ival);
      const auto [alpha, Dus] = m.interval_diffmat_unscaled(ival);
      for (int c = 0; c < N; ++c) {
        double d = 0, s = x(taus[0]), du = 0;
        for (int r = 0; r <= N; ++r) d += x(taus[r]) * D(r, c), du += x(taus[r]) * Dus(r, c);
        for (int r = 0; r < N; ++r) s += dx(taus[r]) * I(r, c);
        if (!near(d, dx(taus[c]), 1e-9) || !near(alpha * du, dx(taus[c]), 1e-9)) return 10;
        if (!near(s, x(taus[c + 1]), 1e-9)) return 11;
      }
    }
  }
  {  // CollocationMesh.FunctionEval (:127-171)
    F::Mesh<5, 5> m;
    const auto ones_ok = [&](const F::Mesh<5, 5> & mm, bool extend) {
      const std::vector<F::Vec<3>> vals(mm.N_colloc() + (extend ? 1 : 0), F::Vec<3>{1, 1, 1});
      for (const double t : {0.0, 0.5, 1.0}) {
        const auto v = mm.eval<3>(t, vals, 0, extend);
        for (int d = 0; d < 3; ++d)
          if (std::fabs(v[d] - 1) > 1e-12) return false;
      }
      return true;
    };
    if (!ones_ok(m, true) || !ones_ok(m, false)) return 12;
    m.refine_ph(0, 40);
    if (!ones_ok(m, true)) return 13;
  }
  {  // CollocationMesh.IntervalNodes (:173-195)
    F::Mesh<5, 5> mesh;
    mesh.refine_ph(0, 10);
    const auto n0 = mesh.interval_nodes(0), n1 = mesh.interval_nodes(1), w0 = mesh.interval_weights(0), w1 = mesh.interval_weights(1);
    for (std::size_t i = 0; i < n0.size(); ++i)
      if (std::fabs(n0[i] + 0.5 - n1[i]) > 1e-9 || std::fabs(w0[i] - w1[i]) > 1e-9) return 14;
    if (!nondecreasing(mesh.all_nodes())) return 15;
    double sum = 0;
    for (const double w : mesh.all_weights()) sum += w;
    if (std::fabs(sum - 1) > 1e-9) return 16;
  }
  {  // CollocationDyn.DynError (test_collocation_dyn_error.cpp:31-79)
    const auto x = [](double t) { return F::Vec<1>{0.1 * t * t - 0.4 * t + 0.2}; };
    const auto f = [](double t, const F::Vec<1> &, const F::Vec<0> &) { return F::Vec<1>{0.2 * t - 0.4}; };
    const double t0 = 3, tf = 5;
    F::Mesh<5, 5> m;
    m.refine_ph(0, 16 * 5);
    if (m.N_ivals() != 16) return 17;
    std::vector<F::Vec<1>> X;
    for (const double tau : m.all_nodes()) X.push_back(x(t0 + (tf - t0) * tau));
    const auto xfun = [X, t0, tf, m](double t) { return m.eval<1>((t - t0) / (tf - t0), X, 0, true); };
    const auto ufun = [](double) { return F::Vec<0>{}; };
    m.increase_degrees();
    const auto rel_errs = F::mesh_dyn_error(f, m, t0, tf, xfun, ufun);
    m.decrease_degrees();
    if (rel_errs.size() != 16) return 18;
    for (const double e : rel_errs)
      if (!(std::fabs(e) <= 1e-8)) return 19;
    const auto Npre = m.N_ivals();
    m.refine_errors(rel_errs, 1e-8);
    if (m.N_ivals() != Npre) return 20;
    for (std::size_t i = 0; i < Npre; ++i)
      if (m.N_colloc_ival(i) != 5) return 21;
  }
  return 0;
}

}  // extern "C"
