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
#include <smooth/feedback/collocation/mesh_function.hpp>
#include <smooth/feedback/mpc.hpp>

#include <thread>

#include "flat_ocp_harness.h"
#include "lie_eval.h"
#include "ocp_nlp_harness.h"
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
    if (kmin == 1 && kmax == 2) return f(run_script<sf::Mesh<1, 2>>(n, k, nops, ops, opdata));        // one point per interval
    if (kmin == 4 && kmax == 6) return f(run_script<sf::Mesh<4, 6>>(n, k, nops, ops, opdata));
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

// ---- functions over a mesh (mesh_function.hpp) ----
// what mesh_eval / mesh_integrate / mesh_dyn ask of a mesh, copied out of any Mesh<Kmin, Kmax>: one instantiation of the
// functions per integrand instead of one per mesh type
struct MeshCopy {
  std::vector<double> nodes, weights;
  std::vector<std::size_t> K;
  std::vector<std::pair<double, sf::MeshMat>> D;
  template<class M>
  explicit MeshCopy(const M & m) : nodes(m.all_nodes()), weights(m.all_weights())
  {
    for (std::size_t s = 0; s < m.N_ivals(); ++s) K.push_back(m.N_colloc_ival(s)), D.push_back(m.interval_diffmat_unscaled(s));
  }
  std::size_t N_ivals() const { return K.size(); }
  std::size_t N_colloc() const { return nodes.size() - 1; }
  std::size_t N_colloc_ival(std::size_t s) const { return K[s]; }
  const std::vector<double> & all_nodes() const { return nodes; }
  const std::vector<double> & all_weights() const { return weights; }
  const std::pair<double, sf::MeshMat> & interval_diffmat_unscaled(std::size_t s) const { return D[s]; }
};

// An integrand as data: output r is the sum of coef phi_ka(z_a) phi_kb(z_b) over its terms (rows r, a, ka, b, kb),
// z = (t, x, u), phi_0 = 1, phi_1 = z, phi_2 = z^2, phi_3 = sin z, phi_4 = cos z; derivatives in closed form.
struct Phi {
  double v, d1, d2;
  Phi(int k, double z)
  {
    switch (k) {
    case 0: v = 1, d1 = 0, d2 = 0; break;
    case 1: v = z, d1 = 1, d2 = 0; break;
    case 2: v = z * z, d1 = 2 * z, d2 = 2; break;
    case 3: v = std::sin(z), d1 = std::cos(z), d2 = -std::sin(z); break;
    default: v = std::cos(z), d1 = -std::sin(z), d2 = -std::cos(z); break;
    }
  }
};
template<int NX, int NU, int NF>
struct TermFn {
  static constexpr int NV = 1 + NX + NU;
  int nterms;
  const int32_t * terms;
  const double * coef;
  static double coord(int a, double t, const sf::Rn<NX> & x, const sf::Rn<NU> & u) { return a == 0 ? t : a <= NX ? x.v[a - 1] : u.v[a - 1 - NX]; }
  sf::Vec<NF> operator()(double t, const sf::Rn<NX> & x, const sf::Rn<NU> & u) const
  {
    sf::Vec<NF> f{};
    for (int m = 0; m < nterms; ++m) {
      const int32_t * q = terms + 5 * m;
      f[q[0]] += coef[m] * Phi(q[2], coord(q[1], t, x, u)).v * Phi(q[4], coord(q[3], t, x, u)).v;
    }
    return f;
  }
  void jacobian(double t, const sf::Rn<NX> & x, const sf::Rn<NU> & u, sf::Mat<NF, NV> & J) const
  {
    J = sf::Mat<NF, NV>::Zero();
    for (int m = 0; m < nterms; ++m) {
      const int32_t * q = terms + 5 * m;
      const Phi A(q[2], coord(q[1], t, x, u)), B(q[4], coord(q[3], t, x, u));
      J(q[0], q[1]) += coef[m] * A.d1 * B.v;
      J(q[0], q[3]) += coef[m] * A.v * B.d1;
    }
  }
  void hessian(double t, const sf::Rn<NX> & x, const sf::Rn<NU> & u, sf::Mat<NV, NF * NV> & H) const
  {
    H = sf::Mat<NV, NF * NV>::Zero();
    for (int m = 0; m < nterms; ++m) {
      const int32_t * q = terms + 5 * m;
      const int r = q[0], a = q[1], b = q[3];
      const Phi A(q[2], coord(a, t, x, u)), B(q[4], coord(b, t, x, u));
      H(a, r * NV + a) += coef[m] * A.d2 * B.v;
      H(a, r * NV + b) += coef[m] * A.d1 * B.d1;
      H(b, r * NV + a) += coef[m] * A.d1 * B.d1;
      H(b, r * NV + b) += coef[m] * A.v * B.d2;
    }
  }
};
// the vehicle's dynamics on SE2 x R^3 as an integrand (t, x, u), with its Jacobian in the (t | x | u) form
struct VehicleFn {
  sfbx::VehicleDyn6 f;
  sf::Vec<6> operator()(double, const sfbx::X6 & x, const sfbx::U2 & u) const { return f(x, u); }
  void jacobian(double, const sfbx::X6 & x, const sfbx::U2 & u, sf::Mat<6, 9> & J) const
  {
    sf::Mat<6, 6> dx;
    sf::Mat<6, 2> du;
    f.jacobian(x, u, dx, du);
    J = sf::Mat<6, 9>::Zero();
    for (int r = 0; r < 6; ++r) {
      for (int c = 0; c < 6; ++c) J(r, 1 + c) = dx(r, c);
      for (int c = 0; c < 2; ++c) J(r, 7 + c) = du(r, c);
    }
  }
};

// an integrand given by its values at the nodes, for comparing the host front with the model-free kernels on the same
// numbers: table [N][NF (2 + NX + NU)] holds node i's values, then its Jacobian row-major; the functions evaluate the
// integrand once per node in node order, and jacobian() belongs to the node evaluated last
template<int NX, int NU, int NF>
struct TableFn {
  static constexpr int NV = 1 + NX + NU;
  const double * table;
  mutable long node = -1;
  sf::Vec<NF> operator()(double, const sf::Rn<NX> &, const sf::Rn<NU> &) const
  {
    ++node;
    sf::Vec<NF> f{};
    for (int r = 0; r < NF; ++r) f[r] = table[node * NF * (1 + NV) + r];
    return f;
  }
  void jacobian(double, const sf::Rn<NX> &, const sf::Rn<NU> &, sf::Mat<NF, NV> & J) const
  {
    for (int r = 0; r < NF; ++r)
      for (int c = 0; c < NV; ++c) J(r, c) = table[node * NF * (1 + NV) + NF + r * NV + c];
  }
};

struct MeshFnOut {
  int32_t * dims;  // rows, cols, nnz, d2 nnz, 1 when no output array moved between the calls
  double * F;
  int32_t *rowptr, *colind;
  double * val;
  int32_t *colptr2, *rowind2;
  double * val2;
};

template<int FN, uint8_t Deriv, sf::diff::Type DT, class Fn, class X, class U>
int meshfn_run(const MeshCopy & m, Fn & f, double t0, double tf, const std::vector<X> & xs, const std::vector<U> & us, bool scale,
               const double * lambda, int calls, const MeshFnOut & o)
{
  sf::MeshValue<Deriv> out;
  const void * where[4] = {nullptr, nullptr, nullptr, nullptr};
  bool stable = true;
  for (int c = 0; c < calls; ++c) {
    if constexpr (Deriv == 2) {
      constexpr std::size_t nf = std::tuple_size_v<decltype(f(0.0, xs[0], us[0]))>;
      if (c == 0) out.lambda.assign(lambda, lambda + (FN == 1 ? nf : nf * m.N_colloc()));
    }
    if constexpr (FN == 0) sf::mesh_eval<Deriv, DT>(out, m, f, t0, tf, xs, us, scale);
    if constexpr (FN == 1) sf::mesh_integrate<Deriv, DT>(out, m, f, t0, tf, xs, us);
    if constexpr (FN == 2) sf::mesh_dyn<Deriv, DT>(out, m, f, t0, tf, xs, us);
    if (!out.allocated) return -7;
    const void * now[4] = {out.F.data(), nullptr, nullptr, nullptr};
    if constexpr (Deriv >= 1) now[1] = out.dF.val.data(), now[2] = out.dF.colind.data();
    if constexpr (Deriv >= 2) now[3] = out.d2F.val.data();
    for (int k = 0; k < 4; ++k) {
      if (c > 0 && now[k] != where[k]) stable = false;
      where[k] = now[k];
    }
  }
  o.dims[0] = (int32_t)out.F.size();
  o.dims[1] = o.dims[2] = o.dims[3] = 0;
  o.dims[4] = stable ? 1 : 0;
  std::copy(out.F.begin(), out.F.end(), o.F);
  if constexpr (Deriv >= 1) {
    if (out.dF.rows != (int32_t)out.F.size()) return -8;
    o.dims[1] = out.dF.cols;
    o.dims[2] = (int32_t)out.dF.val.size();
    std::copy(out.dF.rowptr.begin(), out.dF.rowptr.end(), o.rowptr);
    std::copy(out.dF.colind.begin(), out.dF.colind.end(), o.colind);
    std::copy(out.dF.val.begin(), out.dF.val.end(), o.val);
  }
  if constexpr (Deriv >= 2) {
    o.dims[3] = (int32_t)out.d2F.val.size();
    std::copy(out.d2F.colptr.begin(), out.d2F.colptr.end(), o.colptr2);
    std::copy(out.d2F.rowind.begin(), out.d2F.rowind.end(), o.rowind2);
    std::copy(out.d2F.val.begin(), out.d2F.val.end(), o.val2);
  }
  return 0;
}

// (fn, deriv, numerical) at run time -> the instantiation; MaxDeriv and Dyn say what the state / input types allow
template<int MaxDeriv, bool Dyn, class Fn, class X, class U>
int meshfn_dispatch(int fn, int deriv, int numerical, const MeshCopy & m, Fn & f, double t0, double tf, const std::vector<X> & xs,
                    const std::vector<U> & us, bool scale, const double * lambda, int calls, const MeshFnOut & o)
{
  using T = sf::diff::Type;
#define SFBX_RUN(FN, D) \
  if constexpr (D <= MaxDeriv && (FN < 2 || Dyn)) \
    if (fn == FN && deriv == D) \
      return numerical ? meshfn_run<FN, D, T::Numerical>(m, f, t0, tf, xs, us, scale, lambda, calls, o) \
                       : meshfn_run<FN, D, T::Analytic>(m, f, t0, tf, xs, us, scale, lambda, calls, o);
  SFBX_RUN(0, 0) SFBX_RUN(0, 1) SFBX_RUN(0, 2) SFBX_RUN(1, 0) SFBX_RUN(1, 1) SFBX_RUN(1, 2) SFBX_RUN(2, 0) SFBX_RUN(2, 1) SFBX_RUN(2, 2)
#undef SFBX_RUN
  return -6;  // no such (fn, deriv) for this shape
}

template<int NX, int NU, int NF>
int meshfn_terms(int fn, int deriv, int numerical, const MeshCopy & m, int nterms, const int32_t * terms, const double * coef, double t0, double tf,
                 const double * xs, const double * us, bool scale, const double * lambda, int calls, const MeshFnOut & o)
{
  for (int q = 0; q < nterms; ++q) {
    const int32_t * t = terms + 5 * q;
    if (t[0] < 0 || t[0] >= NF || t[1] < 0 || t[1] > NX + NU || t[3] < 0 || t[3] > NX + NU || t[2] < 0 || t[2] > 4 || t[4] < 0 || t[4] > 4) return -9;
  }
  const std::size_t N = m.N_colloc();
  std::vector<sf::Rn<NX>> X(N + 1);
  std::vector<sf::Rn<NU>> U(N);
  for (std::size_t i = 0; i <= N; ++i)
    for (int d = 0; d < NX; ++d) X[i].v[d] = xs[i * NX + d];
  for (std::size_t i = 0; i < N; ++i)
    for (int d = 0; d < NU; ++d) U[i].v[d] = us[i * NU + d];
  TermFn<NX, NU, NF> f{nterms, terms, coef};
  return meshfn_dispatch<2, NX == NF>(fn, deriv, numerical, m, f, t0, tf, X, U, scale, lambda, calls, o);
}

}  // namespace

extern "C" {

int sfbx_meshfn_host(int kmin, int kmax, int n, int k, int nops, const int32_t * ops, const double * opdata, int fn, int deriv, int numerical,
                     int shape, int nterms, const int32_t * terms, const double * coef, double t0, double tf, const double * xs, const double * us,
                     int scale, const double * lambda, int calls, int32_t * dims, double * F, int32_t * rowptr, int32_t * colind, double * val,
                     int32_t * colptr2, int32_t * rowind2, double * val2)
{
  const MeshFnOut o{dims, F, rowptr, colind, val, colptr2, rowind2, val2};
  return with_mesh(kmin, kmax, n, k, nops, ops, opdata, [&](const auto & mesh) {
    const MeshCopy m(mesh);
    switch (shape) {
    case 0: return meshfn_terms<3, 2, 3>(fn, deriv, numerical, m, nterms, terms, coef, t0, tf, xs, us, scale != 0, lambda, calls, o);
    case 1: return meshfn_terms<3, 2, 1>(fn, deriv, numerical, m, nterms, terms, coef, t0, tf, xs, us, scale != 0, lambda, calls, o);
    case 2: return meshfn_terms<1, 0, 1>(fn, deriv, numerical, m, nterms, terms, coef, t0, tf, xs, us, scale != 0, lambda, calls, o);
    case 3: return meshfn_terms<12, 2, 12>(fn, deriv, numerical, m, nterms, terms, coef, t0, tf, xs, us, scale != 0, lambda, calls, o);
    case 4: {  // the vehicle on SE2 x R^3: states in the flat storage of lie_eval.h
      const std::size_t N = m.N_colloc();
      std::vector<sfbx::X6> X(N + 1);
      std::vector<sfbx::U2> U(N);
      for (std::size_t i = 0; i <= N; ++i) X[i] = sfbx::LieIO<sfbx::X6>::load(xs + 7 * i);
      for (std::size_t i = 0; i < N; ++i) U[i] = sfbx::LieIO<sfbx::U2>::load(us + 2 * i);
      VehicleFn f{};
      return meshfn_dispatch<1, false>(fn, deriv, numerical, m, f, t0, tf, X, U, scale != 0, lambda, calls, o);
    }
    case 5: {  // (6, 2, 6) tabulated: coef is the table, orders 0 and 1, one call
      if (deriv > 1 || numerical || calls != 1) return -6;
      const std::size_t N = m.N_colloc();
      std::vector<sf::Rn<6>> X(N + 1);
      std::vector<sf::Rn<2>> U(N);
      for (std::size_t i = 0; i <= N; ++i)
        for (int d = 0; d < 6; ++d) X[i].v[d] = xs[i * 6 + d];
      for (std::size_t i = 0; i < N; ++i)
        for (int d = 0; d < 2; ++d) U[i].v[d] = us[i * 2 + d];
      TableFn<6, 2, 6> f{coef};
      return meshfn_dispatch<1, true>(fn, deriv, 0, m, f, t0, tf, X, U, scale != 0, lambda, calls, o);
    }
    default: return -5;
    }
  });
}

// OCPNLP of a problem given as term tables (ocp_nlp_harness.h) on the script's mesh.  The harness carries one mesh type per
// shape: dims (1, 0, 0, 0, 0) on Mesh<1, 2>, (2, 1, 1, 4, 6) on Mesh<3, 3>, (3, 2, 2, 1, 3) on Mesh<3, 6>, (3, 2, 1, 3, 2) on Mesh<13, 13>.
int sfbx_ocp_nlp_host(int kmin, int kmax, int n, int k, int nops, const int32_t * ops, const int32_t * dims, const int32_t * nterms,
                      const int32_t * terms, const double * coef, const double * crl, const double * cru, const double * cel, const double * ceu,
                      const double * x, const double * lambda, int order, int numerical, int calls, int32_t * sizes, double * f, double * df, double * g,
                      int32_t * rowptr, int32_t * colind, double * dg, int32_t * hcolptr, int32_t * hrowind, double * d2f, double * d2g, double * xl,
                      double * xu, double * gl, double * gu, double * ws, double * x_back, double * lambda_back)
{
  sfbx::OcpData d{};
  for (int q = 0, at = 0; q < 5; ++q) {
    d.tab[q] = sfbx::TermTable{nterms[q], terms + 7 * at, coef + at};
    at += nterms[q];
  }
  d.crl = crl, d.cru = cru, d.cel = cel, d.ceu = ceu;
  const sfbx::OcpNlpOut o{f, df, g, dg, d2f, d2g, xl, xu, gl, gu, ws, x_back, lambda_back, rowptr, colind, hcolptr, hrowind, sizes};
  using T = sf::diff::Type;
  try {
#define SFBX_NLP(KMIN, KMAX, NX, NU, NQ, NCR, NCE) \
  if (kmin == KMIN && kmax == KMAX && dims[0] == NX && dims[1] == NU && dims[2] == NQ && dims[3] == NCR && dims[4] == NCE) { \
    const auto mesh = run_script<sf::Mesh<KMIN, KMAX>>(n, k, nops, ops, nullptr); \
    return numerical ? sfbx::ocp_nlp_run<NX, NU, NQ, NCR, NCE, T::Numerical>(mesh, d, x, lambda, order, calls, o) \
                     : sfbx::ocp_nlp_run<NX, NU, NQ, NCR, NCE, T::Analytic>(mesh, d, x, lambda, order, calls, o); \
  }
    SFBX_NLP(1, 2, 1, 0, 0, 0, 0) SFBX_NLP(3, 3, 2, 1, 1, 4, 6) SFBX_NLP(3, 6, 3, 2, 2, 1, 3) SFBX_NLP(13, 13, 3, 2, 1, 3, 2)
#undef SFBX_NLP
  } catch (const std::exception & e) {
    std::fprintf(stderr, "collocation harness: %s\n", e.what());
    return -2;
  }
  return -1;  // no such (mesh type, dims)
}

// OCPNLP::d2l_dx2 of the same problems on the same (mesh type, dims) pairs
int sfbx_ocp_nlp_hess_host(int kmin, int kmax, int n, int k, int nops, const int32_t * ops, const int32_t * dims, const int32_t * nterms,
                           const int32_t * terms, const double * coef, const double * crl, const double * cru, const double * cel, const double * ceu,
                           const double * x, const double * lambda, double sigma, int numerical, int calls, int32_t * sizes, int32_t * hcolptr,
                           int32_t * hrowind, int32_t * hcolptr2, int32_t * hrowind2, double * d2l)
{
  sfbx::OcpData d{};
  for (int q = 0, at = 0; q < 5; ++q) {
    d.tab[q] = sfbx::TermTable{nterms[q], terms + 7 * at, coef + at};
    at += nterms[q];
  }
  d.crl = crl, d.cru = cru, d.cel = cel, d.ceu = ceu;
  const sfbx::OcpNlpHessOut o{sizes, hcolptr, hrowind, hcolptr2, hrowind2, d2l};
  using T = sf::diff::Type;
  try {
#define SFBX_NLP(KMIN, KMAX, NX, NU, NQ, NCR, NCE) \
  if (kmin == KMIN && kmax == KMAX && dims[0] == NX && dims[1] == NU && dims[2] == NQ && dims[3] == NCR && dims[4] == NCE) { \
    const auto mesh = run_script<sf::Mesh<KMIN, KMAX>>(n, k, nops, ops, nullptr); \
    return numerical ? sfbx::ocp_nlp_hess_run<NX, NU, NQ, NCR, NCE, T::Numerical>(mesh, d, x, lambda, sigma, calls, o) \
                     : sfbx::ocp_nlp_hess_run<NX, NU, NQ, NCR, NCE, T::Analytic>(mesh, d, x, lambda, sigma, calls, o); \
  }
    SFBX_NLP(1, 2, 1, 0, 0, 0, 0) SFBX_NLP(3, 3, 2, 1, 1, 4, 6) SFBX_NLP(3, 6, 3, 2, 2, 1, 3) SFBX_NLP(13, 13, 3, 2, 1, 3, 2)
#undef SFBX_NLP
  } catch (const std::exception & e) {
    std::fprintf(stderr, "collocation harness: %s\n", e.what());
    return -2;
  }
  return -1;  // no such (mesh type, dims)
}

// the scenario of the reference's tests/test_ocp_to_nlp.cpp as caller code against <smooth/feedback/ocp_to_nlp.hpp>: the
// problem written as lambdas in an OCP<...>, random x and lambda, and df, dg, d2f, d2g against differences of f, g and
// lambda' g at the reference's tolerances (1e-4 first, 1e-3 second derivatives, relative in the Frobenius norm as
// isApprox is); returns 0, or the number of the first expectation that fails
int sfbx_test_ocp_to_nlp_api(void)
{
  namespace F = smooth::feedback;
  using X = F::Rn<2>;
  using U = F::Rn<1>;
  const auto theta = [](double tf, const X & x0, const X & xf, const F::Vec<1> & q) {
    const double a = x0.v[0] * xf.v[0], b = x0.v[1] * xf.v[1];
    return (tf - 2) * (tf - 2) + a * a + b * b + xf.v[0] * xf.v[0] + xf.v[1] * xf.v[1] + q[0];
  };
  const auto f  = [](double t, const X & x, const U & u) { return F::Vec<2>{x.v[1] + t, x.v[0] * u.v[0] * u.v[0]}; };
  const auto g  = [](double t, const X & x, const U & u) { return F::Vec<1>{t + t * (x.v[0] * x.v[0] + x.v[1] * x.v[1]) + u.v[0] * u.v[0]}; };
  const auto cr = [](double t, const X & x, const U & u) { return F::Vec<4>{t, t * x.v[0] * u.v[0], t * x.v[1] * u.v[0], u.v[0] * u.v[0]}; };
  const auto ce = [](double tf, const X & x0, const X & xf, const F::Vec<1> & q) {
    return F::Vec<6>{tf, x0.v[0] * xf.v[0], x0.v[1] * xf.v[1], xf.v[0], xf.v[1], q[0] * q[0]};
  };
  const F::Vec<4> crl{-1, -1, -1, -1}, cru{1, 1, 1, 1};
  const F::Vec<6> cel{-1, -1, -1, -1, -1, -1}, ceu{1, 1, 1, 1, 1, 1};
  const auto ocp = F::make_ocp<X, U>(theta, f, g, cr, crl, cru, ce, cel, ceu);
  F::Mesh<3, 3> mesh;
  mesh.refine_ph(0, 4);
  mesh.refine_ph(0, 4);
  auto nlp = F::ocp_to_nlp(ocp, mesh);
  static_assert(F::HessianNLP<decltype(nlp)>);
  const std::size_t n = nlp.n(), m = nlp.m();
  if (n != 31 || m != 61) return 1;
  std::vector<double> x(n), lambda(m);
  uint64_t state = 5;
  const auto draw = [&]() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11) / 4503599627370496.0 - 1.0;  // [-1, 1)
  };
  for (double & v : x) v = draw();
  for (double & v : lambda) v = draw();
  // the same problem as tables with closed-form derivatives
  static const int32_t terms[][7] = {
    {0, 2, 1, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 0, 0}, {1, 1, 1, 3, 2, 0, 0},                                                    // f
    {0, 0, 1, 0, 0, 0, 0}, {0, 0, 1, 1, 2, 0, 0}, {0, 0, 1, 2, 2, 0, 0}, {0, 3, 2, 0, 0, 0, 0},                              // g
    {0, 0, 1, 0, 0, 0, 0}, {1, 0, 1, 1, 1, 3, 1}, {2, 0, 1, 2, 1, 3, 1}, {3, 3, 2, 0, 0, 0, 0},                              // cr
    {0, 0, 2, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 2, 0, 0}, {0, 2, 2, 4, 2, 0, 0},
    {0, 3, 2, 0, 0, 0, 0}, {0, 4, 2, 0, 0, 0, 0}, {0, 5, 1, 0, 0, 0, 0},                                                    // theta
    {0, 0, 1, 0, 0, 0, 0}, {1, 1, 1, 3, 1, 0, 0}, {2, 2, 1, 4, 1, 0, 0}, {3, 3, 1, 0, 0, 0, 0}, {4, 4, 1, 0, 0, 0, 0}, {5, 5, 2, 0, 0, 0, 0}};  // ce
  static const double coef[25] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -4, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
  sfbx::TermOcp<2, 1, 1, 4, 6> tocp{};
  tocp.f.tab = {3, terms[0], coef}, tocp.g.tab = {4, terms[3], coef + 3}, tocp.cr.tab = {4, terms[7], coef + 7};
  tocp.theta.tab = {8, terms[11], coef + 11}, tocp.ce.tab = {6, terms[19], coef + 19};
  tocp.crl = crl, tocp.cru = cru, tocp.cel = cel, tocp.ceu = ceu;
  auto tnlp = F::ocp_to_nlp<F::diff::Type::Analytic>(tocp, mesh);
  // the lambdas and the tables are one problem
  if (std::fabs(nlp.f(x) - tnlp.f(x)) > 1e-12) return 2;
  {
    const std::vector<double> a = nlp.g(x), b = tnlp.g(x);
    for (std::size_t i = 0; i < m; ++i)
      if (std::fabs(a[i] - b[i]) > 1e-12) return 3;
    if (nlp.gl() != tnlp.gl() || nlp.gu() != tnlp.gu() || nlp.xl() != tnlp.xl()) return 4;
  }
  // differences of f, g, lambda' g (central)
  const auto lg = [&](auto & p, const std::vector<double> & xx) {
    const std::vector<double> & gv = p.g(xx);
    double s = 0;
    for (std::size_t i = 0; i < m; ++i) s += lambda[i] * gv[i];
    return s;
  };
  const auto approx = [](const std::vector<double> & a, const std::vector<double> & b, double tol) {
    double d = 0, na = 0, nb = 0;
    for (std::size_t i = 0; i < a.size(); ++i) d += (a[i] - b[i]) * (a[i] - b[i]), na += a[i] * a[i], nb += b[i] * b[i];
    return std::sqrt(d) <= tol * std::sqrt(std::min(na, nb));
  };
  const double h1 = 1e-6, h2 = 1e-4;
  std::vector<double> df_num(n), dg_num(m * n), d2f_num(n * n), d2g_num(n * n);
  for (std::size_t c = 0; c < n; ++c) {
    std::vector<double> xp = x, xm = x;
    xp[c] += h1, xm[c] -= h1;
    df_num[c] = (tnlp.f(xp) - tnlp.f(xm)) / (2 * h1);
    const std::vector<double> gp = tnlp.g(xp), gm = tnlp.g(xm);
    for (std::size_t r = 0; r < m; ++r) dg_num[r * n + c] = (gp[r] - gm[r]) / (2 * h1);
    for (std::size_t b = c; b < n; ++b) {
      std::vector<double> pp = x, pm = x, mp = x, mm = x;
      pp[c] += h2, pp[b] += h2, pm[c] += h2, pm[b] -= h2, mp[c] -= h2, mp[b] += h2, mm[c] -= h2, mm[b] -= h2;
      d2f_num[c * n + b] = d2f_num[b * n + c] = ((tnlp.f(pp) - tnlp.f(pm)) - (tnlp.f(mp) - tnlp.f(mm))) / (4 * h2 * h2);
      d2g_num[c * n + b] = d2g_num[b * n + c] = ((lg(tnlp, pp) - lg(tnlp, pm)) - (lg(tnlp, mp) - lg(tnlp, mm))) / (4 * h2 * h2);
    }
  }
  const auto dense_csr = [&](const F::MeshCsr & A) {
    std::vector<double> out((std::size_t)A.rows * n, 0.0);
    for (int r = 0; r < A.rows; ++r)
      for (int p = A.rowptr[r]; p < A.rowptr[r + 1]; ++p) out[(std::size_t)r * n + A.colind[p]] = A.val[p];
    return out;
  };
  const auto dense_sym = [&](const F::MeshCsc & H) {
    std::vector<double> out(n * n, 0.0);
    for (int c = 0; c < H.cols; ++c)
      for (int p = H.colptr[c]; p < H.colptr[c + 1]; ++p) out[(std::size_t)H.rowind[p] * n + c] = out[(std::size_t)c * n + H.rowind[p]] = H.val[p];
    return out;
  };
  int at = 5;
  for (int pass = 0; pass < 2; ++pass) {  // the tables' closed forms, then the lambdas' differences
    const auto run = [&](auto & p) {
      if (!approx(dense_csr(p.df_dx(x)), df_num, 1e-4)) return 0;
      if (!approx(dense_csr(p.dg_dx(x)), dg_num, 1e-4)) return 1;
      if (!approx(dense_sym(p.d2f_dx2(x)), d2f_num, 1e-3)) return 2;
      if (!approx(dense_sym(p.d2g_dx2(x, lambda)), d2g_num, 1e-3)) return 3;
      return 4;
    };
    const int ok = pass == 0 ? run(tnlp) : run(nlp);
    if (ok != 4) return at + ok;
    at += 4;
  }
  return 0;
}

// the two trajectory scenarios of the reference's tests/test_collocation_mesh_function.cpp (:522-628) as caller code;
// returns 0, or the number of the first expectation that fails
int sfbx_test_mesh_function_api(void)
{
  namespace F = smooth::feedback;
  const double t0 = 3, tf = 5;
  F::Mesh<5, 5> m;
  m.refine_ph(0, 40);
  const std::size_t N = m.N_colloc();
  const std::vector<F::Rn<0>> U(N);
  const auto maxabs = [](const std::vector<double> & v) {
    double r = 0;
    for (const double e : v) r = std::max(r, std::fabs(e));
    return r;
  };
  {  // x(t) = 0.1 t^2 - 0.4 t + 0.2
    std::vector<F::Rn<1>> X(N + 1);
    const auto nodes = m.all_nodes();
    for (std::size_t i = 0; i <= N; ++i) {
      const double s = t0 + (tf - t0) * nodes[i];
      X[i].v[0]      = 0.1 * s * s - 0.4 * s + 0.2;
    }
    const auto df_dt = [](double t, const F::Rn<1> &, const F::Rn<0> &) { return F::Vec<1>{0.2 * t - 0.4}; };
    const auto g     = [](double, const F::Rn<1> & x, const F::Rn<0> &) { return F::Vec<1>{0.1 + x.v[0] * x.v[0]}; };
    F::MeshValue<0> out;
    F::mesh_integrate(out, m, g, t0, tf, X, U);
    if (!(std::fabs(out.F[0] - (0.217333 + 0.1 * (tf - t0))) <= 1e-4)) return 1;
    F::MeshValue<1> dyn;
    F::mesh_dyn<1>(dyn, m, df_dt, t0, tf, X, U);
    if (dyn.F.size() != N || !(maxabs(dyn.F) <= 1e-8)) return 2;
  }
  {  // x(t) = 1.5 exp(-t)
    std::vector<F::Rn<1>> X(N + 1);
    const auto nodes = m.all_nodes();
    for (std::size_t i = 0; i <= N; ++i) X[i].v[0] = 1.5 * std::exp(-(t0 + (tf - t0) * nodes[i]));
    const auto df_dt = [](double, const F::Rn<1> & x, const F::Rn<0> &) { return F::Vec<1>{-x.v[0]}; };
    const auto g     = [](double, const F::Rn<1> & x, const F::Rn<0> &) { return F::Vec<1>{x.v[0] * x.v[0]}; };
    F::MeshValue<0> out;
    F::mesh_integrate(out, m, g, t0, tf, X, U);
    if (!(std::fabs(out.F[0] - 0.00273752) <= 1e-4)) return 3;
    F::MeshValue<1> dyn;
    F::mesh_dyn<1>(dyn, m, df_dt, t0, tf, X, U);
    if (dyn.F.size() != N || !(maxabs(dyn.F) <= 1e-8)) return 4;
  }
  return 0;
}

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

// ---- flatten_ocp (ocp_flatten.hpp) through examples/flat_ocp_harness.h ----
int sfbx_flat_lie_eval(int group, int op, int64_t count, const double * in, double * out)
{
  if (count < 0 || op < 0 || op > 1) return -1;
  const bool ok = sfbx::flat_lie_dispatch(group, [&]<class G>() {
    constexpr int T = G::Dof;
    for (int64_t k = 0; k < count; ++k) sfbx::flat_lie_item<G>(op, in + k * (op == 0 ? T : 2 * T), out + k * T * T);
  });
  return ok ? 0 : -1;
}

int sfbx_flat_ocp_sizes(int problem, int32_t N, int32_t * sizes)
{
  const bool ok = sfbx::flat_dispatch_problem(problem, [&]<class Ocp>() {
    using S = sfbx::FlatSizes<Ocp>;
    const int32_t v[7] = {S::Nx, S::Nu, S::Nq, S::Ncr, S::Nce, S::stride, (int32_t)S::n(N)};
    std::copy(v, v + 7, sizes);
  });
  return ok ? 0 : -1;
}

int sfbx_flat_ocp_nodes_host(int problem, int64_t agents, int32_t N, const double * tau, const double * x, const double * traj, double * Ff, double * dFf,
                             double * Fg, double * dFg, double * Fcr, double * dFcr, double * ce, double * dce, double * theta, double * dtheta, int threads)
{
  if (agents < 0 || N < 1 || threads < 1) return -1;
  const bool ok = sfbx::flat_dispatch_problem(problem, [&]<class Ocp>() {
    using S = sfbx::FlatSizes<Ocp>;
    const auto part = [&](int64_t b0, int64_t b1) {  // agents [b0, b1): every pointer moved to agent b0
      const auto model = sfbx::flat_swarm_model<Ocp>(traj + b0 * S::stride);
      const sfbx::FlatNodeOut o{Ff + b0 * N * S::Nx,   dFf + b0 * N * S::Nx * S::nz,   Fg + b0 * N * S::Nq, dFg + b0 * N * S::Nq * S::nz,
                                Fcr + b0 * N * S::Ncr, dFcr + b0 * N * S::Ncr * S::nz, ce + b0 * S::Nce,    dce + b0 * S::Nce * S::ne,
                                theta + b0,            dtheta + b0 * S::ne};
      sfbx::flat_nodes_host(model, b1 - b0, N, tau, x + b0 * S::n(N), o);
    };
    if (threads == 1) return part(0, agents);
    std::vector<std::thread> pool;
    for (int k = 0; k < threads; ++k) pool.emplace_back(part, agents * k / threads, agents * (k + 1) / threads);
    for (auto & th : pool) th.join();
  });
  return ok ? 0 : -1;
}

int sfbx_flat_ocp_nlp_host(int problem, int mesh_kind, int64_t agents, const double * x, const double * traj, double * g, double * dg, double * f, double * df,
                           int64_t * differing, int32_t * sizes, double * taus)
{
  if (agents < 0) return -1;
  try {
    const auto mesh = sfbx::flat_mesh(mesh_kind);
    const bool ok   = sfbx::flat_dispatch_problem(problem, [&]<class Ocp>() {
      using S          = sfbx::FlatSizes<Ocp>;
      const auto model = sfbx::flat_swarm_model<Ocp>(traj);
      auto nlp0        = sf::ocp_to_nlp(sfbx::flat_agent_ocp(model, 0), mesh);
      const int64_t n = (int64_t)nlp0.n(), m = (int64_t)nlp0.m(), nnz = nlp0.tables().nnz;
      if (sizes) sizes[0] = (int32_t)n, sizes[1] = (int32_t)m, sizes[2] = (int32_t)nnz, sizes[3] = (int32_t)mesh.N_colloc();
      if (taus) {
        const std::vector<double> t = mesh.all_nodes();
        std::copy(t.begin(), t.end(), taus);
      }
      if (!x) return;
      for (int64_t b = 0; b < agents; ++b)
        sfbx::flat_nlp_host(model, b, mesh, x + b * n, g ? g + b * m : nullptr, dg ? dg + b * nnz : nullptr, f ? f + b : nullptr,
                            df ? df + b * S::ne : nullptr, differing ? differing + b : nullptr);
    });
    return ok ? 0 : -1;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "collocation harness: %s\n", e.what());
    return -2;
  }
}

int sfbx_flat_ocp_hess_nodes_host(int problem, int64_t agents, int32_t N, const double * tau, const double * x, const double * lam, const double * traj,
                                  double * HLf, double * HLg, double * HLcr, double * d2theta, double * d2ce_l, int threads)
{
  if (agents < 0 || N < 1 || threads < 1) return -1;
  const bool ok = sfbx::flat_dispatch_problem(problem, [&]<class Ocp>() {
    using S = sfbx::FlatSizes<Ocp>;
    int64_t cb[5];
    sfbx::flat_con_beg<Ocp>(N, cb);
    const auto part = [&](int64_t b0, int64_t b1) {  // agents [b0, b1): every pointer moved to agent b0
      const auto model = sfbx::flat_swarm_model<Ocp>(traj + b0 * S::stride);
      const int64_t sq = (int64_t)N * S::nz * S::nz, se = (int64_t)S::ne * S::ne;
      sfbx::flat_hess_nodes_host(model, b1 - b0, N, tau, x + b0 * S::n(N), lam + b0 * cb[4],
                                 sfbx::FlatHessOut{HLf + b0 * sq, HLg + b0 * sq, HLcr + b0 * sq, d2theta + b0 * se, d2ce_l + b0 * se});
    };
    if (threads == 1) return part(0, agents);
    std::vector<std::thread> pool;
    for (int k = 0; k < threads; ++k) pool.emplace_back(part, agents * k / threads, agents * (k + 1) / threads);
    for (auto & th : pool) th.join();
  });
  return ok ? 0 : -1;
}

int sfbx_flat_ocp_hess_host(int problem, int mesh_kind, int64_t agents, const double * x, const double * lam, const double * sigma, const double * traj,
                            int value_differences, double * hess, int64_t * differing, int64_t * nnz_hess, int threads)
{
  if (agents < 0 || threads < 1) return -1;
  try {
    const auto mesh = sfbx::flat_mesh(mesh_kind);
    const bool ok   = sfbx::flat_dispatch_problem(problem, [&]<class Ocp>() {
      const auto model = sfbx::flat_swarm_model<Ocp>(traj);
      auto nlp0        = sf::ocp_to_nlp(sfbx::flat_agent_ocp(model, 0), mesh);
      const int64_t n = (int64_t)nlp0.n(), m = (int64_t)nlp0.m(), nnz = nlp0.hess_tables().nnz;
      if (nnz_hess) *nnz_hess = nnz;
      if (!x) return;
      const auto part = [&](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) {
          if (value_differences) {  // the default flattened problem: OCPNLP's second differences of the flat values
            auto nlp = sf::ocp_to_nlp(sfbx::flat_agent_ocp(model, b), mesh);
            const std::vector<double> xv(x + b * n, x + (b + 1) * n), lv(lam + b * m, lam + (b + 1) * m);
            const auto & H = nlp.d2l_dx2(xv, sigma[b], lv);
            if (hess) std::copy(H.val.begin(), H.val.end(), hess + b * nnz);
          } else {
            sfbx::flat_hess_nlp_host(model, b, mesh, x + b * n, lam + b * m, sigma[b], hess ? hess + b * nnz : nullptr, differing ? differing + b : nullptr);
          }
        }
      };
      if (threads == 1) return part(0, agents);
      std::vector<std::thread> pool;
      for (int k = 0; k < threads; ++k) pool.emplace_back(part, agents * k / threads, agents * (k + 1) / threads);
      for (auto & th : pool) th.join();
    });
    return ok ? 0 : -1;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "collocation harness: %s\n", e.what());
    return -2;
  }
}

// The opt-in Hessians of flatten_ocp<FlatHess::Differences> as caller code; figures [8].  Returns 0 or the first failing expectation.
//   1  a QUADRATIC problem on Rn around affine trajectories: the flat Hessians against P' H P, H the analytic Hessian of the
//      original at (t, xl + e, ul + v) and P the constant Jacobian of (t, xl(t) + e, ul(t) + v).  The flat Jacobian is linear in
//      z there, so its central difference has no truncation; what is left is rounding.  figures: worst error, bound, per family.
//   2  the default flatten_ocp has no hessian member (static), the opt-in one has.
int sfbx_test_flatten_hess_api(double * figures)
{
  namespace F = smooth::feedback;
  for (int k = 0; k < 8; ++k) figures[k] = 0.0;
  constexpr int NX = 2, NU = 1, NQ = 1, NCR = 1, NCE = 2, nz = 1 + NX + NU, ne = 1 + 2 * NX + NQ;
  // z = (t, x0, x1, u0): f = (x0 u0 + t^2 / 2, x1^2 - t x0), g = x0^2 + u0^2 + x0 x1, cr = x1 u0 + t u0
  // ze = (tf, x0_0, x0_1, xf_0, xf_1, q): theta = tf q + x0_0 xf_1 + xf_0^2, ce = (tf xf_0, x0_1^2 + q xf_1)
  const int32_t tf_[] = {0, 1, 1, 3, 1, 0, 0,  0, 0, 2, 0, 0, 0, 0,  1, 2, 2, 0, 0, 0, 0,  1, 0, 1, 1, 1, 0, 0};
  const double cf_[]  = {1, 0.5, 1, -1};
  const int32_t tg_[] = {0, 1, 2, 0, 0, 0, 0,  0, 3, 2, 0, 0, 0, 0,  0, 1, 1, 2, 1, 0, 0};
  const double cg_[]  = {1, 1, 1};
  const int32_t tc_[] = {0, 2, 1, 3, 1, 0, 0,  0, 0, 1, 3, 1, 0, 0};
  const double cc_[]  = {1, 1};
  const int32_t tt_[] = {0, 0, 1, 5, 1, 0, 0,  0, 1, 1, 4, 1, 0, 0,  0, 3, 2, 0, 0, 0, 0};
  const double ct_[]  = {1, 1, 1};
  const int32_t te_[] = {0, 0, 1, 3, 1, 0, 0,  1, 2, 2, 0, 0, 0, 0,  1, 5, 1, 4, 1, 0, 0};
  const double ce_[]  = {1, 1, 1};
  sfbx::TermOcp<NX, NU, NQ, NCR, NCE> ocp{};
  ocp.f.tab = {4, tf_, cf_}, ocp.g.tab = {3, tg_, cg_}, ocp.cr.tab = {2, tc_, cc_}, ocp.theta.tab = {3, tt_, ct_}, ocp.ce.tab = {3, te_, ce_};
  if (!ocp.f.tab.valid(NX, nz) || !ocp.g.tab.valid(NQ, nz) || !ocp.cr.tab.valid(NCR, nz) || !ocp.theta.tab.valid(1, ne) || !ocp.ce.tab.valid(NCE, ne)) return 100;
  const F::Vec<NX> a{0.3, -0.2}, da{0.1, 0.25};
  const F::Vec<NU> c{0.2}, dc{-0.3};
  const auto xl = F::trajectory([=](double t) { F::Rn<NX> x; for (int i = 0; i < NX; ++i) x.v[i] = a[i] + t * da[i]; return x; }, [=](double) { return da; });
  const auto ul = F::trajectory([=](double t) { F::Rn<NU> u; for (int i = 0; i < NU; ++i) u.v[i] = c[i] + t * dc[i]; return u; }, [=](double) { return dc; });
  const auto plain = F::flatten_ocp(ocp, xl, ul);
  const auto flat  = F::flatten_ocp<F::FlatHess::Differences>(ocp, xl, ul);
  // ---- 2 ----
  {
    F::Rn<NX> e{};
    F::Rn<NU> v{};
    F::Vec<NQ> q{};
    F::Mat<nz, NX * nz> Hf;
    F::Mat<ne, ne> Ht;
    static_assert(!sfbx::flat_has_hessian<decltype(plain.f), double, decltype(e), decltype(v), decltype(Hf)> &&
                  !sfbx::flat_has_hessian<decltype(plain.theta), double, decltype(e), decltype(e), decltype(q), decltype(Ht)>);
    static_assert(sfbx::flat_has_hessian<decltype(flat.f), double, decltype(e), decltype(v), decltype(Hf)> &&
                  sfbx::flat_has_hessian<decltype(flat.theta), double, decltype(e), decltype(e), decltype(q), decltype(Ht)>);
    (void)e, (void)v, (void)q, (void)Hf, (void)Ht;
  }
  // ---- 1 ----
  const double t = 0.37, tfv = 1.3;
  F::Rn<NX> e, e0, ef;
  F::Rn<NU> v;
  F::Vec<NQ> q{0.45};
  e.v = {0.21, -0.34}, e0.v = {-0.15, 0.4}, ef.v = {0.33, 0.12}, v.v = {0.27};
  F::Mat<nz, nz> P = F::Mat<nz, nz>::Zero();  // d (t, x, u) / d (t, e, v)
  for (int k = 0; k < nz; ++k) P(k, k) = 1.0;
  for (int k = 0; k < NX; ++k) P(1 + k, 0) = da[k];
  for (int k = 0; k < NU; ++k) P(1 + NX + k, 0) = dc[k];
  F::Mat<ne, ne> Pe = F::Mat<ne, ne>::Zero();  // d (tf, x0, xf, q) / d (tf, e0, ef, q): xf = xl(tf) + ef
  for (int k = 0; k < ne; ++k) Pe(k, k) = 1.0;
  for (int k = 0; k < NX; ++k) Pe(1 + NX + k, 0) = da[k];
  const double h = F::detail::flat_hess_step, eps = std::numeric_limits<double>::epsilon();
  double worst = 0.0, hmax = 0.0;
  const auto compare = [&]<int NF, int NV>(const F::Mat<NV, NF * NV> & got, const F::Mat<NV, NF * NV> & H, const F::Mat<NV, NV> & Pm) {
    double err = 0.0;
    for (int r = 0; r < NF; ++r)
      for (int i = 0; i < NV; ++i)
        for (int j = 0; j < NV; ++j) {
          double want = 0.0;
          for (int k = 0; k < NV; ++k)
            for (int l = 0; l < NV; ++l) want += Pm(k, i) * H(k, r * NV + l) * Pm(l, j);
          err  = std::max(err, std::fabs(got(i, r * NV + j) - want));
          hmax = std::max(hmax, std::fabs(want));
        }
    worst = std::max(worst, err);
    return err;
  };
  const F::Rn<NX> x = rplus(xl(t), e.v), x0 = rplus(xl(0.0), e0.v), xf = rplus(xl(tfv), ef.v);
  const F::Rn<NU> u = rplus(ul(t), v.v);
  {
    F::Mat<nz, NX * nz> got, H;
    flat.f.hessian(t, e, v, got), ocp.f.hessian(t, x, u, H);
    figures[2] = compare.template operator()<NX, nz>(got, H, P);
  }
  {
    F::Mat<nz, NQ * nz> got, H;
    flat.g.hessian(t, e, v, got), ocp.g.hessian(t, x, u, H);
    figures[3] = compare.template operator()<NQ, nz>(got, H, P);
  }
  {
    F::Mat<nz, NCR * nz> got, H;
    flat.cr.hessian(t, e, v, got), ocp.cr.hessian(t, x, u, H);
    figures[4] = compare.template operator()<NCR, nz>(got, H, P);
  }
  {
    F::Mat<ne, ne> got, H;
    flat.theta.hessian(tfv, e0, ef, q, got), ocp.theta.hessian(tfv, x0, xf, q, H);
    figures[5] = compare.template operator()<1, ne>(got, H, Pe);
  }
  {
    F::Mat<ne, NCE * ne> got, H;
    flat.ce.hessian(tfv, e0, ef, q, got), ocp.ce.hessian(tfv, x0, xf, q, H);
    figures[6] = compare.template operator()<NCE, ne>(got, H, Pe);
  }
  // An entry of the flat Jacobian is a sum of at most ne = 6 products of numbers below 2, each from a few roundings: off by at
  // most 16 ne eps.  The difference of two of them over 2 h is off by 16 ne eps / h = 2.8e-9; nothing else, the Jacobian being
  // linear in z and z +- h e_a exact to eps |z| (which moves the quotient by eps |z| / h |H|, inside the same bound).
  const double bound = 16.0 * ne * eps / h * (1.0 + hmax);
  figures[0] = worst, figures[1] = bound;
  if (!(hmax >= 1.0)) return 101;  // the Hessians are there: entries 1 and 2
  if (!(worst <= bound)) return 102;
  return 0;
}

// Caller code against <smooth/feedback/ocp_flatten.hpp> under the reference's names; figures [8] receives what each
// scenario measured.  Returns 0, or the number of the first expectation that fails.
//   1  a flattened Rn problem (term tables of ocp_nlp_harness.h around affine trajectories) gives the NLP of the original
//      at x = xl + e: g, and dg with the tf column corrected by the chain rule through xl(tf tau_i), ul(tf tau_i)
//   2  unflatten_ocpsol(nlpsol_to_ocpsol(flat)) at the nodes: x(t_i) = xl(t_i) (+) e_i, u likewise, Q and multipliers carried
//   3  d2l_dx2 of the flattened planar vehicle (symmetric from its upper triangle) against central differences of sigma df + lambda' dg
//   4  spline_trajectory: the adapter's point is the spline's, its velocity the body velocity of the curve
int sfbx_test_flatten_api(double * figures)
{
  namespace F = smooth::feedback;
  for (int k = 0; k < 8; ++k) figures[k] = 0.0;
  // ---- 1 ----
  {
    constexpr int NX = 3, NU = 2, NQ = 2, NCR = 1, NCE = 3, nz = 1 + NX + NU, ne = 1 + 2 * NX + NQ;
    // f = (x1 + sin u0, -x0 + t u1, x2 x0), g = (x0^2 + u0^2, cos x2), cr = x1 u1, theta = tf + q0 + x0_0 xf_1, ce = (tf, x0_0, xf_2 q1)
    const int32_t tf_[] = {0, 2, 1, 0, 0, 0, 0,  0, 4, 3, 0, 0, 0, 0,  1, 1, 1, 0, 0, 0, 0,  1, 0, 1, 5, 1, 0, 0,  2, 3, 1, 1, 1, 0, 0};
    const double cf_[]  = {1, 1, -1, 1, 1};
    const int32_t tg_[] = {0, 1, 2, 0, 0, 0, 0,  0, 4, 2, 0, 0, 0, 0,  1, 3, 4, 0, 0, 0, 0};
    const double cg_[]  = {1, 1, 1};
    const int32_t tc_[] = {0, 2, 1, 5, 1, 0, 0};
    const double cc_[]  = {1};
    const int32_t tt_[] = {0, 0, 1, 0, 0, 0, 0,  0, 7, 1, 0, 0, 0, 0,  0, 1, 1, 5, 1, 0, 0};
    const double ct_[]  = {1, 1, 1};
    const int32_t te_[] = {0, 0, 1, 0, 0, 0, 0,  1, 1, 1, 0, 0, 0, 0,  2, 6, 1, 8, 1, 0, 0};
    const double ce_[]  = {1, 1, 1};
    sfbx::TermOcp<NX, NU, NQ, NCR, NCE> ocp{};
    ocp.f.tab = {5, tf_, cf_}, ocp.g.tab = {3, tg_, cg_}, ocp.cr.tab = {1, tc_, cc_}, ocp.theta.tab = {3, tt_, ct_}, ocp.ce.tab = {3, te_, ce_};
    if (!ocp.f.tab.valid(NX, nz) || !ocp.g.tab.valid(NQ, nz) || !ocp.cr.tab.valid(NCR, nz) || !ocp.theta.tab.valid(1, ne) || !ocp.ce.tab.valid(NCE, ne)) return 100;
    const F::Vec<NX> a{0.3, -0.2, 0.5}, da{0.1, 0.25, -0.15};
    const F::Vec<NU> c{0.2, -0.4}, dc{-0.3, 0.2};
    const auto xl = F::trajectory([=](double t) { F::Rn<NX> x; for (int i = 0; i < NX; ++i) x.v[i] = a[i] + t * da[i]; return x; }, [=](double) { return da; });
    const auto ul = F::trajectory([=](double t) { F::Rn<NU> u; for (int i = 0; i < NU; ++i) u.v[i] = c[i] + t * dc[i]; return u; }, [=](double) { return dc; });
    F::Mesh<3, 6> mesh(2, 3);
    mesh.set_N_colloc_ival(1, 4);
    auto orig = F::ocp_to_nlp(ocp, mesh);
    auto flat = F::ocp_to_nlp(F::flatten_ocp(ocp, xl, ul), mesh);
    if (orig.n() != flat.n() || orig.m() != flat.m()) return 101;
    const std::size_t n = orig.n(), N = mesh.N_colloc();
    const std::vector<double> taus = mesh.all_nodes();
    std::vector<double> z(n), xo(n);
    for (std::size_t k = 0; k < n; ++k) z[k] = 0.3 * std::sin(1.0 + 1.7 * (double)k);
    z[0] = 1.3;
    xo   = z;
    const auto xcol = [&](std::size_t i, int d) { return 1 + NQ + i * NX + d; };
    const auto ucol = [&](std::size_t i, int d) { return 1 + NQ + (N + 1) * NX + i * NU + d; };
    for (std::size_t i = 0; i <= N; ++i) {
      const double t = z[0] * taus[i];
      for (int d = 0; d < NX; ++d) xo[xcol(i, d)] = xl(t).v[d] + z[xcol(i, d)];
      if (i < N)
        for (int d = 0; d < NU; ++d) xo[ucol(i, d)] = ul(t).v[d] + z[ucol(i, d)];
    }
    const std::vector<double> go = orig.g(xo), gf = flat.g(z);
    double eg = 0.0, ej = 0.0, ef = std::fabs(orig.f(xo) - flat.f(z));
    for (std::size_t r = 0; r < go.size(); ++r) eg = std::max(eg, std::fabs(go[r] - gf[r]));
    const F::MeshCsr Jo = orig.dg_dx(xo), Jf = flat.dg_dx(z);
    if (Jo.colind != Jf.colind || Jo.rowptr != Jf.rowptr) return 102;
    for (std::size_t r = 0; r + 1 < Jo.rowptr.size(); ++r) {
      double tfcol = 0.0, chain = 0.0, got = 0.0;
      for (int32_t p = Jo.rowptr[r]; p < Jo.rowptr[r + 1]; ++p) {
        const std::size_t col = (std::size_t)Jo.colind[p];
        if (col == 0) { tfcol = Jo.val[p], got = Jf.val[p]; continue; }
        if (col >= xcol(0, 0) && col < ucol(0, 0)) chain += Jo.val[p] * da[(col - xcol(0, 0)) % NX] * taus[(col - xcol(0, 0)) / NX];
        else if (col >= ucol(0, 0)) chain += Jo.val[p] * dc[(col - ucol(0, 0)) % NU] * taus[(col - ucol(0, 0)) / NU];
        ej = std::max(ej, std::fabs(Jo.val[p] - Jf.val[p]));
      }
      ej = std::max(ej, std::fabs(tfcol + chain - got));
    }
    figures[0] = eg, figures[1] = ej, figures[2] = ef;
    // the same functions at the same points: what is left is the rounding of xl + e against the collocation of xl (exact
    // for an affine trajectory), a few ulps of numbers of size 10
    if (!(eg <= 1e-12) || !(ej <= 1e-12) || !(ef <= 1e-12)) return 103;
  }
  // ---- 2 and 3: the planar vehicle around a constant-twist trajectory ----
  {
    using Ocp = sfbx::OcpSE2;
    using S   = sfbx::FlatSizes<Ocp>;
    const double row[S::stride] = {0.4, -0.3, std::cos(0.7), std::sin(0.7), 0.2, 0.1, 1.1, 0.05, 0.4, 0.3, -0.2, 0.1, 0.3, -0.25, 0.15};
    const auto model = sfbx::flat_swarm_model<Ocp>(row);
    const auto focp  = sfbx::flat_agent_ocp(model, 0);
    F::Mesh<3, 5> mesh(2, 3);
    auto nlp = F::ocp_to_nlp(focp, mesh);
    static_assert(F::HessianNLP<decltype(nlp)>);
    const std::size_t n = nlp.n(), m = nlp.m(), N = mesh.N_colloc();
    F::NLPSolution s;
    s.x.resize(n), s.lambda.resize(m);
    for (std::size_t k = 0; k < n; ++k) s.x[k] = 0.2 * std::sin(0.5 + 1.3 * (double)k);
    for (std::size_t k = 0; k < m; ++k) s.lambda[k] = 0.5 * std::cos(0.2 + 0.9 * (double)k);
    s.x[0] = 2.0;
    const auto flatsol = F::nlpsol_to_ocpsol(focp, mesh, s);
    const auto sol     = F::unflatten_ocpsol<Ocp::X, Ocp::U, Ocp::Nq, Ocp::Ncr, Ocp::Nce>(flatsol, F::AgentStateTrajectory<sfbx::FlatSwarmModel<Ocp>>{&model, 0},
                                                                                      F::AgentInputTrajectory<sfbx::FlatSwarmModel<Ocp>>{&model, 0});
    const std::vector<double> taus = mesh.all_nodes();
    double er = 0.0;
    for (std::size_t i = 0; i <= N; ++i) {
      const double t = s.x[0] * taus[i];
      const auto de  = rminus(sol.x(t), model.xl(0, t));
      for (int d = 0; d < S::Nx; ++d) er = std::max(er, std::fabs(de[d] - s.x[1 + S::Nq + i * S::Nx + d]));
      if (i < N) {
        const auto dv = rminus(sol.u(t), model.ul(0, t));
        for (int d = 0; d < S::Nu; ++d) er = std::max(er, std::fabs(dv[d] - s.x[1 + S::Nq + (N + 1) * S::Nx + i * S::Nu + d]));
      }
    }
    figures[3] = er;
    // log(exp(e)) and the interpolation at a node: a few ulps of numbers below 1
    if (!(er <= 1e-13)) return 200;
    if (sol.tf != s.x[0] || sol.Q[0] != s.x[1] || sol.lambda_q[0] != flatsol.lambda_q[0] || sol.lambda_ce != flatsol.lambda_ce) return 201;
    if (sol.lambda_dyn(0.3) != flatsol.lambda_dyn(0.3) || sol.lambda_cr(0.3) != flatsol.lambda_cr(0.3)) return 202;
    // ---- 3 ----
    const double sigma = 0.7;
    const F::MeshCsc H = nlp.d2l_dx2(s.x, sigma, s.lambda);
    std::vector<double> Hd(n * n, 0.0);
    for (std::size_t c = 0; c < n; ++c)
      for (int32_t p = H.colptr[c]; p < H.colptr[c + 1]; ++p) Hd[(std::size_t)H.rowind[p] * n + c] = Hd[c * n + (std::size_t)H.rowind[p]] = H.val[p];
    const auto grad = [&](const std::vector<double> & xx) {
      std::vector<double> gr(n, 0.0);
      const F::MeshCsr & D = nlp.df_dx(xx);
      for (std::size_t k = 0; k < D.val.size(); ++k) gr[(std::size_t)D.colind[k]] += sigma * D.val[k];
      const F::MeshCsr & J = nlp.dg_dx(xx);
      for (std::size_t r = 0; r < m; ++r)
        for (int32_t p = J.rowptr[r]; p < J.rowptr[r + 1]; ++p) gr[(std::size_t)J.colind[p]] += s.lambda[r] * J.val[p];
      return gr;
    };
    double eh = 0.0, hmax = 0.0;
    for (const double v : Hd) hmax = std::max(hmax, std::fabs(v));
    const double h = 2e-3;  // (chosen below)
    for (std::size_t c = 0; c < n; ++c) {
      auto xp = s.x, xm = s.x;
      xp[c] += h, xm[c] -= h;
      const auto gp = grad(xp), gm = grad(xm);
      for (std::size_t r = 0; r < n; ++r) eh = std::max(eh, std::fabs((gp[r] - gm[r]) / (2 * h) - Hd[r * n + c]));
    }
    figures[4] = eh, figures[5] = hmax;
    // The integrand carries no jacobian, so dg holds forward differences at 2^-26 of its flat value: noise of 2 eps |g| 2^26 =
    // 3e-8 |g| in the gradient.  A central difference of that gradient at step h has noise 3e-8 / h and truncation h^2 / 6
    // times a third derivative; they meet near h = 2e-3, at 1.5e-5 and some 1e-6.  d2l itself (differences of differences of
    // the flat values at step eps^(1/4) = 1.2e-4) adds eps |f| / h^2 = 1.5e-8 |f| and h^2 / 12 = 1e-9 times a fourth derivative,
    // times the weights of the sum.  Bound: 1e-4 (1 + max |H|), a factor of a few over those.  A Hessian off by a factor, or
    // a missing cross block, is off by 1e-2 or more.
    if (!(eh <= 1e-4 * (1.0 + hmax))) return 300;
  }
  // ---- 4: a Spline as a trajectory: the adapter returns the spline's point, and its velocity is the curve's body velocity ----
  {
    std::vector<double> tt;
    std::vector<F::SE2> gg;
    for (int k = 0; k <= 4; ++k) tt.push_back(0.5 * k), gg.push_back(F::SE2::exp({0.5 * k * 1.0, 0.1 * k, 0.5 * k * 0.6}));
    const auto spline = F::fit_spline_cubic<F::SE2>(tt, gg);
    const auto xl     = F::spline_trajectory(spline);
    double ev = 0.0;
    for (const double t : {0.3, 0.9, 1.6}) {
      const F::SE2 a = xl(t), b = spline(t);
      if (a.x != b.x || a.y != b.y || a.c != b.c || a.s != b.s) return 400;
      const double h = 1e-5;
      const auto d   = rminus(xl(t + h), xl(t - h));
      const auto v   = xl.velocity(t);
      for (int i = 0; i < 3; ++i) ev = std::max(ev, std::fabs(d[i] / (2 * h) - v[i]));
    }
    figures[6] = ev;
    // a central difference at 1e-5 of a cubic curve with coefficients of size 1: truncation 1e-10, rounding eps / h = 2e-11
    if (!(ev <= 1e-8)) return 401;
  }
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
