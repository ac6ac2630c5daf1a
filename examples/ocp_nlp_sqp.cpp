// Harness entry of solve_nlp_sqp (part of libsfb_models.so): the scenario of the reference's tests/test_ocp_ipopt.cpp as caller
// code against the reference's include paths and namespace -- the double integrator from (1, 1) to (0, 0), theta = q, integrand
// |x|^2 + |u|^2, -1 <= u <= 1, ce = (tf, x0, xf) with tf in [tf_lo, tf_hi] -- transcribed by ocp_to_nlp on two intervals of
// degree 4 and solved by solve_nlp_sqp from the caller's start; then nlpsol_to_ocpsol and ocpsol_to_nlpsol there and back.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <vector>

#include <smooth/feedback/collocation/mesh.hpp>
#include <smooth/feedback/nlp_solver.hpp>
#include <smooth/feedback/ocp_to_nlp.hpp>

extern "C" {

// x0 [n]: the start (n must be the NLP's, 28).  Out: x [n], lambda [m = 30], *iter, *objective, roundtrip [4] = the 2-norms of
// the differences of (x, zl, zu, lambda) after nlpsol_to_ocpsol / ocpsol_to_nlpsol.  Returns the NLPSolution::Status value,
// -2 after an exception, -3 for a start of another size.
int sfbx_ocp_nlp_sqp(double tf_lo, double tf_hi, const double * x0, int n_given, double tol, int max_iter, double * x, double * lambda,
                     int32_t * iter, double * objective, double * roundtrip)
{
  namespace F = smooth::feedback;
  using X = F::Rn<2>;
  using U = F::Rn<1>;
  try {
    const auto theta = [](double, const X &, const X &, const F::Vec<1> & q) { return q[0]; };
    const auto f     = [](double, const X & xx, const U & u) { return F::Vec<2>{xx.v[1], u.v[0]}; };
    const auto g     = [](double, const X & xx, const U & u) { return F::Vec<1>{xx.v[0] * xx.v[0] + xx.v[1] * xx.v[1] + u.v[0] * u.v[0]}; };
    const auto cr    = [](double, const X &, const U & u) { return F::Vec<1>{u.v[0]}; };
    const auto ce    = [](double tf, const X & a, const X & b, const F::Vec<1> &) { return F::Vec<5>{tf, a.v[0], a.v[1], b.v[0], b.v[1]}; };
    const F::Vec<1> crl{-1}, cru{1};
    const F::Vec<5> cel{tf_lo, 1, 1, 0, 0}, ceu{tf_hi, 1, 1, 0, 0};
    const auto ocp = F::make_ocp<X, U>(theta, f, g, cr, crl, cru, ce, cel, ceu);
    F::Mesh<4, 4> mesh(2, 4);
    auto nlp = F::ocp_to_nlp(ocp, mesh);
    static_assert(F::HessianNLP<decltype(nlp)>);
    const std::size_t n = nlp.n(), m = nlp.m();
    if ((int)n != n_given) return -3;
    F::NLPSolution start;
    start.x.assign(x0, x0 + n);
    start.lambda.assign(m, 0.0), start.zl.assign(n, 0.0), start.zu.assign(n, 0.0);
    F::NLPSQPParams prm;
    prm.tol = tol, prm.max_iter = (std::size_t)max_iter;
    const F::NLPSolution sol = F::solve_nlp_sqp(nlp, start, prm);
    for (std::size_t j = 0; j < n; ++j) x[j] = sol.x[j];
    for (std::size_t r = 0; r < m; ++r) lambda[r] = sol.lambda[r];
    *iter = (int32_t)sol.iter, *objective = sol.objective;
    const auto ocp_sol     = F::nlpsol_to_ocpsol(ocp, mesh, sol);
    const F::NLPSolution c = F::ocpsol_to_nlpsol(ocp, mesh, ocp_sol);
    const auto dist = [](const std::vector<double> & a, const std::vector<double> & b) {
      if (a.size() != b.size()) return (double)INFINITY;
      double s = 0;
      for (std::size_t i = 0; i < a.size(); ++i) s += (a[i] - b[i]) * (a[i] - b[i]);
      return std::sqrt(s);
    };
    roundtrip[0] = dist(c.x, sol.x), roundtrip[1] = dist(c.zl, sol.zl), roundtrip[2] = dist(c.zu, sol.zu), roundtrip[3] = dist(c.lambda, sol.lambda);
    return (int)sol.status;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "ocp_nlp_sqp harness: %s\n", e.what());
    return -2;
  }
}

}  // extern "C"
