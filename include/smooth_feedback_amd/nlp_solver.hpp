// solve_nlp_sqp: ONE nonlinear program (nlp.hpp's HessianNLP) through the swarm SQP solver of sfb.h (sfb_nlp_sqp_*)
// with batch 1 -- the place of the reference's solve_nlp_ipopt (compat/ipopt.hpp).  The NLP is evaluated on the host, every
// array is staged through the host-pointer entries; the QPs are solved on the GPU by the sparse solver.  The method is local
// (l1 merit, no second-order correction): give it a start, as `warmstart`, wherever one is known.
#pragma once
#include <sfb.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "nlp.hpp"
#include "qp.hpp"

namespace smooth_feedback_amd {

/// sfb_nlp_sqp_params
struct NLPSQPParams {
  double tol           = 1e-6;
  std::size_t max_iter = 50;
  double kappa = 1e-8, mu_first = 1e-4, mu_grow = 8.0, mu_max = 1e4;
  QPSolverParams qp = [] {
    QPSolverParams p;
    p.eps_abs = p.eps_rel = 1e-9f;
    p.max_iter            = 10000;
    return p;
  }();
};

namespace detail {
inline void sqp_check(sfb_status st, const char * what)
{
  if (st != SFB_OK) throw std::runtime_error(std::string(what) + ": " + sfb_last_error());
}
struct SqpHandle {
  sfb_nlp_sqp * h = nullptr;
  ~SqpHandle() { sfb_nlp_sqp_destroy(h); }
};
}  // namespace detail

/// warmstart: x, lambda and zu - zl of an earlier solution (without one: x = 0 clipped to its bounds, multipliers 0).
/// Throws std::invalid_argument when d2f_dx2 and d2g_dx2 do not share one pattern (or change it between calls) and
/// std::runtime_error when the library refuses a call.
template<HessianNLP Nlp>
NLPSolution solve_nlp_sqp(Nlp && nlp, const std::optional<NLPSolution> & warmstart = {}, const NLPSQPParams & prm = {})
{
  const std::size_t n = nlp.n(), m = nlp.m();
  const std::vector<double> xl = nlp.xl(), xu = nlp.xu(), gl = nlp.gl(), gu = nlp.gu();
  std::vector<double> x(n, 0.0), lambda(m, 0.0), z(n, 0.0);
  if (warmstart) {
    if (warmstart->x.size() != n || warmstart->lambda.size() != m || warmstart->zl.size() != n || warmstart->zu.size() != n)
      throw std::invalid_argument("solve_nlp_sqp: warmstart of another size");
    x = warmstart->x, lambda = warmstart->lambda;
    for (std::size_t j = 0; j < n; ++j) z[j] = warmstart->zu[j] - warmstart->zl[j];
  }
  for (std::size_t j = 0; j < n; ++j) x[j] = std::min(std::max(x[j], xl[j]), xu[j]);

  // the patterns: dg_dx as the NLP stores it, and the ONE pattern d2f_dx2 and d2g_dx2 must share
  const MeshCsr J0 = nlp.dg_dx(x);
  const MeshCsc H0 = nlp.d2f_dx2(x);
  const auto same_pattern = [&H0](const MeshCsc & a) { return a.colptr == H0.colptr && a.rowind == H0.rowind; };
  {
    const MeshCsc G0 = nlp.d2g_dx2(x, lambda);
    if (!same_pattern(G0)) throw std::invalid_argument("solve_nlp_sqp: d2f_dx2 and d2g_dx2 do not share one pattern");
  }
  sfb_nlp_sqp_params c;
  sfb_nlp_sqp_params_default(&c);
  c.tol = prm.tol, c.max_iter = (int64_t)prm.max_iter, c.kappa = prm.kappa;
  c.mu_first = prm.mu_first, c.mu_grow = prm.mu_grow, c.mu_max = prm.mu_max;
  c.qp = prm.qp.to_c();
  detail::SqpHandle H;
  detail::sqp_check(sfb_nlp_sqp_create((int)n, (int)m, J0.rowptr.data(), J0.colind.data(), H0.colptr.data(), H0.rowind.data(), xl.data(), xu.data(),
                                       gl.data(), gu.data(), 1, &c, nullptr, &H.h),
                    "sfb_nlp_sqp_create");
  detail::sqp_check(sfb_nlp_sqp_set_start_host(H.h, x.data(), lambda.data(), z.data()), "sfb_nlp_sqp_set_start_host");

  std::vector<double> df(n), hess(H0.val.size()), xt(n);
  for (;;) {
    detail::sqp_check(sfb_nlp_sqp_state_host(H.h, x.data(), lambda.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                      "sfb_nlp_sqp_state_host");
    const double f              = nlp.f(x);
    const std::vector<double> g = nlp.g(x);
    const MeshCsr dfx = nlp.df_dx(x), J = nlp.dg_dx(x);
    const MeshCsc Hf = nlp.d2f_dx2(x), Hg = nlp.d2g_dx2(x, lambda);
    if (J.rowptr != J0.rowptr || J.colind != J0.colind) throw std::invalid_argument("solve_nlp_sqp: dg_dx changed its pattern");
    if (!same_pattern(Hf) || !same_pattern(Hg)) throw std::invalid_argument("solve_nlp_sqp: d2f_dx2 / d2g_dx2 changed or do not share their pattern");
    std::fill(df.begin(), df.end(), 0.0);
    for (std::size_t e = 0; e < dfx.colind.size(); ++e) df[(std::size_t)dfx.colind[e]] = dfx.val[e];
    for (std::size_t e = 0; e < hess.size(); ++e) hess[e] = Hf.val[e] + Hg.val[e];
    int64_t searching = 0;
    detail::sqp_check(sfb_nlp_sqp_direction_host(H.h, &f, df.data(), g.data(), J.val.data(), hess.data(), &searching), "sfb_nlp_sqp_direction_host");
    if (searching == 0) break;  // finished: an agent that goes on holds a direction
    while (searching) {
      detail::sqp_check(sfb_nlp_sqp_trial_host(H.h, xt.data()), "sfb_nlp_sqp_trial_host");
      const double ft              = nlp.f(xt);
      const std::vector<double> gt = nlp.g(xt);
      detail::sqp_check(sfb_nlp_sqp_accept_host(H.h, &ft, gt.data(), &searching), "sfb_nlp_sqp_accept_host");
    }
  }
  NLPSolution sol;
  int32_t status = 0, iter = 0;
  sol.x.resize(n), sol.lambda.resize(m), sol.zl.assign(n, 0.0), sol.zu.assign(n, 0.0);
  detail::sqp_check(sfb_nlp_sqp_state_host(H.h, sol.x.data(), sol.lambda.data(), z.data(), &status, &iter, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                    "sfb_nlp_sqp_state_host");
  for (std::size_t j = 0; j < n; ++j) (z[j] > 0 ? sol.zu[j] : sol.zl[j]) = std::fabs(z[j]);
  sol.status    = static_cast<NLPSolution::Status>(status);  // the C values are NLPSolution::Status's
  sol.iter      = (std::size_t)iter;
  sol.objective = nlp.f(sol.x);
  return sol;
}

}  // namespace smooth_feedback_amd
