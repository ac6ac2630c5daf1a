// Nonlinear programs as the collocation front hands them to a solver (reference nlp.hpp): the NLP / HessianNLP concepts
// and NLPSolution, on this repository's types -- vectors are std::vector<double>, first derivatives MeshCsr (CSR, the
// form QuadraticProgramSparse::A_* has), second derivatives MeshCsc (upper triangle in CSC, as P_*).  No solver lives
// here (the reference's is external as well): a swarm of NLPs sharing these patterns is solved on the GPU by the swarm SQP
// solver, sfb_nlp_sqp_* of sfb.h (smooth_feedback_amd/nlp.py), which takes exactly these values as device arrays; solve_nlp_sqp of
// nlp_solver.hpp runs it for one HessianNLP.
#pragma once
#include <concepts>
#include <cstddef>
#include <type_traits>
#include <vector>

#include "mesh_function.hpp"

namespace smooth_feedback_amd {

/// min f(x) s.t. xl <= x <= xu, gl <= g(x) <= gu
template<class T>
concept NLP = requires(std::decay_t<T> & nlp, const std::vector<double> & x) {
  { nlp.n() } -> std::convertible_to<std::size_t>;
  { nlp.m() } -> std::convertible_to<std::size_t>;
  { nlp.xl() } -> std::convertible_to<std::vector<double>>;
  { nlp.xu() } -> std::convertible_to<std::vector<double>>;
  { nlp.f(x) } -> std::convertible_to<double>;
  { nlp.df_dx(x) } -> std::convertible_to<MeshCsr>;
  { nlp.g(x) } -> std::convertible_to<std::vector<double>>;
  { nlp.gl() } -> std::convertible_to<std::vector<double>>;
  { nlp.gu() } -> std::convertible_to<std::vector<double>>;
  { nlp.dg_dx(x) } -> std::convertible_to<MeshCsr>;
};

/// ... with the Hessians of f and of lambda' g (upper triangles)
template<class T>
concept HessianNLP = NLP<T> && requires(std::decay_t<T> & nlp, const std::vector<double> & x, const std::vector<double> & lambda) {
  { nlp.d2f_dx2(x) } -> std::convertible_to<MeshCsc>;
  { nlp.d2g_dx2(x, lambda) } -> std::convertible_to<MeshCsc>;
};

struct NLPSolution {
  enum class Status { Optimal, PrimalInfeasible, DualInfeasible, MaxIterations, MaxTime, Unknown };
  Status status{Status::Unknown};
  std::size_t iter{0};
  std::vector<double> x;       ///< variables
  std::vector<double> zl, zu;  ///< multipliers of the variable bounds
  std::vector<double> lambda;  ///< multipliers of the constraints
  double objective{0};
};

}  // namespace smooth_feedback_amd
