// Host<->kernel interface of the swarm SQP solver (nlp_sqp.hip; the law is in DESIGN.md, "Swarm SQP").  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sfb {

constexpr int kNlpRunning = -1;  // status of an agent that has not finished (the other values: NLPSolution::Status)
constexpr int kNlpOptimal = 0, kNlpPrimalInfeasible = 1, kNlpMaxIterations = 3, kNlpUnknown = 5;

// Everything the kernels index with travels as kernel argument: sizes, the shared patterns and bounds, the per-agent state.
struct NlpSqpDev {
  int n, m, nb, mq, nnzJ, nnzH, nnzP, nnzA;  // mq = m + nb rows and nnzA = nnzJ + nb entries of the QP's A; nnzP = 2 nnzH - n
  int max_iter;
  double tol, kappa, mu_first, mu_grow, mu_max;
  const int32_t *P_row, *P_col, *P_src;  // [nnzP] row, column and Hessian value of every entry of P (both triangles)
  const int32_t *Jc_colptr, *Jc_row, *Jc_pos, *bound_var, *bound_row;
  const double *xl, *xu, *gl, *gu;
  // state, [batch] or [batch][len]
  double *x, *lambda, *z, *mu, *nu, *alpha, *r_stat, *r_pri, *r_comp, *v1, *phi0, *slope, *d, *yqp, *dd, *dPd;
  int32_t *status, *iter, *phase, *need, *halvings;  // phase 1: in line search; need 1: its QP is to be (re-)solved
};

// law 4: residuals, v1 and the status decision of every unfinished agent; need[b] = 1 for those that stay unfinished
hipError_t nlp_sqp_kkt_launch(const NlpSqpDev &p, int64_t batch, const double *df, const double *g, const double *dg_val, hipStream_t s);
// list = the agents with flag != 0 in ascending order, *count = how many
hipError_t nlp_sqp_compact_launch(const int32_t *flag, int64_t batch, int32_t *list, int32_t *count, hipStream_t s);
// law 1 for the listed agents, written compacted: slot k holds agent list[k]
hipError_t nlp_sqp_assemble_launch(const NlpSqpDev &p, const int32_t *list, int64_t count, const double *df, const double *g,
                                   const double *dg_val, const double *hess_val, double *Px, double *q, double *Ax, double *l, double *u,
                                   double *wx, double *wy, hipStream_t s);
// law 2 on the results (xs, ys, code) of the listed agents; accepted agents enter the line search (law 3: nu, phi, D)
hipError_t nlp_sqp_judge_launch(const NlpSqpDev &p, const int32_t *list, int64_t count, int rung, const double *f, const double *Px,
                                const double *q, const double *xs, const double *ys, const int32_t *code, hipStream_t s);
hipError_t nlp_sqp_trial_launch(const NlpSqpDev &p, int64_t batch, double *x_trial, hipStream_t s);
hipError_t nlp_sqp_accept_launch(const NlpSqpDev &p, int64_t batch, const double *f_trial, const double *g_trial, hipStream_t s);
// x, lambda, z from the caller (NULL multipliers: zero); mu, nu, iter, status and the warm starts reset
hipError_t nlp_sqp_start_launch(const NlpSqpDev &p, int64_t batch, const double *x, const double *lambda, const double *z, hipStream_t s);

}  // namespace sfb
