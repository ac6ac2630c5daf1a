// Host-only pattern work of the swarm SQP solver ("Swarm SQP"): from the shared patterns of dg_dx (CSR) and of the
// Lagrangian Hessian (upper-triangle CSC) and the bounds, everything the kernels of nlp_sqp.hip index with.
#pragma once
#include <cstdint>
#include <vector>

namespace sfb {

struct NlpSqpPattern {
  int n = 0, m = 0, nb = 0, nnzJ = 0, nnzH = 0, nnzP = 0;
  // the QP's P: BOTH triangles of the Hessian in CSC (rows ascending), because the sparse solver takes the entries with col >= row into
  // its KKT matrix but multiplies by P AS STORED in its residuals; P_src: the Hessian value every stored entry copies
  std::vector<int32_t> P_colptr, P_rowind, P_src;
  std::vector<int32_t> A_rowptr, A_colind;  // the QP's A: the rows of dg_dx, then one row e_j per bounded variable (ascending j)
  std::vector<int32_t> P_diag;              // [n] slot of P(j, j) in P's value array
  std::vector<int32_t> Jc_colptr, Jc_row, Jc_pos;  // CSC view of dg_dx: per column its rows ascending and their CSR positions
  std::vector<int32_t> bound_var;           // [nb] variable of bound row i
  std::vector<int32_t> bound_row;           // [n] bound row of variable j, -1 without one
};

// false with *msg set: in this order bad sizes, unsorted or out-of-range indices, a missing diagonal, xl > xu or gl > gu, a NaN bound
bool build_nlp_sqp_pattern(int n, int m, const int32_t *J_rowptr, const int32_t *J_colind, const int32_t *H_colptr, const int32_t *H_rowind,
                           const double *xl, const double *xu, const double *gl, const double *gu, NlpSqpPattern &o, const char **msg);

}  // namespace sfb
