// Pattern builder of the swarm SQP solver (nlp_sqp_plan.h).  No HIP: it is also compiled into tests/nlp_sqp_plan_check.cpp.
#include "nlp_sqp_plan.h"

#include <cmath>

namespace sfb {

bool build_nlp_sqp_pattern(int n, int m, const int32_t *Jp, const int32_t *Jj, const int32_t *Hp, const int32_t *Hi, const double *xl,
                           const double *xu, const double *gl, const double *gu, NlpSqpPattern &o, const char **msg)
{
  static const char *ok = "";
  *msg = ok;
  o = NlpSqpPattern();
  if (n < 1 || m < 0 || !Jp || !Hp || !xl || !xu || (m > 0 && (!gl || !gu))) { *msg = "bad sizes / NULL pattern or bounds"; return false; }
  if (Jp[0] != 0 || Hp[0] != 0 || Jp[m] < 0 || Hp[n] < 0) { *msg = "pattern pointers must start at 0"; return false; }
  if ((Jp[m] > 0 && !Jj) || (Hp[n] > 0 && !Hi)) { *msg = "NULL index array"; return false; }
  o.n = n; o.m = m; o.nnzJ = Jp[m]; o.nnzH = Hp[n];
  for (int r = 0; r < m; ++r)
    if (Jp[r + 1] < Jp[r] || Jp[r + 1] > o.nnzJ) { *msg = "dg_dx row pointers not monotone"; return false; }
  for (int c = 0; c < n; ++c)
    if (Hp[c + 1] < Hp[c] || Hp[c + 1] > o.nnzH) { *msg = "Hessian column pointers not monotone"; return false; }
  for (int r = 0; r < m; ++r)
    for (int p = Jp[r]; p < Jp[r + 1]; ++p) {
      if (Jj[p] < 0 || Jj[p] >= n) { *msg = "dg_dx column index out of range"; return false; }
      if (p > Jp[r] && Jj[p] <= Jj[p - 1]) { *msg = "dg_dx column indices must be strictly ascending per row"; return false; }
    }
  for (int c = 0; c < n; ++c)
    for (int p = Hp[c]; p < Hp[c + 1]; ++p) {
      if (Hi[p] < 0 || Hi[p] > c) { *msg = "Hessian row index outside the upper triangle"; return false; }
      if (p > Hp[c] && Hi[p] <= Hi[p - 1]) { *msg = "Hessian row indices must be strictly ascending per column"; return false; }
    }
  for (int c = 0; c < n; ++c)  // rows ascend and stay <= c: the diagonal is the column's last entry or it is missing
    if (Hp[c + 1] == Hp[c] || Hi[Hp[c + 1] - 1] != c) { *msg = "Hessian pattern misses a diagonal entry"; return false; }
  for (int j = 0; j < n; ++j)
    if (xl[j] > xu[j]) { *msg = "xl > xu"; return false; }
  for (int r = 0; r < m; ++r)
    if (gl[r] > gu[r]) { *msg = "gl > gu"; return false; }
  for (int j = 0; j < n; ++j)
    if (std::isnan(xl[j]) || std::isnan(xu[j])) { *msg = "NaN variable bound"; return false; }
  for (int r = 0; r < m; ++r)
    if (std::isnan(gl[r]) || std::isnan(gu[r])) { *msg = "NaN constraint bound"; return false; }

  // P = both triangles: column c holds its upper entries (rows <= c, as the Hessian stores them), then the mirror images of
  // the entries (c, r) of the columns r > c.  Walking the Hessian's columns in ascending order fills them rows ascending.
  o.nnzP = 2 * o.nnzH - n;
  o.P_colptr.assign(n + 1, 0);
  for (int c = 0; c < n; ++c)
    for (int p = Hp[c]; p < Hp[c + 1]; ++p) {
      ++o.P_colptr[c + 1];
      if (Hi[p] != c) ++o.P_colptr[Hi[p] + 1];
    }
  for (int c = 0; c < n; ++c) o.P_colptr[c + 1] += o.P_colptr[c];
  o.P_rowind.resize(o.nnzP);
  o.P_src.resize(o.nnzP);
  o.P_diag.resize(n);
  {
    std::vector<int32_t> lower(n);  // where the next mirrored entry of a column goes
    for (int c = 0; c < n; ++c) lower[c] = o.P_colptr[c] + (Hp[c + 1] - Hp[c]);
    for (int c = 0; c < n; ++c) {
      for (int p = Hp[c]; p < Hp[c + 1]; ++p) {
        const int t   = o.P_colptr[c] + (p - Hp[c]);
        o.P_rowind[t] = Hi[p];
        o.P_src[t]    = p;
        if (Hi[p] != c) {
          const int w   = lower[Hi[p]]++;
          o.P_rowind[w] = c;
          o.P_src[w]    = p;
        }
      }
      o.P_diag[c] = o.P_colptr[c] + (Hp[c + 1] - Hp[c]) - 1;
    }
  }

  o.bound_row.assign(n, -1);
  for (int j = 0; j < n; ++j)
    if (std::isfinite(xl[j]) || std::isfinite(xu[j])) {
      o.bound_row[j] = (int32_t)o.bound_var.size();
      o.bound_var.push_back(j);
    }
  o.nb = (int)o.bound_var.size();
  o.A_rowptr.assign(Jp, Jp + m + 1);
  o.A_colind.assign(Jj, Jj + o.nnzJ);
  for (int i = 0; i < o.nb; ++i) {
    o.A_colind.push_back(o.bound_var[i]);
    o.A_rowptr.push_back(o.nnzJ + i + 1);
  }
  // CSC view of dg_dx by a counting pass over the rows in ascending order: rows come out ascending within a column
  o.Jc_colptr.assign(n + 1, 0);
  for (int p = 0; p < o.nnzJ; ++p) ++o.Jc_colptr[Jj[p] + 1];
  for (int c = 0; c < n; ++c) o.Jc_colptr[c + 1] += o.Jc_colptr[c];
  o.Jc_row.resize(o.nnzJ);
  o.Jc_pos.resize(o.nnzJ);
  std::vector<int32_t> next(o.Jc_colptr.begin(), o.Jc_colptr.end() - 1);
  for (int r = 0; r < m; ++r)
    for (int p = Jp[r]; p < Jp[r + 1]; ++p) {
      const int t = next[Jj[p]]++;
      o.Jc_row[t] = r;
      o.Jc_pos[t] = p;
    }
  return true;
}

}  // namespace sfb
