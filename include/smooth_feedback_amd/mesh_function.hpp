// Functions over a collocation mesh with first and multiplier-weighted second derivatives (reference
// collocation/mesh_function.hpp): MeshValue<Deriv>, mesh_eval (:114-246), mesh_integrate (:273-419), mesh_dyn (:450-665),
// on plain arrays.  Variables [t0 | tf | x_0 .. x_N | u_0 .. u_{N-1}], numVars = 2 + nx (N + 1) + nu N.
//
// One law: the arithmetic of every output entry of orders 0 and 1 is written once below (namespace meshfn, SFB_LIE_HD);
// the host loops of this header and the batched kernels of smooth_feedback_amd/csrc/mesh.hip both call it, and both add
// sums over nodes in node order.  The sparsity patterns are built once as well (meshfn::*_pattern: the host front, and
// sfb_mesh_eval_pattern / sfb_mesh_dyn_pattern of the C-ABI).  The same holds for the Lagrangian Hessian of the collocation
// NLP (meshfn::ocp_nlp_hess_pattern / _value below): one law and one record builder for OCPNLP::d2l_dx2 and the kernel.
//
// dF is CSR in the form QuadraticProgramSparse::A_* has, d2F the upper triangle in CSC as P_*.  Derivatives with respect
// to x and u are right-Jacobians.  mesh_eval and mesh_integrate take any state / input type of the Lie layer for
// Deriv <= 1; mesh_dyn's defect subtracts sum_k D(k, j) x_k and therefore needs a vector state (Rn), as the reference's
// `coef * x` does.  Deriv == 2 needs Rn state and input.
#pragma once
#include <cmath>
#include <cstdint>
#include <iterator>
#include <limits>
#include <tuple>
#include <type_traits>
#include <vector>

#include "lie.hpp"
#include "mesh.hpp"

namespace smooth_feedback_amd {

namespace diff {
/// how the integrand is differentiated: by its jacobian / hessian members, by differences, or members where they exist
enum class Type { Numerical, Analytic, Default };
}  // namespace diff

/// rows x cols CSR (QuadraticProgramSparse::A_*)
struct MeshCsr {
  int32_t rows = 0, cols = 0;
  std::vector<int32_t> rowptr, colind;
  std::vector<double> val;
};
/// upper triangle of a symmetric rows x cols matrix in CSC (QuadraticProgramSparse::P_*)
struct MeshCsc {
  int32_t rows = 0, cols = 0;
  std::vector<int32_t> colptr, rowind;
  std::vector<double> val;
};

template<uint8_t Deriv>
struct MeshValue;
template<>
struct MeshValue<0> {
  std::vector<double> F;  ///< function value
  bool allocated{false};  ///< true: sizes and patterns are taken as correct and no output array is (re)allocated
};
template<>
struct MeshValue<1> : public MeshValue<0> {
  MeshCsr dF;  ///< size(F) x numVars
};
template<>
struct MeshValue<2> : public MeshValue<1> {
  std::vector<double> lambda;  ///< multipliers, one per row of F (set by the caller)
  MeshCsc d2F;                 ///< numVars x numVars, upper triangle
};

/// zero the values, keep the patterns (lambda is the caller's)
template<uint8_t Deriv>
void set_zero(MeshValue<Deriv> & mv)
{
  for (double & v : mv.F) v = 0.0;
  if constexpr (Deriv >= 1)
    for (double & v : mv.dF.val) v = 0.0;
  if constexpr (Deriv >= 2)
    for (double & v : mv.d2F.val) v = 0.0;
}

// ---- the law: one function per kind of output entry (f: a model value, df*: an entry of its Jacobian (t | x | u)) ----
namespace meshfn {

// mesh_eval (:192-201); w is the quadrature weight when scaling, else 1
SFB_LIE_HD inline double eval_F(double w, double f) { return w * f; }
SFB_LIE_HD inline double eval_dt0(double w, double tau, double dft) { return (w * (1. - tau)) * dft; }
SFB_LIE_HD inline double eval_dtf(double w, double tau, double dft) { return (w * tau) * dft; }
SFB_LIE_HD inline double eval_dz(double w, double dfz) { return w * dfz; }

// mesh_integrate (:348-361): what node i adds to the running sums (callers add in node order); h = tf - t0
SFB_LIE_HD inline void integrate_F_add(double & acc, double w, double h, double f) { acc += w * h * f; }
SFB_LIE_HD inline void integrate_dt0_add(double & acc, double w, double h, double tau, double f, double dft)
{
  acc += (w * h * (1. - tau)) * dft;
  acc += (-w) * f;
}
SFB_LIE_HD inline void integrate_dtf_add(double & acc, double w, double h, double tau, double f, double dft)
{
  acc += (w * h * tau) * dft;
  acc += w * f;
}
SFB_LIE_HD inline double integrate_dz(double w, double h, double dfz) { return (w * h) * dfz; }

// mesh_dyn (:545-560, :626-664): row (node M + j of an interval of K points, component d); D(k, j) = Dcol[k], k = 0 .. K
SFB_LIE_HD inline double dyn_coef(double w, double alpha, double Dkj) { return -w * alpha * Dkj; }
/// F = w h f_d - w alpha sum_k D(k, j) x_{M + k, d}: the f term first, then k ascending; x: component d of x_M, rows ldx apart
SFB_LIE_HD inline double dyn_F(int K, double w, double h, double alpha, const double * Dcol, double f, const double * x, int64_t ldx)
{
  double acc = w * h * f;
  for (int k = 0; k <= K; ++k) acc += dyn_coef(w, alpha, Dcol[k]) * x[k * ldx];
  return acc;
}
SFB_LIE_HD inline double dyn_dt0(double w, double h, double tau, double f, double dft)
{
  double acc = (-w) * f;
  acc += (w * h * (1. - tau)) * dft;
  return acc;
}
SFB_LIE_HD inline double dyn_dtf(double w, double h, double tau, double f, double dft)
{
  double acc = w * f;
  acc += (w * h * tau) * dft;
  return acc;
}
/// entry (d, c) of the row's own nx-wide block; Djj = D(j, j)
SFB_LIE_HD inline double dyn_own(double w, double h, double alpha, double Djj, double dfx, bool diagonal)
{
  double acc = (w * h) * dfx;
  if (diagonal) acc += dyn_coef(w, alpha, Djj);
  return acc;
}
SFB_LIE_HD inline double dyn_du(double w, double h, double dfu) { return (w * h) * dfu; }

/// What position p of a mesh_dyn row (node j of an interval of K points) holds: kind 0 t0, 1 tf, 2 another node k's
/// single entry (idx = k), 3 the own block (idx = c), 4 u (idx = c).  2 + K + nx + nu positions, columns ascending.
SFB_LIE_HD inline void dyn_decode(int p, int j, int K, int nx, int & kind, int & idx)
{
  if (p < 2) { kind = p; idx = 0; return; }
  const int q = p - 2;
  if (q < j) { kind = 2; idx = q; }
  else if (q < j + nx) { kind = 3; idx = q - j; }
  else if (q < nx + K) { kind = 2; idx = q - nx + 1; }
  else { kind = 4; idx = q - nx - K; }
}

// ---- patterns (host).  rowptr [rows + 1], colind [nnz]; NULL arrays: only the count is returned ----
inline int64_t eval_pattern(int64_t N, int nx, int nu, int nf, int32_t * rowptr, int32_t * colind)
{
  const int64_t per = 2 + nx + nu, rows = N * nf;
  if (rowptr && colind) {
    for (int64_t r = 0; r <= rows; ++r) rowptr[r] = (int32_t)(r * per);
    for (int64_t r = 0; r < rows; ++r) {
      const int64_t i = r / nf;
      int32_t * c     = colind + r * per;
      *c++ = 0; *c++ = 1;
      for (int k = 0; k < nx; ++k) *c++ = (int32_t)(2 + i * nx + k);
      for (int k = 0; k < nu; ++k) *c++ = (int32_t)(2 + (N + 1) * nx + i * nu + k);
    }
  }
  return rows * per;
}
inline int64_t dyn_pattern(int nivals, const int32_t * K, int nx, int nu, int32_t * rowptr, int32_t * colind)
{
  int64_t N = 0, nnz = 0;
  for (int s = 0; s < nivals; ++s) N += K[s], nnz += (int64_t)K[s] * nx * (2 + K[s] + nx + nu);
  if (rowptr && colind) {
    int64_t M = 0, e = 0, row = 0;
    for (int s = 0; s < nivals; ++s) {
      for (int j = 0; j < K[s]; ++j)
        for (int d = 0; d < nx; ++d) {
          rowptr[row++] = (int32_t)e;
          for (int p = 0; p < 2 + K[s] + nx + nu; ++p) {
            int kind, idx;
            dyn_decode(p, j, K[s], nx, kind, idx);
            colind[e++] = (int32_t)(kind < 2 ? kind : kind == 2 ? 2 + (M + idx) * nx + d : kind == 3 ? 2 + (M + j) * nx + idx : 2 + (N + 1) * nx + (M + j) * nu + idx);
          }
        }
      M += K[s];
    }
    rowptr[row] = (int32_t)e;
  }
  return nnz;
}
/// the upper triangle shared by the three functions' d2F (:159-175): column t0 {t0}, tf {t0, tf}, component j of x_i
/// {t0, tf, x_i0 .. x_ij}, component j of u_i {t0, tf, x_i, u_i0 .. u_ij}; the columns of x_N are empty
inline void d2_pattern(int64_t N, int nx, int nu, MeshCsc & H)
{
  const int64_t nv = 2 + nx * (N + 1) + nu * N;
  H.rows = H.cols = (int32_t)nv;
  H.colptr.assign((size_t)nv + 1, 0);
  H.rowind.clear();
  for (int64_t c = 0; c < nv; ++c) {
    if (c < 2) {
      for (int64_t r = 0; r <= c; ++r) H.rowind.push_back((int32_t)r);
    } else if (c < 2 + nx * N) {
      const int64_t i = (c - 2) / nx, j = (c - 2) % nx;
      H.rowind.push_back(0); H.rowind.push_back(1);
      for (int64_t r = 0; r <= j; ++r) H.rowind.push_back((int32_t)(2 + i * nx + r));
    } else if (c >= 2 + nx * (N + 1)) {
      const int64_t i = (c - 2 - nx * (N + 1)) / nu, j = (c - 2 - nx * (N + 1)) % nu;
      H.rowind.push_back(0); H.rowind.push_back(1);
      for (int64_t r = 0; r < nx; ++r) H.rowind.push_back((int32_t)(2 + i * nx + r));
      for (int64_t r = 0; r <= j; ++r) H.rowind.push_back((int32_t)(2 + nx * (N + 1) + i * nu + r));
    }
    H.colptr[(size_t)c + 1] = (int32_t)H.rowind.size();
  }
  H.val.assign(H.rowind.size(), 0.0);
}

// ---- the collocation NLP of an OCP over a mesh (ocp_to_nlp.hpp; sfb_ocp_nlp_* of the C-ABI) ----
// Variables [tf | q (nq) | x_0 .. x_N | u_0 .. u_{N-1}] (t0 = 0), constraints [dyn nx N | integrals nq | running ncr N | end nce].
struct OcpDims {
  int32_t nx, nu, nq, ncr, nce;
};

// what the NLP adds to the laws above: the mesh-weight scaling ws, ws (I - q), the -ws of the integral rows' q entry, and
// the end constraint, which passes through unscaled
SFB_LIE_HD inline double nlp_scaled(double ws, double v) { return ws * v; }
SFB_LIE_HD inline double nlp_integral(double ws, double I, double q) { return ws * (I - q); }
SFB_LIE_HD inline double nlp_minus_identity(double ws) { return -ws; }
SFB_LIE_HD inline double nlp_end(double v) { return v; }

/// var_beg (tf, q, x, u, n) and con_beg (dyn, integrals, running, end, m)
inline void ocp_nlp_structure(int64_t N, const OcpDims & d, int64_t var_beg[5], int64_t con_beg[5])
{
  const int64_t vl[4] = {1, d.nq, (int64_t)d.nx * (N + 1), (int64_t)d.nu * N};
  const int64_t cl[4] = {(int64_t)d.nx * N, d.nq, (int64_t)d.ncr * N, d.nce};
  var_beg[0] = con_beg[0] = 0;
  for (int k = 0; k < 4; ++k) var_beg[k + 1] = var_beg[k] + vl[k], con_beg[k + 1] = con_beg[k] + cl[k];
}

/// One output double of the NLP (a row of g, or an entry of dg_dx's pattern), decoded once per (mesh, dims): what it is,
/// the node whose weight / time it uses, where its source double sits within one agent's input, and where its mesh
/// coefficient sits in the table of differentiation matrices ((K + 1) x K per interval, one after the other).
struct OcpNlpItem {
  int32_t kind, node, src, aux;
};
enum OcpNlpKind : int32_t {
  kNlpGDyn,     // g, dyn row: src = i nx + d (in Ff), aux = column j of D
  kNlpGInt,     // g, integral r: src = r
  kNlpGCr,      // g, running: src = i ncr + r (in Fcr)
  kNlpGCe,      // g, end: src = r (in ce)
  kNlpDynTf,    // src = i nx + d (Ff; the time derivative is dFf[src nz])
  kNlpDynCoef,  // aux = D(k, j)
  kNlpDynOwn,   // src in dFf, aux = D(j, j)
  kNlpDynOwnDiag,
  kNlpDynDu,    // src in dFf
  kNlpIntTf,    // src = r: a sum over the nodes in node order
  kNlpIntQ,
  kNlpIntDz,    // src in dFg
  kNlpCrTf,     // src = i ncr + r (the time derivative is dFcr[src nz])
  kNlpCrDz,     // src in dFcr
  kNlpCeD,      // src in dce
};

/// CSR pattern of dg_dx (columns ascending, every reserved entry stored) and, with `items`, the decode records: the m
/// rows of g first, then the nnz entries.  NULL arrays: only the count is returned.
///   dyn row (node M + j, d): tf | per node k of the interval its component d, the own node the whole block | u_i
///   integral r: tf | q_r | x_0 .. x_{N-1} | u;   running (i, r): tf | x_i | u_i;   end r: tf | q | x_0 | x_N
inline int64_t ocp_nlp_pattern(int nivals, const int32_t * K, const OcpDims & dm, int32_t * rowptr, int32_t * colind, OcpNlpItem * items)
{
  const int nx = dm.nx, nu = dm.nu, nq = dm.nq, ncr = dm.ncr, nce = dm.nce, nz = 1 + nx + nu, ne = 1 + 2 * nx + nq;
  int64_t N = 0, nnz = 0;
  for (int s = 0; s < nivals; ++s) N += K[s], nnz += (int64_t)K[s] * nx * (1 + K[s] + nx + nu);
  nnz += (int64_t)nq * (2 + (int64_t)(nx + nu) * N) + (int64_t)ncr * N * (1 + nx + nu) + (int64_t)nce * (1 + nq + 2 * nx);
  const bool pat = rowptr && colind;
  if (!pat && !items) return nnz;
  const int64_t qv = 1, xv = 1 + nq, uv = xv + (int64_t)nx * (N + 1), m = (int64_t)nx * N + nq + (int64_t)ncr * N + nce;
  int64_t e = 0, row = 0;
  OcpNlpItem * gi = items, * di = items ? items + m : nullptr;
  const auto put = [&](int64_t col, int32_t kind, int64_t node, int64_t src, int64_t aux) {
    if (pat) colind[e] = (int32_t)col;
    if (di) di[e] = OcpNlpItem{kind, (int32_t)node, (int32_t)src, (int32_t)aux};
    ++e;
  };
  const auto begin_row = [&](int32_t kind, int64_t node, int64_t src, int64_t aux) {
    if (pat) rowptr[row] = (int32_t)e;
    if (gi) gi[row] = OcpNlpItem{kind, (int32_t)node, (int32_t)src, (int32_t)aux};
    ++row;
  };
  int64_t M = 0, Doff = 0;
  for (int s = 0; s < nivals; ++s) {
    const int Ks = K[s];
    for (int j = 0; j < Ks; ++j)
      for (int d = 0; d < nx; ++d) {
        const int64_t i = M + j, fr = i * nx + d, Dcol = Doff + (int64_t)j * (Ks + 1);
        begin_row(kNlpGDyn, i, fr, Dcol);
        put(0, kNlpDynTf, i, fr, 0);
        for (int k = 0; k <= Ks; ++k) {
          if (k != j) put(xv + (M + k) * nx + d, kNlpDynCoef, i, 0, Dcol + k);
          else
            for (int c = 0; c < nx; ++c) put(xv + i * nx + c, c == d ? kNlpDynOwnDiag : kNlpDynOwn, i, fr * nz + 1 + c, Dcol + j);
        }
        for (int c = 0; c < nu; ++c) put(uv + i * nu + c, kNlpDynDu, i, fr * nz + 1 + nx + c, 0);
      }
    M += Ks;
    Doff += (int64_t)(Ks + 1) * Ks;
  }
  for (int r = 0; r < nq; ++r) {
    begin_row(kNlpGInt, 0, r, 0);
    put(0, kNlpIntTf, 0, r, 0);
    put(qv + r, kNlpIntQ, 0, 0, 0);
    for (int64_t i = 0; i < N; ++i)
      for (int c = 0; c < nx; ++c) put(xv + i * nx + c, kNlpIntDz, i, (i * nq + r) * nz + 1 + c, 0);
    for (int64_t i = 0; i < N; ++i)
      for (int c = 0; c < nu; ++c) put(uv + i * nu + c, kNlpIntDz, i, (i * nq + r) * nz + 1 + nx + c, 0);
  }
  for (int64_t i = 0; i < N; ++i)
    for (int r = 0; r < ncr; ++r) {
      const int64_t fr = i * ncr + r;
      begin_row(kNlpGCr, i, fr, 0);
      put(0, kNlpCrTf, i, fr, 0);
      for (int c = 0; c < nx; ++c) put(xv + i * nx + c, kNlpCrDz, i, fr * nz + 1 + c, 0);
      for (int c = 0; c < nu; ++c) put(uv + i * nu + c, kNlpCrDz, i, fr * nz + 1 + nx + c, 0);
    }
  for (int r = 0; r < nce; ++r) {  // dce's columns are (tf | x0 | xf | q)
    begin_row(kNlpGCe, 0, r, 0);
    put(0, kNlpCeD, 0, (int64_t)r * ne, 0);
    for (int c = 0; c < nq; ++c) put(qv + c, kNlpCeD, 0, (int64_t)r * ne + 1 + 2 * nx + c, 0);
    for (int c = 0; c < nx; ++c) put(xv + c, kNlpCeD, 0, (int64_t)r * ne + 1 + c, 0);
    for (int c = 0; c < nx; ++c) put(xv + N * nx + c, kNlpCeD, 0, (int64_t)r * ne + 1 + nx + c, 0);
  }
  if (pat) rowptr[row] = (int32_t)e;
  return nnz;
}

/// per node: its time on [0, 1], quadrature weight, and its interval's 2 / length, point count and first node
struct OcpNlpNode {
  double tau, w, alpha;
  int32_t K, M;
};
/// what every agent of one (mesh, dims) shares
struct OcpNlpTables {
  OcpDims d;
  int32_t N;
  int64_t m, nnz;
  double ws;
  const OcpNlpNode * nodes;  // [N]
  const double * D;          // the unscaled differentiation matrices, D(k, j) of an interval at [k + j (K + 1)]
  const OcpNlpItem * items;  // [m + nnz]
};
/// one agent's arrays: x [n]; the model at the N nodes, F [N][nf] and dF [N][nf][1 + nx + nu] for f, g, cr; ce [nce], dce [nce][1 + 2 nx + nq]
struct OcpNlpAgent {
  const double *x, *Ff, *dFf, *Fg, *dFg, *Fcr, *dFcr, *ce, *dce;
};
/// an item with everything that does not depend on the agent looked up
struct OcpNlpLane {
  int32_t kind, src, K, xoff;  // xoff: component d of x_M within x (kNlpGDyn)
  double tau, w, alpha, Dv;
  const double * Dcol;
};
SFB_LIE_HD inline double ocp_nlp_w_scaling(double max_weight) { return 1. / (max_weight > 1e-6 ? max_weight : 1e-6); }

SFB_LIE_HD inline OcpNlpLane ocp_nlp_decode(const OcpNlpTables & T, const OcpNlpItem it)
{
  const OcpNlpNode nd = T.N > 0 ? T.nodes[it.node] : OcpNlpNode{};
  OcpNlpLane L{it.kind, it.src, nd.K, 0, nd.tau, nd.w, nd.alpha, 0.0, T.D + it.aux};
  if (it.kind == kNlpGDyn) L.xoff = 1 + T.d.nq + nd.M * T.d.nx + it.src % T.d.nx;
  if (it.kind == kNlpDynCoef || it.kind == kNlpDynOwn || it.kind == kNlpDynOwnDiag) L.Dv = T.D[it.aux];
  return L;
}

/// the value of one item for one agent: the laws above, then the multiplication by ws.  t0 = 0, so h = tf.
SFB_LIE_HD inline double ocp_nlp_value(const OcpNlpTables & T, const OcpNlpLane & L, const OcpNlpAgent & a)
{
  const int nx = T.d.nx, nq = T.d.nq, nz = 1 + nx + T.d.nu;
  const double ws = T.ws, tf = a.x[0], h = tf - 0.0;
  switch (L.kind) {
  case kNlpGDyn: return nlp_scaled(ws, dyn_F(L.K, L.w, h, L.alpha, L.Dcol, a.Ff[L.src], a.x + L.xoff, nx));
  case kNlpGInt: {
    double acc = 0.0;
    for (int i = 0; i < T.N; ++i) integrate_F_add(acc, T.nodes[i].w, h, a.Fg[(int64_t)i * nq + L.src]);
    return nlp_integral(ws, acc, a.x[1 + L.src]);
  }
  case kNlpGCr: return nlp_scaled(ws, eval_F(L.w, a.Fcr[L.src]));
  case kNlpGCe: return nlp_end(a.ce[L.src]);
  case kNlpDynTf: return nlp_scaled(ws, dyn_dtf(L.w, h, L.tau, a.Ff[L.src], a.dFf[(int64_t)L.src * nz]));
  case kNlpDynCoef: return nlp_scaled(ws, dyn_coef(L.w, L.alpha, L.Dv));
  case kNlpDynOwn: return nlp_scaled(ws, dyn_own(L.w, h, L.alpha, L.Dv, a.dFf[L.src], false));
  case kNlpDynOwnDiag: return nlp_scaled(ws, dyn_own(L.w, h, L.alpha, L.Dv, a.dFf[L.src], true));
  case kNlpDynDu: return nlp_scaled(ws, dyn_du(L.w, h, a.dFf[L.src]));
  case kNlpIntTf: {
    double acc = 0.0;
    for (int i = 0; i < T.N; ++i) {
      const int64_t fr = (int64_t)i * nq + L.src;
      integrate_dtf_add(acc, T.nodes[i].w, h, T.nodes[i].tau, a.Fg[fr], a.dFg[fr * nz]);
    }
    return nlp_scaled(ws, acc);
  }
  case kNlpIntQ: return nlp_minus_identity(ws);
  case kNlpIntDz: return nlp_scaled(ws, integrate_dz(L.w, h, a.dFg[L.src]));
  case kNlpCrTf: return nlp_scaled(ws, eval_dtf(L.w, L.tau, a.dFcr[(int64_t)L.src * nz]));
  case kNlpCrDz: return nlp_scaled(ws, eval_dz(L.w, a.dFcr[L.src]));
  default: return nlp_end(a.dce[L.src]);
  }
}

/// one agent on the host: g [m] and, with dg, the CSR values [nnz] (the loop the fused kernel spreads over lanes)
inline void ocp_nlp_assemble(const OcpNlpTables & T, const OcpNlpAgent & a, double * g, double * dg)
{
  for (int64_t it = 0; it < T.m; ++it) g[it] = ocp_nlp_value(T, ocp_nlp_decode(T, T.items[it]), a);
  if (dg)
    for (int64_t e = 0; e < T.nnz; ++e) dg[e] = ocp_nlp_value(T, ocp_nlp_decode(T, T.items[T.m + e]), a);
}

/// xl, xu [n]: free except tf >= 0; gl, gu [m]: zero for dyn and integrals, ws w_i crl / cru per node, cel / ceu.  NULL outputs are skipped.
inline void ocp_nlp_bounds(const OcpDims & d, int64_t N, const OcpNlpNode * nodes, double ws, const double * crl, const double * cru,
                           const double * cel, const double * ceu, double * xl, double * xu, double * gl, double * gu)
{
  int64_t vb[5], cb[5];
  ocp_nlp_structure(N, d, vb, cb);
  const double inf = std::numeric_limits<double>::infinity();
  for (int64_t k = 0; k < vb[4]; ++k) {
    if (xl) xl[k] = k == 0 ? 0.0 : -inf;
    if (xu) xu[k] = inf;
  }
  for (int side = 0; side < 2; ++side) {
    double * out = side ? gu : gl;
    const double *cr = side ? cru : crl, *ce = side ? ceu : cel;
    if (!out) continue;
    for (int64_t k = 0; k < cb[2]; ++k) out[k] = 0.0;
    for (int64_t i = 0; i < N; ++i)
      for (int r = 0; r < d.ncr; ++r) out[cb[2] + i * d.ncr + r] = (ws * nodes[i].w) * cr[r];
    for (int r = 0; r < d.nce; ++r) out[cb[3] + r] = ce[r];
  }
}

// ---- the Hessian of the Lagrangian of that NLP (OCPNLP::d2l_dx2; sfb_ocp_nlp_hess_* of the C-ABI) ----
//   H = sigma d2theta + ws (d2 dyn + d2 integrals + d2 running)(lambda) + sum_r lambda_ce[r] d2ce_r
// as values over the upper-triangle CSC pattern d2f_dx2 / d2g_dx2 have (rows ascending in a column, every reserved entry
// stored): the image of d2_pattern under the variable map without the t0 row and column, united with the
// (tf | q | x_0 | x_N)^2 block; the q-x0 and q-xf blocks sit at (q, x0) and (q, xf).
//
// Model-free and CONTRACTED: per node the caller brings HL [nz][nz], the Hessian in z = (t | x | u) of lambda_i . f, of
// lambda_q . g and of lambda_cr,i . cr (full square, row major, only r <= c read), and for the end d2theta [ne][ne] and
// d2ce_l = sum_r lambda_ce[r] d2ce_r, columns (tf | x0 | xf | q).  The uncontracted [N][nx][nz][nz] would be 9 GB for the
// MPC shape at 8 192 agents, and a caller with autodiff gets the Hessian of lambda . f directly.
//
// The node part restates detail::meshfn_d2_node on those contracted inputs: t0 is fixed, so of its lines only add(1, 1),
// add(1, col) and the blocks apply; s = w h for dyn and the integrals (time-scaled), s = w for the running constraints,
// and JL(c) = sum_j lambda_j dF(j, c) takes the place of lambda_j J(j, c).

// (tf, tf), (tf, z_c) and (z_r, z_c) of one model at one node
SFB_LIE_HD inline double d2_tftf(double w, double h, double tau, bool timescaled, double HL, double JL)
{
  const double s = timescaled ? w * h : w;
  double v       = (s * tau * tau) * HL;
  if (timescaled) v += (w * 2 * tau) * JL;
  return v;
}
SFB_LIE_HD inline double d2_tfz(double w, double h, double tau, bool timescaled, double HL, double JL)
{
  const double s = timescaled ? w * h : w;
  double v       = (s * tau) * HL;
  if (timescaled) v += w * JL;
  return v;
}
SFB_LIE_HD inline double d2_zz(double w, double h, bool timescaled, double HL) { return (timescaled ? w * h : w) * HL; }

/// JL(c) = sum_j lambda_j dF(j, c), added in j order; dF points at column c of the node's first row.  Four rows are loaded at
/// a time before their products are added, so a lane has four pairs of loads in flight; the order of the additions is j's.
SFB_LIE_HD inline double d2_JL(int nf, const double * lam, const double * dF, int64_t nz)
{
  double JL = 0.0;
  int j     = 0;
  for (; j + 4 <= nf; j += 4) {
    const double l0 = lam[j], l1 = lam[j + 1], l2 = lam[j + 2], l3 = lam[j + 3];
    const double d0 = dF[j * nz], d1 = dF[(j + 1) * nz], d2 = dF[(j + 2) * nz], d3 = dF[(j + 3) * nz];
    JL += l0 * d0;
    JL += l1 * d1;
    JL += l2 * d2;
    JL += l3 * d3;
  }
  for (; j < nf; ++j) JL += lam[j] * dF[j * nz];
  return JL;
}

/// One entry of the Hessian pattern, a gather: node >= 0 with the position (a, b), a <= b, in that node's z = (t | x_i | u_i)
/// block (kHessNoNode: no node part; kHessAllNodes: every node, the (tf, tf) entry), and end = ea ne + eb, the position in
/// the (tf | x0 | xf | q) block that is read (-1: no end part).
struct OcpNlpHessItem {
  int32_t node, a, b, end;
};
constexpr int32_t kHessNoNode = -1, kHessAllNodes = -2;

/// CSC pattern (colptr [n + 1], rowind [nnzH]) and, with `items`, one record per entry.  NULL arrays: only the count.
///   column tf {tf};  q_r {tf, q_0 .. q_r};  component j of x_0 {tf, q, x_00 .. x_0j};  of x_i {tf, x_i0 .. x_ij};
///   of x_N {tf, q, x_0, x_N0 .. x_Nj};  of u_i {tf, x_i, u_i0 .. u_ij}
inline int64_t ocp_nlp_hess_pattern(int nivals, const int32_t * K, const OcpDims & dm, int32_t * colptr, int32_t * rowind, OcpNlpHessItem * items)
{
  const int64_t nx = dm.nx, nu = dm.nu, nq = dm.nq, ne = 1 + 2 * nx + nq;
  int64_t N = 0;
  for (int s = 0; s < nivals; ++s) N += K[s];
  const int64_t tri_x = nx * (nx + 1) / 2;
  const int64_t nnz = 1 + nq + nq * (nq + 1) / 2 + nx * (1 + nq) + tri_x + (N - 1) * (nx + tri_x) + nx * (1 + nq + nx) + tri_x +
                      N * (nu * (1 + nx) + nu * (nu + 1) / 2);
  const bool pat = colptr && rowind;
  if (!pat && !items) return nnz;
  const int64_t qv = 1, xv = 1 + nq, uv = xv + nx * (N + 1), eq = 1 + 2 * nx;  // eq: q within the end block
  int64_t e = 0, col = 0;
  const auto put = [&](int64_t row, int64_t node, int64_t a, int64_t b, int64_t ea, int64_t eb) {
    if (pat) rowind[e] = (int32_t)row;
    if (items) items[e] = OcpNlpHessItem{(int32_t)node, (int32_t)a, (int32_t)b, ea < 0 ? -1 : (int32_t)(ea * ne + eb)};
    ++e;
  };
  const auto begin_col = [&]() {
    if (pat) colptr[col] = (int32_t)e;
    ++col;
  };
  begin_col();
  put(0, kHessAllNodes, 0, 0, 0, 0);
  for (int64_t r = 0; r < nq; ++r) {
    begin_col();
    put(0, kHessNoNode, 0, 0, 0, eq + r);
    for (int64_t s = 0; s <= r; ++s) put(qv + s, kHessNoNode, 0, 0, eq + s, eq + r);
  }
  for (int64_t i = 0; i <= N; ++i)
    for (int64_t j = 0; j < nx; ++j) {
      begin_col();
      if (i == 0) {
        put(0, 0, 0, 1 + j, 0, 1 + j);
        for (int64_t s = 0; s < nq; ++s) put(qv + s, kHessNoNode, 0, 0, eq + s, 1 + j);
        for (int64_t r = 0; r <= j; ++r) put(xv + r, 0, 1 + r, 1 + j, 1 + r, 1 + j);
      } else if (i < N) {
        put(0, i, 0, 1 + j, -1, 0);
        for (int64_t r = 0; r <= j; ++r) put(xv + i * nx + r, i, 1 + r, 1 + j, -1, 0);
      } else {
        put(0, kHessNoNode, 0, 0, 0, 1 + nx + j);
        for (int64_t s = 0; s < nq; ++s) put(qv + s, kHessNoNode, 0, 0, eq + s, 1 + nx + j);
        for (int64_t r = 0; r < nx; ++r) put(xv + r, kHessNoNode, 0, 0, 1 + r, 1 + nx + j);
        for (int64_t r = 0; r <= j; ++r) put(xv + N * nx + r, kHessNoNode, 0, 0, 1 + nx + r, 1 + nx + j);
      }
    }
  for (int64_t i = 0; i < N; ++i)
    for (int64_t j = 0; j < nu; ++j) {
      begin_col();
      put(0, i, 0, 1 + nx + j, -1, 0);
      for (int64_t r = 0; r < nx; ++r) put(xv + i * nx + r, i, 1 + r, 1 + nx + j, -1, 0);
      for (int64_t r = 0; r <= j; ++r) put(uv + i * nu + r, i, 1 + nx + r, 1 + nx + j, -1, 0);
    }
  if (pat) colptr[col] = (int32_t)e;
  return nnz;
}

/// what every agent of one (mesh, dims) shares
struct OcpNlpHessTables {
  OcpDims d;
  int32_t N;
  int64_t m, nnz;  // rows of lambda; entries of the pattern
  double ws;
  const OcpNlpNode * nodes;      // [N]
  const OcpNlpHessItem * items;  // [nnz]
};
/// one agent's arrays: x [n], lambda [m], sigma; dF [N][nf][nz] of f and g; HL [N][nz][nz] of f, g, cr; d2theta, d2ce_l [ne][ne].
/// A segment of length zero takes NULL arrays.
struct OcpNlpHessAgent {
  const double *x, *lambda;
  double sigma;
  const double *dFf, *HLf, *dFg, *HLg, *HLcr, *d2theta, *d2ce_l;
};
/// a record with everything that does not depend on the agent looked up: the nodes [i0, i1), the offset of (a, b) in a
/// node's HL, whether the entry is in the tf row, and the offset in the end blocks
struct OcpNlpHessLane {
  int32_t i0, i1, a, b, hl, end;
};

SFB_LIE_HD inline OcpNlpHessLane ocp_nlp_hess_decode(const OcpNlpHessTables & T, const OcpNlpHessItem it)
{
  const int32_t nz = 1 + T.d.nx + T.d.nu;
  const int32_t i0 = it.node >= 0 ? it.node : 0, i1 = it.node >= 0 ? it.node + 1 : it.node == kHessAllNodes ? T.N : 0;
  return OcpNlpHessLane{i0, i1, it.a, it.b, it.a * nz + it.b, it.end};
}

/// The value of one entry for one agent.  Fixed order of every sum: nodes ascending; within a node f, g, cr; the product
/// with ws; then theta, then ce.  t0 = 0, so h = tf.
SFB_LIE_HD inline double ocp_nlp_hess_value(const OcpNlpHessTables & T, const OcpNlpHessLane & L, const OcpNlpHessAgent & ag)
{
  const int nx = T.d.nx, nq = T.d.nq, ncr = T.d.ncr, nz = 1 + nx + T.d.nu;
  const int64_t nzz = (int64_t)nz * nz;
  const double h    = ag.x[0] - 0.0;
  const bool tfrow  = L.a == 0;  // (tf, tf) and (tf, z_c) carry the JL term of the time-scaled models
  double acc = 0.0;
  for (int i = L.i0; i < L.i1; ++i) {
    const OcpNlpNode nd = T.nodes[i];
    {
      const double HL = ag.HLf[i * nzz + L.hl];
      const double JL = tfrow ? d2_JL(nx, ag.lambda + (int64_t)i * nx, ag.dFf + (int64_t)i * nx * nz + L.b, nz) : 0.0;
      acc += !tfrow ? d2_zz(nd.w, h, true, HL) : L.b == 0 ? d2_tftf(nd.w, h, nd.tau, true, HL, JL) : d2_tfz(nd.w, h, nd.tau, true, HL, JL);
    }
    if (nq > 0) {
      const double HL = ag.HLg[i * nzz + L.hl];
      const double JL = tfrow ? d2_JL(nq, ag.lambda + (int64_t)T.N * nx, ag.dFg + (int64_t)i * nq * nz + L.b, nz) : 0.0;
      acc += !tfrow ? d2_zz(nd.w, h, true, HL) : L.b == 0 ? d2_tftf(nd.w, h, nd.tau, true, HL, JL) : d2_tfz(nd.w, h, nd.tau, true, HL, JL);
    }
    if (ncr > 0) {
      const double HL = ag.HLcr[i * nzz + L.hl];
      acc += !tfrow ? d2_zz(nd.w, h, false, HL) : L.b == 0 ? d2_tftf(nd.w, h, nd.tau, false, HL, 0.0) : d2_tfz(nd.w, h, nd.tau, false, HL, 0.0);
    }
  }
  double v = nlp_scaled(T.ws, acc);
  if (L.end >= 0) {
    v += nlp_end(ag.sigma * ag.d2theta[L.end]);
    if (T.d.nce > 0) v += nlp_end(ag.d2ce_l[L.end]);
  }
  return v;
}

/// one agent on the host: the values [nnz] of sigma d2f + d2g(lambda) (the loop the kernel spreads over lanes)
inline void ocp_nlp_hess_assemble(const OcpNlpHessTables & T, const OcpNlpHessAgent & agent, double sigma, double * hess_val)
{
  OcpNlpHessAgent a = agent;
  a.sigma           = sigma;
  for (int64_t e = 0; e < T.nnz; ++e) hess_val[e] = ocp_nlp_hess_value(T, ocp_nlp_hess_decode(T, T.items[e]), a);
}

}  // namespace meshfn

namespace detail {

inline double meshfn_fd_step() { return std::sqrt(std::numeric_limits<double>::epsilon()); }

/// The integrand's value, Jacobian J (nf x (1 + nx + nu), columns t | x | u) and Hessians H ((1 + nx + nu) x nf (1 + nx + nu),
/// side by side) at one node.  Analytic: f.jacobian(t, x, u, J), f.hessian(t, x, u, H).  Numerical: forward differences
/// with step sqrt(eps) on the group (x (+) h e_c); second derivatives by differences of differences at step eps^(1/4).
template<uint8_t Deriv, diff::Type DT, class Fn, class X, class U>
struct MeshModelEval {
  static constexpr int nx = X::Dof, nu = U::Dof, nv = 1 + nx + nu;
  using R                 = std::decay_t<std::invoke_result_t<Fn &, double, const X &, const U &>>;
  static constexpr int nf = (int)std::tuple_size_v<R>;
  using JMat              = Mat<nf, nv>;
  using HMat              = Mat<nv, nf * nv>;
  static constexpr bool has_jacobian = requires(Fn & f, const X & x, const U & u, JMat & J) { f.jacobian(0.0, x, u, J); };
  static constexpr bool has_hessian  = requires(Fn & f, const X & x, const U & u, HMat & H) { f.hessian(0.0, x, u, H); };
  static_assert(DT != diff::Type::Analytic || Deriv < 1 || has_jacobian, "diff::Type::Analytic: the integrand needs jacobian(t, x, u, J)");
  static_assert(DT != diff::Type::Analytic || Deriv < 2 || has_hessian, "diff::Type::Analytic: the integrand needs hessian(t, x, u, H)");

  R f{};
  std::conditional_t<(Deriv >= 1), JMat, char> J{};
  std::conditional_t<(Deriv >= 2), HMat, char> H{};

  static R shifted(Fn & fn, double t, const X & x, const U & u, int a, double da, int b, double db)
  {
    typename X::Tangent ex{};
    typename U::Tangent eu{};
    const auto bump = [&](int z, double d) {
      if (z == 0) t += d;
      else if (z <= nx) ex[z - 1] += d;
      else eu[z - 1 - nx] += d;
    };
    bump(a, da);
    if (b >= 0) bump(b, db);
    return fn(t, rplus(x, ex), rplus(u, eu));
  }

  void operator()(Fn & fn, double t, const X & x, const U & u)
  {
    f = fn(t, x, u);
    if constexpr (Deriv >= 1) {
      if constexpr (DT != diff::Type::Numerical && has_jacobian) {
        fn.jacobian(t, x, u, J);
      } else {
        const double h = meshfn_fd_step();
        for (int a = 0; a < nv; ++a) {
          const R fa = shifted(fn, t, x, u, a, h, -1, 0.0);
          for (int r = 0; r < nf; ++r) J(r, a) = (fa[r] - f[r]) / h;
        }
      }
    }
    if constexpr (Deriv >= 2) {
      if constexpr (DT != diff::Type::Numerical && has_hessian) {
        fn.hessian(t, x, u, H);
      } else {
        const double h = std::sqrt(meshfn_fd_step());
        for (int a = 0; a < nv; ++a)
          for (int b = a; b < nv; ++b) {
            const R pp = shifted(fn, t, x, u, a, h, b, h), pm = shifted(fn, t, x, u, a, h, b, -h);
            const R mp = shifted(fn, t, x, u, a, -h, b, h), mm = shifted(fn, t, x, u, a, -h, b, -h);
            for (int r = 0; r < nf; ++r) H(a, r * nv + b) = H(b, r * nv + a) = ((pp[r] - pm[r]) - (mp[r] - mm[r])) / (4 * h * h);
          }
      }
    }
  }
};

/// what node i adds to d2F (eval :208-242 with timescaled = false; integrate :368-415 and dyn :568-615 with true)
template<int nx, int nu, int nf>
void meshfn_d2_node(MeshCsc & H2, std::size_t N, std::size_t i, const double * lam, double w, double h, double tau, bool timescaled,
                    const Mat<nf, 1 + nx + nu> & J, const Mat<1 + nx + nu, nf *(1 + nx + nu)> & H)
{
  constexpr int nv  = 1 + nx + nu;
  const double mtau = 1. - tau;
  const int x_d = (int)(2 + i * nx), u_d = (int)(2 + (N + 1) * nx + i * nu), u_base = (int)(2 + (N + 1) * nx);
  const auto add = [&](int r, int c, double v) {
    const int pos = r < 2 ? r : r < u_base ? 2 + (r - x_d) : 2 + nx + (r - u_d);
    H2.val[(std::size_t)H2.colptr[c] + pos] += v;
  };
  for (int j = 0; j < nf; ++j) {
    const double wl = w * lam[j], s = timescaled ? wl * h : wl;
    const auto h2   = [&](int a, int b) { return H(a, j * nv + b); };
    add(0, 0, (s * mtau * mtau) * h2(0, 0));
    if (timescaled) add(0, 0, (-wl * 2 * mtau) * J(j, 0));
    add(0, 1, (s * mtau * tau) * h2(0, 0));
    if (timescaled) add(0, 1, (wl * (1. - 2 * tau)) * J(j, 0));
    add(1, 1, (s * tau * tau) * h2(0, 0));
    if (timescaled) add(1, 1, (wl * 2 * tau) * J(j, 0));
    for (int c = 0; c < nx + nu; ++c) {
      const int col = c < nx ? x_d + c : u_d + (c - nx);
      add(0, col, (s * mtau) * h2(0, 1 + c));
      if (timescaled) add(0, col, (-wl) * J(j, 1 + c));
      add(1, col, (s * tau) * h2(0, 1 + c));
      if (timescaled) add(1, col, wl * J(j, 1 + c));
    }
    for (int c = 0; c < nx; ++c)
      for (int r = 0; r <= c; ++r) add(x_d + r, x_d + c, s * h2(1 + r, 1 + c));
    for (int c = 0; c < nu; ++c) {
      for (int r = 0; r < nx; ++r) add(x_d + r, u_d + c, s * h2(1 + r, 1 + nx + c));
      for (int r = 0; r <= c; ++r) add(u_d + r, u_d + c, s * h2(1 + nx + r, 1 + nx + c));
    }
  }
}

template<class XS>
using meshfn_value_t = std::decay_t<decltype(*std::begin(std::declval<XS &>()))>;

template<class T>
struct is_rn : std::false_type {};
template<int N>
struct is_rn<Rn<N>> : std::true_type {};

}  // namespace detail

/// [f(t_i, x_i, u_i)]_i over the N collocation nodes, t_i = t0 + (tf - t0) tau_i, each scaled by its quadrature weight
/// when `scale` (:114-246).  Row (node i, output r) of dF holds t0, tf, the nx columns of x_i and the nu columns of u_i.
template<uint8_t Deriv, diff::Type DT = diff::Type::Default, class M, class Fn, class XS, class US>
  requires(Deriv <= 2)
void mesh_eval(MeshValue<Deriv> & out, const M & m, Fn & f, const double t0, const double tf, XS && xs, US && us, bool scale = false)
{
  using X = detail::meshfn_value_t<XS>;
  using U = detail::meshfn_value_t<US>;
  using E = detail::MeshModelEval<Deriv, DT, Fn, X, U>;
  constexpr int nx = E::nx, nu = E::nu, nf = E::nf;
  static_assert(Deriv < 2 || (detail::is_rn<X>::value && detail::is_rn<U>::value), "Deriv == 2 needs Rn state and input");
  const std::size_t N = m.N_colloc();
  if (!out.allocated) {
    out.F.assign(N * nf, 0.0);
    if constexpr (Deriv >= 1) {
      out.dF.rows = (int32_t)(N * nf);
      out.dF.cols = (int32_t)(2 + nx * (N + 1) + nu * N);
      const int64_t nnz = meshfn::eval_pattern((int64_t)N, nx, nu, nf, nullptr, nullptr);
      out.dF.rowptr.assign(N * nf + 1, 0);
      out.dF.colind.assign((std::size_t)nnz, 0);
      out.dF.val.assign((std::size_t)nnz, 0.0);
      meshfn::eval_pattern((int64_t)N, nx, nu, nf, out.dF.rowptr.data(), out.dF.colind.data());
    }
    if constexpr (Deriv >= 2) meshfn::d2_pattern((int64_t)N, nx, nu, out.d2F);
    out.allocated = true;
  }
  set_zero(out);
  const std::vector<double> taus = m.all_nodes(), wts = m.all_weights();
  auto xit = std::begin(xs);
  auto uit = std::begin(us);
  E ev;
  for (std::size_t i = 0; i < N; ++i, ++xit, ++uit) {
    const double tau = taus[i], w = scale ? wts[i] : 1.;
    ev(f, t0 + (tf - t0) * tau, *xit, *uit);
    for (int r = 0; r < nf; ++r) out.F[i * nf + r] = meshfn::eval_F(w, ev.f[r]);
    if constexpr (Deriv >= 1) {
      for (int r = 0; r < nf; ++r) {
        double * v = out.dF.val.data() + out.dF.rowptr[i * nf + r];
        v[0]       = meshfn::eval_dt0(w, tau, ev.J(r, 0));
        v[1]       = meshfn::eval_dtf(w, tau, ev.J(r, 0));
        for (int c = 0; c < nx + nu; ++c) v[2 + c] = meshfn::eval_dz(w, ev.J(r, 1 + c));
      }
    }
    if constexpr (Deriv >= 2) detail::meshfn_d2_node<nx, nu, nf>(out.d2F, N, i, out.lambda.data() + i * nf, w, 1.0, tau, false, ev.J, ev.H);
  }
}

/// (tf - t0) sum_i w_i f(t_i, x_i, u_i) (:273-419).  dF is a dense nf x numVars row block; its last-state columns are zero.
template<uint8_t Deriv, diff::Type DT = diff::Type::Default, class M, class Fn, class XS, class US>
  requires(Deriv <= 2)
void mesh_integrate(MeshValue<Deriv> & out, const M & m, Fn & f, const double t0, const double tf, XS && xs, US && us)
{
  using X = detail::meshfn_value_t<XS>;
  using U = detail::meshfn_value_t<US>;
  using E = detail::MeshModelEval<Deriv, DT, Fn, X, U>;
  constexpr int nx = E::nx, nu = E::nu, nf = E::nf;
  static_assert(Deriv < 2 || (detail::is_rn<X>::value && detail::is_rn<U>::value), "Deriv == 2 needs Rn state and input");
  const std::size_t N = m.N_colloc(), nv = 2 + nx * (N + 1) + nu * N;
  if (!out.allocated) {
    out.F.assign(nf, 0.0);
    if constexpr (Deriv >= 1) {
      out.dF.rows = nf;
      out.dF.cols = (int32_t)nv;
      out.dF.rowptr.resize(nf + 1);
      out.dF.colind.resize(nf * nv);
      out.dF.val.assign(nf * nv, 0.0);
      for (int r = 0; r <= nf; ++r) out.dF.rowptr[r] = (int32_t)(r * nv);
      for (std::size_t e = 0; e < nf * nv; ++e) out.dF.colind[e] = (int32_t)(e % nv);
    }
    if constexpr (Deriv >= 2) meshfn::d2_pattern((int64_t)N, nx, nu, out.d2F);
    out.allocated = true;
  }
  set_zero(out);
  const std::vector<double> taus = m.all_nodes(), wts = m.all_weights();
  const double h = tf - t0;
  auto xit = std::begin(xs);
  auto uit = std::begin(us);
  E ev;
  for (std::size_t i = 0; i < N; ++i, ++xit, ++uit) {
    const double tau = taus[i], w = wts[i];
    ev(f, t0 + (tf - t0) * tau, *xit, *uit);
    for (int r = 0; r < nf; ++r) meshfn::integrate_F_add(out.F[r], w, h, ev.f[r]);
    if constexpr (Deriv >= 1) {
      for (int r = 0; r < nf; ++r) {
        double * v = out.dF.val.data() + r * nv;
        meshfn::integrate_dt0_add(v[0], w, h, tau, ev.f[r], ev.J(r, 0));
        meshfn::integrate_dtf_add(v[1], w, h, tau, ev.f[r], ev.J(r, 0));
        for (int c = 0; c < nx; ++c) v[2 + i * nx + c] = meshfn::integrate_dz(w, h, ev.J(r, 1 + c));
        for (int c = 0; c < nu; ++c) v[2 + (N + 1) * nx + i * nu + c] = meshfn::integrate_dz(w, h, ev.J(r, 1 + nx + c));
      }
    }
    if constexpr (Deriv >= 2) detail::meshfn_d2_node<nx, nu, nf>(out.d2F, N, i, out.lambda.data(), w, h, tau, true, ev.J, ev.H);
  }
}

/// The collocation defects w_i ((tf - t0) f(t_i, x_i, u_i) - sum_k D(k, j) x_{M + k}), interval by interval (:450-665).
/// Row (node M_s + j of interval s, component d) of dF holds t0, tf, one entry per node k = 0 .. K_s of the interval
/// (component d of x_{M_s + k}; for k == j the whole nx-wide block) and the nu columns of u_i: 2 + K_s + nx + nu entries.
template<uint8_t Deriv, diff::Type DT = diff::Type::Default, class M, class Fn, class XS, class US>
  requires(Deriv <= 2)
void mesh_dyn(MeshValue<Deriv> & out, const M & m, Fn & f, const double t0, const double tf, XS && xs, US && us)
{
  using X = detail::meshfn_value_t<XS>;
  using U = detail::meshfn_value_t<US>;
  using E = detail::MeshModelEval<Deriv, DT, Fn, X, U>;
  constexpr int nx = E::nx, nu = E::nu, nf = E::nf;
  static_assert(nx == nf, "Output dimension must be same as state dimension");
  static_assert(detail::is_rn<X>::value, "mesh_dyn: the defect is linear in the node states and needs a vector state (Rn)");
  static_assert(Deriv < 2 || detail::is_rn<U>::value, "Deriv == 2 needs Rn state and input");
  const std::size_t N = m.N_colloc(), S = m.N_ivals();
  if (!out.allocated) {
    out.F.assign(N * nx, 0.0);
    if constexpr (Deriv >= 1) {
      std::vector<int32_t> K(S);
      for (std::size_t s = 0; s < S; ++s) K[s] = (int32_t)m.N_colloc_ival(s);
      const int64_t nnz = meshfn::dyn_pattern((int)S, K.data(), nx, nu, nullptr, nullptr);
      out.dF.rows       = (int32_t)(N * nx);
      out.dF.cols       = (int32_t)(2 + nx * (N + 1) + nu * N);
      out.dF.rowptr.assign(N * nx + 1, 0);
      out.dF.colind.assign((std::size_t)nnz, 0);
      out.dF.val.assign((std::size_t)nnz, 0.0);
      meshfn::dyn_pattern((int)S, K.data(), nx, nu, out.dF.rowptr.data(), out.dF.colind.data());
    }
    if constexpr (Deriv >= 2) meshfn::d2_pattern((int64_t)N, nx, nu, out.d2F);
    out.allocated = true;
  }
  set_zero(out);
  const std::vector<double> taus = m.all_nodes(), wts = m.all_weights();
  const double h = tf - t0;
  auto xit = std::begin(xs);
  auto uit = std::begin(us);
  E ev;
  std::size_t M0 = 0;
  for (std::size_t s = 0; s < S; ++s) {
    const int K             = (int)m.N_colloc_ival(s);
    const auto [alpha, Dus] = m.interval_diffmat_unscaled(s);
    // component d of the interval's K + 1 node states is read at xk[k * nx + d]
    double xk[(detail::kMeshMaxDegree + 1) * (nx > 0 ? nx : 1)];
    {
      auto xj = xit;
      for (int k = 0; k <= K; ++k, ++xj)
        for (int d = 0; d < nx; ++d) xk[k * nx + d] = (*xj).v[d];
    }
    for (int j = 0; j < K; ++j, ++xit, ++uit) {
      const std::size_t i = M0 + j;
      const double tau = taus[i], w = wts[i];
      const double * Dcol = Dus.a.data() + (std::size_t)j * (K + 1);
      ev(f, t0 + (tf - t0) * tau, *xit, *uit);
      for (int d = 0; d < nx; ++d) out.F[i * nx + d] = meshfn::dyn_F(K, w, h, alpha, Dcol, ev.f[d], xk + d, nx);
      if constexpr (Deriv >= 1) {
        for (int d = 0; d < nx; ++d) {
          double * v = out.dF.val.data() + out.dF.rowptr[i * nx + d];
          for (int p = 0; p < 2 + K + nx + nu; ++p) {
            int kind, idx;
            meshfn::dyn_decode(p, j, K, nx, kind, idx);
            v[p] = kind == 0   ? meshfn::dyn_dt0(w, h, tau, ev.f[d], ev.J(d, 0))
                   : kind == 1 ? meshfn::dyn_dtf(w, h, tau, ev.f[d], ev.J(d, 0))
                   : kind == 2 ? meshfn::dyn_coef(w, alpha, Dcol[idx])
                   : kind == 3 ? meshfn::dyn_own(w, h, alpha, Dcol[j], ev.J(d, 1 + idx), idx == d)
                               : meshfn::dyn_du(w, h, ev.J(d, 1 + nx + idx));
          }
        }
      }
      if constexpr (Deriv >= 2) detail::meshfn_d2_node<nx, nu, nf>(out.d2F, N, i, out.lambda.data() + i * nx, w, h, tau, true, ev.J, ev.H);
    }
    M0 += K;
  }
}

}  // namespace smooth_feedback_amd
