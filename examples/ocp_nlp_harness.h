// Optimal control problems as data, for the harness entries of collocation.cpp and the stand-alone self-test
// (ocp_nlp_selftest.cpp): every function is a term table with three factors -- output r is the sum of
// coef phi_ka(z_a) phi_kb(z_b) phi_kc(z_c) over its rows (r, a, ka, b, kb, c, kc), phi_0 = 1, phi_1 = z, phi_2 = z^2,
// phi_3 = sin z, phi_4 = cos z -- with z = (t | x | u) for f, g, cr and z = (tf | x0 | xf | q) for theta, ce, and carries
// its derivatives in closed form (jacobian / hessian members in the forms ocp_to_nlp.hpp takes).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include <smooth/feedback/ocp_to_nlp.hpp>

namespace sfbx {

namespace sfn = smooth::feedback;

struct Phi3 {
  double v, d1, d2;
  Phi3(int k, double z)
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

struct TermTable {
  int nterms         = 0;
  const int32_t * terms = nullptr;  // [nterms][7]
  const double * coef   = nullptr;
  bool valid(int nf, int nv) const
  {
    for (int m = 0; m < nterms; ++m) {
      const int32_t * q = terms + 7 * m;
      if (q[0] < 0 || q[0] >= nf) return false;
      for (int p = 0; p < 3; ++p)
        if (q[1 + 2 * p] < 0 || q[1 + 2 * p] >= nv || q[2 + 2 * p] < 0 || q[2 + 2 * p] > 4) return false;
    }
    return true;
  }
  /// f [NF]; J (NF x NV) when wanted; H (NV x NF NV, side by side) when wanted
  template<int NF, int NV>
  void eval(const double * z, double * f, sfn::Mat<NF, NV> * J, sfn::Mat<NV, NF * NV> * H) const
  {
    for (int r = 0; r < NF; ++r) f[r] = 0.0;
    if (J) *J = sfn::Mat<NF, NV>::Zero();
    if (H) *H = sfn::Mat<NV, NF * NV>::Zero();
    for (int m = 0; m < nterms; ++m) {
      const int32_t * q = terms + 7 * m;
      const int r = q[0], idx[3] = {q[1], q[3], q[5]};
      const Phi3 P[3] = {Phi3(q[2], z[idx[0]]), Phi3(q[4], z[idx[1]]), Phi3(q[6], z[idx[2]])};
      const double co = coef[m];
      f[r] += co * P[0].v * P[1].v * P[2].v;
      for (int p = 0; p < 3; ++p) {
        const int a = (p + 1) % 3, b = (p + 2) % 3;
        if (J) (*J)(r, idx[p]) += co * P[p].d1 * P[a].v * P[b].v;
        if (H) {
          (*H)(idx[p], r * NV + idx[p]) += co * P[p].d2 * P[a].v * P[b].v;
          (*H)(idx[p], r * NV + idx[a]) += co * P[p].d1 * P[a].d1 * P[b].v;
          (*H)(idx[a], r * NV + idx[p]) += co * P[p].d1 * P[a].d1 * P[b].v;
        }
      }
    }
  }
};

/// f, g or cr: (t, x, u) -> Vec<NF>
template<int NX, int NU, int NF>
struct NodeFn {
  static constexpr int NV = 1 + NX + NU;
  TermTable tab;
  static void pack(double t, const sfn::Rn<NX> & x, const sfn::Rn<NU> & u, double * z)
  {
    z[0] = t;
    for (int d = 0; d < NX; ++d) z[1 + d] = x.v[d];
    for (int d = 0; d < NU; ++d) z[1 + NX + d] = u.v[d];
  }
  sfn::Vec<NF> operator()(double t, const sfn::Rn<NX> & x, const sfn::Rn<NU> & u) const
  {
    double z[NV];
    pack(t, x, u, z);
    sfn::Vec<NF> f{};
    tab.eval<NF, NV>(z, f.data(), nullptr, nullptr);
    return f;
  }
  void jacobian(double t, const sfn::Rn<NX> & x, const sfn::Rn<NU> & u, sfn::Mat<NF, NV> & J) const
  {
    double z[NV];
    pack(t, x, u, z);
    sfn::Vec<NF> f{};
    tab.eval<NF, NV>(z, f.data(), &J, nullptr);
  }
  void hessian(double t, const sfn::Rn<NX> & x, const sfn::Rn<NU> & u, sfn::Mat<NV, NF * NV> & H) const
  {
    double z[NV];
    pack(t, x, u, z);
    sfn::Vec<NF> f{};
    tab.eval<NF, NV>(z, f.data(), nullptr, &H);
  }
};

/// theta (Scalar) or ce: (tf, x0, xf, q) -> double or Vec<R>
template<int NX, int NQ, int R, bool Scalar>
struct EndFn {
  static constexpr int NV = 1 + 2 * NX + NQ;
  TermTable tab;
  static void pack(double tf, const sfn::Rn<NX> & x0, const sfn::Rn<NX> & xf, const sfn::Vec<NQ> & q, double * z)
  {
    z[0] = tf;
    for (int d = 0; d < NX; ++d) z[1 + d] = x0.v[d], z[1 + NX + d] = xf.v[d];
    for (int d = 0; d < NQ; ++d) z[1 + 2 * NX + d] = q[d];
  }
  auto operator()(double tf, const sfn::Rn<NX> & x0, const sfn::Rn<NX> & xf, const sfn::Vec<NQ> & q) const
  {
    double z[NV];
    pack(tf, x0, xf, q, z);
    sfn::Vec<R> f{};
    tab.eval<(R > 0 ? R : 1), NV>(z, f.data(), nullptr, nullptr);
    if constexpr (Scalar) return f[0];
    else return f;
  }
  void jacobian(double tf, const sfn::Rn<NX> & x0, const sfn::Rn<NX> & xf, const sfn::Vec<NQ> & q, sfn::Mat<R, NV> & J) const
  {
    double z[NV];
    pack(tf, x0, xf, q, z);
    sfn::Vec<R> f{};
    tab.eval<R, NV>(z, f.data(), &J, nullptr);
  }
  void hessian(double tf, const sfn::Rn<NX> & x0, const sfn::Rn<NX> & xf, const sfn::Vec<NQ> & q, sfn::Mat<NV, R * NV> & H) const
  {
    double z[NV];
    pack(tf, x0, xf, q, z);
    sfn::Vec<R> f{};
    tab.eval<R, NV>(z, f.data(), nullptr, &H);
  }
};

/// the members of OCP<...> of ocp_to_qp.hpp, with sizes that may be zero
template<int NX, int NU, int NQ, int NCR, int NCE>
struct TermOcp {
  using X = sfn::Rn<NX>;
  using U = sfn::Rn<NU>;
  static constexpr int Nx = NX, Nu = NU, Nq = NQ, Ncr = NCR, Nce = NCE;
  EndFn<NX, NQ, 1, true> theta;
  NodeFn<NX, NU, NX> f;
  NodeFn<NX, NU, NQ> g;
  NodeFn<NX, NU, NCR> cr;
  sfn::Vec<NCR> crl{}, cru{};
  EndFn<NX, NQ, NCE, false> ce;
  sfn::Vec<NCE> cel{}, ceu{};
};

/// the five tables (f, g, cr, theta, ce) and the bounds of a problem
struct OcpData {
  TermTable tab[5];
  const double *crl, *cru, *cel, *ceu;
};

struct OcpNlpOut {
  double *f, *df, *g, *dg, *d2f, *d2g, *xl, *xu, *gl, *gu, *ws, *x_back, *lambda_back;
  int32_t *rowptr, *colind, *hcolptr, *hrowind, *sizes;  // sizes: n, m, nnz, hnnz, 1 when no output array moved between the calls
};

/// OCPNLP of the data problem on `mesh` at x (and lambda): orders 0 .. order, each `calls` times; then the two
/// solution conversions, there and back.  NULL outputs are skipped.  Returns 0, or a negative code.
template<int NX, int NU, int NQ, int NCR, int NCE, sfn::diff::Type DT, class Mesh>
int ocp_nlp_run(const Mesh & mesh, const OcpData & d, const double * x, const double * lambda, int order, int calls, const OcpNlpOut & o)
{
  constexpr int nz = 1 + NX + NU, ne = 1 + 2 * NX + NQ;
  if (!d.tab[0].valid(NX, nz) || !d.tab[1].valid(NQ, nz) || !d.tab[2].valid(NCR, nz) || !d.tab[3].valid(1, ne) || !d.tab[4].valid(NCE, ne)) return -9;
  TermOcp<NX, NU, NQ, NCR, NCE> ocp{};
  ocp.f.tab = d.tab[0], ocp.g.tab = d.tab[1], ocp.cr.tab = d.tab[2], ocp.theta.tab = d.tab[3], ocp.ce.tab = d.tab[4];
  for (int r = 0; r < NCR; ++r) ocp.crl[r] = d.crl[r], ocp.cru[r] = d.cru[r];
  for (int r = 0; r < NCE; ++r) ocp.cel[r] = d.cel[r], ocp.ceu[r] = d.ceu[r];
  auto nlp = sfn::ocp_to_nlp<DT>(ocp, mesh);
  static_assert(sfn::HessianNLP<decltype(nlp)>);
  const std::size_t n = nlp.n(), m = nlp.m();
  const std::vector<double> xv(x, x + n), lv(lambda, lambda + m);
  const auto put = [](double * dst, const std::vector<double> & v) {
    if (dst) std::copy(v.begin(), v.end(), dst);
  };
  const auto puti = [](int32_t * dst, const std::vector<int32_t> & v) {
    if (dst) std::copy(v.begin(), v.end(), dst);
  };
  bool stable = true;
  const void * where[5] = {};
  for (int c = 0; c < calls; ++c) {
    const double fv = nlp.f(xv);
    if (o.f) *o.f = fv;
    const void * now[5] = {nlp.g(xv).data(), nullptr, nullptr, nullptr, nullptr};
    if (order >= 1) now[1] = nlp.df_dx(xv).val.data(), now[2] = nlp.dg_dx(xv).val.data();
    if (order >= 2) now[3] = nlp.d2f_dx2(xv).val.data(), now[4] = nlp.d2g_dx2(xv, lv).val.data();
    for (int k = 0; k < 5; ++k) {
      if (c > 0 && now[k] != where[k]) stable = false;
      where[k] = now[k];
    }
  }
  put(o.g, nlp.g(xv));
  put(o.xl, nlp.xl()), put(o.xu, nlp.xu()), put(o.gl, nlp.gl()), put(o.gu, nlp.gu());
  if (o.ws) *o.ws = nlp.w_scaling();
  int64_t nnz = 0, hnnz = 0;
  if (order >= 1) {
    const sfn::MeshCsr & df = nlp.df_dx(xv);
    if (o.df) {
      std::fill(o.df, o.df + n, 0.0);
      for (std::size_t k = 0; k < df.val.size(); ++k) o.df[df.colind[k]] = df.val[k];
    }
    const sfn::MeshCsr & dg = nlp.dg_dx(xv);
    nnz = (int64_t)dg.val.size();
    puti(o.rowptr, dg.rowptr), puti(o.colind, dg.colind), put(o.dg, dg.val);
  }
  if (order >= 2) {
    const sfn::MeshCsc & h = nlp.d2f_dx2(xv);
    hnnz = (int64_t)h.val.size();
    puti(o.hcolptr, h.colptr), puti(o.hrowind, h.rowind), put(o.d2f, h.val);
    put(o.d2g, nlp.d2g_dx2(xv, lv).val);
  }
  sfn::NLPSolution s;
  s.x = xv, s.lambda = lv;
  const auto osol = sfn::nlpsol_to_ocpsol(ocp, mesh, s);
  const sfn::NLPSolution back = sfn::ocpsol_to_nlpsol(ocp, mesh, osol);
  if (back.status != sfn::NLPSolution::Status::Unknown || back.zl.size() != n || back.zu.size() != n) return -7;
  for (const double v : back.zl)
    if (v != 0.0) return -7;
  put(o.x_back, back.x), put(o.lambda_back, back.lambda);
  if (o.sizes) o.sizes[0] = (int32_t)n, o.sizes[1] = (int32_t)m, o.sizes[2] = (int32_t)nnz, o.sizes[3] = (int32_t)hnnz, o.sizes[4] = stable ? 1 : 0;
  return 0;
}

/// d2l_dx2 of the data problem on `mesh` at (x, sigma, lambda), `calls` times: the pattern of the front's member, the
/// pattern of meshfn::ocp_nlp_hess_pattern from the mesh's interval sizes (hcolptr2 / hrowind2), and the values.
/// sizes: n, m, hnnz, 1 when the output array did not move between the calls.  Returns 0, or a negative code.
struct OcpNlpHessOut {
  int32_t *sizes, *hcolptr, *hrowind, *hcolptr2, *hrowind2;
  double * d2l;
};
template<int NX, int NU, int NQ, int NCR, int NCE, sfn::diff::Type DT, class Mesh>
int ocp_nlp_hess_run(const Mesh & mesh, const OcpData & d, const double * x, const double * lambda, double sigma, int calls, const OcpNlpHessOut & o)
{
  constexpr int nz = 1 + NX + NU, ne = 1 + 2 * NX + NQ;
  if (!d.tab[0].valid(NX, nz) || !d.tab[1].valid(NQ, nz) || !d.tab[2].valid(NCR, nz) || !d.tab[3].valid(1, ne) || !d.tab[4].valid(NCE, ne)) return -9;
  TermOcp<NX, NU, NQ, NCR, NCE> ocp{};
  ocp.f.tab = d.tab[0], ocp.g.tab = d.tab[1], ocp.cr.tab = d.tab[2], ocp.theta.tab = d.tab[3], ocp.ce.tab = d.tab[4];
  for (int r = 0; r < NCR; ++r) ocp.crl[r] = d.crl[r], ocp.cru[r] = d.cru[r];
  for (int r = 0; r < NCE; ++r) ocp.cel[r] = d.cel[r], ocp.ceu[r] = d.ceu[r];
  auto nlp = sfn::ocp_to_nlp<DT>(ocp, mesh);
  const std::size_t n = nlp.n(), m = nlp.m();
  const std::vector<double> xv(x, x + n), lv(lambda, lambda + m);
  bool stable        = true;
  const void * where = nullptr;
  for (int c = 0; c < calls; ++c) {
    const void * now = nlp.d2l_dx2(xv, sigma, lv).val.data();
    if (c > 0 && now != where) stable = false;
    where = now;
  }
  const sfn::MeshCsc & h = nlp.d2l_dx2(xv, sigma, lv);
  if (o.hcolptr) std::copy(h.colptr.begin(), h.colptr.end(), o.hcolptr);
  if (o.hrowind) std::copy(h.rowind.begin(), h.rowind.end(), o.hrowind);
  if (o.d2l) std::copy(h.val.begin(), h.val.end(), o.d2l);
  std::vector<int32_t> K(mesh.N_ivals());
  for (std::size_t s = 0; s < K.size(); ++s) K[s] = (int32_t)mesh.N_colloc_ival(s);
  const sfn::meshfn::OcpDims dm{NX, NU, NQ, NCR, NCE};
  const int64_t nnz = sfn::meshfn::ocp_nlp_hess_pattern((int)K.size(), K.data(), dm, nullptr, nullptr, nullptr);
  if (nnz != (int64_t)h.val.size() || nlp.hess_tables().nnz != nnz) return -8;
  if (o.hcolptr2 && o.hrowind2) sfn::meshfn::ocp_nlp_hess_pattern((int)K.size(), K.data(), dm, o.hcolptr2, o.hrowind2, nullptr);
  if (o.sizes) o.sizes[0] = (int32_t)n, o.sizes[1] = (int32_t)m, o.sizes[2] = (int32_t)nnz, o.sizes[3] = stable ? 1 : 0;
  return 0;
}

}  // namespace sfbx
