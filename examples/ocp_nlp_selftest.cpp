// Stand-alone driver of the collocation NLP front (include/smooth_feedback_amd/ocp_to_nlp.hpp) for sanitizer builds:
//   g++ -std=c++20 -fsanitize=address,undefined -fno-sanitize-recover=all -I include examples/ocp_nlp_selftest.cpp
// OCPNLP at every order, analytic and numerical, twice each, on three shapes -- one interval of one point with every
// segment but the dynamics empty, the reference test's problem on three intervals of three points, mixed degrees with
// unequal lengths -- and the two solution conversions there and back.  Header-only: links nothing of the library.
#include <cmath>
#include <cstdio>
#include <vector>

#include "ocp_nlp_harness.h"

namespace {

namespace F = smooth::feedback;

template<int NX, int NU, int NQ, int NCR, int NCE, class Mesh>
int drive(const char * name, const Mesh & mesh, const sfbx::OcpData & d)
{
  const std::size_t N = mesh.N_colloc(), n = 1 + NQ + NX * (N + 1) + NU * N, m = NX * N + NQ + NCR * N + NCE;
  std::vector<double> x(n), lambda(m);
  for (std::size_t i = 0; i < n; ++i) x[i] = 0.9 * std::sin(1.0 + 0.7 * (double)i);
  for (std::size_t i = 0; i < m; ++i) lambda[i] = std::cos(0.3 * (double)i);
  x[0] = 1.7;
  for (int numerical = 0; numerical < 2; ++numerical)
    for (int order = 0; order <= 2; ++order) {
      const std::size_t cap = m * (n + 1) + n * n;
      std::vector<double> f(1), df(n), g(m), dg(cap), d2f(cap), d2g(cap), xl(n), xu(n), gl(m), gu(m), ws(1), xb(n), lb(m);
      std::vector<int32_t> rowptr(m + 1), colind(cap), hcolptr(n + 1), hrowind(cap), sizes(5);
      const sfbx::OcpNlpOut o{f.data(), df.data(), g.data(), dg.data(), d2f.data(), d2g.data(), xl.data(), xu.data(), gl.data(), gu.data(), ws.data(),
                              xb.data(), lb.data(), rowptr.data(), colind.data(), hcolptr.data(), hrowind.data(), sizes.data()};
      const int rc = numerical ? sfbx::ocp_nlp_run<NX, NU, NQ, NCR, NCE, F::diff::Type::Numerical>(mesh, d, x.data(), lambda.data(), order, 2, o)
                               : sfbx::ocp_nlp_run<NX, NU, NQ, NCR, NCE, F::diff::Type::Analytic>(mesh, d, x.data(), lambda.data(), order, 2, o);
      if (rc != 0 || sizes[0] != (int32_t)n || sizes[1] != (int32_t)m || sizes[4] != 1) {
        std::printf("%s: order %d numerical %d: rc %d, sizes %d %d, stable %d\n", name, order, numerical, rc, sizes[0], sizes[1], sizes[4]);
        return 1;
      }
      double worst = 0;
      for (std::size_t i = 0; i < n; ++i) worst = std::fmax(worst, std::fabs(xb[i] - x[i]));
      for (std::size_t i = 0; i < m; ++i) worst = std::fmax(worst, std::fabs(lb[i] - lambda[i]));
      bool finite = std::isfinite(f[0]);
      for (const double v : g) finite = finite && std::isfinite(v);
      for (int e = 0; e < sizes[2]; ++e) finite = finite && std::isfinite(dg[(std::size_t)e]);
      for (int e = 0; e < sizes[3]; ++e) finite = finite && std::isfinite(d2f[(std::size_t)e]) && std::isfinite(d2g[(std::size_t)e]);
      if (!finite || !(worst <= 1e-9)) {
        std::printf("%s: order %d numerical %d: finite %d, there and back %.3e\n", name, order, numerical, (int)finite, worst);
        return 1;
      }
    }
  std::printf("%s: n %zu m %zu ok\n", name, n, m);
  return 0;
}

}  // namespace

int main()
{
  int bad = 0;
  {  // bare
    static const int32_t t[][7] = {{0, 1, 1, 0, 0, 0, 0}, {0, 0, 2, 0, 0, 0, 0}, {0, 1, 3, 0, 4, 0, 0}, {0, 0, 2, 0, 0, 0, 0}, {0, 1, 1, 2, 1, 0, 0}};
    static const double c[] = {-0.8, 0.5, 0.3, 1.0, 0.5};
    sfbx::OcpData d{};
    d.tab[0] = {3, t[0], c}, d.tab[3] = {2, t[3], c + 3};
    static const double none[1] = {0};
    d.crl = d.cru = d.cel = d.ceu = none;
    bad += drive<1, 0, 0, 0, 0>("bare", F::Mesh<1, 2>(), d);
  }
  {  // the reference test's problem
    static const int32_t t[][7] = {
      {0, 2, 1, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 0, 0}, {1, 1, 1, 3, 2, 0, 0}, {0, 0, 1, 0, 0, 0, 0}, {0, 0, 1, 1, 2, 0, 0}, {0, 0, 1, 2, 2, 0, 0},
      {0, 3, 2, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 0, 0}, {1, 0, 1, 1, 1, 3, 1}, {2, 0, 1, 2, 1, 3, 1}, {3, 3, 2, 0, 0, 0, 0}, {0, 0, 2, 0, 0, 0, 0},
      {0, 0, 1, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 2, 0, 0}, {0, 2, 2, 4, 2, 0, 0}, {0, 3, 2, 0, 0, 0, 0}, {0, 4, 2, 0, 0, 0, 0},
      {0, 5, 1, 1, 1, 0, 0}, {0, 0, 1, 0, 0, 0, 0}, {1, 1, 1, 3, 1, 0, 0}, {2, 2, 1, 4, 1, 0, 0}, {3, 3, 1, 0, 0, 0, 0}, {4, 4, 1, 5, 1, 0, 0},
      {5, 5, 2, 0, 0, 0, 0}};
    static const double c[25] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -4, 4, 1, 1, 1, 1, 0.7, 1, 1, 1, 1, 0.6, 1};
    static const double lo[6] = {-1, -1, -1, -1, -1, -1}, hi[6] = {1, 1, 1, 1, 1, 1};
    sfbx::OcpData d{};
    d.tab[0] = {3, t[0], c}, d.tab[1] = {4, t[3], c + 3}, d.tab[2] = {4, t[7], c + 7}, d.tab[3] = {8, t[11], c + 11}, d.tab[4] = {6, t[19], c + 19};
    d.crl = lo, d.cru = hi, d.cel = lo, d.ceu = hi;
    F::Mesh<3, 3> mesh;
    mesh.refine_ph(0, 4);
    mesh.refine_ph(0, 4);
    bad += drive<2, 1, 1, 4, 6>("ref", mesh, d);
  }
  {  // mixed degrees, unequal lengths
    static const int32_t t[][7] = {
      {0, 2, 1, 4, 1, 0, 0}, {1, 3, 3, 0, 1, 5, 1}, {2, 1, 2, 0, 0, 0, 0}, {2, 5, 4, 2, 1, 0, 0},    // f
      {0, 1, 2, 0, 1, 0, 0}, {1, 4, 2, 5, 1, 3, 1},                                                    // g
      {0, 1, 1, 4, 1, 0, 1},                                                                          // cr
      {0, 0, 2, 7, 1, 0, 0}, {0, 1, 1, 4, 1, 8, 1}, {0, 6, 3, 0, 0, 0, 0},                              // theta
      {0, 0, 1, 7, 1, 0, 0}, {1, 2, 1, 5, 1, 8, 1}, {2, 3, 2, 6, 4, 0, 0}};                             // ce
    static const double c[13] = {1.0, -0.5, 0.3, 0.8, 0.6, -0.4, 0.9, 1.0, 0.7, -0.2, 0.5, 0.4, -0.3};
    static const double lo[3] = {-2, -1, -1.5}, hi[3] = {1, 2, 1.5};
    sfbx::OcpData d{};
    d.tab[0] = {4, t[0], c}, d.tab[1] = {2, t[4], c + 4}, d.tab[2] = {1, t[6], c + 6}, d.tab[3] = {3, t[7], c + 7}, d.tab[4] = {3, t[10], c + 10};
    d.crl = lo, d.cru = hi, d.cel = lo, d.ceu = hi;
    F::Mesh<3, 6> mesh(2, 3);
    mesh.refine_ph(1, 7);
    mesh.set_N_colloc_ival(1, 5);
    bad += drive<3, 2, 2, 1, 3>("mixed", mesh, d);
  }
  return bad;
}
