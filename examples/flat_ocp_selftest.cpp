// Stand-alone driver of flatten_ocp (include/smooth_feedback_amd/ocp_flatten.hpp) for sanitizer builds:
//   g++ -std=c++20 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include examples/flat_ocp_selftest.cpp
// The host front on both example problems (ocp_se2_model.h) around two trajectories each: the flat node arrays
// (flat_nodes_host), ocp_to_nlp(flatten_ocp(...)) with g, dg_dx, f, df_dx, and for the planar vehicle d2l_dx2; g and dg_dx
// must be bit-identical to meshfn::ocp_nlp_assemble over the node arrays, and everything finite.  Host only, header-only:
// links nothing of the library.
#include <cmath>
#include <cstdio>
#include <vector>

#include "flat_ocp_harness.h"

namespace {

namespace F = smooth::feedback;

template<class Ocp>
int drive(const char * name, bool hessian)
{
  using S = sfbx::FlatSizes<Ocp>;
  constexpr int B = 2, EX = S::stride - S::Nx - 2 * S::Nu;
  std::vector<double> traj((std::size_t)B * S::stride, 0.0);
  for (int b = 0; b < B; ++b) {
    double * row = traj.data() + (std::size_t)b * S::stride;
    if constexpr (EX == 6) row[2] = b ? 0.6 : 1.0, row[3] = b ? 0.8 : 0.0, row[0] = 0.4 * b;  // SE2: (x, y, cos, sin | R^2)
    else row[3] = b ? 0.8 : 1.0, row[5] = b ? 0.6 : 0.0, row[1] = -0.3 * b;                     // SE3: (p | w, x, y, z | R^6)
    for (int k = EX; k < S::stride; ++k) row[k] = 0.4 * std::sin(0.7 + 1.1 * k + 0.3 * b);
  }
  const auto model = sfbx::flat_swarm_model<Ocp>(traj.data());
  const auto mesh  = sfbx::flat_mesh(0);
  const std::size_t N = mesh.N_colloc(), n = (std::size_t)S::n((int64_t)N);
  std::vector<double> x((std::size_t)B * n);
  for (std::size_t k = 0; k < x.size(); ++k) x[k] = 0.3 * std::sin(1.0 + 0.37 * (double)k);
  x[0] = 1.7, x[n] = 0.9;
  for (std::size_t k = 0; k < (N + 1) * S::Nx; ++k) x[n + 1 + S::Nq + k] = k % 7 == 0 ? 1e-9 : 0.0;  // agent 1: e = 0 and tiny rotations
  for (int b = 0; b < B; ++b) {
    auto nlp = F::ocp_to_nlp(sfbx::flat_agent_ocp(model, b), mesh);
    if (nlp.n() != n) return std::printf("%s: n %zu, expected %zu\n", name, nlp.n(), n), 1;
    std::vector<double> g(nlp.m()), dg((std::size_t)nlp.tables().nnz), df(S::ne);
    double f        = 0.0;
    int64_t differs = -1;
    sfbx::flat_nlp_host(model, b, mesh, x.data() + (std::size_t)b * n, g.data(), dg.data(), &f, df.data(), &differs);
    if (differs != 0) return std::printf("%s agent %d: %lld doubles differ from the model-free loop\n", name, b, (long long)differs), 1;
    double sum = f;
    for (const double v : g) sum += v;
    for (const double v : dg) sum += v;
    for (const double v : df) sum += v;
    if (!std::isfinite(sum)) return std::printf("%s agent %d: not finite\n", name, b), 1;
    if (hessian) {
      std::vector<double> xv(x.begin() + (std::ptrdiff_t)(b * n), x.begin() + (std::ptrdiff_t)((b + 1) * n)), lam(nlp.m());
      for (std::size_t k = 0; k < lam.size(); ++k) lam[k] = std::cos(0.3 * (double)k);
      double hs = 0.0;
      for (const double v : nlp.d2l_dx2(xv, 0.5, lam).val) hs += v;
      if (!std::isfinite(hs)) return std::printf("%s agent %d: d2l not finite\n", name, b), 1;
    }
  }
  std::printf("%s: ok (n %zu, %zu nodes)\n", name, n, N);
  return 0;
}

}  // namespace

int main()
{
  int bad = 0;
  bad += drive<sfbx::OcpSE2>("planar vehicle on Bundle<SE2, Rn<2>>", true);
  bad += drive<sfbx::OcpSE3>("rigid body on Bundle<SE3, Rn<6>>", false);
  return bad ? 1 : 0;
}
