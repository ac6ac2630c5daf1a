// Stand-alone driver of the opt-in second derivatives of flatten_ocp (include/smooth_feedback_amd/ocp_flatten.hpp,
// flatten_ocp<FlatHess::Differences>) for sanitizer builds:
//   g++ -std=c++20 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I examples examples/flat_ocp_hess_selftest.cpp
// Both example problems (ocp_se2_model.h) around two trajectories each, one agent with e = 0 and tiny rotations: d2l_dx2 of the
// opt-in flattened problem through the hessian members must be finite and bit-identical to meshfn::ocp_nlp_hess_assemble over the
// arrays of flat_hess_nodes_host, the contracted per-direction form of the same law; the squares must be symmetric bit for bit.  The default
// flat types must have no hessian member (static_assert).  Host only, header-only: links nothing of the library.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "flat_ocp_harness.h"

namespace {

namespace F = smooth::feedback;

template<class Ocp>
constexpr bool members_are_opt_in()
{
  using S = sfbx::FlatSizes<Ocp>;
  using E = F::Rn<S::Nx>;
  using V = F::Rn<S::Nu>;
  using Q = F::Vec<S::Nq>;
  using Plain = decltype(sfbx::flat_agent_ocp(std::declval<const sfbx::FlatSwarmModel<Ocp> &>(), 0));
  using OptIn = decltype(sfbx::flat_agent_ocp_hess(std::declval<const sfbx::FlatSwarmModel<Ocp> &>(), 0));
  using HF = F::Mat<S::nz, S::Nx * S::nz>;
  using HG = F::Mat<S::nz, S::Nq * S::nz>;
  using HC = F::Mat<S::nz, S::Ncr * S::nz>;
  using HT = F::Mat<S::ne, S::ne>;
  using HE = F::Mat<S::ne, S::Nce * S::ne>;
  constexpr bool plain = sfbx::flat_has_hessian<decltype(Plain::f), double, E, V, HF> || sfbx::flat_has_hessian<decltype(Plain::g), double, E, V, HG> ||
                         sfbx::flat_has_hessian<decltype(Plain::cr), double, E, V, HC> || sfbx::flat_has_hessian<decltype(Plain::theta), double, E, E, Q, HT> ||
                         sfbx::flat_has_hessian<decltype(Plain::ce), double, E, E, Q, HE>;
  constexpr bool optin = sfbx::flat_has_hessian<decltype(OptIn::f), double, E, V, HF> && sfbx::flat_has_hessian<decltype(OptIn::g), double, E, V, HG> &&
                         sfbx::flat_has_hessian<decltype(OptIn::cr), double, E, V, HC> && sfbx::flat_has_hessian<decltype(OptIn::theta), double, E, E, Q, HT> &&
                         sfbx::flat_has_hessian<decltype(OptIn::ce), double, E, E, Q, HE>;
  return !plain && optin;
}
static_assert(members_are_opt_in<sfbx::OcpSE2>(), "flatten_ocp: hessian members only with FlatHess::Differences");
static_assert(members_are_opt_in<sfbx::OcpSE3>(), "flatten_ocp: hessian members only with FlatHess::Differences");

template<class Ocp>
int drive(const char * name)
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
  int64_t cb[5];
  sfbx::flat_con_beg<Ocp>((int64_t)N, cb);
  const std::size_t m = (std::size_t)cb[4];
  std::vector<double> lam((std::size_t)B * m);
  for (std::size_t k = 0; k < lam.size(); ++k) lam[k] = std::cos(0.3 * (double)k);
  const std::vector<double> taus = mesh.all_nodes();
  const std::size_t sq = N * S::nz * S::nz, se = (std::size_t)S::ne * S::ne;
  std::vector<double> HLf(B * sq), HLg(B * sq), HLcr(B * sq), d2t(B * se), d2c(B * se);
  sfbx::flat_hess_nodes_host(model, B, (int32_t)N, taus.data(), x.data(), lam.data(), sfbx::FlatHessOut{HLf.data(), HLg.data(), HLcr.data(), d2t.data(), d2c.data()});
  const auto symmetric = [](const std::vector<double> & a, std::size_t squares, int nv) {
    for (std::size_t s = 0; s < squares; ++s)
      for (int r = 0; r < nv; ++r)
        for (int c = 0; c < nv; ++c) {
          const double p = a[(s * nv + r) * nv + c], q = a[(s * nv + c) * nv + r];
          if (!std::isfinite(p) || std::memcmp(&p, &q, sizeof p) != 0) return false;
        }
    return true;
  };
  if (!symmetric(HLf, B * N, S::nz) || !symmetric(HLg, B * N, S::nz) || !symmetric(HLcr, B * N, S::nz) || !symmetric(d2t, B, S::ne) || !symmetric(d2c, B, S::ne))
    return std::printf("%s: a square is not finite or not symmetric\n", name), 1;
  for (int b = 0; b < B; ++b) {
    auto nlp = F::ocp_to_nlp(sfbx::flat_agent_ocp_hess(model, b), mesh);
    if (nlp.n() != n || nlp.m() != m) return std::printf("%s: n %zu m %zu, expected %zu %zu\n", name, nlp.n(), nlp.m(), n, m), 1;
    std::vector<double> h((std::size_t)nlp.hess_tables().nnz);
    int64_t differs = -1;
    sfbx::flat_hess_nlp_host(model, b, mesh, x.data() + (std::size_t)b * n, lam.data() + (std::size_t)b * m, 0.5 + 0.25 * b, h.data(), &differs);
    if (differs != 0) return std::printf("%s agent %d: %lld values differ from the model-free loop\n", name, b, (long long)differs), 1;
    double sum = 0.0;
    for (const double v : h) sum += v;
    if (!std::isfinite(sum)) return std::printf("%s agent %d: d2l not finite\n", name, b), 1;
  }
  std::printf("%s: ok (n %zu, m %zu, %zu nodes)\n", name, n, m, N);
  return 0;
}

}  // namespace

int main()
{
  int bad = 0;
  bad += drive<sfbx::OcpSE2>("planar vehicle on Bundle<SE2, Rn<2>>");
  bad += drive<sfbx::OcpSE3>("rigid body on Bundle<SE3, Rn<6>>");
  return bad ? 1 : 0;
}
