// Harness of the re-linearisation passes (mpc_relin.hpp): what examples/mpc_relin.cpp (host, libsfb_models.so),
// examples/mpc_relin_device.hip (libsfb_models_dev.so) and examples/mpc_relin_selftest.cpp share.
#pragma once
#include <cstdint>
#include <vector>

#include <smooth_feedback_amd/mpc.hpp>

#include "vehicle_model.h"

namespace sfbx {

/// make_vehicle_mpc with the two parameters the passes are tested with
template<class MPCT, class Model>
MPCT make_relin_mpc(int K, double tf, int passes, bool prune = true)
{
  MPCParams p;
  p.K = (size_t)K; p.tf = tf;
  p.relin_passes         = (size_t)passes;
  p.prune_explicit_zeros = prune;
  const Model mdl{};
  MPCT m(mdl.f, mdl.cr, {-0.5, -0.5}, {0.5, 0.5}, p);
  m.set_xdes([mdl](double t) { return mdl.xdes(t); }, [mdl](double t) { return mdl.dxdes(t); });
  m.set_udes([mdl](double t) { return mdl.udes(t); });
  return m;
}

/// the agents of the harness: state xdes(t[b]) (+) dx0[b]
template<class Model>
auto relin_states(const Model & mdl, int64_t B, const double * t, const double * dx0)
{
  using X = decltype(mdl.xdes(0.0));
  std::vector<X> xs((size_t)B);
  for (int64_t b = 0; b < B; ++b) {
    typename X::Tangent a{};
    for (int i = 0; i < X::Dof; ++i) a[i] = dx0[b * X::Dof + i];
    xs[(size_t)b] = rplus(mdl.xdes(t[b]), a);
  }
  return xs;
}

}  // namespace sfbx
