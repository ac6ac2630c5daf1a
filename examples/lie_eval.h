// Batch evaluation of the operations of include/smooth_feedback_amd/lie.hpp on plain arrays, for the tests that pin them
// to a high-precision reference (tests/golden/lie_reference.npz): the same item function runs on the host
// (sfbx_lie_eval, models.cpp) and as one GPU thread per item (sfbx_lie_eval_device, models_device.hip).
//
// Elements as doubles: R3 (v0, v1, v2); SE2 (x, y, cos, sin); SO3 (w, x, y, z); SE3 (px, py, pz, w, x, y, z); a Bundle is its
// parts one after the other (X6 = 7 doubles, X12 = 14, X12B = Bundle<SE3, Rn<6>> = 13).  Tangents in the order of lie.hpp; matrices column-major.
#pragma once
#include <cstdint>
#include <utility>

#include <smooth_feedback_amd/lie.hpp>

namespace sfbx {
using namespace smooth_feedback_amd;

enum LieGroupId { LIE_R3 = 0, LIE_SE2 = 1, LIE_SO3 = 2, LIE_X6 = 3, LIE_X12 = 4, LIE_SE3 = 5, LIE_X12B = 6 };
// in -> out per item (E doubles per element, T per tangent):
enum LieOp {
  LIE_EXP          = 0,  // tangent -> element                         (SE2, SO3)
  LIE_LOG          = 1,  // element -> tangent                         (SE2, SO3)
  LIE_MUL          = 2,  // element g, element h -> g * h              (SE2, SO3)
  LIE_AD           = 3,  // tangent -> T x T
  LIE_DR_EXPINV    = 4,  // tangent -> T x T
  LIE_RPLUS        = 5,  // element g, tangent a -> rplus(g, a)
  LIE_RMINUS       = 6,  // element a, element b -> rminus(a, b)
  LIE_RMINUS_RPLUS = 7,  // element g, tangent b -> rminus(rplus(g, b), g)
};

template<class G>
struct LieIO;
template<int N>
struct LieIO<Rn<N>> {
  static constexpr int E = N;
  SFB_LIE_HD static Rn<N> load(const double * p)
  {
    Rn<N> g;
    for (int i = 0; i < N; ++i) g.v[i] = p[i];
    return g;
  }
  SFB_LIE_HD static void store(const Rn<N> & g, double * p)
  {
    for (int i = 0; i < N; ++i) p[i] = g.v[i];
  }
};
template<>
struct LieIO<SE2> {
  static constexpr int E = 4;
  SFB_LIE_HD static SE2 load(const double * p) { return SE2{p[0], p[1], p[2], p[3]}; }
  SFB_LIE_HD static void store(const SE2 & g, double * p) { p[0] = g.x; p[1] = g.y; p[2] = g.c; p[3] = g.s; }
};
template<>
struct LieIO<SO3> {
  static constexpr int E = 4;
  SFB_LIE_HD static SO3 load(const double * p) { return SO3{p[0], p[1], p[2], p[3]}; }
  SFB_LIE_HD static void store(const SO3 & g, double * p) { p[0] = g.w; p[1] = g.x; p[2] = g.y; p[3] = g.z; }
};
template<>
struct LieIO<SE3> {
  static constexpr int E = 7;
  SFB_LIE_HD static SE3 load(const double * p) { return SE3{{p[0], p[1], p[2]}, SO3{p[3], p[4], p[5], p[6]}}; }
  SFB_LIE_HD static void store(const SE3 & g, double * p)
  {
    p[0] = g.p[0]; p[1] = g.p[1]; p[2] = g.p[2]; p[3] = g.q.w; p[4] = g.q.x; p[5] = g.q.y; p[6] = g.q.z;
  }
};
template<class... Gs>
struct LieIO<Bundle<Gs...>> {
  static constexpr int E = (LieIO<Gs>::E + ...);
  SFB_LIE_HD static Bundle<Gs...> load(const double * p)
  {
    Bundle<Gs...> g;
    load_parts(g, p, std::index_sequence_for<Gs...>{});
    return g;
  }
  SFB_LIE_HD static void store(const Bundle<Gs...> & g, double * p) { store_parts(g, p, std::index_sequence_for<Gs...>{}); }

private:
  template<size_t... I>
  SFB_LIE_HD static void load_parts(Bundle<Gs...> & g, const double * p, std::index_sequence<I...>)
  {
    int off = 0;
    ((g.template part<I>() = LieIO<Gs>::load(p + off), off += LieIO<Gs>::E), ...);
  }
  template<size_t... I>
  SFB_LIE_HD static void store_parts(const Bundle<Gs...> & g, double * p, std::index_sequence<I...>)
  {
    int off = 0;
    ((LieIO<Gs>::store(g.template part<I>(), p + off), off += LieIO<Gs>::E), ...);
  }
};

template<class G>
inline constexpr bool lie_has_exp = requires(typename G::Tangent t, G g) { G::exp(t); g.log(); g * g; };

// doubles per item read / written by (G, op); false: G has no such operation
template<class G>
inline bool lie_eval_widths_of(int op, int * win, int * wout)
{
  constexpr int E = LieIO<G>::E, T = G::Dof;
  switch (op) {
  case LIE_EXP: *win = T; *wout = E; return lie_has_exp<G>;
  case LIE_LOG: *win = E; *wout = T; return lie_has_exp<G>;
  case LIE_MUL: *win = 2 * E; *wout = E; return lie_has_exp<G>;
  case LIE_AD:
  case LIE_DR_EXPINV: *win = T; *wout = T * T; return true;
  case LIE_RPLUS: *win = E + T; *wout = E; return true;
  case LIE_RMINUS: *win = 2 * E; *wout = T; return true;
  case LIE_RMINUS_RPLUS: *win = E + T; *wout = T; return true;
  default: return false;
  }
}

template<class G>
SFB_LIE_HD void lie_eval_item(int op, const double * in, double * out)
{
  using IO        = LieIO<G>;
  constexpr int E = IO::E, T = G::Dof;
  const auto tangent = [](const double * p) {
    typename G::Tangent t{};
    for (int i = 0; i < T; ++i) t[i] = p[i];
    return t;
  };
  const auto put_tangent = [](const typename G::Tangent & t, double * p) {
    for (int i = 0; i < T; ++i) p[i] = t[i];
  };
  const auto put_matrix = [](const Mat<T, T> & m, double * p) {
    for (int i = 0; i < T * T; ++i) p[i] = m.a[i];
  };
  switch (op) {
  case LIE_EXP:
    if constexpr (lie_has_exp<G>) IO::store(G::exp(tangent(in)), out);
    break;
  case LIE_LOG:
    if constexpr (lie_has_exp<G>) put_tangent(IO::load(in).log(), out);
    break;
  case LIE_MUL:
    if constexpr (lie_has_exp<G>) IO::store(IO::load(in) * IO::load(in + E), out);
    break;
  case LIE_AD: put_matrix(G::ad(tangent(in)), out); break;
  case LIE_DR_EXPINV: put_matrix(G::dr_expinv(tangent(in)), out); break;
  case LIE_RPLUS: IO::store(rplus(IO::load(in), tangent(in + E)), out); break;
  case LIE_RMINUS: put_tangent(rminus(IO::load(in), IO::load(in + E)), out); break;
  case LIE_RMINUS_RPLUS: {
    const G g = IO::load(in);
    put_tangent(rminus(rplus(g, tangent(in + E)), g), out);
    break;
  }
  default: break;
  }
}

// fn.template operator()<G>() for the group of the id; false for an unknown id
template<class Fn>
inline bool lie_dispatch_group(int group, Fn && fn)
{
  switch (group) {
  case LIE_R3: fn.template operator()<Rn<3>>(); return true;
  case LIE_SE2: fn.template operator()<SE2>(); return true;
  case LIE_SO3: fn.template operator()<SO3>(); return true;
  case LIE_X6: fn.template operator()<Bundle<SE2, Rn<3>>>(); return true;
  case LIE_X12: fn.template operator()<Bundle<SE2, Rn<3>, SE2, Rn<3>>>(); return true;
  case LIE_SE3: fn.template operator()<SE3>(); return true;
  case LIE_X12B: fn.template operator()<Bundle<SE3, Rn<6>>>(); return true;
  default: return false;
  }
}

inline bool lie_eval_widths(int group, int op, int * win, int * wout)
{
  bool ok = false;
  return lie_dispatch_group(group, [&]<class G>() { ok = lie_eval_widths_of<G>(op, win, wout); }) && ok;
}

}  // namespace sfbx
