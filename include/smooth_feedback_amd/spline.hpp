// Lie-group splines: the counterpart of smooth::Spline<K, G> and smooth::fit_spline_cubic of pettni/smooth (absent here, so
// nothing below can be compared with it bit for bit: like lie.hpp the curve is DEFINED here and pinned to an independent
// 60-digit matrix-form reference, tests/golden/spline_reference.npz).  What PID::set_xdes(t0, spline) (pid.hpp:142-159 of
// the reference) tracks on the host, and what sfb_spline_eval_batch / sfb_pid_rollout_spline_batch (csrc/spline.hip) and
// SplineTrajectory (for PIDSwarmDevice) evaluate per GPU lane.
//
// The curve.  A spline of degree K on G has S segments and knot times tk[0] < ... < tk[S]; segment i carries a start
// element g_i and K control differences v_{i,1..K} in R^Dof.  With h_i = tk[i+1] - tk[i], u = (s - tk[i]) / h_i:
//   g(s) = g_i exp(B_1(u) v_{i,1}) ... exp(B_K(u) v_{i,K}),   B_j(u) = sum_{l=j..K} C(K,l) u^l (1-u)^(K-l)
// (cumulative Bernstein basis).  Body velocity and acceleration by the recursion over j = 1..K from vel = acc = 0
//   vel <- Ad_{exp(-B_j v_j)} vel + B_j' v_j
//   acc <- Ad_{exp(-B_j v_j)} acc + B_j' ad(vel) v_j + B_j'' v_j        (the new vel; derivatives in u)
// then vel /= h_i, acc /= h_i^2: dynamically consistent inside a segment (d^r g = vel, d vel / ds = acc).
// Outside the knots the pose is held: s < tk[0] gives (g_0, 0, 0), s > tk[S] gives (g_S, 0, 0) with g_S the stored end
// element (S + 1 elements are stored).  An interior knot s == tk[i] belongs to segment i (u = 0), s == tk[S] to the last
// segment (u = 1).  The segment search moves an index by comparisons only and is bounded by S whatever s is: a NaN time
// produces NaNs and reads nothing out of range.
//
// The evaluation is written ONCE, spline_eval on a non-owning SplineView<K, G> (plain pointers into the flat storage of
// PIDFlat<G>): Spline<K, G>::operator(), the kernels and SplineTrajectory call it.  fit_spline_cubic is likewise one
// function, spline_fit_cubic_flat, for the host and for sfb_spline_fit_cubic_batch.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "lie.hpp"
#include "pid.hpp"

// the loops over the K control differences index per-lane arrays: unrolled, they stay in registers on the GPU
#if defined(__clang__)
#define SFB_SPLINE_UNROLL _Pragma("unroll")
#else
#define SFB_SPLINE_UNROLL
#endif

namespace smooth_feedback_amd {

/// Non-owning view of a spline in flat storage: tk [S+1]; element i at g + i * gstride (PIDFlat<G>, S+1 of them);
/// control difference j (0-based) of segment i at V + (i * K + j) * vstride, G::Dof doubles.  The strides are those of
/// the whole bundle when G is one part of it (the kernels), PIDFlat<G>::E and G::Dof otherwise.
template<int K, class G>
struct SplineView {
  int64_t S        = 0;
  const double * tk = nullptr;
  const double * g  = nullptr;
  const double * V  = nullptr;
  int64_t gstride = PIDFlat<G>::E, vstride = G::Dof;
};

/// One segment in registers, and which: what a lane keeps between two evaluations (i < 0: nothing loaded)
template<int K, class G>
struct SplineSegment {
  int64_t i = -1;
  double t0 = 0, h = 1;
  G g{};
  typename G::Tangent v[K]{};
};

namespace detail {

/// C(n, l) u^l (1-u)^(n-l); 0 outside 0 <= l <= n
SFB_LIE_HD inline double bernstein(int n, int l, double u)
{
  if (l < 0 || l > n) return 0.0;
  double c = 1.0;
  for (int i = 0; i < l; ++i) c = c * (double)(n - i) / (double)(i + 1);
  for (int i = 0; i < l; ++i) c *= u;
  for (int i = 0; i < n - l; ++i) c *= (1.0 - u);
  return c;
}

/// cumulative basis B_j of degree K and its first two derivatives in u: B_j' = K b^{K-1}_{j-1},
/// B_j'' = K (K-1) (b^{K-2}_{j-2} - b^{K-2}_{j-1})
template<int K>
SFB_LIE_HD inline void spline_basis(int j, double u, double & B, double & dB, double & ddB)
{
  B = 0.0;
  for (int l = K; l >= j; --l) B += bernstein(K, l, u);
  dB  = (double)K * bernstein(K - 1, j - 1, u);
  ddB = (double)(K * (K - 1)) * (bernstein(K - 2, j - 2, u) - bernstein(K - 2, j - 1, u));
}

template<class G>
SFB_LIE_HD inline typename G::Tangent spline_load_tangent(const double * p)
{
  typename G::Tangent t{};
  for (int i = 0; i < G::Dof; ++i) t[i] = p[i];
  return t;
}

}  // namespace detail

/// the segment of time s, from a starting guess: largest i in [0, S-1] with tk[i] <= s (0 if none).  At most S moves.
SFB_LIE_HD inline int64_t spline_locate(int64_t S, const double * tk, double s, int64_t i)
{
  i = (i < 0) ? 0 : (i > S - 1 ? S - 1 : i);
  for (int64_t n = 0; n < S && i + 1 < S && tk[i + 1] <= s; ++n) ++i;
  for (int64_t n = 0; n < S && i > 0 && s < tk[i]; ++n) --i;
  return i;
}

/// segment i of the view into registers
template<int K, class G>
SFB_LIE_HD void spline_load_segment(const SplineView<K, G> & c, int64_t i, SplineSegment<K, G> & seg)
{
  seg.i  = i;
  seg.t0 = c.tk[i];
  seg.h  = c.tk[i + 1] - c.tk[i];
  seg.g  = PIDFlat<G>::load(c.g + i * c.gstride);
  SFB_SPLINE_UNROLL
  for (int j = 0; j < K; ++j) seg.v[j] = detail::spline_load_tangent<G>(c.V + (i * K + j) * c.vstride);
}

/// the loaded segment at the local parameter u: pose, body velocity, body acceleration (in time, not in u)
template<int K, class G>
SFB_LIE_HD void spline_eval_segment(const SplineSegment<K, G> & seg, double u, G & g, typename G::Tangent & vel, typename G::Tangent & acc)
{
  using Tangent = typename G::Tangent;
  g             = seg.g;
  vel           = Tangent{};
  acc           = Tangent{};
  SFB_SPLINE_UNROLL
  for (int j = 1; j <= K; ++j) {
    double B, dB, ddB;
    detail::spline_basis<K>(j, u, B, dB, ddB);
    const Tangent & vj = seg.v[j - 1];
    Tangent a{}, na{};
    for (int i = 0; i < G::Dof; ++i) {
      a[i]  = B * vj[i];
      na[i] = -a[i];
    }
    g              = rplus(g, a);
    const G hinv   = rplus(G::Identity(), na);  // exp(-B_j v_j)
    const Tangent w = hinv.Ad(vel), z = hinv.Ad(acc);
    for (int i = 0; i < G::Dof; ++i) vel[i] = w[i] + dB * vj[i];
    const Tangent c = G::ad(vel) * vj;
    for (int i = 0; i < G::Dof; ++i) acc[i] = z[i] + dB * c[i] + ddB * vj[i];
  }
  const double ih = 1.0 / seg.h;
  for (int i = 0; i < G::Dof; ++i) {
    vel[i] = vel[i] * ih;
    acc[i] = acc[i] * ih * ih;
  }
}

/// THE evaluation: the curve at time s.  seg is the caller's cache (start with SplineSegment{}); it is reloaded only when
/// the segment index moves, so a lane that walks monotone times touches each segment's data once.
template<int K, class G>
SFB_LIE_HD void spline_eval(const SplineView<K, G> & c, double s, SplineSegment<K, G> & seg, G & g, typename G::Tangent & vel,
                            typename G::Tangent & acc)
{
  if (s < c.tk[0] || s > c.tk[c.S]) {  // held pose, at rest
    g   = PIDFlat<G>::load(c.g + (s < c.tk[0] ? 0 : c.S) * c.gstride);
    vel = typename G::Tangent{};
    acc = typename G::Tangent{};
    return;
  }
  const int64_t i = spline_locate(c.S, c.tk, s, seg.i);
  if (i != seg.i) spline_load_segment<K, G>(c, i, seg);
  spline_eval_segment<K, G>(seg, (s - seg.t0) / seg.h, g, vel, acc);
}

/// Cubic fit through S + 1 knots, S >= 1, in closed form: interpolating and C^1 on every group.
///   D_i = g_{i+1} (-) g_i, d_i = D_i / h_i; the knot velocities sigma_0..sigma_S solve per tangent coordinate
///     2 sigma_0 + sigma_1 = 3 d_0
///     h_i sigma_{i-1} + 2 (h_{i-1} + h_i) sigma_i + h_{i-1} sigma_{i+1} = 3 (h_i d_{i-1} + h_{i-1} d_i)      0 < i < S
///     sigma_{S-1} + 2 sigma_S = 3 d_{S-1}
///   (the natural cubic's system; Thomas algorithm without pivoting: diagonally dominant), then
///     v_{i,1} = h_i sigma_i / 3,  v_{i,3} = h_i sigma_{i+1} / 3,  v_{i,2} = log(exp(-v_{i,1}) g_i^-1 g_{i+1} exp(-v_{i,3}))
/// so that the segment ends exactly on g_{i+1} with end velocities sigma_i, sigma_{i+1}.  On commutative groups this is the
/// classical C^2 natural cubic; elsewhere the acceleration jumps at the knots (commutator order).
/// Precondition: the argument of that log stays away from rotation angle pi; tk strictly increasing and finite.
/// Flat storage as SplineView (K = 3).  No workspace: the sweeps run in V -- sigma_i waits in slot (i, 0) (sigma_S in
/// (S-1, 2)), the eliminated super-diagonal, which depends on h only, in the first double of slot (i, 1).
template<class G>
SFB_LIE_HD void spline_fit_cubic_flat(int64_t S, const double * tk, const double * g, int64_t gstride, double * V, int64_t vstride)
{
  using Tangent  = typename G::Tangent;
  using Flat     = PIDFlat<G>;
  constexpr int N = G::Dof;
  const auto slot = [&](int64_t i, int j) { return V + (i * 3 + j) * vstride; };
  const auto put  = [](double * p, const Tangent & t) { for (int k = 0; k < N; ++k) p[k] = t[k]; };
  // forward sweep
  G g0 = Flat::load(g), g1 = Flat::load(g + gstride);
  double hp       = tk[1] - tk[0];
  Tangent dprev   = rminus(g1, g0);
  for (int k = 0; k < N; ++k) dprev[k] = dprev[k] / hp;
  double cp = 0.5;  // c'_0
  Tangent sp{};     // sigma'_0
  for (int k = 0; k < N; ++k) sp[k] = 3.0 * dprev[k] / 2.0;
  put(slot(0, 0), sp);
  slot(0, 1)[0] = cp;
  for (int64_t i = 1; i < S; ++i) {
    g0              = g1;
    g1              = Flat::load(g + (i + 1) * gstride);
    const double hi = tk[i + 1] - tk[i];
    Tangent d       = rminus(g1, g0);
    for (int k = 0; k < N; ++k) d[k] = d[k] / hi;
    const double den = 2.0 * (hp + hi) - hi * cp;
    for (int k = 0; k < N; ++k) sp[k] = (3.0 * (hi * dprev[k] + hp * d[k]) - hi * sp[k]) / den;
    cp = hp / den;
    put(slot(i, 0), sp);
    slot(i, 1)[0] = cp;
    dprev = d;
    hp    = hi;
  }
  Tangent sn{};  // sigma_S
  for (int k = 0; k < N; ++k) sn[k] = (3.0 * dprev[k] - sp[k]) / (2.0 - cp);
  put(slot(S - 1, 2), sn);
  // back substitution
  for (int64_t i = S - 1; i >= 0; --i) {
    const double ci = slot(i, 1)[0];
    Tangent si      = detail::spline_load_tangent<G>(slot(i, 0));
    for (int k = 0; k < N; ++k) si[k] = si[k] - ci * sn[k];
    put(slot(i, 0), si);
    sn = si;
  }
  // control differences, segment by segment (sigma_{i+1} is read before slot (i+1, 0) is overwritten)
  g1 = Flat::load(g);
  for (int64_t i = 0; i < S; ++i) {
    g0              = g1;
    g1              = Flat::load(g + (i + 1) * gstride);
    const double h3 = (tk[i + 1] - tk[i]) / 3.0;
    Tangent v1 = detail::spline_load_tangent<G>(slot(i, 0)), v3 = detail::spline_load_tangent<G>(i + 1 < S ? slot(i + 1, 0) : slot(i, 2));
    Tangent m3{};
    for (int k = 0; k < N; ++k) {
      v1[k] = h3 * v1[k];
      v3[k] = h3 * v3[k];
      m3[k] = -v3[k];
    }
    // log(exp(-v1) g_i^-1 g_{i+1} exp(-v3)) with g_i^-1 g_{i+1} = exp(D_i): the product is formed from the increments, whose
    // size is that of the knot spacing, not from the poses, whose translations can be much larger
    const Tangent D = rminus(g1, g0);
    Tangent m1{};
    for (int k = 0; k < N; ++k) m1[k] = -v1[k];
    const Tangent v2 = rminus(rplus(rplus(rplus(G::Identity(), m1), D), m3), G::Identity());
    put(slot(i, 0), v1);
    put(slot(i, 1), v2);
    put(slot(i, 2), v3);
  }
}

/// Owning host class: smooth::Spline<K, G>.  K from 1 to 5.
template<int K, class G>
  requires(K >= 1 && K <= 5)
class Spline {
public:
  using Tangent = typename G::Tangent;
  static constexpr int E = PIDFlat<G>::E, D = G::Dof;

  /// no default constructor: a spline has at least one segment, so every object can be evaluated
  /// knot times [S+1] strictly increasing, elements [S+1], control differences [S][K]
  Spline(const std::vector<double> & tk, const std::vector<G> & gk, const std::vector<std::array<Tangent, K>> & v) : tk_(tk)
  {
    const size_t S = v.size();
    if (S < 1 || tk.size() != S + 1 || gk.size() != S + 1) throw std::invalid_argument("Spline: S >= 1 segments need S + 1 knot times and elements");
    check_times(tk_);
    g_.resize((S + 1) * E);
    V_.resize(S * K * D);
    for (size_t i = 0; i <= S; ++i) PIDFlat<G>::store(gk[i], g_.data() + i * E);
    for (size_t i = 0; i < S; ++i)
      for (int j = 0; j < K; ++j)
        for (int k = 0; k < D; ++k) V_[(i * K + j) * D + k] = v[i][j][k];
  }
  /// from flat storage (the layout of SplineView and of the C-ABI)
  Spline(std::vector<double> tk, std::vector<double> g_flat, std::vector<double> v_flat) : tk_(std::move(tk)), g_(std::move(g_flat)), V_(std::move(v_flat))
  {
    const size_t S = tk_.size() < 2 ? 0 : tk_.size() - 1;
    if (S < 1 || g_.size() != (S + 1) * E || V_.size() != S * K * D) throw std::invalid_argument("Spline: flat storage does not match the knot count");
    check_times(tk_);
  }

  int64_t segments() const { return (int64_t)tk_.size() - 1; }
  double t_min() const { return tk_.front(); }
  double t_max() const { return tk_.back(); }
  SplineView<K, G> view() const { return SplineView<K, G>{segments(), tk_.data(), g_.data(), V_.data(), E, D}; }
  const std::vector<double> & knot_times() const { return tk_; }
  const std::vector<double> & elements_flat() const { return g_; }
  const std::vector<double> & control_flat() const { return V_; }

  G operator()(double s) const
  {
    Tangent vel, acc;
    return (*this)(s, vel, acc);
  }
  G operator()(double s, Tangent & vel, Tangent & acc) const
  {
    SplineSegment<K, G> seg;
    G g;
    spline_eval<K, G>(view(), s, seg, g, vel, acc);
    return g;
  }

private:
  static void check_times(const std::vector<double> & tk)
  {
    for (size_t i = 0; i < tk.size(); ++i)
      if (!(tk[i] - tk[i] == 0.0) || (i > 0 && !(tk[i] > tk[i - 1]))) throw std::invalid_argument("Spline: knot times must be finite and strictly increasing");
  }
  std::vector<double> tk_, g_, V_;
};

/// smooth::fit_spline_cubic: the cubic through gg[i] at tt[i] (see spline_fit_cubic_flat)
template<class G>
Spline<3, G> fit_spline_cubic(const std::vector<double> & tt, const std::vector<G> & gg)
{
  if (tt.size() < 2 || gg.size() != tt.size()) throw std::invalid_argument("fit_spline_cubic: at least two knots, one element per knot time");
  const size_t S = tt.size() - 1;
  for (size_t i = 0; i <= S; ++i)
    if (!(tt[i] - tt[i] == 0.0) || (i > 0 && !(tt[i] > tt[i - 1]))) throw std::invalid_argument("fit_spline_cubic: knot times must be finite and strictly increasing");
  constexpr int E = PIDFlat<G>::E, D = G::Dof;
  std::vector<double> g((S + 1) * E), V(S * 3 * D);
  for (size_t i = 0; i <= S; ++i) PIDFlat<G>::store(gg[i], g.data() + i * E);
  spline_fit_cubic_flat<G>((int64_t)S, tt.data(), g.data(), E, V.data(), D);
  return Spline<3, G>(tt, std::move(g), std::move(V));
}

/// Desired trajectory for PIDSwarmDevice (pid_device.hpp): agent b tracks its spline -- or the one shared spline, when
/// shared -- at t - ts0[b] (ts0 nullable: 0).  Device pointers; per agent tk [S+1], g [S+1][E], V [S][K][Dof].
template<int K, class G>
struct SplineTrajectory {
  int64_t S        = 0;
  const double * tk = nullptr;
  const double * g  = nullptr;
  const double * V  = nullptr;
  bool shared       = true;
  const double * ts0 = nullptr;
  SFB_LIE_HD SplineView<K, G> view(int64_t agent) const
  {
    constexpr int64_t E = PIDFlat<G>::E, D = G::Dof;
    const int64_t b     = shared ? 0 : agent;
    return SplineView<K, G>{S, tk + b * (S + 1), g + b * (S + 1) * E, V + b * S * K * D, E, D};
  }
  SFB_LIE_HD PIDDesired<G> operator()(int64_t agent, double t) const
  {
    SplineSegment<K, G> seg;
    PIDDesired<G> d;
    spline_eval<K, G>(view(agent), t - (ts0 ? ts0[agent] : 0.0), seg, d.g, d.v, d.a);
    return d;
  }
};

}  // namespace smooth_feedback_amd
