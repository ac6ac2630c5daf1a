// Legendre-Gauss-Radau collocation meshes on [0,1] (host side).
//  * UniformMesh: n equal intervals of K points, exactly what MPC / ocp_to_qp need from
//    smooth::feedback::Mesh<Kmesh,Kmesh> (reference collocation/mesh.hpp:93-118 equal intervals, :208-297
//    nodes/weights, :343-365 unscaled differentiation matrix) and smooth::lgr_nodes (mesh.hpp:35-48, third party).
//  * Mesh<Kmin, Kmax>: the refinable ph mesh of the reference (collocation/mesh.hpp:60-484) on plain arrays.
//  A Mesh whose intervals all have the same degree converts to the UniformMesh of that shape, so caller code written
//  against the reference (`Mesh mesh(2, 5); ocp_to_qp(ocp, mesh, ...)`) feeds the MPC path unchanged.
#pragma once
#include <algorithm>
#include <array>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

namespace smooth_feedback_amd {

// LGR nodes on [-1,1) and weights for K points: roots of P_{K-1}(x) + P_K(x), node 0 = -1.
inline void lgr_nodes(int K, std::vector<double> &x, std::vector<double> &w)
{
  x.assign(K, 0.0);
  w.assign(K, 0.0);
  auto legendre = [](int n, double t, double &pn, double &pnm1) {  // P_n, P_{n-1}
    double p0 = 1.0, p1 = t;
    if (n == 0) { pn = 1.0; pnm1 = 0.0; return; }
    for (int k = 2; k <= n; ++k) {
      const double p2 = ((2.0 * k - 1.0) * t * p1 - (k - 1.0) * p0) / k;
      p0 = p1; p1 = p2;
    }
    pn = p1; pnm1 = p0;
  };
  x[0] = -1.0;
  for (int i = 1; i < K; ++i) {
    // Chebyshev-like initial guess, then Newton on g(t) = (P_{K-1}(t) + P_K(t)) / (1 + t)
    double t = -std::cos(2.0 * M_PI * i / (2.0 * K - 1.0));
    for (int it = 0; it < 100; ++it) {
      double pK, pKm1;
      legendre(K, t, pK, pKm1);
      const double g = pKm1 + pK;
      // derivatives: (1-t^2) P_n' = n (P_{n-1} - t P_n)
      double pKm2, dummy;
      legendre(K - 1, t, dummy, pKm2);
      const double dK   = K * (pKm1 - t * pK) / (1.0 - t * t);
      const double dKm1 = (K - 1) * (pKm2 - t * pKm1) / (1.0 - t * t);
      // deflate the known root at -1
      const double f = g / (1.0 + t), df = ((dK + dKm1) * (1.0 + t) - g) / ((1.0 + t) * (1.0 + t));
      const double step = f / df;
      t -= step;
      if (std::fabs(step) < 1e-16) break;
    }
    x[i] = t;
  }
  w[0] = 2.0 / (double(K) * K);
  for (int i = 1; i < K; ++i) {
    double pK, pKm1;
    legendre(K, x[i], pK, pKm1);
    w[i] = (1.0 - x[i]) / (double(K) * K * pKm1 * pKm1);
  }
}

template<std::size_t Kmin, std::size_t Kmax>
  requires(Kmin <= Kmax)
class Mesh;

// Mesh with `n` equal intervals of K LGR points each (Mesh<K,K>(n), mesh.hpp:93-104).
struct UniformMesh {
  int n_ivals = 1, K = 4;
  std::vector<double> tau, wts;  // LGR nodes/weights on [-1,1]; extra node +1 with weight 0 appended
  std::vector<double> Dus;       // (K+1) x K, column-major: Dus(j,i) = l_j'(tau_i)

  UniformMesh() : UniformMesh(1, 4) {}
  // a ph mesh of n equal intervals of one degree (throws std::invalid_argument for any other)
  template<std::size_t Kmin, std::size_t Kmax>
  UniformMesh(const Mesh<Kmin, Kmax> & m);
  UniformMesh(int n, int k) : n_ivals(n < 1 ? 1 : n), K(k)
  {
    lgr_nodes(K, tau, wts);
    tau.push_back(1.0);  // lgr_plus_one, mesh.hpp:35-48
    wts.push_back(0.0);
    Dus.assign((size_t)(K + 1) * K, 0.0);
    for (int i = 0; i < K; ++i)       // evaluation node
      for (int j = 0; j <= K; ++j) {  // basis function
        double v = 0.0;
        if (j == i) {
          for (int k2 = 0; k2 <= K; ++k2)
            if (k2 != i) v += 1.0 / (tau[i] - tau[k2]);
        } else {
          double num = 1.0, den = 1.0;
          for (int k2 = 0; k2 <= K; ++k2) {
            if (k2 != j) den *= (tau[j] - tau[k2]);
            if (k2 != j && k2 != i) num *= (tau[i] - tau[k2]);
          }
          v = num / den;
        }
        Dus[(size_t)j + (size_t)i * (K + 1)] = v;
      }
  }
  int N_ivals() const { return n_ivals; }
  int N_colloc() const { return n_ivals * K; }
  double interval_start(int s) const { return double(s) / double(n_ivals); }
  // node tau in [0,1] of global index i in 0..N (N = the extra end point)   mesh.hpp:208-262
  double node(int i) const
  {
    if (i >= N_colloc()) return 1.0;
    const int s = i / K, nu = i % K;
    const double tau0 = interval_start(s), tauf = (s + 1 < n_ivals) ? interval_start(s + 1) : 1.0;
    return tau0 + (tauf - tau0) / 2 * (tau[nu] + 1.0);
  }
  double weight(int i) const  // mesh.hpp:264-297
  {
    if (i >= N_colloc()) return 0.0;
    const int s = i / K, nu = i % K;
    const double tau0 = interval_start(s), tauf = (s + 1 < n_ivals) ? interval_start(s + 1) : 1.0;
    return (tauf - tau0) / 2 * wts[nu];
  }
  // D = alpha * Dus  (mesh.hpp:343-365)
  double alpha(int s) const
  {
    const double tau0 = interval_start(s), tauf = (s + 1 < n_ivals) ? interval_start(s + 1) : 1.0;
    return 2.0 / (tauf - tau0);
  }
  double D(int j, int i) const { return Dus[(size_t)j + (size_t)i * (K + 1)]; }
};


/// Dense matrix the ph mesh hands out (column-major, like Mat<R, C> of lie.hpp, with run-time extents).
struct MeshMat {
  int rows = 0, cols = 0;
  std::vector<double> a;
  MeshMat() = default;
  MeshMat(int r, int c) : rows(r), cols(c), a((std::size_t)r * c, 0.0) {}
  double & operator()(int r, int c) { return a[(std::size_t)r + (std::size_t)c * rows]; }
  double operator()(int r, int c) const { return a[(std::size_t)r + (std::size_t)c * rows]; }
};

namespace detail {

constexpr int kMeshMaxDegree = 16;  // tables are kept for K = 1 .. 16

/// W[j] = d^p/du^p of the j-th Lagrange basis polynomial through x[0..n) at u, p in {0, 1, 2}, by the product formula.
inline void lagrange_weights(const double * x, int n, double u, int p, double * W)
{
  for (int j = 0; j < n; ++j) {
    double den = 1.0;
    for (int k = 0; k < n; ++k)
      if (k != j) den *= (x[j] - x[k]);
    double num = 0.0;
    if (p == 0) {
      num = 1.0;
      for (int k = 0; k < n; ++k)
        if (k != j) num *= (u - x[k]);
    } else if (p == 1) {
      for (int m = 0; m < n; ++m) {
        if (m == j) continue;
        double t = 1.0;
        for (int k = 0; k < n; ++k)
          if (k != j && k != m) t *= (u - x[k]);
        num += t;
      }
    } else {
      for (int m = 0; m < n; ++m) {
        if (m == j) continue;
        for (int l = 0; l < n; ++l) {
          if (l == j || l == m) continue;
          double t = 1.0;
          for (int k = 0; k < n; ++k)
            if (k != j && k != m && k != l) t *= (u - x[k]);
          num += t;
        }
      }
    }
    W[j] = num / den;
  }
}

/// In-place inverse of the n x n column-major matrix A (Gauss-Jordan, partial pivoting).  false: singular.
inline bool invert_dense(std::vector<double> & A, int n)
{
  std::vector<double> B((std::size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) B[(std::size_t)i + (std::size_t)i * n] = 1.0;
  auto at = [n](std::vector<double> & M, int r, int c) -> double & { return M[(std::size_t)r + (std::size_t)c * n]; };
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r)
      if (std::fabs(at(A, r, c)) > std::fabs(at(A, piv, c))) piv = r;
    if (at(A, piv, c) == 0.0) return false;
    if (piv != c)
      for (int k = 0; k < n; ++k) {
        std::swap(at(A, piv, k), at(A, c, k));
        std::swap(at(B, piv, k), at(B, c, k));
      }
    const double d = at(A, c, c);
    for (int k = 0; k < n; ++k) {
      at(A, c, k) /= d;
      at(B, c, k) /= d;
    }
    for (int r = 0; r < n; ++r) {
      if (r == c) continue;
      const double f = at(A, r, c);
      if (f == 0.0) continue;
      for (int k = 0; k < n; ++k) {
        at(A, r, k) -= f * at(A, c, k);
        at(B, r, k) -= f * at(B, c, k);
      }
    }
  }
  A.swap(B);
  return true;
}

/// What one degree K needs, on the [-1, 1] scale: the K LGR nodes / weights with the extra node +1 (weight 0)
/// appended (lgr_plus_one, mesh.hpp:35-48), the (K+1) x K differentiation matrix Dus(j, i) = l_j'(tau_i)
/// (mesh.hpp:321-329) and the inverse of its rows 1..K (mesh.hpp:387-391 before the scaling).
struct LgrTable {
  std::vector<double> tau, w;
  MeshMat Dus, Ius;
};

inline LgrTable make_lgr_table(int K)
{
  LgrTable t;
  lgr_nodes(K, t.tau, t.w);
  t.tau.push_back(1.0);
  t.w.push_back(0.0);
  t.Dus = MeshMat(K + 1, K);
  std::vector<double> W(K + 1);
  for (int i = 0; i < K; ++i) {
    lagrange_weights(t.tau.data(), K + 1, t.tau[i], 1, W.data());
    for (int j = 0; j <= K; ++j) t.Dus(j, i) = W[j];
  }
  t.Ius = MeshMat(K, K);
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) t.Ius(j, i) = t.Dus(j + 1, i);
  invert_dense(t.Ius.a, K);
  return t;
}

inline const LgrTable & lgr_table(int K)
{
  static const std::array<LgrTable, kMeshMaxDegree + 1> tables = [] {
    std::array<LgrTable, kMeshMaxDegree + 1> t;
    for (int k = 1; k <= kMeshMaxDegree; ++k) t[k] = make_lgr_table(k);
    return t;
  }();
  if (K < 1 || K > kMeshMaxDegree) throw std::invalid_argument("Mesh: degree outside 1 .. 16");
  return tables[K];
}

/// Weights that carry node values of a degree-K interval to the nodes of the same interval at degree K + 1
/// (the K + 2 points lgr_plus_one<K + 1>): W(j, i) = l_i(tau^{K+1}_j) over the K + 1 points of lgr_plus_one<K>
/// (`closed`: the interval is closed by the next value, mesh.hpp:452-458) or over the K LGR points alone (:459-466).
inline MeshMat resample_weights(int K, bool closed)
{
  const LgrTable &src = lgr_table(K), &dst = lgr_table(K + 1);
  const int n = closed ? K + 1 : K;
  MeshMat W(K + 2, n);
  std::vector<double> row(n);
  for (int j = 0; j < K + 2; ++j) {
    lagrange_weights(src.tau.data(), n, dst.tau[j], 0, row.data());
    for (int i = 0; i < n; ++i) W(j, i) = row[i];
  }
  return W;
}

}  // namespace detail

/// Refinable LGR mesh of [0, 1]: interval i starts at tau0_i and has K_i collocation points, Kmin <= K_i <= Kmax + 1
/// (collocation/mesh.hpp:60-484).
template<std::size_t _Kmin = 5, std::size_t _Kmax = 10>
  requires(_Kmin <= _Kmax)
class Mesh
{
public:
  static constexpr std::size_t Kmin = _Kmin, Kmax = _Kmax;
  static_assert(_Kmin >= 1 && _Kmax + 1 <= (std::size_t)detail::kMeshMaxDegree, "LGR tables are kept for 1 .. 16 points");

  /// one interval [0, 1] of Kmin points (mesh.hpp:83)
  Mesh() : intervals_(1, Interval{Kmin, 0.}) {}

  /// n equal intervals of k points; n < 2 gives one interval (mesh.hpp:93-104)
  Mesh(const std::size_t n, const std::size_t k = Kmin)
  {
    assert(Kmin <= k && k <= Kmax + 1);
    if (n < 2) {
      intervals_.push_back(Interval{k, 0.});
    } else {
      const double dx = 1. / static_cast<double>(n);
      intervals_.reserve(n);
      for (std::size_t i = 0; i < n; ++i) intervals_.push_back(Interval{k, static_cast<double>(i) * dx});
    }
  }

  std::size_t N_ivals() const { return intervals_.size(); }
  std::size_t N_colloc() const
  {
    std::size_t n = 0;
    for (const auto & iv : intervals_) n += iv.K;
    return n;
  }
  std::size_t N_colloc_ival(std::size_t i) const
  {
    assert(i < intervals_.size());
    return intervals_[i].K;
  }
  /// start / end of interval i on [0, 1]
  double interval_start(std::size_t i) const { return intervals_[i].tau0; }
  double interval_end(std::size_t i) const { return i + 1 < intervals_.size() ? intervals_[i + 1].tau0 : 1.; }

  /// ph refinement (mesh.hpp:145-167): D > Kmax or K_i > Kmax splits the interval into max(2, ceil(D / Kmin))
  /// intervals of Kmin points; D < K_i does nothing; otherwise the degree becomes D.
  void refine_ph(std::size_t i, std::size_t D)
  {
    assert(i < intervals_.size());
    if (D > Kmax || intervals_[i].K > Kmax) {
      std::size_t n     = std::max<std::size_t>(2u, (D + Kmin - 1) / Kmin);
      const double tau0 = intervals_[i].tau0;
      const double tauf = interval_end(i);
      const double taum = (tauf - tau0) / static_cast<double>(n);
      // (the reference leaves the degree of the first piece as it was, :156-160)
      while (n-- > 1)
        intervals_.insert(intervals_.begin() + static_cast<std::ptrdiff_t>(i + 1), Interval{Kmin, tau0 + static_cast<double>(n) * taum});
    } else if (D < intervals_[i].K) {
      return;
    } else if (D <= Kmax) {
      intervals_[i].K = D;
    }
  }

  /// refine every interval whose relative error exceeds the target, last interval first (mesh.hpp:174-189)
  template<class Errs>
  void refine_errors(const Errs & errs, double target_err)
  {
    const std::size_t N = N_ivals();
    assert(N == (std::size_t)std::size(errs));
    for (std::size_t i = N; i-- > 0;) {
      const std::size_t Ki = N_colloc_ival(i);
      const double e       = errs[i];
      if (e > target_err) {
        const double steps = std::log(e / target_err) / std::log((double)Ki) + 1;
        // K_i = 1 (log K_i = 0) or an infinite error asks for more than any degree holds: split
        const std::size_t Ktarget = (std::isfinite(steps) && steps < 1e6) ? Ki + (std::size_t)std::lround(steps) : Kmax + 1 + Ki;
        refine_ph(i, Ktarget);
      }
    }
  }

  void set_N_colloc_ival(std::size_t i, std::size_t K)
  {
    assert(Kmin <= K && K <= Kmax + 1);
    intervals_[i].K = K;
  }

  /// the K_i + 1 nodes of interval i on [0, 1], the interval's end point included (mesh.hpp:208-230)
  std::vector<double> interval_nodes(std::size_t i) const
  {
    const auto & T    = detail::lgr_table((int)intervals_[i].K);
    const double tau0 = intervals_[i].tau0, al = (interval_end(i) - tau0) / 2;
    std::vector<double> r(T.tau.size());
    for (std::size_t j = 0; j < r.size(); ++j) r[j] = tau0 + al * (T.tau[j] + 1);
    return r;
  }
  /// the N_colloc() + 1 nodes of the mesh, the end point 1 included once (mesh.hpp:239-249)
  std::vector<double> all_nodes() const { return gather([this](std::size_t i) { return interval_nodes(i); }); }
  /// quadrature weights of interval i, with a zero for the end point (mesh.hpp:256-278)
  std::vector<double> interval_weights(std::size_t i) const
  {
    const auto & T  = detail::lgr_table((int)intervals_[i].K);
    const double al = (interval_end(i) - intervals_[i].tau0) / 2;
    std::vector<double> r(T.w.size());
    for (std::size_t j = 0; j < r.size(); ++j) r[j] = al * T.w[j];
    return r;
  }
  std::vector<double> all_weights() const { return gather([this](std::size_t i) { return interval_weights(i); }); }
  /// node / weight of global index i in 0 .. N_colloc() (N_colloc(): the end point 1, weight 0), as UniformMesh has them
  double node(std::size_t i) const
  {
    const auto [s, nu] = locate(i);
    return s == intervals_.size() ? 1.0 : interval_nodes(s)[nu];
  }
  double weight(std::size_t i) const
  {
    const auto [s, nu] = locate(i);
    return s == intervals_.size() ? 0.0 : interval_weights(s)[nu];
  }

  /// (K+1) x K matrix D with [y'(tau_0) .. y'(tau_{K-1})] = [y(tau_0) .. y(tau_K)] D on the [0, 1] scale (mesh.hpp:312-334)
  MeshMat interval_diffmat(std::size_t i) const
  {
    auto [alpha, D] = interval_diffmat_unscaled(i);
    for (double & v : D.a) v *= alpha;
    return D;
  }
  /// alpha and D_us with D = alpha D_us (mesh.hpp:343-365)
  std::pair<double, MeshMat> interval_diffmat_unscaled(std::size_t i) const
  {
    return {2. / (interval_end(i) - intervals_[i].tau0), detail::lgr_table((int)intervals_[i].K).Dus};
  }
  /// K x K matrix I with [y(tau_1) .. y(tau_K)] = y(tau_0) [1 .. 1] + [y'(tau_0) .. y'(tau_{K-1})] I (mesh.hpp:387-391)
  MeshMat interval_intmat(std::size_t i) const
  {
    MeshMat I      = detail::lgr_table((int)intervals_[i].K).Ius;
    const double s = (interval_end(i) - intervals_[i].tau0) / 2;
    for (double & v : I.a) v *= s;
    return I;
  }

  /// index of the interval that contains t; boundaries belong to the interval they start (mesh.hpp:396-404)
  std::size_t interval_find(double t) const
  {
    if (t < 0) return 0;
    if (t > 1) return intervals_.size() - 1;
    std::size_t lo = 0, hi = intervals_.size();  // last interval with tau0 <= t
    while (hi - lo > 1) {
      const std::size_t mid = lo + (hi - lo) / 2;
      if (intervals_[mid].tau0 <= t) lo = mid; else hi = mid;
    }
    return lo;
  }

  void increase_degrees()
  {
    for (auto & iv : intervals_) iv.K = std::min(iv.K + 1, Kmax + 1);
  }
  void decrease_degrees()
  {
    for (auto & iv : intervals_) iv.K = std::max(iv.K - 1, Kmin);
  }

  /// The p-th derivative (p in {0, 1, 2}, with respect to the interval's own [-1, 1] variable, as the reference's
  /// monomial_derivative) at t of the polynomials through the node values r: `dim` doubles per node, `stride` apart,
  /// N + 1 nodes when `extend`, else N; then the last interval uses its own K points only (mesh.hpp:433-471).
  void eval_flat(double t, const double * r, std::size_t stride, std::size_t dim, std::size_t p, bool extend, double * out) const
  {
    if (p > 2) throw std::invalid_argument("Mesh::eval: derivative order above 2");
    const std::size_t ival = interval_find(t);
    const int k            = (int)intervals_[ival].K;
    const double tau0 = intervals_[ival].tau0, tauf = interval_end(ival);
    const double u = 2 * (t - tau0) / (tauf - tau0) - 1;
    std::size_t N_before = 0;
    for (std::size_t i = 0; i < ival; ++i) N_before += intervals_[i].K;
    const int npts = (extend || ival + 1 < intervals_.size()) ? k + 1 : k;
    double W[detail::kMeshMaxDegree + 1];
    detail::lagrange_weights(detail::lgr_table(k).tau.data(), npts, u, (int)p, W);
    for (std::size_t d = 0; d < dim; ++d) out[d] = 0.0;
    for (int j = 0; j < npts; ++j)
      for (std::size_t d = 0; d < dim; ++d) out[d] += W[j] * r[(N_before + j) * stride + d];
  }
  template<std::size_t D>
  std::array<double, D> eval(double t, const std::vector<std::array<double, D>> & r, std::size_t p = 0, bool extend = true) const
  {
    std::array<double, D> ret{};
    eval_flat(t, r.empty() ? nullptr : r.front().data(), D, D, p, extend, ret.data());
    return ret;
  }

private:
  // (interval, index inside it) of global node i; (N_ivals(), 0) for the end point
  std::pair<std::size_t, std::size_t> locate(std::size_t i) const
  {
    for (std::size_t s = 0; s < intervals_.size(); ++s) {
      if (i < intervals_[s].K) return {s, i};
      i -= intervals_[s].K;
    }
    return {intervals_.size(), 0};
  }
  template<class F>
  std::vector<double> gather(F && per_interval) const
  {
    std::vector<double> r;
    for (std::size_t i = 0; i < intervals_.size(); ++i) {
      const std::vector<double> v = per_interval(i);
      r.insert(r.end(), v.begin(), v.begin() + (std::ptrdiff_t)(i + 1 < intervals_.size() ? v.size() - 1 : v.size()));
    }
    return r;
  }
  struct Interval {
    std::size_t K;
    double tau0;
  };
  std::vector<Interval> intervals_;
};

template<std::size_t Kmin, std::size_t Kmax>
UniformMesh::UniformMesh(const Mesh<Kmin, Kmax> & m) : UniformMesh((int)m.N_ivals(), (int)m.N_colloc_ival(0))
{
  for (std::size_t i = 0; i < m.N_ivals(); ++i)
    if ((int)m.N_colloc_ival(i) != K || std::fabs(m.interval_start(i) - interval_start((int)i)) > 1e-12)
      throw std::invalid_argument("UniformMesh: the ph mesh is not n equal intervals of one degree");
}

}  // namespace smooth_feedback_amd
