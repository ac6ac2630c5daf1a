// Minimal Lie-group layer for the host side of the MPC / EKF paths.
//
// The reference gets this from pettni/smooth (absent here): right-invariant conventions
//   rplus(g, a) = g * exp(a),  rminus(a, b) = log(b^-1 * a),  body velocities d^r x_t = f
// (reference README.md:17-18, mpc.hpp:498,505,518, ekf.hpp:137).  Only what the hot path's callers
// need is restated: R^n, SE(2), SO(3), SE(3) and Bundle<...> with exp/log, ad, the group adjoint Ad (as an action on a
// tangent: Ad_g a = vee(g hat(a) g^-1), what the splines of spline.hpp need) and dr_expinv (the inverse right
// Jacobian used by MPCCE::jacobian, mpc.hpp:293-301).  Semantics as summarised in SURVEY.md section
// 8 ("smooth semantics the host side must restate").  Every operation is pinned to 60-digit values computed from the
// matrix groups (tests/golden/lie_reference.npz; tests/test_lie_host.py on the host, tests/test_lie_gpu.py in device code;
// SE(3): tests/golden/lie_se3_reference.npz, tests/test_lie_se3_host.py, tests/test_lie_se3_gpu.py).
// dr_exp, the right Jacobian of exp (what ocp_flatten.hpp needs), is pinned by tests/golden/flatten_reference.npz
// (tests/test_flatten_host.py, tests/test_flatten_gpu.py).
#pragma once
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <tuple>
#include <utility>
#include <vector>

// Everything here is usable in HIP device code as well (a model written against these types can be linearised or
// integrated on the GPU, asif_device.hpp): the functions are __host__ __device__ when compiled by hipcc.
#if defined(__HIPCC__)
#define SFB_LIE_HD __host__ __device__
#else
#define SFB_LIE_HD
#endif

namespace smooth_feedback_amd {

// ---- tiny fixed-size column-major matrix ----
template<int R, int C>
struct Mat {
  std::array<double, (R * C > 0 ? R * C : 1)> a{};
  static constexpr int rows = R, cols = C;
  SFB_LIE_HD double &operator()(int r, int c) { return a[(size_t)r + (size_t)c * R]; }
  SFB_LIE_HD double operator()(int r, int c) const { return a[(size_t)r + (size_t)c * R]; }
  SFB_LIE_HD static Mat Zero() { return Mat{}; }
  SFB_LIE_HD static Mat Identity()
  {
    Mat m{};
    for (int i = 0; i < (R < C ? R : C); ++i) m(i, i) = 1.0;
    return m;
  }
};
template<int N>
using Vec = std::array<double, (N > 0 ? N : 1)>;

template<int R, int K, int C>
SFB_LIE_HD Mat<R, C> operator*(const Mat<R, K> &A, const Mat<K, C> &B)
{
  Mat<R, C> out{};
  for (int c = 0; c < C; ++c)
    for (int k = 0; k < K; ++k)
      for (int r = 0; r < R; ++r) out(r, c) += A(r, k) * B(k, c);
  return out;
}
template<int R, int C>
SFB_LIE_HD Mat<R, C> operator+(Mat<R, C> A, const Mat<R, C> &B)
{
  for (size_t i = 0; i < A.a.size(); ++i) A.a[i] += B.a[i];
  return A;
}
template<int R, int C>
SFB_LIE_HD Mat<R, C> operator*(double s, Mat<R, C> A)
{
  for (auto &v : A.a) v *= s;
  return A;
}
template<int R, int C>
SFB_LIE_HD Vec<R> operator*(const Mat<R, C> &A, const Vec<C> &x)
{
  Vec<R> y{};
  for (int c = 0; c < C; ++c)
    for (int r = 0; r < R; ++r) y[r] += A(r, c) * x[c];
  return y;
}

// ---- R^n as a (commutative) Lie group ----
template<int N>
struct Rn {
  static constexpr int Dof           = N;
  static constexpr bool IsCommutative = true;
  using Tangent                      = Vec<N>;
  Vec<N> v{};
  SFB_LIE_HD static Rn Identity() { return Rn{}; }
  SFB_LIE_HD friend Rn rplus(const Rn &g, const Tangent &a)
  {
    Rn r = g;
    for (int i = 0; i < N; ++i) r.v[i] += a[i];
    return r;
  }
  SFB_LIE_HD friend Tangent rminus(const Rn &a, const Rn &b)
  {
    Tangent t{};
    for (int i = 0; i < N; ++i) t[i] = a.v[i] - b.v[i];
    return t;
  }
  SFB_LIE_HD static Mat<N, N> ad(const Tangent &) { return Mat<N, N>::Zero(); }
  SFB_LIE_HD Tangent Ad(const Tangent &a) const { return a; }  // Ad_g a = vee(g hat(a) g^-1): commutative
  SFB_LIE_HD static Mat<N, N> dr_expinv(const Tangent &) { return Mat<N, N>::Identity(); }
  SFB_LIE_HD static Mat<N, N> dr_exp(const Tangent &) { return Mat<N, N>::Identity(); }
};

namespace detail {
// (1 - cos th) / th from sin and cos of th, th != 0.  For cos th > 0 the difference 1 - cos th cancels (to eps / th^2
// relative: 1e-6 at th = 1e-5); sin^2 / (1 + cos) is the same number without a difference.
SFB_LIE_HD inline double one_minus_cos_over(double th, double sn, double cs)
{
  return (cs > 0.0) ? (sn / th) * sn / (1.0 + cs) : (1.0 - cs) / th;
}
// k(th) = 1/th^2 - (1 + cos th) / (2 th sin th), the coefficient of ad^2 in dr_expinv (SE2 and SO3: ad^3 = -th^2 ad)
//       = sum_n |B_2n| th^(2n-2) / (2n)!  (Bernoulli numbers).
// The closed form subtracts two numbers of size 1/th^2 (absolute error eps / th^2: 1e-8 just above a switch at th^2 = 1e-8),
// so the series runs until its truncation, 1.3e-11 th^12, meets that error: th^2 < 0.16 (both 3e-16 there).  Towards pi
// (1 + cos) / sin divides two vanishing numbers; sin / (1 - cos) is the same cotangent of th / 2 without them.
SFB_LIE_HD inline double dr_expinv_coef(double th2)
{
  if (th2 < 0.16)
    return 1.0 / 12.0 + th2 * (1.0 / 720.0 + th2 * (1.0 / 30240.0 + th2 * (1.0 / 1209600.0 + th2 * (1.0 / 47900160.0 + th2 * (691.0 / 1307674368000.0)))));
  const double th = std::sqrt(th2), cs = std::cos(th), sn = std::sin(th);
  const double cot_half = (cs >= 0.0) ? (1.0 + cs) / sn : sn / (1.0 - cs);
  return 1.0 / th2 - cot_half / (2.0 * th);
}
}  // namespace detail

// ---- SE(2): tangent order (v_x, v_y, omega) ----
struct SE2 {
  static constexpr int Dof           = 3;
  static constexpr bool IsCommutative = false;
  using Tangent                      = Vec<3>;
  double x = 0, y = 0, c = 1, s = 0;  // translation, cos/sin of the heading

  SFB_LIE_HD static SE2 Identity() { return SE2{}; }
  SFB_LIE_HD static SE2 FromAngle(double th, double px, double py) { return SE2{px, py, std::cos(th), std::sin(th)}; }
  SFB_LIE_HD double angle() const { return std::atan2(s, c); }

  SFB_LIE_HD static SE2 exp(const Tangent &a)
  {
    const double th = a[2], th2 = th * th;
    double A, B;  // A = sin(th)/th, B = (1-cos(th))/th
    const double cs = std::cos(th), sn = std::sin(th);
    if (th2 < 1e-10) {
      A = 1.0 - th2 / 6.0;
      B = th / 2.0 - th * th2 / 24.0;
    } else {
      A = sn / th;
      B = detail::one_minus_cos_over(th, sn, cs);
    }
    return SE2{A * a[0] - B * a[1], B * a[0] + A * a[1], cs, sn};
  }
  SFB_LIE_HD Tangent log() const
  {
    const double th = angle(), th2 = th * th;
    double A, B;
    if (th2 < 1e-10) {
      A = 1.0 - th2 / 6.0;
      B = th / 2.0 - th * th2 / 24.0;
    } else {
      A = s / th;
      B = detail::one_minus_cos_over(th, s, c);
    }
    const double den = A * A + B * B;
    return {(A * x + B * y) / den, (-B * x + A * y) / den, th};
  }
  SFB_LIE_HD SE2 inverse() const { return SE2{-(c * x + s * y), -(-s * x + c * y), c, -s}; }
  SFB_LIE_HD friend SE2 operator*(const SE2 &g, const SE2 &h)
  {
    return SE2{g.x + g.c * h.x - g.s * h.y, g.y + g.s * h.x + g.c * h.y, g.c * h.c - g.s * h.s, g.s * h.c + g.c * h.s};
  }
  SFB_LIE_HD friend SE2 rplus(const SE2 &g, const Tangent &a) { return g * exp(a); }
  SFB_LIE_HD friend Tangent rminus(const SE2 &a, const SE2 &b) { return (b.inverse() * a).log(); }

  SFB_LIE_HD static Mat<3, 3> ad(const Tangent &a)
  {
    Mat<3, 3> m{};
    m(0, 1) = -a[2]; m(0, 2) = a[1];
    m(1, 0) = a[2];  m(1, 2) = -a[0];
    return m;
  }
  // Ad_g a = vee(g hat(a) g^-1) = (R v - omega J p, omega),  J = [[0, -1], [1, 0]]
  SFB_LIE_HD Tangent Ad(const Tangent &a) const { return {c * a[0] - s * a[1] + a[2] * y, s * a[0] + c * a[1] - a[2] * x, a[2]}; }
  // inverse of the right Jacobian of exp:  I + ad/2 + (1/th^2 - (1+cos th)/(2 th sin th)) ad^2
  SFB_LIE_HD static Mat<3, 3> dr_expinv(const Tangent &a)
  {
    const double k = detail::dr_expinv_coef(a[2] * a[2]);
    const Mat<3, 3> A = ad(a);
    return Mat<3, 3>::Identity() + 0.5 * A + k * (A * A);
  }
  // right Jacobian of exp, sum_n (-1)^n ad^n / (n + 1)! with ad^3 = -th^2 ad:  I - (1 - cos th)/th^2 ad + (th - sin th)/th^3 ad^2
  SFB_LIE_HD static Mat<3, 3> dr_exp(const Tangent &a);
};

// ---- SO(3): unit quaternion (w, x, y, z), tangent = body angular velocity ----
struct SO3 {
  static constexpr int Dof           = 3;
  static constexpr bool IsCommutative = false;
  using Tangent                      = Vec<3>;
  double w = 1, x = 0, y = 0, z = 0;

  SFB_LIE_HD static SO3 Identity() { return SO3{}; }
  SFB_LIE_HD static SO3 exp(const Tangent &a)
  {
    const double th2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    double A, B;  // A = sin(th/2)/th, B = cos(th/2)
    if (th2 < 1e-10) {
      A = 0.5 - th2 / 48.0;
      B = 1.0 - th2 / 8.0;
    } else {
      const double th = std::sqrt(th2);
      A = std::sin(0.5 * th) / th;
      B = std::cos(0.5 * th);
    }
    return SO3{B, A * a[0], A * a[1], A * a[2]};
  }
  SFB_LIE_HD Tangent log() const
  {
    const double s2 = x * x + y * y + z * z;
    double k;  // angle / sin(angle/2), with the shortest rotation (w >= 0 branch)
    const double ww = (w < 0) ? -w : w, sgn = (w < 0) ? -1.0 : 1.0;
    if (s2 < 1e-10) {
      k = 2.0 / ww - 2.0 / 3.0 * s2 / (ww * ww * ww);
    } else {
      const double sn = std::sqrt(s2);
      k               = 2.0 * std::atan2(sn, ww) / sn;
    }
    return {sgn * k * x, sgn * k * y, sgn * k * z};
  }
  SFB_LIE_HD SO3 inverse() const { return SO3{w, -x, -y, -z}; }
  SFB_LIE_HD friend SO3 operator*(const SO3 &a, const SO3 &b)
  {
    SO3 r{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
    const double nrm = std::sqrt(r.w * r.w + r.x * r.x + r.y * r.y + r.z * r.z);
    r.w /= nrm; r.x /= nrm; r.y /= nrm; r.z /= nrm;
    return r;
  }
  SFB_LIE_HD friend SO3 rplus(const SO3 &g, const Tangent &a) { return g * exp(a); }
  SFB_LIE_HD friend Tangent rminus(const SO3 &a, const SO3 &b) { return (b.inverse() * a).log(); }

  SFB_LIE_HD static Mat<3, 3> ad(const Tangent &a)  // = hat(a)
  {
    Mat<3, 3> m{};
    m(0, 1) = -a[2]; m(0, 2) = a[1];
    m(1, 0) = a[2];  m(1, 2) = -a[0];
    m(2, 0) = -a[1]; m(2, 1) = a[0];
    return m;
  }
  // Ad_q a = R(q) a = a + w t + u x t with t = 2 u x a, u the vector part
  SFB_LIE_HD Tangent Ad(const Tangent &a) const
  {
    const double t0 = 2.0 * (y * a[2] - z * a[1]), t1 = 2.0 * (z * a[0] - x * a[2]), t2 = 2.0 * (x * a[1] - y * a[0]);
    return {a[0] + w * t0 + (y * t2 - z * t1), a[1] + w * t1 + (z * t0 - x * t2), a[2] + w * t2 + (x * t1 - y * t0)};
  }
  SFB_LIE_HD static Mat<3, 3> dr_expinv(const Tangent &a)
  {
    const double k = detail::dr_expinv_coef(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const Mat<3, 3> A = ad(a);
    return Mat<3, 3>::Identity() + 0.5 * A + k * (A * A);
  }
  SFB_LIE_HD static Mat<3, 3> dr_exp(const Tangent &a);  // as SE2's, th = |a|
};

namespace detail {
// (th - sin th) / th^3, the coefficient of hat(w)^2 in the translation of SE3::exp
//       = 1/6 - th^2/120 + th^4/5040 - ...
// The closed form loses eps th / (th^3 / 6) = 6 eps / th^2 relative to the difference; the series through th^12 leaves
// 6 th^14 / 17! = 1.7e-14 th^14 relative: they meet at th^2 = 0.67 (1e-15 relative, on a term that weighs th^2 / 6 in the
// translation).  The switch sits a little below, where the series is the better of the two.
SFB_LIE_HD inline double th_minus_sin_over_th3(double th2)
{
  if (th2 < 0.5)
    return 1.0 / 6.0 - th2 * (1.0 / 120.0 - th2 * (1.0 / 5040.0 - th2 * (1.0 / 362880.0 - th2 * (1.0 / 39916800.0 - th2 * (1.0 / 6227020800.0 - th2 / 1307674368000.0)))));
  const double th = std::sqrt(th2);
  return (th - std::sin(th)) / (th2 * th);
}
// (1 - cos th) / th^2 = (sin(th/2) / (th/2))^2 / 2: the half angle has no difference to cancel, the series only bridges 0/0
// (th^2 < 1e-8: truncation th^4 / 1920 = 5e-20).
SFB_LIE_HD inline double one_minus_cos_over_th2(double th2)
{
  if (th2 < 1e-8) return 0.5 - th2 / 24.0;
  const double h = 0.5 * std::sqrt(th2), s = std::sin(h) / h;
  return 0.5 * s * s;
}
// k(th) of dr_expinv_coef for SE(3).  There k multiplies W V + V W, of size 2 th |v| in a block of size |v| / 2, where SE2
// and SO3 only have W^2 (size th^2): the closed form's absolute error of 3 eps / th^2 is 8e-16 of that block just above
// dr_expinv_coef's switch.  So the series runs further here: thirteen terms leave 9e-23 t^13 (t = th^2), which meets
// 3 eps / t at t = 2.3 (4e-18 against 1.4e-16); the switch sits at 2.25.
SFB_LIE_HD inline double dr_expinv_coef_wide(double t)
{
  if (t < 2.25)
    return 1.0 / 12.0 + t * (1.0 / 720.0 + t * (1.0 / 30240.0 + t * (1.0 / 1209600.0 + t * (1.0 / 47900160.0 + t * (691.0 / 1307674368000.0
         + t * (1.0 / 74724249600.0 + t * (3617.0 / 10670622842880000.0 + t * (8.586062056277845e-15 + t * (2.174868698558062e-16
         + t * (5.5090028283602295e-18 + t * (1.3954464685812522e-19 + t * 3.534707039629467e-21)))))))))));
  return dr_expinv_coef(t);
}
// k'(t) = d dr_expinv_coef / d(th^2), t = th^2: the coefficient that couples v and w in SE3::dr_expinv
//       = -1/t^2 + (1 + c^2) / (8 t) + c / (4 t th),  c = cot(th / 2)
//       = sum_n (n - 1) |B_2n| t^(n-2) / (2n)!.
// The closed form subtracts numbers of size 1/t^2 from each other (absolute error 3 eps / t^2); the series through t^11
// leaves 1.2e-21 t^12.  They meet at t = 2.1 (7e-18 against 8e-17: next to a value of 1.7e-3 that is 5e-14 relative, but the
// coefficient multiplies 2 (w.v) hat(w)^2, of size 2 t^1.5 |v|, in a block of size |v| / 2: 1e-15 of the block at most).
SFB_LIE_HD inline double dr_expinv_dcoef(double t)
{
  if (t < 2.0)
    return 1.0 / 720.0 + t * (1.0 / 15120.0 + t * (1.0 / 403200.0 + t * (1.0 / 11975040.0 + t * (691.0 / 261534873600.0 + t * (1.0 / 12454041600.0
         + t * (3617.0 / 1524374691840000.0 + t * (6.868849645022276e-14 + t * (1.9573818287022555e-15 + t * (5.5090028283602297e-17
         + t * (1.5349911154393775e-18 + t * 4.241648447555361e-20))))))))));
  const double th = std::sqrt(t), cs = std::cos(th), sn = std::sin(th);
  const double c = (cs >= 0.0) ? (1.0 + cs) / sn : sn / (1.0 - cs);  // cot(th / 2), as in dr_expinv_coef
  return -1.0 / (t * t) + (1.0 + c * c) / (8.0 * t) + c / (4.0 * t * th);
}
SFB_LIE_HD inline Vec<3> cross(const Vec<3> &a, const Vec<3> &b)
{
  return {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
}
// d/dt of B(t) = (1 - cos th) / th^2 (Odd = false) and of C(t) = (th - sin th) / th^3 (Odd = true), t = th^2: the coefficients
// that couple v and w in SE3::dr_exp.
//   B' = (sin th / th - 2 B) / (2 t) = sum_{n >= 1} (-1)^n n t^(n-1) / (2n + 2)!,
//   C' = (B - 3 C) / (2 t)           = sum_{n >= 1} (-1)^n n t^(n-1) / (2n + 3)!.
// The closed forms divide a difference that vanishes like t / 12 (t / 60) by t: absolute error 2 eps / t.  The series
// through n = 12 leaves 13 t^12 / 28! = 4e-29 t^12 (B') and has no cancellation to speak of up to t = 4 (first terms 0.042,
// 0.011 t); the switch sits there, where the closed form's error is 1e-16 on a value of 0.03.
template<bool Odd>
SFB_LIE_HD inline double dr_exp_dcoef(double t)
{
  if (t < 4.0) {
    double fact = Odd ? 120.0 : 24.0, tp = 1.0, acc = 0.0;  // (2n + 2)! or (2n + 3)! at n = 1
    for (int n = 1; n <= 12; ++n) {
      acc += ((n & 1) ? -double(n) : double(n)) * tp / fact;
      tp *= t;
      fact *= Odd ? double(2 * n + 4) * double(2 * n + 5) : double(2 * n + 3) * double(2 * n + 4);
    }
    return acc;
  }
  const double th = std::sqrt(t), B = one_minus_cos_over_th2(t);
  if constexpr (Odd) return (B - 3.0 * th_minus_sin_over_th3(t)) / (2.0 * t);
  else return (std::sin(th) / th - 2.0 * B) / (2.0 * t);
}
// I - B ad + C ad^2 for a group with ad^3 = -th^2 ad (SE2, SO3)
SFB_LIE_HD inline Mat<3, 3> dr_exp_rot(const Mat<3, 3> &A, double th2)
{
  return Mat<3, 3>::Identity() + (-one_minus_cos_over_th2(th2)) * A + th_minus_sin_over_th3(th2) * (A * A);
}
}  // namespace detail

SFB_LIE_HD inline Mat<3, 3> SE2::dr_exp(const Tangent &a) { return detail::dr_exp_rot(ad(a), a[2] * a[2]); }
SFB_LIE_HD inline Mat<3, 3> SO3::dr_exp(const Tangent &a) { return detail::dr_exp_rot(ad(a), a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// ---- SE(3): translation p and unit quaternion q (as SO3); tangent (v_0, v_1, v_2, w_0, w_1, w_2), body velocities ----
struct SE3 {
  static constexpr int Dof           = 6;
  static constexpr bool IsCommutative = false;
  using Tangent                      = Vec<6>;
  Vec<3> p{};
  SO3 q{};

  SFB_LIE_HD static SE3 Identity() { return SE3{}; }
  // R(q) a = a + w t + u x t with t = 2 u x a, u the vector part
  SFB_LIE_HD static Vec<3> rotate(const SO3 &q, const Vec<3> &a)
  {
    const Vec<3> u{q.x, q.y, q.z};
    Vec<3> t = detail::cross(u, a);
    for (auto &c : t) c *= 2.0;
    const Vec<3> ut = detail::cross(u, t);
    return {a[0] + q.w * t[0] + ut[0], a[1] + q.w * t[1] + ut[1], a[2] + q.w * t[2] + ut[2]};
  }

  // p = (I + B hat(w) + C hat(w)^2) v,  B = (1 - cos th) / th^2,  C = (th - sin th) / th^3
  SFB_LIE_HD static SE3 exp(const Tangent &a)
  {
    const Vec<3> v{a[0], a[1], a[2]}, w{a[3], a[4], a[5]};
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double B = detail::one_minus_cos_over_th2(th2), C = detail::th_minus_sin_over_th3(th2);
    const Vec<3> wv = detail::cross(w, v), wwv = detail::cross(w, wv);
    return SE3{{v[0] + B * wv[0] + C * wwv[0], v[1] + B * wv[1] + C * wwv[1], v[2] + B * wv[2] + C * wwv[2]}, SO3::exp(w)};
  }
  // v = (I - hat(w) / 2 + k hat(w)^2) p with the k of dr_expinv: the inverse of the matrix in exp
  SFB_LIE_HD Tangent log() const
  {
    const Vec<3> w = q.log();
    const double k = detail::dr_expinv_coef_wide(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const Vec<3> wp = detail::cross(w, p), wwp = detail::cross(w, wp);
    return {p[0] - 0.5 * wp[0] + k * wwp[0], p[1] - 0.5 * wp[1] + k * wwp[1], p[2] - 0.5 * wp[2] + k * wwp[2], w[0], w[1], w[2]};
  }
  SFB_LIE_HD SE3 inverse() const
  {
    const SO3 qi = q.inverse();
    const Vec<3> r = rotate(qi, p);
    return SE3{{-r[0], -r[1], -r[2]}, qi};
  }
  SFB_LIE_HD friend SE3 operator*(const SE3 &g, const SE3 &h)
  {
    const Vec<3> r = rotate(g.q, h.p);
    return SE3{{g.p[0] + r[0], g.p[1] + r[1], g.p[2] + r[2]}, g.q * h.q};
  }
  SFB_LIE_HD friend SE3 rplus(const SE3 &g, const Tangent &a) { return g * exp(a); }
  SFB_LIE_HD friend Tangent rminus(const SE3 &a, const SE3 &b) { return (b.inverse() * a).log(); }

  // [[hat(w), hat(v)], [0, hat(w)]]
  SFB_LIE_HD static Mat<6, 6> ad(const Tangent &a)
  {
    Mat<6, 6> m{};
    for (int b = 0; b < 2; ++b) {  // hat(w) on the diagonal blocks
      const int o = 3 * b;
      m(o + 0, o + 1) = -a[5]; m(o + 0, o + 2) = a[4];
      m(o + 1, o + 0) = a[5];  m(o + 1, o + 2) = -a[3];
      m(o + 2, o + 0) = -a[4]; m(o + 2, o + 1) = a[3];
    }
    m(0, 4) = -a[2]; m(0, 5) = a[1];
    m(1, 3) = a[2];  m(1, 5) = -a[0];
    m(2, 3) = -a[1]; m(2, 4) = a[0];
    return m;
  }
  // Ad_g (v, w) = vee(g hat(a) g^-1) = (R v + p x R w, R w)
  SFB_LIE_HD Tangent Ad(const Tangent &a) const
  {
    const Vec<3> rv = rotate(q, {a[0], a[1], a[2]}), rw = rotate(q, {a[3], a[4], a[5]}), pw = detail::cross(p, rw);
    return {rv[0] + pw[0], rv[1] + pw[1], rv[2] + pw[2], rw[0], rw[1], rw[2]};
  }
  // inverse of the right Jacobian of exp, sum_n B_n^+ ad^n / n!, in block form: ad is block upper triangular with equal
  // diagonal blocks, so a function of it is [[J, Q], [0, J]] with J = SO3::dr_expinv(w) = I + W/2 + k W^2 and Q the
  // derivative of J in the direction v:  Q = V/2 + k (W V + V W) + 2 (w.v) k'(th^2) W^2   (W = hat(w), V = hat(v))
  SFB_LIE_HD static Mat<6, 6> dr_expinv(const Tangent &a)
  {
    const Vec<3> v{a[0], a[1], a[2]}, w{a[3], a[4], a[5]};
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double k = detail::dr_expinv_coef_wide(th2), dk2 = 2.0 * (w[0] * v[0] + w[1] * v[1] + w[2] * v[2]) * detail::dr_expinv_dcoef(th2);
    const Mat<3, 3> W = SO3::ad(w), V = SO3::ad(v), W2 = W * W, WV = W * V;
    Mat<6, 6> m{};
    for (int c = 0; c < 3; ++c)
      for (int r = 0; r < 3; ++r) {
        const double J = (r == c ? 1.0 : 0.0) + 0.5 * W(r, c) + k * W2(r, c);
        m(r, c) = J;
        m(3 + r, 3 + c) = J;
        m(r, 3 + c) = 0.5 * V(r, c) + k * (WV(r, c) + WV(c, r)) + dk2 * W2(r, c);  // V W = (W V)' for two skew matrices
      }
    return m;
  }
  // right Jacobian of exp in the same block form [[J, Q], [0, J]]: J = SO3::dr_exp(w) = I - B W + C W^2 and Q its derivative
  // in the direction v:  Q = -B V + C (W V + V W) + 2 (w.v) (-B'(th^2) W + C'(th^2) W^2)
  SFB_LIE_HD static Mat<6, 6> dr_exp(const Tangent &a)
  {
    const Vec<3> v{a[0], a[1], a[2]}, w{a[3], a[4], a[5]};
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], wv2 = 2.0 * (w[0] * v[0] + w[1] * v[1] + w[2] * v[2]);
    const double B = detail::one_minus_cos_over_th2(th2), C = detail::th_minus_sin_over_th3(th2);
    const double dB = wv2 * detail::dr_exp_dcoef<false>(th2), dC = wv2 * detail::dr_exp_dcoef<true>(th2);
    const Mat<3, 3> W = SO3::ad(w), V = SO3::ad(v), W2 = W * W, WV = W * V;
    Mat<6, 6> m{};
    for (int c = 0; c < 3; ++c)
      for (int r = 0; r < 3; ++r) {
        const double J = (r == c ? 1.0 : 0.0) - B * W(r, c) + C * W2(r, c);
        m(r, c) = J;
        m(3 + r, 3 + c) = J;
        m(r, 3 + c) = -B * V(r, c) + C * (WV(r, c) + WV(c, r)) - dB * W(r, c) + dC * W2(r, c);
      }
    return m;
  }
};

// ---- Bundle<G...>: direct product, tangent = concatenation (first part first) ----
template<class... Gs>
struct Bundle {
  static constexpr int Dof           = (Gs::Dof + ...);
  static constexpr bool IsCommutative = (Gs::IsCommutative && ...);
  using Tangent                      = Vec<Dof>;
  std::tuple<Gs...> parts{};

  SFB_LIE_HD static Bundle Identity() { return Bundle{}; }
  template<size_t I>
  SFB_LIE_HD auto &part() { return std::get<I>(parts); }
  template<size_t I>
  SFB_LIE_HD const auto &part() const { return std::get<I>(parts); }

  template<class F>
  SFB_LIE_HD static void for_parts(F &&f)
  {
    for_parts_impl(std::forward<F>(f), std::index_sequence_for<Gs...>{});
  }
  template<class F, size_t... I>
  SFB_LIE_HD static void for_parts_impl(F &&f, std::index_sequence<I...>)
  {
    int off = 0;
    ((f(std::integral_constant<size_t, I>{}, off), off += std::tuple_element_t<I, std::tuple<Gs...>>::Dof), ...);
  }
  template<int N, int O>
  SFB_LIE_HD static Vec<N> seg(const Tangent &a, int off)
  {
    (void)O;
    Vec<N> r{};
    for (int i = 0; i < N; ++i) r[i] = a[off + i];
    return r;
  }

  SFB_LIE_HD friend Bundle rplus(const Bundle &g, const Tangent &a)
  {
    Bundle r = g;
    for_parts([&](auto I, int off) {
      using G = std::tuple_element_t<decltype(I)::value, std::tuple<Gs...>>;
      std::get<decltype(I)::value>(r.parts) = rplus(std::get<decltype(I)::value>(g.parts), seg<G::Dof, 0>(a, off));
    });
    return r;
  }
  SFB_LIE_HD friend Tangent rminus(const Bundle &a, const Bundle &b)
  {
    Tangent t{};
    for_parts([&](auto I, int off) {
      using G       = std::tuple_element_t<decltype(I)::value, std::tuple<Gs...>>;
      const auto ti = rminus(std::get<decltype(I)::value>(a.parts), std::get<decltype(I)::value>(b.parts));
      for (int i = 0; i < G::Dof; ++i) t[off + i] = ti[i];
    });
    return t;
  }
  SFB_LIE_HD Tangent Ad(const Tangent &a) const  // per part
  {
    Tangent t{};
    for_parts([&](auto I, int off) {
      using G       = std::tuple_element_t<decltype(I)::value, std::tuple<Gs...>>;
      const auto ti = std::get<decltype(I)::value>(parts).Ad(seg<G::Dof, 0>(a, off));
      for (int i = 0; i < G::Dof; ++i) t[off + i] = ti[i];
    });
    return t;
  }
  SFB_LIE_HD static Mat<Dof, Dof> ad(const Tangent &a) { return blockdiag(a, [](auto g, const auto &ai) { return decltype(g)::ad(ai); }); }
  SFB_LIE_HD static Mat<Dof, Dof> dr_expinv(const Tangent &a)
  {
    return blockdiag(a, [](auto g, const auto &ai) { return decltype(g)::dr_expinv(ai); });
  }
  SFB_LIE_HD static Mat<Dof, Dof> dr_exp(const Tangent &a) { return blockdiag(a, [](auto g, const auto &ai) { return decltype(g)::dr_exp(ai); }); }

private:
  template<class F>
  SFB_LIE_HD static Mat<Dof, Dof> blockdiag(const Tangent &a, F &&f)
  {
    Mat<Dof, Dof> m{};
    for_parts([&](auto I, int off) {
      using G      = std::tuple_element_t<decltype(I)::value, std::tuple<Gs...>>;
      const auto b = f(G{}, seg<G::Dof, 0>(a, off));
      for (int c = 0; c < G::Dof; ++c)
        for (int r = 0; r < G::Dof; ++r) m(off + r, off + c) = b(r, c);
    });
    return m;
  }
};

// ---- components of a group as (kind, dof) pairs, for ad() on the device (sfb_lie_kind in sfb.h) ----
template<class G>
struct LieParts;
template<int N>
struct LieParts<Rn<N>> {
  static void append(std::vector<int32_t> &kind, std::vector<int32_t> &dof) { kind.push_back(0); dof.push_back(N); }
};
template<>
struct LieParts<SE2> {
  static void append(std::vector<int32_t> &kind, std::vector<int32_t> &dof) { kind.push_back(1); dof.push_back(3); }
};
template<>
struct LieParts<SO3> {
  static void append(std::vector<int32_t> &kind, std::vector<int32_t> &dof) { kind.push_back(2); dof.push_back(3); }
};
template<>
struct LieParts<SE3> {
  static void append(std::vector<int32_t> &kind, std::vector<int32_t> &dof) { kind.push_back(3); dof.push_back(6); }
};
template<class... Gs>
struct LieParts<Bundle<Gs...>> {
  static void append(std::vector<int32_t> &kind, std::vector<int32_t> &dof) { (LieParts<Gs>::append(kind, dof), ...); }
};

}  // namespace smooth_feedback_amd
