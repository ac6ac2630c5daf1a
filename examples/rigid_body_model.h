// A 3-D rigid body as functors usable on the host and in HIP device code, the SE(3) counterpart of vehicle_model.h:
// state X12B = SE3 x R^6 (pose, body twist (v, w)), input U6 = R^6 (body force and torque per unit inertia).
//   d^r pose = twist,   d twist / dt = u - D twist   with a fixed diagonal damping D
// With analytic right-Jacobians, as the vehicle.
#pragma once
#include <cmath>
#include <cstddef>

#include <smooth_feedback_amd/asif.hpp>
#include <smooth_feedback_amd/ekf.hpp>
#include <smooth_feedback_amd/lie.hpp>
#include <smooth_feedback_amd/mpc.hpp>

namespace sfbx {
using namespace smooth_feedback_amd;

using X12B = Bundle<SE3, Rn<6>>;
using U6   = Rn<6>;

// damping of the body twist, (v_0, v_1, v_2, w_0, w_1, w_2)
SFB_LIE_HD inline double rigid_body_damping(int i)
{
  switch (i) {
  case 0: return 0.2;
  case 1: return 0.3;
  case 2: return 0.25;
  case 3: return 0.4;
  case 4: return 0.35;
  default: return 0.5;
  }
}

struct RigidBodyDyn {
  SFB_LIE_HD Vec<12> operator()(const X12B & x, const U6 & u) const
  {
    const auto & w = x.part<1>().v;
    Vec<12> f{};
    for (int i = 0; i < 6; ++i) {
      f[i]     = w[i];
      f[6 + i] = u.v[i] - rigid_body_damping(i) * w[i];
    }
    return f;
  }
  SFB_LIE_HD void jacobian(const X12B &, const U6 &, Mat<12, 12> & dx, Mat<12, 6> & du) const
  {
    dx = Mat<12, 12>::Zero(); du = Mat<12, 6>::Zero();
    for (int i = 0; i < 6; ++i) {
      dx(i, 6 + i)     = 1.0;
      dx(6 + i, 6 + i) = -rigid_body_damping(i);
      du(6 + i, i)     = 1.0;
    }
  }
};

// running constraint: the input itself (bounded to [-0.5, 0.5]^6 by the MPC's crl / cru)
struct InputBox6 {
  SFB_LIE_HD Vec<6> operator()(const X12B &, const U6 & u) const { return u.v; }
  SFB_LIE_HD void jacobian(const X12B &, const U6 &, Mat<6, 12> & dx, Mat<6, 6> & du) const
  {
    dx = Mat<6, 12>::Zero();
    du = Mat<6, 6>::Identity();
  }
};

// desired trajectory: a screw motion with constant body twist from a tilted start pose, held by the input D twist
struct RigidBodyModel {
  RigidBodyDyn f;
  InputBox6 cr;
  SFB_LIE_HD static SE3::Tangent twist() { return {0.8, 0.0, 0.15, 0.1, -0.05, 0.4}; }
  SFB_LIE_HD X12B xdes(double t) const
  {
    const auto xi = twist();
    SE3::Tangent a{};
    for (int i = 0; i < 6; ++i) a[i] = t * xi[i];
    X12B x;
    x.part<0>()   = rplus(SE3::exp({2.5, 0.0, 1.0, 0.3, -0.2, 1.5707963267948966}), a);
    x.part<1>().v = xi;
    return x;
  }
  SFB_LIE_HD Vec<12> dxdes(double) const
  {
    const auto xi = twist();
    return {xi[0], xi[1], xi[2], xi[3], xi[4], xi[5], 0, 0, 0, 0, 0, 0};
  }
  SFB_LIE_HD U6 udes(double) const
  {
    const auto xi = twist();
    U6 u;
    for (int i = 0; i < 6; ++i) u.v[i] = rigid_body_damping(i) * xi[i];
    return u;
  }
};

// safety filter on the rigid body: stay above the plane z = 0.2; backup controller: damp the twist
struct RigidBodyH {
  SFB_LIE_HD Vec<1> operator()(double, const X12B & x) const { return {x.part<0>().p[2] - 0.2}; }
  SFB_LIE_HD Vec<1> operator()(std::size_t, double t, const X12B & x) const { return (*this)(t, x); }  // swarm callbacks
};
struct RigidBodyBU {
  SFB_LIE_HD U6 operator()(double, const X12B & x) const
  {
    U6 u;
    for (int i = 0; i < 6; ++i) u.v[i] = -0.3 * x.part<1>().v[i];
    return u;
  }
  SFB_LIE_HD U6 operator()(std::size_t, double t, const X12B & x) const { return (*this)(t, x); }
};
inline ASIFilterParams<U6> rigid_body_asif_params(int K)
{
  ASIFilterParams<U6> p;
  p.nh        = 1;
  p.asif.K    = (size_t)K;
  p.ulim.rows = 6;
  p.ulim.A.assign(36, 0.0);
  for (int i = 0; i < 6; ++i) p.ulim.A[7 * i] = 1.0;
  p.ulim.l.assign(6, -0.5);
  p.ulim.u.assign(6, 0.5);
  return p;
}
// agent b of the filter tests: on the desired trajectory at t = 0.3 + 0.1 b, asked for an input that pushes it down
inline X12B rigid_body_asif_state(int64_t b) { return RigidBodyModel{}.xdes(0.3 + 0.1 * double(b)); }
inline U6 rigid_body_asif_udes()
{
  U6 u;
  u.v = {0.1, 0.0, -0.4, 0.0, 0.2, 0.0};
  return u;
}

using MPC12B = MPC<double, X12B, U6, RigidBodyDyn, InputBox6>;
inline MPC12B make_rigid_body_mpc(int K, double tf)
{
  MPCParams p;
  p.K = (size_t)K; p.tf = tf;
  const RigidBodyModel mdl{};
  MPC12B m(mdl.f, mdl.cr, {-0.5, -0.5, -0.5, -0.5, -0.5, -0.5}, {0.5, 0.5, 0.5, 0.5, 0.5, 0.5}, p);
  m.set_xdes([mdl](double t) { return mdl.xdes(t); }, [mdl](double t) { return mdl.dxdes(t); });
  m.set_udes([mdl](double t) { return mdl.udes(t); });
  return m;
}

// ---- a pose filter on G = SE3 (Dof 6): driven by a known, time-varying body twist; the position is measured (Ny = 3) ----
struct PoseEkfDyn {
  SFB_LIE_HD Vec<6> operator()(double t, const SE3 &) const
  {
    return {0.8 + 0.3 * std::cos(2.0 * t), 0.1 * std::sin(t), 0.15, 0.1, -0.05 + 0.2 * std::sin(3.0 * t), 0.4};
  }
};
struct PoseEkfMeas {
  SFB_LIE_HD Vec<3> operator()(const SE3 & g) const { return g.p; }
};
inline Mat<6, 6> pose_ekf_Q()
{
  Mat<6, 6> Q{};
  for (int i = 0; i < 6; ++i) Q(i, i) = 0.02 + 0.01 * i;
  Q(0, 1) = Q(1, 0) = 0.004; Q(2, 4) = Q(4, 2) = -0.003;
  return Q;
}
inline Mat<3, 3> pose_ekf_R()
{
  Mat<3, 3> R{};
  R(0, 0) = 0.1; R(1, 1) = 0.12; R(2, 2) = 0.08; R(0, 1) = R(1, 0) = 0.01;
  return R;
}
inline SE3 pose_state(const double * s)  // (px, py, pz, w, x, y, z)
{
  return SE3{{s[0], s[1], s[2]}, SO3{s[3], s[4], s[5], s[6]}};
}
inline void pose_state_out(const SE3 & g, double * s)
{
  s[0] = g.p[0]; s[1] = g.p[1]; s[2] = g.p[2]; s[3] = g.q.w; s[4] = g.q.x; s[5] = g.q.y; s[6] = g.q.z;
}

}  // namespace sfbx
