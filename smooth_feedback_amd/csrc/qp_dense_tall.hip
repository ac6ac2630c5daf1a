// Tall dense QPs (few unknowns, many rows: 1 <= n <= 16, any m): the reduced-KKT route, one QP per wavefront.
//
// The algorithm is QPSolver::solve (qp_solver.hpp:343-568) as restated in oracle/qp_oracle.c -- scaling, pre-check, rho
// classes, warm / cold start, the ADMM update, the `iter % stop_check_iter == 1` check, check_stopping, max_iter,
// max_time, polish, un-scaling, objective -- with ONE difference: the linear solves.  The reference factorises the
// (n+m) x (n+m) KKT matrix [P+sigma I, A'; A, -diag(1/rho)] with a pivoted LDL'.  Only its n x n block is not diagonal,
// so this kernel eliminates the m dual unknowns first:
//     S x = rhs_x + A' diag(rho) rhs_z,   S = P + sigma I + A' diag(rho) A   (n x n, symmetric positive definite)
//     nu  = diag(rho) (A x - rhs_z)
// S gets an unpivoted LDL' once per solve (registers for n <= 8, LDS beyond).  Polish (:92-204) is reduced the same way:
//     Sp = P + delta I + (1/delta) Aa' Aa  over the active rows Aa,  ya = (Aa x - ha) / delta
// with the reference's refinement rounds against the UNPERTURBED system ("Tall dense QPs").
// Results therefore agree with the pivoted kernels to rounding, not bit for bit (include/sfb.h).
//
// Layout: lane L owns rows L, L + 64, ... of A.  Everything a row needs (its scaled A row, sy, y, z, the scaled bounds,
// rho) is private to its lane; the only cross-lane traffic of an iteration is the wave reduction of A' v (n sums).
//   REG (template RM > 0, m <= 64 RM, n RM <= 32): all of it in registers.
//   MEM (RM == 0): sy, y, z and A behind pointers -- LDS copies while they fit, else A is streamed from the caller's
//     array, sy and z live in a per-QP HBM workspace and y in the caller's output array.
// P (n x n) and the factor of S sit in LDS and are read at wave-uniform addresses.
// The hardware dispatcher is the work queue: one single-wave workgroup per QP, no queue memory, no allocation.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <type_traits>

#include "../../include/sfb.h"
#include "qp_dense_kernel.h"
#include "wave_util.h"

namespace sfb {
namespace {

constexpr int kTallFacRegN = 8;            // factor of S in registers up to this n (36 doubles), LDS beyond
constexpr size_t kTallLdsBudget = 60 * 1024;  // MEM: rows and A are copied to LDS while everything fits in this

__device__ __forceinline__ int ptri(const int i, const int j) { return ((i * (i + 1)) >> 1) + j; }

// f(slot, row) for the lane's rows in ascending order; REG: fully unrolled, `slot` is a compile-time register index
template<int RM, class F>
__device__ __forceinline__ void tall_rows(const int m, const int lane, F &&f)
{
  if constexpr (RM > 0) {
#pragma unroll
    for (int s = 0; s < RM; ++s) {
      const int i = lane + kWave * s;
      if (i < m) f(s, i);
    }
  } else {
    for (int i = lane; i < m; i += kWave) f(0, i);
  }
}

struct RowC {
  double sy, lo, hi, rho, rinv;
};

constexpr size_t tall_fixed_doubles(int n) { return (size_t)n * n + (size_t)n * (n + 1) / 2 + 2 * (size_t)n; }

template<int N, int RM>
__global__ void __launch_bounds__(64) qp_dense_tall_kernel(const DenseKernelParams kp, const QpBatch g, double *__restrict__ gws,
                                                          const int in_lds)
{
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr int RS = RM > 0 ? RM : 1;
  constexpr int NF = N <= kTallFacRegN ? N * (N + 1) / 2 : 1;
  const int lane = threadIdx.x;
  const int m    = kp.m;
  const size_t b = blockIdx.x;
  const double inf = INFINITY;
  const double *gl = g.l + b * (size_t)m, *gu = g.u + b * (size_t)m;

  // LDS: P (col-major, as stored), the packed factor of S (strict lower part L, 1 / d on the diagonal), two scratch rows
  double *Pl = sm, *Sl = Pl + N * N, *Wl = Sl + N * (N + 1) / 2, *Dl = Wl + N;
  // MEM mode row state
  double *Msy = nullptr, *Mz = nullptr, *My = nullptr;
  const double *MA = g.A + b * (size_t)m * N;
  if constexpr (RM == 0) {
    if (in_lds) {
      Msy = Dl + N;
      Mz  = Msy + m;
      My  = Mz + m;
      double *Al = My + m;
      for (int e = lane; e < m * N; e += kWave) Al[e] = MA[e];
      MA = Al;
    } else {
      Msy = gws + b * (size_t)(2 * m);
      Mz  = Msy + m;
      My  = g.y + b * (size_t)m;
    }
  }
  // REG mode row state
  double Ra[RS][N], Rsy[RS], Ry[RS], Rz[RS], Rlo[RS], Rhi[RS], Rrho[RS], Rrinv[RS];

  for (int e = lane; e < N * N; e += kWave) Pl[e] = g.P[b * (size_t)(N * N) + e];
  double q[N], sx[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    q[j]  = g.q[b * N + j];
    sx[j] = 1.0;
  }
  if constexpr (RM > 0) {
#pragma unroll
    for (int s = 0; s < RM; ++s) {
      const int i = lane + kWave * s;
#pragma unroll
      for (int j = 0; j < N; ++j) Ra[s][j] = (i < m) ? MA[i + (size_t)j * m] : 0.0;
      Rsy[s] = 1.0;
      Ry[s] = Rz[s] = 0.0;
      Rlo[s] = Rhi[s] = 0.0;
      Rrho[s] = Rrinv[s] = 1.0;
    }
  } else {
    for (int i = lane; i < m; i += kWave) Msy[i] = 1.0;
  }
  wave_lds_fence();

  auto SY = [&](const int s, const int i) -> double & { if constexpr (RM > 0) return Rsy[s]; else return Msy[i]; };
  auto Y  = [&](const int s, const int i) -> double & { if constexpr (RM > 0) return Ry[s]; else return My[i]; };
  auto Z  = [&](const int s, const int i) -> double & { if constexpr (RM > 0) return Rz[s]; else return Mz[i]; };

  // ---- scale :673-730 (maxima only: the same bits as the reference whatever the order) ----
  double c = 1.0;
  if (kp.scaling) {
    double sum = 0.0;
#pragma unroll
    for (int col = 0; col < N; ++col) {  // :681-690
      double t = 0.0;
      for (int row = 0; row < N; ++row) t = fmax(t, fabs(Pl[row + col * N]));
      if (t == 0.0) t = 1.0;
      sum = (col == 0) ? t : sum + t;
    }
    double qn = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) qn = fmax(qn, fabs(q[j]));
    c = 1.0 / fmax(fmax(1e-6, sum / (double)N), qn);  // :693
    int pass = 0;
    double crit;
    do {  // :698-729
      double incx[N];
#pragma unroll
      for (int col = 0; col < N; ++col) {
        double v = 0.0;
#pragma unroll
        for (int row = 0; row < N; ++row) v = fmax(v, fabs(c * sx[row] * sx[col] * Pl[row + col * N]));
        incx[col] = v;
      }
      double cm = 0.0;
      tall_rows<RM>(m, lane, [&](const int s, const int i) {
        const double syi = SY(s, i);
        double inc       = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          double araw;
          if constexpr (RM > 0) araw = Ra[s][j]; else araw = MA[i + (size_t)j * m];
          const double a = fabs(syi * sx[j] * araw);
          incx[j]        = fmax(incx[j], a);
          inc            = fmax(inc, a);
        }
        if (inc == 0.0) inc = 1.0;
        cm       = fmax(cm, fabs(inc - 1.0));
        SY(s, i) = sqrt(1.0 / fmax(inc, 1e-8)) * syi;
      });
#pragma unroll
      for (int j = 0; j < N; ++j) {
        double v = wave_max(incx[j]);
        if (v == 0.0) v = 1.0;
        cm    = fmax(cm, fabs(v - 1.0));
        sx[j] = sqrt(1.0 / fmax(v, 1e-8)) * sx[j];
      }
      crit = wave_max(cm);
    } while (pass++ < 10 && crit > 0.1);
  }

  // ---- pre-check and rho :361-374; REG: the scaled rows (sy_i A_ij) sx_j and bounds replace the raw ones ----
  const double rho_eq = 1e3 * kp.rho_bar;
  const double rinv_free = 1.0 / 1e-6, rinv_eq = 1.0 / rho_eq, rinv_bar = 1.0 / kp.rho_bar;
  int ret_code = -1;
  {
    bool bad = false;
    tall_rows<RM>(m, lane, [&](const int s, const int i) {
      const double li = gl[i], ui = gu[i];
      bad = bad || (li == inf) || (ui == -inf) || (ui - li < 0.0);
      if constexpr (RM > 0) {
        const double syi = Rsy[s];
#pragma unroll
        for (int j = 0; j < N; ++j) Ra[s][j] = syi * Ra[s][j] * sx[j];
        Rlo[s] = syi * li;
        Rhi[s] = syi * ui;
        if (li == -inf && ui == inf) { Rrho[s] = 1e-6; Rrinv[s] = rinv_free; }
        else if (syi * fabs(li - ui) < 1e-5) { Rrho[s] = rho_eq; Rrinv[s] = rinv_eq; }
        else { Rrho[s] = kp.rho_bar; Rrinv[s] = rinv_bar; }
      }
    });
    if (wave_ballot(bad)) ret_code = SFB_QP_PRIMAL_INFEASIBLE;
  }
  // the scaled row and its constants
  auto row_load = [&](const int s, const int i, double (&ar)[N], RowC &rc) {
    if constexpr (RM > 0) {
#pragma unroll
      for (int j = 0; j < N; ++j) ar[j] = Ra[s][j];
      rc = RowC{Rsy[s], Rlo[s], Rhi[s], Rrho[s], Rrinv[s]};
    } else {
      const double syi = Msy[i], li = gl[i], ui = gu[i];
#pragma unroll
      for (int j = 0; j < N; ++j) ar[j] = syi * MA[i + (size_t)j * m] * sx[j];
      rc.sy = syi;
      rc.lo = syi * li;
      rc.hi = syi * ui;
      if (li == -inf && ui == inf) { rc.rho = 1e-6; rc.rinv = rinv_free; }
      else if (syi * fabs(li - ui) < 1e-5) { rc.rho = rho_eq; rc.rinv = rinv_eq; }
      else { rc.rho = kp.rho_bar; rc.rinv = rinv_bar; }
    }
  };
  double qc[N];  // (c sx_j) q_j of :450
#pragma unroll
  for (int j = 0; j < N; ++j) qc[j] = c * sx[j] * q[j];

  const unsigned long long t0_ticks = wall_clock64();  // :376

  // S = Ps + diag_add I + A' diag(w) A into Sl (lower triangle), then its unpivoted LDL' in place.  Ps is the scaled upper
  // triangle of P mirrored (:399-402 / :159-161).  Returns false when a pivot is not positive.
  auto build_and_factor = [&](const double diag_add, auto &&weight) -> bool {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double acc[N];
#pragma unroll
      for (int j = 0; j < N; ++j) acc[j] = 0.0;
      tall_rows<RM>(m, lane, [&](const int s, const int i) {
        double ar[N];
        RowC rc;
        row_load(s, i, ar, rc);
        const double t = weight(s, i, rc) * ar[k];
#pragma unroll
        for (int j = 0; j <= k; ++j) acc[j] = fma(ar[j], t, acc[j]);
      });
#pragma unroll
      for (int j = 0; j <= k; ++j) {
        double v = c * sx[j] * Pl[j + k * N] * sx[k];
        if (j == k) v += diag_add;
        Sl[ptri(k, j)] = v + wave_sum(acc[j]);
      }
    }
    wave_lds_fence();
    // every lane runs the same factorisation on the same LDS words (uniform addresses, identical values written)
    bool ok = true;
    for (int k = 0; k < N; ++k) {
      for (int j = 0; j < k; ++j) Wl[j] = Sl[ptri(k, j)] * Dl[j];
      double d = Sl[ptri(k, k)];
      for (int j = 0; j < k; ++j) d = fma(-Sl[ptri(k, j)], Wl[j], d);
      ok = ok && (d > 0.0);
      const double dinv = 1.0 / d;
      Dl[k] = d;
      for (int i = k + 1; i < N; ++i) {
        double v = Sl[ptri(i, k)];
        for (int j = 0; j < k; ++j) v = fma(-Sl[ptri(i, j)], Wl[j], v);
        Sl[ptri(i, k)] = v * dinv;
      }
      Sl[ptri(k, k)] = dinv;
      wave_lds_fence();
    }
    return ok;
  };
  double Lr[NF];
  auto factor_to_regs = [&]() {
    if constexpr (N <= kTallFacRegN) {
#pragma unroll
      for (int e = 0; e < NF; ++e) Lr[e] = Sl[e];
    }
  };
  auto LF = [&](const int i, const int j) -> double { if constexpr (N <= kTallFacRegN) return Lr[ptri(i, j)]; else return Sl[ptri(i, j)]; };
  auto solve_S = [&](double (&v)[N]) {  // L D L' v_out = v_in
#pragma unroll
    for (int i = 1; i < N; ++i)
#pragma unroll
      for (int j = 0; j < i; ++j) v[i] = fma(-LF(i, j), v[j], v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] *= LF(i, i);
#pragma unroll
    for (int i = N - 2; i >= 0; --i)
#pragma unroll
      for (int j = N - 1; j > i; --j) v[i] = fma(-LF(j, i), v[j], v[i]);
  };

  if (!build_and_factor(kp.sigma, [](int, int, const RowC &rc) { return rc.rho; })) ret_code = SFB_QP_UNKNOWN;  // :428-433
  factor_to_regs();

  // ---- initial iterate :436-445 ----
  double x[N];
  double gp[N];  // this lane's part of A' (rho z - y), the row term of the next right-hand side
#pragma unroll
  for (int j = 0; j < N; ++j) gp[j] = 0.0;
  if (g.wx != nullptr) {
    const double *wx = g.wx + b * (size_t)N, *wy = g.wy + b * (size_t)m;
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = (1.0 / sx[j]) * wx[j];
    tall_rows<RM>(m, lane, [&](const int s, const int i) {
      double ar[N];
      RowC rc;
      row_load(s, i, ar, rc);
      const double y0 = c * ((1.0 / rc.sy) * wy[i]);
      double z0       = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) z0 = fma(ar[j], x[j], z0);
      Y(s, i) = y0;
      Z(s, i) = z0;
      const double w = rc.rho * z0 - y0;
#pragma unroll
      for (int j = 0; j < N; ++j) gp[j] = fma(ar[j], w, gp[j]);
    });
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = 0.0;
    tall_rows<RM>(m, lane, [&](const int s, const int i) {
      Y(s, i) = 0.0;
      Z(s, i) = 0.0;
    });
  }

  // ---- ADMM loop :447-510 ----
  uint32_t iter        = 0;
  const uint32_t sci   = kp.stop_check_iter;
  const uint32_t maxit = kp.max_iter;
  double xt[N], dx[N];
  // one pass over the rows: nu, z, y of :451-477, the next right-hand side, and (CHK) every row quantity of check_stopping
  auto admm_pass = [&](auto chk_tag) -> int {
    constexpr bool CHK = decltype(chk_tag)::value;
    double aty[N], atdy[N];
    double axn = 0.0, rn = 0.0, zun = 0.0, edy = 0.0, ssum = 0.0, mxU = -inf, mxL = -inf, dxn = 0.0, thr_d = 0.0;
    bool rowbad = false;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      gp[j] = 0.0;
      aty[j] = atdy[j] = 0.0;
      if constexpr (CHK) dxn = fmax(dxn, fabs(sx[j] * dx[j]));
    }
    if constexpr (CHK) thr_d = kp.eps_dinf * dxn;
    tall_rows<RM>(m, lane, [&](const int s, const int i) {
      double ar[N];
      RowC rc;
      row_load(s, i, ar, rc);
      double ax = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) ax = fma(ar[j], xt[j], ax);
      const double yo = Y(s, i), zo = Z(s, i);
      const double nu = rc.rho * (ax - zo) + yo;  // rho (A x~ - (z - y / rho))
      double zn       = kp.alpha * (rc.rinv * nu) + kp.alpha_comp * (rc.rinv * yo) + zo;
      zn              = (zn < rc.lo) ? rc.lo : zn;
      zn              = (rc.hi < zn) ? rc.hi : zn;
      const double yn = kp.alpha_comp * yo + kp.alpha * nu + rc.rho * zo - rc.rho * zn;
      Y(s, i) = yn;
      Z(s, i) = zn;
      const double w = rc.rho * zn - yn;
#pragma unroll
      for (int j = 0; j < N; ++j) gp[j] = fma(ar[j], w, gp[j]);
      if constexpr (CHK) {  // :479-487 and the row sums of :584-641; A_ij = a_ij / (sy_i sx_j)
        const double isy = 1.0 / rc.sy, dy = yn - yo;
        double axs = 0.0, adx = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          axs     = fma(ar[j], x[j], axs);
          adx     = fma(ar[j], dx[j], adx);
          aty[j]  = fma(ar[j], yn, aty[j]);
          atdy[j] = fma(ar[j], dy, atdy[j]);
        }
        axs *= isy;
        adx *= isy;
        const double zus = isy * zn, dyus = rc.sy * dy / c;
        axn = fmax(axn, fabs(axs));
        rn  = fmax(rn, fabs(axs - zus));
        zun = fmax(zun, fabs(zus));
        edy = fmax(edy, fabs(dyus));
        if (rc.hi != inf) ssum += rc.hi * fmax(0.0, dy); else mxU = fmax(mxU, dyus);
        if (rc.lo != -inf) ssum += rc.lo * fmin(0.0, dy); else mxL = fmax(mxL, -dyus);
        bool ok;
        if (rc.hi == inf) ok = adx >= -thr_d;
        else if (rc.lo == -inf) ok = adx <= thr_d;
        else ok = fabs(adx) < thr_d;
        rowbad = rowbad || !ok;
      }
    });
    if constexpr (!CHK) return -1;
    else {
      // check_stopping :574-644 on x_us = sx x, y_us = sy y / c, z_us = z / sy, dx_us, dy_us
      const double Ax_norm = wave_max(axn), r_norm = wave_max(rn), z_norm = wave_max(zun);
      const double Edy = wave_max(edy), s_sum = wave_sum(ssum) / c;
      const double dU = wave_max(mxU), dL = wave_max(mxL);
      const bool anybad = wave_ballot(rowbad) != 0ull;
      double Aty[N], Atdy[N], xus[N], dxus[N];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const double f = 1.0 / (c * sx[j]);
        Aty[j]  = wave_sum(aty[j]) * f;
        Atdy[j] = wave_sum(atdy[j]) * f;
        xus[j]  = sx[j] * x[j];
        dxus[j] = sx[j] * dx[j];
      }
      if (r_norm <= kp.eps_abs + kp.eps_rel * fmax(Ax_norm, z_norm)) {  // :584-594
        double pxn = 0.0, qn = 0.0, an = 0.0, resn = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          double px = 0.0;
#pragma unroll
          for (int j = 0; j < N; ++j) px = fma(Pl[i + j * N], xus[j], px);
          pxn  = fmax(pxn, fabs(px));
          qn   = fmax(qn, fabs(q[i]));
          an   = fmax(an, fabs(Aty[i]));
          resn = fmax(resn, fabs(px + (q[i] + Aty[i])));
        }
        if (resn <= kp.eps_abs + kp.eps_rel * fmax(fmax(pxn, qn), an)) return SFB_QP_OPTIMAL;
      }
      {  // :598-621
        const double thr = kp.eps_pinf * Edy;
        double an        = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) an = fmax(an, fabs(Atdy[j]));
        const double sacc = (dU > thr || dL > thr) ? inf : s_sum;
        const double mxv  = (an < sacc) ? sacc : an;
        if (mxv < thr) return SFB_QP_PRIMAL_INFEASIBLE;
      }
      {  // :625-641
        double pn = 0.0, qdx = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          double px = 0.0;
#pragma unroll
          for (int j = 0; j < N; ++j) px = fma(Pl[i + j * N], dxus[j], px);
          pn  = fmax(pn, fabs(px));
          qdx = fma(q[i], dxus[i], qdx);
        }
        if (pn <= thr_d && qdx <= thr_d && !anybad) return SFB_QP_DUAL_INFEASIBLE;
      }
      return -1;
    }
  };

  for (; iter != maxit && ret_code < 0; ++iter) {
#pragma unroll
    for (int j = 0; j < N; ++j) xt[j] = (kp.sigma * x[j] - qc[j]) + wave_sum(gp[j]);  // :450-451 reduced
    solve_S(xt);                                                                         // :462
    const bool chk = (sci != 0) && (iter % sci == 1);                                    // :465
#pragma unroll
    for (int j = 0; j < N; ++j) {  // :470
      const double xn = kp.alpha * xt[j] + kp.alpha_comp * x[j];
      dx[j] = xn - x[j];
      x[j]  = xn;
    }
    if (chk) {
      ret_code = admm_pass(std::true_type{});
      if (ret_code < 0 && max_time_exceeded(kp.max_time_ns, t0_ticks)) ret_code = SFB_QP_MAX_TIME;  // :504-507
    } else {
      (void)admm_pass(std::false_type{});
    }
  }

  // ---- polish :92-204, :515-539, reduced to n x n (a factorisation that fails leaves the ADMM iterate) ----
  if (ret_code == SFB_QP_OPTIMAL && kp.polish) {
    const double eps = DBL_EPSILON, dinv = 1.0 / kp.delta;
    // active rows (:113-123) are recognised from the scaled dual, which stays in place until the end; t_a uses the z slot
    auto act = [&](const double yi, const RowC &rc) -> int {
      if (yi < -100 * eps && rc.lo != -inf) return 1;
      if (yi > 100 * eps && rc.hi != inf) return 2;
      return 0;
    };
    tall_rows<RM>(m, lane, [&](const int s, const int i) { Z(s, i) = 0.0; });
    const bool ok = build_and_factor(kp.delta, [&](const int s, const int i, const RowC &rc) { return act(Y(s, i), rc) ? dinv : 0.0; });
    if (ok) {
      factor_to_regs();
      double tx[N];
#pragma unroll
      for (int j = 0; j < N; ++j) tx[j] = 0.0;
      for (uint32_t it = 0; it != kp.polish_iter; ++it) {  // :193-195  t += Hp^-1 (h - H t)
        // r_x = h_x - Ps t_x - Aa' t_a,  r_a = h_a - Aa t_x;  reduced right-hand side r_x + Aa' r_a / delta
        double acc[N], rhs[N];
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = 0.0;
        tall_rows<RM>(m, lane, [&](const int s, const int i) {
          double ar[N];
          RowC rc;
          row_load(s, i, ar, rc);
          const int a = act(Y(s, i), rc);
          if (a) {
            double at = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) at = fma(ar[j], tx[j], at);
            const double ra = ((a == 1) ? rc.lo : rc.hi) - at;
            const double w  = ra * dinv - Z(s, i);
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] = fma(ar[j], w, acc[j]);
          }
        });
#pragma unroll
        for (int j = 0; j < N; ++j) {
          double pt = 0.0;
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const double pjk = (j <= k) ? c * sx[j] * Pl[j + k * N] * sx[k] : c * sx[k] * Pl[k + j * N] * sx[j];
            pt = fma(pjk, tx[k], pt);
          }
          rhs[j] = (-qc[j] - pt) + wave_sum(acc[j]);
        }
        solve_S(rhs);  // d_x
        tall_rows<RM>(m, lane, [&](const int s, const int i) {
          double ar[N];
          RowC rc;
          row_load(s, i, ar, rc);
          const int a = act(Y(s, i), rc);
          if (a) {
            double at = 0.0, ad = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) {
              at = fma(ar[j], tx[j], at);
              ad = fma(ar[j], rhs[j], ad);
            }
            const double ra = ((a == 1) ? rc.lo : rc.hi) - at;
            Z(s, i) += (ad - ra) * dinv;  // d_a = (Aa d_x - r_a) / delta
          }
        });
#pragma unroll
        for (int j = 0; j < N; ++j) tx[j] += rhs[j];
      }
#pragma unroll
      for (int j = 0; j < N; ++j) x[j] = tx[j];  // :199
      tall_rows<RM>(m, lane, [&](const int s, const int i) {  // :200-201
        double ar[N];
        RowC rc;
        row_load(s, i, ar, rc);
        if (act(Y(s, i), rc)) Y(s, i) = Z(s, i);
      });
    }
  }

  // ---- un-scale and report :544-548 ----
  double xo[N];
#pragma unroll
  for (int j = 0; j < N; ++j) xo[j] = sx[j] * x[j];
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) g.x[b * N + j] = xo[j];
  }
  {
    double *oy = g.y + b * (size_t)m;
    tall_rows<RM>(m, lane, [&](const int s, const int i) { oy[i] = SY(s, i) * Y(s, i) / c; });
  }
  if (lane == 0) {
    if (g.obj != nullptr) {
      double o = 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) s = fma(0.5 * Pl[i + j * N], xo[j], s);
        o = fma(xo[i], s + q[i], o);
      }
      g.obj[b] = o;
    }
    g.code[b] = (ret_code >= 0) ? ret_code : SFB_QP_MAX_ITERATIONS;
    if (g.iter != nullptr) g.iter[b] = iter;
  }
}

// rows per lane the REG instance of this n keeps in registers (0: none) -- n * rows <= 32 doubles of A per lane
constexpr int tall_reg_rows(int n, int m)
{
  const int r = (m + kWave - 1) / kWave;
  if (n <= 4) return r <= 4 ? 4 : (r <= 8 ? 8 : 0);
  if (n <= 8) return r <= 4 ? 4 : 0;
  return 0;
}

size_t tall_lds_doubles(int n, int m, bool rows_in_lds)
{
  return tall_fixed_doubles(n) + (rows_in_lds ? (size_t)3 * m + (size_t)m * n : 0);
}

bool tall_rows_fit_lds(int n, int m) { return tall_lds_doubles(n, m, true) * sizeof(double) <= kTallLdsBudget; }

template<int N>
hipError_t tall_launch_n(const DenseKernelParams &kp, int64_t batch, const QpBatch &g, double *ws, hipStream_t stream)
{
  const dim3 grid((unsigned)batch), block(kWave);
  const int rm = tall_reg_rows(N, kp.m);
  const size_t fixed = tall_fixed_doubles(N) * sizeof(double);
  if constexpr (N <= 8) {
    if (rm == 4) {
      hipLaunchKernelGGL((qp_dense_tall_kernel<N, 4>), grid, block, fixed, stream, kp, g, ws, 0);
      return hipGetLastError();
    }
  }
  if constexpr (N <= 4) {
    if (rm == 8) {
      hipLaunchKernelGGL((qp_dense_tall_kernel<N, 8>), grid, block, fixed, stream, kp, g, ws, 0);
      return hipGetLastError();
    }
  }
  const bool in_lds = tall_rows_fit_lds(N, kp.m);
  if (!in_lds && ws == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL((qp_dense_tall_kernel<N, 0>), grid, block, tall_lds_doubles(N, kp.m, in_lds) * sizeof(double), stream, kp, g, ws,
                     in_lds ? 1 : 0);
  return hipGetLastError();
}

}  // namespace

size_t qp_dense_tall_ws_bytes(int n, int m, int64_t batch)
{
  if (n < 1 || n > kDenseTallMaxN || tall_reg_rows(n, m) != 0 || tall_rows_fit_lds(n, m)) return 0;
  return (size_t)batch * 2 * (size_t)m * sizeof(double);
}

hipError_t qp_dense_tall_launch(const DenseKernelParams &kp, int64_t batch, const QpBatch &g, hipStream_t stream, void *workspace)
{
  double *ws = static_cast<double *>(workspace);
  switch (kp.n) {
#define SFB_TALL_CASE(NN) case NN: return tall_launch_n<NN>(kp, batch, g, ws, stream);
    SFB_TALL_CASE(1) SFB_TALL_CASE(2) SFB_TALL_CASE(3) SFB_TALL_CASE(4) SFB_TALL_CASE(5) SFB_TALL_CASE(6) SFB_TALL_CASE(7) SFB_TALL_CASE(8)
    SFB_TALL_CASE(9) SFB_TALL_CASE(10) SFB_TALL_CASE(11) SFB_TALL_CASE(12) SFB_TALL_CASE(13) SFB_TALL_CASE(14) SFB_TALL_CASE(15) SFB_TALL_CASE(16)
#undef SFB_TALL_CASE
    default: return hipErrorInvalidValue;
  }
}

}  // namespace sfb
