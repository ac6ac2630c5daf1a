// Kernels of the swarm SQP solver: everything around the QP solve of an iteration ("Swarm SQP", holds the law the
// comments below number).  Model-free: values, Jacobians and Hessians arrive as device arrays.  One wave per agent where a
// quantity reduces over an agent (kkt, judge, accept), one lane per double where it does not (assemble, trial, start).
#include <hip/hip_runtime.h>

#include "nlp_sqp_kernel.h"
#include "wave_util.h"

namespace sfb {
namespace {

constexpr int kLaneBlock = 256;

__device__ __forceinline__ double clip(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// sum max(0, gl - g) + sum max(0, g - gu) of one agent, rows strided over the lanes, then the wave tree
__device__ __forceinline__ double violation_l1(const NlpSqpDev &p, const double *g, int lane)
{
  double acc = 0.0;
  for (int r = lane; r < p.m; r += kWave) {
    const double gr = g[r];
    acc = acc + (fmax(0.0, p.gl[r] - gr) + fmax(0.0, gr - p.gu[r]));
  }
  return wave_sum(acc);
}

// |lambda| times the distance to the nearer finite side; rows without a finite side and equalities take no part
__device__ __forceinline__ double comp_term(double mult, double v, double lo, double hi)
{
  const bool fl = isfinite(lo), fh = isfinite(hi);
  if (fl && fh) return lo == hi ? 0.0 : fabs(mult) * fmin(v - lo, hi - v);
  if (fl) return fabs(mult) * (v - lo);
  if (fh) return fabs(mult) * (hi - v);
  return 0.0;
}

__global__ __launch_bounds__(kWave) void nlp_sqp_kkt_kernel(const NlpSqpDev p, const int64_t batch, const double *__restrict__ df_,
                                                            const double *__restrict__ g_, const double *__restrict__ dg_)
{
  const int64_t b = blockIdx.x;
  const int lane  = threadIdx.x;
  if (b >= batch) return;
  if (p.status[b] != kNlpRunning) {  // frozen (law 4)
    if (lane == 0) p.need[b] = 0;
    return;
  }
  if (lane == 0) p.phase[b] = 0;  // a line search the caller left open is dropped, uncommitted: the call starts a new iteration
  const double *df = df_ + b * p.n, *g = g_ + b * p.m, *dg = dg_ + b * (int64_t)p.nnzJ;
  const double *x = p.x + b * p.n, *lam = p.lambda + b * p.m, *z = p.z + b * p.n;
  double rs = 0.0, rp = 0.0, rc = 0.0;
  bool bad = false;
  for (int c = lane; c < p.n; c += kWave) {
    double s = df[c];
    for (int t = p.Jc_colptr[c]; t < p.Jc_colptr[c + 1]; ++t) s = s + dg[p.Jc_pos[t]] * lam[p.Jc_row[t]];
    s = s + z[c];
    bad = bad || !isfinite(s) || !isfinite(x[c]);
    rs  = fmax(rs, fabs(s));
    rp  = fmax(rp, fmax(p.xl[c] - x[c], x[c] - p.xu[c]));
    rc  = fmax(rc, comp_term(z[c], x[c], p.xl[c], p.xu[c]));
  }
  for (int r = lane; r < p.m; r += kWave) {
    bad = bad || !isfinite(g[r]);
    rp  = fmax(rp, fmax(p.gl[r] - g[r], g[r] - p.gu[r]));
    rc  = fmax(rc, comp_term(lam[r], g[r], p.gl[r], p.gu[r]));
  }
  rs = wave_max(rs);
  rp = wave_max(rp);
  rc = wave_max(rc);
  const double v1 = violation_l1(p, g, lane);
  const bool any_bad = wave_ballot(bad) != 0ull;
  if (lane == 0) {
    p.r_stat[b] = rs;
    p.r_pri[b]  = rp;
    p.r_comp[b] = rc;
    p.v1[b]     = v1;
    int st      = kNlpRunning;
    if (!any_bad && rs <= p.tol && rp <= p.tol && rc <= p.tol)
      st = kNlpOptimal;
    else if (p.iter[b] >= p.max_iter)
      st = kNlpMaxIterations;
    p.status[b] = st;
    p.need[b]   = st == kNlpRunning;
  }
}

// one wave walks the flags 64 at a time: a ballot and a popcount below the lane give every kept agent its place
__global__ __launch_bounds__(kWave) void nlp_sqp_compact_kernel(const int32_t *__restrict__ flag, const int64_t batch,
                                                                int32_t *__restrict__ list, int32_t *__restrict__ count)
{
  const int lane = threadIdx.x;
  int base       = 0;
  for (int64_t b0 = 0; b0 < batch; b0 += kWave) {
    const int64_t b   = b0 + lane;
    const bool keep   = b < batch && flag[b] != 0;
    const unsigned long long mask = wave_ballot(keep);
    if (keep) list[base + __popcll(mask & lanemask_lt(lane))] = (int32_t)b;
    base += __popcll(mask);
  }
  if (lane == 0) *count = base;
}

__global__ __launch_bounds__(kLaneBlock) void nlp_sqp_assemble_kernel(const NlpSqpDev p, const int32_t *__restrict__ list, const int64_t count,
                                                                      const double *__restrict__ df, const double *__restrict__ g,
                                                                      const double *__restrict__ dg, const double *__restrict__ hess,
                                                                      double *__restrict__ Px, double *__restrict__ q, double *__restrict__ Ax,
                                                                      double *__restrict__ l, double *__restrict__ u, double *__restrict__ wx,
                                                                      double *__restrict__ wy)
{
  const int64_t per = (int64_t)p.nnzP + p.n + p.nnzA + 2 * (int64_t)p.mq + p.n + p.mq;
  const int64_t idx = (int64_t)blockIdx.x * kLaneBlock + threadIdx.x;
  if (idx >= count * per) return;
  const int64_t k = idx / per;
  int64_t e       = idx - k * per;
  const int64_t a = list[k];
  if (e < p.nnzP) {  // P = H + mu I: the diagonal slots take one add, the others (of both triangles) are copied
    const double h     = hess[a * p.nnzH + p.P_src[e]];
    Px[k * p.nnzP + e] = p.P_row[e] == p.P_col[e] ? h + p.mu[a] : h;
    return;
  }
  e -= p.nnzP;
  if (e < p.n) { q[k * p.n + e] = df[a * p.n + e]; return; }
  e -= p.n;
  if (e < p.nnzA) { Ax[k * p.nnzA + e] = e < p.nnzJ ? dg[a * p.nnzJ + e] : 1.0; return; }
  e -= p.nnzA;
  if (e < 2 * (int64_t)p.mq) {
    const bool upper = e >= p.mq;
    const int r      = (int)(upper ? e - p.mq : e);
    double bound, at;
    if (r < p.m) {
      bound = upper ? p.gu[r] : p.gl[r];
      at    = g[a * p.m + r];
    } else {
      const int j = p.bound_var[r - p.m];
      bound       = upper ? p.xu[j] : p.xl[j];
      at          = p.x[a * p.n + j];
    }
    (upper ? u : l)[k * p.mq + r] = bound - at;
    return;
  }
  e -= 2 * (int64_t)p.mq;
  if (e < p.n) { wx[k * p.n + e] = p.d[a * p.n + e]; return; }  // warm start: the agent's last accepted (d, y)
  e -= p.n;
  wy[k * p.mq + e] = p.yqp[a * p.mq + e];
}

__global__ __launch_bounds__(kWave) void nlp_sqp_judge_kernel(const NlpSqpDev p, const int32_t *__restrict__ list, const int64_t count, const int rung,
                                                              const double *__restrict__ f, const double *__restrict__ Px_,
                                                              const double *__restrict__ q_, const double *__restrict__ xs_,
                                                              const double *__restrict__ ys_, const int32_t *__restrict__ code)
{
  const int64_t k = blockIdx.x;
  const int lane  = threadIdx.x;
  if (k >= count) return;
  const int64_t a  = list[k];
  const double *Px = Px_ + k * p.nnzP, *q = q_ + k * p.n, *d = xs_ + k * p.n, *y = ys_ + k * p.mq;
  bool bad = false, nonzero = false;
  double dd = 0.0, dfd = 0.0, ymax = 0.0;
  for (int j = lane; j < p.n; j += kWave) {
    const double dj = d[j];
    bad     = bad || !isfinite(dj);
    nonzero = nonzero || dj != 0.0;
    dd      = dd + dj * dj;
    dfd     = dfd + q[j] * dj;
  }
  for (int r = lane; r < p.mq; r += kWave) {
    bad = bad || !isfinite(y[r]);
    if (r < p.m) ymax = fmax(ymax, fabs(y[r]));
  }
  double dPd = 0.0;  // over the upper triangle, off-diagonal entries counted twice
  for (int e = lane; e < p.nnzP; e += kWave) {
    const int r = p.P_row[e], c = p.P_col[e];
    if (r > c) continue;
    const double t = (Px[e] * d[r]) * d[c];
    dPd            = dPd + (r == c ? t : 2.0 * t);
  }
  dd   = wave_sum(dd);
  dfd  = wave_sum(dfd);
  dPd  = wave_sum(dPd);
  ymax = wave_max(ymax);
  const bool any_bad = wave_ballot(bad) != 0ull, any_nonzero = wave_ballot(nonzero) != 0ull;
  const int cd        = code[k];
  const bool accepted = cd == 0 && !any_bad && (!any_nonzero || dPd >= p.kappa * dd);
  if (accepted) {  // the direction and its multipliers become the agent's, and its warm start from now on
    for (int j = lane; j < p.n; j += kWave) p.d[a * p.n + j] = d[j];
    for (int r = lane; r < p.mq; r += kWave) p.yqp[a * p.mq + r] = y[r];
  }
  if (lane != 0) return;
  p.dd[a]  = dd;
  p.dPd[a] = dPd;
  if (accepted) {  // law 3, the part that does not depend on alpha
    const double nu = fmax(p.nu[a], 1.1 * ymax), v1 = p.v1[a];
    p.nu[a]       = nu;
    p.phi0[a]     = f[a] + nu * v1;
    p.slope[a]    = dfd - nu * v1;
    p.alpha[a]    = 1.0;
    p.halvings[a] = 0;
    p.phase[a]    = 1;
    p.need[a]     = 0;
    return;
  }
  if (cd == 2 && rung == 0) {  // inconsistent linearised constraints: the shift cannot repair them
    p.status[a] = kNlpPrimalInfeasible;
    p.need[a]   = 0;
    return;
  }
  const double mu = fmax(p.mu_first, p.mu_grow * p.mu[a]);
  p.mu[a]         = mu;
  if (mu > p.mu_max) {
    p.status[a] = kNlpUnknown;
    p.need[a]   = 0;
  }
}

__global__ __launch_bounds__(kLaneBlock) void nlp_sqp_trial_kernel(const NlpSqpDev p, const int64_t batch, double *__restrict__ x_trial)
{
  const int64_t idx = (int64_t)blockIdx.x * kLaneBlock + threadIdx.x;
  if (idx >= batch * p.n) return;
  const int64_t b = idx / p.n;
  const int j     = (int)(idx - b * p.n);
  const double xj = p.x[idx];
  x_trial[idx]    = p.phase[b] == 1 ? clip(xj + p.alpha[b] * p.d[idx], p.xl[j], p.xu[j]) : xj;
}

__global__ __launch_bounds__(kWave) void nlp_sqp_accept_kernel(const NlpSqpDev p, const int64_t batch, const double *__restrict__ f_trial,
                                                               const double *__restrict__ g_trial)
{
  const int64_t b = blockIdx.x;
  const int lane  = threadIdx.x;
  if (b >= batch || p.phase[b] != 1) return;
  const double alpha = p.alpha[b];
  const double *gt   = g_trial + b * p.m;
  bool bad           = false;  // fmax drops a NaN, so violation_l1 would count a row that did not evaluate as satisfied
  for (int r = lane; r < p.m; r += kWave) bad = bad || !isfinite(gt[r]);
  const double v1t  = violation_l1(p, gt, lane);
  const double phit = f_trial[b] + p.nu[b] * v1t;
  const bool finite = wave_ballot(bad) == 0ull && isfinite(phit);  // a merit that is not finite is a rejection
  if (finite && phit <= p.phi0[b] + 1e-4 * alpha * p.slope[b]) {  // Armijo on the l1 merit: commit
    for (int j = lane; j < p.n; j += kWave) {
      const int64_t i = b * p.n + j;
      p.x[i]          = clip(p.x[i] + alpha * p.d[i], p.xl[j], p.xu[j]);
      const int br    = p.bound_row[j];
      const double zq = br >= 0 ? p.yqp[b * p.mq + p.m + br] : 0.0;
      p.z[i]          = p.z[i] + alpha * (zq - p.z[i]);
    }
    for (int r = lane; r < p.m; r += kWave) {
      const int64_t i = b * p.m + r;
      p.lambda[i]     = p.lambda[i] + alpha * (p.yqp[b * p.mq + r] - p.lambda[i]);
    }
    if (lane == 0) {
      const double mu = p.mu[b];
      p.mu[b]         = mu > p.mu_first ? mu / 4.0 : 0.0;
      p.iter[b]       = p.iter[b] + 1;
      p.phase[b]      = 0;
    }
  } else if (lane == 0) {
    const int h = p.halvings[b] + 1;
    if (h > 10) {  // the tenth halving was rejected too: the direction is no descent direction of the merit
      p.status[b] = kNlpUnknown;
      p.phase[b]  = 0;
    } else {
      p.halvings[b] = h;
      p.alpha[b]    = alpha / 2.0;
    }
  }
}

__global__ __launch_bounds__(kLaneBlock) void nlp_sqp_start_kernel(const NlpSqpDev p, const int64_t batch, const double *__restrict__ x,
                                                                   const double *__restrict__ lambda, const double *__restrict__ z)
{
  const int len     = p.n > p.mq ? p.n : p.mq;
  const int64_t idx = (int64_t)blockIdx.x * kLaneBlock + threadIdx.x;
  if (idx >= batch * len) return;
  const int64_t b = idx / len;
  const int j     = (int)(idx - b * len);
  if (j < p.n) {
    p.x[b * p.n + j] = x[b * p.n + j];
    p.z[b * p.n + j] = z ? z[b * p.n + j] : 0.0;
    p.d[b * p.n + j] = 0.0;
  }
  if (j < p.m) p.lambda[b * p.m + j] = lambda ? lambda[b * p.m + j] : 0.0;
  if (j < p.mq) p.yqp[b * p.mq + j] = 0.0;
  if (j == 0) {
    p.mu[b] = p.nu[b] = p.alpha[b] = 0.0;
    p.r_stat[b] = p.r_pri[b] = p.r_comp[b] = p.v1[b] = p.phi0[b] = p.slope[b] = p.dd[b] = p.dPd[b] = 0.0;
    p.status[b] = kNlpRunning;
    p.iter[b] = p.phase[b] = p.need[b] = p.halvings[b] = 0;
  }
}

unsigned lane_grid(int64_t lanes) { return (unsigned)((lanes + kLaneBlock - 1) / kLaneBlock); }

}  // namespace

hipError_t nlp_sqp_kkt_launch(const NlpSqpDev &p, int64_t batch, const double *df, const double *g, const double *dg_val, hipStream_t s)
{
  if (batch <= 0) return hipSuccess;
  nlp_sqp_kkt_kernel<<<dim3((unsigned)batch), dim3(kWave), 0, s>>>(p, batch, df, g, dg_val);
  return hipGetLastError();
}

hipError_t nlp_sqp_compact_launch(const int32_t *flag, int64_t batch, int32_t *list, int32_t *count, hipStream_t s)
{
  nlp_sqp_compact_kernel<<<dim3(1), dim3(kWave), 0, s>>>(flag, batch, list, count);
  return hipGetLastError();
}

hipError_t nlp_sqp_assemble_launch(const NlpSqpDev &p, const int32_t *list, int64_t count, const double *df, const double *g,
                                   const double *dg_val, const double *hess_val, double *Px, double *q, double *Ax, double *l, double *u,
                                   double *wx, double *wy, hipStream_t s)
{
  if (count <= 0) return hipSuccess;
  const int64_t per = (int64_t)p.nnzP + p.n + p.nnzA + 2 * (int64_t)p.mq + p.n + p.mq;
  nlp_sqp_assemble_kernel<<<dim3(lane_grid(count * per)), dim3(kLaneBlock), 0, s>>>(p, list, count, df, g, dg_val, hess_val, Px, q, Ax, l, u, wx, wy);
  return hipGetLastError();
}

hipError_t nlp_sqp_judge_launch(const NlpSqpDev &p, const int32_t *list, int64_t count, int rung, const double *f, const double *Px,
                                const double *q, const double *xs, const double *ys, const int32_t *code, hipStream_t s)
{
  if (count <= 0) return hipSuccess;
  nlp_sqp_judge_kernel<<<dim3((unsigned)count), dim3(kWave), 0, s>>>(p, list, count, rung, f, Px, q, xs, ys, code);
  return hipGetLastError();
}

hipError_t nlp_sqp_trial_launch(const NlpSqpDev &p, int64_t batch, double *x_trial, hipStream_t s)
{
  if (batch <= 0) return hipSuccess;
  nlp_sqp_trial_kernel<<<dim3(lane_grid(batch * p.n)), dim3(kLaneBlock), 0, s>>>(p, batch, x_trial);
  return hipGetLastError();
}

hipError_t nlp_sqp_accept_launch(const NlpSqpDev &p, int64_t batch, const double *f_trial, const double *g_trial, hipStream_t s)
{
  if (batch <= 0) return hipSuccess;
  nlp_sqp_accept_kernel<<<dim3((unsigned)batch), dim3(kWave), 0, s>>>(p, batch, f_trial, g_trial);
  return hipGetLastError();
}

hipError_t nlp_sqp_start_launch(const NlpSqpDev &p, int64_t batch, const double *x, const double *lambda, const double *z, hipStream_t s)
{
  if (batch <= 0) return hipSuccess;
  const int len = p.n > p.mq ? p.n : p.mq;
  nlp_sqp_start_kernel<<<dim3(lane_grid(batch * len)), dim3(kLaneBlock), 0, s>>>(p, batch, x, lambda, z);
  return hipGetLastError();
}

}  // namespace sfb
