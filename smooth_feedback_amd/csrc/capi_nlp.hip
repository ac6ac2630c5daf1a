// C-ABI of the swarm SQP solver (include/sfb.h): the pattern builder's entry and the opaque handle that owns the sparse QP
// plan, the QP arrays, the solver workspace and the agents' state.  The kernels are in nlp_sqp.hip, the law in DESIGN.md.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/sfb.h"
#include "capi_common.h"
#include "nlp_sqp_kernel.h"
#include "nlp_sqp_plan.h"

struct sfb_nlp_sqp {
  sfb::NlpSqpPattern pat;
  sfb::NlpSqpDev dev{};
  sfb_nlp_sqp_params prm{};
  sfb_sparse_qp_plan *plan = nullptr;
  int64_t batch = 0;
  int devid     = 0;
  char *mem     = nullptr;
  // the QP of a rung, compacted: slot k belongs to agent list[k]
  double *Px = nullptr, *q = nullptr, *Ax = nullptr, *l = nullptr, *u = nullptr, *wx = nullptr, *wy = nullptr, *xs = nullptr, *ys = nullptr;
  void *ws         = nullptr;
  uint32_t *qiter  = nullptr;
  int32_t *qcode = nullptr, *list = nullptr, *count = nullptr;
  int32_t *searching = nullptr;  // the list behind the count of agents in line search (kept apart: `list` stays the last rung's)
  int32_t *h_count = nullptr;  // pinned: the one number a rung brings back
  double *stage    = nullptr;  // device staging of the host-pointer entries, made by the first of them (per agent: the arrays of direction)
};

namespace {

sfb_status check_device(const sfb_nlp_sqp *h)
{
  int dev = -1;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return sfb::hip_fail(e, "hipGetDevice");
  if (dev != h->devid) return sfb::fail(SFB_ERR_INVALID_ARG, "the solver was created on another HIP device than the current one");
  return SFB_OK;
}

// how many agents have flag != 0, through the compaction kernel; waits for the stream
sfb_status count_flags(sfb_nlp_sqp *h, const int32_t *flag, int32_t *list, hipStream_t s, int64_t *out)
{
  hipError_t e = sfb::nlp_sqp_compact_launch(flag, h->batch, list, h->count, s);
  if (e == hipSuccess) e = hipMemcpyAsync(h->h_count, h->count, sizeof(int32_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return sfb::hip_fail(e, "nlp_sqp compaction");
  *out = *h->h_count;
  return SFB_OK;
}

}  // namespace

extern "C" {

void sfb_nlp_sqp_params_default(sfb_nlp_sqp_params *p)
{
  if (!p) return;
  p->tol      = 1e-6;
  p->max_iter = 50;
  p->kappa    = 1e-8;
  p->mu_first = 1e-4;
  p->mu_grow  = 8.0;
  p->mu_max   = 1e4;
  sfb_qp_params_default(&p->qp);
  // an SQP step is as good as its QP: tighter than the MPC defaults, and bounded (a shifted-out QP may be non-convex)
  p->qp.eps_abs = p->qp.eps_rel = 1e-9f;
  p->qp.max_iter                = 10000;
}

sfb_status sfb_nlp_sqp_qp_pattern(int n, int m, const int32_t *J_rowptr, const int32_t *J_colind, const int32_t *H_colptr,
                                  const int32_t *H_rowind, const double *xl, const double *xu, const double *gl, const double *gu,
                                  int32_t *A_rowptr, int32_t *A_colind, int32_t *P_colptr, int32_t *P_rowind, int32_t *P_src, int32_t *P_diag,
                                  int32_t *Jc_colptr, int32_t *Jc_row, int32_t *Jc_pos, int32_t *bound_var, int64_t *nb)
{
  if (!nb) return sfb::fail(SFB_ERR_INVALID_ARG, "nb is NULL");
  sfb::NlpSqpPattern o;
  const char *msg = "";
  if (!sfb::build_nlp_sqp_pattern(n, m, J_rowptr, J_colind, H_colptr, H_rowind, xl, xu, gl, gu, o, &msg)) return sfb::fail(SFB_ERR_INVALID_ARG, msg);
  *nb = o.nb;
  const bool none = !A_rowptr && !A_colind && !P_colptr && !P_rowind && !P_src && !P_diag && !Jc_colptr && !Jc_row && !Jc_pos && !bound_var;
  if (none) return SFB_OK;
  if (!A_rowptr || !P_colptr || !P_rowind || !P_src || !P_diag || !Jc_colptr || (!A_colind && !o.A_colind.empty()) || ((!Jc_row || !Jc_pos) && o.nnzJ > 0) || (!bound_var && o.nb > 0))
    return sfb::fail(SFB_ERR_INVALID_ARG, "the output arrays: all or none");
  const auto put = [](int32_t *dst, const std::vector<int32_t> &v) { if (!v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(int32_t)); };
  put(A_rowptr, o.A_rowptr); put(A_colind, o.A_colind); put(P_colptr, o.P_colptr); put(P_rowind, o.P_rowind); put(P_src, o.P_src);
  put(P_diag, o.P_diag); put(Jc_colptr, o.Jc_colptr);
  put(Jc_row, o.Jc_row); put(Jc_pos, o.Jc_pos); put(bound_var, o.bound_var);
  return SFB_OK;
}

sfb_status sfb_nlp_sqp_create(int n, int m, const int32_t *J_rowptr, const int32_t *J_colind, const int32_t *H_colptr,
                              const int32_t *H_rowind, const double *xl, const double *xu, const double *gl, const double *gu,
                              int64_t batch, const sfb_nlp_sqp_params *params, const int32_t *stage, sfb_nlp_sqp **out)
{
  if (!out) return sfb::fail(SFB_ERR_INVALID_ARG, "handle out-pointer is NULL");
  *out = nullptr;
  auto *h = new sfb_nlp_sqp;
  const auto drop = [&](sfb_status st) { sfb_nlp_sqp_destroy(h); return st; };
  const char *msg = "";
  if (!sfb::build_nlp_sqp_pattern(n, m, J_rowptr, J_colind, H_colptr, H_rowind, xl, xu, gl, gu, h->pat, &msg)) return drop(sfb::fail(SFB_ERR_INVALID_ARG, msg));
  if (batch < 0 || batch > 0x7FFFFFFFll) return drop(sfb::fail(SFB_ERR_INVALID_ARG, "batch must be in [0, 2^31-1]"));
  if (params) h->prm = *params; else sfb_nlp_sqp_params_default(&h->prm);
  const sfb_nlp_sqp_params &P = h->prm;
  if (!(P.tol >= 0.0) || P.max_iter < 0 || P.max_iter > 0x7FFFFFFFll || !(P.kappa >= 0.0) || !(P.mu_first > 0.0) || !(P.mu_grow > 1.0) ||
      !(P.mu_max >= 0.0) || !std::isfinite(P.mu_max) || !std::isfinite(P.mu_grow))
    return drop(sfb::fail(SFB_ERR_INVALID_ARG, "params: tol, kappa >= 0, max_iter >= 0, mu_first > 0, mu_grow > 1, 0 <= mu_max < inf"));
  const sfb::NlpSqpPattern &pt = h->pat;
  const int mq = m + pt.nb;
  if (mq < 1) return drop(sfb::fail(SFB_ERR_UNSUPPORTED, "a problem without constraints and without bounds has no QP rows: the sparse solver needs one"));
  sfb_status st = sfb_sparse_qp_plan_create_staged(n, mq, pt.P_colptr.data(), pt.P_rowind.data(), pt.A_rowptr.data(), pt.A_colind.data(), 1, nullptr, stage, &h->plan);
  if (st != SFB_OK) return drop(st);
  st = sfb::require_device();
  if (st != SFB_OK) return drop(st);
  h->batch = batch;
  hipError_t e = hipGetDevice(&h->devid);
  if (e != hipSuccess) return drop(sfb::hip_fail(e, "hipGetDevice"));

  std::vector<int32_t> P_col(pt.nnzP);
  for (int c = 0; c < n; ++c)
    for (int p = pt.P_colptr[c]; p < pt.P_colptr[c + 1]; ++p) P_col[p] = c;
  int64_t wsb = 0;
  if (batch > 0 && (st = sfb_sparse_qp_plan_workspace_bytes(h->plan, batch, &wsb)) != SFB_OK) return drop(st);

  // One allocation: [solver workspace | bounds and the agents' state | the compacted QP arrays | 32-bit integers], every
  // region at a multiple of 16 bytes.  The regions' sizes and every pointer come from these declarations.
  sfb::NlpSqpDev &D = h->dev;
  const size_t B = (size_t)batch, N = (size_t)n, M = (size_t)m, MQ = (size_t)mq, nnzP = (size_t)pt.nnzP, nnzJ = (size_t)pt.nnzJ, nnzA = nnzJ + pt.nb;
  using S = sfb::Staging;
  S state, ints;
  sfb::DeviceArena qp;
  state.add(&D.xl, N, S::In, xl); state.add(&D.xu, N, S::In, xu); state.add(&D.gl, M, S::In, gl); state.add(&D.gu, M, S::In, gu);
  state.add(&D.x, B * N); state.add(&D.z, B * N); state.add(&D.d, B * N); state.add(&D.lambda, B * M); state.add(&D.yqp, B * MQ);
  state.add(&D.mu, B); state.add(&D.nu, B); state.add(&D.alpha, B); state.add(&D.r_stat, B); state.add(&D.r_pri, B); state.add(&D.r_comp, B);
  state.add(&D.v1, B); state.add(&D.phi0, B); state.add(&D.slope, B); state.add(&D.dd, B); state.add(&D.dPd, B);  // (the debug entry's five sums)
  qp.add(&h->Px, B * nnzP); qp.add(&h->q, B * N); qp.add(&h->Ax, B * nnzA); qp.add(&h->l, B * MQ); qp.add(&h->u, B * MQ);
  qp.add(&h->wx, B * N); qp.add(&h->wy, B * MQ); qp.add(&h->xs, B * N); qp.add(&h->ys, B * MQ);
  ints.add(&D.P_row, nnzP, S::In, pt.P_rowind.data()); ints.add(&D.P_col, nnzP, S::In, P_col.data()); ints.add(&D.P_src, nnzP, S::In, pt.P_src.data());
  ints.add(&D.Jc_colptr, N + 1, S::In, pt.Jc_colptr.data()); ints.add(&D.Jc_row, nnzJ, S::In, pt.Jc_row.data());
  ints.add(&D.Jc_pos, nnzJ, S::In, pt.Jc_pos.data()); ints.add(&D.bound_var, (size_t)pt.nb, S::In, pt.bound_var.data());
  ints.add(&D.bound_row, N, S::In, pt.bound_row.data());
  ints.add(&D.status, B); ints.add(&D.iter, B); ints.add(&D.phase, B); ints.add(&D.need, B); ints.add(&D.halvings, B);
  ints.add(&h->qiter, B); ints.add(&h->qcode, B); ints.add(&h->list, B); ints.add(&h->searching, B); ints.add(&h->count, 1);
  const auto next16 = [](size_t at) { return (at + 15) / 16 * 16; };
  const size_t state_at = next16((size_t)wsb), qp_at = next16(state_at + state.bytes()), ints_at = next16(qp_at + qp.bytes());
  if ((e = hipMalloc(reinterpret_cast<void **>(&h->mem), ints_at + ints.bytes())) != hipSuccess) return drop(sfb::hip_fail(e, "hipMalloc(nlp_sqp)"));
  if ((e = hipHostMalloc(reinterpret_cast<void **>(&h->h_count), 16, hipHostMallocDefault)) != hipSuccess) return drop(sfb::hip_fail(e, "hipHostMalloc(nlp_sqp)"));
  h->ws = h->mem;
  if (!state.bind(h->mem + state_at) || !qp.bind(h->mem + qp_at) || !ints.bind(h->mem + ints_at))
    return drop(sfb::fail(SFB_ERR_UNSUPPORTED, "more staged arrays than the table holds"));
  if ((e = state.upload()) == hipSuccess) e = ints.upload();
  // the state starts defined (all zero, nothing running) until sfb_nlp_sqp_set_start; so do the QP arrays the debug entry shows
  const char *qp_end = h->mem + qp_at + qp.bytes(), *ints_end = h->mem + ints_at + ints.bytes();
  if (e == hipSuccess) e = hipMemset(D.x, 0, (size_t)(qp_end - reinterpret_cast<const char *>(D.x)));
  if (e == hipSuccess) e = hipMemset(D.status, 0, (size_t)(ints_end - reinterpret_cast<const char *>(D.status)));
  if (e != hipSuccess) return drop(sfb::hip_fail(e, "sfb_nlp_sqp_create"));
  D.n = n; D.m = m; D.nb = pt.nb; D.mq = mq; D.nnzJ = pt.nnzJ; D.nnzH = pt.nnzH; D.nnzP = pt.nnzP; D.nnzA = (int)nnzA;
  D.max_iter = (int)P.max_iter;
  D.tol = P.tol; D.kappa = P.kappa; D.mu_first = P.mu_first; D.mu_grow = P.mu_grow; D.mu_max = P.mu_max;
  *out = h;
  return SFB_OK;
}

void sfb_nlp_sqp_destroy(sfb_nlp_sqp *h)
{
  if (!h) return;
  if (h->h_count) (void)hipHostFree(h->h_count);
  if (h->stage) (void)hipFree(h->stage);
  if (h->mem) (void)hipFree(h->mem);
  if (h->plan) sfb_sparse_qp_plan_destroy(h->plan);
  delete h;
}

sfb_status sfb_nlp_sqp_info(const sfb_nlp_sqp *h, int64_t *batch, int32_t *n, int32_t *m, int32_t *nb, int64_t *nnzH, int64_t *nnzP, int64_t *nnzA)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (batch) *batch = h->batch;
  if (n) *n = h->dev.n;
  if (m) *m = h->dev.m;
  if (nb) *nb = h->dev.nb;
  if (nnzH) *nnzH = h->dev.nnzH;
  if (nnzP) *nnzP = h->dev.nnzP;
  if (nnzA) *nnzA = h->dev.nnzA;
  return SFB_OK;
}

sfb_status sfb_nlp_sqp_set_start(sfb_nlp_sqp *h, const double *x, const double *lambda, const double *z, void *stream)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (h->batch > 0 && !x) return sfb::fail(SFB_ERR_INVALID_ARG, "x is NULL");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  const hipError_t e = sfb::nlp_sqp_start_launch(h->dev, h->batch, x, lambda, z, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? SFB_OK : sfb::hip_fail(e, "nlp_sqp_start_kernel launch");
}

sfb_status sfb_nlp_sqp_direction(sfb_nlp_sqp *h, const double *f, const double *df, const double *g, const double *dg_val,
                                 const double *hess_val, int64_t *active, void *stream)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (h->batch > 0 && (!f || !df || !hess_val || (h->dev.m > 0 && !g) || (h->dev.nnzJ > 0 && !dg_val)))
    return sfb::fail(SFB_ERR_INVALID_ARG, "NULL f / df / g / dg_val / hess_val");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  if (active) *active = 0;
  if (h->batch == 0) return SFB_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e  = sfb::nlp_sqp_kkt_launch(h->dev, h->batch, df, g, dg_val, s);
  if (e != hipSuccess) return sfb::hip_fail(e, "nlp_sqp_kkt_kernel launch");
  // the shift ladder: every rung re-solves the rejected agents only.  mu grows by mu_grow > 1 from mu_first to beyond mu_max,
  // so the number of rungs is bounded by the parameters.
  for (int rung = 0;; ++rung) {
    int64_t count = 0;
    if (sfb_status st = count_flags(h, h->dev.need, h->list, s, &count); st != SFB_OK) return st;
    if (count == 0) break;
    if ((e = sfb::nlp_sqp_assemble_launch(h->dev, h->list, count, df, g, dg_val, hess_val, h->Px, h->q, h->Ax, h->l, h->u, h->wx, h->wy, s)) != hipSuccess)
      return sfb::hip_fail(e, "nlp_sqp_assemble_kernel launch");
    if (sfb_status st = sfb_sparse_qp_solve_batch(h->plan, &h->prm.qp, count, h->Px, h->q, h->Ax, h->l, h->u, h->wx, h->wy, h->xs, h->ys, nullptr,
                                                  h->qiter, h->qcode, h->ws, stream);
        st != SFB_OK)
      return st;
    if ((e = sfb::nlp_sqp_judge_launch(h->dev, h->list, count, rung, f, h->Px, h->q, h->xs, h->ys, h->qcode, s)) != hipSuccess)
      return sfb::hip_fail(e, "nlp_sqp_judge_kernel launch");
  }
  int64_t searching = 0;
  if (sfb_status st = count_flags(h, h->dev.phase, h->searching, s, &searching); st != SFB_OK) return st;
  if (active) *active = searching;
  return SFB_OK;
}

sfb_status sfb_nlp_sqp_trial(sfb_nlp_sqp *h, double *x_trial, void *stream)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (h->batch > 0 && !x_trial) return sfb::fail(SFB_ERR_INVALID_ARG, "x_trial is NULL");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  const hipError_t e = sfb::nlp_sqp_trial_launch(h->dev, h->batch, x_trial, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? SFB_OK : sfb::hip_fail(e, "nlp_sqp_trial_kernel launch");
}

sfb_status sfb_nlp_sqp_accept(sfb_nlp_sqp *h, const double *f_trial, const double *g_trial, int64_t *searching, void *stream)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (h->batch > 0 && (!f_trial || (h->dev.m > 0 && !g_trial))) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL f_trial / g_trial");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  if (searching) *searching = 0;
  if (h->batch == 0) return SFB_OK;
  hipStream_t s      = static_cast<hipStream_t>(stream);
  const hipError_t e = sfb::nlp_sqp_accept_launch(h->dev, h->batch, f_trial, g_trial, s);
  if (e != hipSuccess) return sfb::hip_fail(e, "nlp_sqp_accept_kernel launch");
  int64_t count = 0;
  if (sfb_status st = count_flags(h, h->dev.phase, h->searching, s, &count); st != SFB_OK) return st;
  if (searching) *searching = count;
  return SFB_OK;
}

sfb_status sfb_nlp_sqp_state(sfb_nlp_sqp *h, const double **x, const double **lambda, const double **z, const int32_t **status,
                             const int32_t **iter, const double **r_stat, const double **r_pri, const double **r_comp, const double **mu,
                             const double **alpha, const double **nu)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  const sfb::NlpSqpDev &D = h->dev;
  if (x) *x = D.x;
  if (lambda) *lambda = D.lambda;
  if (z) *z = D.z;
  if (status) *status = D.status;
  if (iter) *iter = D.iter;
  if (r_stat) *r_stat = D.r_stat;
  if (r_pri) *r_pri = D.r_pri;
  if (r_comp) *r_comp = D.r_comp;
  if (mu) *mu = D.mu;
  if (alpha) *alpha = D.alpha;
  if (nu) *nu = D.nu;
  return SFB_OK;
}

sfb_status sfb_nlp_sqp_debug_buffers(sfb_nlp_sqp *h, const double **Px, const double **q, const double **Ax, const double **l,
                                     const double **u, const double **d, const double **y, const int32_t **code, const uint32_t **iter,
                                     const int32_t **list, const double **sums)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (Px) *Px = h->Px;
  if (q) *q = h->q;
  if (Ax) *Ax = h->Ax;
  if (l) *l = h->l;
  if (u) *u = h->u;
  if (d) *d = h->xs;
  if (y) *y = h->ys;
  if (code) *code = h->qcode;
  if (iter) *iter = h->qiter;
  if (list) *list = h->list;
  if (sums) *sums = h->dev.v1;
  return SFB_OK;
}

// ---- host-pointer variants (synchronous, null stream): what a host front such as solve_nlp_sqp (nlp_solver.hpp) stages through ----
namespace {
// The staged arrays of the host-pointer entries: three layouts of the one buffer the handle keeps, a call at a time.  They are
// declared here, so that the buffer's size and every pointer in it come from the same lists.  (trial's output, [batch][n], is
// the first array of the first layout.)
struct HostStage {
  sfb::Staging s;
  double *a[5];
};
using S = sfb::Staging;
void declare_start(const sfb_nlp_sqp *h, HostStage &g, const double *x, const double *lambda, const double *z)
{
  const size_t B = (size_t)h->batch, N = (size_t)h->dev.n, M = (size_t)h->dev.m;
  g.s.add(&g.a[0], B * N, S::In, x); g.s.add(&g.a[1], B * M, S::In, lambda); g.s.add(&g.a[2], B * N, S::In, z);
}
void declare_direction(const sfb_nlp_sqp *h, HostStage &g, const double *f, const double *df, const double *gv, const double *dg_val, const double *hess_val)
{
  const size_t B = (size_t)h->batch;
  const sfb::NlpSqpDev &D = h->dev;
  g.s.add(&g.a[0], B, S::In, f); g.s.add(&g.a[1], B * D.n, S::In, df); g.s.add(&g.a[2], B * D.m, S::In, gv);
  g.s.add(&g.a[3], B * D.nnzJ, S::In, dg_val); g.s.add(&g.a[4], B * D.nnzH, S::In, hess_val);
}
void declare_accept(const sfb_nlp_sqp *h, HostStage &g, const double *f_trial, const double *g_trial)
{
  const size_t B = (size_t)h->batch;
  g.s.add(&g.a[0], B, S::In, f_trial); g.s.add(&g.a[1], B * h->dev.m, S::In, g_trial);
}
// g's arrays in the handle's staging (made by the first host entry, large enough for every layout), the inputs uploaded
sfb_status host_stage(sfb_nlp_sqp *h, HostStage &g)
{
  if (!h->stage && h->batch > 0) {
    HostStage start, direction, accept;
    declare_start(h, start, nullptr, nullptr, nullptr);
    declare_direction(h, direction, nullptr, nullptr, nullptr, nullptr, nullptr);
    declare_accept(h, accept, nullptr, nullptr);
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&h->stage), std::max({start.s.bytes(), direction.s.bytes(), accept.s.bytes()}));
    if (e != hipSuccess) return sfb::hip_fail(e, "hipMalloc(nlp_sqp host staging)");
  }
  g.s.bind(h->stage);
  const hipError_t e = g.s.upload();
  return e == hipSuccess ? SFB_OK : sfb::hip_fail(e, "hipMemcpy(host to device)");
}
}  // namespace

sfb_status sfb_nlp_sqp_set_start_host(sfb_nlp_sqp *h, const double *x, const double *lambda, const double *z)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (h->batch > 0 && !x) return sfb::fail(SFB_ERR_INVALID_ARG, "x is NULL");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  HostStage g;
  declare_start(h, g, x, lambda, z);
  if (sfb_status st = host_stage(h, g); st != SFB_OK) return st;
  if (sfb_status st = sfb_nlp_sqp_set_start(h, g.a[0], lambda ? g.a[1] : nullptr, z ? g.a[2] : nullptr, nullptr); st != SFB_OK) return st;
  const hipError_t e = hipStreamSynchronize(nullptr);  // the staging is reused by the next call
  return e == hipSuccess ? SFB_OK : sfb::hip_fail(e, "hipStreamSynchronize");
}

sfb_status sfb_nlp_sqp_direction_host(sfb_nlp_sqp *h, const double *f, const double *df, const double *g, const double *dg_val,
                                      const double *hess_val, int64_t *active)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (h->batch > 0 && (!f || !df || !hess_val || (h->dev.m > 0 && !g) || (h->dev.nnzJ > 0 && !dg_val)))
    return sfb::fail(SFB_ERR_INVALID_ARG, "NULL f / df / g / dg_val / hess_val");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  HostStage s;
  declare_direction(h, s, f, df, g, dg_val, hess_val);
  if (sfb_status st = host_stage(h, s); st != SFB_OK) return st;
  return sfb_nlp_sqp_direction(h, s.a[0], s.a[1], s.a[2], s.a[3], s.a[4], active, nullptr);
}

sfb_status sfb_nlp_sqp_trial_host(sfb_nlp_sqp *h, double *x_trial)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (h->batch > 0 && !x_trial) return sfb::fail(SFB_ERR_INVALID_ARG, "x_trial is NULL");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  HostStage g;
  g.s.add(&g.a[0], (size_t)h->batch * h->dev.n, S::Out, x_trial);
  if (sfb_status st = host_stage(h, g); st != SFB_OK) return st;
  if (sfb_status st = sfb_nlp_sqp_trial(h, g.a[0], nullptr); st != SFB_OK) return st;
  const hipError_t e = g.s.download();
  return e == hipSuccess ? SFB_OK : sfb::hip_fail(e, "hipMemcpy(device to host)");
}

sfb_status sfb_nlp_sqp_accept_host(sfb_nlp_sqp *h, const double *f_trial, const double *g_trial, int64_t *searching)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (h->batch > 0 && (!f_trial || (h->dev.m > 0 && !g_trial))) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL f_trial / g_trial");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  HostStage g;
  declare_accept(h, g, f_trial, g_trial);
  if (sfb_status st = host_stage(h, g); st != SFB_OK) return st;
  return sfb_nlp_sqp_accept(h, g.a[0], g.a[1], searching, nullptr);
}

sfb_status sfb_nlp_sqp_state_host(sfb_nlp_sqp *h, double *x, double *lambda, double *z, int32_t *status, int32_t *iter, double *r_stat,
                                  double *r_pri, double *r_comp, double *mu, double *alpha, double *nu)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  const size_t B = (size_t)h->batch;
  const sfb::NlpSqpDev &D = h->dev;
  const struct { void *host; const void *dev; size_t bytes; } rows[] = {
    {x, D.x, B * D.n * 8}, {lambda, D.lambda, B * D.m * 8}, {z, D.z, B * D.n * 8}, {status, D.status, B * 4}, {iter, D.iter, B * 4},
    {r_stat, D.r_stat, B * 8}, {r_pri, D.r_pri, B * 8}, {r_comp, D.r_comp, B * 8}, {mu, D.mu, B * 8}, {alpha, D.alpha, B * 8}, {nu, D.nu, B * 8}};
  for (const auto &r : rows) {
    if (!r.bytes || !r.host) continue;
    const hipError_t e = hipMemcpy(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return sfb::hip_fail(e, "hipMemcpy(device to host)");
  }
  return SFB_OK;
}

}  // extern "C"
