// C-ABI of the swarm SQP solver (include/sfb.h): the pattern builder's entry and the opaque handle that owns the sparse QP
// plan, the QP arrays, the solver workspace and the agents' state.  The kernels are in nlp_sqp.hip, the law in DESIGN.md.
#include <hip/hip_runtime.h>

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

  // one allocation: [solver workspace | doubles | 32-bit integers], every part a multiple of 16 bytes from the start
  sfb::NlpSqpDev &D = h->dev;
  const size_t B = (size_t)batch, N = (size_t)n, M = (size_t)m, MQ = (size_t)mq, nnzP = (size_t)pt.nnzP, nnzJ = (size_t)pt.nnzJ, nnzA = nnzJ + pt.nb;
  const size_t ws_bytes = ((size_t)wsb + 15) / 16 * 16;
  const size_t shared_d = 2 * N + 2 * M;
  const size_t state_d  = B * (3 * N + M + MQ + 12);
  const size_t qp_d     = B * (nnzP + N + nnzA + 2 * MQ + 2 * (N + MQ));
  const size_t doubles  = (shared_d + state_d + qp_d + 1) / 2 * 2;
  const size_t ints     = 3 * nnzP + (N + 1) + 2 * nnzJ + (size_t)pt.nb + N + 5 * B + 4 * B + 4;
  if ((e = hipMalloc(reinterpret_cast<void **>(&h->mem), ws_bytes + doubles * 8 + ints * 4)) != hipSuccess) return drop(sfb::hip_fail(e, "hipMalloc(nlp_sqp)"));
  if ((e = hipHostMalloc(reinterpret_cast<void **>(&h->h_count), 16, hipHostMallocDefault)) != hipSuccess) return drop(sfb::hip_fail(e, "hipHostMalloc(nlp_sqp)"));
  h->ws     = h->mem;
  double *d = reinterpret_cast<double *>(h->mem + ws_bytes);
  double *dxl = d; d += N;
  double *dxu = d; d += N;
  double *dgl = d; d += M;
  double *dgu = d; d += M;
  const auto take = [&d](size_t count) { double *r = d; d += count; return r; };
  D.x = take(B * N); D.z = take(B * N); D.d = take(B * N); D.lambda = take(B * M); D.yqp = take(B * MQ);
  D.mu = take(B); D.nu = take(B); D.alpha = take(B); D.r_stat = take(B); D.r_pri = take(B); D.r_comp = take(B); D.v1 = take(B);
  D.phi0 = take(B); D.slope = take(B); D.dd = take(B); D.dPd = take(B);
  (void)take(B);
  h->Px = take(B * nnzP); h->q = take(B * N); h->Ax = take(B * nnzA); h->l = take(B * MQ); h->u = take(B * MQ);
  h->wx = take(B * N); h->wy = take(B * MQ); h->xs = take(B * N); h->ys = take(B * MQ);
  int32_t *i = reinterpret_cast<int32_t *>(h->mem + ws_bytes + doubles * 8);
  const auto upload = [&i, &e](const int32_t *src, size_t count) {
    int32_t *r = i;
    i += count;
    if (e == hipSuccess && count > 0) e = hipMemcpy(r, src, count * 4, hipMemcpyHostToDevice);
    return r;
  };
  D.P_row     = upload(pt.P_rowind.data(), nnzP);
  D.P_col     = upload(P_col.data(), nnzP);
  D.P_src     = upload(pt.P_src.data(), nnzP);
  D.Jc_colptr = upload(pt.Jc_colptr.data(), N + 1);
  D.Jc_row    = upload(pt.Jc_row.data(), nnzJ);
  D.Jc_pos    = upload(pt.Jc_pos.data(), nnzJ);
  D.bound_var = upload(pt.bound_var.data(), (size_t)pt.nb);
  D.bound_row = upload(pt.bound_row.data(), N);
  const auto itake = [&i](size_t count) { int32_t *r = i; i += count; return r; };
  D.status = itake(B); D.iter = itake(B); D.phase = itake(B); D.need = itake(B); D.halvings = itake(B);
  h->qiter = reinterpret_cast<uint32_t *>(itake(B)); h->qcode = itake(B); h->list = itake(B); h->searching = itake(B); h->count = itake(1);
  if (e == hipSuccess) e = hipMemcpy(dxl, xl, N * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dxu, xu, N * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess && M > 0) e = hipMemcpy(dgl, gl, M * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess && M > 0) e = hipMemcpy(dgu, gu, M * 8, hipMemcpyHostToDevice);
  // the state starts defined (all zero, nothing running) until sfb_nlp_sqp_set_start; so do the QP arrays the debug entry shows
  if (e == hipSuccess) e = hipMemset(h->mem + ws_bytes + shared_d * 8, 0, (doubles - shared_d) * 8);
  if (e == hipSuccess) e = hipMemset(D.status, 0, (9 * B + 1) * 4);
  if (e != hipSuccess) return drop(sfb::hip_fail(e, "sfb_nlp_sqp_create"));
  D.xl = dxl; D.xu = dxu; D.gl = dgl; D.gu = dgu;
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
sfb_status host_stage(sfb_nlp_sqp *h)
{
  if (h->stage || h->batch == 0) return SFB_OK;
  const sfb::NlpSqpDev &D = h->dev;
  const size_t per = 1 + (size_t)D.n + D.m + D.nnzJ + D.nnzH;
  const hipError_t e = hipMalloc(reinterpret_cast<void **>(&h->stage), (size_t)h->batch * per * 8);
  return e == hipSuccess ? SFB_OK : sfb::hip_fail(e, "hipMalloc(nlp_sqp host staging)");
}
sfb_status copy_to_device(double *dst, const double *src, size_t count)
{
  if (!count || !src) return SFB_OK;
  const hipError_t e = hipMemcpy(dst, src, count * 8, hipMemcpyHostToDevice);
  return e == hipSuccess ? SFB_OK : sfb::hip_fail(e, "hipMemcpy(host to device)");
}
sfb_status copy_to_host_bytes(void *dst, const void *src, size_t bytes)
{
  if (!bytes || !dst) return SFB_OK;
  const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  return e == hipSuccess ? SFB_OK : sfb::hip_fail(e, "hipMemcpy(device to host)");
}
}  // namespace

sfb_status sfb_nlp_sqp_set_start_host(sfb_nlp_sqp *h, const double *x, const double *lambda, const double *z)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (h->batch > 0 && !x) return sfb::fail(SFB_ERR_INVALID_ARG, "x is NULL");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  if (sfb_status st = host_stage(h); st != SFB_OK) return st;
  const size_t B = (size_t)h->batch, N = (size_t)h->dev.n, M = (size_t)h->dev.m;
  double *dx = h->stage, *dl = dx + B * N, *dz = dl + B * M;  // (2 n + m <= 1 + n + m + nnzJ + nnzH: every diagonal is stored)
  sfb_status st = copy_to_device(dx, x, B * N);
  if (st == SFB_OK) st = copy_to_device(dl, lambda, B * M);
  if (st == SFB_OK) st = copy_to_device(dz, z, B * N);
  if (st != SFB_OK) return st;
  st = sfb_nlp_sqp_set_start(h, dx, lambda ? dl : nullptr, z ? dz : nullptr, nullptr);
  if (st != SFB_OK) return st;
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
  if (sfb_status st = host_stage(h); st != SFB_OK) return st;
  const size_t B = (size_t)h->batch;
  const sfb::NlpSqpDev &D = h->dev;
  double *d_f = h->stage, *d_df = d_f + B, *d_g = d_df + B * D.n, *d_dg = d_g + B * D.m, *d_h = d_dg + B * (size_t)D.nnzJ;
  sfb_status st = copy_to_device(d_f, f, B);
  if (st == SFB_OK) st = copy_to_device(d_df, df, B * D.n);
  if (st == SFB_OK) st = copy_to_device(d_g, g, B * D.m);
  if (st == SFB_OK) st = copy_to_device(d_dg, dg_val, B * (size_t)D.nnzJ);
  if (st == SFB_OK) st = copy_to_device(d_h, hess_val, B * (size_t)D.nnzH);
  if (st != SFB_OK) return st;
  return sfb_nlp_sqp_direction(h, d_f, d_df, d_g, d_dg, d_h, active, nullptr);
}

sfb_status sfb_nlp_sqp_trial_host(sfb_nlp_sqp *h, double *x_trial)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (h->batch > 0 && !x_trial) return sfb::fail(SFB_ERR_INVALID_ARG, "x_trial is NULL");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  if (sfb_status st = host_stage(h); st != SFB_OK) return st;
  if (sfb_status st = sfb_nlp_sqp_trial(h, h->stage, nullptr); st != SFB_OK) return st;
  return copy_to_host_bytes(x_trial, h->stage, (size_t)h->batch * h->dev.n * 8);
}

sfb_status sfb_nlp_sqp_accept_host(sfb_nlp_sqp *h, const double *f_trial, const double *g_trial, int64_t *searching)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (h->batch > 0 && (!f_trial || (h->dev.m > 0 && !g_trial))) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL f_trial / g_trial");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  if (sfb_status st = host_stage(h); st != SFB_OK) return st;
  const size_t B = (size_t)h->batch;
  double *d_f = h->stage, *d_g = d_f + B;
  sfb_status st = copy_to_device(d_f, f_trial, B);
  if (st == SFB_OK) st = copy_to_device(d_g, g_trial, B * h->dev.m);
  if (st != SFB_OK) return st;
  return sfb_nlp_sqp_accept(h, d_f, d_g, searching, nullptr);
}

sfb_status sfb_nlp_sqp_state_host(sfb_nlp_sqp *h, double *x, double *lambda, double *z, int32_t *status, int32_t *iter, double *r_stat,
                                  double *r_pri, double *r_comp, double *mu, double *alpha, double *nu)
{
  if (!h) return sfb::fail(SFB_ERR_INVALID_ARG, "handle is NULL");
  if (sfb_status st = check_device(h); st != SFB_OK) return st;
  const size_t B = (size_t)h->batch;
  const sfb::NlpSqpDev &D = h->dev;
  sfb_status st = copy_to_host_bytes(x, D.x, (B * D.n) * 8);
  if (st == SFB_OK) st = copy_to_host_bytes(lambda, D.lambda, (B * D.m) * 8);
  if (st == SFB_OK) st = copy_to_host_bytes(z, D.z, (B * D.n) * 8);
  if (st == SFB_OK) st = copy_to_host_bytes(status, D.status, (B) * 4);
  if (st == SFB_OK) st = copy_to_host_bytes(iter, D.iter, (B) * 4);
  if (st == SFB_OK) st = copy_to_host_bytes(r_stat, D.r_stat, (B) * 8);
  if (st == SFB_OK) st = copy_to_host_bytes(r_pri, D.r_pri, (B) * 8);
  if (st == SFB_OK) st = copy_to_host_bytes(r_comp, D.r_comp, (B) * 8);
  if (st == SFB_OK) st = copy_to_host_bytes(mu, D.mu, (B) * 8);
  if (st == SFB_OK) st = copy_to_host_bytes(alpha, D.alpha, (B) * 8);
  if (st == SFB_OK) st = copy_to_host_bytes(nu, D.nu, (B) * 8);
  return st;
}

}  // extern "C"
