// C-ABI shim (include/sfb.h) over the HIP kernels.  No CPU fallback: every compute entry point
// needs a HIP device and fails with SFB_ERR_NO_DEVICE / SFB_ERR_HIP otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "knobs.h"
#include "../../include/sfb.h"
#include "capi_common.h"
#include "qp_dense_kernel.h"
#include "stream_scratch.h"

namespace sfb {

namespace { thread_local std::string g_last_error; }

sfb_status fail(sfb_status st, const std::string &msg)
{
  g_last_error = msg;
  return st;
}

sfb_status hip_fail(hipError_t e, const char *what)
{
  // clear the sticky error so that later calls report their own failure
  (void)hipGetLastError();
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver)
    return fail(SFB_ERR_NO_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
  return fail(SFB_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

sfb_status require_device()
{
  int cnt       = 0;
  hipError_t e  = hipGetDeviceCount(&cnt);
  if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
  if (cnt <= 0) return fail(SFB_ERR_NO_DEVICE, "no HIP device visible; the sfb library has no CPU fallback");
  return SFB_OK;
}

void verbose_report(const char *what, int64_t batch, int n, int m, double h2d_ms, double solve_ms, double d2h_ms,
                    const int32_t *code, const uint32_t *iter)
{
  static const char *names[7] = {"Optimal", "PolishFailed", "PrimalInfeasible", "DualInfeasible", "MaxIterations", "MaxTime", "Unknown"};
  long long hist[7] = {0, 0, 0, 0, 0, 0, 0};
  uint32_t imin = 0xFFFFFFFFu, imax = 0;
  double isum = 0.0;
  for (int64_t b = 0; b < batch; ++b) {
    if (code[b] >= 0 && code[b] < 7) hist[code[b]]++;
    if (iter) { imin = std::min(imin, iter[b]); imax = std::max(imax, iter[b]); isum += iter[b]; }
  }
  std::printf("[sfb] %s: %lld problem(s), n = %d, m = %d\n", what, (long long)batch, n, m);
  if (h2d_ms < 0.0)  // a sharded call: the shards' uploads, solves and downloads overlap -- one wall-clock figure for the call
    std::printf("[sfb]   time: %.3f ms for the whole call (upload, solve on the devices, download; the shards run side by side)\n", solve_ms);
  else
    std::printf("[sfb]   time: upload %.3f ms | solve on device (scaling, factorisation, ADMM, polish) %.3f ms | download %.3f ms\n",
                h2d_ms, solve_ms, d2h_ms);
  std::printf("[sfb]   status:");
  for (int c = 0; c < 7; ++c)
    if (hist[c]) std::printf(" %s %lld", names[c], hist[c]);
  if (iter && batch > 0) std::printf("\n[sfb]   iterations: min %u, mean %.1f, max %u", imin, isum / (double)batch, imax);
  std::printf("\n");
  std::fflush(stdout);
}

// The reference's closing summary of a verbose solve (qp_solver.hpp:550-565), from the per-phase times of the device
// (phase_us: scaling + pre-check | matrix filling | factorisation | iteration | polish | un-scale and report, microseconds).
// Its "Total time" runs from t0 (:376, after the scaling) to the end of the polish; the two parts outside are added as lines.
void verbose_summary(int32_t code, uint32_t iter, const double *phase_us)
{
  std::printf("QP solver summary:\n");
  std::printf("Result %d\n", (int)code);
  std::printf("%-25s%10lld\n", "Iterations", (long long)iter - 1);  // (the reference prints iter - 1, :556)
  std::printf("%-26s%10.0f\n", "Total time (\xC2\xB5s)", phase_us[1] + phase_us[2] + phase_us[3] + phase_us[4]);
  std::printf("%-25s%10.0f\n", "  Matrix filling", phase_us[1]);
  std::printf("%-25s%10.0f\n", "  Factorization", phase_us[2]);
  std::printf("%-25s%10.0f\n", "  Iteration", phase_us[3]);
  std::printf("%-25s%10.0f\n", "  Polish", phase_us[4]);
  std::printf("%-25s%10.0f\n", "(before t0: scaling)", phase_us[0]);
  std::printf("%-25s%10.0f\n", "(after: un-scale, report)", phase_us[5]);
  std::printf("=============================================================\n");
  std::fflush(stdout);
}

void verbose_table(const char *kind, int n, int m, const double *trace, int rows, const char *note)
{
  std::printf("========================= QP Solver =========================\n");
  std::printf("Solving %s QP with n=%d, m=%d\n", kind, n, m);
  if (note) std::printf("%s\n", note);
  std::printf("%8s%14s%14s%14s%10s\n", "ITER", "OBJ", "PRI_RES", "DUA_RES", "TIME");
  for (int r = 0; r < rows && trace[(size_t)r * 5] >= 0.0; ++r)
    std::printf("%7.0f:%14.6e%14.6e%14.6e%10.0f\n", trace[(size_t)r * 5], trace[(size_t)r * 5 + 1], trace[(size_t)r * 5 + 2],
                trace[(size_t)r * 5 + 3], trace[(size_t)r * 5 + 4]);
  std::fflush(stdout);
}

int verbose_table_rows(const sfb_qp_params *prm)
{
  const uint64_t sci = prm->stop_check_iter > 0 ? (uint64_t)prm->stop_check_iter : 1u, cap = 4096;
  const uint64_t mi  = prm->max_iter >= 0 ? (uint64_t)prm->max_iter : cap * sci;  // (negative: no limit)
  return (int)std::min<uint64_t>(cap, mi / sci + 2);
}

DenseKernelParams make_kernel_params(const sfb_qp_params *prm, int n, int m)
{
  DenseKernelParams kp;
  kp.n          = n;
  kp.m          = m;
  kp.alpha      = static_cast<double>(prm->alpha);  // qp_solver.hpp:354
  kp.alpha_comp = 1.0 - kp.alpha;                   // :355
  kp.rho_bar    = static_cast<double>(prm->rho);    // :353
  kp.sigma      = static_cast<double>(prm->sigma);  // :356
  kp.eps_abs    = static_cast<double>(prm->eps_abs);
  kp.eps_rel    = static_cast<double>(prm->eps_rel);
  kp.eps_pinf   = static_cast<double>(prm->eps_primal_inf);
  kp.eps_dinf   = static_cast<double>(prm->eps_dual_inf);
  kp.delta      = static_cast<double>(prm->delta);
  kp.max_iter   = prm->max_iter < 0 ? (uint32_t)SFB_QP_DEVICE_ITER_CAP : (uint32_t)prm->max_iter;
  kp.max_time_ns = prm->max_time_ns < 0 ? -1 : prm->max_time_ns;
  kp.stop_check_iter = prm->stop_check_iter;
  kp.polish_iter     = prm->polish_iter;
  kp.scaling         = prm->scaling ? 1 : 0;
  kp.polish          = prm->polish ? 1 : 0;
  kp.reuse           = prm->reuse_factor ? 1 : 0;
  return kp;
}


}  // namespace sfb

namespace {
using sfb::fail;
using sfb::hip_fail;
using sfb::require_device;
using sfb::make_kernel_params;

using sfb::QpBatch;
using sfb::DenseRoute;

sfb_status check_qp_args(const sfb_qp_params *prm, int64_t batch, int n, int m, const QpBatch &g)
{
  if (!prm) return fail(SFB_ERR_INVALID_ARG, "prm is NULL");
  if (batch < 0) return fail(SFB_ERR_INVALID_ARG, "batch < 0");
  if (n < 1 || m < 1) return fail(SFB_ERR_INVALID_ARG, "n and m must be >= 1");
  if (batch > 0 && (!g.P || !g.q || !g.A || !g.l || !g.u || !g.x || !g.y || !g.code))
    return fail(SFB_ERR_INVALID_ARG, "NULL problem / solution pointer");
  if ((g.wx == nullptr) != (g.wy == nullptr))
    return fail(SFB_ERR_INVALID_ARG, "warm_x and warm_y must both be given or both be NULL");
  if (prm->max_iter > 0xFFFFFFFFll) return fail(SFB_ERR_INVALID_ARG, "max_iter exceeds uint32");
  if (batch > 0x7FFFFFFFll) return fail(SFB_ERR_UNSUPPORTED, "batch exceeds 2^31-1 per call");
  return SFB_OK;
}

// what is left to report once the launches of a scratch user are on the stream: the error of the free, if any
sfb_status released(sfb::StreamScratch &scratch)
{
  const hipError_t e = scratch.release();
  return e == hipSuccess ? SFB_OK : hip_fail(e, "freeing the call's working memory");
}

// ---- DenseRoute::Big: the pivoted dense LDL' with the factor in HBM ----
// (bit-identical to the dense oracle, i.e. to the reference's dense branch as far as that is pinned)
size_t dense_big_bytes(int64_t batch, int n, int m) { return (size_t)batch * sfb::qp_dense_big_ws_doubles(n, m) * sizeof(double); }

sfb_status dense_big(const sfb_qp_params *prm, int64_t batch, int n, int m, const QpBatch &g, hipStream_t stream, void *workspace)
{
  sfb::StreamScratch scratch(workspace, dense_big_bytes(batch, n, m), stream);  // the caller's (sfb_workspace), or per call
  if (scratch.error() != hipSuccess) return hip_fail(scratch.error(), "hipMalloc");
  const hipError_t e = sfb::qp_dense_big_launch(make_kernel_params(prm, n, m), batch, g, static_cast<double *>(scratch.get()), stream);
  if (e != hipSuccess) return hip_fail(e, "qp_dense_big_kernel launch");
  return released(scratch);
}

// ---- DenseRoute::FullPattern: the shared-pattern sparse kernel with a FULL pattern ----
// P (n x n, column-major, all entries stored) IS the CSC value array of a full pattern, so the stopping tests
// and the objective see the same matrix entries in the same order as the dense kernels; only A has to be
// re-laid out by rows.  What differs from the reference's dense solver is the factorisation order (fill-reducing
// elimination order without pivoting instead of pivoted dense LDL'), i.e. rounding.
__global__ void __launch_bounds__(64) dense_A_to_rows_kernel(const double *__restrict__ A, double *__restrict__ Ax,
                                                             const int n, const int m)
{
  const size_t off = (size_t)blockIdx.x * (size_t)(m * n);
  for (int e = threadIdx.x; e < m * n; e += 64) {
    const int r = e / n, c = e - r * n;
    Ax[off + e] = A[off + r + (size_t)c * m];
  }
}

sfb_status dense_full_pattern_plan(int n, int m, sfb_sparse_qp_plan **out)
{
  static std::mutex mu;
  static std::map<std::pair<int, int>, sfb_sparse_qp_plan *> plans;  // one symbolic analysis per shape, kept
  sfb_sparse_qp_plan *plan = nullptr;
  {
    std::lock_guard<std::mutex> lock(mu);
    auto it = plans.find({n, m});
    if (it == plans.end()) {
      std::vector<int32_t> Pp(n + 1), Pi((size_t)n * n), Ap(m + 1), Aj((size_t)m * n);
      for (int c = 0; c <= n; ++c) Pp[c] = c * n;
      for (int c = 0; c < n; ++c)
        for (int r = 0; r < n; ++r) Pi[(size_t)c * n + r] = r;
      for (int r = 0; r <= m; ++r) Ap[r] = r * n;
      for (int r = 0; r < m; ++r)
        for (int c = 0; c < n; ++c) Aj[(size_t)r * n + c] = c;
      const sfb_status st = sfb_sparse_qp_plan_create(n, m, Pp.data(), Pi.data(), Ap.data(), Aj.data(), 1, nullptr, &plan);
      if (st != SFB_OK) return st;
      plans[{n, m}] = plan;
    } else {
      plan = it->second;
    }
  }
  *out = plan;
  return SFB_OK;
}

// bytes of one dense_via_sparse call: A by rows, then the sparse kernel's workspace
sfb_status dense_via_sparse_bytes(sfb_sparse_qp_plan *plan, int64_t batch, int n, int m, size_t *abytes, size_t *bytes)
{
  int64_t wsb   = 0;
  sfb_status st = sfb_sparse_qp_plan_workspace_bytes(plan, batch, &wsb);
  if (st != SFB_OK) return st;
  *abytes = ((size_t)batch * (size_t)m * n * sizeof(double) + 255) / 256 * 256;
  *bytes  = *abytes + (size_t)wsb;
  return SFB_OK;
}

sfb_status dense_via_sparse(const sfb_qp_params *prm, int64_t batch, int n, int m, const QpBatch &g, hipStream_t stream, void *workspace)
{
  sfb_sparse_qp_plan *plan = nullptr;
  sfb_status st            = dense_full_pattern_plan(n, m, &plan);
  if (st != SFB_OK) return st;
  size_t abytes = 0, bytes = 0;
  st = dense_via_sparse_bytes(plan, batch, n, m, &abytes, &bytes);
  if (st != SFB_OK) return st;
  sfb::StreamScratch scratch(workspace, bytes, stream);
  if (scratch.error() != hipSuccess) return hip_fail(scratch.error(), "hipMalloc");
  char *buf  = static_cast<char *>(scratch.get());
  double *Ax = reinterpret_cast<double *>(buf);
  hipLaunchKernelGGL(dense_A_to_rows_kernel, dim3((unsigned)batch), dim3(64), 0, stream, g.A, Ax, n, m);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "dense_A_to_rows_kernel launch");
  QpBatch rows = g;
  rows.A       = Ax;
  st = sfb::sparse_solve_batch(plan, prm, batch, rows, buf + abytes, nullptr, stream);
  if (st != SFB_OK) return st;
  return released(scratch);
}

// ---- one table: a route's working memory and its launch, side by side ----
// SFB_QP_DENSE_BIG=0 (A/B, tests): sizes beyond 128 through the un-pivoted sparse kernel as well
DenseRoute dense_route_of(const sfb_qp_params *prm, int n, int m)
{
  const char *const bv = sfb::knob("SFB_QP_DENSE_BIG");
  return sfb::dense_route(n + m, prm->max_time_ns >= 0, bv && bv[0] == '0');
}

// device memory the route's launch needs beyond its arguments (0: everything on chip)
sfb_status dense_route_bytes(DenseRoute route, const sfb_qp_params *prm, int64_t batch, int n, int m, size_t *bytes)
{
  switch (route) {
    case DenseRoute::Four: *bytes = sfb::qp_dense4_ws_bytes(n, m, batch); return SFB_OK;
    case DenseRoute::Mid: *bytes = sfb::qp_dense_mid_ws_bytes(make_kernel_params(prm, n, m), batch); return SFB_OK;
    case DenseRoute::Big: *bytes = dense_big_bytes(batch, n, m); return SFB_OK;
    case DenseRoute::FullPattern: {
      sfb_sparse_qp_plan *plan = nullptr;
      const sfb_status st      = dense_full_pattern_plan(n, m, &plan);
      if (st != SFB_OK) return st;
      size_t abytes = 0;
      return dense_via_sparse_bytes(plan, batch, n, m, &abytes, bytes);
    }
  }
  return fail(SFB_ERR_UNSUPPORTED, "unknown dense route");
}

// workspace: at least dense_route_bytes of device memory, or nullptr = stream-ordered allocation inside the launch
sfb_status dense_route_launch(DenseRoute route, const sfb_qp_params *prm, int64_t batch, int n, int m, const QpBatch &g, hipStream_t stream,
                              void *workspace)
{
  hipError_t e = hipSuccess;
  switch (route) {
    case DenseRoute::Four:
      e = sfb::qp_dense4_launch(make_kernel_params(prm, n, m), batch, g, stream, workspace);
      return e == hipSuccess ? SFB_OK : hip_fail(e, "qp_dense4_kernel launch");
    case DenseRoute::Mid:
      e = sfb::qp_dense_mid_launch(make_kernel_params(prm, n, m), batch, g, stream, workspace);
      return e == hipSuccess ? SFB_OK : hip_fail(e, "qp_dense_mid_kernel launch");
    case DenseRoute::Big: return dense_big(prm, batch, n, m, g, stream, workspace);
    case DenseRoute::FullPattern: return dense_via_sparse(prm, batch, n, m, g, stream, workspace);
  }
  return fail(SFB_ERR_UNSUPPORTED, "unknown dense route");
}

// ---- verbose, ONE dense problem (device pointers of the call): the per-iteration table of qp_solver.hpp:490-501 ----
// Both tables come from a second, diagnostic solve of the same problem through a TRACE instance.  What they share: the
// solve's results and its table behind whatever the caller declared in `a`, rows preset to ITER = -1, `run(g, dtrace)`,
// then table, iter and code down.  The block stays in `t` so that the caller can fetch its extras.
struct TableSolve {
  sfb::DeviceBlock blk;
  std::vector<double> tr;
  uint32_t iter = 0;
  int32_t code  = -1;
};
template<class Run>
bool table_solve(sfb::DeviceArena &a, int n, int m, int rows, QpBatch g, TableSolve &t, Run run)
{
  double *dtr = nullptr;
  a.add(&g.x, (size_t)n); a.add(&g.y, (size_t)m); a.add(&g.obj, 1); a.add(&dtr, (size_t)rows * 5); a.add(&g.iter, 1); a.add(&g.code, 1);
  t.blk = sfb::DeviceBlock(a.bytes());
  if (t.blk.error() != hipSuccess || !a.bind(t.blk.get())) return false;
  t.tr.assign((size_t)rows * 5, 0.0);
  for (int r = 0; r < rows; ++r) t.tr[(size_t)r * 5] = -1.0;
  return sfb::upload(dtr, t.tr.data(), t.tr.size()) == hipSuccess && run(g, dtr) && hipDeviceSynchronize() == hipSuccess &&
         sfb::download(t.tr.data(), dtr, t.tr.size()) == hipSuccess && sfb::download(&t.iter, g.iter, 1) == hipSuccess &&
         sfb::download(&t.code, g.code, 1) == hipSuccess;
}

// n + m <= 128: the table from the TRACE instance of the on-chip dense kernel (qp_dense_mid.hip) -- the same pivoted arithmetic as
// the solve whose results the caller receives (every dense route is bit-identical to the dense oracle), so the rows ARE that solve's
// iterates.  The closing summary (:550-565) follows from the same launch's phase stamps.  The re-solve runs WITHOUT the caller's time
// limit and for at most the iterations the returned solve took (real_iter, nullable): a solve that ended with MaxTime has
// its table end at the same iteration instead of wherever the second run's clock would cut it.
void dense_native_table(const sfb_qp_params *prm, int n, int m, const QpBatch &g, const uint32_t *real_iter, const int32_t *real_code)
{
  const int rows   = sfb::verbose_table_rows(prm);
  sfb_qp_params p2 = *prm;
  p2.verbose       = 0;
  p2.max_time_ns   = -1;
  if (real_iter != nullptr && (p2.max_iter < 0 || (int64_t)*real_iter < p2.max_iter)) p2.max_iter = (int64_t)*real_iter;
  const sfb::DenseKernelParams kp = make_kernel_params(&p2, n, m);
  sfb::DeviceArena a;
  double *dph = nullptr, ph[6] = {0, 0, 0, 0, 0, 0};
  a.add(&dph, 16);
  TableSolve t;
  // (the phase scratch is zeroed: whatever stamps a kernel variant leaves out read as 0, not as what the allocation held)
  const bool ok = table_solve(a, n, m, rows, g, t, [&](const QpBatch &gt, double *dtr) {
                    return hipMemset(dph, 0, 16 * 8) == hipSuccess && sfb::qp_dense_mid_trace_launch(kp, 1, gt, nullptr, dtr, rows, dph) == hipSuccess;
                  }) && sfb::download(ph, dph, 6) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return; }
  sfb::verbose_table("dense", n, m, t.tr.data(), rows, nullptr);
  sfb::verbose_summary(real_code ? *real_code : t.code, real_iter ? *real_iter : t.iter, ph);
  if (real_iter != nullptr && real_code != nullptr && (t.iter != *real_iter || (t.code != *real_code && *real_code != SFB_QP_MAX_TIME)))
    std::printf("[sfb] verbose: NOTE the table's solve ended after %u iterations with code %d, the returned solve after %u iterations with code %d\n",
                t.iter, (int)t.code, *real_iter, (int)*real_code);
}

// beyond 128 the dense kernels carry no trace: the diagnostic solve goes through the sparse kernel's TRACE instance on the
// full pattern -- no pivoting there, so its iterates equal the dense kernel's up to rounding (the header says so); the
// results the caller receives are the dense kernel's.
void dense_verbose_table(const sfb_qp_params *prm, int n, int m, const QpBatch &g, const uint32_t *real_iter, const int32_t *real_code)
{
  sfb_sparse_qp_plan *plan = nullptr;
  if (dense_full_pattern_plan(n, m, &plan) != SFB_OK) return;
  size_t abytes = 0, bytes = 0;
  if (dense_via_sparse_bytes(plan, 1, n, m, &abytes, &bytes) != SFB_OK) return;
  const int rows   = sfb::verbose_table_rows(prm);
  sfb_qp_params p2 = *prm;
  p2.verbose       = 0;
  sfb::DeviceArena a;
  char *buf = nullptr;  // A by rows, then the sparse kernel's workspace
  a.add(&buf, bytes);
  TableSolve t;
  const bool ok = table_solve(a, n, m, rows, g, t, [&](const QpBatch &gt, double *dtr) {
    QpBatch gr = gt;
    gr.A       = reinterpret_cast<double *>(buf);
    hipLaunchKernelGGL(dense_A_to_rows_kernel, dim3(1), dim3(64), 0, nullptr, g.A, reinterpret_cast<double *>(buf), n, m);
    return hipGetLastError() == hipSuccess && sfb::sparse_solve_batch(plan, &p2, 1, gr, buf + abytes, nullptr, nullptr, dtr, rows) == SFB_OK;
  });
  if (!ok) {
    (void)hipGetLastError();
    if (t.blk.get() != nullptr)  // (without memory: no diagnostic solve, no table, no remark)
      std::printf("[sfb] verbose: the diagnostic solve behind the per-iteration table failed (%s); no table\n", sfb_last_error());
    return;
  }
  sfb::verbose_table("dense", n, m, t.tr.data(), rows,
                     "(table: diagnostic solve without pivoting, equal to the solve's iterates up to rounding)");
  // the solve whose results the caller receives is the pivoted dense kernel's: say so when the two ended differently
  if (real_iter != nullptr && real_code != nullptr && (t.iter != *real_iter || t.code != *real_code))
    std::printf("[sfb] verbose: NOTE the table's diagnostic solve ended after %u iterations with code %d, the returned (pivoted) solve after "
                "%u iterations with code %d\n", t.iter, (int)t.code, *real_iter, (int)*real_code);
}

}  // namespace

namespace sfb {
namespace {
std::mutex g_devices_mu;
std::vector<int> g_devices;  // empty: all visible devices
}  // namespace

std::vector<int> device_list()
{
  {
    std::lock_guard<std::mutex> lk(g_devices_mu);
    if (!g_devices.empty()) return g_devices;
  }
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess) {
    (void)hipGetLastError();
    cnt = 0;
  }
  std::vector<int> all((size_t)std::max(cnt, 0));
  for (int d = 0; d < cnt; ++d) all[(size_t)d] = d;
  return all;
}

sfb_status run_sharded(int64_t batch, const std::function<sfb_status(int, int64_t, int64_t)> &fn)
{
  const std::vector<int> devs = device_list();
  if (devs.empty()) return fail(SFB_ERR_NO_DEVICE, "no HIP device (the sfb library has no CPU fallback)");
  const int64_t G = (int64_t)devs.size();
  std::vector<sfb_status> st((size_t)G, SFB_OK);
  std::vector<std::string> msg((size_t)G);
  std::vector<std::thread> th;
  bool spawn_failed = false;
  for (int64_t g = 0; g < G && !spawn_failed; ++g) {
    const int64_t b0 = batch * g / G, b1 = batch * (g + 1) / G;  // contiguous shards
    if (b1 == b0) continue;
    try {
      th.emplace_back([&, g, b0, b1] {
        try {
          hipError_t e = hipSetDevice(devs[(size_t)g]);
          if (e != hipSuccess) st[(size_t)g] = hip_fail(e, "hipSetDevice");
          else st[(size_t)g] = fn(devs[(size_t)g], b0, b1 - b0);
        } catch (const std::exception &ex) {  // (nothing may leave a thread of an extern "C" entry point)
          st[(size_t)g] = fail(SFB_ERR_HIP, std::string("exception in a shard: ") + ex.what());
        } catch (...) {
          st[(size_t)g] = fail(SFB_ERR_HIP, "exception in a shard");
        }
        if (st[(size_t)g] != SFB_OK) msg[(size_t)g] = sfb_last_error();  // (thread-local: carried over by hand)
      });
    } catch (const std::exception &) {  // std::system_error of the thread constructor: finish what was started, then report
      spawn_failed = true;
    }
  }
  for (auto &t : th) t.join();
  if (spawn_failed) return fail(SFB_ERR_HIP, "could not start a host thread for a device shard");
  for (int64_t g = 0; g < G; ++g)
    if (st[(size_t)g] != SFB_OK) return fail(st[(size_t)g], "device " + std::to_string(devs[(size_t)g]) + ": " + msg[(size_t)g]);
  return SFB_OK;
}
}  // namespace sfb

extern "C" {

const char *sfb_version(void) { return "smooth_feedback_amd 0.1.0 (gfx950)"; }

sfb_status sfb_set_devices(const int *devices, int count)
{
  if (count < 0 || (count > 0 && !devices)) return fail(SFB_ERR_INVALID_ARG, "bad device list");
  int visible = 0;
  if (hipGetDeviceCount(&visible) != hipSuccess) {
    (void)hipGetLastError();
    visible = 0;
  }
  for (int i = 0; i < count; ++i)
    if (devices[i] < 0 || devices[i] >= visible) return fail(SFB_ERR_INVALID_ARG, "device ordinal out of range");
  std::lock_guard<std::mutex> lk(sfb::g_devices_mu);
  sfb::g_devices.assign(devices, devices + count);
  return SFB_OK;
}

sfb_status sfb_get_devices(int *devices, int capacity, int *count)
{
  if (!count) return fail(SFB_ERR_INVALID_ARG, "count is NULL");
  const std::vector<int> d = sfb::device_list();
  *count = (int)d.size();
  for (int i = 0; devices && i < capacity && i < (int)d.size(); ++i) devices[i] = d[(size_t)i];
  return SFB_OK;
}

const char *sfb_last_error(void) { return sfb::g_last_error.c_str(); }

sfb_status sfb_debug_set(const char *name, const char *value)
{
  if (sfb::knob_set(name, value) != 0) return sfb::fail(SFB_ERR_INVALID_ARG, std::string("sfb_debug_set: unknown knob ") + (name ? name : "(null)"));
  return SFB_OK;
}

sfb_status sfb_device_count(int *count)
{
  if (!count) return fail(SFB_ERR_INVALID_ARG, "count is NULL");
  int cnt      = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    cnt = 0;
  }
  *count = cnt;
  return SFB_OK;
}

void sfb_qp_params_default(sfb_qp_params *p)
{
  if (!p) return;
  p->alpha           = 1.6f;
  p->rho             = 0.1f;
  p->sigma           = 1e-6f;
  p->scaling         = 1;
  p->eps_abs         = 1e-3f;
  p->eps_rel         = 1e-3f;
  p->eps_primal_inf  = 1e-4f;
  p->eps_dual_inf    = 1e-4f;
  p->max_iter        = -1;
  p->max_time_ns     = -1;
  p->stop_check_iter = 25;
  p->polish          = 1;
  p->polish_iter     = 5;
  p->delta           = 1e-6f;
  p->verbose         = 0;
  p->reuse_factor    = 0;
}

struct sfb_workspace {
  void *mem    = nullptr;
  size_t bytes = 0;
  int device   = -1;
};

// device workspace one dense call needs beyond its arguments (0: everything on chip)
static sfb_status dense_workspace_need(const sfb_qp_params *prm, int64_t batch, int n, int m, size_t *need)
{
  *need                  = 0;
  const DenseRoute route = dense_route_of(prm, n, m);
  const sfb_status st    = dense_route_bytes(route, prm, batch, n, m, need);
  // the over-ask sfb.h documents: a time limit sends k <= 32 to Mid, which implements it; the larger of the Four and Mid needs is asked for
  if (st == SFB_OK && route == DenseRoute::Mid && n + m <= sfb::kDenseFourMaxK) *need = std::max(*need, sfb::qp_dense4_ws_bytes(n, m, batch));
  return st;
}

static sfb_status dense_solve_impl(const sfb_qp_params *prm, int64_t batch, int n, int m, const QpBatch &g, sfb_workspace *ws, bool ws_given,
                                   void *stream)
{
  sfb_status st = check_qp_args(prm, batch, n, m, g);
  if (st != SFB_OK) return st;
  if (ws_given && !ws) return fail(SFB_ERR_INVALID_ARG, "workspace is NULL");
  st = require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  void *wsmem = nullptr;
  if (ws) {
    size_t need = 0;
    st          = dense_workspace_need(prm, batch, n, m, &need);
    if (st != SFB_OK) return st;
    if (ws->bytes < need) return fail(SFB_ERR_INVALID_ARG, "workspace too small (sfb_qp_dense_workspace_bytes)");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != ws->device)
      return fail(SFB_ERR_INVALID_ARG, "workspace belongs to another device than the current one");
    wsmem = need ? ws->mem : nullptr;
  }
  return dense_route_launch(dense_route_of(prm, n, m), prm, batch, n, m, g, static_cast<hipStream_t>(stream), wsmem);
}

sfb_status sfb_qp_dense_solve_batch(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                    const double *q, const double *A, const double *l, const double *u,
                                    const double *warm_x, const double *warm_y, double *x, double *y, double *obj,
                                    uint32_t *iter, int32_t *code, void *stream)
{
  const QpBatch g{P, q, A, l, u, warm_x, warm_y, x, y, obj, iter, code};
  return dense_solve_impl(prm, batch, n, m, g, nullptr, false, stream);
}

sfb_status sfb_qp_dense_solve_batch_ws(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                       const double *q, const double *A, const double *l, const double *u,
                                       const double *warm_x, const double *warm_y, double *x, double *y, double *obj,
                                       uint32_t *iter, int32_t *code, sfb_workspace *workspace, void *stream)
{
  const QpBatch g{P, q, A, l, u, warm_x, warm_y, x, y, obj, iter, code};
  return dense_solve_impl(prm, batch, n, m, g, workspace, true, stream);
}

// ---- tall problems through the reduced n x n system (qp_dense_tall.hip) ----
static sfb_status check_tall_size(int n, int m)
{
  if (n > SFB_QP_DENSE_TALL_MAX_N || m > SFB_QP_DENSE_TALL_MAX_M)
    return fail(SFB_ERR_UNSUPPORTED, "the reduced-KKT route needs n <= SFB_QP_DENSE_TALL_MAX_N and m <= SFB_QP_DENSE_TALL_MAX_M");
  return SFB_OK;
}

static sfb_status tall_solve_impl(const sfb_qp_params *prm, int64_t batch, int n, int m, const QpBatch &g, void *stream)
{
  sfb_status st = check_qp_args(prm, batch, n, m, g);
  if (st != SFB_OK) return st;
  if ((st = check_tall_size(n, m)) != SFB_OK) return st;
  if ((st = require_device()) != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  // rows that fit neither registers nor LDS keep sy and z in device memory: stream-ordered, like the big dense kernel's factor
  sfb::StreamScratch scratch(nullptr, sfb::qp_dense_tall_ws_bytes(n, m, batch), hs);
  if (scratch.error() != hipSuccess) return hip_fail(scratch.error(), "hipMalloc");
  const hipError_t e = sfb::qp_dense_tall_launch(make_kernel_params(prm, n, m), batch, g, hs, scratch.get());
  if (e != hipSuccess) return hip_fail(e, "qp_dense_tall_kernel launch");
  return released(scratch);
}

sfb_status sfb_qp_dense_tall_solve_batch(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                         const double *q, const double *A, const double *l, const double *u,
                                         const double *warm_x, const double *warm_y, double *x, double *y, double *obj,
                                         uint32_t *iter, int32_t *code, void *stream)
{
  const QpBatch g{P, q, A, l, u, warm_x, warm_y, x, y, obj, iter, code};
  return tall_solve_impl(prm, batch, n, m, g, stream);
}

// ---- the per-iteration table and the phase times as data: always the TRACE instance of the on-chip kernel ----
static sfb_status check_dense_trace(int n, int m, const double *trace, int32_t trace_rows)
{
  if (trace_rows < 0 || (trace_rows > 0 && !trace)) return fail(SFB_ERR_INVALID_ARG, "trace is NULL or trace_rows < 0");
  if (n + m > sfb::kDenseMidMaxK) return fail(SFB_ERR_UNSUPPORTED, "the per-iteration table of a dense problem needs n + m <= 128");
  return SFB_OK;
}

static sfb_status dense_phases_impl(const sfb_qp_params *prm, int64_t batch, int n, int m, const QpBatch &g, double *trace,
                                    int32_t trace_rows, double *phase_us, void *stream)
{
  sfb_status st = check_qp_args(prm, batch, n, m, g);
  if (st != SFB_OK) return st;
  if ((st = check_dense_trace(n, m, trace, trace_rows)) != SFB_OK) return st;
  st = require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  const hipError_t e = sfb::qp_dense_mid_trace_launch(make_kernel_params(prm, n, m), batch, g, static_cast<hipStream_t>(stream),
                                                      trace_rows > 0 ? trace : nullptr, trace_rows, phase_us);
  if (e != hipSuccess) return hip_fail(e, "qp_dense_mid_trace_kernel launch");
  return SFB_OK;
}

sfb_status sfb_qp_dense_solve_batch_trace(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P, const double *q,
                                          const double *A, const double *l, const double *u, const double *warm_x, const double *warm_y,
                                          double *x, double *y, double *obj, uint32_t *iter, int32_t *code, double *trace,
                                          int32_t trace_rows, void *stream)
{
  const QpBatch g{P, q, A, l, u, warm_x, warm_y, x, y, obj, iter, code};
  return dense_phases_impl(prm, batch, n, m, g, trace, trace_rows, nullptr, stream);
}

sfb_status sfb_qp_dense_solve_batch_phases(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P, const double *q,
                                           const double *A, const double *l, const double *u, const double *warm_x, const double *warm_y,
                                           double *x, double *y, double *obj, uint32_t *iter, int32_t *code, double *trace,
                                           int32_t trace_rows, double *phase_us, void *stream)
{
  const QpBatch g{P, q, A, l, u, warm_x, warm_y, x, y, obj, iter, code};
  return dense_phases_impl(prm, batch, n, m, g, trace, trace_rows, phase_us, stream);
}

sfb_status sfb_qp_dense_workspace_bytes(const sfb_qp_params *prm, int64_t batch, int n, int m, int64_t *bytes)
{
  if (!prm || !bytes) return fail(SFB_ERR_INVALID_ARG, "NULL argument");
  if (batch < 0 || n < 1 || m < 1) return fail(SFB_ERR_INVALID_ARG, "batch < 0 or n, m < 1");
  size_t need   = 0;
  sfb_status st = dense_workspace_need(prm, batch, n, m, &need);
  if (st != SFB_OK) return st;
  *bytes = (int64_t)need;
  return SFB_OK;
}

sfb_status sfb_workspace_create(int64_t bytes, sfb_workspace **out)
{
  if (!out || bytes < 0) return fail(SFB_ERR_INVALID_ARG, "out is NULL or bytes < 0");
  *out          = nullptr;
  sfb_status st = require_device();
  if (st != SFB_OK) return st;
  auto *w       = new sfb_workspace();
  hipError_t e  = hipGetDevice(&w->device);
  if (e == hipSuccess && bytes > 0) e = hipMalloc(&w->mem, (size_t)bytes);
  if (e != hipSuccess) {
    delete w;
    return hip_fail(e, "hipMalloc(workspace)");
  }
  w->bytes = (size_t)bytes;
  *out     = w;
  return SFB_OK;
}

void sfb_workspace_destroy(sfb_workspace *ws)
{
  if (!ws) return;
  if (ws->mem) (void)hipFree(ws->mem);
  delete ws;
}

sfb_status sfb_workspace_info(const sfb_workspace *ws, void **device_ptr, int64_t *bytes)
{
  if (!ws) return fail(SFB_ERR_INVALID_ARG, "workspace is NULL");
  if (device_ptr) *device_ptr = ws->mem;
  if (bytes) *bytes = (int64_t)ws->bytes;
  return SFB_OK;
}

}  // extern "C"

namespace {
struct HostStage {
  char *mem;
  size_t bytes;
};
std::mutex g_stage_mu;
std::map<int, HostStage> g_stage;  // per device: the staging buffer kept between host-pointer calls
HostStage host_stage_take(int dev)
{
  std::lock_guard<std::mutex> lk(g_stage_mu);
  HostStage s = {nullptr, 0};
  auto it = g_stage.find(dev);
  if (it != g_stage.end()) { s = it->second; g_stage.erase(it); }
  return s;
}
void host_stage_give(int dev, HostStage s)
{
  if (!s.mem) return;
  HostStage drop = {nullptr, 0};
  {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    auto it = g_stage.find(dev);
    if (it == g_stage.end()) g_stage[dev] = s;
    else if (it->second.bytes < s.bytes) { drop = it->second; it->second = s; }  // keep the larger one
    else drop = s;
  }
  if (drop.mem) (void)hipFree(drop.mem);
}
}  // namespace

extern "C" {

void sfb_host_staging_trim(void)
{
  std::map<int, HostStage> old;
  {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    old.swap(g_stage);
  }
  for (auto &kv : old)
    if (kv.second.mem) (void)hipFree(kv.second.mem);
}

// the host-pointer solve of both dense routes (tall: the reduced-KKT kernel) on the kept staging buffer
static sfb_status dense_host_impl(const sfb_qp_params *prm, int64_t batch, int n, int m, const QpBatch &h, const bool tall)
{
  sfb_status st = check_qp_args(prm, batch, n, m, h);
  if (st != SFB_OK) return st;
  if (tall && (st = check_tall_size(n, m)) != SFB_OK) return st;
  st = require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;

  const size_t B = (size_t)batch, N = (size_t)n, M = (size_t)m;
  sfb::Staging s;
  QpBatch d{};
  sfb::stage_qp(s, B, N * N, N, M * N, M, h, d);
  // Staging memory of the host-pointer entry point: ONE buffer per device is kept between calls (ASIFilter solves one
  // small QP per tick through here, and a hipMalloc / hipFree pair per call would dominate its latency).  The lock is
  // held only while the buffer is taken or handed back: concurrent callers do not serialise -- one of them gets the
  // kept buffer, the others allocate their own for the call.  sfb_host_staging_trim() frees what is kept.
  const size_t bytes = s.bytes();
  int devid          = 0;
  hipError_t e       = hipGetDevice(&devid);
  if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
  HostStage mine = host_stage_take(devid);
  if (mine.bytes < bytes) {
    if (mine.mem) (void)hipFree(mine.mem);
    mine = {nullptr, 0};
    e    = hipMalloc(reinterpret_cast<void **>(&mine.mem), bytes);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    mine.bytes = bytes;
  }
  struct Return {  // hand the buffer back on every exit path
    int dev;
    HostStage &s;
    ~Return() { host_stage_give(dev, s); }
  } ret{devid, mine};
  if (!s.bind(mine.mem)) return fail(SFB_ERR_UNSUPPORTED, "more staged arrays than the table holds");

  st = SFB_OK;
  using clk = std::chrono::steady_clock;
  auto ms   = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const auto tv0 = clk::now();
  auto tv1 = tv0, tv2 = tv0;
  if ((e = s.upload()) == hipSuccess) {
    tv1 = clk::now();
    st  = tall ? tall_solve_impl(prm, batch, n, m, d, nullptr) : dense_solve_impl(prm, batch, n, m, d, nullptr, false, nullptr);
    if (st == SFB_OK && (e = hipDeviceSynchronize()) == hipSuccess) {
      tv2 = clk::now();
      e   = s.download();
    }
  }
  if (e != hipSuccess) st = hip_fail(e, "sfb_qp_dense_solve_batch_host");
  const auto tv3 = clk::now();
  if (st == SFB_OK && prm->verbose && batch == 1 && !tall) {  // (inputs still on the device)
    uint32_t it1 = 0;
    const bool have_it = h.iter ? (it1 = h.iter[0], true) : hipMemcpy(&it1, d.iter, 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (n + m <= sfb::kDenseMidMaxK) dense_native_table(prm, n, m, d, have_it ? &it1 : nullptr, h.code);  // the solve's own iterates
    else dense_verbose_table(prm, n, m, d, have_it ? &it1 : nullptr, h.code);
  }
  if (st == SFB_OK && prm->verbose) {
    std::vector<uint32_t> itv;
    if (!h.iter) {
      itv.resize(B);
      if (hipMemcpy(itv.data(), d.iter, B * 4, hipMemcpyDeviceToHost) != hipSuccess) itv.clear();
    }
    sfb::verbose_report(tall ? "tall dense QP batch (reduced KKT)" : "dense QP batch", batch, n, m, ms(tv0, tv1), ms(tv1, tv2), ms(tv2, tv3), h.code,
                        h.iter ? h.iter : (itv.empty() ? nullptr : itv.data()));
  }
  return st;
}

static sfb_status dense_host_multi_impl(const sfb_qp_params *prm, int64_t batch, int n, int m, const QpBatch &h, const bool tall)
{
  sfb_status st = check_qp_args(prm, batch, n, m, h);
  if (st != SFB_OK) return st;
  if (tall && (st = check_tall_size(n, m)) != SFB_OK) return st;
  if (batch == 0) return require_device();
  const size_t N = (size_t)n, M = (size_t)m;
  return sfb::run_sharded(batch, [&](int, int64_t b0, int64_t cnt) {
    return dense_host_impl(prm, cnt, n, m, sfb::shard(h, (size_t)b0, N * N, N, M * N, M), tall);
  });
}

static sfb_status dense_host_phases_impl(const sfb_qp_params *prm, int64_t batch, int n, int m, const QpBatch &h, double *trace,
                                         int32_t trace_rows, double *phase_us)
{
  sfb_status st = check_qp_args(prm, batch, n, m, h);
  if (st != SFB_OK) return st;
  if ((st = check_dense_trace(n, m, trace, trace_rows)) != SFB_OK) return st;
  st = require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  const size_t B = (size_t)batch, N = (size_t)n, M = (size_t)m, TR = B * (size_t)trace_rows * 5, PH = phase_us ? B * 16 : 0;
  using S = sfb::Staging;
  S s;
  double *dtr, *dph;
  QpBatch d{};
  s.add(&dtr, TR, S::Out, trace); s.add(&dph, PH);  // (16 doubles of phase scratch per item, 6 of them come down)
  sfb::stage_qp(s, B, N * N, N, M * N, M, h, d);
  const char *entry = "sfb_qp_dense_solve_batch_host_trace";
  return sfb::staged_call(s, entry, [&]() -> sfb_status {
    hipError_t e = hipSuccess;
    if (TR) {  // unused rows keep ITER = -1
      std::vector<double> init(TR, 0.0);
      for (size_t r = 0; r < TR; r += 5) init[r] = -1.0;
      e = sfb::upload(dtr, init.data(), TR);
    }
    if (e == hipSuccess && PH) e = hipMemset(dph, 0, PH * 8);
    if (e != hipSuccess) return hip_fail(e, entry);
    const sfb_status st = dense_phases_impl(prm, batch, n, m, d, TR ? dtr : nullptr, trace_rows, PH ? dph : nullptr, nullptr);
    if (st != SFB_OK || !PH) return st;
    if ((e = hipDeviceSynchronize()) == hipSuccess) e = sfb::download(phase_us, dph, B * 6);
    return e == hipSuccess ? SFB_OK : hip_fail(e, entry);
  });
}

sfb_status sfb_qp_dense_solve_batch_host(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                         const double *q, const double *A, const double *l, const double *u,
                                         const double *warm_x, const double *warm_y, double *x, double *y,
                                         double *obj, uint32_t *iter, int32_t *code)
{
  const QpBatch h{P, q, A, l, u, warm_x, warm_y, x, y, obj, iter, code};
  return dense_host_impl(prm, batch, n, m, h, false);
}

sfb_status sfb_qp_dense_tall_solve_batch_host(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                              const double *q, const double *A, const double *l, const double *u,
                                              const double *warm_x, const double *warm_y, double *x, double *y,
                                              double *obj, uint32_t *iter, int32_t *code)
{
  const QpBatch h{P, q, A, l, u, warm_x, warm_y, x, y, obj, iter, code};
  return dense_host_impl(prm, batch, n, m, h, true);
}

sfb_status sfb_qp_dense_solve_batch_host_multi(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                               const double *q, const double *A, const double *l, const double *u,
                                               const double *warm_x, const double *warm_y, double *x, double *y,
                                               double *obj, uint32_t *iter, int32_t *code)
{
  const QpBatch h{P, q, A, l, u, warm_x, warm_y, x, y, obj, iter, code};
  return dense_host_multi_impl(prm, batch, n, m, h, false);
}

sfb_status sfb_qp_dense_tall_solve_batch_host_multi(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                                    const double *q, const double *A, const double *l, const double *u,
                                                    const double *warm_x, const double *warm_y, double *x, double *y,
                                                    double *obj, uint32_t *iter, int32_t *code)
{
  const QpBatch h{P, q, A, l, u, warm_x, warm_y, x, y, obj, iter, code};
  return dense_host_multi_impl(prm, batch, n, m, h, true);
}

sfb_status sfb_qp_dense_solve_batch_host_trace(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P, const double *q,
                                               const double *A, const double *l, const double *u, const double *warm_x, const double *warm_y,
                                               double *x, double *y, double *obj, uint32_t *iter, int32_t *code, double *trace,
                                               int32_t trace_rows)
{
  const QpBatch h{P, q, A, l, u, warm_x, warm_y, x, y, obj, iter, code};
  return dense_host_phases_impl(prm, batch, n, m, h, trace, trace_rows, nullptr);
}

sfb_status sfb_qp_dense_solve_batch_host_phases(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P, const double *q,
                                                const double *A, const double *l, const double *u, const double *warm_x, const double *warm_y,
                                                double *x, double *y, double *obj, uint32_t *iter, int32_t *code, double *trace,
                                                int32_t trace_rows, double *phase_us)
{
  const QpBatch h{P, q, A, l, u, warm_x, warm_y, x, y, obj, iter, code};
  return dense_host_phases_impl(prm, batch, n, m, h, trace, trace_rows, phase_us);
}

}  // extern "C"
