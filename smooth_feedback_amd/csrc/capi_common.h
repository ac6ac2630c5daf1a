// Shared helpers of the C-ABI translation units (error state, device check, params widening).
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/sfb.h"
#include "../../include/smooth_feedback_amd/detail/device_arena.hpp"
#include "qp_dense_kernel.h"

namespace sfb {

sfb_status fail(sfb_status st, const std::string &msg);
sfb_status hip_fail(hipError_t e, const char *what);
sfb_status require_device();
DenseKernelParams make_kernel_params(const sfb_qp_params *prm, int n, int m);
// QPSolverParams::verbose on the host-pointer entry points (qp_solver.hpp:409-420, :550-565 print a per-phase time
// breakdown and the outcome): one summary of the call -- phase times, status histogram, iteration statistics.
void verbose_report(const char *what, int64_t batch, int n, int m, double h2d_ms, double solve_ms, double d2h_ms,
                    const int32_t *code, const uint32_t *iter);
// ... and, for ONE problem, the per-iteration table itself in the reference's format (:409-420, :490-501): trace = rows x 5
// (ITER, OBJ, PRI_RES, DUA_RES, TIME us; ITER < 0 ends the table), as written by sfb_sparse_qp_solve_batch_trace.
void verbose_table(const char *kind, int n, int m, const double *trace, int rows, const char *note = nullptr);
// ... and its closing summary (:550-565) from the six per-phase times of the *_phases entry points
void verbose_summary(int32_t code, uint32_t iter, const double *phase_us);
// rows a table needs for these parameters (capped)
int verbose_table_rows(const sfb_qp_params *prm);
// Multi-device entry points (sfb_*_multi): the device list of sfb_set_devices (default: every visible device), and a
// helper that cuts [0, batch) into one contiguous shard per list entry and runs `fn(device, first, count)` for every
// non-empty shard on its own host thread with that device current.  Returns the first failure (its message becomes
// this thread's sfb_last_error).
std::vector<int> device_list();
sfb_status run_sharded(int64_t batch, const std::function<sfb_status(int device, int64_t first, int64_t count)> &fn);
// Staging of a host-pointer entry point: every array is declared once -- device pointer, count, host pointer and
// direction -- in the order it lies in the device buffer.  bytes() is what the buffer must hold, bind() hands out the
// device pointers, upload() / download() copy the In / Out arrays whose host pointer is given, in declaration order, up
// to the first error.  A NULL host pointer still reserves its space (add) or leaves the array out (add_opt).  Where the
// memory comes from is the caller's business.
class Staging {
public:
  enum Dir { Scratch = 0, In = 1, Out = 2, InOut = 3 };
  template<class T>
  void add(T **dev, size_t count, Dir dir = Scratch, const std::remove_const_t<T> *host = nullptr)
  {
    const int i = arena_.add(dev, count);
    if (i >= 0) host_[i] = {const_cast<std::remove_const_t<T> *>(host), dir};
  }
  // an array that is absent when the caller gave no host pointer: no bytes, *dev stays NULL and goes to the device entry as such
  template<class T>
  void add_opt(T **dev, size_t count, Dir dir, const std::remove_const_t<T> *host)
  {
    *dev = nullptr;
    if (host) add(dev, count, dir, host);
  }
  size_t bytes() const { return arena_.bytes(); }
  bool bind(void *base) { return arena_.bind(base); }
  hipError_t upload() const { return copy(In, hipMemcpyHostToDevice); }
  hipError_t download() const { return copy(Out, hipMemcpyDeviceToHost); }

private:
  hipError_t copy(int dir, hipMemcpyKind kind) const
  {
    for (int i = 0; i < arena_.size(); ++i) {
      if (!(host_[i].dir & dir) || !host_[i].p || !arena_.bytes(i)) continue;
      const bool up      = kind == hipMemcpyHostToDevice;
      const hipError_t e = hipMemcpy(up ? arena_.at(i) : host_[i].p, up ? host_[i].p : arena_.at(i), arena_.bytes(i), kind);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  struct Host { void *p; int dir; };
  smooth_feedback_amd::detail::DeviceArena arena_;
  Host host_[smooth_feedback_amd::detail::DeviceArena::kCapacity];
};
using smooth_feedback_amd::detail::DeviceArena;
using smooth_feedback_amd::detail::DeviceBlock;
using smooth_feedback_amd::detail::download;
using smooth_feedback_amd::detail::upload;
// memory for one call: a block of s.bytes(), bound to s and freed with `blk`; a HIP failure is reported under `who`
inline sfb_status stage_per_call(Staging &s, DeviceBlock &blk, const char *who)
{
  blk = DeviceBlock(s.bytes());
  if (blk.error() != hipSuccess) return hip_fail(blk.error(), who);
  return s.bind(blk.get()) ? SFB_OK : fail(SFB_ERR_UNSUPPORTED, "more staged arrays than the table holds");
}
// ... with the In arrays in it (also how tables that stay on the device are made: `blk` is then kept)
inline sfb_status stage_and_upload(Staging &s, DeviceBlock &blk, const char *who)
{
  const sfb_status st = stage_per_call(s, blk, who);
  if (st != SFB_OK) return st;
  const hipError_t e = s.upload();
  return e == hipSuccess ? SFB_OK : hip_fail(e, who);
}
// The tail of a host-pointer entry: memory for this call, upload, `call` (the device twin on the null stream; its refusal
// is returned as it is, nothing comes down), wait for the device, download.
template<class Call>
sfb_status staged_call(Staging &s, const char *entry, Call &&call)
{
  DeviceBlock blk;
  sfb_status st = stage_and_upload(s, blk, entry);
  if (st != SFB_OK || (st = call()) != SFB_OK) return st;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = s.download();
  return e == hipSuccess ? SFB_OK : hip_fail(e, entry);
}

// The arrays of a QP batch as every host-pointer entry stages them, after whatever the caller declared before: the seven
// inputs, then x, y, obj, iter, code.  sizeP / sizeA: values of P / A per item (dense: n * n and m * n; sparse: the
// pattern's counts, P / A carry Px / Ax).  Without a warm start dev.wx / dev.wy stay NULL and take no space.
inline void stage_qp(Staging &s, size_t B, size_t sizeP, size_t n, size_t sizeA, size_t m, const QpBatch &host, QpBatch &dev)
{
  using S = Staging;
  s.add(&dev.P, B * sizeP, S::In, host.P); s.add(&dev.q, B * n, S::In, host.q); s.add(&dev.A, B * sizeA, S::In, host.A);
  s.add(&dev.l, B * m, S::In, host.l); s.add(&dev.u, B * m, S::In, host.u);
  dev.wx = dev.wy = nullptr;
  if (host.wx) { s.add(&dev.wx, B * n, S::In, host.wx); s.add(&dev.wy, B * m, S::In, host.wy); }
  s.add(&dev.x, B * n, S::Out, host.x); s.add(&dev.y, B * m, S::Out, host.y); s.add(&dev.obj, B, S::Out, host.obj);
  s.add(&dev.iter, B, S::Out, host.iter); s.add(&dev.code, B, S::Out, host.code);
}

// items [b0, ...) of a batch, for the shards of the *_multi entries; NULL stays NULL
inline QpBatch shard(const QpBatch &g, size_t b0, size_t sizeP, size_t n, size_t sizeA, size_t m)
{
  const auto at = [b0](auto *p, size_t stride) { return p ? p + b0 * stride : nullptr; };
  return {at(g.P, sizeP), at(g.q, n), at(g.A, sizeA), at(g.l, m), at(g.u, m), at(g.wx, n), at(g.wy, m),
          at(g.x, n), at(g.y, m), at(g.obj, 1), at(g.iter, 1), at(g.code, 1)};
}

struct SparsePlanHost;
const SparsePlanHost &plan_host(const sfb_sparse_qp_plan *plan);  // capi_sparse.hip: the pattern the kernel works on
const SparsePlanHost &plan_io(const sfb_sparse_qp_plan *plan);    // the caller's pattern (== plan_host unless pruned)
// capi_sparse.hip: every device-pointer solve of the sparse path (g.P / g.A: the value arrays Px / Ax); order, trace
// ([batch][trace_rows][5]) and phase_us are optional
sfb_status sparse_solve_batch(sfb_sparse_qp_plan *plan, const sfb_qp_params *prm, int64_t batch, const QpBatch &g, void *workspace,
                              const int32_t *order, void *stream, double *trace = nullptr, int32_t trace_rows = 0,
                              double *phase_us = nullptr);

}  // namespace sfb
