// Batched ph-mesh kernels (include/sfb.h: sfb_mesh_resample_batch, sfb_mesh_dyn_error_batch).
//
// resample: one lane per output double.  Lane t is (agent, raised point, coordinate) with the coordinate fastest, so
// a wave writes 512 contiguous bytes and reads, per source node, the same run of coordinates of one or two intervals;
// the K + 1 source rows of an interval are read again by its K + 2 raised points out of the cache.  The weights come
// from the per-degree table (at most 15 x 14 doubles per degree, cache resident).
//
// dyn_error: one lane per (agent, interval, raised point), 16 lane slots per interval (K + 2 <= 15 points), four
// intervals to a wave, one wave to a block.  The slots of an interval first copy its X and F rows into LDS -- runs of
// contiguous doubles, up to 16 coordinates of every row at a time -- then every lane integrates F to its own point
// with its column of the integration matrix (dyn_error_point of dyn_error.hpp, the function the host estimate calls;
// the F and X_0 reads are LDS broadcasts), and the maxima are taken across the 16 slots with cross-lane moves.  Lane 0
// of the slot group writes the interval's error.  Plain loads and stores.
#include "mesh_kernel.h"

#include "../../include/smooth_feedback_amd/dyn_error.hpp"

namespace sfb {

namespace {

namespace L = smooth_feedback_amd;

constexpr int kTable = kMeshStride * kMeshStride;

__global__ void __launch_bounds__(256) mesh_resample_kernel(const MeshResampleArgs a)
{
  const int64_t per_agent = (int64_t)a.m.R * a.dim;
  const int64_t t         = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.batch * per_agent) return;
  const int64_t b = t / per_agent;
  const int e     = (int)(t - b * per_agent);
  const int row = e / a.dim, d = e - row * a.dim;
  const MeshIval iv = a.m.ivals[a.m.row_ival[row]];
  const int j       = row - iv.out_off;
  const bool closed = a.extend || iv.closed;
  const int n       = closed ? iv.K + 1 : iv.K;
  const double *W   = a.m.tables + (int64_t)(iv.K - 1) * 3 * kTable + (closed ? 0 : kTable) + j * kMeshStride;
  const int64_t rows_in = (int64_t)a.m.N + (a.extend ? 1 : 0);
  const double *v       = a.vals + (b * rows_in + iv.in_off) * a.dim + d;
  double acc = 0.0;
  for (int i = 0; i < n; ++i) acc += W[i] * v[(int64_t)i * a.dim];
  a.out[t] = acc;
}

constexpr int kSlots = 16;  // lanes per interval
constexpr int kChunk = 16;  // coordinates staged at a time

__global__ void __launch_bounds__(64) mesh_dyn_error_kernel(const MeshDynErrorArgs a)
{
  __shared__ double sX[4][(kMeshMaxK + 2) * kChunk];
  __shared__ double sF[4][(kMeshMaxK + 1) * kChunk];
  const int grp = threadIdx.x / kSlots, slot = threadIdx.x % kSlots;
  const int64_t pair  = (int64_t)blockIdx.x * 4 + grp;  // (agent, interval)
  const bool live     = pair < a.batch * a.m.nivals;
  const int64_t b     = live ? pair / a.m.nivals : 0;
  const int s         = live ? (int)(pair - b * a.m.nivals) : 0;
  const MeshIval iv   = a.m.ivals[s];
  const int Ke        = iv.K + 1;
  const int64_t base  = (b * a.m.R + iv.out_off) * a.nx;
  const double *I     = a.m.tables + (int64_t)(iv.K - 1) * 3 * kTable + 2 * kTable;
  const double h      = live ? a.horizon[b] * iv.half : 0.0;
  const bool point    = live && slot < Ke;  // this lane owns raised point j = slot + 1
  double e2 = 0.0, x2 = 0.0;
  for (int d0 = 0; d0 < a.nx; d0 += kChunk) {  // (the trip count is the same for every lane: barriers inside)
    const int dc = a.nx - d0 < kChunk ? a.nx - d0 : kChunk;
    if (live) {
      for (int k = slot; k < (Ke + 1) * dc; k += kSlots) {
        const int r = k / dc, d = k - r * dc;
        sX[grp][r * kChunk + d] = a.X[base + (int64_t)r * a.nx + d0 + d];
      }
      for (int k = slot; k < Ke * dc; k += kSlots) {
        const int r = k / dc, d = k - r * dc;
        sF[grp][r * kChunk + d] = a.F[base + (int64_t)r * a.nx + d0 + d];
      }
    }
    __syncthreads();
    if (point) L::dyn_error_point(Ke, dc, slot + 1, sX[grp], kChunk, sF[grp], kChunk, I, kMeshStride, h, e2, x2);
    __syncthreads();
  }
  bool bad = e2 != e2 || x2 != x2;
  if (!point) e2 = x2 = 0.0, bad = false;
#pragma unroll
  for (int off = kSlots / 2; off > 0; off >>= 1) {
    const double oe = __shfl_xor(e2, off, kSlots), ox = __shfl_xor(x2, off, kSlots);
    const int ob    = __shfl_xor((int)bad, off, kSlots);
    e2  = oe > e2 ? oe : e2;
    x2  = ox > x2 ? ox : x2;
    bad = bad || ob;
  }
  if (live && slot == 0) a.errs[pair] = L::dyn_error_combine(e2, x2, bad);
}

}  // namespace

hipError_t mesh_resample_launch(const MeshResampleArgs &a, hipStream_t stream)
{
  const int64_t total  = a.batch * a.m.R * a.dim;
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mesh_resample_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t mesh_dyn_error_launch(const MeshDynErrorArgs &a, hipStream_t stream)
{
  const int64_t blocks = (a.batch * a.m.nivals + 3) / 4;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mesh_dyn_error_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace sfb
