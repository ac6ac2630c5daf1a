// Batched ph-mesh kernels (mesh.hip): resampling of node values onto the degree-raised mesh and the collocation
// dynamics-error estimate.  Launch arguments; the tables are built on the host by capi_mesh.hip from mesh.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sfb {

constexpr int kMeshMaxK   = 13;  // K + 1 <= 14 raised collocation points
constexpr int kMeshStride = 16;  // rows / columns of every per-degree table: K + 2 <= 15 points, padded with zeros

// one interval of the mesh, as the kernels see it
struct MeshIval {
  int32_t K;        // collocation points (before raising)
  int32_t in_off;   // index of its first node among the mesh's N (+1) nodes
  int32_t out_off;  // index of its first point among the sum (K + 2) raised points
  int32_t closed;   // 0: last interval (its polynomial uses its own K points when the values are not extended)
  double half;      // (tauf - tau0) / 2
};

// per-degree tables for K = 1 .. kMeshMaxK, each kMeshStride x kMeshStride doubles, at table + (K - 1) * 3 * stride^2:
//   Wc (j, i) at [j * stride + i]: raised point j from the K + 1 points of the closed interval
//   Wo (j, i) likewise from the K collocation points alone
//   I  (i, j) at [j * stride + i]: integration matrix of the raised interval (Ke = K + 1) on [-1, 1]
struct MeshDevice {
  int32_t nivals, N, R;     // intervals, nodes (without the end point), raised points
  const MeshIval *ivals;    // [nivals]
  const int32_t *row_ival;  // [R] interval of every raised point
  const double *tables;
};

struct MeshResampleArgs {
  MeshDevice m;
  int64_t batch;
  int32_t dim, extend;
  const double *vals;
  double *out;
};
struct MeshDynErrorArgs {
  MeshDevice m;
  int64_t batch;
  int32_t nx;
  const double *horizon, *X, *F;
  double *errs;
};

hipError_t mesh_resample_launch(const MeshResampleArgs &a, hipStream_t stream);
hipError_t mesh_dyn_error_launch(const MeshDynErrorArgs &a, hipStream_t stream);

}  // namespace sfb
