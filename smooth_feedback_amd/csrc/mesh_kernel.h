// Batched ph-mesh kernels (mesh.hip): resampling of node values onto the degree-raised mesh, the collocation
// dynamics-error estimate, and the functions over the mesh (eval, integrate, dyn) with their first derivatives.  Launch arguments; the tables are built on the host by capi_mesh.hip from mesh.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/smooth_feedback_amd/mesh_function.hpp"

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

// ---- functions over the mesh with first derivatives (mesh_function.hpp: mesh_eval, mesh_integrate, mesh_dyn) ----
// one interval, as these kernels see it
struct MeshFnIval {
  int32_t K;     // collocation points
  int32_t M;     // index of its first node
  int32_t Doff;  // its (K + 1) x K unscaled differentiation matrix starts at D + Doff: D(k, j) at [k + j (K + 1)]
  int32_t pad;
  double alpha;  // 2 / (tauf - tau0)
};
// what one (mesh, nx, nu) needs on the device; built on the host by capi_mesh.hip and cached with the interval lists
struct MeshFnDevice {
  int32_t nivals, N, nx, nu;
  int64_t dyn_nnz;
  const MeshFnIval *ivals;       // [nivals]
  const int32_t *node_ival;      // [N] interval of every node
  const double *tau, *w;         // [N] nodes on [0, 1] and quadrature weights
  const double *D;
  const int32_t *dyn_rowptr;     // [N nx + 1] CSR row starts of mesh_dyn's dF
  const int32_t *dyn_entry_row;  // [dyn_nnz] the decode table: row (node nx + component) of every entry
};
struct MeshFnArgs {
  MeshFnDevice m;
  int64_t batch;
  int32_t nf, scale;
  const double *t0, *tf, *X, *F, *dF;  // dF NULL: values only
  double *out_F, *out_dF;
};
hipError_t mesh_eval_launch(const MeshFnArgs &a, hipStream_t stream);
hipError_t mesh_integrate_launch(const MeshFnArgs &a, hipStream_t stream);
hipError_t mesh_dyn_launch(const MeshFnArgs &a, hipStream_t stream);

// ---- the collocation NLP of an OCP (ocp_to_nlp.hpp): g [batch][m] and the CSR values of dg_dx [batch][nnz], fused ----
struct OcpNlpArgs {
  smooth_feedback_amd::meshfn::OcpNlpTables T;  // device pointers: nodes, D and the decode records of one (mesh, dims)
  int64_t batch, n;
  int32_t agents;  // agents a lane walks with one decoded item (set by the launch)
  const double *x, *Ff, *dFf, *Fg, *dFg, *Fcr, *dFcr, *ce, *dce;  // the Jacobians NULL: values only
  double *g, *dg;
};
hipError_t ocp_nlp_launch(const OcpNlpArgs &a, hipStream_t stream);

// ---- its Lagrangian Hessian: the values of sigma d2f + d2g(lambda) [batch][nnzH] over the upper-triangle CSC pattern ----
struct OcpNlpHessArgs {
  smooth_feedback_amd::meshfn::OcpNlpHessTables T;  // device pointers: nodes and the decode records of one (mesh, dims)
  int64_t batch, n;
  int32_t agents;  // agents a lane walks with one decoded record (set by the launch)
  const double *x, *lambda, *sigma, *dFf, *HLf, *dFg, *HLg, *HLcr, *d2theta, *d2ce_l;  // per agent; a segment of length zero: NULL
  double *hess;
};
hipError_t ocp_nlp_hess_launch(const OcpNlpHessArgs &a, hipStream_t stream);

}  // namespace sfb
