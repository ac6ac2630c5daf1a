// C-ABI for the batched ph-mesh path (include/sfb.h): resampling onto the degree-raised mesh, dynamics-error estimate,
// the functions over the mesh (eval, integrate, dyn) with first derivatives and their sparsity patterns, and the
// collocation NLP of an OCP over the mesh (structure, pattern, bounds, fused batched g / dg_dx, and the pattern and fused
// batched values of its Lagrangian Hessian).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/sfb.h"
#include "../../include/smooth_feedback_amd/mesh.hpp"
#include "../../include/smooth_feedback_amd/mesh_function.hpp"
#include "capi_common.h"
#include "mesh_kernel.h"

namespace {

namespace L = smooth_feedback_amd;

// what every entry point refuses first: the mesh, then the batch
sfb_status mesh_check(const sfb_mesh *mesh, int64_t batch)
{
  if (!mesh || !mesh->K || !mesh->tau0) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL mesh");
  if (mesh->nivals < 1) return sfb::fail(SFB_ERR_INVALID_ARG, "mesh: nivals < 1");
  for (int32_t s = 0; s < mesh->nivals; ++s)
    if (mesh->K[s] < 1 || mesh->K[s] + 1 > sfb::kMeshMaxK + 1)
      return sfb::fail(SFB_ERR_INVALID_ARG, "mesh: K outside 1 .. 13 (the raised interval has K + 1 <= 14 points)");
  for (int32_t s = 0; s < mesh->nivals; ++s) {
    const double t = mesh->tau0[s];
    if (!(s == 0 ? t == 0.0 : t > mesh->tau0[s - 1]) || !(t < 1.0))
      return sfb::fail(SFB_ERR_INVALID_ARG, "mesh: tau0 must start at 0, increase strictly and stay below 1");
  }
  if (batch < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "batch < 0");
  return SFB_OK;
}

int64_t mesh_nodes(const sfb_mesh *mesh)
{
  int64_t n = 0;
  for (int32_t s = 0; s < mesh->nivals; ++s) n += mesh->K[s];
  return n;
}

sfb_status resample_check(const sfb_mesh *mesh, int64_t batch, int32_t dim, const double *vals, double *out)
{
  const sfb_status st = mesh_check(mesh, batch);
  if (st != SFB_OK) return st;
  if (dim < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "dim < 0");
  if (batch > 0 && dim > 0 && (!vals || !out)) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  return SFB_OK;
}

sfb_status dyn_error_check(const sfb_mesh *mesh, int64_t batch, int32_t nx, const double *horizon, const double *X, const double *F, double *errs)
{
  const sfb_status st = mesh_check(mesh, batch);
  if (st != SFB_OK) return st;
  if (nx < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "nx < 0");
  if (batch > 0 && (!horizon || !errs || (nx > 0 && (!X || !F)))) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  return SFB_OK;
}

// The per-degree tables (once per device) and the interval lists of the meshes seen (per device and mesh content) live
// on the device, so that an asynchronous launch never outlives what it reads.  A list is a few dozen bytes per
// interval; when a device holds kMeshesKept distinct meshes its lists are dropped after a synchronise of that device.
// The cache's lock is held from the lookup to the end of the launch call (with_cached), so a thread that evicts
// never frees a list between another thread's lookup and its launch; what has been launched is covered by the synchronise.
constexpr size_t kMeshesKept = 64;
using MeshDims = std::array<int32_t, 5>;  // none for the interval lists, (nx, nu) for the mesh functions, the OCP's five for the NLP
struct MeshKey {
  int device;
  std::vector<int32_t> K;
  std::vector<uint64_t> tau0;  // bit patterns
  MeshDims dims;
  bool operator<(const MeshKey &o) const { return std::tie(device, dims, K, tau0) < std::tie(o.device, o.dims, o.K, o.tau0); }
};
MeshKey mesh_key(int device, const sfb_mesh *mesh, const MeshDims &dims)
{
  MeshKey key{device, std::vector<int32_t>(mesh->K, mesh->K + mesh->nivals), std::vector<uint64_t>(mesh->nivals), dims};
  std::memcpy(key.tau0.data(), mesh->tau0, sizeof(double) * mesh->nivals);
  return key;
}
struct MeshEntry {
  sfb::DeviceBlock blk;
  sfb::MeshDevice dev;
};
// what the mesh-function kernels read, per (mesh, nx, nu): nodes, weights, differentiation matrices and mesh_dyn's
// entry -> row table; kept and dropped by the same rule as the interval lists
struct MeshFnEntry {
  sfb::DeviceBlock blk;
  sfb::MeshFnDevice dev;
};
// what the fused NLP kernel reads, per (mesh, dims): the node table, the differentiation matrices and one decode record
// per output double; kept and dropped by the same rule
struct OcpNlpEntry {
  sfb::DeviceBlock blk;
  L::meshfn::OcpNlpTables dev;
  // the records of the Lagrangian Hessian, built by the first sfb_ocp_nlp_hess_batch of this (mesh, dims)
  bool has_hess = false;
  sfb::DeviceBlock hblk;
  L::meshfn::OcpNlpHessTables hdev;
};
struct MeshCache {
  std::mutex mu;
  std::map<int, sfb::DeviceBlock> tables;
  std::map<MeshKey, MeshEntry> meshes;
  std::map<MeshKey, MeshFnEntry> fns;
  std::map<MeshKey, OcpNlpEntry> nlps;
};
MeshCache &cache()
{
  static MeshCache *c = new MeshCache;  // never destroyed: device memory is not freed behind the runtime's back at exit
  return *c;
}

// launch(entry) with the entry of (current device, mesh, dims) in one of the cache's maps, under the cache's lock.  An
// entry that is not there is made by build(entry); when its device already holds kMeshesKept of them, they are dropped
// first, after a synchronise of that device.
template<class Entry, class Build, class Launch>
sfb_status with_cached(std::map<MeshKey, Entry> MeshCache::*which, const sfb_mesh *mesh, const MeshDims &dims, Build &&build, Launch &&launch)
{
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return sfb::hip_fail(e, "hipGetDevice");
  MeshCache &c = cache();
  std::lock_guard<std::mutex> lock(c.mu);
  std::map<MeshKey, Entry> &map = c.*which;
  MeshKey key = mesh_key(device, mesh, dims);
  auto it = map.find(key);
  if (it == map.end()) {
    size_t here = 0;
    for (const auto &m : map) here += m.first.device == device ? 1 : 0;
    if (here >= kMeshesKept) {
      if ((e = hipDeviceSynchronize()) != hipSuccess) return sfb::hip_fail(e, "hipDeviceSynchronize");
      for (auto m = map.begin(); m != map.end();) m = m->first.device == device ? map.erase(m) : std::next(m);
    }
    Entry ent;
    const sfb_status st = build(ent);
    if (st != SFB_OK) return st;
    it = map.emplace(std::move(key), std::move(ent)).first;
  }
  return launch(it->second);
}

std::vector<double> build_tables()
{
  constexpr int S = sfb::kMeshStride, T = S * S;
  std::vector<double> t((size_t)sfb::kMeshMaxK * 3 * T, 0.0);
  for (int K = 1; K <= sfb::kMeshMaxK; ++K) {
    double *Wc = t.data() + (size_t)(K - 1) * 3 * T, *Wo = Wc + T, *I = Wo + T;
    const L::MeshMat wc = L::detail::resample_weights(K, true), wo = L::detail::resample_weights(K, false);
    const L::MeshMat &ius = L::detail::lgr_table(K + 1).Ius;
    for (int j = 0; j < K + 2; ++j) {
      for (int i = 0; i <= K; ++i) Wc[j * S + i] = wc(j, i);
      for (int i = 0; i < K; ++i) Wo[j * S + i] = wo(j, i);
    }
    for (int j = 0; j <= K; ++j)
      for (int i = 0; i <= K; ++i) I[j * S + i] = ius(i, j);
  }
  return t;
}

// the per-degree tables of the current device, made at its first call; under the cache's lock
sfb_status device_tables(const double **out)
{
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return sfb::hip_fail(e, "hipGetDevice");
  std::map<int, sfb::DeviceBlock> &tables = cache().tables;
  auto tb = tables.find(device);
  if (tb == tables.end()) {
    const std::vector<double> t = build_tables();
    sfb::DeviceBlock blk(t.size() * sizeof(double));
    if (blk.error() != hipSuccess) return sfb::hip_fail(blk.error(), "hipMalloc");
    if ((e = sfb::upload(static_cast<double *>(blk.get()), t.data(), t.size())) != hipSuccess) return sfb::hip_fail(e, "mesh tables upload");
    tb = tables.emplace(device, std::move(blk)).first;
  }
  *out = static_cast<const double *>(tb->second.get());
  return SFB_OK;
}

// launch(m) with the device copy of `mesh`, under the cache's lock
template<class Launch>
sfb_status with_device_mesh(const sfb_mesh *mesh, Launch &&launch)
{
  const auto build = [&](MeshEntry &ent) {
    const int32_t n = mesh->nivals;
    std::vector<sfb::MeshIval> iv(n);
    std::vector<int32_t> rows;
    int32_t N = 0, R = 0;
    for (int32_t s = 0; s < n; ++s) {
      const double tauf = s + 1 < n ? mesh->tau0[s + 1] : 1.0;
      iv[s]             = sfb::MeshIval{mesh->K[s], N, R, s + 1 < n ? 1 : 0, (tauf - mesh->tau0[s]) / 2};
      N += mesh->K[s];
      R += mesh->K[s] + 2;
      rows.insert(rows.end(), mesh->K[s] + 2, s);
    }
    sfb::Staging st;
    ent.dev = sfb::MeshDevice{n, N, R, nullptr, nullptr, nullptr};
    st.add(&ent.dev.ivals, (size_t)n, sfb::Staging::In, iv.data());
    st.add(&ent.dev.row_ival, rows.size(), sfb::Staging::In, rows.data());
    return sfb::stage_and_upload(st, ent.blk, "mesh upload");
  };
  return with_cached(&MeshCache::meshes, mesh, MeshDims{}, build, [&](const MeshEntry &ent) {
    sfb::MeshDevice out = ent.dev;
    const sfb_status st = device_tables(&out.tables);
    return st != SFB_OK ? st : launch(out);
  });
}

// per node its time and weight, per interval 2 / (tauf - tau0), and the intervals' differentiation matrices one after the
// other: the expressions of Mesh::interval_nodes / interval_weights / interval_diffmat_unscaled
struct MeshHostTables {
  std::vector<double> tau, w, scale, D;
};
MeshHostTables mesh_host_tables(const sfb_mesh *mesh)
{
  MeshHostTables t;
  const int32_t n = mesh->nivals;
  for (int32_t s = 0; s < n; ++s) {
    const L::detail::LgrTable &T = L::detail::lgr_table(mesh->K[s]);
    const double tau0 = mesh->tau0[s], tauf = s + 1 < n ? mesh->tau0[s + 1] : 1.0, al = (tauf - tau0) / 2;
    t.scale.push_back(2. / (tauf - tau0));
    for (int32_t j = 0; j < mesh->K[s]; ++j) {
      t.tau.push_back(tau0 + al * (T.tau[j] + 1));
      t.w.push_back(al * T.w[j]);
    }
    t.D.insert(t.D.end(), T.Dus.a.begin(), T.Dus.a.end());
  }
  return t;
}

// launch(m) with the device tables of (mesh, nx, nu), under the cache's lock
template<class Launch>
sfb_status with_device_meshfn(const sfb_mesh *mesh, int32_t nx, int32_t nu, Launch &&launch)
{
  const auto build = [&](MeshFnEntry &ent) {
    const int32_t n = mesh->nivals;
    const MeshHostTables t = mesh_host_tables(mesh);
    std::vector<sfb::MeshFnIval> iv(n);
    std::vector<int32_t> node_ival;
    int32_t N = 0, at = 0;
    for (int32_t s = 0; s < n; ++s) {
      iv[s] = sfb::MeshFnIval{mesh->K[s], N, at, 0, t.scale[s]};
      node_ival.insert(node_ival.end(), mesh->K[s], s);
      N += mesh->K[s];
      at += (int32_t)L::detail::lgr_table(mesh->K[s]).Dus.a.size();
    }
    const int64_t nnz = L::meshfn::dyn_pattern(n, mesh->K, nx, nu, nullptr, nullptr);
    std::vector<int32_t> rowptr((size_t)N * nx + 1, 0), colind((size_t)nnz), entry_row((size_t)nnz);
    L::meshfn::dyn_pattern(n, mesh->K, nx, nu, rowptr.data(), colind.data());
    for (int32_t r = 0; r < N * nx; ++r)
      for (int32_t q = rowptr[r]; q < rowptr[r + 1]; ++q) entry_row[q] = r;
    sfb::Staging st;
    sfb::MeshFnDevice &d = ent.dev;
    d.nivals = n; d.N = N; d.nx = nx; d.nu = nu; d.dyn_nnz = nnz;
    st.add(&d.ivals, (size_t)n, sfb::Staging::In, iv.data());
    st.add(&d.tau, t.tau.size(), sfb::Staging::In, t.tau.data());
    st.add(&d.w, t.w.size(), sfb::Staging::In, t.w.data());
    st.add(&d.D, t.D.size(), sfb::Staging::In, t.D.data());
    st.add(&d.node_ival, node_ival.size(), sfb::Staging::In, node_ival.data());
    st.add(&d.dyn_rowptr, rowptr.size(), sfb::Staging::In, rowptr.data());
    st.add(&d.dyn_entry_row, entry_row.size(), sfb::Staging::In, entry_row.data());
    return sfb::stage_and_upload(st, ent.blk, "mesh function tables upload");
  };
  return with_cached(&MeshCache::fns, mesh, MeshDims{nx, nu}, build, [&](const MeshFnEntry &ent) { return launch(ent.dev); });
}

// the node table and the differentiation matrices of a mesh as the NLP law reads them; returns ws
double ocp_nlp_host_tables(const sfb_mesh *mesh, std::vector<L::meshfn::OcpNlpNode> &nodes, std::vector<double> &D)
{
  MeshHostTables t = mesh_host_tables(mesh);
  int32_t N = 0;
  for (int32_t s = 0; s < mesh->nivals; N += mesh->K[s++])
    for (int32_t j = 0; j < mesh->K[s]; ++j) nodes.push_back(L::meshfn::OcpNlpNode{t.tau[N + j], t.w[N + j], t.scale[s], mesh->K[s], N});
  D = std::move(t.D);
  double wmax = 0.0;
  for (const double w : t.w) wmax = std::max(wmax, w);
  return L::meshfn::ocp_nlp_w_scaling(wmax);
}

L::meshfn::OcpDims to_dims(const sfb_ocp_dims *d) { return L::meshfn::OcpDims{d->nx, d->nu, d->nq, d->ncr, d->nce}; }
// for Staging::add_opt: the arrays of an empty segment are left out, given or not
const double *unless_empty(size_t width, const double *a) { return width ? a : nullptr; }

// what every sfb_ocp_nlp_* entry refuses first: the mesh, the batch, the dims, sizes beyond 32-bit indices
sfb_status ocp_dims_check(const sfb_mesh *mesh, int64_t batch, const sfb_ocp_dims *d)
{
  const sfb_status st = mesh_check(mesh, batch);
  if (st != SFB_OK) return st;
  if (!d) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL dims");
  if (d->nx < 1) return sfb::fail(SFB_ERR_INVALID_ARG, "dims: nx < 1");
  if (d->nu < 0 || d->nq < 0 || d->ncr < 0 || d->nce < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "dims: nu, nq, ncr or nce < 0");
  const int64_t N = mesh_nodes(mesh), nz = 1 + (int64_t)d->nx + d->nu;
  int64_t vb[5], cb[5];
  L::meshfn::ocp_nlp_structure(N, to_dims(d), vb, cb);
  const int64_t widest = std::max<int64_t>({d->nx, d->nq, d->ncr});
  const int64_t row_max = std::max<int64_t>({2 + sfb::kMeshMaxK + nz, 2 + (nz - 1) * N, 1 + (int64_t)d->nq + 2 * (int64_t)d->nx});
  if (vb[4] > 0x7fffffff || cb[4] > 0x7fffffff || cb[4] * row_max > 0x7fffffff || N * widest * nz > 0x7fffffff ||
      (int64_t)d->nce * (1 + 2 * (int64_t)d->nx + d->nq) > 0x7fffffff)
    return sfb::fail(SFB_ERR_INVALID_ARG, "ocp nlp: more variables, constraints or entries than 32-bit indices hold");
  return SFB_OK;
}

sfb_status ocp_nlp_check(const sfb_mesh *mesh, const sfb_ocp_dims *d, int64_t batch, const double *x, const double *Ff, const double *dFf,
                         const double *Fg, const double *dFg, const double *Fcr, const double *dFcr, const double *ce, const double *dce,
                         double *g, double *dg_val)
{
  const sfb_status st = ocp_dims_check(mesh, batch, d);
  if (st != SFB_OK) return st;
  const bool want = dg_val != nullptr;
  if ((dFf != nullptr) != want || (d->nq > 0 && (dFg != nullptr) != want) || (d->ncr > 0 && (dFcr != nullptr) != want) ||
      (d->nce > 0 && (dce != nullptr) != want))
    return sfb::fail(SFB_ERR_INVALID_ARG, "the Jacobian inputs and dg_val: all or none");
  if (batch > 0 && (!x || !Ff || !g || (d->nq > 0 && !Fg) || (d->ncr > 0 && !Fcr) || (d->nce > 0 && !ce)))
    return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  return SFB_OK;
}

// launch(entry) with the device tables of (mesh, dims), under the cache's lock; hess: with the Hessian's records as well
template<class Launch>
sfb_status with_device_ocpnlp_entry(const sfb_mesh *mesh, const sfb_ocp_dims *d, bool hess, Launch &&launch)
{
  namespace MF = L::meshfn;
  const MF::OcpDims dm = to_dims(d);
  const auto build = [&](OcpNlpEntry &ent) {
    std::vector<MF::OcpNlpNode> nodes;
    std::vector<double> D;
    const double ws = ocp_nlp_host_tables(mesh, nodes, D);
    int64_t vb[5], cb[5];
    MF::ocp_nlp_structure((int64_t)nodes.size(), dm, vb, cb);
    const int64_t nnz = MF::ocp_nlp_pattern(mesh->nivals, mesh->K, dm, nullptr, nullptr, nullptr);
    std::vector<MF::OcpNlpItem> items((size_t)(cb[4] + nnz));
    MF::ocp_nlp_pattern(mesh->nivals, mesh->K, dm, nullptr, nullptr, items.data());
    sfb::Staging st;
    ent.dev = MF::OcpNlpTables{dm, (int32_t)nodes.size(), cb[4], nnz, ws, nullptr, nullptr, nullptr};
    st.add(&ent.dev.nodes, nodes.size(), sfb::Staging::In, nodes.data());
    st.add(&ent.dev.D, D.size(), sfb::Staging::In, D.data());
    st.add(&ent.dev.items, items.size(), sfb::Staging::In, items.data());
    return sfb::stage_and_upload(st, ent.blk, "ocp nlp tables upload");
  };
  return with_cached(&MeshCache::nlps, mesh, MeshDims{d->nx, d->nu, d->nq, d->ncr, d->nce}, build, [&](OcpNlpEntry &ent) {
    if (hess && !ent.has_hess) {
      const int64_t nnzh = MF::ocp_nlp_hess_pattern(mesh->nivals, mesh->K, dm, nullptr, nullptr, nullptr);
      std::vector<MF::OcpNlpHessItem> items((size_t)nnzh);
      MF::ocp_nlp_hess_pattern(mesh->nivals, mesh->K, dm, nullptr, nullptr, items.data());
      sfb::Staging st;
      ent.hdev = MF::OcpNlpHessTables{dm, ent.dev.N, ent.dev.m, nnzh, ent.dev.ws, ent.dev.nodes, nullptr};
      st.add(&ent.hdev.items, items.size(), sfb::Staging::In, items.data());
      const sfb_status rc = sfb::stage_and_upload(st, ent.hblk, "ocp nlp hessian records upload");
      if (rc != SFB_OK) return rc;
      ent.has_hess = true;
    }
    return launch(ent);
  });
}
template<class Launch>
sfb_status with_device_ocpnlp(const sfb_mesh *mesh, const sfb_ocp_dims *d, Launch &&launch)
{
  return with_device_ocpnlp_entry(mesh, d, false, [&](const OcpNlpEntry &ent) { return launch(ent.dev); });
}

// what the Hessian entries refuse, in the order of ocp_nlp_check: the mesh, the batch, the dims, sizes beyond 32-bit
// indices, a NULL array with work to do (dFcr is not read: the running constraints are not time-scaled)
sfb_status ocp_nlp_hess_check(const sfb_mesh *mesh, const sfb_ocp_dims *d, int64_t batch, const double *x, const double *lambda, const double *sigma,
                              const double *dFf, const double *HLf, const double *dFg, const double *HLg, const double *HLcr, const double *d2theta,
                              const double *d2ce_l, double *hess_val)
{
  const sfb_status st = ocp_dims_check(mesh, batch, d);
  if (st != SFB_OK) return st;
  const int64_t N = mesh_nodes(mesh), nz = 1 + (int64_t)d->nx + d->nu, ne = 1 + 2 * (int64_t)d->nx + d->nq;
  if (N * nz * nz > 0x7fffffff || ne * ne > 0x7fffffff ||
      L::meshfn::ocp_nlp_hess_pattern(mesh->nivals, mesh->K, to_dims(d), nullptr, nullptr, nullptr) > 0x7fffffff)
    return sfb::fail(SFB_ERR_INVALID_ARG, "ocp nlp hessian: more entries than 32-bit indices hold");
  if (batch > 0 && (!x || !lambda || !sigma || !dFf || !HLf || !d2theta || !hess_val || (d->nq > 0 && (!dFg || !HLg)) || (d->ncr > 0 && !HLcr) ||
                    (d->nce > 0 && !d2ce_l)))
    return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  return SFB_OK;
}

// What the three mesh-function entries refuse, in this order: the mesh, the batch, negative sizes, an index range the
// 32-bit patterns cannot hold (meshfn_sizes_check, shared with their pattern entries; dense_rows: integrate's nf rows over
// all the variables count as well), a derivative input without its output (or the reverse), a NULL array with work to do
sfb_status meshfn_sizes_check(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf, bool dense_rows)
{
  const sfb_status st = mesh_check(mesh, batch);
  if (st != SFB_OK) return st;
  if (nx < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "nx < 0");
  if (nu < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "nu < 0");
  if (nf < 0) return sfb::fail(SFB_ERR_INVALID_ARG, "nf < 0");
  const int64_t N = mesh_nodes(mesh), nv = 2 + (int64_t)nx * (N + 1) + (int64_t)nu * N;
  if (nv > 0x7fffffff || N * nf * (2 + (int64_t)sfb::kMeshMaxK + nx + nu) > 0x7fffffff || (dense_rows && (int64_t)nf * (nv + 1) > 0x7fffffff))
    return sfb::fail(SFB_ERR_INVALID_ARG, "mesh function: more variables or entries than 32-bit indices hold");
  return SFB_OK;
}

sfb_status meshfn_check(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf, const double *t0, const double *tf, bool needs_X,
                        const double *X, const double *F, const double *dF, double *out_F, double *out_dF)
{
  const sfb_status st = meshfn_sizes_check(mesh, batch, nx, nu, nf, true);
  if (st != SFB_OK) return st;
  if ((dF == nullptr) != (out_dF == nullptr)) return sfb::fail(SFB_ERR_INVALID_ARG, "dF and the derivative output: both or neither");
  if (batch > 0 && nf > 0 && (!t0 || !tf || !F || !out_F || (needs_X && !X))) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  return SFB_OK;
}

// The tail of every pattern entry, behind its own size checks: `both` when one index array is given without the other,
// nothing to write at all; then the count, which is what the entry returns with
sfb_status pattern_out_check(const int32_t *ptr, const int32_t *ind, const int64_t *nnz, const char *both)
{
  if ((ptr == nullptr) != (ind == nullptr)) return sfb::fail(SFB_ERR_INVALID_ARG, both);
  if (!ptr && !nnz) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  return SFB_OK;
}
sfb_status pattern_done(int64_t *nnz, int64_t n)
{
  if (nnz) *nnz = n;
  return SFB_OK;
}

sfb_status pattern_check(const sfb_mesh *mesh, int32_t nx, int32_t nu, int32_t nf, int32_t *rowptr, int32_t *colind, int64_t *nnz)
{
  const sfb_status st = meshfn_sizes_check(mesh, 0, nx, nu, nf, false);
  return st != SFB_OK ? st : pattern_out_check(rowptr, colind, nnz, "rowptr and colind: both or neither");
}

enum MeshFn { kEval, kIntegrate, kDyn };

sfb_status meshfn_device(MeshFn fn, const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf, int scale, const double *t0,
                         const double *tf, const double *X, const double *F, const double *dF, double *out_F, double *out_dF, void *stream)
{
  sfb_status st = meshfn_check(mesh, batch, nx, nu, nf, t0, tf, fn == kDyn, X, F, dF, out_F, out_dF);
  if (st != SFB_OK) return st;
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0 || nf == 0) return SFB_OK;
  return with_device_meshfn(mesh, nx, nu, [&](const sfb::MeshFnDevice &m) {
    sfb::MeshFnArgs a{};
    a.m = m; a.batch = batch; a.nf = nf; a.scale = scale ? 1 : 0; a.t0 = t0; a.tf = tf; a.X = X; a.F = F; a.dF = dF; a.out_F = out_F; a.out_dF = out_dF;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e  = fn == kEval ? sfb::mesh_eval_launch(a, s) : fn == kIntegrate ? sfb::mesh_integrate_launch(a, s) : sfb::mesh_dyn_launch(a, s);
    return e != hipSuccess ? sfb::hip_fail(e, "mesh function kernel launch") : SFB_OK;
  });
}

sfb_status meshfn_host(MeshFn fn, const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf, int scale, const double *t0,
                       const double *tf, const double *X, const double *F, const double *dF, double *out_F, double *out_dF)
{
  sfb_status st = meshfn_check(mesh, batch, nx, nu, nf, t0, tf, fn == kDyn, X, F, dF, out_F, out_dF);
  if (st != SFB_OK) return st;
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0 || nf == 0) return SFB_OK;
  const size_t B = (size_t)batch, N = (size_t)mesh_nodes(mesh), nz = 1 + (size_t)nx + (size_t)nu, nv = 2 + (size_t)nx * (N + 1) + (size_t)nu * N;
  const size_t rows = fn == kIntegrate ? (size_t)nf : N * (size_t)nf;
  const size_t dcount = fn == kIntegrate ? (size_t)nf * nv
                        : fn == kEval    ? N * (size_t)nf * (2 + (size_t)nx + (size_t)nu)
                                         : (size_t)L::meshfn::dyn_pattern(mesh->nivals, mesh->K, nx, nu, nullptr, nullptr);
  using S = sfb::Staging;
  S s;
  double *d0, *d1, *dX, *dFv, *ddF, *doF, *dodF;
  s.add(&d0, B, S::In, t0); s.add(&d1, B, S::In, tf);
  s.add_opt(&dX, B * (N + 1) * (size_t)nx, S::In, X);  // (mesh_dyn alone is given one)
  s.add(&dFv, B * N * (size_t)nf, S::In, F);
  s.add_opt(&ddF, B * N * (size_t)nf * nz, S::In, dF);
  s.add(&doF, B * rows, S::Out, out_F);
  s.add_opt(&dodF, B * dcount, S::Out, out_dF);
  return sfb::staged_call(s, "mesh function host entry",
                          [&] { return meshfn_device(fn, mesh, batch, nx, nu, nf, scale, d0, d1, dX, dFv, ddF, doF, dodF, nullptr); });
}

}  // namespace

extern "C" {

sfb_status sfb_mesh_eval_pattern(const sfb_mesh *mesh, int32_t nx, int32_t nu, int32_t nf, int32_t *rowptr, int32_t *colind, int64_t *nnz)
{
  const sfb_status st = pattern_check(mesh, nx, nu, nf, rowptr, colind, nnz);
  if (st != SFB_OK) return st;
  return pattern_done(nnz, L::meshfn::eval_pattern(mesh_nodes(mesh), nx, nu, nf, rowptr, colind));
}

sfb_status sfb_mesh_dyn_pattern(const sfb_mesh *mesh, int32_t nx, int32_t nu, int32_t *rowptr, int32_t *colind, int64_t *nnz)
{
  const sfb_status st = pattern_check(mesh, nx, nu, nx, rowptr, colind, nnz);
  if (st != SFB_OK) return st;
  return pattern_done(nnz, L::meshfn::dyn_pattern(mesh->nivals, mesh->K, nx, nu, rowptr, colind));
}

sfb_status sfb_mesh_eval_batch(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf, int scale, const double *t0, const double *tf,
                               const double *F, const double *dF, double *out_F, double *out_dF_val, void *stream)
{
  return meshfn_device(kEval, mesh, batch, nx, nu, nf, scale, t0, tf, nullptr, F, dF, out_F, out_dF_val, stream);
}
sfb_status sfb_mesh_integrate_batch(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf, const double *t0, const double *tf,
                                    const double *F, const double *dF, double *out_F, double *out_dF, void *stream)
{
  return meshfn_device(kIntegrate, mesh, batch, nx, nu, nf, 0, t0, tf, nullptr, F, dF, out_F, out_dF, stream);
}
sfb_status sfb_mesh_dyn_batch(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, const double *t0, const double *tf, const double *X,
                              const double *F, const double *dF, double *out_F, double *out_dF_val, void *stream)
{
  return meshfn_device(kDyn, mesh, batch, nx, nu, nx, 0, t0, tf, X, F, dF, out_F, out_dF_val, stream);
}
sfb_status sfb_mesh_eval_batch_host(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf, int scale, const double *t0,
                                    const double *tf, const double *F, const double *dF, double *out_F, double *out_dF_val)
{
  return meshfn_host(kEval, mesh, batch, nx, nu, nf, scale, t0, tf, nullptr, F, dF, out_F, out_dF_val);
}
sfb_status sfb_mesh_integrate_batch_host(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf, const double *t0, const double *tf,
                                         const double *F, const double *dF, double *out_F, double *out_dF)
{
  return meshfn_host(kIntegrate, mesh, batch, nx, nu, nf, 0, t0, tf, nullptr, F, dF, out_F, out_dF);
}
sfb_status sfb_mesh_dyn_batch_host(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, const double *t0, const double *tf, const double *X,
                                   const double *F, const double *dF, double *out_F, double *out_dF_val)
{
  return meshfn_host(kDyn, mesh, batch, nx, nu, nx, 0, t0, tf, X, F, dF, out_F, out_dF_val);
}

sfb_status sfb_ocp_nlp_structure(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int64_t var_beg[5], int64_t con_beg[5])
{
  const sfb_status st = ocp_dims_check(mesh, 0, dims);
  if (st != SFB_OK) return st;
  if (!var_beg || !con_beg) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  L::meshfn::ocp_nlp_structure(mesh_nodes(mesh), to_dims(dims), var_beg, con_beg);
  return SFB_OK;
}

sfb_status sfb_ocp_nlp_pattern(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int32_t *rowptr, int32_t *colind, int64_t *nnz)
{
  sfb_status st = ocp_dims_check(mesh, 0, dims);
  if (st == SFB_OK) st = pattern_out_check(rowptr, colind, nnz, "rowptr and colind: both or neither");
  if (st != SFB_OK) return st;
  return pattern_done(nnz, L::meshfn::ocp_nlp_pattern(mesh->nivals, mesh->K, to_dims(dims), rowptr, colind, nullptr));
}

sfb_status sfb_ocp_nlp_bounds(const sfb_mesh *mesh, const sfb_ocp_dims *dims, const double *crl, const double *cru, const double *cel,
                              const double *ceu, double *xl, double *xu, double *gl, double *gu, double *w_scaling)
{
  const sfb_status st = ocp_dims_check(mesh, 0, dims);
  if (st != SFB_OK) return st;
  if (((gl || gu) && ((dims->ncr > 0 && (!crl || !cru)) || (dims->nce > 0 && (!cel || !ceu)))))
    return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  std::vector<L::meshfn::OcpNlpNode> nodes;
  std::vector<double> D;
  const double ws = ocp_nlp_host_tables(mesh, nodes, D);
  int64_t vb[5], cb[5];
  L::meshfn::ocp_nlp_structure((int64_t)nodes.size(), to_dims(dims), vb, cb);
  if (w_scaling) *w_scaling = ws;
  L::meshfn::ocp_nlp_bounds(to_dims(dims), (int64_t)nodes.size(), nodes.data(), ws, crl, cru, cel, ceu, xl, xu, gl, gu);
  return SFB_OK;
}

sfb_status sfb_ocp_nlp_batch(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int64_t batch, const double *x, const double *Ff, const double *dFf,
                             const double *Fg, const double *dFg, const double *Fcr, const double *dFcr, const double *ce, const double *dce,
                             double *g, double *dg_val, void *stream)
{
  sfb_status st = ocp_nlp_check(mesh, dims, batch, x, Ff, dFf, Fg, dFg, Fcr, dFcr, ce, dce, g, dg_val);
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;  // nothing to write: no device is asked for
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  return with_device_ocpnlp(mesh, dims, [&](const L::meshfn::OcpNlpTables &T) {
    int64_t vb[5], cb[5];
    L::meshfn::ocp_nlp_structure(T.N, T.d, vb, cb);
    sfb::OcpNlpArgs a{};
    a.T = T; a.batch = batch; a.n = vb[4]; a.x = x; a.Ff = Ff; a.dFf = dFf; a.Fg = Fg; a.dFg = dFg; a.Fcr = Fcr; a.dFcr = dFcr; a.ce = ce; a.dce = dce;
    a.g = g; a.dg = dg_val;
    const hipError_t e = sfb::ocp_nlp_launch(a, static_cast<hipStream_t>(stream));
    return e != hipSuccess ? sfb::hip_fail(e, "ocp_nlp_kernel launch") : SFB_OK;
  });
}

sfb_status sfb_ocp_nlp_batch_host(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int64_t batch, const double *x, const double *Ff, const double *dFf,
                                  const double *Fg, const double *dFg, const double *Fcr, const double *dFcr, const double *ce, const double *dce,
                                  double *g, double *dg_val)
{
  sfb_status st = ocp_nlp_check(mesh, dims, batch, x, Ff, dFf, Fg, dFg, Fcr, dFcr, ce, dce, g, dg_val);
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;  // nothing to write: no device is asked for
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  const size_t B = (size_t)batch, N = (size_t)mesh_nodes(mesh), nx = (size_t)dims->nx, nq = (size_t)dims->nq, ncr = (size_t)dims->ncr,
               nce = (size_t)dims->nce, nz = 1 + nx + (size_t)dims->nu, ne = 1 + 2 * nx + nq;
  int64_t vb[5], cb[5];
  L::meshfn::ocp_nlp_structure((int64_t)N, to_dims(dims), vb, cb);
  const size_t nnz = (size_t)L::meshfn::ocp_nlp_pattern(mesh->nivals, mesh->K, to_dims(dims), nullptr, nullptr, nullptr);
  using S = sfb::Staging;
  S s;
  double *dx, *d1, *d2, *d3, *d4, *d5, *d6, *d7, *d8, *dg, *ddg;
  s.add(&dx, B * (size_t)vb[4], S::In, x);
  s.add(&d1, B * N * nx, S::In, Ff);
  s.add_opt(&d2, B * N * nx * nz, S::In, dFf);
  s.add_opt(&d3, B * N * nq, S::In, unless_empty(nq, Fg)); s.add_opt(&d4, B * N * nq * nz, S::In, unless_empty(nq, dFg));
  s.add_opt(&d5, B * N * ncr, S::In, unless_empty(ncr, Fcr)); s.add_opt(&d6, B * N * ncr * nz, S::In, unless_empty(ncr, dFcr));
  s.add_opt(&d7, B * nce, S::In, unless_empty(nce, ce)); s.add_opt(&d8, B * nce * ne, S::In, unless_empty(nce, dce));
  s.add(&dg, B * (size_t)cb[4], S::Out, g);
  s.add_opt(&ddg, B * nnz, S::Out, dg_val);
  return sfb::staged_call(s, "sfb_ocp_nlp_batch_host",
                          [&] { return sfb_ocp_nlp_batch(mesh, dims, batch, dx, d1, d2, d3, d4, d5, d6, d7, d8, dg, ddg, nullptr); });
}

sfb_status sfb_ocp_nlp_hess_pattern(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int32_t *colptr, int32_t *rowind, int64_t *nnz)
{
  sfb_status st = ocp_dims_check(mesh, 0, dims);
  if (st == SFB_OK) st = pattern_out_check(colptr, rowind, nnz, "colptr and rowind: both or neither");
  if (st != SFB_OK) return st;
  const int64_t n = L::meshfn::ocp_nlp_hess_pattern(mesh->nivals, mesh->K, to_dims(dims), nullptr, nullptr, nullptr);
  if (n > 0x7fffffff) return sfb::fail(SFB_ERR_INVALID_ARG, "ocp nlp hessian: more entries than 32-bit indices hold");
  if (colptr) L::meshfn::ocp_nlp_hess_pattern(mesh->nivals, mesh->K, to_dims(dims), colptr, rowind, nullptr);
  return pattern_done(nnz, n);
}

sfb_status sfb_ocp_nlp_hess_batch(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int64_t batch, const double *x, const double *lambda,
                                  const double *sigma, const double *dFf, const double *HLf, const double *dFg, const double *HLg, const double *dFcr,
                                  const double *HLcr, const double *d2theta, const double *d2ce_l, double *hess_val, void *stream)
{
  (void)dFcr;
  sfb_status st = ocp_nlp_hess_check(mesh, dims, batch, x, lambda, sigma, dFf, HLf, dFg, HLg, HLcr, d2theta, d2ce_l, hess_val);
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;  // nothing to write: no device is asked for
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  return with_device_ocpnlp_entry(mesh, dims, true, [&](const OcpNlpEntry &ent) {
    int64_t vb[5], cb[5];
    L::meshfn::ocp_nlp_structure(ent.hdev.N, ent.hdev.d, vb, cb);
    sfb::OcpNlpHessArgs a{};
    a.T = ent.hdev; a.batch = batch; a.n = vb[4]; a.x = x; a.lambda = lambda; a.sigma = sigma; a.dFf = dFf; a.HLf = HLf; a.dFg = dFg; a.HLg = HLg;
    a.HLcr = HLcr; a.d2theta = d2theta; a.d2ce_l = d2ce_l; a.hess = hess_val;
    const hipError_t e = sfb::ocp_nlp_hess_launch(a, static_cast<hipStream_t>(stream));
    return e != hipSuccess ? sfb::hip_fail(e, "ocp_nlp_hess_kernel launch") : SFB_OK;
  });
}

sfb_status sfb_ocp_nlp_hess_batch_host(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int64_t batch, const double *x, const double *lambda,
                                       const double *sigma, const double *dFf, const double *HLf, const double *dFg, const double *HLg,
                                       const double *dFcr, const double *HLcr, const double *d2theta, const double *d2ce_l, double *hess_val)
{
  (void)dFcr;
  sfb_status st = ocp_nlp_hess_check(mesh, dims, batch, x, lambda, sigma, dFf, HLf, dFg, HLg, HLcr, d2theta, d2ce_l, hess_val);
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;  // nothing to write: no device is asked for
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  const size_t B = (size_t)batch, N = (size_t)mesh_nodes(mesh), nx = (size_t)dims->nx, nq = (size_t)dims->nq, ncr = (size_t)dims->ncr,
               nce = (size_t)dims->nce, nz = 1 + nx + (size_t)dims->nu, ne = 1 + 2 * nx + nq;
  int64_t vb[5], cb[5];
  L::meshfn::ocp_nlp_structure((int64_t)N, to_dims(dims), vb, cb);
  const size_t nnz = (size_t)L::meshfn::ocp_nlp_hess_pattern(mesh->nivals, mesh->K, to_dims(dims), nullptr, nullptr, nullptr);
  using S = sfb::Staging;
  S s;
  double *dx, *dl, *ds, *d1, *d2, *d3, *d4, *d5, *d6, *d7, *dh;
  s.add(&dx, B * (size_t)vb[4], S::In, x);
  s.add(&dl, B * (size_t)cb[4], S::In, lambda);
  s.add(&ds, B, S::In, sigma);
  s.add(&d1, B * N * nx * nz, S::In, dFf);
  s.add(&d2, B * N * nz * nz, S::In, HLf);
  s.add_opt(&d3, B * N * nq * nz, S::In, unless_empty(nq, dFg)); s.add_opt(&d4, B * N * nz * nz, S::In, unless_empty(nq, HLg));
  s.add_opt(&d5, B * N * nz * nz, S::In, unless_empty(ncr, HLcr));
  s.add(&d6, B * ne * ne, S::In, d2theta);
  s.add_opt(&d7, B * ne * ne, S::In, unless_empty(nce, d2ce_l));
  s.add(&dh, B * nnz, S::Out, hess_val);
  return sfb::staged_call(s, "sfb_ocp_nlp_hess_batch_host", [&] {
    return sfb_ocp_nlp_hess_batch(mesh, dims, batch, dx, dl, ds, d1, d2, d3, d4, nullptr, d5, d6, d7, dh, nullptr);
  });
}

sfb_status sfb_mesh_resample_batch(const sfb_mesh *mesh, int64_t batch, int32_t dim, int extend, const double *vals, double *out, void *stream)
{
  sfb_status st = resample_check(mesh, batch, dim, vals, out);
  if (st != SFB_OK) return st;
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0 || dim == 0) return SFB_OK;
  return with_device_mesh(mesh, [&](const sfb::MeshDevice &m) {
    sfb::MeshResampleArgs a{};
    a.m = m; a.batch = batch; a.dim = dim; a.extend = extend ? 1 : 0; a.vals = vals; a.out = out;
    const hipError_t e = sfb::mesh_resample_launch(a, static_cast<hipStream_t>(stream));
    return e != hipSuccess ? sfb::hip_fail(e, "mesh_resample_kernel launch") : SFB_OK;
  });
}

sfb_status sfb_mesh_dyn_error_batch(const sfb_mesh *mesh, int64_t batch, int32_t nx, const double *horizon, const double *X, const double *F,
                                    double *errs, void *stream)
{
  sfb_status st = dyn_error_check(mesh, batch, nx, horizon, X, F, errs);
  if (st != SFB_OK) return st;
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  return with_device_mesh(mesh, [&](const sfb::MeshDevice &m) {
    sfb::MeshDynErrorArgs a{};
    a.m = m; a.batch = batch; a.nx = nx; a.horizon = horizon; a.X = X; a.F = F; a.errs = errs;
    const hipError_t e = sfb::mesh_dyn_error_launch(a, static_cast<hipStream_t>(stream));
    return e != hipSuccess ? sfb::hip_fail(e, "mesh_dyn_error_kernel launch") : SFB_OK;
  });
}

sfb_status sfb_mesh_raised_nodes(const sfb_mesh *mesh, double *tau)
{
  const sfb_status st = mesh_check(mesh, 0);
  if (st != SFB_OK) return st;
  if (!tau) return sfb::fail(SFB_ERR_INVALID_ARG, "NULL array");
  for (int32_t s = 0; s < mesh->nivals; ++s) {
    const std::vector<double> &x = L::detail::lgr_table(mesh->K[s] + 1).tau;  // K + 1 LGR points and +1
    const double tau0 = mesh->tau0[s], al = ((s + 1 < mesh->nivals ? mesh->tau0[s + 1] : 1.0) - tau0) / 2;
    for (const double v : x) *tau++ = tau0 + al * (v + 1);
  }
  return SFB_OK;
}

sfb_status sfb_mesh_resample_batch_host(const sfb_mesh *mesh, int64_t batch, int32_t dim, int extend, const double *vals, double *out)
{
  sfb_status st = resample_check(mesh, batch, dim, vals, out);
  if (st != SFB_OK) return st;
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0 || dim == 0) return SFB_OK;
  const size_t B = (size_t)batch, D = (size_t)dim, N = (size_t)mesh_nodes(mesh), R = N + 2 * (size_t)mesh->nivals;
  using S = sfb::Staging;
  S s;
  double *dv, *dout;
  s.add(&dv, B * (N + (extend ? 1 : 0)) * D, S::In, vals); s.add(&dout, B * R * D, S::Out, out);
  return sfb::staged_call(s, "sfb_mesh_resample_batch_host", [&] { return sfb_mesh_resample_batch(mesh, batch, dim, extend, dv, dout, nullptr); });
}

sfb_status sfb_mesh_dyn_error_batch_host(const sfb_mesh *mesh, int64_t batch, int32_t nx, const double *horizon, const double *X, const double *F,
                                         double *errs)
{
  sfb_status st = dyn_error_check(mesh, batch, nx, horizon, X, F, errs);
  if (st != SFB_OK) return st;
  st = sfb::require_device();
  if (st != SFB_OK) return st;
  if (batch == 0) return SFB_OK;
  const size_t B = (size_t)batch, D = (size_t)nx, R = (size_t)mesh_nodes(mesh) + 2 * (size_t)mesh->nivals;
  using S = sfb::Staging;
  S s;
  double *dh, *dX, *dF, *de;
  s.add(&dh, B, S::In, horizon); s.add(&dX, B * R * D, S::In, X); s.add(&dF, B * R * D, S::In, F); s.add(&de, B * (size_t)mesh->nivals, S::Out, errs);
  return sfb::staged_call(s, "sfb_mesh_dyn_error_batch_host", [&] { return sfb_mesh_dyn_error_batch(mesh, batch, nx, dh, dX, dF, de, nullptr); });
}

}  // extern "C"
