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
//
// mesh_eval / mesh_integrate / mesh_dyn (include/sfb.h: sfb_mesh_eval_batch, ...; model-free: the caller's model values
// F [batch][N][nf] and Jacobians dF [batch][N][nf][1 + nx + nu] come in): one lane per output double, the entry index
// fastest and the agent slowest, so a wave stores 512 contiguous bytes.  Every entry is one call of the law of
// mesh_function.hpp (namespace meshfn), the functions the host front calls.  The CSR values of mesh_eval have rows of one
// length and are decoded by division; those of mesh_dyn go entry -> row through the per-(mesh, nx, nu) table
// dyn_entry_row (4 bytes per entry, shared by every agent: cache resident) and row -> position through dyn_rowptr, and
// read the row's own block of dF contiguously.  mesh_integrate's t0, tf and F lanes loop over the nodes in node order
// (the host's order of summation); its x and u lanes do one product.  No LDS, plain loads and stores.
//
// ocp_nlp (include/sfb.h: sfb_ocp_nlp_batch): g and the CSR values of dg_dx of the collocation NLP in one launch, every
// output double written once and no t0 entry computed.  The outputs of one agent are m + nnz items (the rows of g, then
// the entries of the pattern); the host builds one 16-byte decode record per item, once per (mesh, dims).  A lane takes
// one item, decodes it once (record -> node table -> mesh coefficient) and then walks kNlpAgents agents with it; the
// lanes of a wave hold consecutive items, so every store instruction of a wave writes 512 contiguous bytes of one
// agent.  Every value is meshfn::ocp_nlp_value, the function the host front calls.
//
// ocp_nlp_hess (sfb_ocp_nlp_hess_batch): the values of sigma d2f + d2g(lambda) over the upper-triangle CSC pattern, in the
// same shape: a lane takes one of the nnzH records (a gather: a node and a position in its (t | x | u) block, a position
// in the end block, or both), decodes it once and walks kNlpHessAgents agents; consecutive lanes hold consecutive entries
// of one agent.  Every value is meshfn::ocp_nlp_hess_value with its fixed order of summation (nodes ascending; f, g, cr;
// theta, ce): the tf-row lanes sum JL = sum_j lambda_j dF(j, c) themselves, and the (tf, tf) lane loops over all N nodes.
// Every output double is written once; no LDS, plain loads and stores.
#include "mesh_kernel.h"

#include <cstdlib>

#include "knobs.h"

#include "../../include/smooth_feedback_amd/dyn_error.hpp"
#include "../../include/smooth_feedback_amd/mesh_function.hpp"

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

namespace MF = smooth_feedback_amd::meshfn;

// lane t -> (agent, entry of that agent), by a 32-bit division when both fit (wave-uniform); at the benchmark shape the
// kernels measured the same with the 64-bit division alone
__device__ inline void agent_entry(const int64_t t, const int64_t per, int64_t &b, int &e)
{
  if (((uint64_t)t | (uint64_t)per) >> 32 == 0) {
    const uint32_t q = (uint32_t)t / (uint32_t)per;
    b = q;
    e = (int)((uint32_t)t - q * (uint32_t)per);
  } else {
    b = t / per;
    e = (int)(t - b * per);
  }
}

__global__ void __launch_bounds__(256) mesh_eval_F_kernel(const MeshFnArgs a)
{
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per   = a.m.N * a.nf;
  if (t >= a.batch * per) return;
  int64_t b;
  int e;
  agent_entry(t, per, b, e);
  a.out_F[t] = MF::eval_F(a.scale ? a.m.w[e / a.nf] : 1., a.F[t]);
}

__global__ void __launch_bounds__(256) mesh_eval_dF_kernel(const MeshFnArgs a)
{
  const int per   = 2 + a.m.nx + a.m.nu, rows = a.m.N * a.nf;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.batch * rows * per) return;
  int64_t b;
  int e;
  agent_entry(t, (int64_t)rows * per, b, e);
  const int row = e / per, p = e - row * per;  // (node, output) and the position in its row
  const int i   = row / a.nf;
  const double w = a.scale ? a.m.w[i] : 1., tau = a.m.tau[i];
  const double *df = a.dF + (b * rows + row) * (per - 1);
  a.out_dF[t] = p == 0 ? MF::eval_dt0(w, tau, df[0]) : p == 1 ? MF::eval_dtf(w, tau, df[0]) : MF::eval_dz(w, df[p - 1]);
}

__global__ void __launch_bounds__(256) mesh_integrate_kernel(const MeshFnArgs a)
{
  const int nx = a.m.nx, nu = a.m.nu, nf = a.nf, N = a.m.N, nz = 1 + nx + nu;
  const int64_t nv  = 2 + (int64_t)nx * (N + 1) + (int64_t)nu * N;
  const int64_t per = a.dF ? nf * (nv + 1) : nf;  // per agent: nf values, then the nf x nv derivative block
  const int64_t t   = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.batch * per) return;
  int64_t b;
  int q;
  agent_entry(t, per, b, q);
  const double h  = a.tf[b] - a.t0[b];
  const double *Fb = a.F + b * N * nf;
  if (q < nf) {
    double acc = 0.0;
    for (int i = 0; i < N; ++i) MF::integrate_F_add(acc, a.m.w[i], h, Fb[(int64_t)i * nf + q]);
    a.out_F[b * nf + q] = acc;
    return;
  }
  const int e = q - nf;
  const int r = e / (int)nv;
  const int64_t c = e - r * (int)nv;
  const double *dfb = a.dF + (b * N * nf + r) * nz;  // node i's row r at dfb + i nf nz
  double v = 0.0;
  if (c < 2) {
    for (int i = 0; i < N; ++i) {
      const double f = Fb[(int64_t)i * nf + r], dft = dfb[(int64_t)i * nf * nz];
      if (c == 0) MF::integrate_dt0_add(v, a.m.w[i], h, a.m.tau[i], f, dft);
      else MF::integrate_dtf_add(v, a.m.w[i], h, a.m.tau[i], f, dft);
    }
  } else if (c < 2 + (int64_t)nx * N) {
    const int i = (int)((c - 2) / nx), k = (int)((c - 2) - (int64_t)i * nx);
    v           = MF::integrate_dz(a.m.w[i], h, dfb[(int64_t)i * nf * nz + 1 + k]);
  } else if (c >= 2 + (int64_t)nx * (N + 1)) {
    const int64_t cu = c - 2 - (int64_t)nx * (N + 1);
    const int i = (int)(cu / nu), k = (int)(cu - (int64_t)i * nu);
    v           = MF::integrate_dz(a.m.w[i], h, dfb[(int64_t)i * nf * nz + 1 + nx + k]);
  }  // (the columns of x_N stay zero)
  a.out_dF[b * nf * nv + e] = v;
}

__global__ void __launch_bounds__(256) mesh_dyn_F_kernel(const MeshFnArgs a)
{
  const int nx = a.m.nx, N = a.m.N;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.batch * N * nx) return;
  int64_t b;
  int e;
  agent_entry(t, (int64_t)N * nx, b, e);
  const int i = e / nx, d = e - i * nx;
  const MeshFnIval iv = a.m.ivals[a.m.node_ival[i]];
  const int j         = i - iv.M;
  const double *x     = a.X + (b * (N + 1) + iv.M) * nx + d;
  a.out_F[t] = MF::dyn_F(iv.K, a.m.w[i], a.tf[b] - a.t0[b], iv.alpha, a.m.D + iv.Doff + j * (iv.K + 1), a.F[t], x, nx);
}

__global__ void __launch_bounds__(256) mesh_dyn_dF_kernel(const MeshFnArgs a)
{
  const int nx = a.m.nx, nu = a.m.nu, N = a.m.N, nz = 1 + nx + nu;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.batch * a.m.dyn_nnz) return;
  int64_t b;
  int e;
  agent_entry(t, a.m.dyn_nnz, b, e);
  const int row   = a.m.dyn_entry_row[e];
  const int p     = e - a.m.dyn_rowptr[row];
  const int i = row / nx, d = row - i * nx;
  const MeshFnIval iv = a.m.ivals[a.m.node_ival[i]];
  const int j         = i - iv.M;
  int kind, idx;
  MF::dyn_decode(p, j, iv.K, nx, kind, idx);
  const double w = a.m.w[i], tau = a.m.tau[i], h = a.tf[b] - a.t0[b];
  const double *Dcol = a.m.D + iv.Doff + j * (iv.K + 1);
  const int64_t fr   = (b * N + i) * nx + d;
  const double *df   = a.dF + fr * nz;
  double v;
  if (kind == 0) v = MF::dyn_dt0(w, h, tau, a.F[fr], df[0]);
  else if (kind == 1) v = MF::dyn_dtf(w, h, tau, a.F[fr], df[0]);
  else if (kind == 2) v = MF::dyn_coef(w, iv.alpha, Dcol[idx]);
  else if (kind == 3) v = MF::dyn_own(w, h, iv.alpha, Dcol[j], df[1 + idx], idx == d);
  else v = MF::dyn_du(w, h, df[1 + nx + idx]);
  a.out_dF[t] = v;
}

constexpr int kNlpAgents = 8;  // agents a lane walks with one decoded item (the knob SFB_NLP_AGENTS overrides it for A/B runs)

__global__ void __launch_bounds__(256) ocp_nlp_kernel(const OcpNlpArgs a)
{
  const MF::OcpNlpTables &T = a.T;
  const int64_t m = T.m, items = a.dg ? m + T.nnz : m;
  const int64_t b0 = (int64_t)blockIdx.x * a.agents;
  const int64_t b1 = b0 + a.agents < a.batch ? b0 + a.agents : a.batch;
  const int64_t N = T.N, nz = 1 + T.d.nx + T.d.nu;
  const int64_t sFf = N * T.d.nx, sFg = N * T.d.nq, sFcr = N * T.d.ncr, sdce = (int64_t)T.d.nce * (1 + 2 * T.d.nx + T.d.nq);
  for (int64_t it = (int64_t)blockIdx.y * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.y * 256) {
    const MF::OcpNlpLane L = MF::ocp_nlp_decode(T, T.items[it]);
    const bool row = it < m;
    double *out    = row ? a.g + b0 * m + it : a.dg + b0 * T.nnz + (it - m);
    const int64_t so = row ? m : T.nnz;
    for (int64_t b = b0; b < b1; ++b, out += so) {
      const MF::OcpNlpAgent ag{a.x + b * a.n, a.Ff + b * sFf, a.dFf + b * sFf * nz, a.Fg + b * sFg, a.dFg + b * sFg * nz,
                               a.Fcr + b * sFcr, a.dFcr + b * sFcr * nz, a.ce + b * T.d.nce, a.dce + b * sdce};
      *out = MF::ocp_nlp_value(T, L, ag);
    }
  }
}

constexpr int kNlpHessAgents = 4;  // agents a lane walks with one decoded record (the knob SFB_NLP_HESS_AGENTS overrides it for A/B runs)

__global__ void __launch_bounds__(256) ocp_nlp_hess_kernel(const OcpNlpHessArgs a)
{
  const MF::OcpNlpHessTables &T = a.T;
  const int64_t b0 = (int64_t)blockIdx.x * a.agents;
  const int64_t b1 = b0 + a.agents < a.batch ? b0 + a.agents : a.batch;
  const int64_t N = T.N, nz = 1 + T.d.nx + T.d.nu, ne = 1 + 2 * T.d.nx + T.d.nq;
  const int64_t sdF = N * nz, sHL = N * nz * nz, sE = ne * ne;
  for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < T.nnz; e += (int64_t)gridDim.y * 256) {
    const MF::OcpNlpHessLane L = MF::ocp_nlp_hess_decode(T, T.items[e]);
    double *out = a.hess + b0 * T.nnz + e;
    for (int64_t b = b0; b < b1; ++b, out += T.nnz) {
      const MF::OcpNlpHessAgent ag{a.x + b * a.n, a.lambda + b * T.m, a.sigma[b], a.dFf + b * sdF * T.d.nx, a.HLf + b * sHL,
                                   a.dFg + b * sdF * T.d.nq, a.HLg + b * sHL, a.HLcr + b * sHL, a.d2theta + b * sE, a.d2ce_l + b * sE};
      *out = MF::ocp_nlp_hess_value(T, L, ag);
    }
  }
}

template<class Kern>
hipError_t lane_launch(Kern kern, const int64_t total, const MeshFnArgs &a, hipStream_t stream)
{
  if (total <= 0) return hipSuccess;
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t mesh_eval_launch(const MeshFnArgs &a, hipStream_t stream)
{
  const int64_t rows = a.batch * a.m.N * a.nf;
  const hipError_t e = lane_launch(mesh_eval_F_kernel, rows, a, stream);
  if (e != hipSuccess || !a.dF) return e;
  return lane_launch(mesh_eval_dF_kernel, rows * (2 + a.m.nx + a.m.nu), a, stream);
}

hipError_t mesh_integrate_launch(const MeshFnArgs &a, hipStream_t stream)
{
  const int64_t nv = 2 + (int64_t)a.m.nx * (a.m.N + 1) + (int64_t)a.m.nu * a.m.N;
  return lane_launch(mesh_integrate_kernel, a.batch * (a.dF ? a.nf * (nv + 1) : a.nf), a, stream);
}

hipError_t mesh_dyn_launch(const MeshFnArgs &a, hipStream_t stream)
{
  const hipError_t e = lane_launch(mesh_dyn_F_kernel, a.batch * a.m.N * a.m.nx, a, stream);
  if (e != hipSuccess || !a.dF) return e;
  return lane_launch(mesh_dyn_dF_kernel, a.batch * a.m.dyn_nnz, a, stream);
}

hipError_t ocp_nlp_launch(const OcpNlpArgs &args, hipStream_t stream)
{
  OcpNlpArgs a = args;
  a.agents     = kNlpAgents;
  if (const char *k = knob("SFB_NLP_AGENTS")) {
    const int v = std::atoi(k);
    if (v >= 1 && v <= 1024) a.agents = v;
  }
  const int64_t items = a.dg ? a.T.m + a.T.nnz : a.T.m;
  if (a.batch <= 0 || items <= 0) return hipSuccess;
  const int64_t groups = (a.batch + a.agents - 1) / a.agents, chunks = (items + 255) / 256;
  if (groups > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ocp_nlp_kernel, dim3((unsigned)groups, (unsigned)(chunks < 65535 ? chunks : 65535)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t ocp_nlp_hess_launch(const OcpNlpHessArgs &args, hipStream_t stream)
{
  OcpNlpHessArgs a = args;
  a.agents         = kNlpHessAgents;
  if (const char *k = knob("SFB_NLP_HESS_AGENTS")) {
    const int v = std::atoi(k);
    if (v >= 1 && v <= 1024) a.agents = v;
  }
  if (a.batch <= 0 || a.T.nnz <= 0) return hipSuccess;
  const int64_t groups = (a.batch + a.agents - 1) / a.agents, chunks = (a.T.nnz + 255) / 256;
  if (groups > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ocp_nlp_hess_kernel, dim3((unsigned)groups, (unsigned)(chunks < 65535 ? chunks : 65535)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

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
