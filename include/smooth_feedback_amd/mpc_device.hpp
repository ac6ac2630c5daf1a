// MPC swarm whose LINEARISATION runs on the GPU as well (HIP only: include from a translation unit compiled by hipcc).
// MPCSwarmDevice (mpc.hpp) already keeps assembly, solve and warm starts on the device; what is left on the host there
// is MPC::fill_record -- the desired trajectory, the dynamics and the running constraint with their Jacobians at every
// collocation node (ocp_to_qp.hpp:250-257, :300-313, :345-357) -- and the upload of the records.  For a model whose
// functors are device-callable, one GPU thread per agent and node writes its part of the record straight into the
// swarm's device buffer (sfb_mpc_swarm_device_records) and the tick continues from there
// (sfb_mpc_swarm_step_resident): only the agents' times and states go up.
//
// Model: a struct with `__host__ __device__` members
//   X xdes(double t), Vec<Nx> dxdes(double t), U udes(double t)   desired trajectory (MPC::set_xdes / set_udes)
//   F f, CR cr                                                    dynamics f(x, u) and running constraint cr(x, u),
//                                                                 optionally with jacobian(x, u, dx, du) members
// -- the same functions the host MPC object of the swarm was built from.  Records equal the host's fill_record up to
// what sin / cos of the two maths libraries differ; everything downstream is the same kernels.
#pragma once
#ifndef __HIPCC__
#error "mpc_device.hpp needs hipcc"
#endif
#include <hip/hip_runtime.h>

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "detail/device_arena.hpp"
#include "mesh_device.hpp"
#include "mpc.hpp"
#include "mpc_relin.hpp"

namespace smooth_feedback_amd {

namespace detail {

/// where the pieces of a record go (sfb.h: [ f | dxdes | dfdx | dfdu | c | dcdx | dcdu | e | J ], Jacobians packed by pos_*)
template<int Nx, int Nu, int Ncr>
struct RecordMapDev {
  int N;
  double tf;
  int n_fx, n_fu, n_cx, n_cu, n_J;
  int o_f, o_dx, o_dfdx, o_dfdu, o_c, o_dcdx, o_dcdu, o_e, o_J;
  int64_t rec_doubles;
  int16_t pos_fx[Nx * Nx], pos_fu[Nx * Nu], pos_cx[(Ncr > 0 ? Ncr : 1) * Nx], pos_cu[(Ncr > 0 ? Ncr : 1) * Nu], pos_J[Nx * Nx];  // -1: not carried
};

template<class X, class U, int Ncr, class Model>
__global__ void __launch_bounds__(64) mpc_linearise_kernel(const int64_t B, const RecordMapDev<X::Dof, U::Dof, Ncr> map, const Model model,
                                                           const double * __restrict__ tau, const double * __restrict__ t,
                                                           const X * __restrict__ xs, double * __restrict__ records,
                                                           int * __restrict__ misfit)
{
  constexpr int Nx = X::Dof, Nu = U::Dof;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per     = map.N + 1;
  const int64_t b   = gid / per;
  const int node    = (int)(gid - b * per);
  if (b >= B) return;
  double * rec = records + b * map.rec_doubles;
  bool bad     = false;
  auto put = [&](double * dst, const int16_t * pos, int kept, int block, int e, double v) {
    const int p = pos[e];
    if (p >= 0) dst[(int64_t)block * kept + p] = v;
    else bad = bad || !(v == 0.0);
  };
  if (node < map.N) {
    const double ti = t[b] + map.tf * tau[node];
    const X xl      = model.xdes(ti);
    const auto dxl  = model.dxdes(ti);
    const U ul      = model.udes(ti);
    Vec<Nx> fv;
    Mat<Nx, Nx> dfdx;
    Mat<Nx, Nu> dfdu;
    xu_jacobian<Nx>(model.f, xl, ul, fv, dfdx, dfdu);
    // (every loop over matrix entries unrolled: with run-time indices the matrices live in scratch memory -- 1.4 KB per lane at Nx = 12)
#pragma unroll
    for (int d = 0; d < Nx; ++d) {
      rec[map.o_f + node * Nx + d]  = fv[d];
      rec[map.o_dx + node * Nx + d] = dxl[d];
#pragma unroll
      for (int c = 0; c < Nx; ++c) put(rec + map.o_dfdx, map.pos_fx, map.n_fx, node, d * Nx + c, dfdx(d, c));
#pragma unroll
      for (int c = 0; c < Nu; ++c) put(rec + map.o_dfdu, map.pos_fu, map.n_fu, node, d * Nu + c, dfdu(d, c));
    }
    if constexpr (Ncr > 0) {
      Vec<Ncr> cv;
      Mat<Ncr, Nx> dcdx;
      Mat<Ncr, Nu> dcdu;
      xu_jacobian<Ncr>(model.cr, xl, ul, cv, dcdx, dcdu);
#pragma unroll
      for (int d = 0; d < Ncr; ++d) {
        rec[map.o_c + node * Ncr + d] = cv[d];
#pragma unroll
        for (int c = 0; c < Nx; ++c) put(rec + map.o_dcdx, map.pos_cx, map.n_cx, node, d * Nx + c, dcdx(d, c));
#pragma unroll
        for (int c = 0; c < Nu; ++c) put(rec + map.o_dcdu, map.pos_cu, map.n_cu, node, d * Nu + c, dcdu(d, c));
      }
    }
  } else {  // the initial-state constraint: e = xdes(t) (-) x, J = d^r exp^-1(e)   (MPCCE, mpc.hpp:288-301)
    const auto e = rminus(model.xdes(t[b]), xs[b]);
    const auto J = X::dr_expinv(e);
#pragma unroll
    for (int d = 0; d < Nx; ++d) {
      rec[map.o_e + d] = e[d];
#pragma unroll
      for (int c = 0; c < Nx; ++c) put(rec + map.o_J, map.pos_J, map.n_J, 0, d * Nx + c, J(d, c));
    }
  }
  if (bad) atomicOr(misfit, 1);
}

/// The re-linearisation pass of mpc_relin.hpp: one lane per (agent, node) writes its slice of the agent's FLAT record
/// (unpacked: the offsets of sfb.h at N nodes) about the plan the swarm holds -- primal [B][n] = [e_0 .. e_N | v_0 .. v_{N-1}],
/// code [B] (sfb_mpc_swarm_device_solution); an agent whose code is not one the swarm keeps is re-linearised about
/// e = v = 0.  Lane `N` of an agent pins the initial state.  The law is relin_dyn_node / relin_cr_node, the functions the
/// host's MPC::fill_flat_record calls, forced inline; every loop over matrix entries has compile-time bounds.
template<class X, class U, int Ncr, class Model>
__global__ void __launch_bounds__(64) mpc_relinearise_kernel(const int64_t B, const int N, const double tf, const int64_t n, const Model model,
                                                             const double * __restrict__ tau, const double * __restrict__ t,
                                                             const X * __restrict__ xs, const double * __restrict__ primal,
                                                             const int32_t * __restrict__ code, double * __restrict__ records)
{
  constexpr int Nx = X::Dof, Nu = U::Dof;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per     = N + 1;
  const int64_t b   = gid / per;
  const int node    = (int)(gid - b * per);
  if (b >= B) return;
  const int o_f = 0, o_dx = o_f + N * Nx, o_dfdx = o_dx + N * Nx, o_dfdu = o_dfdx + N * Nx * Nx, o_c = o_dfdu + N * Nx * Nu,
            o_dcdx = o_c + N * Ncr, o_dcdu = o_dcdx + N * Ncr * Nx, o_e = o_dcdu + N * Ncr * Nu, o_J = o_e + Nx;
  double * rec = records + b * (int64_t)(o_J + Nx * Nx);
  if (node < N) {
    const double ti = t[b] + tf * tau[node];
    const X xl      = model.xdes(ti);
    const auto dxl  = model.dxdes(ti);
    const U ul      = model.udes(ti);
    const bool kept = relin_plan_kept(code[b]);
    const double * pe = primal + b * n + (int64_t)node * Nx;
    const double * pv = primal + b * n + (int64_t)(N + 1) * Nx + (int64_t)node * Nu;
    Vec<Nx> ebar;
    Vec<Nu> vbar;
#pragma unroll
    for (int d = 0; d < Nx; ++d) ebar[d] = kept ? pe[d] : 0.0;
#pragma unroll
    for (int d = 0; d < Nu; ++d) vbar[d] = kept ? pv[d] : 0.0;
    {
      Vec<Nx> f0;
      Mat<Nx, Nx> A;
      Mat<Nx, Nu> Bm;
      relin_dyn_node<X, U>(model.f, xl, dxl, ul, ebar, vbar, f0, A, Bm);
#pragma unroll
      for (int d = 0; d < Nx; ++d) {
        rec[o_f + node * Nx + d]  = f0[d];
        rec[o_dx + node * Nx + d] = 0.0;
#pragma unroll
        for (int c = 0; c < Nx; ++c) rec[o_dfdx + (node * Nx + d) * Nx + c] = A(d, c);
#pragma unroll
        for (int c = 0; c < Nu; ++c) rec[o_dfdu + (node * Nx + d) * Nu + c] = Bm(d, c);
      }
    }
    if constexpr (Ncr > 0) {
      Vec<Ncr> c0;
      Mat<Ncr, Nx> C;
      Mat<Ncr, Nu> D;
      relin_cr_node<X, U, Ncr>(model.cr, xl, dxl, ul, ebar, vbar, c0, C, D);
#pragma unroll
      for (int d = 0; d < Ncr; ++d) {
        rec[o_c + node * Ncr + d] = c0[d];
#pragma unroll
        for (int c = 0; c < Nx; ++c) rec[o_dcdx + (node * Ncr + d) * Nx + c] = C(d, c);
#pragma unroll
        for (int c = 0; c < Nu; ++c) rec[o_dcdu + (node * Ncr + d) * Nu + c] = D(d, c);
      }
    }
  } else {  // e_0 = log(xdes(t)^-1 x) exactly: J = I and e = xdes(t) (-) x = -e_0 (the assembled row is J e_0 = 0 - e)
    const auto e = rminus(model.xdes(t[b]), xs[b]);
#pragma unroll
    for (int d = 0; d < Nx; ++d) {
      rec[o_e + d] = e[d];
#pragma unroll
      for (int c = 0; c < Nx; ++c) rec[o_J + d * Nx + c] = (c == d) ? 1.0 : 0.0;
    }
  }
}

}  // namespace detail

/// MPCSwarmDevice with the linearisation on the GPU.  `proto` is the host MPC object of the same model (structure probing,
/// symbolic analysis, mesh, parameters), `model` its device-callable twin.
template<class MPCT, class Model>
class MPCSwarmDeviceLin {
public:
  using X = decltype(std::declval<const Model &>().xdes(0.0));
  using U = decltype(std::declval<const Model &>().udes(0.0));
  static constexpr int Nx = MPCT::Nx, Nu = MPCT::Nu, Ncr = MPCT::Ncr;
  using Map = detail::RecordMapDev<Nx, Nu, Ncr>;

  MPCSwarmDeviceLin(MPCT & proto, Model model, int64_t agents, double t_probe = 0.0, bool probe_empty = false)
      : mpc_(proto), model_(model), B_(agents)
  {
    if (!mpc_.solver().analyzed()) {
      std::vector<uint8_t> keep;
      mpc_.probe_default(t_probe, keep);
      mpc_.analyze_solver(&keep);
    }
    if (!probe_empty) pack_ = mpc_.probe_record_default(t_probe);  // probe_empty: tests of the misfit fallback
    packed_ = mpc_.params().prune_explicit_zeros && pack_.doubles(mpc_.N()) < MPCT::record_doubles(mpc_.N());
    layout_ = mpc_.device_layout(packed_ ? &pack_.keep : nullptr);
    const auto & qp = mpc_.qp();
    static_assert(std::is_same_v<typename MPCT::TimeT, double>, "the device-side linearisation takes time as double seconds");
    sfb_check(sfb_mpc_swarm_create(mpc_.solver().plan(), &layout_->c, qp.P_val.data(), qp.q.data(), B_, &swarm_));
    mpc_.solver().pin_plan();  // the swarm holds the raw plan pointer
    sfb_check(sfb_mpc_swarm_device_records(swarm_, &drec_, nullptr));
    const int Nn = mpc_.N();
    std::vector<double> tau((size_t)Nn + 1);
    for (int i = 0; i <= Nn; ++i) tau[(size_t)i] = mpc_.mesh().node(i);
    detail::DeviceArena a;
    a.add(&dtau_, tau.size()); a.add(&dt_, (size_t)B_); a.add(&dx_, (size_t)B_); a.add(&dmisfit_, 1);
    dmem_ = detail::DeviceBlock(a, "mpc_device");
    check(detail::upload(dtau_, tau.data(), tau.size()), "hipMemcpy(tau)");
    build_map();
    du0_.resize((size_t)B_ * Nu);
    iter_.resize((size_t)B_);
    code_.resize((size_t)B_);
  }
  MPCSwarmDeviceLin(const MPCSwarmDeviceLin &)             = delete;
  MPCSwarmDeviceLin & operator=(const MPCSwarmDeviceLin &) = delete;
  ~MPCSwarmDeviceLin()
  {
    sfb_mpc_swarm_destroy(swarm_);
    mpc_.solver().unpin_plan();
  }

  void reset_warmstart() { sfb_check(sfb_mpc_swarm_reset_warmstart(swarm_)); }

  /// one control tick for all agents
  void step(const std::vector<double> & t, const std::vector<X> & xs, std::vector<U> & us, std::vector<QPSolutionStatus> & codes)
  {
    if ((int64_t)t.size() != B_ || (int64_t)xs.size() != B_) throw std::invalid_argument("MPCSwarmDeviceLin: one time and state per agent");
    us.resize((size_t)B_);
    codes.resize((size_t)B_);
    step(t.data(), xs.data(), us.data(), codes.data());
  }
  /// the same on arrays of size() entries (a shard of a larger swarm: multi_device.hpp)
  void step(const double * t, const X * xs, U * us, QPSolutionStatus * codes)
  {
    check(detail::upload(dt_, t, (size_t)B_), "hipMemcpy(t)");
    check(detail::upload(dx_, xs, (size_t)B_), "hipMemcpy(x)");
    linearise();
    int misfit = 0;
    check(detail::download(&misfit, dmisfit_, 1), "hipMemcpy(flag)");
    if (misfit && packed_) {
      // a linearisation has a non-zero where the probe saw none: unpacked records from now on (same results; warm
      // starts and solver memory of the swarm are untouched), and this tick's records once more
      packed_ = false;
      sfb_check(sfb_mpc_swarm_set_jac_keep(swarm_, nullptr, nullptr));
      build_map();
      linearise();
    }
    const sfb_qp_params c = mpc_.solver().params().to_c();
    sfb_check(sfb_mpc_swarm_step_resident(swarm_, &c, mpc_.params().warmstart ? 1 : 0, du0_.data(), iter_.data(), code_.data(), nullptr,
                                          nullptr));
    for (int64_t b = 0; b < B_; ++b) {
      us[(size_t)b]    = mpc_.input_from_du0(t[(size_t)b], &du0_[(size_t)b * Nu]);
      codes[(size_t)b] = static_cast<QPSolutionStatus>(code_[(size_t)b]);
    }
  }
  /// one control tick followed by `passes` re-linearisation passes (sequential convex MPC, mpc_relin.hpp): the tick above,
  /// then `passes` times mpc_relinearise_kernel about the plans the swarm holds and sfb_mpc_swarm_step_resident_flat, all
  /// on the null stream.  The host only waits where step() already does, for the small outputs of every solve; nothing is
  /// allocated.  passes == 0 is step(t, xs, us, codes).  us / codes / iterations() are those of the plans held at the end.
  /// A prototype analysed with a mask of MPC::probe_relin keeps the passes on the pruned plan.
  void step(const std::vector<double> & t, const std::vector<X> & xs, std::vector<U> & us, std::vector<QPSolutionStatus> & codes, int passes)
  {
    if ((int64_t)t.size() != B_ || (int64_t)xs.size() != B_) throw std::invalid_argument("MPCSwarmDeviceLin: one time and state per agent");
    us.resize((size_t)B_);
    codes.resize((size_t)B_);
    step(t.data(), xs.data(), us.data(), codes.data(), passes);
  }
  void step(const double * t, const X * xs, U * us, QPSolutionStatus * codes, int passes)
  {
    if (passes < 0) throw std::invalid_argument("MPCSwarmDeviceLin: passes < 0");
    step(t, xs, us, codes);
    if (passes == 0) return;
    const sfb_qp_params c = mpc_.solver().params().to_c();
    for (int pass = 0; pass < passes; ++pass) {
      relinearise(nullptr);
      sfb_check(sfb_mpc_swarm_step_resident_flat(swarm_, &c, du0_.data(), iter_.data(), code_.data(), nullptr, nullptr));
    }
    for (int64_t b = 0; b < B_; ++b) {
      us[(size_t)b]    = mpc_.input_from_du0(t[(size_t)b], &du0_[(size_t)b * Nu]);
      codes[(size_t)b] = static_cast<QPSolutionStatus>(code_[(size_t)b]);
    }
  }
  /// the kernel of a pass alone, on `stream`: flat records about the swarm's current plans into its device record buffer,
  /// from the times and states of the last step() (unpacked: MPCT::record_doubles(N) per agent, whatever packed_records())
  void relinearise(hipStream_t stream)
  {
    const double * dprimal = nullptr;
    const int32_t * dcode  = nullptr;
    sfb_check(sfb_mpc_swarm_device_solution(swarm_, &dprimal, nullptr, &dcode));
    const int Nn = mpc_.N();
    hipLaunchKernelGGL((detail::mpc_relinearise_kernel<X, U, Ncr, Model>), detail::lane_grid(B_ * (Nn + 1)), dim3(64), 0, stream, B_, Nn,
                       mpc_.params().tf, (int64_t)mpc_.qp().n, model_, dtau_, dt_, dx_, dprimal, dcode, drec_);
    check(hipGetLastError(), "mpc_relinearise_kernel");
  }
  /// the flat records of the last pass (device -> host), [agents][MPCT::record_doubles(N)]
  void copy_flat_records(double * out) const
  {
    check(detail::download(out, drec_, (size_t)B_ * (size_t)MPCT::record_doubles(mpc_.N())), "hipMemcpy(records)");
  }
  /// what audit() brings back: 8 bytes per agent and per interval
  struct Audit {
    std::vector<double> agent_max;  // [agents] largest interval error of the agent's plan (NaN: the plan has a NaN)
    std::vector<double> ival_max;   // [intervals] largest error over the agents whose plan the swarm keeps
    int32_t skipped = 0;            // agents left out of ival_max (status not kept, or a NaN)
  };
  /// Dynamics-error audit (mesh_device.hpp: mpc_dyn_error_device) of the plans of the last step(), on the device, with
  /// t the times that step was given.  `errs` (nullable) also receives the full [agents][intervals] table.  A separate
  /// call: step() is as it was, and the next step() does not depend on it.
  Audit audit(const double * t, std::vector<double> * errs = nullptr)
  {
    const int nivals = mpc_.mesh().N_ivals();
    if (!daudit_.get()) {
      detail::DeviceArena a;
      a.add(&derrs_, (size_t)B_ * nivals); a.add(&damax_, (size_t)B_); a.add(&dimax_, (size_t)nivals); a.add(&dskip_, 1);
      daudit_ = detail::DeviceBlock(a, "mpc_device");
    }
    const double * dprimal = nullptr;
    const int32_t * dcode  = nullptr;
    sfb_check(sfb_mpc_swarm_device_solution(swarm_, &dprimal, nullptr, &dcode));
    check(detail::upload(dt_, t, (size_t)B_), "hipMemcpy(t)");
    check(mpc_dyn_error_device(mpc_, model_, B_, dt_, dprimal, dcode, derrs_, damax_, dimax_, dskip_, nullptr), "mpc_audit_kernel");
    Audit r;
    r.agent_max.resize((size_t)B_);
    r.ival_max.resize((size_t)nivals);
    check(detail::download(r.agent_max.data(), damax_, (size_t)B_), "hipMemcpy(agent_max)");  // (synchronises with the launches)
    check(detail::download(r.ival_max.data(), dimax_, (size_t)nivals), "hipMemcpy(ival_max)");
    check(detail::download(&r.skipped, dskip_, 1), "hipMemcpy(skipped)");
    if (errs) {
      errs->resize((size_t)B_ * nivals);
      check(detail::download(errs->data(), derrs_, errs->size()), "hipMemcpy(errs)");
    }
    return r;
  }
  /// the swarm's shared mesh refined where the audit's interval errors exceed `target` (Mesh::refine_errors);
  /// rebuilding the swarm on it is the caller's business
  Mesh<MPCT::Kmesh, MPCT::Kmesh> refined_mesh(const std::vector<double> & ival_max, double target) const
  {
    Mesh<MPCT::Kmesh, MPCT::Kmesh> m((std::size_t)mpc_.mesh().N_ivals(), (std::size_t)MPCT::Kmesh);
    m.refine_errors(ival_max, target);
    return m;
  }
  /// the solution of the last step() where it lies: device pointers, valid until the next call on the swarm
  void device_solution(const double ** primal, const int32_t ** code) const
  {
    sfb_check(sfb_mpc_swarm_device_solution(swarm_, primal, nullptr, code));
  }
  /// the solution of the last step() (device -> host): primal [agents][n], code [agents]; each nullable
  void copy_solution(double * primal, int32_t * code) const
  {
    const double * dprimal = nullptr;
    const int32_t * dcode  = nullptr;
    sfb_check(sfb_mpc_swarm_device_solution(swarm_, &dprimal, nullptr, &dcode));
    if (primal) check(detail::download(primal, dprimal, (size_t)B_ * (size_t)mpc_.qp().n), "hipMemcpy(primal)");
    if (code) check(detail::download(code, dcode, (size_t)B_), "hipMemcpy(code)");
  }
  int64_t size() const { return B_; }
  sfb_mpc_swarm * handle() { return swarm_; }
  const std::vector<uint32_t> & iterations() const { return iter_; }
  bool packed_records() const { return packed_; }
  int64_t record_doubles() const { return map_.rec_doubles; }
  /// the records of the last tick (device -> host), [agents][record_doubles()]
  void copy_records(double * out) const
  {
    check(detail::download(out, drec_, (size_t)B_ * (size_t)map_.rec_doubles), "hipMemcpy(records)");
  }

private:
  static void check(hipError_t e, const char * what) { detail::hip_check(e, "mpc_device", what); }
  void build_map()
  {
    const int Nn = mpc_.N();
    Map & m = map_;
    m.N  = Nn;
    m.tf = mpc_.params().tf;
    const uint8_t * k = pack_.keep.data();
    auto fill = [&](int16_t * pos, int len) {
      int cnt = 0;
      for (int e = 0; e < len; ++e) pos[e] = (!packed_ || k[e]) ? (int16_t)cnt++ : (int16_t)-1;
      k += len;
      return cnt;
    };
    m.n_fx = fill(m.pos_fx, Nx * Nx); m.n_fu = fill(m.pos_fu, Nx * Nu); m.n_cx = fill(m.pos_cx, Ncr * Nx);
    m.n_cu = fill(m.pos_cu, Ncr * Nu); m.n_J = fill(m.pos_J, Nx * Nx);
    int64_t o = 0;
    m.o_f = (int)o; o += (int64_t)Nn * Nx;
    m.o_dx = (int)o; o += (int64_t)Nn * Nx;
    m.o_dfdx = (int)o; o += (int64_t)Nn * m.n_fx;
    m.o_dfdu = (int)o; o += (int64_t)Nn * m.n_fu;
    m.o_c = (int)o; o += (int64_t)Nn * Ncr;
    m.o_dcdx = (int)o; o += (int64_t)Nn * m.n_cx;
    m.o_dcdu = (int)o; o += (int64_t)Nn * m.n_cu;
    m.o_e = (int)o; o += Nx;
    m.o_J = (int)o; o += m.n_J;
    m.rec_doubles = o;
    int64_t rd = 0;
    sfb_check(sfb_mpc_swarm_device_records(swarm_, &drec_, &rd));
    if (rd != o) throw std::logic_error("mpc_device: record layout differs from the swarm's");
  }
  void linearise()
  {
    check(hipMemsetAsync(dmisfit_, 0, sizeof(int), nullptr), "hipMemsetAsync");
    const int64_t threads = B_ * (map_.N + 1);
    hipLaunchKernelGGL((detail::mpc_linearise_kernel<X, U, Ncr, Model>), detail::lane_grid(threads), dim3(64), 0, nullptr, B_, map_,
                       model_, dtau_, dt_, dx_, drec_, dmisfit_);
    check(hipGetLastError(), "mpc_linearise_kernel");
  }

  MPCT & mpc_;
  Model model_;
  int64_t B_;
  typename MPCT::RecordPacking pack_;
  bool packed_ = false;
  std::unique_ptr<typename MPCT::DeviceLayout> layout_;
  sfb_mpc_swarm * swarm_ = nullptr;
  Map map_{};
  detail::DeviceBlock dmem_, daudit_;
  double * derrs_ = nullptr, *damax_ = nullptr, *dimax_ = nullptr;
  int32_t * dskip_ = nullptr;
  double * dtau_ = nullptr, *dt_ = nullptr, *drec_ = nullptr;
  X * dx_        = nullptr;
  int * dmisfit_ = nullptr;
  std::vector<double> du0_;
  std::vector<uint32_t> iter_;
  std::vector<int32_t> code_;
};

}  // namespace smooth_feedback_amd
