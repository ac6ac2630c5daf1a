/* Example / test harness around the C++ host front (the headers under include/smooth_feedback_amd): concrete MPC
 * models with a C interface so that Python tests and bench.py can drive the host-side assembly.
 * NOT part of the product C-ABI (that is include/sfb.h); built into libsfb_models.so. */
#ifndef SFBX_MODELS_H
#define SFBX_MODELS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* variant 6 : X = Bundle<SE2,R3>, U = R2   -- the vehicle of examples/mpc_asif_vehicle.cpp:42-79
 * variant 12: X = Bundle<SE2,R3,SE2,R3>, U = R2 -- two such vehicles driven by one input pair
 *             (synthetic: matches BASELINE.json's "nx=12, nu=2" problem size n = m = 740 at K = 50)
 * variant 13: X = Bundle<SE3,R6>, U = R6  -- a 3-D rigid body, pose and body twist (rigid_body_model.h); u0 is [batch][6] */
int sfbx_mpc_dims(int variant, int K, int *n, int *m, int *nnzP, int *nnzA, int *Nx, int *Nu, int *N);
/* pattern (+ P values, identical for all agents).  Arrays sized by sfbx_mpc_dims. */
int sfbx_mpc_pattern(int variant, int K, double tf, int32_t *Pp, int32_t *Pi, double *Pval, int32_t *Ap, int32_t *Aj);
/* elimination stages (n+m entries) suggested by the MPC front for the solver's ordering */
int sfbx_mpc_stage(int variant, int K, int32_t *stage);
/* Assemble `batch` agents: agent b runs at time t_b = 0.025*(b % 400) from x_b = xdes(t_b) (+) xi_b,
 * xi_b ~ U(-0.5,0.5)^Nx from std::mt19937_64(seed + b).  Aval [batch][nnzA], l,u [batch][m]. */
int sfbx_mpc_assemble_batch(int variant, int K, double tf, int64_t batch, uint64_t seed, double *Aval, double *l,
                            double *u, int threads);
/* Closed loop of tests/test_mpc.cpp:34-117 (SE2 state, R2 input, f = (u0, 0, u1), -1 <= u <= 1):
 * three consecutive MPC calls with warm start, then three without. u_out[6][2], codes[6]. Needs a GPU. */
int sfbx_test_mpc_se2(double *u_out, int32_t *codes, int32_t *traj_sizes);
/* tests/test_mpc.cpp:60-155 (StaticProperties as static_asserts, Api, Constructors) written against
 * <smooth/feedback/mpc.hpp> with only the Lie types renamed, plus the declaration of examples/mpc_asif_vehicle.cpp:64.
 * codes[12]: Api code0..3, Constructors code1..5, original-after-the-copy's-setter / fresh controller, the vehicle.
 * out[14]: [0] rel |u1 - u2|, [1] rel |u3 - u1|, [2] us.size() + 1 == xs.size(), [3] f.t_, [4] cr.t_, [5] pointer overload,
 * [6..9] rel |u1 - u2..5| of the copies / moves, [10] max |u| of the vehicle, [11] copies own their analyses,
 * [12] rel |original after set_udes on a COPY - fresh controller with that udes| (copies share the desired
 * trajectories, mpc.hpp:407, 607-608), [13] ... and that input differs from before.  Needs a GPU. */
int sfbx_test_mpc_api(double *out, int32_t *codes);
/* The host-only half of that front (no GPU): out[0] > 0 a setter on a COPY moves the original's assembly, out[1] == 0 every copy
 * sees the same desired trajectories, out[2] copies own their QP, out[3] no analysis travels with a copy, out[4] == 0 the const
 * assembly path leaves a by-reference functor's set_time alone, out[5] == 232 (Ncr 2, Nx 3, Nu 2), out[6] type properties. */
int sfbx_test_mpc_front_host(double *out);
/* MPC API beyond operator(): out[0] set_xdes_rel / set_udes_rel (mpc.hpp:539-586) vs the absolute-time setters (max abs
 * difference of A, l, u), out[1] the same controller with Time = std::chrono::steady_clock::time_point (time.hpp:25-89),
 * out[2..4] set_weights (mpc.hpp:593-598: stored, not transcribed; the constructor transcribes), out[5..8] lazy structure
 * refresh after set_xdes / set_udes and plan pinning (1.0 = as specified).  Host only (no GPU). */
int sfbx_test_mpc_time_and_setters(double *out);
/* examples/mpc_doubleintegrator.cpp:31-101 in closed loop for `ticks` ticks of 50 ms (time-invariant QP matrices: the
 * solver front flags every tick after the first as reuse_factor), then the same loop with the reuse switched off:
 * u_out / iters / codes [ticks] and u_ref / iters_ref [ticks]; reuse_count = flagged solves of the first loop;
 * seconds[2] = wall time of the two loops.  Needs a GPU. */
int sfbx_test_mpc_doubleintegrator(int ticks, double *u_out, uint32_t *iters, int32_t *codes, double *u_ref, uint32_t *iters_ref,
                                   int64_t *reuse_count, double *seconds);
/* tests/test_ocp_to_qp.cpp:41-107 with the GENERIC front ocp_to_qp() (include/smooth_feedback_amd/ocp_to_qp.hpp):
 * out[0..6] sizes (n, m, |q|, |l|, |u|, cols of P, rows of A), out[7..8] = min(A var - l), min(u - A var) for the exact
 * trajectory (:105-106), out[9..11] cost entries; solve != 0 (needs a GPU): out[12] status of solve_qp, out[13..17]
 * values of the qpsol_to_ocpsol() trajectory. */
int sfbx_test_ocp_to_qp_basic(double *out, int solve);
/* tests/test_ocp_to_qp.cpp:41-107 through the MPC transcription (double integrator, two intervals of 5 LGR nodes, tf = 2):
 * out = {min(A var - l), min(u - A var), N, n, m, intervals} for the exact parabola trajectory.  Host only (no GPU). */
int sfbx_test_ocp_to_qp_parabola(double *out);
/* tests/test_qp.cpp StaticProperties (:37-52, static_asserts in models.cpp), SolverAPI (:338-372), SparseSolverAPI
 * (:374-415) and PartialDynamic (:124-147) through the reference's include path <smooth/feedback/qp_solver.hpp> and
 * namespace: primal_dense / primal_sparse [5][2] = the five solvers' primal (original, copy, copy-assigned, moved,
 * move-assigned); primal_partial = {x0, x1, objective, hot-start x0, x1}.  Returns 0 on success.  Needs a GPU. */
int sfbx_test_qp_solver_api(double *primal_dense, double *primal_sparse, double *primal_partial);
/* QPSolver<sparse>: solve(A1), solve_batch(A2), solve(A1), solve(A1) on one solver (shared device workspace): out[0] third
 * == first bit for bit, out[1] / out[2] solves flagged reuse_factor after the third / fourth call (0 / 1), out[3] fourth
 * == first, out[4..7] primal of first and of the batch call.  Needs a GPU. */
int sfbx_test_solve_after_solve_batch(double *out);
/* Swarm tick through MPCSwarm (host assembly + one batched GPU solve): returns u0 [batch][2], codes. */
int sfbx_mpc_swarm_step(int variant, int K, double tf, int64_t batch, uint64_t seed, int ticks, double *u0,
                        int32_t *codes, uint32_t *iters);
/* The same swarm with every batched solve sharded over `devices` (sfb_set_devices; an ordinal may repeat) from this
 * one process: one host thread, plan upload and workspace per device.  Same outputs as sfbx_mpc_swarm_step. */
int sfbx_mpc_swarm_step_multi(int variant, int K, double tf, int64_t batch, uint64_t seed, int ticks, const int *devices,
                              int ndev, double *u0, int32_t *codes, uint32_t *iters);
/* Device-side assembly (sfb_mpc_assemble_batch / sfb_mpc_swarm, include/sfb.h): the layout of the variant's
 * transcription -- dims = {nx, nu, ncr, kmesh, nivals, nparts}, alpha [nivals], D [(kmesh+1)*kmesh], kind / dof
 * [nparts], crl / cru [ncr] --, the linearisation records of the agents of sfbx_mpc_assemble_batch
 * (rec [batch][record doubles]) and the swarm tick of sfbx_mpc_swarm_step through MPCSwarmDevice. */
int sfbx_mpc_layout(int variant, int K, double tf, int32_t *dims, double *alpha, double *D, int32_t *kind,
                    int32_t *dof, double *crl, double *cru);
int sfbx_mpc_records(int variant, int K, double tf, int64_t batch, uint64_t seed, double *rec, int threads);
int sfbx_mpc_swarm_device_step(int variant, int K, double tf, int64_t batch, uint64_t seed, int ticks, double *u0,
                               int32_t *codes, uint32_t *iters);
/* wall seconds of every swarm.step() of the last sfbx_mpc_swarm[_device]_step call; returns their number */
int sfbx_last_tick_seconds(double *out, int n);
/* group identities for the tests: returns max abs error over a set of checks */
double sfbx_lie_selftest(void);
/* the carver of the staging buffers (detail/device_arena.hpp), no GPU: 0, or the number of the first check that fails */
int sfbx_arena_selftest(void);
/* EKF<G> front (include/smooth_feedback_amd/ekf.hpp) against the reference's own checks: PredictTimeCut
 * (tests/test_ekf.cpp:155-180), UpdateLinear (:50-103, R^3 / Ny 3) and an SE2 predict+update smoke.
 * Returns 0 and writes max errors: err[0] time-cut, err[1] linear update state, err[2] linear update cov. Needs a GPU. */
int sfbx_test_ekf(double *err);
/* PredictLinear (tests/test_ekf.cpp:104-153) with EKF<R^Nx, RK4>, dt = 1e-3, tau = 0.7, Q = 0, Nx in {3, 6}:
 * err[0] = max relative error of the estimate vs expm(A tau) xhat, err[1] = of the covariance vs F P F'.
 * The exact F (Nx*Nx, column-major, for Nx = 3 then 6) is supplied by the caller.  Needs a GPU. */
int sfbx_test_ekf_predict_linear(const double *A3, const double *F3, const double *A6, const double *F6, double *err);
/* the third size of the reference's test, Nx = 9 (tests/test_ekf.cpp:152): the generic one-filter-per-wave kernel */
int sfbx_test_ekf_predict_linear9(const double *A9, const double *F9, double *err);
/* asif_to_qp() (include/smooth_feedback_amd/asif.hpp) for the case of tests/test_asif.cpp:37-95: X = SE2, f = (u0, 0, u1),
 * h = position (nh = 2), bu = (-0.1, 1), K = 3, input box [-1,1]^2 around c = 0, T = 1, alpha = 1, dt = 0.1.
 * x0 = (angle, px, py).  Out, column-major: P[9] q[3] A[9*3] l[9] u[9].  Host only (no GPU). */
int sfbx_asif_basic_qp(const double *x0, const double *udes, double *P, double *q, double *A, double *l, double *u);
/* ASIFilter on the GPU.  which = 0: the SO3 filter of tests/test_asif.cpp:103-131 (K = 100, nh = 3: n = 4, m = 301,
 * sparse-kernel path); which = 1: the vehicle filter of examples/mpc_asif_vehicle.cpp:95-129 (K = 200: n = 3, m = 203,
 * polish off); which = 2: the same vehicle with the default K = 10 (n = 3, m = 13: dense-kernel path).
 * Out: u[3], code, iter, and the QP that was solved (sized by dims[0] = n, dims[1] = m) with its primal/dual. */
int sfbx_test_asif(int which, double *u_out, int32_t *code, uint32_t *iter, int32_t *dims, double *P, double *q,
                   double *A, double *l, double *u, double *x, double *y);
/* ASIFSwarm: `batch` vehicles (state = xdes(t_b) (+) xi_b as in sfbx_mpc_assemble_batch, u_des ~ U(-0.5,0.5)^2),
 * K constraint instances, `ticks` consecutive calls (warm start from tick 2).  Out for the LAST tick: filtered
 * u [batch][2], codes, iters, the QPs [batch][...] (n = 3, m = K + 3) and their primal/dual solutions. */
int sfbx_asif_swarm_step(int64_t batch, uint64_t seed, int K, int ticks, double *u_out, int32_t *codes, uint32_t *iters,
                         double *P, double *q, double *A, double *l, double *u, double *x, double *y, double *wx,
                         double *wy);
/* the states (x, y, cos, sin, v0, v1, v2) [batch][7] and desired inputs [batch][2] sfbx_asif_swarm_step starts from */
int sfbx_asif_swarm_states(int64_t batch, uint64_t seed, double *states, double *udes);
/* the QPs [batch][...] of the FIRST tick of sfbx_asif_swarm_step (same agents, same assembly code path), not solved.
 * Host only (no GPU). */
int sfbx_asif_swarm_assemble(int64_t batch, uint64_t seed, int K, double *P, double *q, double *A, double *l, double *u);
/* The operations of include/smooth_feedback_amd/lie.hpp on `count` items (examples/lie_eval.h: group and operation
 * ids, element layouts): in [count][win], out [count][wout] with the widths of sfbx_lie_eval_widths.  Returns -1 when
 * the group has no such operation.  Host code; sfbx_lie_eval_device (models_device.hip) runs the same item function as
 * one GPU thread per item. */
int sfbx_lie_eval_widths(int group, int op, int *win, int *wout);
int sfbx_lie_eval(int group, int op, int64_t count, const double *in, double *out);
/* vehicle EKFs, one host EKF<> object per filter: `steps` x (predict(Q, tau, dt) + update(y[step], R)); the host twin of
 * sfbx_ekf_swarm_device (models_device.hip) */
int sfbx_ekf_swarm_host(int64_t batch, int steps, int rk4, double tau, double dt, const double *states, const double *P0,
                        const double *y, double *states_out, double *P_out);
/* the pose filter on SE3 of rigid_body_model.h, one host EKF<SE3> object per filter; states [batch][7] = (px, py, pz, w, x, y, z) */
int sfbx_pose_ekf_swarm_host(int64_t batch, int steps, int rk4, double tau, double dt, const double *states, const double *P0,
                             const double *y, double *states_out, double *P_out);
/* ASIFilter<Bundle<SE3,R6>, R6> on the rigid body, agent b of the filter tests: filtered input u [6], solver code, smallest constraint slack at the solution */
int sfbx_test_asif_rigid_body(int64_t b, double *u_out, int32_t *code, double *slack);
/* PID<T, G> through <smooth/feedback/pid.hpp> (host only): the call sequence of the reference's first PID test -- setters
 * in both forms, calls at and away from the target, reset_integral() -- then a function trajectory with kp = 2, kd = 3.
 * out [4]: |u|^2 at the target before / after integrating / after the reset, worst relative error of the trajectory check.
 * Returns 0 when all four are as expected. */
int sfbx_test_pid_api(double *out);
/* A batch pushed through one host PID<double, G> per agent: group 0 Rn<2>, 1 SE2, 2 SO3, 3 SE3, 4 Bundle<SE3, Rn<3>>,
 * 5 Bundle<SE2, Rn<1>>.  Every controller is called at times[0 .. ncalls) with the state x, v [batch][ncalls][...] and the
 * desired triple gd, vd, ad [batch][ncalls][...] of that call (element layout of sfb_pid_*); gains [batch][dof].
 * Out: u and the integral state after each call, [batch][ncalls][dof]. */
int sfbx_pid_host(int group, int64_t batch, int ncalls, const double *times, const double *x, const double *v, const double *gd,
                  const double *vd, const double *ad, const double *kp, const double *kd, const double *ki, double windup,
                  double *u_out, double *ie_out);
/* pid_rollout of pid.hpp -- the per-lane function of sfb_pid_rollout_batch and PIDSwarmDevice -- on the CPU, whole group at once
 * (no part-by-part split): arguments as sfb_pid_rollout_batch_host with per-agent gains and trajectories, groups as above. */
int sfbx_pid_rollout_host(int group, int64_t batch, double t0, double dt, int64_t steps, double *x, double *v, const double *g0,
                          const double *w, const double *kp, const double *kd, const double *ki, double windup, const double *u_max,
                          double *ie, double *t_last, double *u_last, double *cost);
/* PID<T, G>::set_xdes(t0, spline) through <smooth/feedback/pid.hpp> and <smooth/feedback/spline.hpp> (host only): five rounds
 * of a controller (kp = 2, kd = 3) following the cubic fitted through four random SE2 knots at times 0, 1, 2, 3, curve origin
 * at 0.5 s, called at 1 s, against the law written out from the curve at 0.5.  out [2]: worst relative error, smallest
 * |v_des|^2 + |a_des|^2 met.  Returns 0 when the error is <= 1e-12 and the curve was in motion. */
int sfbx_test_pid_spline_api(double *out);
/* Ad_g a on the host (lie.hpp), groups as sfbx_pid_host: g [count][elem], a and out [count][dof] */
int sfbx_lie_Ad(int group, int64_t count, const double *g, const double *a, double *out);
/* fit_spline_cubic per agent: tk [batch][nknots], gk [batch][nknots][elem] -> V [batch][nknots-1][3][dof] */
int sfbx_spline_fit_host(int group, int64_t batch, int64_t nknots, const double *tk, const double *gk, double *V);
/* Spline<degree, G>::operator() per agent, degree 2 or 3: V [batch][nknots-1][degree][dof], t [batch][nt] ->
 * g [batch][nt][elem], vel and acc [batch][nt][dof] */
int sfbx_spline_eval_host(int group, int degree, int64_t batch, int64_t nknots, const double *tk, const double *gk, const double *V,
                          int64_t nt, const double *t, double *g, double *vel, double *acc);
/* pid_rollout of pid.hpp along Spline<3, G> on the CPU: arguments as sfb_pid_rollout_spline_batch_host with per-agent splines
 * and gains */
int sfbx_pid_rollout_spline_host(int group, int64_t batch, double t0, double dt, int64_t steps, double *x, double *v, int64_t nknots,
                                 const double *tk, const double *gk, const double *V, const double *ts0, const double *kp,
                                 const double *kd, const double *ki, double windup, const double *u_max, double *ie, double *t_last,
                                 double *u_last, double *cost);
/* mesh: nodes (N+1), weights (N+1), Dus ((K+1)*K col-major) for `n` intervals of K points */
int sfbx_mesh(int n_ivals, int K, double *nodes, double *weights, double *Dus);

/* ---- collocation layer (collocation.cpp): the ph mesh Mesh<kmin, kmax> for <5,10>, <5,5>, <8,8>, <3,6>, <4,4>, <13,13>, <1,2>, <4,6> (-1: no such
 * instantiation) built as Mesh(n, k) and driven by an op script: ops [nops][3] rows (code, a, b) with 0 refine_ph(a, b),
 * 1 increase_degrees, 2 decrease_degrees, 3 set_N_colloc_ival(a, b), 4 refine_errors taking (target, errs[N_ivals]) from
 * opdata.  Out: nivals (-3 when above cap_ivals), K, tau0 [nivals], all nodes / weights [N + 1], the interval
 * differentiation ((K + 1) x K) and integration (K x K) matrices row-major and concatenated, and for nt times t
 * eval(t, vals, p, extend) [nt][dim] with interval_find(t) in found. */
int sfbx_mesh_script(int kmin, int kmax, int n, int k, int nops, const int32_t *ops, const double *opdata, int cap_ivals,
                     int32_t *nivals, int32_t *K, double *tau0, double *nodes, double *weights, double *diffmat, double *intmat,
                     int nt, const double *t, int dim, const double *vals, int p, int extend, double *eval_out, int32_t *found);
/* mesh_dyn_error on the script's mesh with its degrees raised by one; x(t), u(t) are the script's mesh polynomials through
 * vals_x [N + 1][nx] (extended) and vals_u [N][nu] (not extended).  Built-in dynamics fid: 0 time only, the derivative of
 * sum_k coef[d][k] t^k (coef [nx][4]); 1 harmonic pairs (x2, -x1); 2 pendulum pairs (x2, -sin x1 + u[pair mod nu]).
 * (nx, nu) in {(1,0), (1,1), (2,0), (2,1), (2,2), (12,2)} (-5 otherwise).  Out: errs [nivals]. */
int sfbx_mesh_dyn_error_host(int kmin, int kmax, int n, int k, int nops, const int32_t *ops, const double *opdata, int fid,
                             const double *coef, int nx, int nu, double t0, double tf, const double *vals_x, const double *vals_u,
                             double *errs);
/* flat_dynamics of model 0 (vehicle, SE2 x R^3, inputs R^2) / 1 (rigid body, SE3 x R^6, inputs R^6), row by row: elements
 * xl, ul in the flat storage of lie_eval.h, tangents dxl, e [rows][Nx], v [rows][Nu].  Out: [rows][Nx]. */
int sfbx_flat_dynamics_host(int model, int rows, const double *xl, const double *dxl, const double *ul, const double *e,
                            const double *v, double *out);
/* MPC::dyn_error(t[b], primal[b]) of the host front for GIVEN primals [batch][n] (variant 6 / 12: the vehicles, 13: the rigid
 * body; -1 otherwise).  Out: errs [batch][ceil(K / 4)]. */
int sfbx_mpc_dyn_error_host(int variant, int K, double tf, int64_t batch, const double *t, const double *primal, double *errs);
/* one tick of the host front from the state xdes(t) (+) dx0 at time t, then MPC::dyn_error(t) of the plan it stored; before
 * the tick dyn_error(t) must throw (-3 if it does not).  Out: errs [ceil(K / 4)], the tick's status code. */
int sfbx_mpc_tick_dyn_error_host(int variant, int K, double tf, double t, const double *dx0, double *errs, int32_t *code);
/* the reference's mesh and dyn-error tests as caller code against <smooth/feedback/collocation/{mesh,dyn_error}.hpp>: 0, or the number of
 * the first expectation that fails */
int sfbx_test_collocation_api(void);

/* ---- flatten_ocp (include/smooth_feedback_amd/ocp_flatten.hpp; harness: examples/flat_ocp_harness.h) ----
 * The Lie operations the flattening adds, per item: op 0 dr_exp(a) (in [T], out [T x T] column-major), op 1
 * d/de (dr_expinv(e) w) (in [e | w], out [T x T]).  Groups: 1 SE2, 2 SO3, 5 SE3, 6 Bundle<SE3, Rn<6>>, 7 Bundle<SE2, Rn<2>>.
 * -1 for anything else.  sfbx_flat_lie_eval_device (models_device.hip) runs the same item function, one GPU thread per item. */
int sfbx_flat_lie_eval(int group, int op, int64_t count, const double *in, double *out);
/* Problems: 0 the planar vehicle on Bundle<SE2, Rn<2>>, 1 the rigid body on Bundle<SE3, Rn<6>> (examples/ocp_se2_model.h).
 * sizes [7]: nx, nu, nq, ncr, nce, doubles per trajectory row, n of the NLP on N nodes. */
int sfbx_flat_ocp_sizes(int problem, int32_t N, int32_t *sizes);
/* The flattened problem at the nodes tau [N] of `agents` agents on the host (`threads` threads): x [agents][n] in the NLP's
 * layout, traj [agents][row] = [x0 | xi | u0 | du] (xl = rplus(x0, t xi), ul = u0 + t du).  Out, in the layout of
 * sfb_ocp_nlp_batch: Ff, dFf, Fg, dFg, Fcr, dFcr, ce, dce, and theta [agents], dtheta [agents][1 + 2 nx + nq]. */
int sfbx_flat_ocp_nodes_host(int problem, int64_t agents, int32_t N, const double *tau, const double *x, const double *traj,
                             double *Ff, double *dFf, double *Fg, double *dFg, double *Fcr, double *dFcr, double *ce,
                             double *dce, double *theta, double *dtheta, int threads);
/* ocp_to_nlp(flatten_ocp(problem, agent's trajectories), mesh) per agent: g [agents][m], dg [agents][nnz], f [agents], df
 * [agents][1 + 2 nx + nq] over (tf | e0 | ef | q); differing [agents] (nullable) counts the doubles of g and dg that are not
 * bit-identical to meshfn::ocp_nlp_assemble over the arrays of sfbx_flat_ocp_nodes_host.  mesh_kind 0: two intervals with
 * K = (3, 5); 1: 13 intervals of 4.  sizes [4] (nullable): n, m, nnz, N; taus [N + 1] (nullable).  x NULL: sizes only. */
int sfbx_flat_ocp_nlp_host(int problem, int mesh_kind, int64_t agents, const double *x, const double *traj, double *g,
                           double *dg, double *f, double *df, int64_t *differing, int32_t *sizes, double *taus);
/* The multiplier-contracted Hessians of the flattened problem at the nodes tau [N] on the host, by the difference law of
 * ocp_flatten.hpp, one (agent, node, direction) at a time: lam [agents][m'] with
 * m' = N nx + nq + N ncr + nce (dynamics | integrals | running | end).  Out, in the layout of sfb_ocp_nlp_hess_batch: HLf, HLg,
 * HLcr [agents][N][nz][nz], d2theta, d2ce_l [agents][ne][ne], full squares. */
int sfbx_flat_ocp_hess_nodes_host(int problem, int64_t agents, int32_t N, const double *tau, const double *x, const double *lam,
                                  const double *traj, double *HLf, double *HLg, double *HLcr, double *d2theta, double *d2ce_l,
                                  int threads);
/* d2l_dx2 of ocp_to_nlp(flatten_ocp<FlatHess::Differences>(...), mesh) per agent: hess [agents][nnzH]; differing [agents]
 * (nullable) counts the values not bit-identical to meshfn::ocp_nlp_hess_assemble over the host arrays above.
 * value_differences != 0: the default flatten_ocp instead, whose d2l_dx2 differences the flat values (differing untouched).
 * nnz_hess (nullable) receives nnzH; x NULL: that only. */
int sfbx_flat_ocp_hess_host(int problem, int mesh_kind, int64_t agents, const double *x, const double *lam, const double *sigma,
                            const double *traj, int value_differences, double *hess, int64_t *differing, int64_t *nnz_hess,
                            int threads);
/* Scenarios of the opt-in Hessians as caller code: figures [8]; 0 or the first failing expectation (see collocation.cpp). */
int sfbx_test_flatten_hess_api(double *figures);
/* Scenarios written as caller code against <smooth/feedback/ocp_flatten.hpp> (a flattened Rn problem against its original,
 * the unflatten round trip, d2l_dx2 against differences of the gradient, a Spline as a trajectory); figures [8]; 0 or the first failing expectation. */
int sfbx_test_flatten_api(double *figures);

/* mesh_eval (fn 0) / mesh_integrate (1) / mesh_dyn (2) of mesh_function.hpp at order deriv, differentiating the integrand by its
 * members (numerical 0) or by differences (1), on the script's mesh (also <1,2> and <4,6>).  Shapes 0 .. 3: an integrand given
 * as a term table on Rn state and input with (nx, nu, nf) = (3,2,3), (3,2,1), (1,0,1), (12,2,12): terms [nterms][5] rows
 * (r, a, ka, b, kb), output r += coef phi_ka(z_a) phi_kb(z_b), z = (t, x, u), phi = 1, z, z^2, sin z, cos z (-9: a row out of
 * range); shape 4: the vehicle's dynamics on SE2 x R^3 (xs in the flat storage of lie_eval.h; deriv <= 1, fn <= 1); shape 5:
 * (6, 2, 6) with the integrand tabulated, coef = [N][6 (1 + 9)] node by node the values, then the Jacobian row-major
 * (deriv <= 1, analytic, calls == 1).  -5 / -6:
 * no such shape / (fn, deriv) for it.  xs [N + 1][..], us [N][nu], lambda one per row of F (deriv 2).  The function is called
 * `calls` times on one MeshValue.  Out: dims = rows, cols, nnz of dF, nnz of d2F, 1 when no output array moved between the
 * calls; F; dF as CSR; d2F (upper triangle) as CSC. */
int sfbx_meshfn_host(int kmin, int kmax, int n, int k, int nops, const int32_t *ops, const double *opdata, int fn, int deriv,
                     int numerical, int shape, int nterms, const int32_t *terms, const double *coef, double t0, double tf,
                     const double *xs, const double *us, int scale, const double *lambda, int calls, int32_t *dims, double *F,
                     int32_t *rowptr, int32_t *colind, double *val, int32_t *colptr2, int32_t *rowind2, double *val2);
/* the reference's two trajectory scenarios of mesh_function (tests/test_collocation_mesh_function.cpp:522-628) as caller code
 * against <smooth/feedback/collocation/mesh_function.hpp>: 0, or the number of the first expectation that fails */
int sfbx_test_mesh_function_api(void);
/* OCPNLP (include/smooth_feedback_amd/ocp_to_nlp.hpp) of a problem given as three-factor term tables (rows r, a, ka, b, kb,
 * c, kc; nterms[5] and the rows of f, g, cr, theta, ce one after the other) on the script's mesh, at x and lambda, orders
 * 0 .. order, `calls` times; then nlpsol_to_ocpsol and ocpsol_to_nlpsol there and back (x_back, lambda_back).  Out: sizes = n,
 * m, nnz of dg, nnz of the Hessians, 1 when no output array moved between the calls; df dense; dg as CSR; d2f, d2g over one
 * CSC pattern.  NULL outputs are skipped.  -1: the harness does not carry this (mesh type, dims). */
int sfbx_ocp_nlp_host(int kmin, int kmax, int n, int k, int nops, const int32_t *ops, const int32_t *dims, const int32_t *nterms,
                      const int32_t *terms, const double *coef, const double *crl, const double *cru, const double *cel,
                      const double *ceu, const double *x, const double *lambda, int order, int numerical, int calls, int32_t *sizes,
                      double *f, double *df, double *g, int32_t *rowptr, int32_t *colind, double *dg, int32_t *hcolptr,
                      int32_t *hrowind, double *d2f, double *d2g, double *xl, double *xu, double *gl, double *gu, double *ws,
                      double *x_back, double *lambda_back);
/* OCPNLP::d2l_dx2(x, sigma, lambda) of the same problems, `calls` times.  sizes [4]: n, m, nnz of the Hessian, 1 when the output
 * array did not move between the calls; (hcolptr, hrowind): the pattern of the front's member; (hcolptr2, hrowind2): the pattern of
 * meshfn::ocp_nlp_hess_pattern from the mesh's interval sizes; d2l: the values.  NULL outputs are skipped. */
int sfbx_ocp_nlp_hess_host(int kmin, int kmax, int n, int k, int nops, const int32_t *ops, const int32_t *dims, const int32_t *nterms,
                           const int32_t *terms, const double *coef, const double *crl, const double *cru, const double *cel,
                           const double *ceu, const double *x, const double *lambda, double sigma, int numerical, int calls,
                           int32_t *sizes, int32_t *hcolptr, int32_t *hrowind, int32_t *hcolptr2, int32_t *hrowind2, double *d2l);
/* the scenario of the reference's tests/test_ocp_to_nlp.cpp as caller code against <smooth/feedback/ocp_to_nlp.hpp>: 0, or the
 * number of the first expectation that fails */
int sfbx_test_ocp_to_nlp_api(void);

#ifdef __cplusplus
}
#endif
#endif
