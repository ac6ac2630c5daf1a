/*
 * sfb.h -- C-ABI of the MI355X-native batched QP / MPC / EKF engine.
 *
 * This is the drop-in boundary for the hot path of pettni/smooth_feedback (reference @ v1).
 * The reference has no FFI layer: its boundary is a set of C++ templates instantiated in the
 * caller's translation unit.  Each entry point below names the reference interface it replaces
 * (file:line relative to the reference tree).  The C++ front in include/smooth_feedback_amd/
 * keeps the reference's class/function names and forwards to these functions.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types;
 *   - every function returns an sfb_status (0 = ok); per-problem results use the reference's
 *     QPSolutionStatus values (qp.hpp:82-92) in `code[]`; the library never aborts or throws;
 *   - `*_batch` functions take DEVICE pointers and are asynchronous on `stream` (a hipStream_t, NULL = default stream,
 *     non-blocking streams included): the call enqueues and returns.  The stream contract, as tested entry by entry on
 *     non-blocking side streams (tests/test_stream_contract_gpu.py):
 *       (1) every input is read behind `stream`: work enqueued on `stream` before the call -- a copy or a kernel that
 *           produces P, q, a warm start, a launch order -- is seen by it, with no synchronisation in between;
 *       (2) every output and every in-out buffer (EKF P, PID i_err / t_last, rollout states, trace tables) is complete for
 *           whatever is enqueued on `stream` after the call, and for any stream that waits on an event recorded on `stream`
 *           after it; the host needs a synchronisation of `stream` (not of the device) to read them.  Streams the library
 *           owns (the polishers' stream of the sparse solve) are joined back into `stream` before the call's last launch;
 *       (3) temporary memory is taken and released in stream order (hipMallocAsync / hipFreeAsync on `stream`), and
 *           nothing is shared between two caller streams: calls on different streams with their own buffers (and
 *           workspaces) may be in flight at once.
 *     Blocking entries: none -- in its steady state no device-pointer entry waits on the host for `stream` to drain.  What may wait on the host is
 *     first-use work (the upload of a plan's or a mesh's tables, creation of a stream's slot) and the fall-back to hipMalloc /
 *     hipFree with a synchronisation of `stream` when the runtime refuses a stream-ordered allocation;
 *   - `*_batch_host` functions take HOST pointers, stage through device memory and are synchronous;
 *   - all floating point data is IEEE fp64; batch items are contiguous, batch-major;
 *   - there is NO CPU fallback: without a usable HIP device every compute call fails with
 *     SFB_ERR_NO_DEVICE;
 *   - DEVICES: every call works on the calling thread's CURRENT HIP device (hipSetDevice); the library never
 *     switches devices.  Several GPUs = one process (or one thread with its own current device) per GPU, each
 *     with its own plans' device copies, workspaces and streams -- items are independent, so a batch is sharded
 *     by slicing the arrays (bench.py --gpus N: one rank per GPU, one gather of the small outputs).  Objects
 *     that own device memory (sfb_mpc_swarm) remember their device and refuse calls from another one.
 */
#ifndef SFB_H
#define SFB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sfb_status {
  SFB_OK              = 0,
  SFB_ERR_INVALID_ARG = 1,
  SFB_ERR_UNSUPPORTED = 2, /* size / option outside what the HIP kernels implement */
  SFB_ERR_HIP         = 3, /* a HIP runtime call failed; see sfb_last_error() */
  SFB_ERR_NO_DEVICE   = 4
} sfb_status;

/* smooth::feedback::QPSolutionStatus, qp.hpp:82-92 (declaration order == value) */
typedef enum sfb_qp_status {
  SFB_QP_OPTIMAL           = 0,
  SFB_QP_POLISH_FAILED     = 1,
  SFB_QP_PRIMAL_INFEASIBLE = 2,
  SFB_QP_DUAL_INFEASIBLE   = 3,
  SFB_QP_MAX_ITERATIONS    = 4,
  SFB_QP_MAX_TIME          = 5,
  SFB_QP_UNKNOWN           = 6
} sfb_qp_status;

/*
 * smooth::feedback::QPSolverParams, qp_solver.hpp:29-68.  Numeric options are `float` exactly as
 * in the reference and are widened to double at the same places (:353-356, :587, :593, ...).
 * std::optional members are encoded with a negative value meaning "unset".
 */
typedef struct sfb_qp_params {
  float alpha;              /* :35  relaxation parameter                (1.6f)  */
  float rho;                /* :37  first dual step size                (0.1f)  */
  float sigma;              /* :39  second dual step length             (1e-6f) */
  int32_t scaling;          /* :42  scale problem                       (1)     */
  float eps_abs;            /* :45                                      (1e-3f) */
  float eps_rel;            /* :47                                      (1e-3f) */
  float eps_primal_inf;     /* :49                                      (1e-4f) */
  float eps_dual_inf;       /* :51                                      (1e-4f) */
  int64_t max_iter;         /* :54  optional<uint32_t>; <0 = unset      (-1)    */
  int64_t max_time_ns;      /* :57  optional<nanoseconds>; <0 = unset   (-1).  As in the reference (:504-507) the
                                    limit is tested at stopping checks that leave the status open, against
                                    the time since THIS problem's solve started -- here on the device clock
                                    (10 ns ticks), per batch item, time spent suspended in a time-sliced
                                    launch included.  Wall-clock limits are nondeterministic by nature:
                                    prefer max_iter for reproducible runs.                       */
  uint32_t stop_check_iter; /* :60                                      (25)    */
  int32_t polish;           /* :63                                      (1)     */
  uint32_t polish_iter;     /* :65                                      (5)     */
  float delta;              /* :67                                      (1e-6f) */
  int32_t verbose;          /* :32  host-pointer entry points print a summary of the call (phase times,
                                    status histogram, iteration statistics) and, when the call is ONE problem,
                                    the reference's per-iteration table before it (:409-420, :490-501; as data
                                    for any batch: sfb_sparse_qp_solve_batch_trace); ignored by the asynchronous
                                    device-pointer entry points                 (0)     */
  int32_t reuse_factor;     /* NOT in the reference (which re-scales and re-factorises on every solve(), reusing
                                    only the symbolic analysis, :424-426).  Shared-pattern sparse entry points only;
                                    the dense kernels ignore it.  Non-zero = the caller vouches that P and A of
                                    EVERY item are bit-identical to what the previous call with the same plan,
                                    workspace, batch, sigma and scaling solved for that item (a time-invariant
                                    MPC: only q, l, u move between ticks).  The kernel then keeps, per item,
                                    whatever that call left in the workspace and this call would recompute to the
                                    same bits: the compacted A, the scaling when c (which depends on |q|) comes
                                    out the same, and the LDL' factor when additionally the rho vector (which
                                    rows are equalities) is unchanged -- otherwise it recomputes.  Results are
                                    bit-identical to a call without the flag by construction.  The first call
                                    on a workspace may set it too (nothing to keep yet).  Ignored for items a
                                    pruned plan's guard sends to the fallback pool and in launches with an
                                    explicit order (their workspace slots are not the items').   (0)     */
} sfb_qp_params;

/* With max_iter unset the reference loops until a stopping test fires (possibly forever, e.g.
 * stop_check_iter==1, qp_solver.hpp:465).  The device path bounds every solve by this many
 * iterations and reports SFB_QP_MAX_ITERATIONS (iter == cap) when it is hit. */
#define SFB_QP_DEVICE_ITER_CAP 20000000

/* The dense entry points accept every size; n+m decides which of four routes solves a batch (csrc/qp_dense_route.h):
 *   n+m <= 32 and no max_time_ns: four QPs per wavefront, factor in registers; per-QP records and a queue in device memory;
 *   otherwise n+m <= 128: one QP per wavefront, KKT matrix and factor on chip (registers / LDS).  No working memory
 *     while the device holds the batch's waves at once; larger batches run time-sliced over per-QP records in
 *     device memory;
 *   otherwise n+m <= SFB_QP_DENSE_BIG_MAX_K: one QP per wavefront with the KKT matrix and its PIVOTED dense LDL'
 *     (Eigen::LDLT<.,Upper>, qp_solver.hpp:259,:428,:462) in a per-QP HBM workspace (the reference's ASIF example,
 *     n = 3, m = 203, and test, n = 4, m = 301, are of this size);
 *   beyond: the shared-pattern sparse kernel with a full pattern -- same ADMM and stopping tests on the same
 *     matrix entries, but a fill-reducing elimination order without pivoting: agreement to rounding only.  Working
 *     memory: A by rows and the sparse kernel's workspace.
 * The first three share one arithmetic and are bit-identical to the dense CPU restatement, so the boundaries between
 * them never show in a result.  SFB_QP_DENSE_MAX_K marks none of these boundaries any more (up to it the on-chip route
 * keeps the factor in registers during the iterations); it stays defined for callers that refer to it. */
#define SFB_QP_DENSE_MAX_K 64
#define SFB_QP_DENSE_BIG_MAX_K 1024

const char *sfb_version(void);
/* Thread-local description of the last non-OK status returned on this thread. */
const char *sfb_last_error(void);

/* Debug knobs (tests, A/B measurements, diagnostics): launch shapes and engine choices, listed in
 * smooth_feedback_amd/csrc/knobs.h -- e.g. "SFB_SP_GRID" = "4" forces the time-sliced launch of the sparse kernel on a tiny
 * grid.  None changes a result.  value == NULL clears a knob; an unknown name is SFB_ERR_INVALID_ARG.  This call is the ONLY
 * way to set them: the library reads no environment variable. */
sfb_status sfb_debug_set(const char *name, const char *value);
/* Number of visible HIP devices (0 if none / runtime unusable). */
sfb_status sfb_device_count(int *count);

/*
 * Several devices from ONE process.  The reference has no parallelism (its benchmark "batch"
 * is a sequential for loop, benchmarks/bench_types.hpp:93); the items of a batch are independent, so a batch shards
 * trivially.  Two ways to use more than one GPU:
 *   - one process per GPU (torchrun / MPI): every entry point of this header works on the process's current device;
 *     the launcher shards the batch (bench.py, smooth_feedback_amd/sharding.py);
 *   - one process, the *_multi host-pointer entry points below: the batch is cut into one contiguous shard per entry
 *     of the device list, every shard runs on its own host thread with its device current (own plan upload, own
 *     workspace, own stream) and writes its slice of the caller's output arrays -- host memory is the gathering
 *     point, there is no device-to-device exchange on this path.  Results are identical to the single-device call.
 * sfb_set_devices: the device list of the *_multi entry points (default / count == 0: every visible device).  An
 * ordinal may appear more than once (its shards are then serialised on that device; used by the tests on 1-GPU boxes).
 */
sfb_status sfb_set_devices(const int *devices, int count);
sfb_status sfb_get_devices(int *devices, int capacity, int *count);

/* Defaults of QPSolverParams (qp_solver.hpp:29-68). */
void sfb_qp_params_default(sfb_qp_params *prm);

/*
 * Batched dense QP solve:   min 1/2 x'Px + q'x   s.t.  l <= Ax <= u      for `batch` problems.
 *
 * Replaces, per batch item, smooth::feedback::solve_qp(pbm, prm, warmstart)
 * (qp_solver.hpp:779-787) == QPSolver<QuadraticProgram<M,N,double>>(pbm, prm).solve(pbm, warmstart)
 * (:276, :343-568): scaling (:673-730), rho selection (:361-374), KKT + pivoted LDL' (:399-433),
 * ADMM loop with stopping tests every stop_check_iter iterations (:447-510, :574-644), polish
 * (:92-204, :515-539) and un-scaling (:544-548).
 *
 * Layout (qp.hpp:31-45, Eigen default column-major), item b at offset b*size:
 *   P  [batch][n*n]  col-major n x n (upper triangle feeds the KKT matrix, the full matrix is
 *                    used for residuals/objective exactly as the reference does)
 *   q  [batch][n]    A [batch][m*n] col-major m x n      l,u [batch][m]  (+-inf allowed)
 *   warm_x [batch][n], warm_y [batch][m]: previous primal/dual (both NULL = cold start)
 * Outputs (QPSolution, qp.hpp:95-108):
 *   x [batch][n] primal, y [batch][m] dual, obj [batch] (nullable), iter [batch] (nullable),
 *   code [batch] (sfb_qp_status values).
 * Non-finite data: like the reference, no input is validated -- NaN / inf in P, q, A propagate through the IEEE arithmetic
 * (l = +inf or u = -inf is the pre-check's PrimalInfeasible), and the kernels make of them exactly what the CPU restatement
 * does (tests/test_qp_dense_gpu.py, tests/test_qp_sparse_gpu.py::test_non_finite_*: codes, iteration counts and values up to
 * NaN payloads).  Shortcuts that rest on "0 times an entry is 0" (the first refinement round of polish) are covered by them.
 * Requires 1 <= n, 1 <= m, n+m <= 19 198 (the four routes by n+m: see SFB_QP_DENSE_MAX_K above).
 * Working memory: every route but the on-chip one (32 < n+m <= 128, or n+m <= 32 with max_time_ns, at a batch the device
 * holds at once) needs device memory beyond the arguments -- the four-per-wave records and queue, the factor in HBM,
 * the full-pattern sparse workspace, the records of a time-sliced on-chip launch.  This entry point takes it stream-ordered
 * (hipMallocAsync / hipFreeAsync) per call; sfb_qp_dense_solve_batch_ws below takes it from the caller instead.
 */
sfb_status sfb_qp_dense_solve_batch(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                    const double *q, const double *A, const double *l, const double *u,
                                    const double *warm_x, const double *warm_y, double *x, double *y,
                                    double *obj, uint32_t *iter, int32_t *code, void *stream);

/* Same (n+m <= 128) with the reference's verbose table (qp_solver.hpp:409-420, :490-501) as DATA: trace [batch][trace_rows][5]
 * (device) receives one row (ITER, OBJ, PRI_RES, DUA_RES, TIME in microseconds of the device clock since the solve began) per
 * stopping check of every problem, computed on the iterates of the solve itself; checks beyond trace_rows are dropped, the caller
 * presets ITER = -1 to tell used rows from unused ones.  One wave per problem whatever the batch size (a diagnostic path);
 * results are those of sfb_qp_dense_solve_batch, bit for bit.  SFB_ERR_UNSUPPORTED for n+m > 128. */
sfb_status sfb_qp_dense_solve_batch_trace(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                          const double *q, const double *A, const double *l, const double *u,
                                          const double *warm_x, const double *warm_y, double *x, double *y, double *obj,
                                          uint32_t *iter, int32_t *code, double *trace, int32_t trace_rows, void *stream);
/* Same, and the reference's closing summary (qp_solver.hpp:550-565) as DATA: phase_us (device, nullable) = batch x 16 doubles, of
 * which the first batch x 6 receive per problem the microseconds of the device's wall clock spent in
 *   [0] scaling and pre-check (before the reference's t0, :376)   [1] matrix filling (pivot order, zero, fill)
 *   [2] factorization   [3] iteration   [4] polish   [5] un-scale and report
 * (the remaining batch x 10 doubles are scratch for the kernel's stamps).  trace is nullable when trace_rows == 0. */
sfb_status sfb_qp_dense_solve_batch_phases(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                           const double *q, const double *A, const double *l, const double *u,
                                           const double *warm_x, const double *warm_y, double *x, double *y, double *obj,
                                           uint32_t *iter, int32_t *code, double *trace, int32_t trace_rows, double *phase_us,
                                           void *stream);

/*
 * Explicit workspaces.  The reference's QPSolver owns its work memory, allocated once by analyze()
 * (qp_solver.hpp:297-338) and re-used by every solve(); the equivalent here is an opaque device buffer the caller
 * creates once and hands to every call, so that no call allocates:
 *   sfb_qp_dense_workspace_bytes   device bytes a dense call of this shape needs (0 for 32 < n+m <= 64)
 *   sfb_workspace_create/destroy   device memory on the CURRENT device (bytes = 0 is allowed)
 *   sfb_workspace_info             its device pointer and size -- the pointer is also what the shared-pattern sparse
 *                                  entry points take as `workspace` (sfb_sparse_qp_plan_workspace_bytes)
 *   sfb_qp_dense_solve_batch_ws    sfb_qp_dense_solve_batch on that memory; asynchronous on `stream`.  One call at
 *                                  a time per workspace (calls on the same stream are ordered; use one workspace
 *                                  per stream otherwise).  SFB_ERR_INVALID_ARG if the workspace is too small or of
 *                                  another device.
 */
typedef struct sfb_workspace sfb_workspace;
sfb_status sfb_qp_dense_workspace_bytes(const sfb_qp_params *prm, int64_t batch, int n, int m, int64_t *bytes);
sfb_status sfb_workspace_create(int64_t bytes, sfb_workspace **out);
void sfb_workspace_destroy(sfb_workspace *workspace);
sfb_status sfb_workspace_info(const sfb_workspace *workspace, void **device_ptr, int64_t *bytes);
sfb_status sfb_qp_dense_solve_batch_ws(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                       const double *q, const double *A, const double *l, const double *u,
                                       const double *warm_x, const double *warm_y, double *x, double *y,
                                       double *obj, uint32_t *iter, int32_t *code, sfb_workspace *workspace,
                                       void *stream);

/* Same with host pointers (H2D copy, solve, D2H copy, synchronous) on the current device.  One device staging buffer
 * per device is kept between calls (the analogue of the working memory a reference QPSolver object keeps,
 * qp_solver.hpp:297-338); concurrent callers are not serialised.  sfb_host_staging_trim() frees what is kept. */
sfb_status sfb_qp_dense_solve_batch_host(const sfb_qp_params *prm, int64_t batch, int n, int m,
                                         const double *P, const double *q, const double *A, const double *l,
                                         const double *u, const double *warm_x, const double *warm_y,
                                         double *x, double *y, double *obj, uint32_t *iter, int32_t *code);
void sfb_host_staging_trim(void);
/* ... with the verbose table as data (trace [batch][trace_rows][5], HOST memory; see sfb_qp_dense_solve_batch_trace; n+m <= 128).
 * With prm->verbose on ONE problem of that size class the host entry point above prints this table itself. */
sfb_status sfb_qp_dense_solve_batch_host_trace(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                               const double *q, const double *A, const double *l, const double *u,
                                               const double *warm_x, const double *warm_y, double *x, double *y, double *obj,
                                               uint32_t *iter, int32_t *code, double *trace, int32_t trace_rows);
/* ... and the per-phase times (phase_us [batch][6], HOST memory, nullable; see sfb_qp_dense_solve_batch_phases).
 * sfb_qp_dense_solve_batch_host with prm->verbose set and batch == 1 prints table and summary from the same data. */
sfb_status sfb_qp_dense_solve_batch_host_phases(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                                const double *q, const double *A, const double *l, const double *u,
                                                const double *warm_x, const double *warm_y, double *x, double *y, double *obj,
                                                uint32_t *iter, int32_t *code, double *trace, int32_t trace_rows,
                                                double *phase_us);
/* ... and sharded over the device list (sfb_set_devices); same arguments, same results. */
sfb_status sfb_qp_dense_solve_batch_host_multi(const sfb_qp_params *prm, int64_t batch, int n, int m,
                                               const double *P, const double *q, const double *A, const double *l,
                                               const double *u, const double *warm_x, const double *warm_y,
                                               double *x, double *y, double *obj, uint32_t *iter, int32_t *code);

/*
 * Tall dense QPs (few unknowns, many rows -- a safety filter has n = nu + 1 and m = K nh + nu + 1): the reduced-KKT route.
 *
 * Same problem, same layout, same arguments and outputs as sfb_qp_dense_solve_batch / _host / _host_multi, and the same
 * algorithm (scaling, pre-check, rho classes, warm start, ADMM update, stopping checks, max_iter, max_time, polish,
 * un-scaling, objective).  What is reduced: the linear solves.  Instead of the pivoted LDL' of the (n+m) x (n+m) KKT matrix
 * [P + sigma I, A'; A, -diag(1/rho)], the m dual unknowns are eliminated first,
 *     S x = rhs_x + A' diag(rho) rhs_z,   S = P + sigma I + A' diag(rho) A  (n x n),   nu = diag(rho) (A x - rhs_z),
 * and S gets an unpivoted LDL' once per solve; polish solves (P + delta I + A_act' A_act / delta) the same way and keeps the
 * reference's refinement rounds against the unperturbed system.  A factorisation costs O(m n^2) instead of O((n+m)^3), an
 * iteration O(m n) instead of O((n+m)^2), and a problem with n = 3, m = 203 lives in the registers of one wavefront.
 * Results agree with sfb_qp_dense_solve_batch TO ROUNDING, NOT bit for bit: sums over the rows of A are wave reductions
 * and there is no pivoting, so iteration counts can differ where a stopping test is met within rounding.  This is an
 * opt-in route: sfb_qp_dense_solve_batch never takes it.  S must be positive definite (sigma > 0 or P + A'A definite);
 * a pivot that is not positive ends the solve with SFB_QP_UNKNOWN like a failed LDL' of the reference.
 * Sizes: 1 <= n <= SFB_QP_DENSE_TALL_MAX_N, 1 <= m <= SFB_QP_DENSE_TALL_MAX_M (so n + m may exceed the 19 198 of the
 * entry points above); anything else is SFB_ERR_UNSUPPORTED.
 * Working memory: none while a problem's rows fit in registers (m <= 512 for n <= 4, m <= 256 for n <= 8) or in LDS
 * ((3 + n) m doubles within 60 KB); beyond that 2 m doubles per problem are taken stream-ordered per call.
 */
#define SFB_QP_DENSE_TALL_MAX_N 16
#define SFB_QP_DENSE_TALL_MAX_M 1048576
sfb_status sfb_qp_dense_tall_solve_batch(const sfb_qp_params *prm, int64_t batch, int n, int m, const double *P,
                                         const double *q, const double *A, const double *l, const double *u,
                                         const double *warm_x, const double *warm_y, double *x, double *y,
                                         double *obj, uint32_t *iter, int32_t *code, void *stream);
/* ... with host pointers (synchronous, on the staging buffer sfb_qp_dense_solve_batch_host keeps) */
sfb_status sfb_qp_dense_tall_solve_batch_host(const sfb_qp_params *prm, int64_t batch, int n, int m,
                                              const double *P, const double *q, const double *A, const double *l,
                                              const double *u, const double *warm_x, const double *warm_y,
                                              double *x, double *y, double *obj, uint32_t *iter, int32_t *code);
/* ... and sharded over the device list (sfb_set_devices); same arguments, same results. */
sfb_status sfb_qp_dense_tall_solve_batch_host_multi(const sfb_qp_params *prm, int64_t batch, int n, int m,
                                                    const double *P, const double *q, const double *A, const double *l,
                                                    const double *u, const double *warm_x, const double *warm_y,
                                                    double *x, double *y, double *obj, uint32_t *iter, int32_t *code);

/* ------------------------------------------------------------------------------------------
 * Sparse QPs sharing ONE sparsity pattern (a swarm of MPC problems from the same transcription).
 *
 * Layout follows QuadraticProgramSparse (qp.hpp:60-79): P in CSC (Eigen::SparseMatrix default)
 * exactly as the caller stores it -- only entries with col >= row enter the KKT matrix
 * (qp_solver.hpp:384) while residuals/objective multiply by P as stored (:589,:547) --, A in CSR
 * (Eigen::RowMajor, qp.hpp:74).  Index arrays are shared by the batch; values are per item:
 *   Px [batch][nnzP], q [batch][n], Ax [batch][nnzA], l,u [batch][m].
 * Indices must be strictly ascending inside each column of P / row of A (Eigen compressed form).
 * ---------------------------------------------------------------------------------------- */
typedef struct sfb_sparse_qp_plan sfb_sparse_qp_plan; /* opaque */

/*
 * Symbolic analysis, once per pattern.  Replaces QPSolver<QuadraticProgramSparse>::analyze
 * (qp_solver.hpp:297-338) and SimplicialLDLT::analyzePattern (:424): KKT pattern, fill-reducing
 * elimination order, pattern of L.  Host only (no device needed).
 *   ordering: 0 natural, 1 minimum degree (Eigen's AMD is not reproducible without Eigen; any
 *   fill-reducing order yields the same algorithm up to rounding);  user_perm (n+m entries,
 *   new -> old, nullable) overrides `ordering`.
 */
sfb_status sfb_sparse_qp_plan_create(int n, int m, const int32_t *P_colptr, const int32_t *P_rowind,
                                     const int32_t *A_rowptr, const int32_t *A_colind, int ordering,
                                     const int32_t *user_perm, sfb_sparse_qp_plan **plan);
/* Same with a constrained minimum-degree order: stage[n+m] (nullable) -- unknowns (variables 0..n-1,
 * constraint duals n..n+m-1) of a lower stage are eliminated before any of a higher stage.  An MPC
 * transcription marks the states shared by neighbouring mesh intervals as stage 1: shorter
 * elimination tree and less fill than unconstrained minimum degree. */
sfb_status sfb_sparse_qp_plan_create_staged(int n, int m, const int32_t *P_colptr, const int32_t *P_rowind,
                                            const int32_t *A_rowptr, const int32_t *A_colind, int ordering,
                                            const int32_t *user_perm, const int32_t *stage,
                                            sfb_sparse_qp_plan **plan);
/*
 * Same for a transcription that stores entries of A which are zero for EVERY item (the reference's ocp_to_qp
 * writes dense Jacobian blocks: block_add, utils/sparse.hpp:33-50, ocp_to_qp.hpp:258-264 -- two thirds of the
 * stored entries of the SE2 x R^3 MPC problem are explicit zeros).  A_keep[nnzA] (nullable): 0 = the caller
 * declares this stored entry zero in every item solved with the plan.  The KKT pattern, the elimination order
 * and the pattern of L are built from the kept entries only (the headline MPC pattern: nnz(L) 41 030 -> 13 710);
 * the value arrays keep the caller's layout.  Exactness: a zero entry contributes exact zeros to every sum it
 * takes part in, so the results equal those of the whole pattern under the same elimination order up to the
 * sign of zeros.  The declaration is CHECKED on the device for every item: an item with a non-zero (or NaN)
 * masked entry is solved on the whole pattern instead (same elimination order), by fallback launches inside
 * the same call -- a wrong mask costs time, never correctness.
 */
sfb_status sfb_sparse_qp_plan_create_pruned(int n, int m, const int32_t *P_colptr, const int32_t *P_rowind,
                                            const int32_t *A_rowptr, const int32_t *A_colind, int ordering,
                                            const int32_t *user_perm, const int32_t *stage, const uint8_t *A_keep,
                                            sfb_sparse_qp_plan **plan);
void sfb_sparse_qp_plan_destroy(sfb_sparse_qp_plan *plan);
/* nnz of the KKT upper triangle, nnz of L (strictly lower), bytes of device workspace PER ITEM (batch times this
 * always suffices; sfb_sparse_qp_plan_workspace_bytes is the exact requirement of a call). */
sfb_status sfb_sparse_qp_plan_info(const sfb_sparse_qp_plan *plan, int64_t *nnzK, int64_t *nnzL,
                                   int64_t *workspace_bytes_per_item);
/* Exact device workspace of one call with `batch` items. */
sfb_status sfb_sparse_qp_plan_workspace_bytes(const sfb_sparse_qp_plan *plan, int64_t batch, int64_t *bytes);
/* Pruned plans: kept entries of A and nnz(L) of the fallback (whole-pattern) analysis; otherwise nnzA and nnz(L). */
sfb_status sfb_sparse_qp_plan_pruned_info(const sfb_sparse_qp_plan *plan, int64_t *nnzA_kept, int64_t *nnzL_fallback);
/* The elimination order in use (n+m entries, new -> old). */
sfb_status sfb_sparse_qp_plan_get_perm(const sfb_sparse_qp_plan *plan, int32_t *perm);
/* The order in which the numeric factorisation sums the contributions to an entry of L: rank[n+m] of every
 * column of the permuted matrix (a postorder of the plan's elimination tree; sources are summed in ascending
 * rank).  A floating-point detail, exposed so that a CPU restatement can reproduce the factor bit for bit.
 * fallback != 0: the order of a pruned plan's whole-pattern fallback analysis. */
sfb_status sfb_sparse_qp_plan_get_factor_order(const sfb_sparse_qp_plan *plan, int fallback, int32_t *rank);

/*
 * Batched sparse solve (device pointers, asynchronous on `stream`).  Replaces, per item,
 * QPSolver<QuadraticProgramSparse<double>>::solve(pbm, warmstart) (qp_solver.hpp:343-568 with the
 * sparse branches :379-397, :423-426, :452-460) as called by MPC::operator() (mpc.hpp:491).
 * `workspace`: device buffer of sfb_sparse_qp_plan_workspace_bytes(plan, batch) bytes (batch *
 * workspace_bytes_per_item always suffices), 16-byte aligned, caller-owned, reusable.
 * Outputs as sfb_qp_dense_solve_batch.
 */
sfb_status sfb_sparse_qp_solve_batch(sfb_sparse_qp_plan *plan, const sfb_qp_params *prm, int64_t batch,
                                     const double *Px, const double *q, const double *Ax, const double *l,
                                     const double *u, const double *warm_x, const double *warm_y, double *x,
                                     double *y, double *obj, uint32_t *iter, int32_t *code, void *workspace,
                                     void *stream);
/* Same with a launch order: order[batch] (device, nullable) is a permutation of 0..batch-1, launch position -> item.
 * The results do not depend on it.  A caller that can predict the iteration counts (an MPC swarm: those of the
 * previous tick) puts the longest-running items first, so that they run alongside the bulk of the batch instead of
 * finishing alone at the end of the launch. */
sfb_status sfb_sparse_qp_solve_batch_ordered(sfb_sparse_qp_plan *plan, const sfb_qp_params *prm, int64_t batch,
                                             const double *Px, const double *q, const double *Ax, const double *l,
                                             const double *u, const double *warm_x, const double *warm_y, double *x,
                                             double *y, double *obj, uint32_t *iter, int32_t *code, void *workspace,
                                             const int32_t *order, void *stream);
/* Same with the reference's verbose table (qp_solver.hpp:409-420, :490-501) as DATA: trace [batch][trace_rows][5] (device)
 * receives, per item and stopping check, one row (ITER, OBJ = (0.5 P x + q).x, PRI_RES = |A x - z|_inf,
 * DUA_RES = |P x + q + A'y|_inf on the unscaled iterate -- the reference's expressions -- and TIME in microseconds of
 * the device clock since the item's solve began); checks beyond trace_rows are dropped, the caller presets ITER = -1 to
 * recognise unused rows.  One wave per item without time slicing, same arithmetic and results as the plain call
 * (a launch of a separate instance of the kernel: diagnostics, not the fast path). */
sfb_status sfb_sparse_qp_solve_batch_trace(sfb_sparse_qp_plan *plan, const sfb_qp_params *prm, int64_t batch,
                                           const double *Px, const double *q, const double *Ax, const double *l,
                                           const double *u, const double *warm_x, const double *warm_y, double *x,
                                           double *y, double *obj, uint32_t *iter, int32_t *code, void *workspace,
                                           double *trace, int32_t trace_rows, void *stream);
/* Same, and the reference's closing summary (qp_solver.hpp:550-565: Matrix filling / Factorization / Iteration / Polish) as
 * DATA: phase_us [batch][6] (device, required) receives per item the microseconds of the device's wall clock spent in
 *   [0] scaling and pre-check (before the reference's t0, :376)   [1] matrix filling   [2] factorization   [3] iteration
 *   [4] polish   [5] un-scale and report
 * -- their sum is the time the item held its wavefront, [1] + .. + [4] is the reference's "Total time".  trace is nullable here.
 * Like the table: the TRACE instance of the kernel, one wave per item, same arithmetic and results as the plain call. */
sfb_status sfb_sparse_qp_solve_batch_phases(sfb_sparse_qp_plan *plan, const sfb_qp_params *prm, int64_t batch,
                                            const double *Px, const double *q, const double *Ax, const double *l,
                                            const double *u, const double *warm_x, const double *warm_y, double *x,
                                            double *y, double *obj, uint32_t *iter, int32_t *code, void *workspace,
                                            double *trace, int32_t trace_rows, double *phase_us, void *stream);
/* Same with host pointers (synchronous).  The device buffers are owned by the plan and kept between calls
 * (grow-only, freed by sfb_sparse_qp_plan_destroy) -- the analogue of the working memory a QPSolver object
 * keeps between solves (qp_solver.hpp:242-338); host-pointer calls on ONE plan and ONE device are serialised. */
sfb_status sfb_sparse_qp_solve_batch_host(sfb_sparse_qp_plan *plan, const sfb_qp_params *prm, int64_t batch,
                                          const double *Px, const double *q, const double *Ax, const double *l,
                                          const double *u, const double *warm_x, const double *warm_y,
                                          double *x, double *y, double *obj, uint32_t *iter, int32_t *code);
/* ... with the verbose table as data (trace [batch][trace_rows][5], HOST memory, nullable; see
 * sfb_sparse_qp_solve_batch_trace).  sfb_sparse_qp_solve_batch_host with prm->verbose set and batch == 1 -- the
 * reference's use of the flag, one QPSolver object -- collects the table this way and prints it in the reference's
 * format (header, one line per stopping check, summary). */
sfb_status sfb_sparse_qp_solve_batch_host_trace(sfb_sparse_qp_plan *plan, const sfb_qp_params *prm, int64_t batch,
                                                const double *Px, const double *q, const double *Ax, const double *l,
                                                const double *u, const double *warm_x, const double *warm_y, double *x,
                                                double *y, double *obj, uint32_t *iter, int32_t *code, double *trace,
                                                int32_t trace_rows);
/* ... and the per-phase times (phase_us [batch][6], HOST memory, nullable; see sfb_sparse_qp_solve_batch_phases).  With
 * prm->verbose set and batch == 1 the summary of qp_solver.hpp:550-565 is printed from them. */
sfb_status sfb_sparse_qp_solve_batch_host_phases(sfb_sparse_qp_plan *plan, const sfb_qp_params *prm, int64_t batch,
                                                 const double *Px, const double *q, const double *Ax, const double *l,
                                                 const double *u, const double *warm_x, const double *warm_y,
                                                 double *x, double *y, double *obj, uint32_t *iter, int32_t *code,
                                                 double *trace, int32_t trace_rows, double *phase_us);
/* ... and sharded over the device list (sfb_set_devices): one contiguous shard, host thread, plan upload and workspace
 * per device; same arguments, same results (calls on different devices are not serialised). */
sfb_status sfb_sparse_qp_solve_batch_host_multi(sfb_sparse_qp_plan *plan, const sfb_qp_params *prm, int64_t batch,
                                                const double *Px, const double *q, const double *Ax, const double *l,
                                                const double *u, const double *warm_x, const double *warm_y,
                                                double *x, double *y, double *obj, uint32_t *iter, int32_t *code);

/* ------------------------------------------------------------------------------------------
 * Device-side MPC assembly and the device-resident swarm.
 *
 * sfb_mpc_assemble_batch replaces, per agent, the numeric fill of the QP that MPC::operator() does before
 * the solve (mpc.hpp:473-486): ocp_to_qp_update_dyn (ocp_to_qp.hpp:240-275), ocp_to_qp_update_cr (:279-323)
 * and ocp_to_qp_update_ce (:326-373) -- given the per-node linearisation that needs the user's callbacks
 * (dynamics f, its right-Jacobians, the desired trajectory), which stays on the host.  The kernel performs
 * the arithmetic of those functions in their order, including ad(f + dxdes) of the state group (:262-264),
 * so A, l, u equal the host transcription bit for bit.
 *
 * Constraint rows [dyn (N*nx) | cr (N*ncr) | ce (nx)], variables [x_0..x_N (nx each) | u_0..u_{N-1} (nu each)],
 * N = kmesh * nivals collocation nodes; A in CSR with the pattern of ocp_to_qp_allocate (:56-69):
 *   dyn row (node M+i of interval starting at node M, component d):
 *        for j = 0..kmesh: block j == i -> nx entries (columns of x_{M+i}), else 1 entry (component d of x_{M+j});
 *        then nu entries (u_{M+i})                                   => kmesh + nx + nu entries
 *   cr row: nx entries (x_node) then nu entries (u_node);   ce row: nx entries (x_0).
 *
 * Per-agent record of the linearisation ("stage blocks"), contiguous doubles, matrices ROW-major (d, c):
 *   [ f (N*nx) | dxdes (N*nx) | dfdx (N*nx*nx) | dfdu (N*nx*nu) | c (N*ncr) | dcdx (N*ncr*nx) | dcdu (N*ncr*nu)
 *     | e (nx) | J (nx*nx) ]
 *   f, dfdx, dfdu: dynamics and right-Jacobians at (xdes(t+t_i), udes(t+t_i)); dxdes: body velocity of the
 *   desired trajectory; c, dcdx, dcdu: running constraint and Jacobians; e = xdes(t) (-) x and
 *   J = d^r exp^{-1}(e) (MPCCE, mpc.hpp:288-301).
 * With layout->jac_keep the Jacobian blocks are packed: [ f | dxdes | dfdx kept (N * n_fx) | dfdu kept | c | dcdx kept |
 * dcdu kept | e | J kept ].
 * If shared_jac is given (time-invariant linearisation: group-linear model on a fixed trajectory), the
 * Jacobians [dfdx | dfdu | dcdx | dcdu] are read from that ONE record and the per-agent record shrinks to
 *   [ f | dxdes | c | e | J ].
 * ---------------------------------------------------------------------------------------- */
typedef enum { SFB_LIE_RN = 0, SFB_LIE_SE2 = 1, SFB_LIE_SO3 = 2, SFB_LIE_SE3 = 3 } sfb_lie_kind;

typedef struct sfb_mpc_layout {
  int32_t nx, nu, ncr;      /* dof of state and input, running-constraint rows per node */
  int32_t kmesh, nivals;    /* collocation nodes per interval, intervals */
  double tf;                /* horizon (MPCParams::tf, mpc.hpp:322) */
  const double *alpha;      /* [nivals] interval scale alpha of interval_diffmat_unscaled (ocp_to_qp.hpp:243)  */
  const double *D;          /* [(kmesh+1)*kmesh] differentiation matrix, D[j*kmesh + i] = Dus(j, i) (:243,:268) */
  int32_t nparts;           /* components of the state bundle, in order; 0 = commutative state (no ad term) */
  const int32_t *part_kind; /* [nparts] sfb_lie_kind */
  const int32_t *part_dof;  /* [nparts] sums to nx (SE2 and SO3: 3, SE3: 6) */
  const double *crl, *cru;  /* [ncr] bounds of the running constraint (OCP::crl / cru as set by the MPC constructor) */
  const uint8_t *jac_keep;  /* nullable.  Packed per-agent Jacobians: one flag per entry of the blocks
                               [dfdx nx*nx | dfdu nx*nu | dcdx ncr*nx | dcdu ncr*nu | J nx*nx], row-major (d, c);
                               the record then holds, per node (J: once), only the entries whose flag is set, in
                               that order -- the others are 0.0 by the CALLER's guarantee (the dense Jacobian blocks
                               of a bundle state are mostly structural zeros: two thirds of the headline model's
                               record).  Ignored for records that share their Jacobians.  nu <= 32. */
} sfb_mpc_layout;

/* doubles in one per-agent record (shared_jac == 0: with the Jacobians) and in the shared Jacobian record */
int64_t sfb_mpc_record_doubles(const sfb_mpc_layout *layout, int shared_jac);
int64_t sfb_mpc_shared_jac_doubles(const sfb_mpc_layout *layout);
/* nnz of A for the layout */
int64_t sfb_mpc_nnzA(const sfb_mpc_layout *layout);

/* Device pointers, asynchronous on `stream`.  records [batch][record_doubles], shared_jac nullable,
 * Ax [batch][nnzA], l, u [batch][m = N*nx + N*ncr + nx].  layout and its arrays are host memory. */
sfb_status sfb_mpc_assemble_batch(const sfb_mpc_layout *layout, int64_t batch, const double *records,
                                  const double *shared_jac, double *Ax, double *l, double *u, void *stream);

/*
 * A swarm of `agents` MPC controllers with one transcription, resident on the device: P, q (constant over
 * ticks: set by the constructor, mpc.hpp:423), the warm start each agent keeps between calls (mpc.hpp:509-516) and all solver
 * memory stay in HBM.  One tick = upload the records, assemble, solve, store the warm starts, download the
 * small outputs.  Replaces the loop `for each agent: u = mpc(t, x)` (MPC::operator(), mpc.hpp:458-519).
 * Warm-started ticks launch the agents in descending order of their previous tick's iteration count
 * (sfb_sparse_qp_solve_batch_ordered).
 *   plan: pattern of the transcription's QP (its A pattern is checked against the layout); must outlive the swarm.
 *   Px [nnzP], q [n]: host, shared by all agents.
 */
typedef struct sfb_mpc_swarm sfb_mpc_swarm; /* opaque */
sfb_status sfb_mpc_swarm_create(sfb_sparse_qp_plan *plan, const sfb_mpc_layout *layout, const double *Px,
                                const double *q, int64_t agents, sfb_mpc_swarm **swarm);
void sfb_mpc_swarm_destroy(sfb_mpc_swarm *swarm);
/* forget the warm starts (MPC::reset_warmstart, mpc.hpp:603) */
sfb_status sfb_mpc_swarm_reset_warmstart(sfb_mpc_swarm *swarm);
/*
 * One tick, host pointers, synchronous.  records / shared_jac as above (host).  warmstart != 0: every agent
 * starts from the last solution it stored; a solution is stored when its code is Optimal, MaxTime or
 * MaxIterations (mpc.hpp:510-516), otherwise the agent keeps the older one.
 * Outputs (host): du0 [agents][nu] = primal entries of u_0 (the caller applies udes(t) (+) du0, mpc.hpp:518),
 * iter [agents] (nullable), code [agents], primal [agents][n] and dual [agents][m] (both nullable: full
 * solution for x_traj / u_traj, mpc.hpp:494-507).
 */
sfb_status sfb_mpc_swarm_step_host(sfb_mpc_swarm *swarm, const sfb_qp_params *prm, const double *records,
                                   const double *shared_jac, int warmstart, double *du0, uint32_t *iter,
                                   int32_t *code, double *primal, double *dual);

/* Pipelined upload (optional).  sfb_mpc_swarm_host_records returns a PINNED host buffer [agents][record_doubles
 * (shared_jac = 0)] owned by the swarm; the host threads that linearise write their agents' records straight into it
 * and announce finished ranges with sfb_mpc_swarm_upload(first, count), which starts an asynchronous copy on the
 * swarm's copy stream and returns at once -- the DMA of one chunk overlaps with the linearisation of the next.
 * sfb_mpc_swarm_step_host called with records == that buffer (and shared_jac == NULL) waits for those copies, uploads
 * whatever was not announced, and proceeds as above.  A range must not be rewritten between its upload and the step. */
sfb_status sfb_mpc_swarm_host_records(sfb_mpc_swarm *swarm, double **records);
sfb_status sfb_mpc_swarm_upload(sfb_mpc_swarm *swarm, int64_t first, int64_t count);

/* Records produced ON the device.  sfb_mpc_swarm_device_records returns the swarm's device record buffer
 * ([agents][record_doubles], the current packing); a caller whose model is device-callable fills it with its own kernel
 * (include/smooth_feedback_amd/mpc_device.hpp does, one thread per agent and node) on the null stream, and
 * sfb_mpc_swarm_step_resident runs the tick from there: assemble, solve, warm starts, small outputs -- nothing but the
 * agents' times and states goes up. */
sfb_status sfb_mpc_swarm_device_records(sfb_mpc_swarm *swarm, double **records, int64_t *record_doubles);
sfb_status sfb_mpc_swarm_step_resident(sfb_mpc_swarm *swarm, const sfb_qp_params *prm, int warmstart, double *du0,
                                       uint32_t *iter, int32_t *code, double *primal, double *dual);
/* A re-linearisation pass behind a tick (sequential convex MPC, include/smooth_feedback_amd/mpc_relin.hpp): the resident
 * tick for FLAT records -- dynamics and running constraint linearised about the plan of the last solve
 * (sfb_mpc_swarm_device_solution) in the same unknowns, written into the swarm's device record buffer by the caller's kernel
 * on the null stream.  Flat records are always UNPACKED (the record layout above, whatever the swarm's packing) and are
 * assembled in the commutative mode whatever the layout's state group: the Jacobians as they are, no ad(f + dxdes) term.
 * The warm start is always on: every agent starts from the solution it has stored.  An agent whose solve ends Optimal,
 * MaxTime or MaxIterations takes the new solution (and stores it); any other agent keeps the plan, dual, code and iteration
 * count it had, so the swarm's solution buffers hold every agent's last accepted plan.  Outputs as
 * sfb_mpc_swarm_step_resident, of the plans the swarm holds afterwards; same stream and ownership contract. */
sfb_status sfb_mpc_swarm_step_resident_flat(sfb_mpc_swarm *swarm, const sfb_qp_params *prm, double *du0, uint32_t *iter,
                                            int32_t *code, double *primal, double *dual);

/* Switch the packing of the per-agent records (layout->jac_keep semantics; NULL = unpacked) of an existing swarm --
 * e.g. back to full records when a linearisation turns out to have a non-zero where the flags said zero.  The swarm's
 * buffers are sized for unpacked records, warm starts and solver memory are untouched.  record_doubles (nullable)
 * receives the new record length.  Pending uploads are waited for and forgotten. */
sfb_status sfb_mpc_swarm_set_jac_keep(sfb_mpc_swarm *swarm, const uint8_t *jac_keep, int64_t *record_doubles);
/* Device buffers of the last tick (Ax [agents][nnzA], l, u [agents][m]) for inspection; valid until the next call. */
sfb_status sfb_mpc_swarm_debug_buffers(sfb_mpc_swarm *swarm, const double **Ax, const double **l, const double **u);
/* Device buffers of the last tick's solution (primal [agents][n], dual [agents][m], code [agents]; each nullable), for
 * work that continues on the device, such as the dynamics-error audit of mesh_device.hpp; valid until the next call. */
sfb_status sfb_mpc_swarm_device_solution(sfb_mpc_swarm *swarm, const double **primal, const double **dual,
                                         const int32_t **code);

/* ------------------------------------------------------------------------------------------
 * Batched Lie-group EKF: covariance propagation and Kalman update for `batch` independent filters.
 *
 * Replaces the matrix part of smooth::feedback::EKF<G>::predict / ::update (ekf.hpp:79-103,
 * :116-139).  The caller (host) keeps what needs the user's callbacks on the group:
 *   predict: A = -ad(f(t,g)) + d^r f/dx at the estimate (ekf.hpp:86-87) and the state step
 *            g <- g (+) dt f (:97);     update: H = d^r h/dx (:119), r = y (-) h(g), g <- g (+) delta (:137).
 * One predict call is ONE explicit-Euler substep of the covariance ODE (the default stepper,
 * ekf.hpp:30,:96); substepping and re-linearisation are the caller's loop exactly as in :93-102.
 * Layout: item-major contiguous, matrices column-major (Eigen default): P, A, Q [batch][dof*dof],
 * H [batch][ny*dof], R [batch][ny*ny], r [batch][ny], delta [batch][dof].  Only the upper triangles
 * of Q and R are read (ekf.hpp:77,:114).  q_shared / r_shared / dt_shared != 0: Q / R / dt point to
 * ONE matrix / scalar used by every item.  info[batch] (nullable): 0 ok, 1 = LDLT of S failed.
 * Supported sizes: dof, ny <= 16.  dof in {2,3,4,6,7} with ny in {1,2,3}, and (4,4), (6,6), run one filter per lane,
 * register-resident (the streaming kernels of the benchmark configuration); dof in {8,9,10} with ny <= 3 use a
 * per-lane update behind a separate predict launch; every other size (the reference's own tests also use (3,10))
 * runs one filter per wavefront with its matrices in LDS.  Same results in every case.
 * Device pointers, asynchronous on `stream`; P is updated in place.
 * ---------------------------------------------------------------------------------------- */
sfb_status sfb_ekf_predict_batch(int64_t batch, int dof, const double *A, const double *Q, int q_shared,
                                 const double *dt, int dt_shared, double *P, void *stream);
sfb_status sfb_ekf_update_batch(int64_t batch, int dof, int ny, const double *H, const double *R, int r_shared,
                                const double *r, double *P, double *delta, int32_t *info, void *stream);
/* predict with an explicit choice of the stepper (ekf.hpp:27-31: the Stp template argument): ONE step of the
 * covariance ODE dP/dt = symU(A P + P A' + Q) by explicit Euler (SFB_EKF_EULER == sfb_ekf_predict_batch) or by
 * boost::numeric::odeint::runge_kutta4 (SFB_EKF_RK4, the stepper tests/test_ekf.cpp:113-115 instantiates) with ONE
 * A for all four stages -- exact for dynamics f(t, x) that do not depend on t explicitly; see
 * sfb_ekf_predict_rk4_batch otherwise.  The state step g <- stepper(g) stays on the host. */
typedef enum { SFB_EKF_EULER = 0, SFB_EKF_RK4 = 1 } sfb_ekf_stepper;
sfb_status sfb_ekf_predict_stepper_batch(int stepper, int64_t batch, int dof, const double *A, const double *Q,
                                         int q_shared, const double *dt, int dt_shared, double *P, void *stream);
/* runge_kutta4 step of the covariance ODE with the linearisation at the stage times: the reference evaluates
 * A = -ad(f(t_s, g)) + d^r f/dx|_(t_s, g) inside cov_ode (ekf.hpp:84-89) at t_s = t (A), t + dt/2 (A_mid, stages 2
 * and 3) and t + dt (A_end); g is frozen during the covariance step (:96).  A_mid == A_end == NULL: A everywhere. */
sfb_status sfb_ekf_predict_rk4_batch(int64_t batch, int dof, const double *A, const double *A_mid, const double *A_end,
                                     const double *Q, int q_shared, const double *dt, int dt_shared, double *P,
                                     void *stream);
sfb_status sfb_ekf_predict_rk4_batch_host(int64_t batch, int dof, const double *A, const double *A_mid,
                                          const double *A_end, const double *Q, int q_shared, const double *dt,
                                          int dt_shared, double *P);
/* predict immediately followed by update in one launch (one pass over P). */
sfb_status sfb_ekf_predict_update_batch(int64_t batch, int dof, int ny, const double *A, const double *Q,
                                        int q_shared, const double *dt, int dt_shared, const double *H,
                                        const double *R, int r_shared, const double *r, double *P,
                                        double *delta, int32_t *info, void *stream);
/* Host-pointer variants (stage through device memory, synchronous).  Pass NULL A to skip predict,
 * NULL H to skip update. */
sfb_status sfb_ekf_predict_stepper_batch_host(int stepper, int64_t batch, int dof, const double *A, const double *Q,
                                              int q_shared, const double *dt, int dt_shared, double *P);
sfb_status sfb_ekf_step_batch_host(int64_t batch, int dof, int ny, const double *A, const double *Q, int q_shared,
                                   const double *dt, int dt_shared, const double *H, const double *R,
                                   int r_shared, const double *r, double *P, double *delta, int32_t *info);

/* ------------------------------------------------------------------------------------------
 * Batched Lie-group PID: smooth::feedback::PID<T, G>::operator() (pid.hpp:74-87) for `batch` independent controllers,
 * and the closed loop on the system the controller is designed for (d^r x = v, dv/dt = u; pid.hpp:29-35) in one launch.
 *
 * The group is described at run time like the state of sfb_mpc_layout: parts in order, each an sfb_lie_kind with its
 * dof (SFB_LIE_RN: any dof >= 1; SE2 and SO3: 3; SE3: 6), at most SFB_PID_MAX_PARTS parts.  Element storage per part:
 *   RN  N values | SE2 (x, y, cos, sin) | SO3 (w, x, y, z) | SE3 (px, py, pz, w, x, y, z)
 * a bundle is the concatenation of its parts, tangents are concatenated in the same order (SE2 (vx, vy, omega), SE3
 * (v, omega)).  elem = sfb_pid_elem_doubles(group), dof = sfb_pid_dof(group) (both -1 for a bad descriptor).
 * All arrays are [batch][...] contiguous doubles.  des_shared != 0: g_des, v_des (and a_des) hold ONE item used by every
 * agent; gains_shared != 0: the same for kp, kd, ki.  t_last [batch]: NaN = unset (first call).  windup_limit >= 0,
 * +inf = no clamp.  One agent per GPU lane; a bundle is run part by part (law, clamp and step are componentwise in the
 * tangent and rplus / rminus of a bundle act per part).  Device pointers, asynchronous on `stream`; the descriptor is
 * host memory.  SFB_ERR_INVALID_ARG for a bad descriptor, steps < 0, a non-finite dt, a negative or NaN windup_limit or
 * a NULL array with batch > 0, then SFB_ERR_NO_DEVICE without a device: both before any device work.
 * ---------------------------------------------------------------------------------------- */
#define SFB_PID_MAX_PARTS 8
typedef struct sfb_pid_group {
  int32_t nparts;           /* 1 .. SFB_PID_MAX_PARTS */
  const int32_t *part_kind; /* [nparts] sfb_lie_kind */
  const int32_t *part_dof;  /* [nparts] */
} sfb_pid_group;
int64_t sfb_pid_elem_doubles(const sfb_pid_group *group);
int64_t sfb_pid_dof(const sfb_pid_group *group);
/* One controller call at time t for every agent.  In: x [elem], v [dof], g_des [elem], v_des, a_des [dof], kp, kd, ki
 * [dof].  In/out: i_err [dof], t_last [1].  Out: u [dof]. */
sfb_status sfb_pid_step_batch(const sfb_pid_group *group, int64_t batch, double t, const double *x, const double *v,
                              const double *g_des, const double *v_des, const double *a_des, int des_shared,
                              const double *kp, const double *kd, const double *ki, int gains_shared,
                              double windup_limit, double *i_err, double *t_last, double *u, void *stream);
/* `steps` closed-loop ticks of length dt from t0 in ONE launch.  Every agent tracks the constant-twist reference
 * g_des(t) = rplus(g_des0, t v_des) with velocity v_des and acceleration 0 (recomputed from t each tick).  Tick k at
 * t_k = t0 + k dt: the law, u <- clamp(u, -u_max, u_max) (u_max [dof] shared by all agents, NULL: no clamp), then
 * x <- rplus(x, dt v + dt^2/2 u), v <- v + dt u (classical RK4 with u held, in closed form).  In/out: x, v, i_err,
 * t_last.  Out: u_last [dof] (the last tick's input) and cost [1] = sum_k dt |g_des(t_k) (-) x_k|^2 in tick order.
 * steps == 0 writes nothing. */
sfb_status sfb_pid_rollout_batch(const sfb_pid_group *group, int64_t batch, double t0, double dt, int64_t steps,
                                 double *x, double *v, const double *g_des0, const double *v_des, int des_shared,
                                 const double *kp, const double *kd, const double *ki, int gains_shared,
                                 double windup_limit, const double *u_max, double *i_err, double *t_last,
                                 double *u_last, double *cost, void *stream);
/* Host-pointer variants (stage through device memory, synchronous). */
sfb_status sfb_pid_step_batch_host(const sfb_pid_group *group, int64_t batch, double t, const double *x,
                                   const double *v, const double *g_des, const double *v_des, const double *a_des,
                                   int des_shared, const double *kp, const double *kd, const double *ki,
                                   int gains_shared, double windup_limit, double *i_err, double *t_last, double *u);
sfb_status sfb_pid_rollout_batch_host(const sfb_pid_group *group, int64_t batch, double t0, double dt, int64_t steps,
                                      double *x, double *v, const double *g_des0, const double *v_des, int des_shared,
                                      const double *kp, const double *kd, const double *ki, int gains_shared,
                                      double windup_limit, const double *u_max, double *i_err, double *t_last,
                                      double *u_last, double *cost);

/* ------------------------------------------------------------------------------------------
 * Batched Lie-group cubic splines (include/smooth_feedback_amd/spline.hpp: Spline<3, G>, fit_spline_cubic) and the PID
 * rollout that tracks them: waypoints -> curve -> closed loop without leaving the GPU.  The group is an sfb_pid_group,
 * elements and tangents are stored as for sfb_pid_*.  A spline has nknots = S + 1 >= 2 knots; per agent
 *   tk [S+1] knot times, strictly increasing | gk [S+1][elem] knot elements | V [S][3][dof] control differences
 * and the curve on segment i is g_i exp(B_1(u) v_i1) exp(B_2(u) v_i2) exp(B_3(u) v_i3) with the cumulative cubic Bernstein
 * basis, u = (s - tk[i]) / (tk[i+1] - tk[i]).  Before tk[0] the value is (g_0, 0, 0), after tk[S] it is (g_S, 0, 0).
 * spline_shared != 0: ONE spline (tk, gk, V) for every agent.  ts0 [batch], nullable (NULL: 0): agent b sees its spline at
 * time t - ts0[b], so a shared curve can be flown staggered.  One agent per GPU lane, a bundle part by part.  Device
 * pointers, asynchronous on `stream`.  SFB_ERR_INVALID_ARG, in this order, for a bad descriptor, batch < 0, nknots < 2,
 * nt < 0, steps < 0, a non-finite t0 / dt, a negative or NaN windup_limit, a NULL array with work to do; then
 * SFB_ERR_NO_DEVICE without a device: all before any device work, and there is no CPU fallback.  The device entry
 * points cannot see the knot times and trust them; the _host variants also refuse, when there is work to do (batch > 0,
 * and nt > 0 or steps > 0), knot times that are not finite and strictly increasing.
 * ---------------------------------------------------------------------------------------- */
/* The interpolating C^1 cubic through gk at tk (fit_spline_cubic; tk_shared != 0: one row of knot times for every agent).
 * Out: V.  Precondition: consecutive knots, after the end-velocity corrections, stay away from rotation angle pi. */
sfb_status sfb_spline_fit_cubic_batch(const sfb_pid_group *group, int64_t batch, int64_t nknots, const double *tk,
                                      int tk_shared, const double *gk, double *V, void *stream);
/* nt times per agent: t [batch][nt], or [nt] with t_shared != 0.  Out: g [batch][nt][elem], body velocity vel and body
 * acceleration acc [batch][nt][dof].  nt == 0 writes nothing. */
sfb_status sfb_spline_eval_batch(const sfb_pid_group *group, int64_t batch, int64_t nknots, const double *tk,
                                 const double *gk, const double *V, int spline_shared, const double *ts0, int64_t nt,
                                 const double *t, int t_shared, double *g, double *vel, double *acc, void *stream);
/* sfb_pid_rollout_batch with the spline as the desired trajectory: every other argument and all semantics are the same
 * (tick k at t0 + k dt, clamp, closed-form double-integrator step, u_last, cost in tick order, steps == 0 writes
 * nothing); agent b tracks (g, vel, acc) of its spline at t_k - ts0[b]. */
sfb_status sfb_pid_rollout_spline_batch(const sfb_pid_group *group, int64_t batch, double t0, double dt, int64_t steps,
                                        double *x, double *v, int64_t nknots, const double *tk, const double *gk,
                                        const double *V, int spline_shared, const double *ts0, const double *kp,
                                        const double *kd, const double *ki, int gains_shared, double windup_limit,
                                        const double *u_max, double *i_err, double *t_last, double *u_last, double *cost,
                                        void *stream);
/* Host-pointer variants (stage through device memory, synchronous). */
sfb_status sfb_spline_fit_cubic_batch_host(const sfb_pid_group *group, int64_t batch, int64_t nknots, const double *tk,
                                           int tk_shared, const double *gk, double *V);
sfb_status sfb_spline_eval_batch_host(const sfb_pid_group *group, int64_t batch, int64_t nknots, const double *tk,
                                      const double *gk, const double *V, int spline_shared, const double *ts0,
                                      int64_t nt, const double *t, int t_shared, double *g, double *vel, double *acc);
sfb_status sfb_pid_rollout_spline_batch_host(const sfb_pid_group *group, int64_t batch, double t0, double dt,
                                             int64_t steps, double *x, double *v, int64_t nknots, const double *tk,
                                             const double *gk, const double *V, int spline_shared, const double *ts0,
                                             const double *kp, const double *kd, const double *ki, int gains_shared,
                                             double windup_limit, const double *u_max, double *i_err, double *t_last,
                                             double *u_last, double *cost);

/* ------------------------------------------------------------------------------------------
 * ph collocation meshes (include/smooth_feedback_amd/mesh.hpp: Mesh<Kmin, Kmax>) and the batched dynamics-error
 * estimate (include/smooth_feedback_amd/dyn_error.hpp; reference collocation/dyn_error.hpp:28-73).  Model-free: the
 * caller evaluates its dynamics between the two calls, as with the EKF.
 *   1. sfb_mesh_resample_batch carries node values of the mesh to the points of the same mesh with every degree raised
 *      by one (K_s + 2 points per interval, the interval's end point included);
 *   2. the caller evaluates F = f(t, X, U) at those points (their times: t0 + (tf - t0) tau, tau from sfb_mesh_raised_nodes);
 *   3. sfb_mesh_dyn_error_batch integrates F through every interval and reports how far that lands from X.
 * The mesh is described by HOST arrays (also in the device-pointer entry points): K [nivals] collocation points per
 * interval, tau0 [nivals] interval starts on [0, 1], tau0[0] == 0, strictly increasing, below 1.  N = sum K.  The
 * library builds the per-degree tables (resampling weights, integration matrices) on the host in double
 * from the code of mesh.hpp and keeps them and the interval list on the device.  One GPU lane per (agent, interval,
 * raised point).  SFB_ERR_INVALID_ARG, in this order, for a NULL mesh or mesh array, nivals < 1, a K below 1 or with
 * K + 1 > 14, interval starts that are not as above, batch < 0, dim / nx < 0, a NULL array with work to do; then
 * SFB_ERR_NO_DEVICE without a device: all before any device work, and there is no CPU fallback.
 * ---------------------------------------------------------------------------------------- */
typedef struct sfb_mesh {
  int32_t nivals;
  const int32_t *K;   /* [nivals] host */
  const double *tau0; /* [nivals] host */
} sfb_mesh;
/* The points of the degree-raised mesh on [0, 1]: tau [sum_s (K_s + 2)], interval by interval, both end points included
 * (the order of the rows sfb_mesh_resample_batch writes).  Host arrays, CPU only: needs no device. */
sfb_status sfb_mesh_raised_nodes(const sfb_mesh *mesh, double *tau);
/* vals [batch][N + 1][dim] (extend != 0) or [batch][N][dim] (extend == 0: the last interval's polynomial goes through its
 * own K points only, Mesh::eval with extend = false).  Out: out [batch][sum_s (K_s + 2)][dim], interval by interval; an
 * interval's end point appears again as the next interval's first.  batch == 0 or dim == 0 writes nothing. */
sfb_status sfb_mesh_resample_batch(const sfb_mesh *mesh, int64_t batch, int32_t dim, int extend, const double *vals,
                                   double *out, void *stream);
/* X, F [batch][sum_s (K_s + 2)][nx] in the layout sfb_mesh_resample_batch writes (F at an interval's end point is never
 * read); horizon [batch] = tf - t0.  Out: errs [batch][nivals],
 *   Xest_j = X_0 + horizon sum_{i < Ke} F_i I(i, j - 1),  err = max_j |Xest_j - X_j| / (1 + max_{j >= 1} |X_j|),
 * Ke = K_s + 1, I the raised interval's integration matrix on [0, 1].  nx == 0 writes zeros. */
sfb_status sfb_mesh_dyn_error_batch(const sfb_mesh *mesh, int64_t batch, int32_t nx, const double *horizon,
                                    const double *X, const double *F, double *errs, void *stream);
/* Host-pointer variants (stage through device memory, synchronous). */
sfb_status sfb_mesh_resample_batch_host(const sfb_mesh *mesh, int64_t batch, int32_t dim, int extend, const double *vals,
                                        double *out);
sfb_status sfb_mesh_dyn_error_batch_host(const sfb_mesh *mesh, int64_t batch, int32_t nx, const double *horizon,
                                         const double *X, const double *F, double *errs);

/* ------------------------------------------------------------------------------------------
 * Functions over a mesh with first derivatives (include/smooth_feedback_amd/mesh_function.hpp: mesh_eval,
 * mesh_integrate, mesh_dyn; reference collocation/mesh_function.hpp:114-665).  Model-free: the caller evaluates its
 * model at the N collocation nodes (times t0 + (tf - t0) tau_i) and hands in
 *   F  [batch][N][nf]                  the values, and
 *   dF [batch][N][nf][1 + nx + nu]     the Jacobians, columns (t | x | u), right-Jacobians on a group;
 * the library does everything that depends on the mesh, with the arithmetic of the host front (one source).  Variables
 * are ordered [t0 | tf | x_0 .. x_N | u_0 .. u_{N-1}], numVars = 2 + nx (N + 1) + nu N.  The derivative of the two CSR
 * outputs comes as values out_dF_val [batch][nnz] in the order of one pattern per mesh, shared by every agent -- the
 * form (A pattern once, A values [agents][nnz]) a sparse QP plan consumes:
 *   eval: row (node i, output r) holds t0, tf, the nx columns of x_i, the nu columns of u_i;
 *   dyn:  row (node i = M_s + j of interval s, component d) holds t0, tf, for k = 0 .. K_s one entry (component d of
 *         x_{M_s + k}; for k == j the whole nx-wide block), then the nu columns of u_i: 2 + K_s + nx + nu entries,
 *         columns ascending -- the dyn row of sfb_mpc_layout with the two time columns in front.
 * dF == NULL together with a NULL derivative output: values only.  nu == 0 is legal.  One GPU lane per output double.
 * Errors as above (the mesh, then batch < 0), then nx < 0, nu < 0, nf < 0, sizes beyond 32-bit indices, dF without its
 * output or the reverse, a NULL array with work to do; then SFB_ERR_NO_DEVICE for the compute entries.  batch == 0
 * writes nothing.
 * ---------------------------------------------------------------------------------------- */
/* Patterns: rowptr [rows + 1], colind [nnz], rows = N nf (eval) or N nx (dyn).  Both arrays NULL: only *nnz is set.
 * Host arrays, CPU only: needs no device. */
sfb_status sfb_mesh_eval_pattern(const sfb_mesh *mesh, int32_t nx, int32_t nu, int32_t nf, int32_t *rowptr,
                                 int32_t *colind, int64_t *nnz);
sfb_status sfb_mesh_dyn_pattern(const sfb_mesh *mesh, int32_t nx, int32_t nu, int32_t *rowptr, int32_t *colind,
                                int64_t *nnz);
/* out_F [batch][N][nf] = w_i f_i (w_i: the quadrature weight when scale != 0, else 1) */
sfb_status sfb_mesh_eval_batch(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf, int scale,
                               const double *t0, const double *tf, const double *F, const double *dF, double *out_F,
                               double *out_dF_val, void *stream);
/* out_F [batch][nf] = (tf - t0) sum_i w_i f_i, the nodes added in order; out_dF [batch][nf][numVars] dense, the
 * columns of x_N zero */
sfb_status sfb_mesh_integrate_batch(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf,
                                    const double *t0, const double *tf, const double *F, const double *dF,
                                    double *out_F, double *out_dF, void *stream);
/* X [batch][N + 1][nx]; F is [batch][N][nx].  out_F [batch][N][nx] = w_i ((tf - t0) f_i - alpha_s sum_k D(k, j) x_{M_s + k}) */
sfb_status sfb_mesh_dyn_batch(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, const double *t0,
                              const double *tf, const double *X, const double *F, const double *dF, double *out_F,
                              double *out_dF_val, void *stream);
/* Host-pointer variants (stage through device memory, synchronous). */
sfb_status sfb_mesh_eval_batch_host(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf, int scale,
                                    const double *t0, const double *tf, const double *F, const double *dF,
                                    double *out_F, double *out_dF_val);
sfb_status sfb_mesh_integrate_batch_host(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, int32_t nf,
                                         const double *t0, const double *tf, const double *F, const double *dF,
                                         double *out_F, double *out_dF);
sfb_status sfb_mesh_dyn_batch_host(const sfb_mesh *mesh, int64_t batch, int32_t nx, int32_t nu, const double *t0,
                                   const double *tf, const double *X, const double *F, const double *dF, double *out_F,
                                   double *out_dF_val);

/* ------------------------------------------------------------------------------------------
 * The collocation NLP of an optimal control problem over a mesh (include/smooth_feedback_amd/ocp_to_nlp.hpp:
 * ocp_to_nlp; reference ocp_to_nlp.hpp).  t0 = 0.  Variables [tf | q (nq) | x_0 .. x_N | u_0 .. u_{N-1}],
 * n = 1 + nq + nx (N + 1) + nu N; constraints [dyn nx N | integrals nq | running ncr N | end nce].  With
 * ws = 1 / max(1e-6, max_i w_i):
 *   g = [ws mesh_dyn.F | ws (mesh_integrate.F - q) | ws mesh_eval(cr, scaled by the weights).F | ce(tf, x_0, x_N, q)]
 * and dg_dx comes as values dg_val [batch][nnz] over ONE CSR pattern per (mesh, dims), columns ascending, every
 * reserved entry stored:
 *   dyn row (node M_s + j, component d): tf, one entry per other node of the interval, the own nx-wide block, u_i;
 *   integral r: tf, q_r (the value -ws), x_0 .. x_{N-1}, u_0 .. u_{N-1};   running (node i, r): tf, x_i, u_i;
 *   end r: tf, q, x_0, x_N (unscaled).
 * Model-free like the entries above: the model arrives at the N nodes (times tf tau_i) as F [batch][N][nf] and
 * dF [batch][N][nf][1 + nx + nu] for f (nf = nx), g (nf = nq) and cr (nf = ncr), the end constraint as ce [batch][nce] and
 * dce [batch][nce][1 + 2 nx + nq], columns (tf | x0 | xf | q).  x [batch][n] holds each agent's own tf, q, X, U.  One
 * fused launch writes every output double once.  The four Jacobian inputs NULL together with dg_val NULL: values only.
 * A segment of length zero takes NULL arrays.  nx >= 1, the other dims >= 0.
 * Errors: the mesh, batch < 0, the dims, sizes beyond 32-bit indices, Jacobian inputs without dg_val or the reverse
 * (or only some of the Jacobian inputs that have work), a NULL array with work to do; then SFB_ERR_NO_DEVICE for
 * the compute entries.  batch == 0 writes nothing and returns SFB_OK with or without a device.
 * ---------------------------------------------------------------------------------------- */
typedef struct sfb_ocp_dims {
  int32_t nx, nu, nq, ncr, nce;
} sfb_ocp_dims;
/* var_beg: where tf, q, x, u start and n; con_beg: where the four constraint segments start and m.  Host only. */
sfb_status sfb_ocp_nlp_structure(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int64_t var_beg[5], int64_t con_beg[5]);
/* rowptr [m + 1], colind [nnz].  Both arrays NULL: only *nnz is set.  Host only. */
sfb_status sfb_ocp_nlp_pattern(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int32_t *rowptr, int32_t *colind,
                               int64_t *nnz);
/* xl, xu [n]: -inf / +inf except tf >= 0; gl, gu [m]: zero for dyn and integrals, ws w_i crl / cru per node, cel / ceu.
 * crl, cru [ncr], cel, ceu [nce].  Any output may be NULL.  Host only. */
sfb_status sfb_ocp_nlp_bounds(const sfb_mesh *mesh, const sfb_ocp_dims *dims, const double *crl, const double *cru,
                              const double *cel, const double *ceu, double *xl, double *xu, double *gl, double *gu,
                              double *w_scaling);
sfb_status sfb_ocp_nlp_batch(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int64_t batch, const double *x,
                             const double *Ff, const double *dFf, const double *Fg, const double *dFg, const double *Fcr,
                             const double *dFcr, const double *ce, const double *dce, double *g, double *dg_val,
                             void *stream);
/* Host-pointer variant (stages through device memory, synchronous). */
sfb_status sfb_ocp_nlp_batch_host(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int64_t batch, const double *x,
                                  const double *Ff, const double *dFf, const double *Fg, const double *dFg,
                                  const double *Fcr, const double *dFcr, const double *ce, const double *dce, double *g,
                                  double *dg_val);

/* ------------------------------------------------------------------------------------------
 * The Hessian of the Lagrangian of that NLP (OCPNLP::d2l_dx2 of ocp_to_nlp.hpp), the other half of each QP of a swarm
 * SQP iteration:
 *   H = sigma d2theta + ws (d2 dyn + d2 integrals + d2 running)(lambda) + sum_r lambda_ce[r] d2ce_r
 * as values hess_val [batch][nnzH] over ONE upper-triangle CSC pattern per (mesh, dims), rows ascending within a column,
 * every reserved entry stored -- the P_* form of a sparse QP plan, and the pattern of d2f_dx2 / d2g_dx2:
 *   column tf {tf};  q_r {tf, q_0 .. q_r};  component j of x_0 {tf, q, x_00 .. x_0j};  of x_i {tf, x_i0 .. x_ij};
 *   of x_N {tf, q, x_0, x_N0 .. x_Nj};  of u_i {tf, x_i, u_i0 .. u_ij}.
 * The q-x0 and q-xf blocks of theta and ce sit at (q, x0) and (q, xf).
 * Model-free, per agent (C order), with nz = 1 + nx + nu and ne = 1 + 2 nx + nq:
 *   x [n], lambda [m], sigma (one double);
 *   dFf [N][nx][nz], dFg [N][nq][nz], dFcr [N][ncr][nz]: the Jacobians sfb_ocp_nlp_batch takes (dFcr is accepted for
 *     symmetry and not read: the running constraints are not time-scaled; it may be NULL);
 *   HLf, HLg, HLcr [N][nz][nz]: the Hessian in (t, x, u) at node i of lambda_i . f, of lambda_q . g and of lambda_cr,i . cr,
 *     that is the model Hessians CONTRACTED with that node's multipliers by the caller (the multipliers of the integral
 *     rows are the same at every node).  Full square, row major; only r <= c is read.  Contracted because the
 *     uncontracted [N][nx][nz][nz] is 9 GB for nx = 12, nu = 2 on 52 nodes at 8 192 agents, and a caller with automatic
 *     differentiation gets the Hessian of lambda . f directly;
 *   d2theta [ne][ne], and d2ce_l [ne][ne] = sum_r lambda_ce[r] d2ce_r, rows and columns (tf | x0 | xf | q); only the
 *     part that is upper in the NLP's column order is read.
 * A segment with nq, ncr or nce of zero takes NULL arrays.  One launch writes every output double once; every sum runs
 * in one fixed order (nodes ascending; within a node f, g, cr; then theta, then ce), the order of the host front.
 * Errors: the mesh, batch < 0, the dims, sizes beyond 32-bit indices, a NULL array with work to do; then
 * SFB_ERR_NO_DEVICE for the compute entries.  batch == 0 writes nothing and returns SFB_OK with or without a device.
 * ---------------------------------------------------------------------------------------- */
/* colptr [n + 1], rowind [nnzH].  Both arrays NULL: only *nnz is set.  Host only. */
sfb_status sfb_ocp_nlp_hess_pattern(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int32_t *colptr, int32_t *rowind,
                                    int64_t *nnz);
/* Device pointers, asynchronous on `stream`. */
sfb_status sfb_ocp_nlp_hess_batch(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int64_t batch, const double *x,
                                  const double *lambda, const double *sigma, const double *dFf, const double *HLf,
                                  const double *dFg, const double *HLg, const double *dFcr, const double *HLcr,
                                  const double *d2theta, const double *d2ce_l, double *hess_val, void *stream);
/* Host-pointer variant (stages through device memory, synchronous). */
sfb_status sfb_ocp_nlp_hess_batch_host(const sfb_mesh *mesh, const sfb_ocp_dims *dims, int64_t batch, const double *x,
                                       const double *lambda, const double *sigma, const double *dFf, const double *HLf,
                                       const double *dFg, const double *HLg, const double *dFcr, const double *HLcr,
                                       const double *d2theta, const double *d2ce_l, double *hess_val);

/* ------------------------------------------------------------------------------------------
 * Swarm SQP: a solver for a batch of NLPs  min f(x) s.t. xl <= x <= xu, gl <= g(x) <= gu  that share n, m, the CSR pattern
 * of dg_dx (columns strictly ascending), the upper-triangle CSC pattern of the Lagrangian Hessian (rows strictly ascending,
 * EVERY diagonal entry present) and the bounds.  The law -- QP of an iteration, the shift ladder that convexifies it, the l1
 * merit line search, the stopping test -- is DESIGN.md, "Swarm SQP"; the inner solver is the shared-pattern sparse QP solver
 * above.  Model-free: the caller evaluates f, df, g, the CSR values of dg_dx and the CSC values of the Hessian of
 * f + lambda . g at the state's (x, lambda) and hands them in as device arrays, [batch] / [batch][len], C order.
 *
 * One iteration:  evaluate at x (sfb_nlp_sqp_state) -> sfb_nlp_sqp_direction -> while agents search: sfb_nlp_sqp_trial, evaluate
 * f and g at x_trial, sfb_nlp_sqp_accept.  An agent that has finished is frozen: no later call changes a bit of its state.
 * set_start, direction, trial and accept take the caller's stream (`hip_stream`: a hipStream_t, NULL = the null stream) and do
 * all their work on it -- kernels, the QP solve and the copy of the counts --, under the contract of the `*_batch` entries:
 * inputs are read behind the stream, outputs are complete for what the stream runs next.  direction and accept WAIT for that
 * stream (they hand a count back).  One handle serves one stream at a time.  Call order: a direction call starts a new
 * iteration for every unfinished agent; agents a caller left in line search are taken out of it, uncommitted.
 * status: a value of NLPSolution::Status (nlp.hpp; 0 Optimal, 1 PrimalInfeasible, 3 MaxIterations, 5 Unknown), or
 * SFB_NLP_RUNNING while the agent has not finished.
 * ---------------------------------------------------------------------------------------- */
#define SFB_NLP_RUNNING (-1)
typedef struct sfb_nlp_sqp_params {
  double tol;       /* Optimal when stationarity, violation and complementarity are all <= tol            (1e-6) */
  int64_t max_iter; /* MaxIterations when an agent has taken this many steps                              (50)   */
  double kappa;     /* a QP direction d != 0 is accepted only with d.P d >= kappa d.d                     (1e-8) */
  double mu_first;  /* first non-zero shift of the ladder                                                 (1e-4) */
  double mu_grow;   /* factor between rungs, > 1                                                          (8)    */
  double mu_max;    /* an agent whose shift grows beyond this ends Unknown (below mu_first: no shift)  (1e4)  */
  sfb_qp_params qp; /* the inner solver's (defaults, but eps_abs = eps_rel = 1e-9 and max_iter = 10000)          */
} sfb_nlp_sqp_params;
void sfb_nlp_sqp_params_default(sfb_nlp_sqp_params *p);

/* The pattern work, host only:
 *   the QP's P: BOTH triangles of the Hessian in CSC, rows ascending (the sparse solver takes the entries with col >= row into
 *     its KKT matrix but multiplies by P as stored in its stopping test, so a P stored as one triangle never reports Optimal),
 *     with the Hessian value each stored entry copies (P_src) and the slot of every diagonal (P_diag); nnzP = 2 nnzH - n;
 *   the QP's A: the rows of dg_dx, then one row e_j per variable with a finite xl_j or xu_j, ascending j: nb rows;
 *   a CSC view of dg_dx: per column its rows ascending and their positions in the CSR value array;
 *   the variable of every bound row.
 * A_rowptr [m + nb + 1], A_colind [nnzJ + nb], P_colptr [n + 1], P_rowind, P_src [nnzP], P_diag [n], Jc_colptr [n + 1],
 * Jc_row, Jc_pos [nnzJ], bound_var [nb].  All ten NULL: only *nb is set.  Errors (SFB_ERR_INVALID_ARG), in this order: bad
 * sizes (n < 1, m < 0, a NULL pattern or bound array), unsorted or out-of-range indices, a missing diagonal, xl > xu or
 * gl > gu, a NaN bound. */
sfb_status sfb_nlp_sqp_qp_pattern(int n, int m, const int32_t *J_rowptr, const int32_t *J_colind, const int32_t *H_colptr,
                                  const int32_t *H_rowind, const double *xl, const double *xu, const double *gl, const double *gu,
                                  int32_t *A_rowptr, int32_t *A_colind, int32_t *P_colptr, int32_t *P_rowind, int32_t *P_src,
                                  int32_t *P_diag, int32_t *Jc_colptr, int32_t *Jc_row, int32_t *Jc_pos, int32_t *bound_var,
                                  int64_t *nb);

typedef struct sfb_nlp_sqp sfb_nlp_sqp; /* opaque */
/* Patterns and bounds are host arrays.  params NULL: the defaults.  stage [n + m + nb] (nullable): elimination stages of the
 * QP plan (sfb_sparse_qp_plan_create_staged; the plan is made with ordering = 1).  Owns the plan, the QP arrays, the solver
 * workspace and the state of `batch` agents on the current device (the plan's own device copy, some KB of index tables, is uploaded by the first direction call; nothing
 * else is allocated later).  Errors: those of the pattern
 * builder, batch < 0, bad params, SFB_ERR_UNSUPPORTED for m + nb == 0; then SFB_ERR_NO_DEVICE.  batch == 0 is legal. */
sfb_status sfb_nlp_sqp_create(int n, int m, const int32_t *J_rowptr, const int32_t *J_colind, const int32_t *H_colptr,
                              const int32_t *H_rowind, const double *xl, const double *xu, const double *gl, const double *gu,
                              int64_t batch, const sfb_nlp_sqp_params *params, const int32_t *stage, sfb_nlp_sqp **solver);
void sfb_nlp_sqp_destroy(sfb_nlp_sqp *solver);
/* Any output may be NULL.  nnzH: stored entries of the Hessian pattern; nnzP, nnzA: of the QP's P and A. */
sfb_status sfb_nlp_sqp_info(const sfb_nlp_sqp *solver, int64_t *batch, int32_t *n, int32_t *m, int32_t *nb, int64_t *nnzH,
                            int64_t *nnzP, int64_t *nnzA);
/* x [batch][n], lambda [batch][m], z [batch][n]: device pointers, the multipliers nullable (zero).  Resets shift, penalty,
 * iteration count, status and the QP warm starts of every agent.  Asynchronous on `hip_stream`. */
sfb_status sfb_nlp_sqp_set_start(sfb_nlp_sqp *solver, const double *x, const double *lambda, const double *z,
                                 void *hip_stream);
/* The stopping test on the current (x, lambda, z), then for the agents that go on the QP of the iteration through the shift
 * ladder.  f [batch], df [batch][n], g [batch][m], dg_val [batch][nnzJ], hess_val [batch][nnzH]: device pointers.  *active
 * (host, nullable): agents that now hold a direction and are in line search.  SYNCHRONISES `hip_stream`: the host reads
 * one count per rung of the ladder (the rejected agents alone are solved again, compacted). */
sfb_status sfb_nlp_sqp_direction(sfb_nlp_sqp *solver, const double *f, const double *df, const double *g, const double *dg_val,
                                 const double *hess_val, int64_t *active, void *hip_stream);
/* x_trial [batch][n] (device) = clip(x + alpha d) for agents in line search, x for the rest.  Asynchronous on `hip_stream`. */
sfb_status sfb_nlp_sqp_trial(sfb_nlp_sqp *solver, double *x_trial, void *hip_stream);
/* The Armijo test from f_trial [batch], g_trial [batch][m] (device) at x_trial: commit or halve.  *searching (host, nullable):
 * agents still in line search.  Synchronises `hip_stream` for that count. */
sfb_status sfb_nlp_sqp_accept(sfb_nlp_sqp *solver, const double *f_trial, const double *g_trial, int64_t *searching,
                              void *hip_stream);
/* Device pointers into the state, any may be NULL: x, z [batch][n], lambda [batch][m], the others [batch]. */
sfb_status sfb_nlp_sqp_state(sfb_nlp_sqp *solver, const double **x, const double **lambda, const double **z, const int32_t **status,
                             const int32_t **iter, const double **r_stat, const double **r_pri, const double **r_comp,
                             const double **mu, const double **alpha, const double **nu);
/* Host-pointer variants of the five entries above (synchronous, null stream): inputs are staged through a device buffer the
 * first of these calls allocates (per agent 1 + n + m + nnzJ + nnzH doubles, freed with the handle), outputs are copied back.
 * What a host front for ONE problem -- solve_nlp_sqp of nlp_solver.hpp -- calls with batch 1.  Any output of _state_host may be
 * NULL. */
sfb_status sfb_nlp_sqp_set_start_host(sfb_nlp_sqp *solver, const double *x, const double *lambda, const double *z);
sfb_status sfb_nlp_sqp_direction_host(sfb_nlp_sqp *solver, const double *f, const double *df, const double *g,
                                      const double *dg_val, const double *hess_val, int64_t *active);
sfb_status sfb_nlp_sqp_trial_host(sfb_nlp_sqp *solver, double *x_trial);
sfb_status sfb_nlp_sqp_accept_host(sfb_nlp_sqp *solver, const double *f_trial, const double *g_trial, int64_t *searching);
sfb_status sfb_nlp_sqp_state_host(sfb_nlp_sqp *solver, double *x, double *lambda, double *z, int32_t *status, int32_t *iter,
                                  double *r_stat, double *r_pri, double *r_comp, double *mu, double *alpha, double *nu);
/* For tests (as sfb_mpc_swarm_debug_buffers): the QP arrays of the LAST rung, compacted -- slot k belongs to agent list[k] --
 * with its results (d, y, code, iter), and sums = [v1 | phi0 | D | d.d | d.P d], each [batch] by agent.  Any may be NULL. */
sfb_status sfb_nlp_sqp_debug_buffers(sfb_nlp_sqp *solver, const double **Px, const double **q, const double **Ax, const double **l,
                                     const double **u, const double **d, const double **y, const int32_t **code,
                                     const uint32_t **iter, const int32_t **list, const double **sums);

/*
 * Synthetic workload of the reference benchmark: random_qp(m, n, density, rng)
 * (benchmarks/bench_types.hpp:19-41) drawn `batch` times from ONE std::default_random_engine
 * seeded with `seed` (benchmarks/bench.cpp:146,170).  Host buffers, layout as above. CPU only.
 */
sfb_status sfb_random_qp_batch(uint32_t seed, int64_t batch, int m, int n, double density, double *P,
                               double *q, double *A, double *l, double *u);

#ifdef __cplusplus
}
#endif
#endif /* SFB_H */
