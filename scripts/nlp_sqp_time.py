"""Time of one sfb_nlp_sqp_direction call, inside the QP solve and outside it ("Swarm SQP"):
python scripts/nlp_sqp_time.py [agents] [intervals] [K] [nx] [nu] [nq] [ncr] [nce] [qp_iter].
Default: 8 192 agents on the MPC's 13 x 4 mesh, dims (12, 2, 1, 2, 12): n = 742, m = 741, one bounded variable (tf).
The patterns and bounds are the collocation NLP's (sfb_ocp_nlp_pattern / _hess_pattern / _bounds); the values are seeded random
numbers with a diagonally dominant Hessian -- the kernels around the solve move the same bytes whatever the values are, and
mu_max = 0 keeps the call to ONE rung, so that what is timed is: stopping test, compaction, assembly, one solve of every agent's
QP (capped at qp_iter iterations, default 200), judge, compaction.  The call ends in a device synchronise of its own (it brings a
count back), so a host clock around it is the call's time.  Timed alternately in one process, warmed, five windows of three calls,
the least window per call reported with the spread:
  direction       the whole call (set_start before it, outside the window, so that every agent is solved again);
  solve           sfb_sparse_qp_solve_batch alone on the QP arrays the call assembled, with a plan of the same patterns;
  solve, 1 iter   the same with max_iter = 1: the solve's set-up (scaling, factorisation) and one iteration.
outside = direction - solve."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(B=8192, nivals=4, K=13, nx=12, nu=2, nq=1, ncr=2, nce=12, qp_iter=200):
    import numpy as np
    import torch

    import smooth_feedback_amd as sfb

    mesh, dims = sfb.PHMesh.uniform(nivals, K), (nx, nu, nq, ncr, nce)
    Jp, Jj = sfb.ocp_nlp_pattern(mesh, dims)
    Hp, Hi = sfb.ocp_nlp_hess_pattern(mesh, dims)
    xl, xu, gl, gu, _ = sfb.ocp_nlp_bounds(mesh, dims, -np.ones(ncr), np.ones(ncr), np.zeros(nce), np.zeros(nce))
    n, m, nnzJ, nnzH = len(xl), len(gl), len(Jj), len(Hi)
    qp = sfb.QPSolverParams(eps_abs=1e-9, eps_rel=1e-9, max_iter=qp_iter)
    s = sfb.NLPSwarmSQP(n, m, Jp, Jj, Hp, Hi, xl, xu, gl, gu, B, sfb.NLPSQPParams(mu_max=0.0, qp=qp))
    gen = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)   # noqa: E731
    x, f, df, g, dg, hess = rnd(B, n), rnd(B), rnd(B, n), 0.1 * rnd(B, m), rnd(B, nnzJ), 0.1 * rnd(B, nnzH)
    x[:, 0] = 1.0 + x[:, 0].abs()
    diag = torch.from_numpy(np.asarray(Hi) == np.repeat(np.arange(n), np.diff(Hp))).to("cuda")
    hess[:, diag] = 10.0 + hess[:, diag].abs()
    pat = sfb.nlp_sqp_qp_pattern(n, m, Jp, Jj, Hp, Hi, xl, xu, gl, gu)
    plan = sfb.SparseQPPlan(n, s.mq, pat["P_colptr"], pat["P_rowind"], pat["A_rowptr"], pat["A_colind"], ordering=1)
    ws = torch.empty(plan.workspace_bytes(B) // 8 + 2, dtype=torch.float64, device="cuda")
    xs, ys = torch.empty((B, n), dtype=torch.float64, device="cuda"), torch.empty((B, s.mq), dtype=torch.float64, device="cuda")
    it, code = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    wx, wy = torch.zeros_like(xs), torch.zeros_like(ys)
    dbg = s.debug_views()

    def direction():
        s.set_start(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.direction(f, df, g, dg, hess)
        return time.perf_counter() - t0

    def solve(prm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan.solve_batch_device(B, *[dbg[k].data_ptr() for k in ("Px", "q", "Ax", "l", "u")], xs.data_ptr(), ys.data_ptr(), 0, it.data_ptr(),
                                code.data_ptr(), ws.data_ptr(), prm=prm, dwarm_x=wx.data_ptr(), dwarm_y=wy.data_ptr())
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    one = sfb.QPSolverParams(eps_abs=1e-9, eps_rel=1e-9, max_iter=1)
    what = {"direction": direction, "solve": lambda: solve(qp), "solve, 1 iter": lambda: solve(one)}
    for fn in what.values():                                                        # warm-up of every shape the windows use
        fn()
        fn()
    windows = {k: [] for k in what}
    for _ in range(5):
        for k, fn in what.items():
            windows[k].append(sum(fn() for _ in range(3)) / 3.0)
    ms = {k: 1e3 * min(v) for k, v in windows.items()}
    spread = {k: 1e3 * (max(v) - min(v)) for k, v in windows.items()}
    codes = np.bincount(dbg["code"].cpu().numpy(), minlength=7)
    print("swarm SQP direction: %d agents, n = %d, m = %d (+ %d bound rows), nnz dg %d, nnz H %d (P %d), QP capped at %d iterations" %
          (B, n, m, s.nb, nnzJ, nnzH, s.nnzP, qp_iter))
    for k in what:
        print("  %-14s %9.3f ms per call (spread %.3f ms over five windows of three calls)" % (k, ms[k], spread[k]))
    print("  %-14s %9.3f ms per call = direction - solve: stopping test, two compactions, assembly, judge, one count read back" %
          ("outside", ms["direction"] - ms["solve"]))
    print("  QP codes of the rung (Optimal, PolishFailed, PrimalInf, DualInf, MaxIter, MaxTime, Unknown): %s" % codes.tolist())
    return ms


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:]])
