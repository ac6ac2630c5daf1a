"""Every QP route of the library against the oracle-free certificates of tests/qp_certify.py (and, where the CPU oracle
is affordable, bit for bit against the oracle): dense sizes at every kernel boundary, batch edges and launch knobs,
the shared-pattern sparse kernel under its launch knobs, and full-size batches certified on every item.
Each test prints its certified-item counts.  Needs an MI355X."""
import numpy as np
import pytest

import qp_certify as QC
import qp_families as QF
from sparse_cases import dense_batch_to_sparse

pytestmark = pytest.mark.gpu


def _same(r, ref):
    for a, b in ((r.code, ref["code"]), (r.iter, ref["iter"]), (r.primal, ref["x"]), (r.dual, ref["y"]),
                 (r.objective, ref["obj"])):
        assert np.array_equal(a, b, equal_nan=True)


def _dense(sfb, oracle, P, q, A, l, u, parity=True, warm=None, **kw):
    wx, wy = warm if warm is not None else (None, None)

    def solve(prm):
        r = sfb.solve_qp_batch_host(P, q, A, l, u, prm.sfb(sfb), warm_x=wx, warm_y=wy, **kw)
        if parity:
            _same(r, oracle.qp_dense_solve_batch(P, q, A, l, u, params=prm.oracle(oracle), warm_x=wx, warm_y=wy,
                                                 nthreads=16))
        return r
    return solve


# n + m at every dense boundary: four-per-wave (<= 32), one-per-wave / mid (<= 64, <= 128), big <8> with and without
# the diagonal cache (<= 384, <= 512), big <16> (<= 1024), sparse fallback (1025).  n + m = 1 has no QP (m >= 1).
KS = [2, 31, 32, 33, 48, 49, 64, 65, 127, 128, 129, 256, 257, 384, 385, 512, 513, 700, 1024, 1025]


@pytest.mark.parametrize("shape", ["wide", "tall"])
@pytest.mark.parametrize("k", KS)
def test_dense_sizes_at_every_boundary(sfb, oracle, k, shape):
    n = max(1, k // 8) if shape == "wide" else max(1, k - max(1, k // 4))
    m = k - n
    big = k > 512
    B = 3 if big else (4 if k > 256 else 12)
    prm = QC.Params(max_iter=2000 if big else 4000)
    verdict, (P, q, A, l, u) = QF.build("pd_mixed", B, n, m, seed=k * 7 + (shape == "tall"))
    prob = QC.Problem.dense(P, q, A, l, u)
    # k = 1025 runs on the sparse kernel, whose summation order is the sparse oracle's, not the dense one's
    _, _, s = QC.solve_and_certify(_dense(sfb, oracle, P, q, A, l, u, parity=k <= 1024), prob, prm, verdict)
    print(k, shape, n, m, s)


@pytest.mark.parametrize("n,m", [(48, 337), (100, 413), (64, 960)])
def test_big_dense_batched_lds_configuration(sfb, oracle, n, m):
    """A batch above the CU count (the batched LDS configuration of the big kernel) beyond the diagonal cache and in the
    <16> instance: certified on every item, parity on the first items (the dense CPU LDL' costs ~k^3)."""
    B = 300
    prm = QC.Params(max_iter=200)
    verdict, (P, q, A, l, u) = QF.build("pd_mixed", B, n, m, seed=n + m)
    prob = QC.Problem.dense(P, q, A, l, u)
    r1, r0, s = QC.solve_and_certify(_dense(sfb, oracle, P, q, A, l, u, parity=False), prob, prm, verdict)
    for r, p in ((r0, prm.but(polish=False)), (r1, prm)):   # parity on the first items of the batched launch
        ref = oracle.qp_dense_solve_batch(P[:3], q[:3], A[:3], l[:3], u[:3], params=p.oracle(oracle), nthreads=3)
        _same(type(r)(code=r.code[:3], iter=r.iter[:3], primal=r.primal[:3], dual=r.dual[:3], objective=r.objective[:3]), ref)
    print(n, m, s)


def test_big_dense_parity_after_a_batched_launch(sfb, oracle):
    """The <16> instance at n = 100, m = 413: a batch of 300 (batched LDS configuration) and then a batch of 3 (roomy)
    in the same process, each bit-identical to the dense oracle on the same items -- nothing of one launch may leak
    into the next."""
    n, m = 100, 413
    prm = QC.Params(max_iter=200)
    _, (P, q, A, l, u) = QF.build("pd_mixed", 300, n, m, seed=n + m)
    ref = oracle.qp_dense_solve_batch(P[:3], q[:3], A[:3], l[:3], u[:3], params=prm.oracle(oracle), nthreads=3)
    r = sfb.solve_qp_batch_host(P, q, A, l, u, prm.sfb(sfb))
    _same(type(r)(code=r.code[:3], iter=r.iter[:3], primal=r.primal[:3], dual=r.dual[:3], objective=r.objective[:3]), ref)
    r = sfb.solve_qp_batch_host(P[:3], q[:3], A[:3], l[:3], u[:3], prm.sfb(sfb))
    _same(r, ref)


@pytest.mark.parametrize("fam", list(QF.FAMILIES))
@pytest.mark.parametrize("n,m", [(1, 12), (5, 9), (10, 20), (30, 60), (60, 330)])
def test_dense_families_and_parameter_sweep(sfb, oracle, fam, n, m):
    """The verdict families through the dense routes under alpha {1, 1.6}, stop_check_iter {1, 2, 25}, eps_rel 0,
    scaling on / off, polish on / off, and warm starts."""
    B = 4 if n + m > 300 else 16
    verdict, (P, q, A, l, u) = QF.build(fam, B, n, m, seed=31 * n + m)
    prob = QC.Problem.dense(P, q, A, l, u)
    mi = 4000 if verdict == "feasible" else 200000
    for prm in (QC.Params(max_iter=mi), QC.Params(alpha=1.0, stop_check_iter=2, eps_rel=0.0, scaling=False, max_iter=mi),
                QC.Params(stop_check_iter=2, eps_rel=0.0, max_iter=mi), QC.Params(stop_check_iter=1, max_iter=150)):
        r1, _, s = QC.solve_and_certify(_dense(sfb, oracle, P, q, A, l, u), prob, prm, verdict, family=fam)
        print(fam, n, m, prm.alpha, prm.stop_check_iter, prm.scaling, s)
    warm = (np.nan_to_num(r1.primal) * 1.01, np.nan_to_num(r1.dual) * 0.99)
    _, _, s = QC.solve_and_certify(_dense(sfb, oracle, P, q, A, l, u, warm=warm), prob, QC.Params(max_iter=mi), verdict,
                                   family=fam)
    print(fam, "warm", s)


def test_dense_max_time_route(sfb, oracle):
    """max_time (k <= 32): codes 0 / 2 / 3 / 5 with consistent iteration counts and objectives."""
    _, (P, q, A, l, u) = QF.build("pd_mixed", 64, 10, 20, seed=3)
    prob = QC.Problem.dense(P, q, A, l, u)
    for mt in (1e-9, 1.0):
        prm = QC.Params(max_iter=4000, polish=False)
        r = sfb.solve_qp_batch_host(P, q, A, l, u, sfb.QPSolverParams(max_iter=4000, polish=False, max_time=mt))
        rep = QC.certify(prob, r, prm)
        assert rep.passed, str(rep)
        print(mt, rep)


@pytest.mark.parametrize("B", [5, 6, 7, 9])
@pytest.mark.parametrize("route", ["qp4_one_wave", "mid_sliced", "device_ptr", "workspace", "multi_device"])
def test_dense_batch_edges(sfb, oracle, knobs, route, B):
    import torch
    n, m = (10, 20) if route in ("qp4_one_wave", "device_ptr", "multi_device") else (20, 44)
    if route == "workspace":
        n, m = 40, 300
    if route == "qp4_one_wave":
        knobs.set(SFB_QP4_MAX_WAVES=1)
    if route == "mid_sliced":
        knobs.set(SFB_MID_GRID=2, SFB_MID_SLICE=1)
    verdict, (P, q, A, l, u) = QF.build("pd_edges", B, n, m, seed=B)
    prob = QC.Problem.dense(P, q, A, l, u)
    mm = l.shape[1]
    dev = torch.device("cuda:0")

    def device_solve(prm, ws=None):
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (P, q, A, l, u)]
        x = torch.empty((B, n), dtype=torch.float64, device=dev); y = torch.empty((B, mm), dtype=torch.float64, device=dev)
        obj = torch.empty(B, dtype=torch.float64, device=dev)
        it = torch.empty(B, dtype=torch.int32, device=dev); code = torch.empty(B, dtype=torch.int32, device=dev)
        args = [B, n, mm, *[a.data_ptr() for a in d], x.data_ptr(), y.data_ptr(), obj.data_ptr(), it.data_ptr(),
                code.data_ptr()]
        st = torch.cuda.current_stream().cuda_stream
        if ws is None:
            sfb.solve_qp_batch_device(*args, prm.sfb(sfb), stream=st)
        else:
            sfb.solve_qp_batch_device_ws(*args, ws, prm.sfb(sfb), stream=st)
        torch.cuda.synchronize()
        return dict(code=code.cpu().numpy(), iter=it.cpu().numpy().astype(np.uint32), x=x.cpu().numpy(),
                    y=y.cpu().numpy(), obj=obj.cpu().numpy())

    def solve(prm):
        if route == "device_ptr":
            r = device_solve(prm)
        elif route == "workspace":
            r = device_solve(prm, sfb.Workspace.for_dense(B, n, mm, prm.sfb(sfb)))
        else:
            r = sfb.solve_qp_batch_host(P, q, A, l, u, prm.sfb(sfb), multi_device=(route == "multi_device"))
        ref = oracle.qp_dense_solve_batch(P, q, A, l, u, params=prm.oracle(oracle), nthreads=8)
        for a, b in (("code", "code"), ("iter", "iter"), ("x", "x"), ("y", "y"), ("obj", "obj")):
            got = r[a] if isinstance(r, dict) else getattr(r, {"x": "primal", "y": "dual", "obj": "objective"}.get(a, a))
            assert np.array_equal(np.asarray(got), ref[b], equal_nan=True), (route, a)
        return r
    if route == "multi_device":
        sfb._capi.set_devices([0])
    try:
        _, _, s = QC.solve_and_certify(solve, prob, QC.Params(max_iter=3000), verdict)
    finally:
        if route == "multi_device":
            sfb._capi.set_devices()
    print(route, B, s)


SP_KNOBS = {"default": {}, "grid4": {"SFB_SP_GRID": 4}, "force_lat": {"SFB_SP_FORCE_LAT": 1}, "lat0": {"SFB_SP_LAT": 0},
            "polishers0": {"SFB_SP_POLISHERS": 0}, "units0": {"SFB_PLAN_UNITS": 0}}


@pytest.mark.parametrize("B", [1, 767, 768, 769])
@pytest.mark.parametrize("knob", list(SP_KNOBS))
def test_sparse_routes(sfb, oracle, knobs, knob, B):
    """The families through SparseQPPlan under every launch knob, around the hold threshold of 768 = 3 x 256 CUs;
    cold, warm and reuse_factor solves; parity with the sparse oracle on every item."""
    if SP_KNOBS[knob]:
        knobs.set(**SP_KNOBS[knob])
    n, m = 10, 20
    fams = ["pd_mixed", "pd_edges", "infeasible_zero_row", "unbounded_lp"]   # one m for the shared pattern
    per = -(-B // len(fams))
    parts = [QF.build(f, per, n, m, seed=B + i)[1] for i, f in enumerate(fams)]
    P, q, A, l, u = (np.concatenate([p[j] for p in parts])[:B] for j in range(5))
    verdict = np.repeat([QF.FAMILIES[f][0] for f in fams], per)[:B]
    mm = l.shape[1]
    Pp, Pi, Px, Ap, Aj, Ax = dense_batch_to_sparse(P, A, n, mm)
    plan = sfb.SparseQPPlan(n, mm, Pp, Pi, Ap, Aj)
    prob = QC.Problem.sparse(Pp, Pi, Px, q, Ap, Aj, Ax, l, u)
    state = {}

    def solve(prm):
        wx, wy = state.get("warm", (None, None))
        r = plan.solve_batch_host(Px, q, Ax, l, u, prm.sfb(sfb), warm_x=wx, warm_y=wy)
        ref = oracle.qp_sparse_solve_batch(Pp, Pi, Px, q, Ap, Aj, Ax, l, u, perm=plan.perm, forder=plan.factor_order(),
                                           params=prm.oracle(oracle), warm_x=wx, warm_y=wy, nthreads=16)
        _same(r, ref)
        return r
    r1, _, s = QC.solve_and_certify(solve, prob, QC.Params(max_iter=20000), verdict)
    print(knob, B, "cold", s)
    state["warm"] = (np.nan_to_num(r1.primal) * 1.01, np.nan_to_num(r1.dual) * 0.99)
    _, _, s = QC.solve_and_certify(solve, prob, QC.Params(max_iter=20000, reuse_factor=True), verdict)
    print(knob, B, "warm + reuse_factor", s)


@pytest.mark.parametrize("B", [1, 767, 768, 769])
def test_sparse_mpc_plan_routes(sfb, oracle, B):
    """The MPC plan (nx = 12, K = 50: n = m = 740) with its stage ordering, around the hold threshold."""
    from examples import models_lib as M
    d, Pp, Pi, Pv, Ap, Aj = M.mpc_pattern(12, 50)
    Av, l, u = M.mpc_assemble_batch(12, 50, B, seed=11)
    plan = sfb.SparseQPPlan(d["n"], d["m"], Pp, Pi, Ap, Aj, stage=M.mpc_stage(12, 50))
    Px, q = np.tile(Pv, (B, 1)), np.zeros((B, d["n"]))
    prob = QC.Problem.sparse(Pp, Pi, Px, q, Ap, Aj, Av, l, u)
    prm = QC.Params(max_iter=4000)
    r0 = plan.solve_batch_host(Px, q, Av, l, u, prm.but(polish=False).sfb(sfb))
    r1 = plan.solve_batch_host(Px, q, Av, l, u, prm.sfb(sfb))
    k = min(B, 8)
    for r, p in ((r0, prm.but(polish=False)), (r1, prm)):
        ref = oracle.qp_sparse_solve_batch(Pp, Pi, Px[:k], q[:k], Ap, Aj, Av[:k], l[:k], u[:k], perm=plan.perm,
                                           forder=plan.factor_order(), params=p.oracle(oracle), nthreads=8)
        assert np.array_equal(r.code[:k], ref["code"]) and np.array_equal(r.iter[:k], ref["iter"])
        assert np.array_equal(r.primal[:k], ref["x"]) and np.array_equal(r.dual[:k], ref["y"])
    reps = [QC.certify(prob, r0, prm.but(polish=False)), QC.certify(prob, r1, prm),
            QC.certify_polish(prob, r1, r0, prm, items=np.arange(min(B, 4)))]
    assert all(rp.passed for rp in reps), [str(rp) for rp in reps]
    print(B, [str(rp) for rp in reps])


def test_full_size_cfg2_certified_on_every_item(sfb):
    """BASELINE configs[1] at 65 536 QPs with general finite l, scaling on, polish off and on: every item certified,
    polish checked on every Optimal item whose reduced KKT matrix is well conditioned."""
    B, m, n = 65536, 20, 10
    P, q, A, l, u = sfb.random_qp_batch(5, B, m, n, 1.0)
    l = u - 1.0 - np.random.default_rng(0).random((B, m))
    prob = QC.Problem.dense(P, q, A, l, u)

    def solve(prm):
        return sfb.solve_qp_batch_host(P, q, A, l, u, prm.sfb(sfb))
    _, _, s = QC.solve_and_certify(solve, prob, QC.Params(max_iter=10000), None, min_polish_share=0.9)
    print(s)


def test_full_size_mpc_headline_certified_on_every_item(sfb):
    """The MPC headline batch (nx = 12, K = 50, 8 192 agents) with default parameters: the pruned plan and the
    polishers; every item certified with polish off, iteration counts and objectives with polish on, and the polish
    rules (code, iter, polish set) on every item."""
    from examples import models_lib as M
    B = 8192
    d, Pp, Pi, Pv, Ap, Aj = M.mpc_pattern(12, 50)
    Av, l, u = M.mpc_assemble_batch(12, 50, B, seed=3)
    keep = (Av != 0).any(axis=0)
    plan = sfb.SparseQPPlan(d["n"], d["m"], Pp, Pi, Ap, Aj, stage=M.mpc_stage(12, 50), keep=keep)
    Px, q = np.tile(Pv, (B, 1)), np.zeros((B, d["n"]))
    prob = QC.Problem.sparse(Pp, Pi, Px, q, Ap, Aj, Av, l, u)
    prm = QC.Params(max_iter=None)
    r0 = plan.solve_batch_host(Px, q, Av, l, u, prm.but(polish=False).sfb(sfb))
    r1 = plan.solve_batch_host(Px, q, Av, l, u, prm.sfb(sfb))
    reps = [QC.certify(prob, r0, prm.but(polish=False)), QC.certify(prob, r1, prm),
            QC.certify_polish(prob, r1, r0, prm, items=np.arange(16))]
    assert all(rp.passed for rp in reps), [str(rp) for rp in reps]
    assert reps[0].counts["optimal"] >= B // 2
    print([str(rp) for rp in reps])
