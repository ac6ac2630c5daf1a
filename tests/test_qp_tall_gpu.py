"""The reduced-KKT route for tall dense QPs (sfb_qp_dense_tall_solve_batch*, csrc/qp_dense_tall.hip): every item against
the oracle-free certificates of tests/qp_certify.py, verdicts against the CPU oracle, the reference's known answers, launch
shapes, and the vehicle's safety filter with its opt-in switch.  The route agrees with the pivoted kernels to rounding, not
bit for bit: iteration counts and |dx| against the oracle are printed, not asserted.  Needs an MI355X."""
import numpy as np
import pytest

import qp_certify as QC
import qp_families as QF
from qp_cases import KNOWN_ANSWERS, as_batch, is_approx

pytestmark = pytest.mark.gpu

SHAPES = [(3, 203), (4, 301), (1, 12), (8, 64), (16, 1000), (3, 20000)]
ORACLE_MAX_K = 1016   # the dense CPU oracle keeps an (n+m)^2 matrix and costs (n+m)^3: up to (16, 1 000)


def _batch(n, m):
    return 2 if m >= 1000 else (8 if m > 100 else 16)


def _tall(sfb, P, q, A, l, u, warm=None, **kw):
    wx, wy = warm if warm is not None else (None, None)
    return lambda prm: sfb.solve_qp_tall_batch_host(P, q, A, l, u, prm.sfb(sfb), warm_x=wx, warm_y=wy, **kw)


def _param_sets(mi):
    """those of test_qp_certify_gpu.py::test_dense_families_and_parameter_sweep (solve_and_certify runs each with polish
    off and on)"""
    return (QC.Params(max_iter=mi), QC.Params(alpha=1.0, stop_check_iter=2, eps_rel=0.0, scaling=False, max_iter=mi),
            QC.Params(stop_check_iter=2, eps_rel=0.0, max_iter=mi), QC.Params(stop_check_iter=1, max_iter=150))


@pytest.mark.parametrize("fam", list(QF.FAMILIES))
@pytest.mark.parametrize("n,m", SHAPES)
def test_tall_families_certified_and_verdicts_like_the_oracle(sfb, oracle, fam, n, m):
    """Certificates on every item under the parameter sweep, polish off / on and a warm start; (3, 20 000) lies beyond what
    sfb_qp_dense_solve_batch_host accepts.  Up to (16, 1 000) the oracle solves the same items with default parameters:
    equal codes on the infeasible / unbounded families (asserted), share of equal iteration counts and the largest
    scaled |dx| on the feasible ones (printed), and the polish certificate's counts for both (printed)."""
    B = _batch(n, m)
    verdict, (P, q, A, l, u) = QF.build(fam, B, n, m, seed=31 * n + m)
    mm = l.shape[1]
    prob = QC.Problem.dense(P, q, A, l, u)
    mi = 4000 if verdict == "feasible" else 200000
    r1 = None
    for i, prm in enumerate(_param_sets(mi)):
        r1_, r0_, s = QC.solve_and_certify(_tall(sfb, P, q, A, l, u), prob, prm, verdict, family=fam)
        print("tall", fam, n, mm, "alpha", prm.alpha, "sci", prm.stop_check_iter, "scaling", prm.scaling, s)
        if i == 0:
            r1, r0 = r1_, r0_
    warm = (np.nan_to_num(r1.primal) * 1.01, np.nan_to_num(r1.dual) * 0.99)
    _, _, s = QC.solve_and_certify(_tall(sfb, P, q, A, l, u, warm=warm), prob, QC.Params(max_iter=mi), verdict, family=fam)
    print("tall", fam, n, mm, "warm", s)
    if n + mm > ORACLE_MAX_K + 4:
        print("tall", fam, n, mm, "oracle: not run at this size ((n+m)^2 doubles per item)")
        return
    prm = QC.Params(max_iter=mi)
    o0 = oracle.qp_dense_solve_batch(P, q, A, l, u, params=prm.but(polish=False).oracle(oracle), nthreads=16)
    o1 = oracle.qp_dense_solve_batch(P, q, A, l, u, params=prm.oracle(oracle), nthreads=16)
    pol_t, pol_o = QC.certify_polish(prob, r1, r0, prm), QC.certify_polish(prob, o1, o0, prm)
    print("polish", fam, n, mm, "tall", pol_t.counts, pol_t.worst, "passed", pol_t.passed, "| oracle", pol_o.counts, pol_o.worst,
          "passed", pol_o.passed)
    assert pol_t.passed or not pol_o.passed, "polished items fail certify_polish where the oracle's pass: " + str(pol_t)
    if verdict != "feasible":
        assert np.array_equal(r0.code, o0["code"]), (r0.code.tolist(), o0["code"].tolist())
    else:
        same_iter = float(np.mean(r0.iter == o0["iter"]))
        fin = np.isfinite(o0["x"]).all(axis=1) & np.isfinite(r0.primal).all(axis=1)
        scale = 1.0 + np.abs(o0["x"]).max(axis=1)
        dx = (np.abs(r0.primal - o0["x"]).max(axis=1) / scale)[fin]
        eq = r0.iter == o0["iter"]
        dx_eq = (np.abs(r0.primal - o0["x"]).max(axis=1) / scale)[fin & eq]
        print("rounding", fam, n, mm, "codes equal", bool(np.array_equal(r0.code, o0["code"])), "share equal iter %.3f" % same_iter,
              "max scaled |dx| %.3g (items with equal iter: %.3g)" % (dx.max(initial=0.0), dx_eq.max(initial=0.0)))


def test_beyond_the_old_size_limit(sfb):
    """(3, 20 000): n + m > 19 198 is refused by the pivoted entry point and solved (certified above) by the new one."""
    n, m = 3, 20000
    _, (P, q, A, l, u) = QF.build("pd_mixed", 1, n, m, seed=5)
    with pytest.raises(sfb._capi.SfbError) as e:
        sfb.solve_qp_batch_host(P, q, A, l, u, sfb.QPSolverParams(max_iter=50))
    assert e.value.status == sfb._capi.SFB_ERR_UNSUPPORTED
    r = sfb.solve_qp_tall_batch_host(P, q, A, l, u, sfb.QPSolverParams(max_iter=4000))
    assert int(r.code[0]) == 0


@pytest.mark.parametrize("name", sorted(k for k, c in KNOWN_ANSWERS.items() if len(c[1]) <= 16))
def test_known_answers(sfb, name):
    """tests/test_qp.cpp:54-336 through the reduced-KKT route at that file's tolerances, incl. the hot start."""
    case = KNOWN_ANSWERS[name]
    P, q, A, l, u = as_batch(case)
    prm = sfb.QPSolverParams(max_iter=100000)
    code, primal, ptol, objv, otol = case[5:]
    r = sfb.solve_qp_tall_batch_host(P, q, A, l, u, prm)
    r2 = sfb.solve_qp_tall_batch_host(P, q, A, l, u, prm, warm_x=np.nan_to_num(r.primal), warm_y=np.nan_to_num(r.dual))
    for s in (r, r2):
        assert int(s.code[0]) == code
        if primal is not None:
            assert is_approx(s.primal[0], primal, ptol)
        if objv is not None:
            assert abs(s.objective[0] - objv) <= otol


def _device_solve(sfb, B, n, m, P, q, A, l, u, prm):
    import torch
    dev = torch.device("cuda:0")
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (P, q, A, l, u)]
    x = torch.empty((B, n), dtype=torch.float64, device=dev); y = torch.empty((B, m), dtype=torch.float64, device=dev)
    obj = torch.empty(B, dtype=torch.float64, device=dev)
    it = torch.empty(B, dtype=torch.int32, device=dev); code = torch.empty(B, dtype=torch.int32, device=dev)
    sfb.solve_qp_tall_batch_device(B, n, m, *[a.data_ptr() for a in d], x.data_ptr(), y.data_ptr(), obj.data_ptr(), it.data_ptr(),
                                   code.data_ptr(), prm, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return sfb.QPBatchSolution(code=code.cpu().numpy(), iter=it.cpu().numpy().astype(np.uint32), primal=x.cpu().numpy(),
                               dual=y.cpu().numpy(), objective=obj.cpu().numpy())


@pytest.mark.parametrize("B", [1, 5, 767, 769, 65536])
def test_launch_shapes(sfb, B):
    """Batch edges at (3, 203): the device-pointer, host and sharded entries give identical bits, and the results certify."""
    n, m = 3, 203
    verdict, (P, q, A, l, u) = QF.build("pd_mixed", B, n, m, seed=B)
    prm = QC.Params(max_iter=4000, polish=False)
    rh = sfb.solve_qp_tall_batch_host(P, q, A, l, u, prm.sfb(sfb))
    rd = _device_solve(sfb, B, n, m, P, q, A, l, u, prm.sfb(sfb))
    sfb._capi.set_devices([0, 0])   # two shards on the one device
    try:
        rm = sfb.solve_qp_tall_batch_host(P, q, A, l, u, prm.sfb(sfb), multi_device=True)
    finally:
        sfb._capi.set_devices()
    for r in (rd, rm):
        for a in ("code", "iter", "primal", "dual", "objective"):
            assert np.array_equal(getattr(r, a), getattr(rh, a), equal_nan=True), a
    rep = QC.certify(QC.Problem.dense(P, q, A, l, u), rh, prm)
    assert rep.passed, str(rep)
    assert QF.verdict_ok(verdict, rh.code, prm).all()
    print(B, rep)


@pytest.mark.parametrize("n,m", [(17, 40), (3, (1 << 20) + 1)])
def test_sizes_outside_the_limits(sfb, n, m):
    """n > 16 or m > 2^20: SFB_ERR_UNSUPPORTED from every entry, before any argument is read."""
    import ctypes as C
    cp = sfb.QPSolverParams().to_c()
    p = np.zeros(8).ctypes.data
    L = sfb._capi.lib
    for fn in (L.sfb_qp_dense_tall_solve_batch_host, L.sfb_qp_dense_tall_solve_batch_host_multi):
        assert fn(C.byref(cp), 1, n, m, p, p, p, p, p, None, None, p, p, p, p, p) == sfb._capi.SFB_ERR_UNSUPPORTED
    assert L.sfb_qp_dense_tall_solve_batch(C.byref(cp), 1, n, m, p, p, p, p, p, None, None, p, p, p, p, p, None) == sfb._capi.SFB_ERR_UNSUPPORTED


def test_vehicle_filter_switch_first_tick_and_drift(sfb):
    """The vehicle's ASI filter (K = 200: n = 3, m = 203, polish off), 2 048 vehicles, switch off and on: equal codes on the
    first tick from the same states; over several ticks every QP of the new route certified; the largest difference of the
    filtered inputs printed."""
    from examples import models_lib as M
    B, K = 2048, 200
    st, ud = M.asif_swarm_states(B, seed=0)
    prm = QC.Params(polish=False, max_iter=None)
    for ticks in (1, 2, 4):
        new = M.asif_swarm_device_step(st, ud, K, ticks=ticks, reduced_kkt=True)
        old = M.asif_swarm_device_step(st, ud, K, ticks=ticks)
        if ticks == 1:
            assert np.array_equal(new["code"], old["code"])
            for k in ("P", "q", "A", "l", "ub"):
                assert np.array_equal(new[k], old[k]), k   # the same QPs went in
        prob = QC.Problem.dense(new["P"], new["q"], new["A"], new["l"], new["ub"])
        res = dict(code=new["code"], iter=new["iter"], x=new["x"], y=new["y"],
                   obj=np.einsum("bi,bi->b", new["x"], 0.5 * np.einsum("bji,bj->bi", new["P"].reshape(B, 3, 3), new["x"]) + new["q"]))
        rep = QC.certify(prob, res, prm)
        assert rep.passed, str(rep)
        print("ticks", ticks, rep, "| codes equal %.4f" % float(np.mean(new["code"] == old["code"])),
              "iter equal %.4f" % float(np.mean(new["iter"] == old["iter"])),
              "max |du| %.3g" % float(np.abs(new["u"] - old["u"]).max()))


def test_swarm_follows_the_circle_with_the_switch_on():
    """tests/test_vehicle_swarm_gpu.py's scenario with the filter on the reduced-KKT route: every vehicle stays off the obstacle."""
    from examples import models_lib as M
    batch, ticks = 48, 620
    r = M.vehicle_swarm_sim(batch, ticks, K_mpc=30, K_asif=200, seed=0, reduced_kkt=True)
    assert r["mpc_bad"].sum() == 0 and r["asif_bad"].sum() == 0
    assert np.all(np.isfinite(r["xy"])) and np.all(np.isfinite(r["u_asif"]))
    assert np.array_equal(r["xy"][0, 0], [0.0, 0.0])
    assert r["u_asif"][..., 0].min() >= -0.2 - 5e-3 and r["u_asif"][..., 0].max() <= 0.5 + 5e-3
    assert np.abs(r["u_asif"][..., 1]).max() <= 0.5 + 5e-3
    assert -0.1 < r["hmin"].min() < 0.3
    active = np.abs(r["u_asif"] - r["u_mpc"]).max(axis=2) > 1e-3
    assert 0.02 < active.mean() < 0.6
    assert not active[:100].any()
    rad = np.linalg.norm(r["xy"][350:450], axis=2)
    assert np.median(np.abs(rad - 2.5)) < 0.1 and np.abs(rad - 2.5).max() < 0.8
    print("hmin", r["hmin"].min(), "seconds per tick (MPC, ASIF)", r["seconds"][50:].mean(axis=0))
