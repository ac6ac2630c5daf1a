"""The CPU oracle against optimality certificates that do not use it (tests/qp_certify.py), on QP families whose verdict
is known from their construction (tests/qp_families.py), for the dense and the sparse oracle; and mutation tests that
show the certificates fail on corrupted results.  Every kernel is pinned bit for bit to the oracle, so this pins what
the kernels compute to what a solution means.  No GPU needed."""
import numpy as np
import pytest

import qp_certify as QC
import qp_families as QF
from sparse_cases import dense_batch_to_sparse

SIZES = [(1, 12), (5, 9), (10, 20), (30, 60)]
MAX_ITER = {"feasible": 4000, "infeasible": 200000, "unbounded": 200000}  # detection of infeasibility can be slow
# the parameter sweep: alpha {1, 1.6}, stop_check_iter {1, 2, 25}, eps_rel 0, scaling on / off (polish on and off in
# every case, see QC.solve_and_certify)
PARAMS = {
    "default": QC.Params(),
    "a1_sci2_rel0_noscale": QC.Params(alpha=1.0, stop_check_iter=2, eps_rel=0.0, scaling=False),
    "a16_sci2_rel0": QC.Params(stop_check_iter=2, eps_rel=0.0),
    "a1_sci25_noscale": QC.Params(alpha=1.0, scaling=False),
    "sci1": QC.Params(stop_check_iter=1, max_iter=300),
}


def _dense_solver(oracle, P, q, A, l, u, warm=None):
    def solve(prm):
        wx, wy = warm if warm is not None else (None, None)
        return oracle.qp_dense_solve_batch(P, q, A, l, u, params=prm.oracle(oracle), warm_x=wx, warm_y=wy, nthreads=8)
    return solve


def _aggregate(total, s):
    for k in ("optimal", "polish_checked", "polish_skipped"):
        total[k] = total.get(k, 0) + s[k]


@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("n,m", SIZES)
def test_dense_oracle_meets_the_certificates_on_every_family(oracle, n, m, pname):
    prm, total = PARAMS[pname], {}
    for fam in QF.FAMILIES:
        verdict, (P, q, A, l, u) = QF.build(fam, 24 if n + m < 90 else 8, n, m, seed=1000 * n + m)
        prob = QC.Problem.dense(P, q, A, l, u)
        p = prm.but(max_iter=MAX_ITER[verdict] if prm.stop_check_iter >= 2 else prm.max_iter)
        _, _, s = QC.solve_and_certify(_dense_solver(oracle, P, q, A, l, u), prob, p, verdict, family=fam)
        _aggregate(total, s)
        print(fam, s)
    if prm.stop_check_iter >= 2 and n >= 10 and prm.scaling:   # small n: a few active rows make the KKT matrix singular
        assert total["polish_checked"] >= 0.9 * total["optimal"] > 0, total
    print("total", total)


def test_dense_oracle_certificates_near_400_and_warm_starts(oracle):
    """n + m = 390 (the size of the big kernel's diagonal cache), and warm starts from a perturbed solution."""
    total = {}
    for fam in ("pd_mixed", "pd_edges", "infeasible_pair", "unbounded_rankdef"):
        verdict, (P, q, A, l, u) = QF.build(fam, 3, 60, 330, seed=7)
        prob = QC.Problem.dense(P, q, A, l, u)
        _, _, s = QC.solve_and_certify(_dense_solver(oracle, P, q, A, l, u), prob, QC.Params(max_iter=4000), verdict)
        _aggregate(total, s)
    for fam in QF.FAMILIES:
        verdict, (P, q, A, l, u) = QF.build(fam, 16, 10, 20, seed=99)
        r = oracle.qp_dense_solve_batch(P, q, A, l, u, params=QC.Params().oracle(oracle), nthreads=8)
        wx, wy = np.nan_to_num(r["x"]) * 1.01, np.nan_to_num(r["y"]) * 0.99
        prob = QC.Problem.dense(P, q, A, l, u)
        _, _, s = QC.solve_and_certify(_dense_solver(oracle, P, q, A, l, u, (wx, wy)), prob, QC.Params(), verdict)
        _aggregate(total, s)
    assert total["polish_checked"] >= 0.75 * total["optimal"] > 0, total   # measured: 49 of 60
    print(total)


@pytest.mark.parametrize("pname", ["default", "a1_sci2_rel0_noscale", "sci1"])
@pytest.mark.parametrize("n,m", [(1, 12), (10, 20), (30, 60)])
def test_sparse_oracle_meets_the_certificates_on_every_family(oracle, n, m, pname):
    """The same families through the sparse oracle (shared pattern = union of the batch's nonzeros, P stored in full)."""
    prm, total = PARAMS[pname], {}
    for fam in QF.FAMILIES:
        verdict, (P, q, A, l, u) = QF.build(fam, 16, n, m, seed=2000 * n + m)
        mm = l.shape[1]
        Pp, Pi, Px, Ap, Aj, Ax = dense_batch_to_sparse(P, A, n, mm)
        prob = QC.Problem.sparse(Pp, Pi, Px, q, Ap, Aj, Ax, l, u)

        def solve(p):
            return oracle.qp_sparse_solve_batch(Pp, Pi, Px, q, Ap, Aj, Ax, l, u, params=p.oracle(oracle), nthreads=8)
        _, _, s = QC.solve_and_certify(solve, prob, prm.but(max_iter=MAX_ITER[verdict] if prm.stop_check_iter >= 2 else prm.max_iter), verdict,
                                       family=fam)
        _aggregate(total, s)
    if prm.stop_check_iter >= 2 and n >= 10 and prm.scaling:
        assert total["polish_checked"] >= 0.9 * total["optimal"] > 0, total


def test_infeasibility_verdicts_confirmed_by_linprog(oracle):
    """Oracle-free cross-check of a sample of code 2 / code 3 verdicts (HiGHS): the least box violation is > 0, the
    recession LP has a descent direction."""
    seen = {2: 0, 3: 0}
    for fam in ("infeasible_pair", "infeasible_zero_row", "unbounded_lp", "unbounded_rankdef"):
        for n, m in ((3, 8), (10, 20)):
            _, (P, q, A, l, u) = QF.build(fam, 6, n, m, seed=5 + n)
            r = oracle.qp_dense_solve_batch(P, q, A, l, u, params=QC.Params().oracle(oracle), nthreads=8)
            for b in range(6):
                c = int(r["code"][b])
                assert c in (2, 3), (fam, b, c)
                assert QF.linprog_confirms(P[b], q[b], A[b], l[b], u[b], n, l.shape[1], c), (fam, n, m, b, c)
                seen[c] += 1
    assert seen[2] >= 10 and seen[3] >= 10, seen


# --------------------------------------------------------------------------------------------------------------------
# mutation tests: the certificates must catch each corruption
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def passing(oracle):
    n, m = 10, 20
    _, (P, q, A, l, u) = QF.build("pd_mixed", 32, n, m, seed=3)
    prob = QC.Problem.dense(P, q, A, l, u)
    prm = QC.Params(polish=False)
    r0 = oracle.qp_dense_solve_batch(P, q, A, l, u, params=prm.oracle(oracle), nthreads=8)
    r1 = oracle.qp_dense_solve_batch(P, q, A, l, u, params=prm.but(polish=True).oracle(oracle), nthreads=8)
    assert QC.certify(prob, r0, prm).passed and QC.certify_polish(prob, r1, r0, prm.but(polish=True)).passed
    opt = np.flatnonzero((r0["code"] == 0))
    assert opt.size >= 16
    return prob, prm, r0, r1, opt


def _copy(r):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def _obj(prob, x):
    X = x.astype(QC.LD)
    Px = QC._mv(prob.prow, prob.pcol, prob.Pv, X, prob.n)
    return np.sum(X * (QC.LD(0.5) * Px + prob.q.astype(QC.LD)), axis=1).astype(np.float64)


def test_mutation_primal_moved_by_ten_tolerances(passing):
    prob, prm, r0, _, opt = passing
    b = opt[0]
    bad = _copy(r0)
    Ax = QC._mv(prob.arow, prob.acol, prob.Av[b:b + 1], bad["x"][b:b + 1].astype(QC.LD), prob.m)[0].astype(float)
    j = 0
    a = np.zeros(prob.m); col = prob.acol == j
    a[prob.arow[col]] = prob.Av[b, col]                     # column j of A
    step = 10 * (1e-3 + 1e-3 * np.abs(Ax).max()) / max(np.abs(a).max(), 1e-12)
    bad["x"][b, j] += step
    bad["obj"] = _obj(prob, bad["x"])                       # keep the objective consistent: only the residuals see it
    rep = QC.certify(prob, bad, prm)
    assert not rep.passed and not rep.ok[b], str(rep)


def test_mutation_one_dual_sign_flipped(passing):
    prob, prm, r0, _, opt = passing
    b = opt[0]
    i = int(np.argmax(np.abs(r0["y"][b])))
    assert abs(r0["y"][b, i]) > 1e-3
    bad = _copy(r0)
    bad["y"][b, i] = -bad["y"][b, i]
    rep = QC.certify(prob, bad, prm)
    assert not rep.ok[b], str(rep)


def test_mutation_codes_of_two_items_swapped(passing):
    prob, prm, r0, _, _ = passing
    a = int(np.flatnonzero(r0["code"] == 0)[0])
    b = int(np.flatnonzero(r0["code"] != 0)[0]) if (r0["code"] != 0).any() else a + 1
    bad = _copy(r0)
    if bad["code"][a] == bad["code"][b]:                    # all Optimal: make the swap visible with a max_iter item
        bad["code"][b] = QC.CODE_MAX_ITER
        bad["iter"][b] = prm.max_iter
    bad["code"][[a, b]] = bad["code"][[b, a]]
    rep = QC.certify(prob, bad, prm)
    assert not rep.passed, str(rep)


def test_mutation_iteration_count_off_by_one(passing):
    prob, prm, r0, _, opt = passing
    for d in (-1, 1):
        bad = _copy(r0)
        bad["iter"][opt[0]] = int(bad["iter"][opt[0]]) + d
        assert not QC.certify(prob, bad, prm).ok[opt[0]]


def test_mutation_stale_objective(passing):
    prob, prm, r0, r1, opt = passing
    bad = _copy(r1)
    bad["obj"] = r0["obj"].copy()                           # the objective of the iterate before polish
    changed = opt[r0["obj"][opt] != r1["obj"][opt]]
    assert changed.size
    rep = QC.certify(prob, bad, prm.but(polish=True))
    assert not rep.ok[changed].any(), str(rep)


def test_mutation_pre_polish_values_returned(passing):
    prob, prm, r0, r1, opt = passing
    rep = QC.certify_polish(prob, _copy(r0), r0, prm.but(polish=True))
    failed = ~rep.ok[opt]
    assert failed.mean() >= 0.9, str(rep)


def test_mutation_one_dual_outside_the_polish_set_moved_by_one_ulp(passing):
    prob, prm, r0, r1, opt = passing
    caught = 0
    for b in opt[:8]:
        S = r1["y"][b] != r0["y"][b]
        outside = np.flatnonzero(~S)
        assert outside.size
        i = outside[0]
        bad = _copy(r1)
        bad["y"][b, i] = np.nextafter(bad["y"][b, i], np.inf)
        caught += not QC.certify_polish(prob, bad, r0, prm.but(polish=True)).ok[b]
    assert caught == min(8, opt.size)


def test_polish_iter_zero_leaves_zeros(oracle):
    _, (P, q, A, l, u) = QF.build("pd_mixed", 16, 10, 20, seed=4)
    prob = QC.Problem.dense(P, q, A, l, u)
    prm = QC.Params(polish_iter=0)
    _, r0, s = QC.solve_and_certify(_dense_solver(oracle, P, q, A, l, u), prob, prm, "feasible")
    assert s["polish_checked"] == s["optimal"] > 0
    # and a result with a nonzero x is caught
    r1 = oracle.qp_dense_solve_batch(P, q, A, l, u, params=prm.oracle(oracle), nthreads=8)
    b = int(np.flatnonzero(r1["code"] == 0)[0])
    bad = _copy(r1)
    bad["x"][b, 0] = 1e-300
    assert not QC.certify_polish(prob, bad, r0, prm).ok[b]
