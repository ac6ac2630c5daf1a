"""Every regime of the sparse plan on the GPU: the patterns of tests/sparse_zoo.py (engine, LDS budget, segment mix and sweep
encoding each pinned by name; tests/test_sparse_plan_host.py validates the same plans' schedules on the CPU) through
SparseQPPlan.solve_batch_host against the sparse CPU oracle -- codes, iterations, primal, dual and objective bit for bit --
and against the independent optimality certificates of tests/qp_certify.py.  Needs an MI355X."""
import numpy as np
import pytest

import qp_certify as QC
import sparse_zoo as Z
from test_mpc_gpu import sweep_mode  # noqa: F401  (fixture: the forms of the sweeps' value loads)
from test_qp_dense_gpu import _compare, _oracle_params

pytestmark = pytest.mark.gpu

UNIT_DEFAULT = [n for n in Z.NAMES if Z.EXPECT[n][2] == 1]      # the supernodal engine is the other engine there
CASES = [(n, B, "default") for n in Z.NAMES for B in (1, 3)] + [(n, B, "units0") for n in UNIT_DEFAULT for B in (1, 3)]


def _solve_and_check(sfb, oracle, name, B):
    z = Z.batch(name, B)
    Pp, Pi, Ap, Aj = z["Pp"], z["Pi"], z["Ap"], z["Aj"]
    Px, q, Ax, l, u = z["Px"], z["q"], z["Ax"].copy(), z["l"], z["u"]
    keep = z["keep"]
    bad = np.zeros(B, bool)
    if keep is not None and B > 1:     # one item violates the mask: the whole-pattern fallback plan solves it
        Ax[1, np.nonzero(~keep)[0][0]] = 0.05
        bad = np.any((Ax != 0) & ~keep[None, :], axis=1)
        assert bad.tolist() == [False, True] + [False] * (B - 2)
    plan = sfb.SparseQPPlan(z["n"], z["m"], Pp, Pi, Ap, Aj, ordering=z["ordering"], user_perm=z["user_perm"], stage=z["stage"], keep=keep)
    assert plan.nnzL == Z.EXPECT[name][1]                       # the plan the host test checked
    if keep is not None:
        assert plan.nnzL_fallback == Z.EXPECT[name + ".fallback"][1]
    prm = sfb.QPSolverParams(max_iter=120)
    assert prm.polish
    prob = QC.Problem.sparse(Pp, Pi, Px, q, Ap, Aj, Ax, l, u)
    wx = wy = None
    codes = []
    for _ in ("cold", "warm from the first"):
        r = plan.solve_batch_host(Px, q, Ax, l, u, prm, warm_x=wx, warm_y=wy)
        for sel, fo in ((~bad, plan.factor_order()), (bad, plan.factor_order(fallback=True) if bad.any() else None)):
            if not sel.any():
                continue
            ref = oracle.qp_sparse_solve_batch(Pp, Pi, Px[sel], q[sel], Ap, Aj, Ax[sel], l[sel], u[sel], perm=plan.perm, forder=fo,
                                               params=_oracle_params(oracle, prm), warm_x=None if wx is None else wx[sel],
                                               warm_y=None if wy is None else wy[sel], nthreads=8)

            class Sel:
                code, iter, primal, dual, objective = r.code[sel], r.iter[sel], r.primal[sel], r.dual[sel], r.objective[sel]
            assert _compare(Sel, ref), "primal / dual differ from the oracle in some bit"
            assert np.array_equal(Sel.objective, ref["obj"], equal_nan=True)
        rep = QC.certify(prob, r, prm)
        assert rep.passed, str(rep)
        codes.append(r.code.copy())
        wx, wy = np.nan_to_num(r.primal), np.nan_to_num(r.dual)
    plan.close()
    return codes


@pytest.mark.parametrize("name,B,engine", CASES)
def test_zoo_entry_matches_the_oracle_bit_for_bit(sfb, oracle, knobs, name, B, engine):
    if engine == "units0":
        knobs.set(SFB_PLAN_UNITS=0)
    codes = _solve_and_check(sfb, oracle, name, B)
    print(name, B, engine, "codes", [c.tolist() for c in codes])


@pytest.mark.parametrize("name", Z.BOUNDARY)
def test_boundary_pairs_under_every_form_of_the_sweeps(sfb, oracle, name, sweep_mode):  # noqa: F811
    _solve_and_check(sfb, oracle, name, 3)


@pytest.mark.parametrize("name", Z.BOUNDARY)
def test_boundary_pairs_with_the_lat_form_forced(sfb, oracle, knobs, name):
    knobs.set(SFB_SP_FORCE_LAT=1)
    _solve_and_check(sfb, oracle, name, 3)
