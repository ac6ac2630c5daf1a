"""The register tail of the LAT form's forward sweep (csrc/qp_sparse.hip kLatTail / lat_tail_load / ldl_solve_lat): the last columns
of the forward schedule -- the plan's column tail, csrc/sparse_plan.h -- are solved in registers instead of one LDS round trip per
column.  Every case runs in the LAT form (SFB_SP_FORCE_LAT=1: the register tail) and in the standard form (SFB_SP_LAT=0: the same
tail units as ordinary units of the sweep); the two must agree bit for bit, and with the sparse CPU oracle in codes, iterations,
x, y and objective.  The plans' tails (ftail0 / ftail, which columns lack entries) are pinned on the CPU by
tests/test_sparse_plan_tail_host.py.  Needs an MI355X."""
import numpy as np
import pytest

import sparse_tail_patterns as TP
from test_qp_dense_gpu import _compare, _oracle_params

pytestmark = pytest.mark.gpu

FORMS = (("lat", {"SFB_SP_FORCE_LAT": 1}), ("standard", {"SFB_SP_LAT": 0}))


def _same_bits(a, b):
    return (np.array_equal(a.code, b.code) and np.array_equal(a.iter, b.iter) and np.array_equal(a.primal, b.primal, equal_nan=True)
            and np.array_equal(a.dual, b.dual, equal_nan=True) and np.array_equal(a.objective, b.objective, equal_nan=True))


def _run(sfb, oracle, knobs, z, prm, forms=FORMS, edit=None):
    """solve z's batch in every form; -> (result of the first form, oracle's result)"""
    plan = sfb.SparseQPPlan(z["n"], z["m"], z["Pp"], z["Pi"], z["Ap"], z["Aj"], ordering=z["ordering"], user_perm=z["user_perm"],
                            stage=z["stage"], keep=z["keep"])
    Px, q, Ax, l, u = z["Px"], z["q"].copy(), z["Ax"], z["l"], z["u"]
    if edit is not None:
        edit(plan, q)
    res = []
    for name, kn in forms:
        knobs.set(**kn)
        res.append(plan.solve_batch_host(Px, q, Ax, l, u, prm))
        knobs.clear(*kn)
    ref = oracle.qp_sparse_solve_batch(z["Pp"], z["Pi"], Px, q, z["Ap"], z["Aj"], Ax, l, u, perm=plan.perm, forder=plan.factor_order(),
                                       params=_oracle_params(oracle, prm), nthreads=8)
    plan.close()
    for (name, _), r in zip(forms, res):
        assert _same_bits(r, res[0]), "the %s form differs from the %s form in some bit" % (name, forms[0][0])
    _compare(res[0], ref)  # codes, iterations; x, y and objective of the finite items within the dense tests' tolerance ... and
    for got, want in ((res[0].primal, ref["x"]), (res[0].dual, ref["y"]), (res[0].objective, ref["obj"])):  # ... every item bit for bit
        assert np.array_equal(got, want, equal_nan=True), "differs from the oracle in some bit"
    return res[0], ref


# no tail (tiny2, blockdiag400) | a tail of single entries (chain399) | the smallest tail, 8 (mpc6_10_pruned) | the longest, 48, dense
# (clique53) | a dense row's trailing block (arrow800) | 48 with trailing entries missing (twoclique60)
@pytest.mark.parametrize("name,B", [("tiny2", 8), ("blockdiag400", 8), ("chain399", 8), ("mpc6_10_pruned", 12), ("clique53", 16),
                                    ("arrow800", 8), ("twoclique60", 16)])
def test_register_tail_matches_the_standard_form_and_the_oracle(sfb, oracle, knobs, name, B):
    r, _ = _run(sfb, oracle, knobs, TP.batch(name, B), sfb.QPSolverParams(max_iter=120))
    print(name, "codes", r.code.tolist(), "iterations", r.iter.tolist())
    assert r.iter.max() >= 25


@pytest.mark.parametrize("name", ["clique53", "twoclique60"])
def test_a_non_finite_pivot_reaches_the_tail(sfb, oracle, knobs, name):
    """one NaN in q, in an unknown the elimination order puts among the tail's rows (items 0 and 3 only): a lane without an entry in
    a step keeps its value whatever the pivot is, as a padding slot does"""
    def edit(plan, q):
        k = len(plan.perm)
        v = int(plan.perm[k - 3])
        assert v < q.shape[1]  # (an unknown of x: the cliques' rows of A are eliminated first)
        q[0, v] = q[3, v] = np.nan
    r, ref = _run(sfb, oracle, knobs, TP.batch(name, 8), sfb.QPSolverParams(max_iter=120), edit=edit)
    print(name, "codes", r.code.tolist(), "iterations", r.iter.tolist())
    assert not np.isfinite(ref["x"][0]).all() or r.code[0] != 0


@pytest.mark.parametrize("name", ["clique53", "mpc6_10_pruned"])
def test_the_tail_survives_stopping_checks(sfb, oracle, knobs, name):
    """stop_check_iter = 2: the iterate leaves for the workspace and comes back at every other iteration (vectors_home /
    iterate_in); the tail's AccVGPRs and the lane's entry mask are loaded once per item and must still be there"""
    r, _ = _run(sfb, oracle, knobs, TP.batch(name, 8), sfb.QPSolverParams(max_iter=120, stop_check_iter=2))
    print(name, "codes", r.code.tolist(), "iterations", r.iter.tolist())
    assert r.iter.min() >= 4  # at least two checks passed


def test_headline_model_through_the_predicted_order_launch_with_polishers(sfb, oracle, knobs):
    """variant 12, K = 50 (forward schedule: 120 body units + 48 tail units, the trailing block not dense), batch 16 on a tiny grid:
    the LAT loop launch with its resident head, the register tail and the polishers, against the standard-form loop launch"""
    knobs.set(SFB_SP_GRID=12)
    r, _ = _run(sfb, oracle, knobs, TP.headline(16, seed=43), sfb.QPSolverParams(), forms=(("default", {}), ("standard_loop", {"SFB_SP_LAT": 0})))
    assert r.iter.max() > 100 and (r.code == 0).all()
