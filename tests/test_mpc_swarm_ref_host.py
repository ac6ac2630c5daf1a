"""CPU checks of the swarm's bookkeeping model (tests/mpc_swarm_ref.py) and of the scenario (tests/mpc_swarm_scenario.py) that
tests/test_mpc_swarm_state_gpu.py stands on: driven with the CPU oracle as the solver (on the QPs of the reference assembly,
with the plan's elimination and summation orders), the scenario refuses exactly where its script says, reaches MaxIterations
among the solves it keeps, and can tell: the starting point of every solve behind a refusal or a cold tick matters, and every
deliberate mistake of the model's switchboard changes something a step returns.  Prints, per case, the verdict histogram and
the step and observable that expose each mistake.  No GPU.

Where the scenario cannot tell, and why (asserted below, so that the list stays true):

  * du0_stale_when_refused: a refused pass leaves the plan alone, and du0 was read from that plan by the step before; the
    refusing branch of mpc_accept_kernel rewrites du0 with the bits it already holds.  No sequence of the swarm's entries
    can show the difference.
  * polish_failed_kept: the oracle ends no solve of the scenario with PolishFailed, with polish on or off (seeds 0..3 of
    every case tried); the switch is checked on the model alone with a made-up solve.
  * a pre-check refusal returns the solver's starting point (scaled and scaled back).  For role 4, refused at every step, that
    is zero like everything it holds; for the roles refused at a pass behind an accepted solve it equals the plan up to last
    bits, and in some agents exactly.  So "the refused first input differs from the held one" is asserted per role (one agent
    of each at least) on the injected script, and for every agent and step on the script with the solver's own refusals
    (case `natural`), where the two are far apart."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_assembly_ref as AR  # noqa: E402
import mpc_swarm_ref as SR  # noqa: E402
import mpc_swarm_scenario as S  # noqa: E402
from test_qp_dense_gpu import _oracle_params  # noqa: E402

NEEDS_A_REFUSAL = ("accept_all", "du0_from_new_when_refused", "warm_from_refused_pass")


def applies(mistake, cs):
    """can the mistake show on this case at all?"""
    if mistake in ("du0_stale_when_refused", "polish_failed_kept"):
        return False                                                   # (see the docstring)
    if mistake == "px_first_entry_for_all":
        return not cs.emptyP
    if mistake in NEEDS_A_REFUSAL:
        return any(st["refused"].any() for st in cs.steps if st["kind"] == "pass")
    if mistake == "warm_from_refused_tick":                            # (role 1's refused tick returns zeros onto a zero warm start)
        return cs.script == "natural" or cs.B > 5
    return True


def make_solver(sfb, oracle, cs):
    plan = sfb.SparseQPPlan(cs.n, cs.m, cs.Pp, cs.Pi, cs.Ap, cs.Aj)
    params_of = lambda k: _oracle_params(oracle, sfb.QPSolverParams(max_iter=k, polish=cs.polish))      # noqa: E731
    solver = S.OracleSolver(oracle, params_of, plan.perm, plan.factor_order())
    plan.close()
    return solver


def _differ(a, b, rows):
    """per row: another iteration count or other bits of x"""
    return (a.iter[rows] != b.iter[rows]) | ~AR.same_bits(a.x[rows], b.x[rows]).all(axis=1)


def check_scenario(cs, solver, say=print):
    truth = S.drive(cs, solver)
    solves = [(at, e) for at, e in enumerate(truth) if e["kind"] != "reset"]
    roles = np.array([S.role(b) if cs.script == "main" else 0 for b in range(cs.B)])
    u = slice(cs.uoff, cs.uoff + cs.nu)

    # every role behaved as scripted; MaxIterations among the kept solves
    hist, kept4 = np.zeros(7, dtype=int), 0
    for at, e in solves:
        refused = ~np.isin(e["sol"].code, SR.KEPT)
        assert np.array_equal(refused, cs.steps[at]["refused"]), (cs.id, e["no"], e["sol"].code.tolist())
        hist += np.bincount(e["sol"].code, minlength=7)
        kept4 += int((e["sol"].code == SR.MAX_ITERATIONS).sum())
    say("%s: verdicts [Optimal PolishFailed PrimalInf DualInf MaxIter MaxTime Unknown] = %s" % (cs.id, hist.tolist()))
    assert kept4 >= 1

    # the refused solve's first input differs from the held plan's
    seen, total, differing = {}, 0, 0
    for k, (at, e) in enumerate(solves):
        if e["kind"] != "pass":
            continue
        held = solves[k - 1][1]["ret"][3]
        for b in np.flatnonzero(cs.steps[at]["refused"]):
            d = not AR.all_same_bits(e["sol"].x[b, u], held[b, u])
            total, differing = total + 1, differing + int(d)
            seen[roles[b]] = seen.get(roles[b], False) or d
            if cs.script == "main" and roles[b] == 4:
                assert not e["sol"].x[b].any() and not held[b].any()           # zero against zero
            if cs.script == "natural":
                assert d and np.max(np.abs(e["sol"].x[b, u] - held[b, u])) > 1e-3 * np.max(np.abs(held[b, u]))
    say("%s: refused first input differs from the held one in %d of %d refused agent-passes" % (cs.id, differing, total))
    for r, d in seen.items():
        assert d or (cs.script == "main" and r == 4), (cs.id, "role", r)

    # behind a refusal or the cold tick: the right start, a cold start and the refused (unstored) solve give different solves
    told = {}
    for k, (at, e) in enumerate(solves[1:], 1):
        p, st = solves[k - 1][1], cs.steps[at]
        pst = cs.steps[solves[k - 1][0]]
        rows = np.arange(cs.B) if (pst["kind"] == "tick" and not pst["warm"]) else np.flatnonzero(pst["refused"])
        if not len(rows):
            continue
        mdl = cs.model()
        cold = solver(cs, st, rows, mdl.Px, mdl.q, None)
        wrong = solver(cs, st, rows, mdl.Px, mdl.q, (p["sol"].x, p["sol"].y))
        right = SR.Solve(e["sol"].x[rows], e["sol"].y[rows], e["sol"].code[rows], e["sol"].iter[rows])
        both = _differ(right, cold, slice(None)) & _differ(right, wrong, slice(None))
        (sx, sy), (rx, ry) = S.start_of(cs, e["warm"]), (p["sol"].x, p["sol"].y)
        for j, b in enumerate(rows):
            told.setdefault(roles[b], []).append(bool(both[j]))
            if cs.script == "main" and roles[b] == 4:                            # three times the same start: all zero
                assert not sx[b].any() and not sy[b].any() and not rx[b].any() and not ry[b].any()
    for r, hits in sorted(told.items()):
        say("%s: role %d (%s): the start matters in %d of %d solves behind a refusal / the cold tick" % (
            cs.id, r, S.ROLE_TEXT[r] if cs.script == "main" else "refused by the solver", sum(hits), len(hits)))
        assert any(hits) or (cs.script == "main" and r == 4), (cs.id, "role", r)
    assert set(told) == set(roles.tolist())

    # every mistake shows where it can, and does not where it cannot
    for mistake in SR.MISTAKES:
        d = S.first_difference(S.drive(cs, solver, (mistake,), truth), truth)
        say("%s: %-26s %s" % (cs.id, mistake, "step %d, %s" % d if d else "not visible"))
        if applies(mistake, cs):
            assert d is not None, (cs.id, mistake)
        else:
            assert d is None, (cs.id, mistake, d)
    return truth


@pytest.mark.parametrize("cid", list(S.CASES))
def test_scenario_can_tell(sfb, oracle, cid):
    cs = S.case(cid)
    check_scenario(cs, make_solver(sfb, oracle, cs))


def test_polish_failed_is_neither_stored_nor_accepted():
    """the switch the scenario cannot reach: a made-up PolishFailed solve on the model alone"""
    rng = np.random.default_rng(5)
    mk = lambda code: SR.Solve(rng.normal(size=(2, 4)), rng.normal(size=(2, 3)), [0, code], [7, 9])       # noqa: E731
    for mistakes, kept in (((), False), (("polish_failed_kept",), True)):
        s = SR.Swarm(2, 4, 3, 2, 2, mistakes=mistakes)
        a, b = mk(0), mk(SR.POLISH_FAILED)
        s.tick(a)
        s.relin_pass(b)
        du0, code, it, x, y = s.returned()
        assert np.array_equal(x[0], b.x[0]) and np.array_equal(s.wx[0], b.x[0])
        want = b if kept else a
        assert np.array_equal(x[1], want.x[1]) and np.array_equal(s.wy[1], want.y[1]) and (code[1], it[1]) == (want.code[1], want.iter[1])
        assert np.array_equal(du0, x[:, 2:4])
        s.tick(mk(SR.POLISH_FAILED))
        assert np.array_equal(s.wx[1], s.x[1]) == kept                           # a tick stores it only by mistake


def test_model_refuses_to_be_read_before_the_first_tick():
    s = SR.Swarm(3, 5, 4, 3, 2)
    sol = SR.Solve(np.ones((3, 5)), np.ones((3, 4)), [0, 0, 0], [1, 1, 1])
    with pytest.raises(SR.Undefined):
        s.relin_pass(sol)
    with pytest.raises(SR.Undefined):
        s.warm(is_pass=True)
    with pytest.raises(SR.Undefined):
        s.returned()
    assert s.warm(warmstart=False) is None
    wx, wy = s.warm()
    assert not wx.any() and not wy.any() and wx.shape == (3, 5) and wy.shape == (3, 4)
    s.tick(sol)
    s.relin_pass(sol)
    s.reset_warmstart()
    assert not s.wx.any() and not s.wy.any() and s.returned()[3].all()
