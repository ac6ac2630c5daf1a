"""The per-agent bookkeeping of the device-resident MPC swarm (mpc_replicate_kernel, mpc_store_kernel, mpc_accept_kernel of
csrc/mpc_assemble.hip behind sfb_mpc_swarm_create / _step_host / _step_resident_flat / _reset_warmstart) against the numpy
state machine tests/mpc_swarm_ref.py, on the scenario of tests/mpc_swarm_scenario.py (which tests/test_mpc_swarm_ref_host.py
shows able to tell every slip of the model's switchboard): injected and solver-made refusals at ticks and passes, a cold tick
in front of a pass, reset_warmstart, a non-zero q, a P with distinct entries and an empty one, n, m and nu on both sides of
the kernels' 64-lane trips, B = 1, 4, 5 and 12.

After every step of a swarm (full=True):
  * solve parity: where the swarm took the solve (every agent at a tick, the accepted ones at a pass) what it returns equals
    the CPU oracle's solve of the reference assembly's QP FROM THE MODEL'S WARM START, by the bar of tests/test_qp_dense_gpu.py
    (_compare: codes and iteration counts exact, primal and dual within TOL; non-finite entries in the same places);
  * bookkeeping, bit for bit: an agent the model refuses at a pass returns the x, y, code, iter it returned the step before;
    du0 equals the returned x[:, uoff:uoff + nu] everywhere; and the model, advanced with the device's own values where a
    solve was taken (no rounding accumulates over the steps), returns the same bits as the swarm.
Then the same bits with the time-sliced launch (SFB_SP_GRID=4), and with two swarms alive and stepped alternately.

Hand check (once, on a scratch build, not committed): with the condition of mpc_accept_kernel inverted, and with `store &&`
dropped from mpc_store_kernel, this file fails.  Needs an MI355X."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_assembly_ref as AR  # noqa: E402
import mpc_layout_zoo as Z  # noqa: E402
import mpc_swarm_ref as SR  # noqa: E402
import mpc_swarm_scenario as S  # noqa: E402
from stream_contract import hip_runtime  # noqa: E402
from test_qp_dense_gpu import _compare, _oracle_params  # noqa: E402

pytestmark = pytest.mark.gpu


def _h2d(ptr, a):
    import torch
    torch.cuda.init()
    lib = hip_runtime()
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.ascontiguousarray(a, dtype=np.float64)
    rc = lib.hipMemcpy(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, 1)
    assert rc == 0, "hipMemcpy H2D: %d" % rc


def _bits(a, b):
    return AR.all_same_bits(a, b) if a.dtype == np.float64 else bool(np.array_equal(a, b))


def _bar(got, ref, rows, what):
    """the project's bar on the given agents (the swarm returns no objective: that clause of _compare gets equal zeros)"""
    du0, code, it, x, y = got
    if not len(rows):
        return
    r = types.SimpleNamespace(code=code[rows], iter=it[rows], primal=x[rows], dual=y[rows], objective=np.zeros(len(rows)))
    want = dict(code=ref.code[rows], iter=ref.iter[rows], x=ref.x[rows], y=ref.y[rows], obj=np.zeros(len(rows)))
    try:
        _compare(r, want)
    except AssertionError as e:
        raise AssertionError("%s: %s | codes %s / %s iters %s / %s" % (what, e, r.code.tolist(), want["code"].tolist(),
                                                                        r.iter.tolist(), want["iter"].tolist())) from e
    assert np.array_equal(np.isfinite(r.primal), np.isfinite(want["x"])) and np.array_equal(np.isfinite(r.dual), np.isfinite(want["y"])), what


class Run:
    """one swarm on one case, stepped through the script against the model; .returned[k] is what step k gave"""

    def __init__(self, sfb, oracle, cid):
        cs = self.cs = S.case(cid)
        self.sfb = sfb
        self.plan = sfb.SparseQPPlan(cs.n, cs.m, cs.Pp, cs.Pi, cs.Ap, cs.Aj)
        assert self.plan.nnzP == (0 if cs.emptyP else cs.n)
        self.Ls = Z.to_sfb(sfb, cs.name)
        assert (self.Ls.n, self.Ls.m, self.Ls.nu, self.Ls.nx * (self.Ls.N + 1)) == (cs.n, cs.m, cs.nu, cs.uoff)
        params_of = lambda k: _oracle_params(oracle, sfb.QPSolverParams(max_iter=k, polish=cs.polish))      # noqa: E731
        self.solver = S.OracleSolver(oracle, params_of, self.plan.perm, self.plan.factor_order())
        self.swarm = sfb.MPCSwarm(self.plan, self.Ls, cs.Px, cs.q, cs.B)
        self.model = cs.model()
        self.returned, self.at = [], 0
        self.verdicts = np.zeros(7, dtype=int)

    def close(self):
        self.swarm.close()
        self.plan.close()

    @property
    def done(self):
        return self.at == len(self.cs.steps)

    def step(self):
        cs, mdl, sw, st = self.cs, self.model, self.swarm, self.cs.steps[self.at]
        self.at += 1
        if st["kind"] == "reset":
            sw.reset_warmstart()
            mdl.reset_warmstart()
            self.returned.append(None)
            return
        what = "%s step %d (%s)" % (cs.id, st["no"], st["kind"])
        is_pass = st["kind"] == "pass"
        prm = self.sfb.QPSolverParams(max_iter=st["max_iter"], polish=cs.polish)
        rows = np.arange(cs.B)
        ref = self.solver(cs, st, rows, mdl.Px, mdl.q, mdl.warm(warmstart=bool(st["warm"]), is_pass=is_pass))
        refused = ~np.isin(ref.code, SR.KEPT)
        assert np.array_equal(refused, st["refused"]), (what, ref.code.tolist())           # the script, as on the CPU
        self.verdicts += np.bincount(ref.code, minlength=7)
        if is_pass:
            ptr, rd = sw.device_records()
            assert rd == st["recs"].shape[1] == AR.record_doubles(cs.L)
            _h2d(ptr, st["recs"])
            got = sw.step_resident_flat(prm, full=True)
        else:
            got = sw.step_host(st["recs"], prm, warmstart=bool(st["warm"]), full=True)
        du0, code, it, x, y = got
        taken = rows[~refused] if is_pass else rows
        _bar(got, ref, taken, what)
        if is_pass:                                                   # a refused agent returns what it returned before
            prev = next(r for r in reversed(self.returned) if r is not None)
            for nm, a, b in zip(S.OBSERVABLES[1:], got[1:], prev[1:]):
                assert _bits(a[refused], b[refused]), "%s: %s of a refused agent moved" % (what, nm)
        assert _bits(du0, x[:, cs.uoff:cs.uoff + cs.nu]), "%s: du0 is not the first input of the returned plan" % what
        # the model goes on with the device's values where the solve was taken (a refused pass-solve is dropped anyway)
        sol = SR.Solve(ref.x, ref.y, ref.code, ref.iter)
        sol.x[taken], sol.y[taken], sol.code[taken], sol.iter[taken] = x[taken], y[taken], code[taken], it[taken]
        if is_pass:
            mdl.relin_pass(sol)
        else:
            mdl.tick(sol, warmstart=bool(st["warm"]))
        for nm, a, b in zip(S.OBSERVABLES, got, mdl.returned()):
            assert _bits(a, b), "%s: %s differs from the model's" % (what, nm)
        self.returned.append(got)

    def all(self):
        while not self.done:
            self.step()
        return self.returned


_ALONE = {}


def _alone(sfb, oracle, cid):
    """what the case returns, run alone with no knob set (once per session)"""
    if cid not in _ALONE:
        r = Run(sfb, oracle, cid)
        try:
            _ALONE[cid] = r.all()
        finally:
            r.close()
        print("%s: verdicts [Optimal PolishFailed PrimalInf DualInf MaxIter MaxTime Unknown] = %s" % (cid, r.verdicts.tolist()))
    return _ALONE[cid]


def _same_run(a, b, what):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert (u is None) == (v is None)
        if u is not None:
            for nm, p, q in zip(S.OBSERVABLES, u, v):
                assert _bits(p, q), "%s: %s differs at step %d" % (what, nm, k + 1)


@pytest.mark.parametrize("cid", list(S.CASES))
def test_swarm_keeps_its_books_like_the_model(sfb, oracle, cid):
    ret = _alone(sfb, oracle, cid)
    cs = S.case(cid)
    assert sum(r is not None for r in ret) == sum(st["kind"] != "reset" for st in cs.steps)
    if cs.script == "main":                       # reset_warmstart: steps 9 and 10 start from zero like steps 1 and 2 did
        never = np.array([S.role(b) == 0 for b in range(cs.B)])
        for nm, a, b in zip(S.OBSERVABLES, ret[8], ret[0]):
            assert _bits(a[never], b[never]), nm


def test_time_sliced_launch_gives_the_same_bits(sfb, oracle, knobs):
    """SFB_SP_GRID=4: the twelve agents share four workgroups (time-sliced, launched in the predicted order); a pass there
    solves into xn / yn like any other"""
    want = _alone(sfb, oracle, "km8")
    knobs.set(SFB_SP_GRID=4)
    r = Run(sfb, oracle, "km8")
    try:
        got = r.all()
    finally:
        r.close()
    _same_run(got, want, "km8 with SFB_SP_GRID=4")


def test_two_swarms_alive_do_not_share_state(sfb, oracle):
    want = {cid: _alone(sfb, oracle, cid) for cid in ("so3", "commutative")}
    runs = {cid: Run(sfb, oracle, cid) for cid in want}
    try:
        while not all(r.done for r in runs.values()):
            for r in runs.values():
                if not r.done:
                    r.step()
        for cid, r in runs.items():
            _same_run(r.returned, want[cid], "%s next to another swarm" % cid)
    finally:
        for r in runs.values():
            r.close()
