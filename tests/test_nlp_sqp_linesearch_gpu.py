"""Law 3 of the swarm SQP solver on the GPU ("Swarm SQP": penalty, merit, Armijo search, commit, relaxation of mu,
iteration count) against its own functions in tests/nlp_sqp_ref.py: step_start_ref, trial_ref, accept_ref.  The solver is
model-free, so the evaluations are scripted: f, df, g, dg, hess, f_trial and g_trial are what a test hands in and come from no
model.  A trial point is refused or taken by construction -- f_trial is built from the device's own phi0 and slope (which the
first test pins) a factor 2 to either side of the Armijo line, or on the taking side with one row violated by 1.0 where nu times
that is at least 10 times the Armijo term -- so the reference and the kernel decide alike without any tolerance, and after every
call every field of the state is compared bit for bit, `_bits`, with accept_ref applied to the state before it.  The factors 2 and
10 are conditions on the inputs, asserted, not measurements.  Batches 1, 3 and 67; every case runs in a few seconds."""
import ctypes as C

import numpy as np
import pytest

import nlp_sqp_ref as R
import test_nlp_sqp_gpu as G0

pytestmark = pytest.mark.gpu
BATCHES = (1, 3, 67)
LD = np.longdouble
QP_ITER = 4000
STATE = ("x", "lam", "z", "status", "iter", "r_stat", "r_pri", "r_comp", "mu", "alpha", "nu")
INPUTS = ("f", "df", "g", "dg", "hess")
QP_ARRAYS = ("Px", "q", "Ax", "l", "u")
REJECTIONS = (0, 1, 2, 5, 10, 11)
# seeds per batch of the cases that need their agents to come through several QPs (a random QP here is infeasible now and then)
SEEDS_C, SEEDS_E = {1: 506, 3: 515, 67: 500}, {1: 800, 3: 803, 67: 800}


def T(a):
    return G0.T(a)


def H(t):
    return G0.H(t)


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# --------------------------------------------------------------------------------------------------------------------- fronts
class _Dev:
    """the device-pointer entries (NLPSwarmSQP on torch tensors) on numpy arrays"""

    def __init__(self, sfb, s):
        self.s = s

    def set_start(self, x, lam, z):
        self.s.set_start(T(x), T(lam), T(z))

    def direction(self, d):
        return self.s.direction(*[T(d[k]) for k in INPUTS])

    def trial(self):
        return H(self.s.trial())

    def accept(self, ft, gt):
        return self.s.accept(T(ft), T(gt))

    def state(self):
        return {k: H(v).copy() for k, v in self.s.state_views().items()}


class _Host:
    """the host-pointer entries sfb_nlp_sqp_{set_start,direction,trial,accept,state}_host on the same handle"""

    def __init__(self, sfb, s):
        self.s, self.lib, self.check = s, sfb._capi.lib, sfb._capi.check

    @staticmethod
    def _p(a):
        return a.ctypes.data if a.size else None

    def set_start(self, x, lam, z):
        a = [np.ascontiguousarray(v, np.float64) for v in (x, lam, z)]
        self.check(self.lib.sfb_nlp_sqp_set_start_host(self.s._h, *[self._p(v) for v in a]))

    def direction(self, d):
        a, n = [np.ascontiguousarray(d[k], np.float64) for k in INPUTS], C.c_int64(-1)
        self.check(self.lib.sfb_nlp_sqp_direction_host(self.s._h, *[self._p(v) for v in a], C.byref(n)))
        return n.value

    def trial(self):
        out = np.full((self.s.batch, self.s.n), np.nan)
        self.check(self.lib.sfb_nlp_sqp_trial_host(self.s._h, self._p(out)))
        return out

    def accept(self, ft, gt):
        a, n = [np.ascontiguousarray(v, np.float64) for v in (ft, gt)], C.c_int64(-1)
        self.check(self.lib.sfb_nlp_sqp_accept_host(self.s._h, *[self._p(v) for v in a], C.byref(n)))
        return n.value

    def state(self):
        B, n, m = self.s.batch, self.s.n, self.s.m
        shapes = dict(x=(B, n), lam=(B, m), z=(B, n))
        out = {k: np.zeros(shapes.get(k, (B,)), np.int32 if k in ("status", "iter") else np.float64) for k in STATE}
        self.check(self.lib.sfb_nlp_sqp_state_host(self.s._h, *[self._p(out[k]) for k in STATE]))
        return out


def _debug(s):
    return {k: H(v).copy() for k, v in s.debug_views().items()}


# --------------------------------------------------------------------------------------------------------------------- inputs
def _inputs(pb, B, seed, frozen=()):
    """test_nlp_sqp_gpu's random inputs with a diagonally dominant Hessian, x clipped into the box (so the bound rows hold at
    d = 0, many of them active: x sits on a bound wherever the draw fell outside) and the agents of `frozen` at a KKT point"""
    d = G0._random_inputs(pb, B, seed, definite=True, optimal=frozen)
    d["x"] = np.fmin(np.fmax(d["x"], pb.xl), pb.xu)
    d["g"] = np.fmin(np.fmax(d["g"], pb.gl - 0.2), pb.gu + 0.2)                     # no row violated by more than 0.2: few QPs are infeasible
    return d


def _ladder_case(B, seed=11):
    """the ladder problem with non-zero random lambda and z, x inside the box and g inside its rows.  At B = 67 also: agent 0 concave
    (H = -I: climbs to mu = 3.2768), agent 1 with the single diagonal -5e-5 and a gradient along it (d = -+e_1 to the box at mu = 0,
    so d.P d < 0; convex at mu = mu_first), one agent with inconsistent rows, three at a KKT point.  -> pb, inputs, the rejections per
    agent, the special agents."""
    pb = G0._ladder_problem()
    sp = dict(concave=0, first=1, infeasible=30, optimal=(5, 20, 41)) if B == 67 else dict(concave=None, first=None, infeasible=None, optimal=())
    kinds = ["convex"] * B
    if B == 67:
        kinds[sp["concave"]], kinds[sp["infeasible"]] = "concave", "infeasible"
    d = G0._ladder_inputs(B, kinds, seed=seed)
    rng = np.random.default_rng(seed + 1)
    d["x"], d["g"] = rng.uniform(-0.5, 0.5, (B, 3)), rng.uniform(0.05, 0.95, (B, 2))
    d["lam"], d["z"], d["f"] = rng.normal(size=(B, 2)), rng.normal(size=(B, 3)), rng.normal(size=B)
    if B == 67:
        d["x"][sp["concave"]], d["g"][sp["concave"]], d["g"][sp["infeasible"]] = 0.0, 0.5, (-5.0, 5.0)
        d["x"][sp["first"]], d["g"][sp["first"]], d["df"][sp["first"]], d["hess"][sp["first"]] = 0.0, 0.5, (0.0, 0.5, 0.0), (2.0, -5e-5, 2.0)
        for b in sp["optimal"]:
            d["x"][b], d["g"][b], d["df"][b], d["lam"][b], d["z"][b] = 0.0, 0.5, 0.0, 0.0, 0.0
    rej = _rejections(B)
    if B == 67:
        rej[sp["concave"]], rej[sp["first"]] = 1, 0
    return pb, d, rej, sp


def _rejections(B):
    """how many trial points each agent is refused: 1 at B = 1, {0, 2, 11} at B = 3, every value of REJECTIONS interleaved by a
    stride (as test_nlp_sqp_gpu._kinds places its agents) beyond"""
    if B == 1:
        return [1]
    if B == 3:
        return [0, 2, 11]
    rej = [0] * B
    for k in range(B):
        rej[(k * 29 + B // 2) % B] = REJECTIONS[k % len(REJECTIONS)]
    return rej


def _finite_row(pb):
    """(row, +1) for the first row with a finite upper side, else (row, -1) for the first with a finite lower side, else None"""
    for side, bound in ((1, pb.gu), (-1, pb.gl)):
        rows = np.nonzero(np.isfinite(bound))[0]
        if len(rows):
            return int(rows[0]), side
    return None


# --------------------------------------------------------------------------------------------------------------------- the engine
def _ref_states(pb, st, dbg, slot):
    """per agent the state accept_ref takes: the device's own state after a direction call, (d, y) from the slot of the QP arrays
    that holds the agent's accepted solve, phi0 and D from the judge's sums.  After direction an agent searches iff it is running."""
    out = []
    for b in range(len(st["status"])):
        k = slot.get(b, 0)
        out.append(dict(x=st["x"][b].copy(), lam=st["lam"][b].copy(), z=st["z"][b].copy(), mu=float(st["mu"][b]), nu=float(st["nu"][b]),
                        alpha=float(st["alpha"][b]), iter=int(st["iter"][b]), status=int(st["status"][b]), d=dbg["d"][k].copy(),
                        y=dbg["y"][k].copy(), phi0=float(dbg["sums"][1][b]), D=float(dbg["sums"][2][b]), halvings=0,
                        searching=bool(st["status"][b] == R.RUNNING)))
    return out


def _check_state(st, ref, before, tag):
    for b, r in enumerate(ref):
        for key in ("x", "lam", "z", "mu", "nu", "alpha"):
            assert _bits(st[key][b], r[key]), (tag, b, key, st[key][b], r[key])
        assert st["iter"][b] == r["iter"] and st["status"][b] == r["status"], (tag, b, st["iter"][b], st["status"][b], r["iter"], r["status"])
        for key in ("r_stat", "r_pri", "r_comp"):                                   # the search never touches the residuals
            assert _bits(st[key][b], before[key][b]), (tag, b, key)


def _search(front, pb, ref, cur, rej, how=None, stats=None, log=None, max_rounds=12, tag=""):
    """the scripted search.  ref: _ref_states; cur: the state the front shows now; rej[b]: how many trial points agent b is refused
    before one is taken; how[b]: None (refused by the Armijo line or, for a share, by a violation), "fnan", "finf" or ("gnan", row):
    refused through a value that is not finite.  Checks every trial point and, after every accept, the whole state and the count.
    -> (ref, cur) after the search, or after max_rounds rounds."""
    B = len(ref)
    how = how or [None] * B
    stats = stats if stats is not None else {}
    feasible, row = G0._feasible(pb.gl, pb.gu), _finite_row(pb)
    for rounds in range(max_rounds):
        if not any(r["searching"] for r in ref):
            break
        xt = front.trial()
        # who is not searching is offered a point no Armijo test would refuse: it must be ignored
        ft, gt = np.full(B, -1e300), np.tile(feasible, (B, 1))
        for b, r in enumerate(ref):
            if not r["searching"]:
                assert _bits(xt[b], r["x"]), (tag, rounds, b, "trial of an agent that does not search")
                continue
            assert r["alpha"] == 2.0 ** -r["halvings"]
            assert _bits(xt[b], R.trial_ref(pb, r["x"], r["d"], r["alpha"])), (tag, rounds, b, "trial")
            assert r["D"] < 0.0, (tag, b, r["D"])                                   # a descent direction of the merit: t < 0 below
            t = 1e-4 * r["alpha"] * r["D"]
            ft[b] = r["phi0"] + 2.0 * t                                             # taken, unless something below refuses it
            if r["halvings"] >= rej[b]:
                stats["taken"] = stats.get("taken", 0) + 1
            elif how[b] == "fnan":
                ft[b] = np.nan
            elif how[b] == "finf":
                ft[b] = np.inf
            elif how[b] is not None:
                gt[b, how[b][1]] = np.nan
            elif (b + r["halvings"]) % 2 == 0 and row is not None and r["nu"] * 1.0 >= 10.0 * abs(t):
                gt[b, row[0]] = (pb.gu[row[0]] + 1.0) if row[1] > 0 else (pb.gl[row[0]] - 1.0)   # infeasible by v = 1.0: nu v >= 10 |t|
                stats["violation"] = stats.get("violation", 0) + 1
            else:
                ft[b] = r["phi0"] + 0.5 * t
                stats["armijo"] = stats.get("armijo", 0) + 1
        left = front.accept(ft, gt)
        ref = [R.accept_ref(pb, r, ft[b], gt[b]) for b, r in enumerate(ref)]
        assert left == sum(r["searching"] for r in ref), (tag, rounds, left)
        st = front.state()
        _check_state(st, ref, cur, (tag, rounds))
        if log is not None:
            log.append(("trial", xt))
            log.append(("accept", left, st))
        cur = st
    return ref, cur


def _one_rung_slots(st_before, st, dbg, count_running):
    """with mu_max = 0 a direction call has one rung: the list is the agents that ran before the call and that the stopping test
    did not end, ascending, and slot k of the QP arrays is agent list[k].  -> listed, {agent: slot}"""
    listed = [b for b in range(len(st["status"])) if st_before["status"][b] == R.RUNNING and st["status"][b] not in (R.OPTIMAL, R.MAX_ITERATIONS)]
    assert np.array_equal(dbg["list"][:len(listed)], listed)
    assert count_running == int(np.sum(st["status"] == R.RUNNING))
    return listed, {b: k for k, b in enumerate(listed)}


def _scripted_round(sfb, pb, B, seed, tag):
    """one direction call and the scripted search of _rejections on random inputs, three agents at a KKT point at B = 67"""
    frozen = (3, 17, 40) if B == 67 else ()
    d = _inputs(pb, B, seed, frozen)
    s = G0._solver(sfb, pb, B, qp_iter=QP_ITER, mu_max=0.0)                         # no shifted rung: slot k of the QP arrays is agent list[k]
    front = _Dev(sfb, s)
    front.set_start(d["x"], d["lam"], d["z"])
    start = front.state()
    n = front.direction(d)
    st, dbg = front.state(), _debug(s)
    listed, slot = _one_rung_slots(start, st, dbg, n)
    assert listed == [b for b in range(B) if b not in frozen] and np.all(st["status"][list(frozen)] == R.OPTIMAL), tag
    ref, rej, stats = _ref_states(pb, st, dbg, slot), _rejections(B), {}
    searched = [b for b in range(B) if ref[b]["searching"]]
    end, cur = _search(front, pb, ref, st, rej, stats=stats, tag=tag)
    for b in searched:
        if rej[b] == 11:                                                            # exhausted: Unknown, alpha = 2^-10, the rest as before
            assert end[b]["status"] == R.UNKNOWN and cur["alpha"][b] == 2.0 ** -10, (tag, b)
            for key in ("x", "lam", "z", "iter", "mu"):
                assert _bits(cur[key][b], st[key][b]), (tag, b, key)
        else:
            assert cur["status"][b] == R.RUNNING and cur["iter"][b] == 1 and cur["alpha"][b] == 2.0 ** -rej[b] and cur["mu"][b] == 0.0, (tag, b)
    s.close()
    return st, cur, searched, rej, stats


# --------------------------------------------------------------------------------------------------------------------- (a)
def _problems():
    zoo = dict(R.zoo())
    return [("convexqp", G0._convex_qp_nlp(1, 31)[0])] + [(k, zoo[k]) for k in ("n65", "n130", "m0", "nb0", "allbounded")]


@pytest.mark.parametrize("B", BATCHES)
def test_judge_scalars_nu_phi0_and_slope(sfb, B):
    """after one direction call: nu is max(nu_prev, 1.1 max|y[:m]|) bit for bit (one multiply, one fmax; nu_prev = 0 here, the running
    maximum is in the three-iteration test), phi0 = f + nu v1 bit for bit on the device's own v1 (-ffp-contract=off), and the slope
    is df.d - nu v1 within 4 (k + 2) eps of the absolute terms, k = n + 1: n products reduced across the wave, one product, one
    subtraction.  Agents whose largest multiplier sits on a bound row show that nu reads the m constraint rows only."""
    bound_row_larger = checked = 0
    for name, pb in _problems():
        d = _inputs(pb, B, 300)
        s = G0._solver(sfb, pb, B, qp_iter=QP_ITER, mu_max=0.0)
        front = _Dev(sfb, s)
        front.set_start(d["x"], d["lam"], d["z"])
        start = front.state()
        n = front.direction(d)
        st, dbg = front.state(), _debug(s)
        listed, slot = _one_rung_slots(start, st, dbg, n)
        assert listed == list(range(B)), name
        for b in np.nonzero(st["status"] == R.RUNNING)[0]:
            dq, yq = dbg["d"][slot[b]], dbg["y"][slot[b]]
            nu, _, _, dfd, absdfd, k = R.step_start_ref(pb, d["f"][b], d["df"][b], d["g"][b], dq, yq, 0.0)
            v1 = dbg["sums"][0][b]
            assert _bits(st["nu"][b], nu), (name, b, st["nu"][b], nu)
            assert _bits(dbg["sums"][1][b], d["f"][b] + nu * v1), (name, b, "phi0")
            want, absterms = dfd - LD(nu) * LD(v1), absdfd + LD(nu) * LD(v1)
            assert abs(LD(dbg["sums"][2][b]) - want) <= R.slack(pb.n + 1, absterms), (name, b, "slope", dbg["sums"][2][b], want)
            assert st["alpha"][b] == 1.0 and st["mu"][b] == 0.0
            checked += 1
            if pb.m and pb.nb and np.abs(yq[pb.m:]).max() > np.abs(yq[:pb.m]).max():
                assert nu == 1.1 * np.abs(yq[:pb.m]).max() < 1.1 * np.abs(yq).max(), (name, b)
                bound_row_larger += 1
        s.close()
    assert checked >= 3 * B and bound_row_larger >= 1, (checked, bound_row_larger)


# --------------------------------------------------------------------------------------------------------------------- (b), (h)
def _ladder_script(sfb, B, front_cls, log=None):
    pb, d, rej, sp = _ladder_case(B)
    s = G0._solver(sfb, pb, B, qp_iter=QP_ITER)
    front = front_cls(sfb, s)
    front.set_start(d["x"], d["lam"], d["z"])
    start = front.state()
    n = front.direction(d)
    st, dbg = front.state(), _debug(s)
    if log is not None:
        log += [("start", start), ("direction", n, st)]
    # slots: rung 0 solved every agent that is not at a KKT point, ascending; the later rungs held agents 0 and 1 (then 0 alone),
    # who are the first two of that list, so every agent's last solve is still in the slot rung 0 gave it
    listed0 = [b for b in range(B) if b not in sp["optimal"]]
    slot = {b: k for k, b in enumerate(listed0)}
    assert n == B - len(sp["optimal"]) - (sp["infeasible"] is not None) == int(np.sum(st["status"] == R.RUNNING))
    if B == 67:
        assert np.all(st["status"][list(sp["optimal"])] == R.OPTIMAL) and st["status"][sp["infeasible"]] == R.PRIMAL_INFEASIBLE
        assert st["mu"][sp["concave"]] == 3.2768 and st["mu"][sp["first"]] == 1e-4 and dbg["list"][0] == sp["concave"]
        assert not np.delete(st["mu"], [sp["concave"], sp["first"]]).any()
        assert (slot[sp["concave"]], slot[sp["first"]]) == (0, 1)
    for b in range(B):                                                              # the start was not trivial
        if b not in sp["optimal"]:
            assert st["lam"][b].all() and st["z"][b].all()
    ref, stats = _ref_states(pb, st, dbg, slot), {}
    end, cur = _search(front, pb, ref, st, rej, stats=stats, log=log, tag="ladder B=%d" % B)
    for b in range(B):
        if not ref[b]["searching"]:                                                 # frozen or failed before the search: every bit kept
            for key in STATE:
                assert _bits(cur[key][b], st[key][b]), (b, key)
        elif rej[b] == 11:
            assert cur["status"][b] == R.UNKNOWN and cur["alpha"][b] == 2.0 ** -10
            for key in ("x", "lam", "z", "iter", "mu"):
                assert _bits(cur[key][b], st[key][b]), (b, key)
        else:
            assert cur["status"][b] == R.RUNNING and cur["iter"][b] == 1 and cur["alpha"][b] == 2.0 ** -rej[b], b
    if B == 67:
        assert cur["mu"][sp["concave"]] == 0.8192 and cur["alpha"][sp["concave"]] == 0.5   # 3.2768 / 4, above mu_first
        assert cur["mu"][sp["first"]] == 0.0 and cur["iter"][sp["first"]] == 1             # exactly mu_first: to 0
        for v in REJECTIONS:
            assert sum(ref[b]["searching"] and rej[b] == v for b in range(B)) >= 3, v
        assert stats["armijo"] >= 20 and stats["violation"] >= 20, stats
    s.close()
    return stats


@pytest.mark.parametrize("B", BATCHES)
def test_scripted_search_on_a_mixed_swarm(sfb, B):
    """the ladder problem: searching agents refused 0, 1, 2, 5, 10 or 11 times among frozen, failed and shifted ones"""
    stats = _ladder_script(sfb, B, _Dev)
    print("B = %d: %r" % (B, stats))


@pytest.mark.parametrize("B", BATCHES)
def test_scripted_search_on_a_partly_bounded_problem(sfb, B):
    """n = 9, m = 5, bounds on some variables only: zq is gathered through bound_row, 0 for the free ones"""
    pb = G0._convex_qp_nlp(1, 31)[0]
    assert 0 < pb.nb < pb.n
    _, _, searched, rej, stats = _scripted_round(sfb, pb, B, 400, "convexqp B=%d" % B)
    assert len(searched) >= (B + 1) // 2 and (B < 67 or all(sum(rej[b] == v for b in searched) >= 2 for v in REJECTIONS)), (searched, stats)
    assert B < 67 or (stats.get("armijo", 0) >= 10 and stats.get("violation", 0) >= 10), stats


@pytest.mark.parametrize("B", (3, 67))
def test_host_pointer_entries_equal_the_device_entries(sfb, B):
    """the same script through sfb_nlp_sqp_*_host on numpy arrays: after every call the state sfb_nlp_sqp_state_host returns and the
    returned count are those of the run through the device entries, bit for bit"""
    dev, host = [], []
    _ladder_script(sfb, B, _Dev, log=dev)
    _ladder_script(sfb, B, _Host, log=host)
    assert len(dev) == len(host) and len(dev) >= 4
    for a, b in zip(dev, host):
        assert a[0] == b[0]
        if a[0] == "trial":
            assert _bits(a[1], b[1])
            continue
        assert a[0] == "start" or a[1] == b[1], (a[0], a[1], b[1])
        for key in STATE:
            assert _bits(a[-1][key], b[-1][key]), (a[0], key)


# --------------------------------------------------------------------------------------------------------------------- (c)
def _direct_solve(sfb, s, plan, pb, count, wx, wy):
    """the sparse solver called directly on the first `count` slots of the solver's own QP arrays -> d, y, code, iter"""
    torch = G0._torch()
    dbg = s.debug_views()
    x, y = torch.empty((count, pb.n), dtype=torch.float64, device="cuda"), torch.empty((count, pb.mq), dtype=torch.float64, device="cuda")
    it, code = torch.empty(count, dtype=torch.int32, device="cuda"), torch.empty(count, dtype=torch.int32, device="cuda")
    twx, twy = T(wx), T(wy)
    ws = torch.empty(plan.workspace_bytes(count) // 8 + 2, dtype=torch.float64, device="cuda")
    plan.solve_batch_device(count, *[dbg[k].data_ptr() for k in QP_ARRAYS], x.data_ptr(), y.data_ptr(), 0, it.data_ptr(), code.data_ptr(),
                            ws.data_ptr(), prm=s.params.qp, dwarm_x=twx.data_ptr(), dwarm_y=twy.data_ptr())
    torch.cuda.synchronize()
    return H(x), H(y), H(code), H(it)


@pytest.mark.parametrize("B", BATCHES)
def test_three_scripted_iterations_and_the_warm_start(sfb, B):
    """three direction / search / commit rounds on fresh random inputs, steps 1, 1/4 and 1/2 by agent, some agents frozen from the
    start so that slot k of the list is not agent k.  nu is the running maximum, bit for bit, and is held by it for some agent; at
    rounds 2 and 3 the rung's (d, y, code, iter) are bit for bit the sparse solver's on the rung's own arrays warm-started from the
    (d, y) each listed agent was given the round before, gathered by the list -- and not those of a cold start."""
    pb = G0._convex_qp_nlp(1, 31)[0]
    pat = pb.pat
    frozen = {1: (), 3: (0,), 67: (0, 7, 8, 33, 66)}[B]
    s = G0._solver(sfb, pb, B, qp_iter=QP_ITER, mu_max=0.0)
    plan = sfb.SparseQPPlan(pb.n, pb.mq, pat["P_colptr"], pat["P_rowind"], pat["A_rowptr"], pat["A_colind"], ordering=1)
    front = _Dev(sfb, s)
    last_d, last_y, nu_prev = np.zeros((B, pb.n)), np.zeros((B, pb.mq)), np.zeros(B)
    held = warm_differs = compacted = 0
    for rnd in range(3):
        d = _inputs(pb, B, SEEDS_C[B] + rnd, frozen if rnd == 0 else ())
        if rnd == 0:
            front.set_start(d["x"], d["lam"], d["z"])
        before = front.state()
        n = front.direction(d)
        st, dbg = front.state(), _debug(s)
        listed, slot = _one_rung_slots(before, st, dbg, n)
        assert listed and all(b not in frozen for b in listed)
        compacted += any(k != b for k, b in enumerate(listed))
        if rnd:
            got = _direct_solve(sfb, s, plan, pb, len(listed), last_d[listed], last_y[listed])
            for key, g in zip(("d", "y", "code", "iter"), got):
                assert _bits(dbg[key][:len(listed)], g), (rnd, key)
            cold = _direct_solve(sfb, s, plan, pb, len(listed), np.zeros((len(listed), pb.n)), np.zeros((len(listed), pb.mq)))
            warm_differs += int(np.sum(got[3] != cold[3]))
        for b in np.nonzero(st["status"] == R.RUNNING)[0]:
            nu = R.step_start_ref(pb, d["f"][b], d["df"][b], d["g"][b], dbg["d"][slot[b]], dbg["y"][slot[b]], nu_prev[b])[0]
            assert _bits(st["nu"][b], nu) and nu >= nu_prev[b], (rnd, b)
            held += bool(rnd and nu == nu_prev[b] and 1.1 * np.abs(dbg["y"][slot[b]][:pb.m]).max() < nu)
            last_d[b], last_y[b] = dbg["d"][slot[b]], dbg["y"][slot[b]]
        nu_prev = st["nu"].copy()
        rej = [(0, 2, 1)[(b + rnd) % 3] for b in range(B)]
        ref, cur = _search(front, pb, _ref_states(pb, st, dbg, slot), st, rej, tag="round %d B=%d" % (rnd, B))
        for b in range(B):
            if ref[b]["status"] == R.RUNNING:
                assert cur["iter"][b] == rnd + 1 and cur["alpha"][b] == 2.0 ** -rej[b], (rnd, b)
    assert np.sum(cur["iter"] == 3) >= (B + 1) // 2, cur["iter"]
    assert warm_differs >= 1, "no iteration count differs from a cold start's: the case shows nothing"
    assert B == 1 or (compacted == 3 and held >= 1), (compacted, held)
    plan.close()
    s.close()


# --------------------------------------------------------------------------------------------------------------------- (d)
def _kkt_inputs(pb, d, b, st):
    """inputs that make agent b's current (x, lambda, z) a KKT point on a problem without bounds: g on a finite side of every row
    (no violation, no complementarity gap) and df = -(J' lambda + z), column by column"""
    assert pb.nb == 0
    d["g"][b] = G0._feasible(pb.gl, pb.gu)
    pat = pb.pat
    for c in range(pb.n):
        acc = 0.0
        for t in range(pat["Jc_colptr"][c], pat["Jc_colptr"][c + 1]):
            acc = acc + d["dg"][b][pat["Jc_pos"][t]] * st["lam"][b][pat["Jc_row"][t]]
        d["df"][b][c] = -(acc + st["z"][b][c])


@pytest.mark.parametrize("B", BATCHES)
def test_max_iterations_and_its_precedence(sfb, B):
    """max_iter = 2: after two commits the third direction call returns 0 and ends the running agents MaxIterations -- but Optimal
    where it finds a KKT point: the stopping test comes first -- writes the residuals of the stopping test, bit for bit kkt_ref's, and
    changes no other bit: no QP is assembled.  max_iter = 0: the first call ends everybody and the QP arrays stay zero."""
    pb = dict(R.zoo())["nb0"]
    s = G0._solver(sfb, pb, B, qp_iter=QP_ITER, mu_max=0.0, max_iter=2)
    front = _Dev(sfb, s)
    for rnd in range(2):
        d = _inputs(pb, B, 700 + rnd)
        if rnd == 0:
            front.set_start(d["x"], d["lam"], d["z"])
        before = front.state()
        n = front.direction(d)
        st, dbg = front.state(), _debug(s)
        _, slot = _one_rung_slots(before, st, dbg, n)
        _search(front, pb, _ref_states(pb, st, dbg, slot), st, [0] * B, tag="max_iter round %d" % rnd)
    before, qp = front.state(), _debug(s)
    running = [b for b in range(B) if before["status"][b] == R.RUNNING]
    assert len(running) >= (B + 1) // 2 and np.all(before["iter"][running] == 2)
    at_kkt = [b for b in running if B > 1 and b % 3 == 1]
    d = _inputs(pb, B, 702)
    for b in at_kkt:
        _kkt_inputs(pb, d, b, before)
    assert front.direction(d) == 0
    st, qp_after = front.state(), _debug(s)
    for b in range(B):
        res = R.kkt_ref(pb, before["x"][b], before["lam"][b], before["z"][b], d["df"][b], d["g"][b], d["dg"][b])
        if b in running:
            assert (max(res) <= 1e-6) == (b in at_kkt), (b, res)                    # a condition on the inputs
            assert st["status"][b] == (R.OPTIMAL if b in at_kkt else R.MAX_ITERATIONS), (b, st["status"][b])
            assert (st["r_stat"][b], st["r_pri"][b], st["r_comp"][b]) == res, b
        for key in STATE:
            if not (b in running and key in ("status", "r_stat", "r_pri", "r_comp")):
                assert _bits(st[key][b], before[key][b]), (b, key)
    assert B == 1 or (at_kkt and len(at_kkt) < len(running))
    for key in qp:
        assert _bits(qp_after[key], qp[key]) or key == "sums", key                  # (sums holds v1, which the stopping test writes)
    s.close()
    frozen = (1,) if B > 1 else ()
    s = G0._solver(sfb, pb, B, qp_iter=QP_ITER, mu_max=0.0, max_iter=0)
    front, d = _Dev(sfb, s), _inputs(pb, B, 703, frozen)
    front.set_start(d["x"], d["lam"], d["z"])
    assert front.direction(d) == 0
    st, dbg = front.state(), _debug(s)
    for b in range(B):
        assert st["status"][b] == (R.OPTIMAL if b in frozen else R.MAX_ITERATIONS) and st["iter"][b] == 0, b
        res = R.kkt_ref(pb, d["x"][b], d["lam"][b], d["z"][b], d["df"][b], d["g"][b], d["dg"][b])
        assert (st["r_stat"][b], st["r_pri"][b], st["r_comp"][b]) == res, b
    for key in QP_ARRAYS + ("d", "y"):
        assert not dbg[key].any(), key
    s.close()


# --------------------------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("B", BATCHES)
def test_a_direction_call_drops_an_open_line_search(sfb, B):
    """direction, trial, one refused accept (alpha = 1/2), then direction again on other inputs: x, lambda, z and iter are what they
    were, alpha is 1 again, the next trial point is clip(x + d_new), and the agent again has 11 trial points before Unknown: the
    halving count was reset."""
    pb = G0._convex_qp_nlp(1, 31)[0]
    s = G0._solver(sfb, pb, B, qp_iter=QP_ITER, mu_max=0.0)
    front, d = _Dev(sfb, s), _inputs(pb, B, SEEDS_E[B])
    front.set_start(d["x"], d["lam"], d["z"])
    start = front.state()
    n = front.direction(d)
    st, dbg = front.state(), _debug(s)
    _, slot = _one_rung_slots(start, st, dbg, n)
    ref, mid = _search(front, pb, _ref_states(pb, st, dbg, slot), st, [5] * B, max_rounds=1, tag="opened")
    open_ = [b for b in range(B) if ref[b]["searching"]]
    assert len(open_) >= (B + 1) // 2 and np.all(mid["alpha"][open_] == 0.5)
    d2 = _inputs(pb, B, SEEDS_E[B] + 1)
    n2 = front.direction(d2)
    st2, dbg2 = front.state(), _debug(s)
    _, slot2 = _one_rung_slots(mid, st2, dbg2, n2)
    again = [b for b in open_ if st2["status"][b] == R.RUNNING]
    assert len(again) >= (B + 1) // 2
    for b in again:
        for key in ("x", "lam", "z", "iter"):
            assert _bits(st2[key][b], start[key][b]), (b, key)
        assert st2["alpha"][b] == 1.0 and st2["iter"][b] == 0
    assert not _bits(dbg2["d"], dbg["d"])
    # _search checks the first trial point against clip(x + 1.0 d_new), and that the agents still search after 10 refusals
    end, cur = _search(front, pb, _ref_states(pb, st2, dbg2, slot2), st2, [11] * B, tag="reopened")
    for b in again:
        assert end[b]["halvings"] == 10 and cur["status"][b] == R.UNKNOWN and cur["alpha"][b] == 2.0 ** -10 and cur["iter"][b] == 0, b
    s.close()


# --------------------------------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("B", BATCHES)
def test_a_trial_point_that_does_not_evaluate_is_refused(sfb, B):
    """f_trial = NaN, f_trial = +inf, and f_trial on the taking side of the Armijo line with one NaN entry in g_trial -- in row 0, in
    row 64 (n130 has m = 65: the second stride of the wave) and in a row with an infinite side -- are refusals: alpha halves and
    nothing else of the agent changes, eleven in a row end it Unknown, three in a row and a finite point commit at alpha = 1/8;
    the neighbours with finite values commit as ever.  The NaN entries of g_trial fail on the kernel before this test: its violation
    sum went through fmax, which drops a NaN, so the row counted as satisfied and the point was committed."""
    pb = dict(R.zoo())["n130"]
    assert pb.m == 65
    open_rows = [r for r in range(1, 64) if np.isinf(pb.gl[r]) or np.isinf(pb.gu[r])]
    kinds = (("gnan", 0), None, ("gnan", open_rows[0]), "fnan", ("gnan", 64), "finf")
    how = [("gnan", 64)] if B == 1 else [kinds[b % 6] for b in range(B)]
    rej = [((11, 3)[(b // 6) % 2] if how[b] is not None else b % 3) for b in range(B)]
    d = _inputs(pb, B, 900)
    s = G0._solver(sfb, pb, B, qp_iter=QP_ITER, mu_max=0.0)
    front = _Dev(sfb, s)
    front.set_start(d["x"], d["lam"], d["z"])
    start = front.state()
    n = front.direction(d)
    st, dbg = front.state(), _debug(s)
    _, slot = _one_rung_slots(start, st, dbg, n)
    ref = _ref_states(pb, st, dbg, slot)
    end, cur = _search(front, pb, ref, st, rej, how=how, tag="non-finite B=%d" % B)
    seen = set()
    for b in range(B):
        if not ref[b]["searching"]:
            continue
        seen.add((how[b], rej[b]) if how[b] is not None else None)
        if rej[b] == 11:
            assert cur["status"][b] == R.UNKNOWN and cur["alpha"][b] == 2.0 ** -10 and cur["iter"][b] == 0, (b, how[b])
            for key in ("x", "lam", "z", "mu", "nu"):
                assert _bits(cur[key][b], st[key][b]), (b, key)
        else:
            assert cur["status"][b] == R.RUNNING and cur["iter"][b] == 1 and cur["alpha"][b] == 2.0 ** -rej[b], (b, how[b])
    want = {(how[b], rej[b]) if how[b] is not None else None for b in range(B)}     # every kind the script holds was searched
    assert seen == want and (B < 67 or len(want) == 11), (seen, want)
    s.close()


# --------------------------------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("B", (3, 67))
@pytest.mark.parametrize("name", ("m0", "nb0", "allbounded", "n65", "n130"))
def test_scripted_search_at_the_edges_of_shape(sfb, name, B):
    """m = 0 (g_trial is an empty tensor: the C entry receives NULL), no bound row (every zq is 0: z <- z + alpha (0 - z)), every
    variable bounded, n and m beyond one wave"""
    pb = dict(R.zoo())[name]
    st, cur, searched, rej, stats = _scripted_round(sfb, pb, B, 600, "%s B=%d" % (name, B))
    assert len(searched) >= (B + 1) // 2, (name, searched)
    assert B < 67 or all(sum(rej[b] == v for b in searched) >= 2 for v in REJECTIONS), (name, searched)
    assert stats.get("armijo", 0) >= 1 and (pb.m == 0) == (stats.get("violation", 0) == 0), (name, stats)
    if name == "nb0":
        for b in searched:
            if rej[b] < 11:
                alpha = 2.0 ** -rej[b]
                assert _bits(cur["z"][b], st["z"][b] + alpha * (0.0 - st["z"][b])), b
