"""The swarm SQP solver on the GPU (smooth_feedback_amd/nlp.py over sfb_nlp_sqp_*; kernels in csrc/nlp_sqp.hip) against the CPU
reference of tests/nlp_sqp_ref.py: the assembly and the stopping test bit for bit, the wave-reduced sums against np.longdouble
within the 4 (k + 2) eps slack of tests/qp_certify.py, a direction against the sparse solver called directly on the same arrays,
the shift ladder on a concave agent among convex ones, and HS71 and a collocation OCP end to end within the gates of
tests/nlp_sqp_gates.py.  Batches
1, 3 and 67 (more than one wave of agents, no multiple of it); every case runs in a few seconds."""
import numpy as np
import pytest

import nlp_sqp_gates as G
import nlp_sqp_ref as R

pytestmark = pytest.mark.gpu
BATCHES = (1, 3, 67)
LD = np.longdouble


def _torch():
    import torch
    return torch


def T(a):
    torch = _torch()
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to("cuda")


def H(t):
    return t.cpu().numpy()


def _solver(sfb, pb, B, qp_iter=200, **kw):
    prm = sfb.NLPSQPParams(qp=sfb.QPSolverParams(eps_abs=1e-9, eps_rel=1e-9, max_iter=qp_iter), **kw)
    return sfb.NLPSwarmSQP(*pb.args(), B, prm)


def _feasible(lo, hi):
    """a point inside [lo, hi] per entry (on a finite side, 0 between two infinite ones)"""
    return np.where(np.isfinite(lo), lo, np.where(np.isfinite(hi), hi, 0.0))


def _random_inputs(pb, B, seed, definite, optimal=()):
    """per agent random x, lam, z, f, df, g, dg, hess; definite: a diagonally dominant Hessian.  Agents in `optimal` sit at a KKT
    point (zero gradient and multipliers, feasible g and x): the stopping test takes them out of the list."""
    rng = np.random.default_rng(seed)
    d = dict(x=rng.normal(size=(B, pb.n)), lam=rng.normal(size=(B, pb.m)), z=rng.normal(size=(B, pb.n)), f=rng.normal(size=B),
             df=rng.normal(size=(B, pb.n)), g=rng.normal(size=(B, pb.m)), dg=rng.normal(size=(B, pb.nnzJ)), hess=rng.normal(size=(B, pb.nnzH)))
    if definite:
        diag = np.asarray(pb.Hi) == np.repeat(np.arange(pb.n), np.diff(pb.Hp))
        d["hess"][:, diag] = 2.0 * pb.n + rng.random((B, pb.n))
    for b in optimal:
        d["x"][b], d["g"][b] = _feasible(pb.xl, pb.xu), _feasible(pb.gl, pb.gu)
        d["lam"][b], d["z"][b], d["df"][b] = 0.0, 0.0, 0.0
    return d


def _direction(s, d):
    s.set_start(T(d["x"]), T(d["lam"]), T(d["z"]))
    return s.direction(T(d["f"]), T(d["df"]), T(d["g"]), T(d["dg"]), T(d["hess"]))


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# --------------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("B", BATCHES)
def test_assembly_and_stopping_test_equal_the_reference_bit_for_bit(sfb, B):
    """over the zoo's patterns, random values, infinite bounds included: the QP arrays of the rung are numpy's copies, one add
    (mu = 0 here) and one subtraction; the three residuals are the law's fixed-order maxima; v1, d.d and d.P d reduce across a wave
    and are held to np.longdouble within 4 (k + 2) eps times the sum of the absolute terms.  Lists: everybody, nobody, one agent,
    every other agent."""
    for name, pb in R.zoo():
        lists = [set()] if B == 1 else [set(), set(range(B)), set(range(B)) - {B // 2}, set(range(0, B, 2))]
        for li, optimal in enumerate(lists):
            if li and name not in ("n4", "n65", "m0"):                              # the list shapes on three patterns, everybody on all
                continue
            d = _random_inputs(pb, B, 1000 + li, definite=True, optimal=optimal)
            s = _solver(sfb, pb, B, qp_iter=50, mu_max=0.0)                         # no shifted rung: the first rung is the last
            _direction(s, d)
            st, dbg = {k: H(v) for k, v in s.state_views().items()}, {k: H(v) for k, v in s.debug_views().items()}
            listed = [b for b in range(B) if b not in optimal]
            assert np.all(st["status"][sorted(optimal)] == R.OPTIMAL), (name, li)
            assert np.array_equal(dbg["list"][:len(listed)], listed), (name, li)
            for k, b in enumerate(listed):
                want = R.assemble_ref(pb, d["x"][b], 0.0, d["df"][b], d["g"][b], d["dg"][b], d["hess"][b])
                for key, w in zip(("Px", "q", "Ax", "l", "u"), want):
                    assert _same(dbg[key][k], w), (name, li, b, key)
            for key in ("Px", "q", "Ax", "l", "u"):                                 # nothing is written behind the list
                assert not dbg[key][len(listed):].any(), (name, li, key)
            for b in range(B):
                rs, rp, rc = R.kkt_ref(pb, d["x"][b], d["lam"][b], d["z"][b], d["df"][b], d["g"][b], d["dg"][b])
                assert (st["r_stat"][b], st["r_pri"][b], st["r_comp"][b]) == (rs, rp, rc), (name, li, b)
                v1, absv, kv = R.v1_ref(pb, d["g"][b])
                assert abs(LD(dbg["sums"][0][b]) - v1) <= R.slack(kv, absv), (name, li, b, "v1")
            checked = 0
            for k, b in enumerate(listed):                                          # the judge's sums, from the rung's own Px and d
                if not np.all(np.isfinite(dbg["d"][k])):
                    continue
                dd, absdd, kdd, dPd, absdPd, kP = R.judge_sums_ref(pb, dbg["Px"][k], dbg["d"][k])
                assert abs(LD(dbg["sums"][3][b]) - dd) <= R.slack(kdd, absdd), (name, li, b, "d.d")
                assert abs(LD(dbg["sums"][4][b]) - dPd) <= R.slack(kP, absdPd), (name, li, b, "d.P d")
                checked += 1
            assert checked == len(listed), (name, li, checked, len(listed))         # the capped solves still return finite iterates
            s.close()


@pytest.mark.parametrize("B", (3, 67))
def test_assembly_with_a_shift_and_a_compacted_list(sfb, B):
    """indefinite Hessians and mu_max = mu_first: the rung after the first has mu = 1e-4 on its diagonals and holds the agents
    the first rung rejected, compacted in ascending order; the others are not assembled again"""
    for name in ("n4", "n64", "allbounded"):
        pb = dict(R.zoo())[name]
        d = _random_inputs(pb, B, 2000, definite=False)
        s = _solver(sfb, pb, B, qp_iter=50, mu_max=1e-4)
        _direction(s, d)
        st, dbg = {k: H(v) for k, v in s.state_views().items()}, {k: H(v) for k, v in s.debug_views().items()}
        listed = [b for b in range(B) if st["mu"][b] != 0.0]                        # whoever was rejected once was solved with mu = 1e-4
        assert set(np.unique(st["mu"])) <= {0.0, 1e-4, 8e-4}, name
        assert np.all(st["status"][st["mu"] == 8e-4] == R.UNKNOWN), name            # rejected again: beyond mu_max
        assert np.array_equal(dbg["list"][:len(listed)], listed), name
        assert listed, "%s: no agent was rejected, the case shows nothing" % name
        for k, b in enumerate(listed):
            want = R.assemble_ref(pb, d["x"][b], 1e-4, d["df"][b], d["g"][b], d["dg"][b], d["hess"][b])
            for key, w in zip(("Px", "q", "Ax", "l", "u"), want):
                assert _same(dbg[key][k], w), (name, b, key)
        s.close()


# --------------------------------------------------------------------------------------------------------------------- 3
def _convex_qp_nlp(B, seed):
    """a strictly convex QP posed as an NLP: f = x.H x / 2 + c.x with one H pattern and per-agent values, g = J x, a feasible box"""
    rng = np.random.default_rng(seed)
    n, m = 9, 5
    base = R.random_problem(seed, n, m, jac_density=0.5, hess_density=0.4)
    xl, xu = np.full(n, -np.inf), np.full(n, np.inf)
    xl[::2], xu[::3] = -1.0, 1.0
    J0 = np.zeros((m, n))
    rows = np.repeat(np.arange(m), np.diff(base.Jp))
    dgv = rng.normal(size=(B, base.nnzJ))
    xs = rng.uniform(-0.5, 0.5, n)
    J0[rows, base.Jj] = dgv[0]
    gl, gu = J0 @ xs - 0.5, J0 @ xs + 0.5
    gu[1], gl[2] = np.inf, -np.inf
    pb = R.Problem(n, m, base.Jp, base.Jj, base.Hp, base.Hi, xl, xu, gl, gu)
    dgv[:] = dgv[0]                                                                 # one J, so that xs is feasible for every agent
    hv = 0.3 * rng.normal(size=(B, pb.nnzH))
    diag = np.asarray(pb.Hi) == np.repeat(np.arange(n), np.diff(pb.Hp))
    hv[:, diag] = n + rng.random((B, n))
    c = rng.normal(size=(B, n))
    Hd = np.zeros((B, n, n))
    cols = np.repeat(np.arange(n), np.diff(pb.Hp))
    Hd[:, pb.Hi, cols] = hv
    Hd = Hd + np.transpose(np.triu(Hd, 1), (0, 2, 1))
    torch = _torch()
    tH, tJ, tc, thv, tdg = T(Hd), T(np.broadcast_to(J0, (B, m, n))), T(c), T(hv), T(dgv)

    def evaluate(x, lam, want):
        Hx = torch.einsum("bij,bj->bi", tH, x)
        f = 0.5 * (x * Hx).sum(1) + (tc * x).sum(1)
        g = torch.einsum("bij,bj->bi", tJ, x).contiguous()
        if not want:
            return f, g
        return f, g, (Hx + tc).contiguous(), tdg, thv
    return pb, evaluate, rng.uniform(-0.4, 0.4, (B, n))


@pytest.mark.parametrize("B", BATCHES)
def test_direction_of_a_convex_qp_is_the_sparse_solver(sfb, B):
    torch = _torch()
    pb, evaluate, x0 = _convex_qp_nlp(B, 31)
    s = _solver(sfb, pb, B, qp_iter=4000, tol=1e-6)
    s.set_start(T(x0))
    sv = s.state_views()
    assert s.direction(*_order(evaluate(sv["x"], sv["lam"], True))) == B
    dbg = s.debug_views()
    pat = pb.pat
    plan = sfb.SparseQPPlan(pb.n, pb.mq, pat["P_colptr"], pat["P_rowind"], pat["A_rowptr"], pat["A_colind"], ordering=1)
    x, y = torch.empty((B, pb.n), dtype=torch.float64, device="cuda"), torch.empty((B, pb.mq), dtype=torch.float64, device="cuda")
    it, code = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    wx, wy = torch.zeros_like(x), torch.zeros_like(y)
    ws = torch.empty(plan.workspace_bytes(B) // 8 + 2, dtype=torch.float64, device="cuda")
    plan.solve_batch_device(B, *[dbg[k].data_ptr() for k in ("Px", "q", "Ax", "l", "u")], x.data_ptr(), y.data_ptr(), 0, it.data_ptr(),
                            code.data_ptr(), ws.data_ptr(), prm=s.params.qp, dwarm_x=wx.data_ptr(), dwarm_y=wy.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(H(dbg["list"]), np.arange(B))
    assert np.all(H(code) == 0)
    for a, b in ((dbg["d"], x), (dbg["y"], y), (dbg["code"], code), (dbg["iter"], it)):
        assert np.array_equal(H(a), H(b))
    assert np.all(H(sv["mu"]) == 0.0) and np.all(H(sv["alpha"]) == 1.0) and np.all(H(sv["status"]) == R.RUNNING)
    # one full step, then Optimal at the next call
    d, xb = H(dbg["d"]), H(sv["x"]).copy()
    xt = s.trial()
    assert np.array_equal(H(xt), np.fmin(np.fmax(xb + 1.0 * d, pb.xl), pb.xu))
    assert s.accept(*evaluate(xt, sv["lam"], False)) == 0
    assert np.array_equal(H(sv["x"]), H(xt)) and np.all(H(sv["iter"]) == 1) and np.all(H(sv["alpha"]) == 1.0)
    assert np.array_equal(H(sv["lam"]), H(dbg["y"])[:, :pb.m])                      # lambda + 1.0 (y - lambda) from lambda = 0
    assert s.direction(*_order(evaluate(sv["x"], sv["lam"], True))) == 0
    assert np.all(H(sv["status"]) == R.OPTIMAL), (H(sv["r_stat"]).max(), H(sv["r_pri"]).max(), H(sv["r_comp"]).max())
    plan.close()
    s.close()


def _order(ev):
    f, g, df, dg, hess = ev
    return f, df, g, dg, hess


# --------------------------------------------------------------------------------------------------------------------- 4
def _ladder_problem():
    """n = 3, diagonal Hessian pattern, the box [-1, 1]^3, two rows that both read x0 with bounds [0, 1]"""
    return R.Problem(3, 2, [0, 1, 2], [0, 0], [0, 1, 2, 3], [0, 1, 2], [-1.0] * 3, [1.0] * 3, [0.0, 0.0], [1.0, 1.0])


def _ladder_inputs(B, kinds, seed=5):
    """kinds[b]: 'convex' (H = 2 I), 'concave' (H = -I), 'infeasible' (g = (-5, 5): the rows ask d0 >= 5 and d0 <= -4), 'nan'"""
    rng = np.random.default_rng(seed)
    d = dict(x=np.zeros((B, 3)), f=np.zeros(B), df=rng.uniform(0.2, 0.8, (B, 3)) * rng.choice([-1.0, 1.0], (B, 3)), g=np.full((B, 2), 0.5),
             dg=np.ones((B, 2)), hess=np.full((B, 3), 2.0), lam=np.zeros((B, 2)), z=np.zeros((B, 3)))
    for b, kind in enumerate(kinds):
        if kind == "concave":
            d["hess"][b] = -1.0
        elif kind == "infeasible":
            d["g"][b] = (-5.0, 5.0)
        elif kind == "nan":
            d["hess"][b, 1] = np.nan
    return d


def _kinds(B, special):
    kinds = ["convex"] * B
    for k, kind in enumerate(special):
        kinds[(k * 29 + B // 2) % B] = kind
    return kinds


@pytest.mark.parametrize("B", BATCHES)
def test_ladder_shifts_the_concave_agent_alone(sfb, B):
    pb = _ladder_problem()
    kinds = _kinds(B, ["concave"])
    d = _ladder_inputs(B, kinds)
    conc = kinds.index("concave")
    s = _solver(sfb, pb, B, qp_iter=500)
    assert _direction(s, d) == B
    st, dbg = {k: H(v) for k, v in s.state_views().items()}, {k: H(v) for k, v in s.debug_views().items()}
    assert st["mu"][conc] == 1e-4 * 8 ** 5 == 3.2768                                # every lower rung has d.P d < 0 for d != 0
    assert np.all(np.delete(st["mu"], conc) == 0.0) and np.all(st["status"] == R.RUNNING) and np.all(st["alpha"] == 1.0)
    assert dbg["list"][0] == conc and np.array_equal(dbg["Px"][0], -1.0 + np.full(3, 3.2768))   # the last rung: that agent alone
    assert dbg["sums"][4][conc] >= 1e-8 * dbg["sums"][3][conc] > 0.0
    keep = {k: v.copy() for k, v in st.items()}
    s.close()
    # mu_max = 1: the same agent ends Unknown, and nothing of the others differs
    s = _solver(sfb, pb, B, qp_iter=500, mu_max=1.0)
    assert _direction(s, d) == B - 1
    st = {k: H(v) for k, v in s.state_views().items()}
    assert st["status"][conc] == R.UNKNOWN and st["mu"][conc] == 3.2768
    others = np.arange(B) != conc
    for k in st:
        assert _same(st[k][others], keep[k][others]), k
    s.close()


@pytest.mark.parametrize("B", (3, 67))
def test_infeasible_rows_and_a_nan_hessian_end_their_agents_alone(sfb, B):
    pb = _ladder_problem()
    kinds = _kinds(B, ["infeasible", "nan"] if B == 3 else ["infeasible", "nan", "concave", "nan"])
    d = _ladder_inputs(B, kinds)
    s = _solver(sfb, pb, B, qp_iter=500)
    n_ok = sum(k in ("convex", "concave") for k in kinds)
    assert _direction(s, d) == n_ok
    st = {k: H(v) for k, v in s.state_views().items()}
    for b, kind in enumerate(kinds):
        want = {"convex": R.RUNNING, "concave": R.RUNNING, "infeasible": R.PRIMAL_INFEASIBLE, "nan": R.UNKNOWN}[kind]
        assert st["status"][b] == want, (b, kind, st["status"][b])
        if kind == "convex":
            assert st["mu"][b] == 0.0
        if kind == "infeasible":
            assert st["mu"][b] == 0.0                                               # the first rung decides: no shift is tried
        if kind == "nan":
            assert st["mu"][b] > 1e4
    # the convex agents are what they are in a batch without the others' trouble
    clean = _ladder_inputs(B, ["convex"] * B)
    s2 = _solver(sfb, pb, B, qp_iter=500)
    assert _direction(s2, clean) == B
    st2 = {k: H(v) for k, v in s2.state_views().items()}
    conv = np.array([k == "convex" for k in kinds])
    xt, xt2 = H(s.trial()), H(s2.trial())
    assert np.array_equal(xt[conv], xt2[conv])
    for k in st:
        assert _same(st[k][conv], st2[k][conv]), k
    s.close()
    s2.close()


# --------------------------------------------------------------------------------------------------------------------- 5
def test_hs71_end_to_end(sfb):
    """the standard start and the 24 perturbed starts in one batch, model in torch on the device.  tol and the iteration cap come from
    the CPU reference's run (tests/nlp_sqp_gates.py); every agent must report Optimal, pass an independent np.longdouble KKT
    statement and reach f*; agents that finish early are not touched by later calls."""
    torch = _torch()
    pb, starts = R.hs71_problem(), R.hs71_starts()
    B = len(starts)
    evaluate = R.hs71_eval(torch)
    s = _solver(sfb, pb, B, qp_iter=10000, tol=G.HS71_GPU_TOL, max_iter=G.HS71_GPU_CAP)
    s.set_start(T(starts))
    sv = s.state_views()
    frozen = {}
    calls = 0
    while True:
        searching = s.direction(*_order(evaluate(sv["x"], sv["lam"], True)))
        calls += 1
        now = {k: H(v).copy() for k, v in sv.items()}
        for b, snap in frozen.items():                                              # finished earlier: bit for bit what it was
            for k in now:
                assert _same(now[k][b], snap[k]), (b, k)
        for b in np.nonzero(now["status"] != R.RUNNING)[0]:
            frozen.setdefault(int(b), {k: now[k][b].copy() for k in now})
        if searching == 0:
            break
        assert calls <= G.HS71_GPU_CAP + 1
        while searching:
            xt = s.trial()
            searching = s.accept(*evaluate(xt, sv["lam"], False))
    st = {k: H(v) for k, v in s.state_views().items()}
    f, g, df, dg, _ = [H(a) for a in evaluate(sv["x"], sv["lam"], True)]
    for b in range(B):
        print("start %2d: status %d iter %d  stat %.3g pri %.3g comp %.3g  |f - f*| %.3g" %
              (b, st["status"][b], st["iter"][b], st["r_stat"][b], st["r_pri"][b], st["r_comp"][b], abs(f[b] - R.HS71_F)))
    assert np.all(st["status"] == R.OPTIMAL), st["status"]
    assert np.all(st["iter"] <= G.HS71_GPU_CAP)
    for b in range(B):
        cert = R.certify_kkt(pb, st["x"][b], st["lam"][b], st["z"][b], df[b], g[b], dg[b])
        assert max(cert) <= G.HS71_GPU_TOL * (1 + 1e-6), (b, cert)
        assert abs(f[b] - R.HS71_F) <= G.HS71_F_TOL, (b, f[b])
    # the convenience loop gives the same swarm
    s2 = _solver(sfb, pb, B, qp_iter=10000, tol=G.HS71_GPU_TOL, max_iter=G.HS71_GPU_CAP)
    sol = s2.solve(lambda x, lam, want: evaluate(x, lam, want), T(starts))
    for k, v in st.items():
        assert _same(H(getattr(sol, k)), v), k
    s.close()
    s2.close()


@pytest.mark.parametrize("duals", (True, False))
def test_host_entries_stage_one_full_step_to_the_bits_of_the_device_entries(sfb, duals):
    """HS71 with batch 3 (odd, so that every staged array behind the first is only 8-byte aligned): set_start, direction, trial,
    accept and state through the _host entries on numpy arrays, and the same step through the device-pointer entries on torch
    tensors, from the same numbers.  The trial point and the eleven arrays of state are equal bit for bit; once with lambda and z
    given, once with both NULL."""
    import ctypes as C
    pb, B, ev = R.hs71_problem(), 3, R.hs71_eval(np)
    rng = np.random.default_rng(71)
    x0 = np.ascontiguousarray(R.hs71_starts()[[0, 1, 13]])
    lam0, z0 = (rng.uniform(0.05, 0.3, (B, pb.m)), rng.uniform(-0.1, 0.1, (B, pb.n))) if duals else (None, None)
    lam = lam0 if duals else np.zeros((B, pb.m))
    f, g, df, dg, hess = [np.ascontiguousarray(a) for a in ev(x0, lam, True)]
    dev, host = _solver(sfb, pb, B, qp_iter=4000), _solver(sfb, pb, B, qp_iter=4000)
    dev.set_start(T(x0), T(lam0) if duals else None, T(z0) if duals else None)
    n_dev = dev.direction(T(f), T(df), T(g), T(dg), T(hess))
    xt_dev = H(dev.trial())
    ft, gt = [np.ascontiguousarray(a) for a in ev(xt_dev, lam, False)]
    left_dev = dev.accept(T(ft), T(gt))
    st_dev = {k: H(v) for k, v in dev.state_views().items()}

    lib, check, n = sfb._capi.lib, sfb._capi.check, C.c_int64()
    P = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))    # noqa: E731
    check(lib.sfb_nlp_sqp_set_start_host(host._h, P(x0), P(lam0), P(z0)))
    check(lib.sfb_nlp_sqp_direction_host(host._h, P(f), P(df), P(g), P(dg), P(hess), C.byref(n)))
    assert n.value == n_dev == B                                                    # everybody takes the step
    xt = np.full((B, pb.n), 7.0)
    check(lib.sfb_nlp_sqp_trial_host(host._h, P(xt)))
    assert np.array_equal(xt, xt_dev)
    check(lib.sfb_nlp_sqp_accept_host(host._h, P(ft), P(gt), C.byref(n)))
    assert n.value == left_dev
    st = {k: np.full(v.shape, 7, dtype=v.dtype) for k, v in st_dev.items()}
    check(lib.sfb_nlp_sqp_state_host(host._h, *[st[k].ctypes.data for k in ("x", "lam", "z", "status", "iter", "r_stat", "r_pri", "r_comp", "mu", "alpha", "nu")]))
    assert len(st) == 11
    for k in st:
        assert _same(st[k], st_dev[k]), k
    dev.close()
    host.close()


def test_batch_zero_is_legal(sfb):
    torch = _torch()
    pb = R.hs71_problem()
    s = _solver(sfb, pb, 0)
    e = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")       # noqa: E731
    s.set_start(e(0, 4))
    assert s.direction(e(0), e(0, 4), e(0, 2), e(0, 8), e(0, 10)) == 0
    assert s.accept(e(0), e(0, 2)) == 0 and tuple(s.trial().shape) == (0, 4)
    s.close()


# --------------------------------------------------------------------------------------------------------------------- 6
def _ocp_torch_model(sfb, B):
    """the double integrator of nlp_sqp_ref.ocp_problem in torch on the device: model values, Jacobians and multiplier-contracted
    Hessians at the mesh's nodes, assembled into g, dg_dx and the Lagrangian Hessian by sfb_ocp_nlp_batch / sfb_ocp_nlp_hess_batch"""
    torch = _torch()
    mesh, dims = sfb.PHMesh(R.OCP_K, R.OCP_TAU0), R.OCP_DIMS
    vb, cb = [[int(v) for v in a] for a in sfb.ocp_nlp_structure(mesh, dims)]
    N, n = int(R.OCP_K.sum()), vb[4]
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")       # noqa: E731
    dFf, dFcr, dce = z(B, N, 2, 4), z(B, N, 1, 4), z(B, 5, 6)
    dFf[:, :, 0, 2] = dFf[:, :, 1, 3] = dFcr[:, :, 0, 3] = 1.0                      # f = (x1, u), cr = u over (t | x0 x1 | u)
    dce[:, torch.arange(5), torch.arange(5)] = 1.0                                  # ce = (tf, x0, xf) over (tf | x0 | xf | q)
    HLf, HLcr, d2theta, d2ce_l, sigma = z(B, N, 4, 4), z(B, N, 4, 4), z(B, 6, 6), z(B, 6, 6), torch.ones(B, dtype=torch.float64, device="cuda")
    Hg = torch.diag(torch.tensor([0.0, 2.0, 2.0, 2.0], dtype=torch.float64, device="cuda"))
    df = z(B, n)
    df[:, vb[1]] = 1.0                                                              # theta = q

    def evaluate(x, lam, want):
        X, U = x[:, vb[2]:vb[3]].reshape(B, N + 1, 2), x[:, vb[3]:vb[4]].reshape(B, N, 1)
        Ff = torch.stack([X[:, :N, 1], U[:, :, 0]], 2).contiguous()
        Fg = (X[:, :N, 0] ** 2 + X[:, :N, 1] ** 2 + U[:, :, 0] ** 2).unsqueeze(2).contiguous()
        Fcr = U.contiguous()
        ce = torch.cat([x[:, :1], X[:, 0, :], X[:, N, :]], 1).contiguous()
        f = x[:, vb[1]].contiguous()
        if not want:
            return f, sfb.ocp_nlp_batch(mesh, dims, x, Ff, None, Fg, None, Fcr, None, ce, None)[0]
        dFg = z(B, N, 1, 4)
        dFg[:, :, 0, 1], dFg[:, :, 0, 2], dFg[:, :, 0, 3] = 2.0 * X[:, :N, 0], 2.0 * X[:, :N, 1], 2.0 * U[:, :, 0]
        g, dg = sfb.ocp_nlp_batch(mesh, dims, x, Ff, dFf, Fg, dFg, Fcr, dFcr, ce, dce)
        HLg = (lam[:, cb[1]].reshape(B, 1, 1, 1) * Hg).expand(B, N, 4, 4).contiguous()
        hess = sfb.ocp_nlp_hess_batch(mesh, dims, x.contiguous(), lam.contiguous(), sigma, dFf, HLf, dFg, HLg, dFcr, HLcr, d2theta, d2ce_l)
        return f, g, df, dg, hess
    return mesh, dims, evaluate


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("free", (False, True))
def test_double_integrator_ocp_end_to_end(sfb, B, free):
    """the reference's Ipopt-test problem on two intervals of degree 4, model in torch through sfb_ocp_nlp_batch / _hess_batch, from
    the straight line between the end states (with tf pinned to 5 also from two perturbations of it); free: the reference's own
    scenario, tf in [3, 6].  Gates as for HS71, from the CPU reference's run at tol 1e-7 (tests/nlp_sqp_gates.py: with tf pinned the
    reference's straight-line run crawls to its cap, so tol is four times the residual it had there and the cap is 40 + 2).  Every
    agent Optimal, certified by the independent longdouble KKT statement on the numpy restatement's own evaluation at the returned
    point, and at the reference's objective."""
    pb = R.ocp_problem(free)
    tol, cap, objective = (G.OCP_FREE_GPU_TOL, G.OCP_FREE_GPU_CAP, G.OCP_FREE_OBJECTIVE) if free else (G.OCP_GPU_TOL, G.OCP_GPU_CAP, G.OCP_OBJECTIVE)
    mesh, dims, evaluate = _ocp_torch_model(sfb, B)
    assert np.array_equal(sfb.ocp_nlp_pattern(mesh, dims)[1], pb.Jj) and np.array_equal(sfb.ocp_nlp_hess_pattern(mesh, dims)[1], pb.Hi)
    kinds = 1 if free else 3
    starts = (R.ocp_start()[None] if free else R.ocp_starts())[np.arange(B) % kinds]
    s = _solver(sfb, pb, B, qp_iter=10000, tol=tol, max_iter=cap)
    sol = s.solve(evaluate, T(starts))
    st = {k: H(getattr(sol, k)) for k in ("x", "lam", "z", "status", "iter", "r_stat", "r_pri", "r_comp")}
    ev = R.ocp_eval()
    for b in range(min(B, kinds)):
        print("%s agent %d: status %d iter %d  stat %.3g pri %.3g comp %.3g  tf %.9f objective %.10f" %
              ("tf in [3, 6]" if free else "tf = 5", b, st["status"][b], st["iter"][b], st["r_stat"][b], st["r_pri"][b], st["r_comp"][b], st["x"][b, 0], st["x"][b, 1]))
    assert np.all(st["status"] == R.OPTIMAL), st["status"]
    assert np.all(st["iter"] <= cap)
    for b in range(min(B, kinds)):                                                  # one of each start
        _, g, df, dg, _ = ev(st["x"][b], st["lam"][b], True)
        cert = R.certify_kkt(pb, st["x"][b], st["lam"][b], st["z"][b], df, g, dg)
        assert max(cert) <= tol * (1 + 1e-6), (b, cert)
        assert abs(st["x"][b, 1] - objective) <= G.OCP_OBJECTIVE_TOL, (b, st["x"][b, 1])
        if free:
            assert abs(st["x"][b, 0] - G.OCP_FREE_TF) <= 1e-6, st["x"][b, 0]
    for b in range(kinds, B):                                                       # equal starts give equal bits wherever they sit
        for k in st:
            assert _same(st[k][b], st[k][b % kinds]), (b, k)
    s.close()


# --------------------------------------------------------------------------------------------------------------------- 7
def test_reference_scenario_through_the_cpp_front(sfb):
    """examples/ocp_nlp_sqp.cpp: the reference's test_ocp_ipopt.cpp scenario (tf in [3, 6]) as caller code -- ocp_to_nlp on the
    lambdas (numerical derivatives), solve_nlp_sqp with batch 1 through host staging -- from the straight line; the CPU reference
    law arrives on this scenario (tests/nlp_sqp_gates.py), so: Optimal within its gates, at its objective, and nlpsol_to_ocpsol /
    ocpsol_to_nlpsol there and back within 1e-8 as test_ocp_ipopt.cpp:109-112 asks"""
    import ctypes as C
    from examples import models_lib as M
    lib = C.CDLL(M.PATH)
    pb = R.ocp_problem(free=True)
    dp = C.POINTER(C.c_double)
    lib.sfbx_ocp_nlp_sqp.argtypes = [C.c_double, C.c_double, dp, C.c_int, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_int32), dp, dp]
    x0, x, lam, rt = R.ocp_start(), np.zeros(pb.n), np.zeros(pb.m), np.zeros(4)
    it, obj = C.c_int32(), C.c_double()
    P = lambda a: a.ctypes.data_as(dp)                                              # noqa: E731
    st = lib.sfbx_ocp_nlp_sqp(3.0, 6.0, P(x0), pb.n, G.OCP_FREE_GPU_TOL, G.OCP_FREE_GPU_CAP, P(x), P(lam), C.byref(it), C.byref(obj), P(rt))
    print("C++ front: status %d iter %d objective %.10f tf %.9f  round trip |dx| %.2e |dzl| %.2e |dzu| %.2e |dlambda| %.2e" %
          (st, it.value, obj.value, x[0], *rt))
    assert st == R.OPTIMAL and it.value <= G.OCP_FREE_GPU_CAP
    assert abs(obj.value - G.OCP_FREE_OBJECTIVE) <= G.OCP_OBJECTIVE_TOL and abs(x[0] - G.OCP_FREE_TF) <= 1e-6
    assert np.all(rt <= 1e-8), rt
    st = lib.sfbx_ocp_nlp_sqp(3.0, 6.0, P(x0), pb.n - 1, 1e-6, 5, P(x), P(lam), C.byref(it), C.byref(obj), P(rt))
    assert st == -3


# --------------------------------------------------------------------------------------------------------------------- 8
STREAM_ENTRIES = ("sfb_nlp_sqp_set_start", "sfb_nlp_sqp_direction", "sfb_nlp_sqp_trial", "sfb_nlp_sqp_accept")


def _stream_job(sfb, B, seed):
    """one Job of tests/stream_contract.py over the four stream entries: set_start, direction, trial, accept, trial on one handle.
    The problem is the ladder's with convex agents only (H = 2 I at x = 0, both rows g = x0 + 0.5 in [0, 1]): the QP's solution is
    d = -df / 2, inside every bound, so the first trial point is -df / 2, the full step passes the Armijo test with the f and g given
    for it, and the second trial point is the committed x, the same."""
    import ctypes as C
    import stream_contract as SC
    pb = _ladder_problem()
    d = _ladder_inputs(B, ["convex"] * B, seed=seed)
    step = -d["df"] / 2.0
    inputs = dict(x=d["x"], f=d["f"], df=d["df"], g=d["g"], dg=d["dg"], hess=d["hess"],
                  ft=(step * step).sum(1) + (d["df"] * step).sum(1), gt=0.5 + np.repeat(step[:, :1], 2, axis=1))
    s = _solver(sfb, pb, B, qp_iter=500)
    lib = sfb._capi.lib

    def call(ptr, stream):
        h, st, n = s._h, stream or None, C.c_int64()
        sfb._capi.check(lib.sfb_nlp_sqp_set_start(h, ptr["x"], None, None, st))
        sfb._capi.check(lib.sfb_nlp_sqp_direction(h, ptr["f"], ptr["df"], ptr["g"], ptr["dg"], ptr["hess"], C.byref(n), st))
        assert n.value == B
        sfb._capi.check(lib.sfb_nlp_sqp_trial(h, ptr["xt1"], st))
        sfb._capi.check(lib.sfb_nlp_sqp_accept(h, ptr["ft"], ptr["gt"], C.byref(n), st))
        assert n.value == 0
        sfb._capi.check(lib.sfb_nlp_sqp_trial(h, ptr["xt2"], st))

    def check(res):
        # the QP is solved to eps_abs = eps_rel = 1e-9 on data of size 1 and polished: 1e-7 holds it with two digits to spare
        assert np.abs(res["xt1"] - step).max() <= 1e-7, np.abs(res["xt1"] - step).max()
        assert np.array_equal(res["xt2"], res["xt1"])
    return SC.Job(inputs=inputs, inout={}, outputs={"xt1": ((B, 3), np.float64), "xt2": ((B, 3), np.float64)}, call=call, check=check, keep=[s])


def test_every_stream_entry_of_the_solver_is_in_the_contract_case():
    """the four entries that take the caller's stream (sfb.h names the parameter hip_stream) are the ones _stream_job calls"""
    import inspect
    import re
    import stream_contract as SC
    text = re.sub(r"/\*.*?\*/", " ", open(SC.HEADER).read(), flags=re.S)
    declared = sorted(m.group(1) for m in re.finditer(r"\bsfb_status\s+(sfb_\w+)\s*\(([^;{]*)\)\s*;", text) if re.search(r"void\s*\*\s*hip_stream\b", m.group(2)))
    assert declared == sorted(STREAM_ENTRIES)
    src = inspect.getsource(_stream_job)
    assert all("lib.%s(" % e in src for e in STREAM_ENTRIES)


@pytest.mark.parametrize("B", (3, 67))
def test_stream_contract_of_the_solver(sfb, B):
    """tests/stream_contract.py's run_case on non-blocking side streams behind a spin: baseline on the null stream twice, warm-up,
    the ordered run with the decoy's data in the buffers until the real inputs arrive on the stream, two handles on two streams at
    once.  direction and accept wait for their stream by contract (blocking=True): the asynchrony guard does not apply, the
    ordering and two-stream steps do."""
    import stream_contract as SC
    real, decoy = _stream_job(sfb, B, 5), _stream_job(sfb, B, 6)
    SC.run_case(real, decoy, blocking=True, name="sfb_nlp_sqp set_start/direction/trial/accept B=%d" % B)
    for job in (real, decoy):
        job.keep[0].close()
