"""The host-pointer entry points stage their arrays through one carved device buffer (capi_common.h, Staging).  Here
each of them is compared with its device-pointer twin, bit for bit: same seeded inputs, torch does the uploads of the
device-pointer call.  Odd batches, so that the later arrays of the buffer start at addresses that are only 8-byte
aligned; every optional pointer NULL and given."""
import ctypes as C

import numpy as np
import pytest

import pid_gates as G
from sparse_cases import dense_batch_to_sparse

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return 0 if t is None else t.data_ptr()


@pytest.mark.parametrize("outputs", ["obj+iter", "none"])
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("route,n,m", [("dense", 3, 5), ("dense", 40, 60), ("tall", 3, 40)])  # registers, LDS, reduced KKT
def test_dense_host_entry_equals_device_entry(sfb, route, n, m, warm, outputs):
    import torch
    B = 3
    P, q, A, l, u = (np.ascontiguousarray(a, dtype=np.float64) for a in sfb.random_qp_batch(11, B, m, n, 1.0))
    rng = np.random.default_rng(5)
    wx, wy = (0.1 * rng.standard_normal((B, n)), 0.1 * rng.standard_normal((B, m))) if warm else (None, None)
    cp = sfb.QPSolverParams(max_iter=500).to_c()
    lib = sfb._capi.lib
    host_fn, dev_fn = ((lib.sfb_qp_dense_tall_solve_batch_host, lib.sfb_qp_dense_tall_solve_batch) if route == "tall"
                       else (lib.sfb_qp_dense_solve_batch_host, lib.sfb_qp_dense_solve_batch))
    hp = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    x, y, obj = np.empty((B, n)), np.empty((B, m)), np.empty(B)
    it, code = np.empty(B, np.uint32), np.empty(B, np.int32)
    want = outputs != "none"
    sfb._capi.check(host_fn(C.byref(cp), B, n, m, hp(P), hp(q), hp(A), hp(l), hp(u), hp(wx), hp(wy), hp(x), hp(y),
                            hp(obj) if want else None, hp(it) if want else None, hp(code)))
    d = [_dev(a) for a in (P, q, A, l, u, wx, wy)]
    dx, dy, dobj = (torch.empty(s, dtype=torch.float64, device="cuda") for s in ((B, n), (B, m), (B,)))
    dit, dcode = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    sfb._capi.check(dev_fn(C.byref(cp), B, n, m, *[_p(t) or None for t in d], _p(dx), _p(dy), _p(dobj), _p(dit), _p(dcode), None))
    torch.cuda.synchronize()
    assert np.array_equal(x, dx.cpu().numpy()) and np.array_equal(y, dy.cpu().numpy())
    assert np.array_equal(code, dcode.cpu().numpy())
    if want:
        assert np.array_equal(obj, dobj.cpu().numpy())
        assert np.array_equal(it, dit.cpu().numpy().view(np.uint32))


def _trace_init(B, rows):
    t = np.zeros((B, rows, 5))
    t[:, :, 0] = -1.0  # the caller presets ITER = -1 (sfb.h); the host entries do it themselves
    return t


@pytest.mark.parametrize("rows,phases", [(8, False), (0, True), (8, True)])
def test_dense_phases_host_entry_equals_device_entry(sfb, rows, phases):
    import torch
    B, n, m = 2, 3, 5
    P, q, A, l, u = (np.ascontiguousarray(a, dtype=np.float64) for a in sfb.random_qp_batch(12, B, m, n, 1.0))
    prm = sfb.QPSolverParams(max_iter=500)
    r = sfb.solve_qp_batch_host(P, q, A, l, u, prm, trace_rows=rows, phases=phases)
    d = [_dev(a) for a in (P, q, A, l, u)]
    dx, dy, dobj = (torch.empty(s, dtype=torch.float64, device="cuda") for s in ((B, n), (B, m), (B,)))
    dit, dcode = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    dtr = _dev(_trace_init(B, rows)) if rows else None
    dph = torch.zeros((B, 16), dtype=torch.float64, device="cuda") if phases else None
    cp = prm.to_c()
    sfb._capi.check(sfb._capi.lib.sfb_qp_dense_solve_batch_phases(
        C.byref(cp), B, n, m, *[_p(t) for t in d], None, None, _p(dx), _p(dy), _p(dobj), _p(dit), _p(dcode), _p(dtr) or None, rows,
        _p(dph) or None, None))
    torch.cuda.synchronize()
    assert np.array_equal(r.primal, dx.cpu().numpy()) and np.array_equal(r.dual, dy.cpu().numpy())
    assert np.array_equal(r.objective, dobj.cpu().numpy()) and np.array_equal(r.code, dcode.cpu().numpy())
    assert np.array_equal(r.iter, dit.cpu().numpy().view(np.uint32))
    if rows:  # ITER, OBJ, PRI_RES, DUA_RES (TIME is a clock); rows the solve did not reach keep ITER = -1 and zeros
        assert np.array_equal(r.trace[:, :, :4], dtr.cpu().numpy()[:, :, :4])
        unused = r.trace[:, :, 0] < 0
        assert np.all(r.trace[unused][:, 0] == -1.0) and np.all(r.trace[unused][:, 1:] == 0.0)
    if phases:  # microseconds of a clock: not comparable, but they came down, six per problem
        assert r.phase_us.shape == (B, 6) and np.all(np.isfinite(r.phase_us)) and np.all(r.phase_us >= 0) and r.phase_us.sum() > 0


@pytest.fixture
def sparse_plan(sfb):
    n, m = 4, 6
    P, q, A, l, u = (np.ascontiguousarray(a, dtype=np.float64) for a in sfb.random_qp_batch(21, 5, m, n, 0.5))
    Pp, Pi, Px, Ap, Aj, Ax = dense_batch_to_sparse(P, A, n, m, upper_only=True)
    return sfb.SparseQPPlan(n, m, Pp, Pi, Ap, Aj), (Px, q, Ax, l, u)


@pytest.mark.parametrize("phases", [False, True])
@pytest.mark.parametrize("rows", [0, 8])
@pytest.mark.parametrize("warm", [False, True])
def test_sparse_host_entry_equals_device_entry(sfb, sparse_plan, warm, rows, phases):
    """Batch 3, then 5, then 3 on ONE plan: the plan's cached buffer grows, then is reused with room to spare.  The host
    calls ask for reuse_factor; on a batch that differs from the previous call's the entry must drop it, so every call
    equals the device-pointer solve with reuse_factor = 0 on a fresh workspace."""
    import torch
    plan, data = sparse_plan
    n, m = plan.n, plan.m
    rng = np.random.default_rng(8)
    for B in (3, 5, 3):
        Px, q, Ax, l, u = (np.ascontiguousarray(a[:B]) for a in data)
        wx, wy = (0.1 * rng.standard_normal((B, n)), 0.1 * rng.standard_normal((B, m))) if warm else (None, None)
        r = plan.solve_batch_host(Px, q, Ax, l, u, sfb.QPSolverParams(max_iter=500, reuse_factor=True), wx, wy, trace_rows=rows, phases=phases)
        d = [_dev(a) for a in (Px, q, Ax, l, u)]
        dx, dy, dobj = (torch.empty(s, dtype=torch.float64, device="cuda") for s in ((B, n), (B, m), (B,)))
        dit, dcode = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        ws = torch.zeros((plan.workspace_bytes(B) + 7) // 8, dtype=torch.float64, device="cuda")
        dtr = _dev(_trace_init(B, rows)) if rows else None
        dph = torch.zeros((B, 6), dtype=torch.float64, device="cuda") if phases else None
        dwx, dwy = _dev(wx), _dev(wy)
        cp = sfb.QPSolverParams(max_iter=500, reuse_factor=False).to_c()
        head = [plan._h, C.byref(cp), B] + [_p(t) for t in d] + [_p(dwx) or None, _p(dwy) or None, _p(dx), _p(dy), _p(dobj), _p(dit), _p(dcode),
                                                                 _p(ws)]
        lib = sfb._capi.lib
        if phases:
            sfb._capi.check(lib.sfb_sparse_qp_solve_batch_phases(*head, _p(dtr) or None, rows, _p(dph), None))
        elif rows:
            sfb._capi.check(lib.sfb_sparse_qp_solve_batch_trace(*head, _p(dtr), rows, None))
        else:
            sfb._capi.check(lib.sfb_sparse_qp_solve_batch(*head, None))
        torch.cuda.synchronize()
        assert np.array_equal(r.primal, dx.cpu().numpy()) and np.array_equal(r.dual, dy.cpu().numpy()), B
        assert np.array_equal(r.objective, dobj.cpu().numpy()) and np.array_equal(r.code, dcode.cpu().numpy()), B
        assert np.array_equal(r.iter, dit.cpu().numpy().view(np.uint32)), B
        if rows:
            assert np.array_equal(r.trace[:, :, :4], dtr.cpu().numpy()[:, :, :4]), B
            unused = r.trace[:, :, 0] < 0
            assert np.all(r.trace[unused][:, 0] == -1.0) and np.all(r.trace[unused][:, 1:] == 0.0)
        if phases:
            assert r.phase_us.shape == (B, 6) and np.all(np.isfinite(r.phase_us)) and np.all(r.phase_us >= 0) and r.phase_us.sum() > 0


def test_sparse_host_entry_without_obj_and_iter(sfb, sparse_plan):
    plan, data = sparse_plan
    B = 3
    Px, q, Ax, l, u = (np.ascontiguousarray(a[:B]) for a in data)
    prm = sfb.QPSolverParams(max_iter=500)
    ref = plan.solve_batch_host(Px, q, Ax, l, u, prm)
    x, y, code = np.empty((B, plan.n)), np.empty((B, plan.m)), np.empty(B, np.int32)
    cp = prm.to_c()
    hp = lambda a: a.ctypes.data  # noqa: E731
    sfb._capi.check(sfb._capi.lib.sfb_sparse_qp_solve_batch_host(plan._h, C.byref(cp), B, hp(Px), hp(q), hp(Ax), hp(l), hp(u), None, None,
                                                                 hp(x), hp(y), None, None, hp(code)))
    assert np.array_equal(x, ref.primal) and np.array_equal(y, ref.dual) and np.array_equal(code, ref.code)


@pytest.mark.parametrize("gains_shared", [0, 1])
@pytest.mark.parametrize("des_shared", [0, 1])
@pytest.mark.parametrize("group", ["SE2", "SE3R3"])  # one plain group, one bundle
def test_pid_step_host_entry_equals_device_entry(sfb, group, des_shared, gains_shared):
    import torch
    B, d, grp = 5, G.section("step", group), G.GROUPS[group]
    a = {k: np.ascontiguousarray(d[k][:B]) for k in ("x", "v", "gd", "vd", "ad", "kp", "kd", "ki", "ie", "t_last")}
    des = [a[k][2] if des_shared else a[k] for k in ("gd", "vd", "ad")]
    gains = [a[k][2] if gains_shared else a[k] for k in ("kp", "kd", "ki")]
    u, ie, tl = sfb.pid_step_batch_host(grp, G.T_STEP, a["x"], a["v"], *des, *gains, a["ie"], a["t_last"], windup_limit=G.WINDUP)
    dv = [_dev(t) for t in (a["x"], a["v"], *des)]
    dg = [_dev(t) for t in gains]
    die, dtl = _dev(a["ie"]), _dev(a["t_last"])
    du = torch.zeros((B, a["v"].shape[1]), dtype=torch.float64, device="cuda")
    sfb.pid_step_batch_device(grp, B, G.T_STEP, *[_p(t) for t in dv], des_shared, *[_p(t) for t in dg], gains_shared, G.WINDUP, _p(die), _p(dtl),
                              _p(du))
    torch.cuda.synchronize()
    assert np.array_equal(u, du.cpu().numpy()) and np.array_equal(ie, die.cpu().numpy())
    assert np.array_equal(tl, dtl.cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("gains_shared", [0, 1])
@pytest.mark.parametrize("des_shared", [0, 1])
@pytest.mark.parametrize("group", ["SE2", "SE3R3"])
def test_pid_rollout_host_entry_equals_device_entry(sfb, group, des_shared, gains_shared, clamp):
    import torch
    B, d, grp = 5, G.section("roll", group), G.GROUPS[group]
    a = {k: np.ascontiguousarray(d[k][:B]) for k in ("x", "v", "g0", "w", "kp", "kd", "ki", "ie", "t_last")}
    des = [a[k][1] if des_shared else a[k] for k in ("g0", "w")]
    gains = [a[k][1] if gains_shared else a[k] for k in ("kp", "kd", "ki")]
    um = np.ascontiguousarray(d["umax"]) if clamp else None
    r = sfb.pid_rollout_batch_host(grp, G.T0, G.DT, 3, a["x"], a["v"], *des, *gains, a["ie"], a["t_last"], windup_limit=G.WINDUP, u_max=um)
    dx, dvel = _dev(a["x"]), _dev(a["v"])
    dd, dg = [_dev(t) for t in des], [_dev(t) for t in gains]
    die, dtl, dum = _dev(a["ie"]), _dev(a["t_last"]), _dev(um)
    du = torch.zeros((B, a["v"].shape[1]), dtype=torch.float64, device="cuda")
    dc = torch.zeros(B, dtype=torch.float64, device="cuda")
    sfb.pid_rollout_batch_device(grp, B, G.T0, G.DT, 3, _p(dx), _p(dvel), *[_p(t) for t in dd], des_shared, *[_p(t) for t in dg], gains_shared,
                                 G.WINDUP, _p(dum), _p(die), _p(dtl), _p(du), _p(dc))
    torch.cuda.synchronize()
    for k, t in (("x", dx), ("v", dvel), ("i_err", die), ("t_last", dtl), ("u_last", du), ("cost", dc)):
        assert np.array_equal(r[k], t.cpu().numpy(), equal_nan=True), k


@pytest.mark.parametrize("info", [False, True])
@pytest.mark.parametrize("qs,ds,rs", [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)])
@pytest.mark.parametrize("part", ["predict", "update", "both"])
def test_ekf_host_entry_equals_device_entry(sfb, part, qs, ds, rs, info):
    import torch
    B, dof, ny = 5, 3, 2
    rng = np.random.default_rng(3)
    spd = lambda k, cnt: np.stack([(lambda M: M @ M.T + k * np.eye(k))(rng.standard_normal((k, k))).ravel() for _ in range(cnt)])  # noqa: E731
    P0, A = spd(dof, B), rng.standard_normal((B, dof * dof))
    Q, R = spd(dof, 1 if qs else B), spd(ny, 1 if rs else B)
    dt = np.full(1 if ds else B, 0.01) + (0 if ds else 0.001 * np.arange(B))
    H, r = rng.standard_normal((B, ny * dof)), rng.standard_normal((B, ny))
    predict, update = part != "update", part != "predict"
    lib = sfb._capi.lib
    hp = lambda a, on=True: a.ctypes.data if on else None  # noqa: E731
    P, delta, inf = P0.copy(), np.zeros((B, dof)), np.full(B, -7, np.int32)
    sfb._capi.check(lib.sfb_ekf_step_batch_host(B, dof, ny, hp(A, predict), hp(Q, predict), qs, hp(dt, predict), ds,
                                                hp(H, update), hp(R, update), rs, hp(r, update), hp(P), hp(delta, update),
                                                hp(inf, update and info)))
    dP, dA, dQ, ddt, dH, dR, dr = (_dev(a) for a in (P0, A, Q, dt, H, R, r))
    dd = torch.zeros((B, dof), dtype=torch.float64, device="cuda")
    di = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    dinfo = _p(di) if info else 0
    if part == "predict":
        sfb.ekf_predict_batch_device(B, dof, _p(dA), _p(dQ), qs, _p(ddt), ds, _p(dP))
    elif part == "update":
        sfb.ekf_update_batch_device(B, dof, ny, _p(dH), _p(dR), rs, _p(dr), _p(dP), _p(dd), dinfo)
    else:
        sfb.ekf_predict_update_batch_device(B, dof, ny, _p(dA), _p(dQ), qs, _p(ddt), ds, _p(dH), _p(dR), rs, _p(dr), _p(dP),
                                            _p(dd), dinfo)
    torch.cuda.synchronize()
    assert np.array_equal(P, dP.cpu().numpy())
    assert np.array_equal(delta, dd.cpu().numpy())  # (zeros on both sides without an update)
    assert np.array_equal(inf, di.cpu().numpy())    # (-7 on both sides where info is not asked for)
    if update and info:
        assert np.all(inf == 0)


@pytest.mark.parametrize("qs,ds", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("stages", [False, True])
def test_ekf_rk4_host_entry_equals_device_entry(sfb, stages, qs, ds):
    import torch
    B, dof = 5, 3
    rng = np.random.default_rng(4)
    spd = lambda: (lambda M: M @ M.T + 3 * np.eye(3))(rng.standard_normal((3, 3))).ravel()  # noqa: E731
    P0 = np.stack([spd() for _ in range(B)])
    A, Am, Ae = (rng.standard_normal((B, dof * dof)) for _ in range(3))
    Q = np.stack([0.1 * spd() for _ in range(1 if qs else B)])
    dt = 0.02 + 0.001 * np.arange(1 if ds else B)
    lib = sfb._capi.lib
    hp = lambda a, on=True: a.ctypes.data if on else None  # noqa: E731
    P = P0.copy()
    sfb._capi.check(lib.sfb_ekf_predict_rk4_batch_host(B, dof, hp(A), hp(Am, stages), hp(Ae, stages), hp(Q), qs, hp(dt), ds, hp(P)))
    dP, dA, dAm, dAe, dQ, ddt = (_dev(a) for a in (P0, A, Am, Ae, Q, dt))
    sfb._capi.check(lib.sfb_ekf_predict_rk4_batch(B, dof, _p(dA), _p(dAm) if stages else None, _p(dAe) if stages else None, _p(dQ), qs, _p(ddt),
                                                  ds, _p(dP), None))
    torch.cuda.synchronize()
    assert np.array_equal(P, dP.cpu().numpy())


def test_ekf_host_entry_refuses_an_update_without_delta(sfb):
    """as the device-pointer entry does: SFB_ERR_INVALID_ARG, and the covariance is left alone"""
    B, dof, ny = 5, 3, 2
    P = np.tile(np.eye(dof).ravel(), (B, 1))
    H, R, r = np.ones((B, ny * dof)), np.tile(np.eye(ny).ravel(), (B, 1)), np.ones((B, ny))
    hp = lambda a: a.ctypes.data  # noqa: E731
    st = sfb._capi.lib.sfb_ekf_step_batch_host(B, dof, ny, None, None, 0, None, 0, hp(H), hp(R), 0, hp(r), hp(P), None, None)
    assert st == 1 and b"update needs H, R, r, delta" in sfb._capi.lib.sfb_last_error()  # SFB_ERR_INVALID_ARG
    assert np.array_equal(P, np.tile(np.eye(dof).ravel(), (B, 1)))
