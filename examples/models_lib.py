"""ctypes loader of the example harness library (examples/models.cpp -> libsfb_models.so): concrete MPC / ASIF / EKF
models behind the C++ host front, used by bench.py, scripts/ and tests/ (`from examples import models_lib`)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "smooth_feedback_amd", "libsfb_models.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(PATH):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s"])
        import smooth_feedback_amd  # noqa: F401  (loads libsfb.so / torch's HIP runtime first)
        L = C.CDLL(PATH)
        L.sfbx_lie_selftest.restype = C.c_double
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def mpc_dims(variant, K):
    v = [C.c_int() for _ in range(7)]
    assert lib().sfbx_mpc_dims(variant, K, *[C.byref(x) for x in v]) == 0
    return dict(zip(("n", "m", "nnzP", "nnzA", "Nx", "Nu", "N"), [x.value for x in v]))


def mpc_pattern(variant, K, tf=5.0):
    d = mpc_dims(variant, K)
    Pp = np.zeros(d["n"] + 1, np.int32); Pi = np.zeros(d["nnzP"], np.int32); Pv = np.zeros(d["nnzP"])
    Ap = np.zeros(d["m"] + 1, np.int32); Aj = np.zeros(d["nnzA"], np.int32)
    assert lib().sfbx_mpc_pattern(variant, K, C.c_double(tf), _p(Pp), _p(Pi), _p(Pv), _p(Ap), _p(Aj)) == 0
    return d, Pp, Pi, Pv, Ap, Aj


def mpc_assemble_batch(variant, K, batch, seed=0, tf=5.0, threads=8):
    d = mpc_dims(variant, K)
    Av = np.zeros((batch, d["nnzA"])); l = np.zeros((batch, d["m"])); u = np.zeros((batch, d["m"]))
    assert lib().sfbx_mpc_assemble_batch(variant, K, C.c_double(tf), C.c_int64(batch), C.c_uint64(seed), _p(Av), _p(l),
                                         _p(u), threads) == 0
    return Av, l, u


def mesh(n_ivals, K):
    N = n_ivals * K
    nodes = np.zeros(N + 1); w = np.zeros(N + 1); D = np.zeros((K + 1) * K)
    assert lib().sfbx_mesh(n_ivals, K, _p(nodes), _p(w), _p(D)) == 0
    return nodes, w, D.reshape(K, K + 1).T  # D[j, i]


def mpc_stage(variant, K):
    d = mpc_dims(variant, K)
    st = np.zeros(d["n"] + d["m"], np.int32)
    assert lib().sfbx_mpc_stage(variant, K, _p(st)) == 0
    return st


def asif_basic_qp(x0, udes):
    """asif_to_qp of tests/test_asif.cpp:37-95 (host only): dict P (3,3), q, A (9,3), l, u."""
    x0 = np.asarray(x0, dtype=np.float64); udes = np.asarray(udes, dtype=np.float64)
    P = np.zeros(9); q = np.zeros(3); A = np.zeros(27); l = np.zeros(9); u = np.zeros(9)
    assert lib().sfbx_asif_basic_qp(_p(x0), _p(udes), _p(P), _p(q), _p(A), _p(l), _p(u)) == 0
    return dict(P=P.reshape(3, 3).T, q=q, A=A.reshape(3, 9).T, l=l, u=u)


def test_asif(which):
    """ASIFilter on the GPU (see models.h): dict u, code, iter, n, m and the QP (flat column-major) + x, y."""
    nmax, mmax = 8, 512
    u_out = np.zeros(3); code = C.c_int32(-1); it = C.c_uint32(0); dims = np.zeros(2, np.int32)
    P = np.zeros(nmax * nmax); q = np.zeros(nmax); A = np.zeros(mmax * nmax); l = np.zeros(mmax); u = np.zeros(mmax)
    x = np.zeros(nmax); y = np.zeros(mmax)
    rc = lib().sfbx_test_asif(which, _p(u_out), C.byref(code), C.byref(it), _p(dims), _p(P), _p(q), _p(A), _p(l), _p(u),
                              _p(x), _p(y))
    assert rc == 0
    n, m = int(dims[0]), int(dims[1])
    return dict(u=u_out, code=code.value, iter=it.value, n=n, m=m, P=P[:n * n].copy(), q=q[:n].copy(),
                A=A[:m * n].copy(), l=l[:m].copy(), ub=u[:m].copy(), x=x[:n].copy(), y=y[:m].copy())


def asif_swarm_step(batch, K, ticks=1, seed=0):
    n, m = 3, K + 3
    out = dict(u=np.zeros((batch, 2)), code=np.zeros(batch, np.int32), iter=np.zeros(batch, np.uint32),
               P=np.zeros((batch, n * n)), q=np.zeros((batch, n)), A=np.zeros((batch, m * n)), l=np.zeros((batch, m)),
               ub=np.zeros((batch, m)), x=np.zeros((batch, n)), y=np.zeros((batch, m)), wx=np.zeros((batch, n)),
               wy=np.zeros((batch, m)))
    rc = lib().sfbx_asif_swarm_step(C.c_int64(batch), C.c_uint64(seed), K, ticks, _p(out["u"]), _p(out["code"]),
                                    _p(out["iter"]), _p(out["P"]), _p(out["q"]), _p(out["A"]), _p(out["l"]), _p(out["ub"]),
                                    _p(out["x"]), _p(out["y"]), _p(out["wx"]), _p(out["wy"]))
    assert rc == 0
    return out


def mpc_layout(variant, K, tf=5.0):
    """MPCLayout (smooth_feedback_amd.mpc) of the variant's transcription, from the C++ front (MPC::device_layout)."""
    import smooth_feedback_amd as sfb
    dims = np.zeros(6, np.int32); alpha = np.zeros(128); D = np.zeros(72); kind = np.zeros(16, np.int32)
    dof = np.zeros(16, np.int32); crl = np.zeros(16); cru = np.zeros(16)
    assert lib().sfbx_mpc_layout(variant, K, C.c_double(tf), _p(dims), _p(alpha), _p(D), _p(kind), _p(dof), _p(crl), _p(cru)) == 0
    nx, nu, ncr, kmesh, nivals, nparts = [int(v) for v in dims]
    return sfb.MPCLayout(nx, nu, ncr, kmesh, nivals, tf, alpha[:nivals], D[:(kmesh + 1) * kmesh].reshape(kmesh + 1, kmesh),
                         parts=[(int(kind[g]), int(dof[g])) for g in range(nparts)], crl=crl[:ncr], cru=cru[:ncr])


def mpc_records(variant, K, batch, seed=0, tf=5.0, threads=8):
    """Linearisation records (MPC::fill_record) of the agents of mpc_assemble_batch."""
    L = mpc_layout(variant, K, tf)
    rec = np.zeros((batch, L.record_doubles()))
    assert lib().sfbx_mpc_records(variant, K, C.c_double(tf), C.c_int64(batch), C.c_uint64(seed), _p(rec), threads) == 0
    return L, rec


def mpc_swarm_step(variant, K, batch, ticks, seed=1, tf=5.0, device=False):
    """`ticks` closed-loop ticks through MPCSwarm (host assembly) or MPCSwarmDevice; outputs of the last tick."""
    u0 = np.zeros((batch, mpc_dims(variant, K)["Nu"])); codes = np.zeros(batch, np.int32); iters = np.zeros(batch, np.uint32)
    fn = lib().sfbx_mpc_swarm_device_step if device else lib().sfbx_mpc_swarm_step
    rc = fn(variant, K, C.c_double(tf), C.c_int64(batch), C.c_uint64(seed), ticks, _p(u0), _p(codes), _p(iters))
    assert rc == 0, rc
    return u0, codes, iters


def mpc_swarm_step_multi(variant, K, batch, ticks, devices, seed=1, tf=5.0):
    """mpc_swarm_step with every batched solve sharded over `devices` from this one process (MPCSwarm +
    QPSolver::shard_over_devices + sfb_set_devices)."""
    u0 = np.zeros((batch, mpc_dims(variant, K)["Nu"])); codes = np.zeros(batch, np.int32); iters = np.zeros(batch, np.uint32)
    dev = (C.c_int * len(devices))(*devices)
    rc = lib().sfbx_mpc_swarm_step_multi(variant, K, C.c_double(tf), C.c_int64(batch), C.c_uint64(seed), ticks, dev, len(devices),
                                         _p(u0), _p(codes), _p(iters))
    assert rc == 0, rc
    return u0, codes, iters


def last_tick_seconds(n):
    """wall seconds of every swarm.step() of the last mpc_swarm_step call"""
    out = np.zeros(n)
    k = lib().sfbx_last_tick_seconds(_p(out), n)
    return out[:k]


def mpc_doubleintegrator(ticks):
    """examples/mpc_doubleintegrator.cpp in closed loop, with the factor reuse of the solver front and without."""
    u = np.zeros(ticks); it = np.zeros(ticks, np.uint32); codes = np.zeros(ticks, np.int32)
    ur = np.zeros(ticks); itr = np.zeros(ticks, np.uint32); cnt = C.c_int64(0); sec = np.zeros(2)
    rc = lib().sfbx_test_mpc_doubleintegrator(ticks, _p(u), _p(it), _p(codes), _p(ur), _p(itr), C.byref(cnt), _p(sec))
    assert rc == 0, rc
    return dict(u=u, iter=it, code=codes, u_ref=ur, iter_ref=itr, reuse_count=cnt.value, seconds=sec)


def ocp_to_qp_basic(solve=False):
    """tests/test_ocp_to_qp.cpp:41-107 with the generic ocp_to_qp() front; solve=True also runs solve_qp and
    qpsol_to_ocpsol (needs a GPU)."""
    out = np.full(18, np.nan)
    rc = lib().sfbx_test_ocp_to_qp_basic(_p(out), int(solve))
    assert rc == 0, rc
    return out


_dev = None


def dev_lib():
    """libsfb_models_dev.so: the device-side fronts (examples/models_device.hip, compiled by hipcc)."""
    global _dev
    if _dev is None:
        lib()  # libsfb.so / the host harness first
        _dev = C.CDLL(os.path.join(ROOT, "smooth_feedback_amd", "libsfb_models_dev.so"))
    return _dev


def asif_swarm_states(batch, seed=0):
    st = np.zeros((batch, 7)); ud = np.zeros((batch, 2))
    assert lib().sfbx_asif_swarm_states(C.c_int64(batch), C.c_uint64(seed), _p(st), _p(ud)) == 0
    return st, ud


def asif_swarm_device_step(states, udes, K, ticks=1, reduced_kkt=False):
    """ASIFSwarmDevice (assembly and solve on the GPU) from the states of asif_swarm_states; outputs like asif_swarm_step.
    reduced_kkt: the filter's opt-in switch (ASIFilterParams::reduced_kkt), the QPs on the reduced-KKT route for tall problems."""
    batch = len(states)
    n, m = 3, K + 3
    out = dict(u=np.zeros((batch, 2)), code=np.zeros(batch, np.int32), iter=np.zeros(batch, np.uint32), P=np.zeros((batch, n * n)),
               q=np.zeros((batch, n)), A=np.zeros((batch, m * n)), l=np.zeros((batch, m)), ub=np.zeros((batch, m)),
               x=np.zeros((batch, n)), y=np.zeros((batch, m)), wx=np.zeros((batch, n)), wy=np.zeros((batch, m)), seconds=np.zeros(ticks))
    st = np.ascontiguousarray(states, dtype=np.float64); ud = np.ascontiguousarray(udes, dtype=np.float64)
    fn = dev_lib().sfbx_asif_swarm_device_step_tall if reduced_kkt else dev_lib().sfbx_asif_swarm_device_step
    rc = fn(C.c_int64(batch), K, ticks, _p(st), _p(ud), _p(out["u"]), _p(out["code"]), _p(out["iter"]),
                                               _p(out["P"]), _p(out["q"]), _p(out["A"]), _p(out["l"]), _p(out["ub"]), _p(out["x"]),
                                               _p(out["y"]), _p(out["wx"]), _p(out["wy"]), _p(out["seconds"]))
    assert rc == 0, rc
    return out


def mpc_swarm_devlin_step(variant, K, batch, ticks, seed=1, tf=5.0, probe_empty=False, want_records=True):
    """MPCSwarmDeviceLin (linearisation, assembly and solve on the GPU): the agents and closed loop of mpc_swarm_step;
    also the records of the last tick as the device wrote them."""
    dims = mpc_dims(variant, K)
    Nx, Nu, N = dims["Nx"], dims["Nu"], dims["N"]
    full = N * (2 * Nx + Nx * Nx + Nx * Nu + 2 + 2 * Nx + 2 * Nu) + Nx + Nx * Nx
    out = dict(u0=np.zeros((batch, Nu)), code=np.zeros(batch, np.int32), iter=np.zeros(batch, np.uint32), seconds=np.zeros(ticks))
    rec = np.zeros((batch, full)) if want_records else None
    rd = C.c_int64(0); packed = C.c_int32(0)
    rc = dev_lib().sfbx_mpc_swarm_devlin_step(variant, K, C.c_double(tf), C.c_int64(batch), C.c_uint64(seed), ticks, int(probe_empty),
                                              _p(out["u0"]), _p(out["code"]), _p(out["iter"]), _p(rec) if want_records else None,
                                              C.byref(rd), C.byref(packed), _p(out["seconds"]))
    assert rc == 0, rc
    out["record_doubles"] = rd.value
    out["packed"] = bool(packed.value)
    if want_records:
        out["records"] = rec.reshape(-1)[: batch * rd.value].reshape(batch, rd.value).copy()
    return out


def mpc_swarm_devlin_step_multi(variant, K, batch, ticks, devices, seed=1, tf=5.0, thread_per_shard=False):
    """MPCSwarmMultiDeviceLin (multi_device.hpp): mpc_swarm_devlin_step with the agents sharded over `devices` from this one
    process, one resident swarm per shard."""
    out = dict(u0=np.zeros((batch, mpc_dims(variant, K)["Nu"])), code=np.zeros(batch, np.int32), iter=np.zeros(batch, np.uint32),
               seconds=np.zeros(ticks))
    dev = (C.c_int * len(devices))(*devices)
    rc = dev_lib().sfbx_mpc_swarm_devlin_step_multi(variant, K, C.c_double(tf), C.c_int64(batch), C.c_uint64(seed), ticks, dev, len(devices),
                                                    int(thread_per_shard), _p(out["u0"]), _p(out["code"]), _p(out["iter"]), _p(out["seconds"]))
    assert rc == 0, rc
    return out


def ekf_swarm_device_multi(states, P0, y, devices, tau=0.1, dt=0.0, rk4=False, fused=False, thread_per_shard=False):
    """EKFSwarmMultiDevice (multi_device.hpp): ekf_swarm_device with the filters sharded over `devices`."""
    batch, steps = len(states), len(y)
    out = dict(states=np.zeros((batch, 7)), P=np.zeros((batch, 36)), info=np.zeros(batch, np.int32))
    st = np.ascontiguousarray(states, dtype=np.float64); P0 = np.ascontiguousarray(P0, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
    dev = (C.c_int * len(devices))(*devices)
    rc = dev_lib().sfbx_ekf_swarm_device_multi(C.c_int64(batch), steps, int(rk4), int(fused), C.c_double(tau), C.c_double(dt), dev, len(devices),
                                               int(thread_per_shard), _p(st), _p(P0), _p(y), _p(out["states"]), _p(out["P"]), _p(out["info"]))
    assert rc == 0, rc
    return out


def ekf_swarm_inputs(batch, steps, seed=0):
    """states [batch][7] of asif_swarm_states, SPD covariances, measurements near the states' (x, y, v0)"""
    st, _ = asif_swarm_states(batch, seed)
    rng = np.random.default_rng(seed)
    G = rng.uniform(-1, 1, (batch, 6, 6))
    P0 = (np.eye(6)[None] * 0.5 + G @ G.transpose(0, 2, 1) / 12).reshape(batch, 36)
    y = st[None, :, [0, 1, 4]] + rng.normal(0, 0.2, (steps, batch, 3))
    return st, np.ascontiguousarray(P0), np.ascontiguousarray(y)


def ekf_swarm_device(states, P0, y, tau=0.1, dt=0.0, rk4=False, fused=False):
    """EKFSwarmDevice (ekf_device.hpp): len(y) predict+update rounds of every filter on the GPU."""
    batch, steps = len(states), len(y)
    out = dict(states=np.zeros((batch, 7)), P=np.zeros((batch, 36)), info=np.zeros(batch, np.int32), seconds=np.zeros(steps))
    st = np.ascontiguousarray(states, dtype=np.float64); P0 = np.ascontiguousarray(P0, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
    rc = dev_lib().sfbx_ekf_swarm_device(C.c_int64(batch), steps, int(rk4), int(fused), C.c_double(tau), C.c_double(dt), _p(st), _p(P0),
                                         _p(y), _p(out["states"]), _p(out["P"]), _p(out["info"]), _p(out["seconds"]))
    assert rc == 0, rc
    return out


def ekf_swarm_host(states, P0, y, tau=0.1, dt=0.0, rk4=False):
    """the same through one host EKF<> object per filter"""
    batch, steps = len(states), len(y)
    out = dict(states=np.zeros((batch, 7)), P=np.zeros((batch, 36)))
    st = np.ascontiguousarray(states, dtype=np.float64); P0 = np.ascontiguousarray(P0, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
    rc = lib().sfbx_ekf_swarm_host(C.c_int64(batch), steps, int(rk4), C.c_double(tau), C.c_double(dt), _p(st), _p(P0), _p(y),
                                   _p(out["states"]), _p(out["P"]))
    assert rc == 0, rc
    return out


def pose_ekf_swarm_device(states, P0, y, tau=0.1, dt=0.0, rk4=False, fused=False):
    """EKFSwarmDevice on the pose filter of rigid_body_model.h (G = SE3): states [batch][7] = (px, py, pz, w, x, y, z)"""
    batch, steps = len(states), len(y)
    out = dict(states=np.zeros((batch, 7)), P=np.zeros((batch, 36)), info=np.zeros(batch, np.int32))
    st = np.ascontiguousarray(states, dtype=np.float64); P0 = np.ascontiguousarray(P0, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
    rc = dev_lib().sfbx_pose_ekf_swarm_device(C.c_int64(batch), steps, int(rk4), int(fused), C.c_double(tau), C.c_double(dt), _p(st), _p(P0),
                                              _p(y), _p(out["states"]), _p(out["P"]), _p(out["info"]))
    assert rc == 0, rc
    return out


def pose_ekf_swarm_host(states, P0, y, tau=0.1, dt=0.0, rk4=False):
    """the same through one host EKF<SE3> object per filter"""
    batch, steps = len(states), len(y)
    out = dict(states=np.zeros((batch, 7)), P=np.zeros((batch, 36)))
    st = np.ascontiguousarray(states, dtype=np.float64); P0 = np.ascontiguousarray(P0, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
    rc = lib().sfbx_pose_ekf_swarm_host(C.c_int64(batch), steps, int(rk4), C.c_double(tau), C.c_double(dt), _p(st), _p(P0), _p(y),
                                        _p(out["states"]), _p(out["P"]))
    assert rc == 0, rc
    return out


def asif_rigid_body(b=0):
    """ASIFilter<Bundle<SE3, R6>, R6> on the rigid body, agent b (needs a GPU): filtered input, solver code, smallest row slack"""
    u = np.zeros(6); code = C.c_int32(-1); slack = C.c_double(0.0)
    rc = lib().sfbx_test_asif_rigid_body(C.c_int64(b), _p(u), C.byref(code), C.byref(slack))
    assert rc == 0, rc
    return u, code.value, slack.value


def asif_rigid_body_swarm_device(batch):
    """ASIFSwarmDevice on the same agents: u [batch][6], codes"""
    u = np.zeros((batch, 6)); codes = np.zeros(batch, np.int32)
    rc = dev_lib().sfbx_asif_rigid_body_swarm_device(C.c_int64(batch), _p(u), _p(codes))
    assert rc == 0, rc
    return u, codes


def vehicle_swarm_sim(batch, ticks, K_mpc=30, K_asif=200, seed=0, reduced_kkt=False):
    """examples/mpc_asif_vehicle.cpp's closed loop for a swarm, MPC and ASI filter on the GPU (models_device.hip).
    reduced_kkt: the filter's QPs on the reduced-KKT route for tall problems (ASIFilterParams::reduced_kkt)."""
    out = dict(xy=np.zeros((ticks, batch, 2)), u_mpc=np.zeros((ticks, batch, 2)), u_asif=np.zeros((ticks, batch, 2)),
               mpc_bad=np.zeros(ticks, np.int32), asif_bad=np.zeros(ticks, np.int32), hmin=np.zeros(ticks), seconds=np.zeros((ticks, 2)))
    fn = dev_lib().sfbx_vehicle_swarm_sim_tall if reduced_kkt else dev_lib().sfbx_vehicle_swarm_sim
    rc = fn(C.c_int64(batch), K_mpc, K_asif, ticks, C.c_uint64(seed), _p(out["xy"]), _p(out["u_mpc"]),
                                          _p(out["u_asif"]), _p(out["mpc_bad"]), _p(out["asif_bad"]), _p(out["hmin"]), _p(out["seconds"]))
    assert rc == 0, rc
    return out


def asif_swarm_assemble(batch, K, seed=0):
    """The QPs of asif_swarm_step's first tick, assembled on the host and not solved (no GPU)."""
    n, m = 3, K + 3
    out = dict(P=np.zeros((batch, n * n)), q=np.zeros((batch, n)), A=np.zeros((batch, m * n)), l=np.zeros((batch, m)),
               ub=np.zeros((batch, m)))
    rc = lib().sfbx_asif_swarm_assemble(C.c_int64(batch), C.c_uint64(seed), K, _p(out["P"]), _p(out["q"]), _p(out["A"]), _p(out["l"]),
                                        _p(out["ub"]))
    assert rc == 0, rc
    return out


LIE_GROUPS = dict(R3=0, SE2=1, SO3=2, X6=3, X12=4, SE3=5, X12B=6)
LIE_OPS = dict(exp=0, log=1, mul=2, ad=3, dr_expinv=4, rplus=5, rminus=6, rminus_rplus=7)


def lie_eval_widths(group, op):
    """doubles per item (in, out) of lie_eval, or None when the group has no such operation (examples/lie_eval.h)"""
    win, wout = C.c_int(0), C.c_int(0)
    if lib().sfbx_lie_eval_widths(LIE_GROUPS[group], LIE_OPS[op], C.byref(win), C.byref(wout)) != 0:
        return None
    return win.value, wout.value


def lie_eval(group, op, inp, device=False):
    """The lie.hpp operation `op` of `group` on every row of inp [count][win]: on the host, or (device=True) one GPU thread
    per item running the same functions."""
    win, wout = lie_eval_widths(group, op)
    inp = np.ascontiguousarray(inp, dtype=np.float64).reshape(-1, win)
    out = np.full((len(inp), wout), np.nan)
    fn = dev_lib().sfbx_lie_eval_device if device else lib().sfbx_lie_eval
    rc = fn(LIE_GROUPS[group], LIE_OPS[op], C.c_int64(len(inp)), _p(inp), _p(out))
    assert rc == 0, rc
    return out


PID_GROUPS = dict(R2=0, SE2=1, SO3=2, SE3=3, SE3R3=4, SE2R1=5)
PID_PARTS = dict(R2=[("RN", 2)], SE2=[("SE2", 3)], SO3=[("SO3", 3)], SE3=[("SE3", 6)], SE3R3=[("SE3", 6), ("RN", 3)], SE2R1=[("SE2", 3), ("RN", 1)])


def test_pid_api():
    """PID<T, G> under the reference's include path (models.h): (ok, [|u|^2 at the target x 3, trajectory check])"""
    out = np.zeros(4)
    rc = lib().sfbx_test_pid_api(_p(out))
    return rc == 0, out


def pid_host(group, times, x, v, gd, vd, ad, kp, kd, ki, windup=np.inf):
    """one host PID<double, G> per agent, called at `times`: x, gd [B][ncalls][elem]; v, vd, ad [B][ncalls][dof]; gains
    [B][dof].  Returns u and the integral state after each call, [B][ncalls][dof]."""
    times = np.ascontiguousarray(times, dtype=np.float64)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, v, gd, vd, ad, kp, kd, ki)]
    B, n = arrs[0].shape[0], len(times)
    D = arrs[5].shape[1]
    assert all(a.shape[:2] == (B, n) for a in arrs[:5]) and all(a.shape == (B, D) for a in arrs[5:])
    u = np.zeros((B, n, D)); ie = np.zeros((B, n, D))
    rc = lib().sfbx_pid_host(PID_GROUPS[group], C.c_int64(B), n, _p(times), *[_p(a) for a in arrs], C.c_double(windup), _p(u), _p(ie))
    assert rc == 0, rc
    return u, ie


def pid_rollout_host(group, t0, dt, steps, x, v, g0, w, kp, kd, ki, ie, t_last, windup=np.inf, u_max=None):
    """pid_rollout (pid.hpp) on the CPU for every agent; arrays as smooth_feedback_amd.pid_rollout_batch_host, same dict back"""
    x, v, ie, t_last = [np.array(a, dtype=np.float64, order="C") for a in (x, v, ie, t_last)]
    g0, w, kp, kd, ki = [np.ascontiguousarray(a, dtype=np.float64) for a in (g0, w, kp, kd, ki)]
    um = None if u_max is None else np.ascontiguousarray(u_max, dtype=np.float64)
    B = len(x)
    u = np.zeros_like(v); cost = np.zeros(B)
    rc = lib().sfbx_pid_rollout_host(PID_GROUPS[group], C.c_int64(B), C.c_double(t0), C.c_double(dt), C.c_int64(steps), _p(x), _p(v), _p(g0), _p(w),
                                     _p(kp), _p(kd), _p(ki), C.c_double(windup), None if um is None else _p(um), _p(ie), _p(t_last), _p(u), _p(cost))
    assert rc == 0, rc
    return dict(x=x, v=v, i_err=ie, t_last=t_last, u_last=u, cost=cost)


def test_pid_spline_api():
    """PID::set_xdes(t0, spline) under the reference's include paths (models.h): (ok, [worst relative error, least motion])"""
    out = np.zeros(2)
    rc = lib().sfbx_test_pid_spline_api(_p(out))
    return rc == 0, out


def lie_Ad(group, g, a):
    """Ad_g a of lie.hpp on the host: g [n][elem], a [n][dof] -> [n][dof]"""
    g, a = np.ascontiguousarray(g, dtype=np.float64), np.ascontiguousarray(a, dtype=np.float64)
    out = np.zeros_like(a)
    rc = lib().sfbx_lie_Ad(PID_GROUPS[group], C.c_int64(len(g)), _p(g), _p(a), _p(out))
    assert rc == 0, rc
    return out


def spline_fit_host(group, tk, gk):
    """fit_spline_cubic per agent: tk [B][S+1], gk [B][S+1][elem] -> V [B][S][3][dof]"""
    tk, gk = np.ascontiguousarray(tk, dtype=np.float64), np.ascontiguousarray(gk, dtype=np.float64)
    B, K = tk.shape
    D = sum(d for _, d in PID_PARTS[group])
    V = np.zeros((B, K - 1, 3, D))
    rc = lib().sfbx_spline_fit_host(PID_GROUPS[group], C.c_int64(B), C.c_int64(K), _p(tk), _p(gk), _p(V))
    assert rc == 0, rc
    return V


def spline_eval_host(group, tk, gk, V, t):
    """Spline<K, G>::operator() per agent (K = V.shape[2], 2 or 3): t [B][nt] -> g [B][nt][elem], vel, acc [B][nt][dof]"""
    tk, gk, V, t = [np.ascontiguousarray(a, dtype=np.float64) for a in (tk, gk, V, t)]
    B, K = tk.shape
    nt, E, D = t.shape[1], gk.shape[2], V.shape[3]
    g, vel, acc = np.zeros((B, nt, E)), np.zeros((B, nt, D)), np.zeros((B, nt, D))
    rc = lib().sfbx_spline_eval_host(PID_GROUPS[group], int(V.shape[2]), C.c_int64(B), C.c_int64(K), _p(tk), _p(gk), _p(V), C.c_int64(nt), _p(t),
                                     _p(g), _p(vel), _p(acc))
    assert rc == 0, rc
    return g, vel, acc


def pid_rollout_spline_host(group, t0, dt, steps, x, v, tk, gk, V, kp, kd, ki, ie, t_last, ts0=None, windup=np.inf, u_max=None):
    """pid_rollout (pid.hpp) along Spline<3, G> on the CPU; arrays as smooth_feedback_amd.pid_rollout_spline_batch_host (per agent)"""
    x, v, ie, t_last = [np.array(a, dtype=np.float64, order="C") for a in (x, v, ie, t_last)]
    tk, gk, V, kp, kd, ki = [np.ascontiguousarray(a, dtype=np.float64) for a in (tk, gk, V, kp, kd, ki)]
    um = None if u_max is None else np.ascontiguousarray(u_max, dtype=np.float64)
    ts = None if ts0 is None else np.ascontiguousarray(ts0, dtype=np.float64)
    B = len(x)
    u = np.zeros_like(v); cost = np.zeros(B)
    rc = lib().sfbx_pid_rollout_spline_host(PID_GROUPS[group], C.c_int64(B), C.c_double(t0), C.c_double(dt), C.c_int64(steps), _p(x), _p(v),
                                            C.c_int64(tk.shape[1]), _p(tk), _p(gk), _p(V), None if ts is None else _p(ts), _p(kp), _p(kd), _p(ki),
                                            C.c_double(windup), None if um is None else _p(um), _p(ie), _p(t_last), _p(u), _p(cost))
    assert rc == 0, rc
    return dict(x=x, v=v, i_err=ie, t_last=t_last, u_last=u, cost=cost)


def pid_swarm_device(t0, dt, steps, x, v, ie, t_last, kp, kd, ki, g0, w, kind, windup=np.inf, u_max=None):
    """PIDSwarmDevice<SE3, functor> (pid_device.hpp, models_device.hip): rollout(t0, dt, steps), or one step(t0) for steps == 0,
    of agents tracking rplus(g0, t w) (kind 0) or a twist of changing size along w (kind 1).  Returns dict x, v, ie, u, cost."""
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, v, ie, t_last, kp, kd, ki, g0, w)]
    B = len(arrs[0])
    kind = np.ascontiguousarray(kind, dtype=np.int32)
    um = None if u_max is None else np.ascontiguousarray(u_max, dtype=np.float64)
    out = dict(x=np.zeros((B, 7)), v=np.zeros((B, 6)), ie=np.zeros((B, 6)), u=np.zeros((B, 6)), cost=np.zeros(B))
    rc = dev_lib().sfbx_pid_swarm_device(C.c_int64(B), C.c_double(t0), C.c_double(dt), C.c_int64(steps), *[_p(a) for a in arrs], _p(kind),
                                         C.c_double(windup), None if um is None else _p(um), *[_p(out[k]) for k in ("x", "v", "ie", "u", "cost")])
    assert rc == 0, rc
    return out


def pid_swarm_spline_device(t0, dt, steps, x, v, ie, t_last, kp, kd, ki, tk, gk, V, ts0=None, windup=np.inf, u_max=None):
    """PIDSwarmDevice<SE3, SplineTrajectory<3, SE3>> (pid_device.hpp, spline.hpp, models_device.hip): rollout(t0, dt, steps) of
    agents following their splines (tk [B][S+1], gk [B][S+1][7], V [B][S][3][6]) or ONE spline (no batch axis) at t - ts0.
    Returns dict x, v, ie, u, cost."""
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, v, ie, t_last, kp, kd, ki)]
    tk, gk, V = [np.ascontiguousarray(a, dtype=np.float64) for a in (tk, gk, V)]
    B = len(arrs[0])
    um = None if u_max is None else np.ascontiguousarray(u_max, dtype=np.float64)
    ts = None if ts0 is None else np.ascontiguousarray(ts0, dtype=np.float64)
    out = dict(x=np.zeros((B, 7)), v=np.zeros((B, 6)), ie=np.zeros((B, 6)), u=np.zeros((B, 6)), cost=np.zeros(B))
    rc = dev_lib().sfbx_pid_swarm_spline_device(C.c_int64(B), C.c_double(t0), C.c_double(dt), C.c_int64(steps), *[_p(a) for a in arrs],
                                                C.c_int64(tk.shape[-1]), _p(tk), _p(gk), _p(V), int(tk.ndim == 1), None if ts is None else _p(ts),
                                                C.c_double(windup), None if um is None else _p(um), *[_p(out[k]) for k in ("x", "v", "ie", "u", "cost")])
    assert rc == 0, rc
    return out


# ---- collocation layer (examples/collocation.cpp)
def _script_args(spec, ops, opdata):
    ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 3)
    opdata = np.ascontiguousarray(opdata if opdata is not None else [], dtype=np.float64)
    kmin, kmax, n, k = [int(v) for v in spec]
    return (kmin, kmax, n, k, len(ops), _p(ops), _p(opdata)), (ops, opdata)


def mesh_script(spec, ops=(), opdata=None, t=(), vals=None, p=0, extend=True, cap_ivals=256):
    """Mesh<kmin, kmax>(n, k) (spec = kmin, kmax, n, k) after the op script (sfbx_mesh_script): dict K, tau0, nodes, weights,
    diffmat / intmat (lists of per-interval matrices), and with times t and node values vals (N (+1), dim): eval (nt, dim),
    found (nt,).  Raises LookupError for an instantiation the harness does not carry."""
    args, keep = _script_args(spec, ops, opdata)
    kcap = int(spec[1]) + 1
    nivals = C.c_int32()
    K = np.zeros(cap_ivals, np.int32); tau0 = np.zeros(cap_ivals)
    nodes = np.zeros(cap_ivals * kcap + 1); weights = np.zeros_like(nodes)
    D = np.zeros(cap_ivals * (kcap + 1) * kcap); I = np.zeros(cap_ivals * kcap * kcap)
    t = np.ascontiguousarray(t, dtype=np.float64)
    vals = np.ascontiguousarray(vals if vals is not None else np.zeros((cap_ivals * kcap + 1, 1)), dtype=np.float64)
    ev = np.zeros((len(t), vals.shape[1])); found = np.zeros(len(t), np.int32)
    rc = lib().sfbx_mesh_script(*args, cap_ivals, C.byref(nivals), _p(K), _p(tau0), _p(nodes), _p(weights), _p(D), _p(I), len(t), _p(t),
                                vals.shape[1], _p(vals), int(p), 1 if extend else 0, _p(ev), _p(found))
    if rc == -1:
        raise LookupError("no Mesh<%d, %d> in the harness" % (spec[0], spec[1]))
    assert rc == 0, rc
    n = nivals.value
    K = K[:n].copy()
    N = int(K.sum())
    dm, im, a, b = [], [], 0, 0
    for k in K:
        dm.append(D[a:a + (k + 1) * k].reshape(k + 1, k)); a += (k + 1) * k
        im.append(I[b:b + k * k].reshape(k, k)); b += k * k
    return {"K": K, "tau0": tau0[:n].copy(), "nodes": nodes[:N + 1].copy(), "weights": weights[:N + 1].copy(), "diffmat": dm, "intmat": im,
            "eval": ev, "found": found}


def mesh_dyn_error_host(spec, ops, opdata, fid, coef, t0, tf, vals_x, vals_u):
    """mesh_dyn_error on the script's mesh raised by one degree, for the built-in dynamics `fid` (sfbx_mesh_dyn_error_host)."""
    args, keep = _script_args(spec, ops, opdata)
    vals_x = np.ascontiguousarray(vals_x, dtype=np.float64); vals_u = np.ascontiguousarray(vals_u, dtype=np.float64)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    errs = np.full(4096, np.nan)
    rc = lib().sfbx_mesh_dyn_error_host(*args, int(fid), _p(coef), vals_x.shape[1], vals_u.shape[1], C.c_double(t0), C.c_double(tf), _p(vals_x),
                                        _p(vals_u), _p(errs))
    assert rc == 0, rc
    return errs[~np.isnan(errs)]


def flat_dynamics_host(model, xl, dxl, ul, e, v):
    """flat_dynamics of model 0 (vehicle) / 1 (rigid body), row by row (sfbx_flat_dynamics_host)."""
    xl, dxl, ul, e, v = [np.ascontiguousarray(a, dtype=np.float64) for a in (xl, dxl, ul, e, v)]
    out = np.zeros_like(e)
    assert lib().sfbx_flat_dynamics_host(int(model), len(e), _p(xl), _p(dxl), _p(ul), _p(e), _p(v), _p(out)) == 0
    return out


def mpc_dyn_error_host(variant, K, tf, t, primal):
    """MPC::dyn_error of the host front for given primals (B, n) at times t (B,) -> (B, ceil(K / 4)) (sfbx_mpc_dyn_error_host)."""
    primal = np.ascontiguousarray(np.atleast_2d(primal), dtype=np.float64)
    B = len(primal)
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (B,)))
    errs = np.zeros((B, -(-K // 4)))
    assert primal.shape[1] == mpc_dims(variant, K)["n"], primal.shape
    assert lib().sfbx_mpc_dyn_error_host(variant, K, C.c_double(tf), C.c_int64(B), _p(t), _p(primal), _p(errs)) == 0
    return errs


def mpc_tick_dyn_error_host(variant, K, tf, t, dx0):
    """one tick of the host front from xdes(t) (+) dx0, then MPC::dyn_error(t) of its plan -> (errs, status code)."""
    x = np.ascontiguousarray(dx0, dtype=np.float64)
    errs, code = np.zeros(-(-K // 4)), C.c_int32()
    rc = lib().sfbx_mpc_tick_dyn_error_host(variant, K, C.c_double(tf), C.c_double(t), _p(x), _p(errs), C.byref(code))
    assert rc == 0, rc
    return errs, code.value


def mpc_audit_device(variant, K, tf, t, primal, code=None):
    """the fused audit kernel of mesh_device.hpp on given plans (B, n) (sfbx_mpc_audit_device) -> dict errs (B, nivals),
    agent_max (B,), ival_max (nivals,), skipped."""
    primal = np.ascontiguousarray(np.atleast_2d(primal), dtype=np.float64)
    B, nivals = len(primal), -(-K // 4)
    assert primal.shape[1] == mpc_dims(variant, K)["n"], primal.shape
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (B,)))
    code = None if code is None else np.ascontiguousarray(code, dtype=np.int32)
    errs, amax, imax, skipped = np.zeros((B, nivals)), np.zeros(B), np.zeros(nivals), C.c_int32(-1)
    rc = dev_lib().sfbx_mpc_audit_device(variant, K, C.c_double(tf), C.c_int64(B), _p(t), _p(primal), _p(code) if code is not None else None,
                                         _p(errs), _p(amax), _p(imax), C.byref(skipped))
    assert rc == 0, rc
    return {"errs": errs, "agent_max": amax, "ival_max": imax, "skipped": skipped.value}


def mpc_swarm_devlin_audit(variant, K, tf, t, dx0, audit=True, target=1e-3):
    """one tick of MPCSwarmDeviceLin from xdes(t[b]) (+) dx0[b], optionally its audit(), then the same tick again
    (sfbx_mpc_swarm_devlin_audit) -> dict primal (B, n), code, u_next (B, Nu), and with audit: errs (B, nivals), agent_max,
    ival_max, skipped, refined_ivals, audit_seconds (a second, warmed audit() call, wall clock), audit_kernel_seconds (its two launches between device
    events, least of five); tick_seconds is the second tick (wall clock)."""
    dx0 = np.ascontiguousarray(dx0, dtype=np.float64)
    B, nivals, d = len(dx0), -(-K // 4), mpc_dims(variant, K)
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (B,)))
    primal, code, u_next = np.zeros((B, d["n"])), np.zeros(B, np.int32), np.zeros((B, d["Nu"]))
    errs, amax, imax, skipped, refined = np.zeros((B, nivals)), np.zeros(B), np.zeros(nivals), C.c_int32(-1), C.c_int32(-1)
    seconds = np.zeros(3)
    rc = dev_lib().sfbx_mpc_swarm_devlin_audit(variant, K, C.c_double(tf), C.c_int64(B), _p(t), _p(dx0), 1 if audit else 0, C.c_double(target),
                                               _p(primal), _p(code), _p(errs), _p(amax), _p(imax), C.byref(skipped), C.byref(refined), _p(u_next), _p(seconds))
    assert rc == 0, rc
    out = {"primal": primal, "code": code, "u_next": u_next, "tick_seconds": seconds[0]}
    if audit:
        out.update(audit_seconds=seconds[1], audit_kernel_seconds=seconds[2], errs=errs, agent_max=amax, ival_max=imax, skipped=skipped.value, refined_ivals=refined.value)
    return out


def test_collocation_api():
    return lib().sfbx_test_collocation_api()


MESHFN = {"eval": 0, "integrate": 1, "dyn": 2}
MESHFN_SHAPES = {(3, 2, 3): 0, (3, 2, 1): 1, (1, 0, 1): 2, (12, 2, 12): 3, "vehicle": 4, "table": 5}


def meshfn_host(spec, ops, opdata, fn, deriv, shape, terms, coef, t0, tf, xs, us, scale=False, lam=None, numerical=False, calls=1):
    """mesh_eval / mesh_integrate / mesh_dyn (fn: a key of MESHFN) of the host front at order deriv on the script's mesh
    (sfbx_meshfn_host); shape: a key of MESHFN_SHAPES, (nx, nu, nf) of an integrand given as a term table (terms (nterms, 5),
    coef (nterms,)) or "vehicle".  xs (N + 1, ..), us (N, nu).  Returns dict F, stable, and with deriv >= 1 rowptr, colind, val,
    cols (dF as CSR), with deriv 2 colptr2, rowind2, val2 (d2F, upper triangle, CSC).  LookupError for a shape or
    (fn, deriv) the harness does not carry."""
    args, keep = _script_args(spec, ops, opdata)
    xs = np.ascontiguousarray(xs, dtype=np.float64); us = np.ascontiguousarray(us, dtype=np.float64)
    terms = np.ascontiguousarray(terms, dtype=np.int32).reshape(-1, 5); coef = np.ascontiguousarray(coef, dtype=np.float64)
    N = len(xs) - 1
    if shape in ("vehicle", "table"):    # "table": coef (N, 6 * 10), node by node the values and the Jacobian row-major
        nx, nu, nf = 6, 2, 6
    else:
        nx, nu, nf = shape
    nv = 2 + nx * (N + 1) + nu * N
    rows_cap = N * nf
    nnz_cap = max(rows_cap * (2 + 17 + nx + nu), nf * nv)
    lam = np.ascontiguousarray(lam if lam is not None else np.zeros(rows_cap), dtype=np.float64)
    dims = np.zeros(5, np.int32)
    F = np.zeros(rows_cap); rowptr = np.zeros(rows_cap + 1, np.int32); colind = np.zeros(nnz_cap, np.int32); val = np.zeros(nnz_cap)
    colptr2 = np.zeros(nv + 1, np.int32); rowind2 = np.zeros(nv * (3 + nx + nu), np.int32); val2 = np.zeros(nv * (3 + nx + nu))
    rc = lib().sfbx_meshfn_host(*args, MESHFN[fn], int(deriv), 1 if numerical else 0, MESHFN_SHAPES[shape], len(terms), _p(terms), _p(coef),
                                C.c_double(t0), C.c_double(tf), _p(xs), _p(us), 1 if scale else 0, _p(lam), int(calls), _p(dims), _p(F),
                                _p(rowptr), _p(colind), _p(val), _p(colptr2), _p(rowind2), _p(val2))
    if rc in (-1, -5, -6):
        raise LookupError("sfbx_meshfn_host: %d" % rc)
    assert rc == 0, rc
    rows, cols, nnz, nnz2, stable = [int(v) for v in dims]
    out = {"F": F[:rows].copy(), "stable": bool(stable)}
    if deriv >= 1:
        out.update(rowptr=rowptr[:rows + 1].copy(), colind=colind[:nnz].copy(), val=val[:nnz].copy(), cols=cols)
    if deriv >= 2:
        out.update(colptr2=colptr2[:cols + 1].copy(), rowind2=rowind2[:nnz2].copy(), val2=val2[:nnz2].copy())
    return out


def test_mesh_function_api():
    return lib().sfbx_test_mesh_function_api()


def ocp_nlp_host(spec, ops, dims, tables, bounds, x, lam=None, order=1, numerical=False, calls=1):
    """detail::OCPNLP of ocp_to_nlp.hpp on the script's mesh for a problem given as three-factor term tables (sfbx_ocp_nlp_host):
    tables maps "terms.f" / "coef.f" (and g, cr, theta, ce) to (nterms, 7) rows and coefficients, bounds = (crl, cru, cel, ceu).
    Orders 0 .. order at x (n,) and lam (m,), `calls` times.  Returns dict n, m, stable, f, g, xl, xu, gl, gu, w_scaling, x_back,
    lambda_back (nlpsol_to_ocpsol, then ocpsol_to_nlpsol), with order >= 1 df (n,), rowptr, colind, dg, with order 2 hcolptr,
    hrowind, d2f, d2g.  LookupError for a (mesh type, dims) the harness does not carry."""
    args, keep = _script_args(spec, ops, None)
    dims = np.ascontiguousarray(dims, dtype=np.int32)
    nx, nu, nq, ncr, nce = [int(v) for v in dims]
    names = ("f", "g", "cr", "theta", "ce")
    nterms = np.array([len(tables["coef." + k]) for k in names], dtype=np.int32)
    terms = np.ascontiguousarray(np.concatenate([np.asarray(tables["terms." + k], dtype=np.int32).reshape(-1, 7) for k in names]), dtype=np.int32)
    coef = np.ascontiguousarray(np.concatenate([np.asarray(tables["coef." + k], dtype=np.float64) for k in names]))
    crl, cru, cel, ceu = [np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.float64).ravel(), [0.0]])) for b in bounds]
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    N = (n - 1 - nq - nx) // (nx + nu)
    m = nx * N + nq + ncr * N + nce
    lam = np.ascontiguousarray(lam if lam is not None else np.zeros(m), dtype=np.float64)
    nnz_cap = m * (2 + 14 + nx + nu) + nq * (nx + nu) * N + nce * (1 + nq + 2 * nx)
    h_cap = n * (2 + nx + nu + nq + 2 * nx)
    sizes = np.zeros(5, np.int32)
    f, ws = np.zeros(1), np.zeros(1)
    df, g, xl, xu, gl, gu, xb, lb = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(n), np.zeros(m), np.zeros(m), np.zeros(n), np.zeros(m)
    rowptr, colind, dg = np.zeros(m + 1, np.int32), np.zeros(nnz_cap, np.int32), np.zeros(nnz_cap)
    hcolptr, hrowind, d2f, d2g = np.zeros(n + 1, np.int32), np.zeros(h_cap, np.int32), np.zeros(h_cap), np.zeros(h_cap)
    rc = lib().sfbx_ocp_nlp_host(*args[:6], _p(dims), _p(nterms), _p(terms), _p(coef), _p(crl), _p(cru), _p(cel), _p(ceu), _p(x), _p(lam), int(order),
                                 1 if numerical else 0, int(calls), _p(sizes), _p(f), _p(df), _p(g), _p(rowptr), _p(colind), _p(dg), _p(hcolptr),
                                 _p(hrowind), _p(d2f), _p(d2g), _p(xl), _p(xu), _p(gl), _p(gu), _p(ws), _p(xb), _p(lb))
    if rc == -1:
        raise LookupError("sfbx_ocp_nlp_host: %d" % rc)
    assert rc == 0, rc
    assert (int(sizes[0]), int(sizes[1])) == (n, m), (sizes, n, m)
    nnz, hnnz = int(sizes[2]), int(sizes[3])
    out = {"n": n, "m": m, "stable": bool(sizes[4]), "f": float(f[0]), "g": g, "xl": xl, "xu": xu, "gl": gl, "gu": gu, "w_scaling": float(ws[0]),
           "x_back": xb, "lambda_back": lb}
    if order >= 1:
        out.update(df=df, rowptr=rowptr, colind=colind[:nnz].copy(), dg=dg[:nnz].copy())
    if order >= 2:
        out.update(hcolptr=hcolptr, hrowind=hrowind[:hnnz].copy(), d2f=d2f[:hnnz].copy(), d2g=d2g[:hnnz].copy())
    return out


def ocp_nlp_hess_host(spec, ops, dims, tables, bounds, x, lam, sigma, numerical=False, calls=1):
    """OCPNLP::d2l_dx2(x, sigma, lam) of ocp_to_nlp.hpp on the script's mesh for a problem given as term tables, as ocp_nlp_host takes
    it (sfbx_ocp_nlp_hess_host).  Returns dict n, m, stable, d2l (nnzH,), hcolptr, hrowind (the member's pattern) and hcolptr2, hrowind2
    (meshfn::ocp_nlp_hess_pattern from the mesh's interval sizes).  LookupError for a (mesh type, dims) the harness does not carry."""
    args, keep = _script_args(spec, ops, None)
    dims = np.ascontiguousarray(dims, dtype=np.int32)
    nx, nu, nq, ncr, nce = [int(v) for v in dims]
    names = ("f", "g", "cr", "theta", "ce")
    nterms = np.array([len(tables["coef." + k]) for k in names], dtype=np.int32)
    terms = np.ascontiguousarray(np.concatenate([np.asarray(tables["terms." + k], dtype=np.int32).reshape(-1, 7) for k in names]), dtype=np.int32)
    coef = np.ascontiguousarray(np.concatenate([np.asarray(tables["coef." + k], dtype=np.float64) for k in names]))
    crl, cru, cel, ceu = [np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.float64).ravel(), [0.0]])) for b in bounds]
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    N = (n - 1 - nq - nx) // (nx + nu)
    m = nx * N + nq + ncr * N + nce
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    assert lam.shape == (m,), (lam.shape, m)
    h_cap = n * (2 + nx + nu + nq + 2 * nx)
    sizes = np.zeros(4, np.int32)
    hcolptr, hrowind, hcolptr2, hrowind2, d2l = np.zeros(n + 1, np.int32), np.zeros(h_cap, np.int32), np.zeros(n + 1, np.int32), np.zeros(h_cap, np.int32), np.zeros(h_cap)
    rc = lib().sfbx_ocp_nlp_hess_host(*args[:6], _p(dims), _p(nterms), _p(terms), _p(coef), _p(crl), _p(cru), _p(cel), _p(ceu), _p(x), _p(lam),
                                      C.c_double(float(sigma)), 1 if numerical else 0, int(calls), _p(sizes), _p(hcolptr), _p(hrowind), _p(hcolptr2),
                                      _p(hrowind2), _p(d2l))
    if rc == -1:
        raise LookupError("sfbx_ocp_nlp_hess_host: %d" % rc)
    assert rc == 0, rc
    assert (int(sizes[0]), int(sizes[1])) == (n, m), (sizes, n, m)
    hnnz = int(sizes[2])
    return {"n": n, "m": m, "stable": bool(sizes[3]), "d2l": d2l[:hnnz].copy(), "hcolptr": hcolptr, "hrowind": hrowind[:hnnz].copy(),
            "hcolptr2": hcolptr2, "hrowind2": hrowind2[:hnnz].copy()}


def test_ocp_to_nlp_api():
    return lib().sfbx_test_ocp_to_nlp_api()


# ---- flatten_ocp (include/smooth_feedback_amd/ocp_flatten.hpp; examples/flat_ocp_harness.h) ----
FLAT_GROUPS = dict(SE2=(1, 3), SO3=(2, 3), SE3=(5, 6), X12B=(6, 12), X5=(7, 5))
FLAT_PROBLEMS = dict(se2=0, se3=1)
FLAT_NODE_KEYS = ("Ff", "dFf", "Fg", "dFg", "Fcr", "dFcr", "ce", "dce", "theta", "dtheta")


def flat_lie_eval(group, op, a, w=None, device=False):
    """op "dr_exp": dr_exp(a) per row of a [count][T]; op "d_expinv": d/de (dr_expinv(e) w) at e = a.  Returns [count][T][T]
    (row, column).  device=True: one GPU thread per item runs the same item function."""
    gid, T = FLAT_GROUPS[group]
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, T)
    inp = a if op == "dr_exp" else np.ascontiguousarray(np.concatenate([a, np.asarray(w, dtype=np.float64).reshape(-1, T)], axis=1))
    out = np.full((len(a), T * T), np.nan)
    fn = dev_lib().sfbx_flat_lie_eval_device if device else lib().sfbx_flat_lie_eval
    rc = fn(gid, 0 if op == "dr_exp" else 1, C.c_int64(len(a)), _p(inp), _p(out))
    assert rc == 0, rc
    return out.reshape(len(a), T, T).transpose(0, 2, 1)


def flat_ocp_sizes(problem, N):
    """dict nx, nu, nq, ncr, nce, row (doubles per trajectory row), n (NLP variables on N nodes), nz, ne"""
    v = np.zeros(7, np.int32)
    assert lib().sfbx_flat_ocp_sizes(FLAT_PROBLEMS[problem], N, _p(v)) == 0
    d = dict(zip(("nx", "nu", "nq", "ncr", "nce", "row", "n"), [int(k) for k in v]))
    d["nz"], d["ne"] = 1 + d["nx"] + d["nu"], 1 + 2 * d["nx"] + d["nq"]
    return d


def _flat_node_arrays(d, B, N):
    nz, ne = d["nz"], d["ne"]
    return dict(Ff=np.full((B, N, d["nx"]), np.nan), dFf=np.full((B, N, d["nx"], nz), np.nan), Fg=np.full((B, N, d["nq"]), np.nan),
                dFg=np.full((B, N, d["nq"], nz), np.nan), Fcr=np.full((B, N, d["ncr"]), np.nan), dFcr=np.full((B, N, d["ncr"], nz), np.nan),
                ce=np.full((B, d["nce"]), np.nan), dce=np.full((B, d["nce"], ne), np.nan), theta=np.full(B, np.nan), dtheta=np.full((B, ne), np.nan))


def flat_ocp_nodes(problem, tau, x, traj, device=False, threads=1):
    """The flattened problem at the nodes tau [N] for agents x [B][n], traj [B][row]: dict of the arrays sfb_ocp_nlp_batch takes
    (Ff [B][N][nx], dFf [B][N][nx][nz], ..., ce, dce) and theta [B], dtheta [B][ne].  Host front, or (device=True)
    flat_ocp_nodes_kernel of ocp_flatten_device.hpp."""
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    N = len(tau)
    d = flat_ocp_sizes(problem, N)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, d["n"])
    traj = np.ascontiguousarray(traj, dtype=np.float64).reshape(len(x), d["row"])
    out = _flat_node_arrays(d, len(x), N)
    ptrs = [_p(out[k]) for k in FLAT_NODE_KEYS]
    if device:
        rc = dev_lib().sfbx_flat_ocp_nodes_device(FLAT_PROBLEMS[problem], C.c_int64(len(x)), N, _p(tau), _p(x), _p(traj), *ptrs)
    else:
        rc = lib().sfbx_flat_ocp_nodes_host(FLAT_PROBLEMS[problem], C.c_int64(len(x)), N, _p(tau), _p(x), _p(traj), *ptrs, threads)
    assert rc == 0, rc
    return out


def flat_ocp_mesh(problem, mesh_kind=0):
    """dict n, m, nnz, N, taus [N + 1] of the harness mesh (0: two intervals with K = (3, 5); 1: 13 intervals of 4)"""
    sizes = np.zeros(4, np.int32); taus = np.zeros(128)
    assert lib().sfbx_flat_ocp_nlp_host(FLAT_PROBLEMS[problem], mesh_kind, C.c_int64(1), None, None, None, None, None, None, None, _p(sizes), _p(taus)) == 0
    n, m, nnz, N = [int(v) for v in sizes]
    return dict(n=n, m=m, nnz=nnz, N=N, taus=taus[:N + 1].copy())


def flat_ocp_nlp_host(problem, x, traj, mesh_kind=0):
    """ocp_to_nlp(flatten_ocp(...), mesh) per agent on the host: dict g [B][m], dg [B][nnz], f [B], df [B][ne], differing [B]
    (doubles of g, dg not bit-identical to meshfn::ocp_nlp_assemble over the host node arrays)."""
    s = flat_ocp_mesh(problem, mesh_kind)
    d = flat_ocp_sizes(problem, s["N"])
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, s["n"])
    B = len(x)
    traj = np.ascontiguousarray(traj, dtype=np.float64).reshape(B, d["row"])
    out = dict(g=np.full((B, s["m"]), np.nan), dg=np.full((B, s["nnz"]), np.nan), f=np.full(B, np.nan), df=np.full((B, d["ne"]), np.nan),
               differing=np.full(B, -1, np.int64))
    rc = lib().sfbx_flat_ocp_nlp_host(FLAT_PROBLEMS[problem], mesh_kind, C.c_int64(B), _p(x), _p(traj), _p(out["g"]), _p(out["dg"]), _p(out["f"]),
                                      _p(out["df"]), _p(out["differing"]), None, None)
    assert rc == 0, rc
    return out


def flat_ocp_front_device(problem, x, traj, mesh_kind=0, side=False, reps=0):
    """FlatOCPSwarmDevice::eval on the GPU (sfbx_flat_ocp_front_device): dict g, dg, f, df, the front's node arrays (Ff .. dce),
    info (free device memory before and after a further eval, the front's bytes, n); side=True adds g2, dg2, f2, df2 of a run
    on a non-blocking stream behind pending work; reps > 0 adds seconds (node kernel, sfb_ocp_nlp_batch)."""
    s = flat_ocp_mesh(problem, mesh_kind)
    d = flat_ocp_sizes(problem, s["N"])
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, s["n"])
    B = len(x)
    traj = np.ascontiguousarray(traj, dtype=np.float64).reshape(B, d["row"])
    out = dict(g=np.full((B, s["m"]), np.nan), dg=np.full((B, s["nnz"]), np.nan), f=np.full(B, np.nan), df=np.full((B, d["ne"]), np.nan),
               info=np.zeros(4, np.int64), seconds=np.zeros(2))
    nodes = _flat_node_arrays(d, B, s["N"])
    out.update({k: nodes[k] for k in FLAT_NODE_KEYS[:8]})
    node_ptrs = (C.c_void_p * 8)(*[nodes[k].ctypes.data for k in FLAT_NODE_KEYS[:8]])
    second = [None] * 4
    if side:
        for k in ("g", "dg", "f", "df"):
            out[k + "2"] = np.full_like(out[k], np.nan)
        second = [_p(out[k + "2"]) for k in ("g", "dg", "f", "df")]
    rc = dev_lib().sfbx_flat_ocp_front_device(FLAT_PROBLEMS[problem], mesh_kind, C.c_int64(B), _p(x), _p(traj), int(side), int(reps), _p(out["g"]),
                                              _p(out["dg"]), _p(out["f"]), _p(out["df"]), node_ptrs, *second, _p(out["info"]), _p(out["seconds"]))
    assert rc == 0, rc
    return out


FLAT_HESS_KEYS = ("HLf", "HLg", "HLcr", "d2theta", "d2ce_l")


def _flat_hess_arrays(d, B, N):
    nz, ne = d["nz"], d["ne"]
    return dict(HLf=np.full((B, N, nz, nz), np.nan), HLg=np.full((B, N, nz, nz), np.nan), HLcr=np.full((B, N, nz, nz), np.nan),
                d2theta=np.full((B, ne, ne), np.nan), d2ce_l=np.full((B, ne, ne), np.nan))


def flat_ocp_hess_nodes(problem, tau, x, lam, traj, threads=1):
    """The multiplier-contracted Hessians of the flattened problem at the nodes tau [N], the arrays sfb_ocp_nlp_hess_batch takes:
    dict HLf, HLg, HLcr [B][N][nz][nz], d2theta, d2ce_l [B][ne][ne] (full squares) for x [B][n], lam [B][N nx + nq + N ncr + nce],
    traj [B][row].  Host loop over the law of ocp_flatten.hpp."""
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    N = len(tau)
    d = flat_ocp_sizes(problem, N)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, d["n"])
    B = len(x)
    lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(B, N * d["nx"] + d["nq"] + N * d["ncr"] + d["nce"])
    traj = np.ascontiguousarray(traj, dtype=np.float64).reshape(B, d["row"])
    out = _flat_hess_arrays(d, B, N)
    ptrs = [_p(out[k]) for k in FLAT_HESS_KEYS]
    rc = lib().sfbx_flat_ocp_hess_nodes_host(FLAT_PROBLEMS[problem], C.c_int64(B), N, _p(tau), _p(x), _p(lam), _p(traj), *ptrs, threads)
    assert rc == 0, rc
    return out


def flat_ocp_nnz_hess(problem, mesh_kind=0):
    nnz = np.zeros(1, np.int64)
    assert lib().sfbx_flat_ocp_hess_host(FLAT_PROBLEMS[problem], mesh_kind, C.c_int64(1), None, None, None, None, 0, None, None, _p(nnz), 1) == 0
    return int(nnz[0])


def flat_ocp_hess_host(problem, x, lam, sigma, traj, mesh_kind=0, value_differences=False, threads=1):
    """d2l_dx2 of ocp_to_nlp(flatten_ocp<FlatHess::Differences>(...), mesh) per agent on the host: dict hess [B][nnzH], differing [B]
    (values not bit-identical to meshfn::ocp_nlp_hess_assemble over the host arrays of flat_ocp_hess_nodes).
    value_differences=True: the default flatten_ocp, whose d2l_dx2 differences the flat values (differing stays -1)."""
    s = flat_ocp_mesh(problem, mesh_kind)
    d = flat_ocp_sizes(problem, s["N"])
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, s["n"])
    B = len(x)
    lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(B, s["m"])
    sigma = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B,)))
    traj = np.ascontiguousarray(traj, dtype=np.float64).reshape(B, d["row"])
    out = dict(hess=np.full((B, flat_ocp_nnz_hess(problem, mesh_kind)), np.nan), differing=np.full(B, -1, np.int64))
    rc = lib().sfbx_flat_ocp_hess_host(FLAT_PROBLEMS[problem], mesh_kind, C.c_int64(B), _p(x), _p(lam), _p(sigma), _p(traj), int(value_differences),
                                       _p(out["hess"]), _p(out["differing"]), None, threads)
    assert rc == 0, rc
    return out


def test_flatten_hess_api():
    """(code, figures [8]) of sfbx_test_flatten_hess_api: 0, or the first failing expectation"""
    fig = np.zeros(8)
    return int(lib().sfbx_test_flatten_hess_api(_p(fig))), fig


def test_flatten_api():
    """(code, figures [8]) of sfbx_test_flatten_api: 0, or the first failing expectation"""
    fig = np.zeros(8)
    return int(lib().sfbx_test_flatten_api(_p(fig))), fig
