"""ctypes wrappers of the re-linearisation harness (examples/mpc_relin.cpp in libsfb_models.so, examples/mpc_relin_device.hip in
libsfb_models_dev.so), used by tests/test_mpc_relin_*.py, tests/golden/make_golden_mpc_relin.py and scripts/mpc_relin_time.py."""
import ctypes as C

import numpy as np

from examples import models_lib as M

_p = M._p


def _agents(t, dx0):
    dx0 = np.ascontiguousarray(dx0, dtype=np.float64)
    return np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (len(dx0),))), dx0


def record_doubles(variant, K):
    d = M.mpc_dims(variant, K)
    Nx, Nu, N = d["Nx"], d["Nu"], d["N"]
    return N * (2 * Nx + Nx * Nx + Nx * Nu + 2 + 2 * Nx + 2 * Nu) + Nx + Nx * Nx


def split_record(variant, K, rec):
    """one unpacked record -> dict of its fields (sfb.h)"""
    d = M.mpc_dims(variant, K)
    Nx, Nu, N, ncr = d["Nx"], d["Nu"], d["N"], 2
    sz = [N * Nx, N * Nx, N * Nx * Nx, N * Nx * Nu, N * ncr, N * ncr * Nx, N * ncr * Nu, Nx, Nx * Nx]
    f, dx, dfx, dfu, c, dcx, dcu, e, J = np.split(np.asarray(rec), np.cumsum(sz)[:-1])
    return dict(f=f.reshape(N, Nx), dxdes=dx.reshape(N, Nx), dfdx=dfx.reshape(N, Nx, Nx), dfdu=dfu.reshape(N, Nx, Nu), c=c.reshape(N, ncr),
                dcdx=dcx.reshape(N, ncr, Nx), dcdu=dcu.reshape(N, ncr, Nu), e=e, J=J.reshape(Nx, Nx))


def flat_records(variant, K, tf, t, dx0, primal=None):
    """MPC::fill_flat_record of the agents xdes(t[b]) (+) dx0[b] about primal (B, n) (None: the plan e = v = 0)"""
    t, dx0 = _agents(t, dx0)
    rec = np.zeros((len(dx0), record_doubles(variant, K)))
    pr = None if primal is None else np.ascontiguousarray(primal, dtype=np.float64)
    rc = M.lib().sfbx_mpc_relin_flat_records(variant, K, C.c_double(tf), C.c_int64(len(dx0)), _p(t), _p(dx0), None if pr is None else _p(pr), _p(rec))
    assert rc == 0, rc
    return rec


def assemble_flat(variant, K, tf, rec):
    """MPC::assemble_flat_record -> Av (B, nnzA), l, u (B, m)"""
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    d, B = M.mpc_dims(variant, K), len(rec)
    Av, l, u = np.zeros((B, d["nnzA"])), np.zeros((B, d["m"])), np.zeros((B, d["m"]))
    assert M.lib().sfbx_mpc_relin_assemble_flat(variant, K, C.c_double(tf), C.c_int64(B), _p(rec), _p(Av), _p(l), _p(u)) == 0
    return Av, l, u


def assemble(variant, K, tf, t, dx0):
    """MPC::assemble (the pass-one problem) of the same agents"""
    t, dx0 = _agents(t, dx0)
    d, B = M.mpc_dims(variant, K), len(dx0)
    Av, l, u = np.zeros((B, d["nnzA"])), np.zeros((B, d["m"])), np.zeros((B, d["m"]))
    assert M.lib().sfbx_mpc_relin_assemble(variant, K, C.c_double(tf), C.c_int64(B), _p(t), _p(dx0), _p(Av), _p(l), _p(u)) == 0
    return Av, l, u


def probe(variant, K, tf, t=0.0):
    """the A_keep masks of MPC::probe_default and MPC::probe_relin"""
    nnz = M.mpc_dims(variant, K)["nnzA"]
    kd, kr = np.zeros(nnz, np.uint8), np.zeros(nnz, np.uint8)
    assert M.lib().sfbx_mpc_relin_probe(variant, K, C.c_double(tf), C.c_double(t), _p(kd), _p(kr)) == 0
    return kd.astype(bool), kr.astype(bool)


def tick_host(variant, K, tf, t, dx0, passes):
    """the host path: per agent one cold tick of MPC::operator() with MPCParams::relin_passes = passes (solves on the GPU)"""
    t, dx0 = _agents(t, dx0)
    d, B, nivals = M.mpc_dims(variant, K), len(dx0), -(-K // 4)
    out = dict(primal=np.zeros((B, d["n"])), code=np.zeros(B, np.int32), u0=np.zeros((B, d["Nu"])), errs=np.zeros((B, nivals)))
    rc = M.lib().sfbx_mpc_relin_tick_host(variant, K, C.c_double(tf), C.c_int64(B), _p(t), _p(dx0), passes, _p(out["primal"]), _p(out["code"]),
                                          _p(out["u0"]), _p(out["errs"]))
    assert rc == 0, rc
    out["agent_max"] = out["errs"].max(axis=1)
    return out


def swarm(K, tf, t, dx0, passes, prune=0, ticks=1, want_records=False, want_Ax=False):
    """MPCSwarmDeviceLin::step(.., passes) of the planar vehicle (variant 6), `ticks` times from the same states; prune: 0 the
    swarm's own probe, 1 the mask of MPC::probe_relin, 2 the whole pattern"""
    t, dx0 = _agents(t, dx0)
    d, B = M.mpc_dims(6, K), len(dx0)
    out = dict(primal=np.zeros((B, d["n"])), code=np.zeros(B, np.int32), iter=np.zeros(B, np.uint32), u0=np.zeros((B, 2)), agent_max=np.zeros(B))
    rec = np.zeros((B, record_doubles(6, K))) if want_records else None
    Ax = np.zeros((B, d["nnzA"])) if want_Ax else None
    info, seconds = np.zeros(6, np.int64), np.zeros(1)
    rc = M.dev_lib().sfbx_mpc_relin_swarm(K, C.c_double(tf), C.c_int64(B), _p(t), _p(dx0), passes, prune, ticks, _p(out["primal"]), _p(out["code"]),
                                          _p(out["iter"]), _p(out["u0"]), _p(out["agent_max"]), None if rec is None else _p(rec),
                                          None if Ax is None else _p(Ax), _p(info), _p(seconds))
    assert rc == 0, rc
    out.update(free_before=int(info[0]), free_after=int(info[1]), nnzA_kept=int(info[2]), nnzL_fallback=int(info[3]), nnzA=int(info[4]),
               packed=bool(info[5]), seconds=float(seconds[0]), flat_records=rec, Ax=Ax)
    return out


def kernel(K, tf, t, dx0, plan=None, code=None, side=False, reps=0, want_status=False):
    """mpc_relinearise_kernel alone behind one tick of the swarm; plan (B, n) / code (B) replace the swarm's solution first"""
    t, dx0 = _agents(t, dx0)
    d, B = M.mpc_dims(6, K), len(dx0)
    pl = None if plan is None else np.ascontiguousarray(plan, dtype=np.float64)
    cd = None if code is None else np.ascontiguousarray(code, dtype=np.int32)
    out = dict(plan=np.zeros((B, d["n"])), code=np.zeros(B, np.int32), rec=np.zeros((B, record_doubles(6, K))))
    side_rec = np.zeros_like(out["rec"]) if side else None
    status, seconds = np.full(3, -1, np.int32), np.zeros(1)
    rc = M.dev_lib().sfbx_mpc_relin_kernel(K, C.c_double(tf), C.c_int64(B), _p(t), _p(dx0), None if pl is None else _p(pl), None if cd is None else _p(cd),
                                           int(side), reps, _p(out["plan"]), _p(out["code"]), _p(out["rec"]), None if side_rec is None else _p(side_rec),
                                           _p(status) if want_status else None, _p(seconds))
    assert rc == 0, rc
    out.update(rec_side=side_rec, status=status, seconds=float(seconds[0]))
    return out


def swarm_multi(K, tf, t, dx0, passes, devices):
    """one tick with `passes` passes through MPCSwarmMultiDeviceLin, the agents sharded over `devices`"""
    t, dx0 = _agents(t, dx0)
    B = len(dx0)
    out = dict(u0=np.zeros((B, 2)), code=np.zeros(B, np.int32), iter=np.zeros(B, np.uint32))
    dev = (C.c_int * len(devices))(*devices)
    rc = M.dev_lib().sfbx_mpc_relin_swarm_multi(K, C.c_double(tf), C.c_int64(B), _p(t), _p(dx0), passes, dev, len(devices), _p(out["u0"]),
                                                _p(out["code"]), _p(out["iter"]))
    assert rc == 0, rc
    return out
