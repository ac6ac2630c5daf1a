"""Batched Lie-group PID over the C-ABI (smooth::feedback::PID, pid.hpp:74-87; include/sfb.h: sfb_pid_*).

A group is a list of parts such as [("SE3", 6), ("RN", 3)] (names or sfb_lie_kind numbers).  Element storage per part:
RN N values, SE2 (x, y, cos, sin), SO3 (w, x, y, z), SE3 (px, py, pz, w, x, y, z); a bundle is its parts one after the
other and tangents are concatenated in the same order.  include/smooth_feedback_amd/pid.hpp has the C++ front PID<T, G>
(one controller, CPU) and pid_device.hpp the device-resident swarm for functor trajectories."""
import ctypes as C

import numpy as np

from . import _capi
from .qp import _ptr

LIE_KINDS = {"RN": 0, "SE2": 1, "SO3": 2, "SE3": 3}  # sfb_lie_kind
_ELEM = {0: None, 1: 4, 2: 4, 3: 7}


class PIDGroup:
    """sfb_pid_group: the parts of the state bundle in order.  elem / dof: doubles per element / per tangent."""

    def __init__(self, parts):
        parts = [(LIE_KINDS[k.upper()] if isinstance(k, str) else int(k), int(d)) for k, d in parts]
        self.parts = parts
        self._kind = np.array([k for k, _ in parts], dtype=np.int32)
        self._dof = np.array([d for _, d in parts], dtype=np.int32)
        self.c = _capi.SfbPIDGroup(len(parts), self._kind.ctypes.data, self._dof.ctypes.data)
        self.elem = int(_capi.lib.sfb_pid_elem_doubles(C.byref(self.c)))
        self.dof = int(_capi.lib.sfb_pid_dof(C.byref(self.c)))
        if self.elem < 0:
            raise ValueError("bad PID group %r: kinds are RN / SE2 / SO3 / SE3, dof 3 for SE2 and SO3, 6 for SE3, >= 1 for RN, "
                             "at most 8 parts" % (parts,))


def _group(group):
    return group if isinstance(group, PIDGroup) else PIDGroup(group)


def _rows(a, B, w, name, shared_ok=False):
    """(array [B][w] or, if allowed, [w]; shared flag)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shared_ok and a.shape == (w,):
        return a, 1
    if a.shape != (B, w):
        raise ValueError("%s: expected shape (%d, %d)%s, got %r" % (name, B, w, " or (%d,)" % w if shared_ok else "", a.shape))
    return a, 0


def _shared_together(flags, what):
    if len(set(flags)) != 1:
        raise ValueError("%s must all be per agent or all shared" % what)
    return flags[0]


def pid_step_batch_host(group, t, x, v, g_des, v_des, a_des, kp, kd, ki, i_err, t_last, windup_limit=np.inf):
    """One controller call at time t for every agent (sfb_pid_step_batch_host).  x (B, elem), v (B, dof); the desired
    triple g_des (B, elem), v_des, a_des (B, dof) or ONE triple (elem,), (dof,), (dof,) for the whole swarm; gains
    (B, dof) or (dof,); state i_err (B, dof), t_last (B,) with NaN = unset.  Returns (u, i_err, t_last) as new arrays."""
    g = _group(group)
    x = np.ascontiguousarray(x, dtype=np.float64)
    B = x.shape[0]
    x, _ = _rows(x, B, g.elem, "x")
    v, _ = _rows(v, B, g.dof, "v")
    gd, s0 = _rows(g_des, B, g.elem, "g_des", True)
    vd, s1 = _rows(v_des, B, g.dof, "v_des", True)
    ad, s2 = _rows(a_des, B, g.dof, "a_des", True)
    des_shared = _shared_together([s0, s1, s2], "g_des, v_des, a_des")
    kp, g0 = _rows(kp, B, g.dof, "kp", True)
    kd, g1 = _rows(kd, B, g.dof, "kd", True)
    ki, g2 = _rows(ki, B, g.dof, "ki", True)
    gains_shared = _shared_together([g0, g1, g2], "kp, kd, ki")
    ie = np.array(_rows(i_err, B, g.dof, "i_err")[0])
    tl = np.array(_rows(np.reshape(t_last, (-1, 1)), B, 1, "t_last")[0]).reshape(B)
    u = np.zeros((B, g.dof))
    _capi.check(_capi.lib.sfb_pid_step_batch_host(C.byref(g.c), B, float(t), _ptr(x), _ptr(v), _ptr(gd), _ptr(vd), _ptr(ad), des_shared,
                                                  _ptr(kp), _ptr(kd), _ptr(ki), gains_shared, float(windup_limit), _ptr(ie), _ptr(tl), _ptr(u)))
    return u, ie, tl


def pid_rollout_batch_host(group, t0, dt, steps, x, v, g_des0, v_des, kp, kd, ki, i_err, t_last, windup_limit=np.inf, u_max=None):
    """`steps` closed-loop ticks on the double integrator d^r x = v, dv/dt = u in ONE launch (sfb_pid_rollout_batch_host);
    every agent tracks g_des(t) = rplus(g_des0, t v_des).  Shapes as pid_step_batch_host; u_max (dof,) or None.  Returns a
    dict of new arrays x, v, i_err, t_last, u_last, cost.  steps = 0: the state comes back as it went in, u_last and cost 0."""
    g = _group(group)
    x = np.array(x, dtype=np.float64, order="C")
    B = x.shape[0]
    x = np.array(_rows(x, B, g.elem, "x")[0])
    v = np.array(_rows(v, B, g.dof, "v")[0])
    g0, s0 = _rows(g_des0, B, g.elem, "g_des0", True)
    vd, s1 = _rows(v_des, B, g.dof, "v_des", True)
    des_shared = _shared_together([s0, s1], "g_des0, v_des")
    kp, f0 = _rows(kp, B, g.dof, "kp", True)
    kd, f1 = _rows(kd, B, g.dof, "kd", True)
    ki, f2 = _rows(ki, B, g.dof, "ki", True)
    gains_shared = _shared_together([f0, f1, f2], "kp, kd, ki")
    ie = np.array(_rows(i_err, B, g.dof, "i_err")[0])
    tl = np.array(_rows(np.reshape(t_last, (-1, 1)), B, 1, "t_last")[0]).reshape(B)
    um = None
    if u_max is not None:
        um = np.ascontiguousarray(u_max, dtype=np.float64)
        if um.shape != (g.dof,):
            raise ValueError("u_max: expected shape (%d,), got %r" % (g.dof, um.shape))
    u = np.zeros((B, g.dof))
    cost = np.zeros(B)
    _capi.check(_capi.lib.sfb_pid_rollout_batch_host(C.byref(g.c), B, float(t0), float(dt), int(steps), _ptr(x), _ptr(v), _ptr(g0), _ptr(vd),
                                                     des_shared, _ptr(kp), _ptr(kd), _ptr(ki), gains_shared, float(windup_limit),
                                                     _ptr(um) if um is not None else None, _ptr(ie), _ptr(tl), _ptr(u), _ptr(cost)))
    return dict(x=x, v=v, i_err=ie, t_last=tl, u_last=u, cost=cost)


def _spline_arrays(g, B, tk, gk, V, ts0):
    """the spline arguments of the C-ABI: tk (S+1,), gk (S+1, elem), V (S, 3, dof) for ONE shared spline, or each with a
    leading batch axis; ts0 (B,) or None.  -> tk, gk, V, shared flag, nknots, ts0"""
    tk = np.ascontiguousarray(tk, dtype=np.float64)
    gk = np.ascontiguousarray(gk, dtype=np.float64)
    V = np.ascontiguousarray(V, dtype=np.float64)
    shared = 1 if tk.ndim == 1 else 0
    K = tk.shape[-1]
    lead = () if shared else (B,)
    if tk.shape != lead + (K,) or gk.shape != lead + (K, g.elem) or V.shape != lead + (K - 1, 3, g.dof):
        raise ValueError("spline: expected tk %r, gk %r, V %r (all shared or all per agent), got %r, %r, %r"
                         % (lead + (K,), lead + (K, g.elem), lead + (K - 1, 3, g.dof), tk.shape, gk.shape, V.shape))
    if ts0 is not None:
        ts0 = np.ascontiguousarray(ts0, dtype=np.float64)
        if ts0.shape != (B,):
            raise ValueError("ts0: expected shape (%d,), got %r" % (B, ts0.shape))
    return tk, gk, V, shared, K, ts0


def pid_rollout_spline_batch_host(group, t0, dt, steps, x, v, tk, gk, V, kp, kd, ki, i_err, t_last, ts0=None, windup_limit=np.inf, u_max=None):
    """pid_rollout_batch_host with a cubic spline as the desired trajectory (sfb_pid_rollout_spline_batch_host): agent b
    tracks its spline -- tk (B, S+1), gk (B, S+1, elem), V (B, S, 3, dof) as spline_fit_cubic_batch_host returns them, or
    ONE spline without the batch axis -- at t_k - ts0[b] (ts0 (B,) or None: 0).  Everything else, and the returned dict, as
    pid_rollout_batch_host."""
    g = _group(group)
    x = np.array(x, dtype=np.float64, order="C")
    B = x.shape[0]
    x = np.array(_rows(x, B, g.elem, "x")[0])
    v = np.array(_rows(v, B, g.dof, "v")[0])
    tk, gk, V, shared, K, ts0 = _spline_arrays(g, B, tk, gk, V, ts0)
    kp, f0 = _rows(kp, B, g.dof, "kp", True)
    kd, f1 = _rows(kd, B, g.dof, "kd", True)
    ki, f2 = _rows(ki, B, g.dof, "ki", True)
    gains_shared = _shared_together([f0, f1, f2], "kp, kd, ki")
    ie = np.array(_rows(i_err, B, g.dof, "i_err")[0])
    tl = np.array(_rows(np.reshape(t_last, (-1, 1)), B, 1, "t_last")[0]).reshape(B)
    um = None
    if u_max is not None:
        um = np.ascontiguousarray(u_max, dtype=np.float64)
        if um.shape != (g.dof,):
            raise ValueError("u_max: expected shape (%d,), got %r" % (g.dof, um.shape))
    u = np.zeros((B, g.dof))
    cost = np.zeros(B)
    _capi.check(_capi.lib.sfb_pid_rollout_spline_batch_host(C.byref(g.c), B, float(t0), float(dt), int(steps), _ptr(x), _ptr(v), K, _ptr(tk), _ptr(gk),
                                                            _ptr(V), shared, _ptr(ts0) if ts0 is not None else None, _ptr(kp), _ptr(kd), _ptr(ki),
                                                            gains_shared, float(windup_limit), _ptr(um) if um is not None else None, _ptr(ie),
                                                            _ptr(tl), _ptr(u), _ptr(cost)))
    return dict(x=x, v=v, i_err=ie, t_last=tl, u_last=u, cost=cost)


def pid_step_batch_device(group, B, t, dx, dv, dg_des, dv_des, da_des, des_shared, dkp, dkd, dki, gains_shared, windup_limit, di_err, dt_last, du,
                          stream=0):
    """sfb_pid_step_batch on device pointers (ints), asynchronous on `stream`."""
    g = _group(group)
    _capi.check(_capi.lib.sfb_pid_step_batch(C.byref(g.c), B, float(t), dx, dv, dg_des, dv_des, da_des, int(des_shared), dkp, dkd, dki,
                                             int(gains_shared), float(windup_limit), di_err, dt_last, du, stream or None))


def pid_rollout_batch_device(group, B, t0, dt, steps, dx, dv, dg_des0, dv_des, des_shared, dkp, dkd, dki, gains_shared, windup_limit, du_max,
                             di_err, dt_last, du_last, dcost, stream=0):
    """sfb_pid_rollout_batch on device pointers (ints; du_max 0 / None: no clamp), asynchronous on `stream`."""
    g = _group(group)
    _capi.check(_capi.lib.sfb_pid_rollout_batch(C.byref(g.c), B, float(t0), float(dt), int(steps), dx, dv, dg_des0, dv_des, int(des_shared), dkp,
                                                dkd, dki, int(gains_shared), float(windup_limit), du_max or None, di_err, dt_last, du_last, dcost,
                                                stream or None))


def pid_rollout_spline_batch_device(group, B, t0, dt, steps, dx, dv, nknots, dtk, dgk, dV, spline_shared, dts0, dkp, dkd, dki, gains_shared,
                                    windup_limit, du_max, di_err, dt_last, du_last, dcost, stream=0):
    """sfb_pid_rollout_spline_batch on device pointers (ints; dts0 and du_max 0 / None: no time origins, no clamp), asynchronous
    on `stream`."""
    g = _group(group)
    _capi.check(_capi.lib.sfb_pid_rollout_spline_batch(C.byref(g.c), B, float(t0), float(dt), int(steps), dx, dv, int(nknots), dtk, dgk, dV,
                                                       int(spline_shared), dts0 or None, dkp, dkd, dki, int(gains_shared), float(windup_limit),
                                                       du_max or None, di_err, dt_last, du_last, dcost, stream or None))
