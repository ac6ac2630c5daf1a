"""Batched Lie-group cubic splines over the C-ABI (include/sfb.h: sfb_spline_*; the C++ side is
include/smooth_feedback_amd/spline.hpp: Spline<K, G>, fit_spline_cubic).  Groups and element storage as in pid.py.  A
spline has S + 1 knots: knot times tk (S+1,), knot elements gk (S+1, elem), control differences V (S, 3, dof); a batch
carries a leading axis B on each.  pid.pid_rollout_spline_batch_host closes the PID loop along such splines."""
import ctypes as C

import numpy as np

from . import _capi
from .pid import _group, _spline_arrays
from .qp import _ptr


def spline_fit_cubic_batch_host(group, tk, gk):
    """The interpolating C^1 cubic through gk (B, S+1, elem) at the knot times tk (B, S+1), or (S+1,) shared by all
    (sfb_spline_fit_cubic_batch_host).  Returns V (B, S, 3, dof)."""
    g = _group(group)
    gk = np.ascontiguousarray(gk, dtype=np.float64)
    tk = np.ascontiguousarray(tk, dtype=np.float64)
    if gk.ndim != 3 or gk.shape[2] != g.elem:
        raise ValueError("gk: expected shape (B, S+1, %d), got %r" % (g.elem, gk.shape))
    B, K = gk.shape[:2]
    if tk.shape not in ((K,), (B, K)):
        raise ValueError("tk: expected shape (%d, %d) or (%d,), got %r" % (B, K, K, tk.shape))
    V = np.zeros((B, max(K - 1, 0), 3, g.dof))
    _capi.check(_capi.lib.sfb_spline_fit_cubic_batch_host(C.byref(g.c), B, K, _ptr(tk), 1 if tk.ndim == 1 else 0, _ptr(gk), _ptr(V)))
    return V


def spline_eval_batch_host(group, tk, gk, V, t, ts0=None, batch=None):
    """Every agent's spline at its times (sfb_spline_eval_batch_host): the spline per agent (leading axis B) or ONE for all
    (then B comes from t (B, nt), or from `batch` when t is (nt,) and shared too); agent b evaluates at t - ts0[b].
    Returns g (B, nt, elem), body velocity and body acceleration (B, nt, dof)."""
    g = _group(group)
    t = np.ascontiguousarray(t, dtype=np.float64)
    tk_ = np.asarray(tk)
    B = tk_.shape[0] if tk_.ndim == 2 else (t.shape[0] if t.ndim == 2 else batch)
    if B is None:
        raise ValueError("a shared spline at shared times needs batch=")
    tk, gk, V, shared, K, ts0 = _spline_arrays(g, B, tk, gk, V, ts0)
    nt = t.shape[-1]
    if t.shape not in ((nt,), (B, nt)):
        raise ValueError("t: expected shape (%d, nt) or (nt,), got %r" % (B, t.shape))
    out = np.zeros((B, nt, g.elem)), np.zeros((B, nt, g.dof)), np.zeros((B, nt, g.dof))
    _capi.check(_capi.lib.sfb_spline_eval_batch_host(C.byref(g.c), B, K, _ptr(tk), _ptr(gk), _ptr(V), shared, _ptr(ts0) if ts0 is not None else None,
                                                     nt, _ptr(t), 1 if t.ndim == 1 else 0, *[_ptr(a) for a in out]))
    return out


def spline_fit_cubic_batch_device(group, B, nknots, dtk, tk_shared, dgk, dV, stream=0):
    """sfb_spline_fit_cubic_batch on device pointers (ints), asynchronous on `stream`."""
    g = _group(group)
    _capi.check(_capi.lib.sfb_spline_fit_cubic_batch(C.byref(g.c), int(B), int(nknots), dtk, int(tk_shared), dgk, dV, stream or None))


def spline_eval_batch_device(group, B, nknots, dtk, dgk, dV, spline_shared, dts0, nt, dt, t_shared, dg, dvel, dacc, stream=0):
    """sfb_spline_eval_batch on device pointers (ints; dts0 0 / None: no time origins), asynchronous on `stream`."""
    g = _group(group)
    _capi.check(_capi.lib.sfb_spline_eval_batch(C.byref(g.c), int(B), int(nknots), dtk, dgk, dV, int(spline_shared), dts0 or None, int(nt), dt,
                                                int(t_shared), dg, dvel, dacc, stream or None))
