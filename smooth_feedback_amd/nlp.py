"""Swarm SQP for a batch of NLPs that share their patterns and bounds (sfb_nlp_sqp_* of include/sfb.h; the law is in
DESIGN.md, "Swarm SQP").  The solver is model-free: the caller's `evaluate` is a torch function on device tensors."""
import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _capi
from .qp import QPSolverParams, _ptr

RUNNING, OPTIMAL, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE, MAX_ITERATIONS, MAX_TIME, UNKNOWN = -1, 0, 1, 2, 3, 4, 5


def _default_qp():
    return QPSolverParams(eps_abs=1e-9, eps_rel=1e-9, max_iter=10000)


@dataclass
class NLPSQPParams:
    """sfb_nlp_sqp_params; qp: the inner solver's QPSolverParams."""
    tol: float = 1e-6
    max_iter: int = 50
    kappa: float = 1e-8
    mu_first: float = 1e-4
    mu_grow: float = 8.0
    mu_max: float = 1e4
    qp: QPSolverParams = field(default_factory=_default_qp)

    def to_c(self):
        p = _capi.SfbNlpSqpParams()
        p.tol, p.max_iter, p.kappa = float(self.tol), int(self.max_iter), float(self.kappa)
        p.mu_first, p.mu_grow, p.mu_max = float(self.mu_first), float(self.mu_grow), float(self.mu_max)
        p.qp = self.qp.to_c()
        return p


def _patterns(n, m, J_rowptr, J_colind, H_colptr, H_rowind, xl, xu, gl, gu):
    ints = [np.ascontiguousarray(a, dtype=np.int32).ravel() for a in (J_rowptr, J_colind, H_colptr, H_rowind)]
    dbls = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (xl, xu, gl, gu)]
    for a, want, name in zip(ints[::2] + dbls, (m + 1, n + 1, n, n, m, m), ("J_rowptr", "H_colptr", "xl", "xu", "gl", "gu")):
        if len(a) != want:
            raise ValueError("%s: expected %d entries, got %d" % (name, want, len(a)))
    return ints, dbls


def nlp_sqp_qp_pattern(n, m, J_rowptr, J_colind, H_colptr, H_rowind, xl, xu, gl, gu):
    """-> dict(nb, A_rowptr, A_colind, P_colptr, P_rowind, P_src, P_diag, Jc_colptr, Jc_row, Jc_pos, bound_var)
    (sfb_nlp_sqp_qp_pattern; host only)"""
    n, m = int(n), int(m)
    ints, dbls = _patterns(n, m, J_rowptr, J_colind, H_colptr, H_rowind, xl, xu, gl, gu)
    args = [_ptr(a) if a.size else None for a in ints + dbls]
    nb = C.c_int64()
    _capi.check(_capi.lib.sfb_nlp_sqp_qp_pattern(n, m, *args, *([None] * 10), C.byref(nb)))
    nnzJ, nnzP = int(ints[0][-1]), 2 * int(ints[2][-1]) - n
    out = [np.zeros(k, np.int32) for k in (m + nb.value + 1, nnzJ + nb.value, n + 1, nnzP, nnzP, n, n + 1, nnzJ, nnzJ, nb.value)]
    _capi.check(_capi.lib.sfb_nlp_sqp_qp_pattern(n, m, *args, *[_ptr(a) if a.size else None for a in out], C.byref(nb)))
    names = ("A_rowptr", "A_colind", "P_colptr", "P_rowind", "P_src", "P_diag", "Jc_colptr", "Jc_row", "Jc_pos", "bound_var")
    return dict(zip(names, out), nb=nb.value)


@dataclass
class NLPSwarmSolution:
    """The state of the swarm as torch tensors (clones): x, z (B, n), lam (B, m), the others (B,)."""
    x: object
    lam: object
    z: object
    status: object
    iter: object
    r_stat: object
    r_pri: object
    r_comp: object
    mu: object
    alpha: object
    nu: object


class NLPSwarmSQP:
    """Owns an sfb_nlp_sqp: the sparse QP plan, the QP arrays, the workspace and the state of `batch` agents on the current
    device.  direction / trial / accept are the C entries on torch tensors and torch's current stream; solve() runs the loop."""

    def __init__(self, n, m, J_rowptr, J_colind, H_colptr, H_rowind, xl, xu, gl, gu, batch, params: Optional[NLPSQPParams] = None,
                 stage=None):
        self.n, self.m, self.batch = int(n), int(m), int(batch)
        ints, dbls = _patterns(self.n, self.m, J_rowptr, J_colind, H_colptr, H_rowind, xl, xu, gl, gu)
        self.params = params or NLPSQPParams()
        cp = self.params.to_c()
        st = None if stage is None else np.ascontiguousarray(stage, dtype=np.int32)
        h = C.c_void_p()
        _capi.check(_capi.lib.sfb_nlp_sqp_create(self.n, self.m, *[_ptr(a) if a.size else None for a in ints + dbls], self.batch,
                                                 C.byref(cp), _ptr(st), C.byref(h)))
        self._h = h
        b, nn, mm, nb, nnzH, nnzP, nnzA = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        _capi.check(_capi.lib.sfb_nlp_sqp_info(h, C.byref(b), C.byref(nn), C.byref(mm), C.byref(nb), C.byref(nnzH), C.byref(nnzP), C.byref(nnzA)))
        self.nb, self.nnzH, self.nnzP, self.nnzA, self.nnzJ = nb.value, nnzH.value, nnzP.value, nnzA.value, int(ints[0][-1])
        self.mq = self.m + self.nb

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib.sfb_nlp_sqp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the C entries on torch tensors ----
    @staticmethod
    def _p(t, shape):
        import torch
        if t is None:
            return None
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise ValueError("expected a contiguous float64 device tensor of shape %r, got %r" % (tuple(shape), tuple(t.shape)))
        return t.data_ptr() or None

    @staticmethod
    def _stream():
        import torch
        return torch.cuda.current_stream().cuda_stream or None

    def set_start(self, x, lam=None, z=None):
        B, n, m = self.batch, self.n, self.m
        _capi.check(_capi.lib.sfb_nlp_sqp_set_start(self._h, self._p(x, (B, n)), self._p(lam, (B, m)), self._p(z, (B, n)), self._stream()))

    def direction(self, f, df, g, dg_val, hess_val):
        """-> number of agents now in line search (sfb_nlp_sqp_direction; synchronises the current stream)"""
        B, n, m = self.batch, self.n, self.m
        active = C.c_int64()
        _capi.check(_capi.lib.sfb_nlp_sqp_direction(self._h, self._p(f, (B,)), self._p(df, (B, n)), self._p(g, (B, m)),
                                                    self._p(dg_val, (B, self.nnzJ)), self._p(hess_val, (B, self.nnzH)), C.byref(active), self._stream()))
        return active.value

    def trial(self, out=None):
        import torch
        if out is None:
            out = torch.empty((self.batch, self.n), dtype=torch.float64, device="cuda")
        _capi.check(_capi.lib.sfb_nlp_sqp_trial(self._h, self._p(out, (self.batch, self.n)), self._stream()))
        return out

    def accept(self, f_trial, g_trial):
        """-> number of agents still in line search (sfb_nlp_sqp_accept)"""
        B = self.batch
        left = C.c_int64()
        _capi.check(_capi.lib.sfb_nlp_sqp_accept(self._h, self._p(f_trial, (B,)), self._p(g_trial, (B, self.m)), C.byref(left), self._stream()))
        return left.value

    def _view(self, ptr, shape, dtype):
        """a tensor over the solver's own device memory (no copy; valid while the solver lives)"""
        import torch
        count = int(np.prod(shape))
        if count == 0 or not ptr:
            return torch.empty(shape, dtype=dtype, device="cuda")
        size = {torch.float64: 8, torch.int32: 4}[dtype]
        typestr = {torch.float64: "<f8", torch.int32: "<i4"}[dtype]

        class _Mem:
            __cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                        "strides": (size,)}
        return torch.as_tensor(_Mem(), device="cuda").view(shape)

    def state_views(self):
        """dict of tensors over the live state: x, lam, z, status, iter, r_stat, r_pri, r_comp, mu, alpha, nu"""
        import torch
        ptrs = [C.c_void_p() for _ in range(11)]
        _capi.check(_capi.lib.sfb_nlp_sqp_state(self._h, *[C.byref(p) for p in ptrs]))
        B, n, m = self.batch, self.n, self.m
        shapes = [(B, n), (B, m), (B, n), (B,), (B,), (B,), (B,), (B,), (B,), (B,), (B,)]
        dtypes = [torch.float64] * 3 + [torch.int32] * 2 + [torch.float64] * 6
        names = ("x", "lam", "z", "status", "iter", "r_stat", "r_pri", "r_comp", "mu", "alpha", "nu")
        return {k: self._view(p.value, s, d) for k, p, s, d in zip(names, ptrs, shapes, dtypes)}

    def state(self):
        return NLPSwarmSolution(**{k: v.clone() for k, v in self.state_views().items()})

    def debug_views(self):
        """dict of tensors over the QP arrays of the last rung (compacted: slot k is agent list[k]) and the judge's sums"""
        import torch
        ptrs = [C.c_void_p() for _ in range(11)]
        _capi.check(_capi.lib.sfb_nlp_sqp_debug_buffers(self._h, *[C.byref(p) for p in ptrs]))
        B, n, mq = self.batch, self.n, self.mq
        shapes = [(B, self.nnzP), (B, n), (B, self.nnzA), (B, mq), (B, mq), (B, n), (B, mq), (B,), (B,), (B,), (5, B)]
        dtypes = [torch.float64] * 7 + [torch.int32] * 3 + [torch.float64]
        names = ("Px", "q", "Ax", "l", "u", "d", "y", "code", "iter", "list", "sums")
        return {k: self._view(p.value, s, d) for k, p, s, d in zip(names, ptrs, shapes, dtypes)}

    # ---- the loop ----
    def solve(self, evaluate, x0, lambda0=None, z0=None, max_calls=None):
        """evaluate(x, lam, want_derivatives) -> (f (B,), g (B, m)) or, with derivatives, (f, g, df (B, n), dg_val (B, nnzJ),
        hess_val (B, nnzH)): the Hessian of f + lam . g over the upper-triangle CSC pattern.  Contiguous float64 device
        tensors.  Runs until no agent is running; -> NLPSwarmSolution."""
        self.set_start(x0, lambda0, z0)
        sv = self.state_views()
        calls = 0
        while max_calls is None or calls < max_calls:
            f, g, df, dg, hess = evaluate(sv["x"], sv["lam"], True)
            calls += 1
            searching = self.direction(f, df, g, dg, hess)
            if searching == 0:  # every agent has finished: one that goes on holds a direction
                break
            while searching:
                xt = self.trial()
                ft, gt = evaluate(xt, sv["lam"], False)[:2]
                searching = self.accept(ft, gt)
        return self.state()
