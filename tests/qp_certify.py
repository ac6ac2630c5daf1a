"""Optimality certificates for QP results that do not use the CPU oracle (test infrastructure).

`certify(prob, res, prm)` checks what a result of QPSolver (qp_solver.hpp) claims for its status code, from the problem
data as the caller passed it: dense col-major (`Problem.dense`) or CSC P / CSR A (`Problem.sparse`).  Arithmetic is in
np.longdouble, P is used as stored (check_stopping computes pbm.P * x, :586/:590), and the float parameters are widened
exactly as the reference widens them: float(np.float32(eps)).

Claims per code (line numbers: qp_solver.hpp of the reference):

* every code: obj == x . (1/2 P x + q) (:547), to the round-off of a float64 dot product of length n + 2.
  Codes 0 / 2 / 3 come out of a stopping check, which runs at iter % sci == 1 before ++iter (:449, :465, :479), so
  (iter - 1) % sci == 1 for sci >= 2; the only exception is code 2 at iter 0 from inconsistent bounds (:361-364).
  With sci < 2 no check ever runs (1 % 1 == 0): codes 0 and 3 are impossible and code 2 needs such bounds.
  Code 4 => iter == max_iter.  Codes 4, 5, 6: nothing more.
* code 0, polish off: the returned (x, y) are the ones check_stopping accepted (:544-546 only unscale them).
  ||Ax - z|| <= eps_abs + eps_rel max(||Ax||, ||z||) with z in [l, u] (:584-587) gives, with ||z|| <= ||Ax|| + ||Ax - z||,
  r = dist(Ax, [l, u])_inf <= (eps_abs + eps_rel ||Ax||) / (1 - eps_rel) =: r_max.  The dual residual obeys
  ||Px + q + A'y|| <= eps_abs + eps_rel max(||Px||, ||q||, ||A'y||) =: d_max (:588-593).
  Dual sign and complementarity: in exact arithmetic the last dual update is rho (v - clip(v)) (:471-476), positive only
  where z was clipped to a finite u and negative only where it was clipped to a finite l.  Round-off leaves tiny
  duals of either sign on the other rows; a wrong-signed dual of size tau_i = 1e-3 d_max / ||a_i||_1 moves A'y by at
  most 1e-3 of the dual tolerance, so the solver could not tell it from zero.  Hence: y_i > tau_i only if u_i is finite
  and then (Ax)_i >= u_i - r_max; y_i < -tau_i only if l_i is finite and then (Ax)_i <= l_i + r_max.
  Round-off slack: float64 sums of length k carry at most ~k ulps of the sum of absolute terms; the checker adds
  4 (k + 2) eps times that sum to every bound (`_slack`).
* code 0, polish on: nothing about feasibility or dual signs.  Polish (detail::polish_qp, :92-204) is accepted
  unconditionally (:515-539: the result of a successful factorisation replaces the iterate whatever its residuals),
  so a polished x may sit far outside the primal bound and polished duals may have the wrong sign: the reference's
  behaviour.  It is checked as an operation of its own (`certify_polish`) against a second solve with polish off.
* codes 2, 3: whether the verdict is right follows from how the problem was built (tests/qp_families.py).

Documented exceptions (the reference behaves this way):
* sci == 1 never runs a stopping check (:465, :479 test iter % stop_check_iter == 1), so infeasible and unbounded
  problems end with code 4 there.
"""
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
CODE_OPTIMAL, CODE_PRIMAL_INF, CODE_DUAL_INF, CODE_MAX_ITER = 0, 2, 3, 4


def f32(v):
    """A float parameter as the reference widens it (float member -> double)."""
    return float(np.float32(v))


# --------------------------------------------------------------------------------------------------------------------
# problem data: one shared pattern, per-item values
# --------------------------------------------------------------------------------------------------------------------
@dataclass
class Problem:
    n: int
    m: int
    prow: np.ndarray   # P entries (row, col), values Pv (B, nnzP), as stored
    pcol: np.ndarray
    Pv: np.ndarray
    arow: np.ndarray   # A entries, values Av (B, nnzA)
    acol: np.ndarray
    Av: np.ndarray
    q: np.ndarray
    l: np.ndarray
    u: np.ndarray

    @property
    def B(self):
        return self.q.shape[0]

    @classmethod
    def dense(cls, P, q, A, l, u):
        """Flat col-major buffers P (B, n*n), A (B, m*n) as solve_qp_batch_host takes them."""
        q = np.asarray(q, float); l = np.asarray(l, float)
        B, n = q.shape
        m = l.shape[1]
        pr, pc = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        ar, ac = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
        # col-major: entry (i, j) at j * rows + i
        return cls(n, m, pr.ravel(), pc.ravel(), np.asarray(P, float).reshape(B, n, n)[:, pc.ravel(), pr.ravel()],
                   ar.ravel(), ac.ravel(), np.asarray(A, float).reshape(B, n, m)[:, ac.ravel(), ar.ravel()],
                   q, l, np.asarray(u, float))

    @classmethod
    def sparse(cls, Pp, Pi, Px, q, Ap, Aj, Ax, l, u):
        q = np.asarray(q, float); l = np.asarray(l, float)
        n, m = q.shape[1], l.shape[1]
        Pp, Ap = np.asarray(Pp), np.asarray(Ap)
        pcol = np.repeat(np.arange(n), np.diff(Pp))
        arow = np.repeat(np.arange(m), np.diff(Ap))
        B = q.shape[0]
        return cls(n, m, np.asarray(Pi, np.int64), pcol, np.asarray(Px, float).reshape(B, -1), arow,
                   np.asarray(Aj, np.int64), np.asarray(Ax, float).reshape(B, -1), q, l, np.asarray(u, float))

    def take(self, idx):
        idx = np.asarray(idx)
        return Problem(self.n, self.m, self.prow, self.pcol, self.Pv[idx], self.arow, self.acol, self.Av[idx],
                       self.q[idx], self.l[idx], self.u[idx])


def _mv(rows, cols, vals, x, nrows, absolute=False):
    """(B, nrows) = M x per item in longdouble; M given by entries (rows, cols) with values vals (B, nnz)."""
    out = np.zeros((x.shape[0], nrows), dtype=LD)
    if rows.size == 0:
        return out
    v = np.abs(vals.astype(LD)) if absolute else vals.astype(LD)
    prod = v * (np.abs(x[:, cols]) if absolute else x[:, cols])
    order = np.argsort(rows, kind="stable")
    rs = rows[order]
    starts = np.flatnonzero(np.r_[True, rs[1:] != rs[:-1]])
    out[:, rs[starts]] = np.add.reduceat(prod[:, order], starts, axis=1)
    return out


def _ninf(a):
    return np.max(np.abs(a), axis=1, initial=LD(0))


def _slack(k, absterms):
    """Round-off bound of a float64 sum of k terms whose absolute values add up to absterms."""
    return LD(4 * (k + 2)) * LD(EPS) * absterms


# --------------------------------------------------------------------------------------------------------------------
# the per-code certificate
# --------------------------------------------------------------------------------------------------------------------
@dataclass
class Report:
    ok: np.ndarray                      # per item
    why: list = field(default_factory=list)
    counts: dict = field(default_factory=dict)
    worst: dict = field(default_factory=dict)

    def fail(self, mask, what):
        mask = np.asarray(mask, bool)
        if mask.any():
            self.ok &= ~mask
            self.why.append("%s: items %s" % (what, np.flatnonzero(mask)[:8].tolist()))

    def ratio(self, name, r):
        r = np.asarray(r, float)
        if r.size:
            self.worst[name] = max(self.worst.get(name, 0.0), float(np.nanmax(r)))

    @property
    def passed(self):
        return bool(self.ok.all())

    def __str__(self):
        return "certified %s; worst ratios %s%s" % (
            self.counts, {k: "%.3g" % v for k, v in self.worst.items()},
            "" if self.passed else "; FAILED " + "; ".join(self.why))


def _get(res, name):
    alias = {"x": ("primal", "x"), "y": ("dual", "y"), "obj": ("objective", "obj"), "iter": ("iter",), "code": ("code",)}
    for a in alias[name]:
        if isinstance(res, dict) and a in res:
            return np.asarray(res[a])
        if hasattr(res, a):
            return np.asarray(getattr(res, a))
    raise KeyError(name)


def _prm(prm, name, default=None):
    return getattr(prm, name, default)


def certify(prob: Problem, res, prm, chunk=1 << 22) -> Report:
    """Per-item certificate of `res` (a QPBatchSolution or the oracle's dict) for the solver parameters `prm`
    (smooth_feedback_amd.QPSolverParams or the oracle's params).  Polish is certified separately (certify_polish)."""
    code, it = _get(res, "code").astype(np.int64), _get(res, "iter").astype(np.int64)
    x, y, obj = _get(res, "x"), _get(res, "y"), _get(res, "obj")
    B, n, m = prob.B, prob.n, prob.m
    rep = Report(ok=np.ones(B, bool))
    sci = int(_prm(prm, "stop_check_iter"))
    max_iter = _prm(prm, "max_iter")
    max_iter = None if max_iter is None or max_iter < 0 else int(max_iter)
    polish = bool(_prm(prm, "polish"))
    eps_abs, eps_rel = f32(_prm(prm, "eps_abs")), f32(_prm(prm, "eps_rel"))

    bad_bounds = ((prob.l == np.inf) | (prob.u == -np.inf) | (prob.u - prob.l < 0)).any(axis=1)
    from_check = np.isin(code, (0, 2, 3))
    at_zero = (code == CODE_PRIMAL_INF) & (it == 0) & bad_bounds
    if sci >= 2:
        rep.fail(from_check & ~at_zero & ((it - 1) % sci != 1), "iter of a stopping check: (iter - 1) % sci != 1")
    else:
        rep.fail(from_check & ~at_zero, "code %s with no stopping check (sci < 2)")
    if max_iter is None:
        rep.fail(code == CODE_MAX_ITER, "code 4 without max_iter")
    else:
        rep.fail((code == CODE_MAX_ITER) & (it != max_iter), "code 4 with iter != max_iter")
        rep.fail(it > max_iter, "iter > max_iter")
    rep.fail((code < 0) | (code > 6) | (code == 1), "status code out of range")

    step = max(1, chunk // max(1, prob.Pv.shape[1], prob.Av.shape[1], n + m))
    for s in range(0, B, step):
        sl = slice(s, min(B, s + step))
        rep.ok[sl] &= _certify_chunk(prob.take(np.arange(B)[sl]), code[sl], x[sl], y[sl], obj[sl], polish, eps_abs,
                                     eps_rel, rep, s)
    rep.counts = {"items": B, "optimal": int((code == 0).sum()), "certified": int(rep.ok.sum()),
                  **{"code%d" % c: int((code == c).sum()) for c in (2, 3, 4, 5, 6) if (code == c).any()}}
    return rep


def _certify_chunk(pb, code, x, y, obj, polish, eps_abs, eps_rel, rep, offset):
    n, m = pb.n, pb.m
    ok = np.ones(pb.B, bool)

    def fail(mask, what):
        mask = np.asarray(mask, bool)
        if mask.any():
            ok[mask] = False
            rep.why.append("%s: items %s" % (what, (offset + np.flatnonzero(mask)[:8]).tolist()))

    fin = np.isfinite(x).all(axis=1) & np.isfinite(y).all(axis=1)
    X, Y = x.astype(LD), y.astype(LD)
    X[~fin] = 0
    Y[~fin] = 0
    Px = _mv(pb.prow, pb.pcol, pb.Pv, X, n)
    aPx = _mv(pb.prow, pb.pcol, pb.Pv, X, n, absolute=True)
    q = pb.q.astype(LD)
    # objective (:547)
    o = np.sum(X * (LD(0.5) * Px + q), axis=1)
    oabs = np.sum(np.abs(X) * (LD(0.5) * aPx + np.abs(q)), axis=1)
    otol = _slack(n, oabs) + LD(1e-300)
    do = np.abs(obj.astype(LD) - o)
    fail(fin & ~(do <= otol), "objective != x.(Px/2 + q)")
    fail(~fin & np.isfinite(obj), "finite objective of a non-finite iterate")
    rep.ratio("objective", (do / otol)[fin])

    opt = (code == CODE_OPTIMAL) & fin
    fail((code == CODE_OPTIMAL) & ~fin, "non-finite Optimal result")
    if polish or not opt.any():
        return ok
    l, u = pb.l.astype(LD), pb.u.astype(LD)
    Ax = _mv(pb.arow, pb.acol, pb.Av, X, m)
    aAx = _mv(pb.arow, pb.acol, pb.Av, X, m, absolute=True)
    Aty = _mv(pb.acol, pb.arow, pb.Av, Y, n)
    aAty = _mv(pb.acol, pb.arow, pb.Av, Y, n, absolute=True)
    # primal: r = dist(Ax, [l, u])
    viol = np.maximum(np.maximum(l - Ax, Ax - u), LD(0))
    rsl = _slack(n, aAx) + LD(4 * EPS) * np.abs(Ax)
    r_max = (LD(eps_abs) + LD(eps_rel) * _ninf(Ax)) / (LD(1) - LD(eps_rel))
    pr = np.max(viol - rsl, axis=1, initial=LD(0)) / r_max
    fail(opt & (pr > 1), "primal residual above (eps_abs + eps_rel ||Ax||) / (1 - eps_rel)")
    rep.ratio("primal", pr[opt])
    # dual residual
    res = Px + q + Aty
    d_max = LD(eps_abs) + LD(eps_rel) * np.maximum(np.maximum(_ninf(Px), _ninf(q)), _ninf(Aty))
    dsl = _slack(n + m, np.max(aPx + np.abs(q) + aAty, axis=1, initial=LD(0)))
    dr = _ninf(res) / (d_max + dsl)
    fail(opt & (dr > 1), "dual residual above eps_abs + eps_rel max(||Px||, ||q||, ||A'y||)")
    rep.ratio("dual", dr[opt])
    # dual signs and complementarity
    arow1 = _mv(pb.arow, pb.acol, pb.Av, np.ones((pb.B, n), LD), m, absolute=True)
    tau = LD(1e-3) * d_max[:, None] / np.maximum(arow1, LD(1e-300))
    pos, neg = Y > tau, Y < -tau
    fail(opt & (pos & ~np.isfinite(pb.u)).any(axis=1), "y_i > tau on a row with u_i = +inf")
    fail(opt & (neg & ~np.isfinite(pb.l)).any(axis=1), "y_i < -tau on a row with l_i = -inf")
    lim = r_max[:, None] + rsl
    fail(opt & (pos & np.isfinite(pb.u) & (Ax < u - lim)).any(axis=1), "y_i > tau but (Ax)_i < u_i - r_max")
    fail(opt & (neg & np.isfinite(pb.l) & (Ax > l + lim)).any(axis=1), "y_i < -tau but (Ax)_i > l_i + r_max")
    return ok


# --------------------------------------------------------------------------------------------------------------------
# polish as an operation of its own
# --------------------------------------------------------------------------------------------------------------------
def _psym_dense(pb, b):
    """P of the polish KKT matrix: the upper triangle as stored, mirrored (:159-165 reads the upper part only)."""
    P = np.zeros((pb.n, pb.n))
    up = pb.prow <= pb.pcol
    np.add.at(P, (pb.prow[up], pb.pcol[up]), pb.Pv[b, up])
    return P + np.triu(P, 1).T


def _a_dense(pb, b, rows=None):
    A = np.zeros((pb.m, pb.n))
    np.add.at(A, (pb.arow, pb.acol), pb.Av[b])
    return A if rows is None else A[rows]


def _ruiz(prob, b, scaling):
    """The equilibration of QPSolver::scale (qp_solver.hpp:673-730) for item b: (sx, sy, c); ones without scaling.
    Needed to state polish in the solver's variables: its refinement (:193-195) runs a fixed number of steps in them."""
    n, m = prob.n, prob.m
    if not scaling:
        return np.ones(n), np.ones(m), 1.0
    Pv, Av = np.abs(prob.Pv[b]), np.abs(prob.Av[b])
    inc = np.zeros(n)
    np.maximum.at(inc, prob.pcol, Pv)
    inc[inc == 0] = 1.0
    c = 1.0 / max(1e-6, inc.sum() / n, np.abs(prob.q[b]).max(initial=0.0))
    sx, sy = np.ones(n), np.ones(m)
    for _ in range(11):                              # do { ... } while (iter++ < 10 && crit > 0.1)
        ix, iy = np.zeros(n), np.zeros(m)
        np.maximum.at(ix, prob.pcol, c * sx[prob.prow] * sx[prob.pcol] * Pv)
        t = sy[prob.arow] * sx[prob.acol] * Av
        np.maximum.at(ix, prob.acol, t)
        np.maximum.at(iy, prob.arow, t)
        ix[ix == 0] = 1.0
        iy[iy == 0] = 1.0
        sx = np.sqrt(1.0 / np.maximum(ix, 1e-8)) * sx
        sy = np.sqrt(1.0 / np.maximum(iy, 1e-8)) * sy
        if max(np.abs(ix - 1).max(initial=0.0), np.abs(iy - 1).max(initial=0.0)) <= 0.1:
            break
    return sx, sy, c


def _exact_kkt(K, rhs):
    """float64 solve plus two refinement steps with longdouble residuals; None when K is singular."""
    try:
        s = np.linalg.solve(K, rhs)
    except np.linalg.LinAlgError:
        return None
    KL = K.astype(LD)
    for _ in range(2):
        r = (rhs.astype(LD) - KL @ s.astype(LD)).astype(np.float64)
        s = s + np.linalg.solve(K, r)
    return s


def certify_polish(prob: Problem, res, res0, prm, rel_tol=1e-6, cond_max=1e8, items=None) -> Report:
    """Polish (qp_solver.hpp:92-204, :515-539) checked against the same batch solved with polish=False (res0):
    * code and iter equal (polish is post-processing);
    * S = rows whose dual changed, and every row whose scaled dual c |y0| / sy (_ruiz) exceeds 200 eps on the side of
      a finite bound -- the reference's test is 100 eps (:113-123); the factor 2 absorbs the rounding of recomputing
      the scaled dual.  A changed row whose scaled dual is below 50 eps fails.  (A row of the active set may keep its
      dual bit for bit: on LP vertices ADMM's dual can equal the polished dual exactly.)  Rows outside S keep the
      unpolished dual bit for bit, by the definition of S;
    * every row of S has a finite bound on the side of y0's sign (:113-123);
    * Optimal items: (x, y_S) equals polish_iter exact steps of the reference's refinement (:193-195)
      t <- t + Hp^-1 (h - H t), t = 0 at first, with H = [P A_S'; A_S 0] and h = [-q; b_S] (b = l where y0 < 0, u
      where y0 > 0) in the solver's scaled variables (_ruiz) and Hp = H + diag(delta I, -delta I) (:174-177), to
      max(rel_tol, 1e3 eps cond(H)): the reference's float64 LDL' solves carry about k eps cond(H) themselves.  The steps converge to the exact reduced KKT solution at the rate of Hp^-1 diag(delta, -delta); the
      reference stops after polish_iter of them and accepts what it has (:199-201) -- so on a slowly converging item
      (rows scaled by 1e4, a tiny dual pulling an inactive row into S) polish is not the KKT solution.  An
      H that is singular or has a condition number > cond_max (duplicate active rows) does not contract along its
      null space, where the reference's result is set by rounding: such items are skipped and counted;
    * polish_iter == 0: x == 0 and y_S == 0 exactly on Optimal items (t starts at 0 and is never updated).
    """
    code, it, x, y = (_get(res, k) for k in ("code", "iter", "x", "y"))
    code0, it0, x0, y0 = (_get(res0, k) for k in ("code", "iter", "x", "y"))
    B = prob.B
    rep = Report(ok=np.ones(B, bool))
    rep.fail(code != code0, "polish changed the status code")
    rep.fail(it != it0, "polish changed the iteration count")
    opt = (code == CODE_OPTIMAL) & (code0 == CODE_OPTIMAL)
    rep.fail((code != CODE_OPTIMAL) & ((x.view(np.uint64) != x0.view(np.uint64)).any(1) |
                                       (y.view(np.uint64) != y0.view(np.uint64)).any(1)), "polish ran on a non-Optimal item")
    polish_iter = int(_prm(prm, "polish_iter"))
    delta = f32(_prm(prm, "delta"))
    S = y.view(np.uint64) != y0.view(np.uint64)
    lfin, ufin = np.isfinite(prob.l), np.isfinite(prob.u)
    side_ok = ((y0 < 0) & lfin) | ((y0 > 0) & ufin)
    rep.fail(opt & (S & ~side_ok).any(1), "dual changed on a row without a finite bound on the side of y0's sign")
    checked = skipped = 0
    todo = np.flatnonzero(opt) if items is None else np.intersect1d(np.flatnonzero(opt), items)
    worst = []
    for b in todo:
        sx, sy, c = _ruiz(prob, b, bool(_prm(prm, "scaling")))
        sd = c * np.abs(y0[b]) / sy                  # |scaled dual|: the polish set is where it exceeds 100 eps (:113-123)
        if (S[b] & (sd < 50 * EPS)).any():
            rep.fail(np.arange(B) == b, "dual changed on a row below the polish threshold")
        rows = np.flatnonzero(S[b] | (side_ok[b] & (sd > 200 * EPS)))
        if polish_iter == 0:
            good = (x[b] == 0).all() and (y[b, rows] == 0).all()
            if not good:
                rep.fail(np.arange(B) == b, "polish_iter = 0 but x or y_S != 0")
            checked += 1
            continue
        n, ns = prob.n, rows.size
        P, AS = _psym_dense(prob, b), _a_dense(prob, b, rows)
        bS = np.where(y0[b, rows] < 0, prob.l[b, rows], prob.u[b, rows])
        if not np.isfinite(bS).all():
            rep.fail(np.arange(B) == b, "polish row with an infinite bound")
            continue
        # the reduced system in the solver's scaled variables (:159-182)
        H = np.zeros((n + ns, n + ns))
        H[:n, :n] = c * sx[:, None] * P * sx[None, :]
        H[n:, :n] = sy[rows, None] * AS * sx[None, :]
        H[:n, n:] = H[n:, :n].T
        h = np.r_[-c * sx * prob.q[b], sy[rows] * bS]
        Hp = H + np.diag(np.r_[np.full(n, delta), np.full(ns, -delta)])
        condH = np.linalg.cond(H)
        if not condH <= cond_max:         # along a (near) null space of H the steps do not contract and
            skipped += 1                              # the result is set by rounding (duplicate active rows)
            continue
        t = np.zeros(n + ns)
        for _ in range(polish_iter):                 # :193-195, each step solved exactly
            t = t + _exact_kkt(Hp, (h.astype(LD) - H.astype(LD) @ t.astype(LD)).astype(np.float64))
        sol = np.r_[sx * t[:n], sy[rows] * t[n:] / c]
        got = np.r_[x[b], y[b, rows]]
        err = np.abs(got - sol).max() / max(np.abs(sol).max(), 1e-12)
        tol = max(rel_tol, 1e3 * EPS * condH)       # float64 LDL' solves (:187-188) carry ~k eps cond(H), k <= 1e3
        worst.append(err / tol * rel_tol)
        if not err <= tol:
            rep.fail(np.arange(B) == b, "polished (x, y_S) != polish_iter exact refinement steps (rel %.3g)" % err)
        checked += 1
    rep.ratio("polish_kkt_rel", np.asarray(worst) / rel_tol)
    rep.counts = {"items": B, "optimal": int(opt.sum()), "polish_checked": checked, "polish_skipped": skipped}
    return rep


# --------------------------------------------------------------------------------------------------------------------
# one batch through a solver: both polish settings, every certificate
# --------------------------------------------------------------------------------------------------------------------
@dataclass
class Params:
    """QPSolverParams (qp_solver.hpp:29-68) for both the product and the oracle."""
    alpha: float = 1.6
    rho: float = 0.1
    sigma: float = 1e-6
    scaling: bool = True
    eps_abs: float = 1e-3
    eps_rel: float = 1e-3
    eps_primal_inf: float = 1e-4
    eps_dual_inf: float = 1e-4
    max_iter: int = 20000
    stop_check_iter: int = 25
    polish: bool = True
    polish_iter: int = 5
    delta: float = 1e-6
    reuse_factor: bool = False

    def but(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Params(**d)

    def sfb(self, sfb):
        return sfb.QPSolverParams(**{k: v for k, v in self.__dict__.items()})

    def oracle(self, O):
        d = {k: (int(v) if isinstance(v, bool) else v) for k, v in self.__dict__.items() if k != "reuse_factor"}
        return O.default_params(**d)


def solve_and_certify(solve, prob: Problem, prm: Params, verdict=None, min_polish_share=0.0, family=None):
    """solve(prm) -> result.  Solves with polish off and on, certifies both, polish as an operation, and the family's
    verdict.  Returns (polished result, unpolished result, summary dict); raises AssertionError with the reasons."""
    from qp_families import verdict_ok
    r0 = solve(prm.but(polish=False))
    r1 = solve(prm.but(polish=True))
    reps = [certify(prob, r0, prm.but(polish=False)), certify(prob, r1, prm.but(polish=True)),
            certify_polish(prob, r1, r0, prm)]
    msgs = [str(r) for r in reps if not r.passed]
    if verdict is not None:
        bad = ~verdict_ok(verdict, _get(r0, "code"), prm, family)
        if bad.any():
            msgs.append("%s family: codes %s at items %s" % (verdict, _get(r0, "code")[bad][:8].tolist(),
                                                            np.flatnonzero(bad)[:8].tolist()))
    pc = reps[2].counts
    if prm.polish_iter and pc["optimal"] and pc["polish_checked"] < min_polish_share * pc["optimal"]:
        msgs.append("polish checked on %d of %d Optimal items" % (pc["polish_checked"], pc["optimal"]))
    summary = dict(codes=np.bincount(_get(r0, "code"), minlength=7).tolist(), **{k: v for k, v in pc.items() if k != "items"},
                   worst={**reps[0].worst, **reps[2].worst})
    assert not msgs, "; ".join(msgs)
    return r1, r0, summary
