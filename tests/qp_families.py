"""QP families whose verdict is known from their construction (test data for tests/qp_certify.py).

Every family returns dense batches in the layout of solve_qp_batch_host (flat col-major P (B, n*n), A (B, m*n)) and the
verdict class the construction fixes:

* "feasible": an interior point x0 with slack >= 0.1 on every inequality side, consistent equalities, free rows, and
  a bounded objective (P positive definite, or every variable boxed around x0 when P is zero / rank-deficient).
  Optimal is expected; PrimalInfeasible / DualInfeasible are wrong.
* "infeasible": a feasible family plus rows that contradict each other by a margin of 2 (a.x <= -1 and a.x >= 1) or a
  zero row whose box [1, 2] misses 0.  Margins are absolute: the reference's certificates (qp_solver.hpp:598-641)
  are not invariant under row scaling, so a row scaled by 1e4 gets a slack scaled with it, a row scaled by 1e-4 keeps
  a slack of 0.1, not 1e-5, and equality rows are never scaled down (a tolerance of eps_primal_inf = 1e-4 on a row of norm 1e-4 cannot tell b = 1e-5 from 0).  Bounds of +-1e20 are kept out of these families: the infeasibility test
  (qp_solver.hpp:598-621) adds u_i * max(0, dy_i), which a bound of 1e20 makes large.
* "unbounded": P = 0 or rank-deficient, a direction d with P d = 0, A d = 0 and q.d = -||d|| (margin 1 per unit step),
  and a feasible x0.

Edges mixed in by `feasible(..., edges)`: P = 0 / rank-deficient, equality-only, one-sided and free rows, zero rows and
zero columns of A, duplicate rows, rows scaled by 1e+-4, finite bounds of +-1e20 next to +-inf.
"""
import numpy as np

EDGES = ("zero_rows", "zero_cols", "dup_rows", "row_scale", "big_bounds")


def _colmajor(M):
    return np.ascontiguousarray(np.transpose(M, (0, 2, 1)).reshape(M.shape[0], -1))


def _P(rng, B, n, rank):
    if rank == 0:
        return np.zeros((B, n, n))
    M = rng.standard_normal((B, n, rank))
    return M @ np.transpose(M, (0, 2, 1)) / max(1, rank) + (1e-1 * np.eye(n) if rank >= n else 0.0)


def feasible(rng, B, n, m, rank=None, edges=(), density=0.7, box=None):
    """-> (P, q, A, l, u) flat col-major, feasible with a margin and bounded.  rank: of P (None = n, positive definite).
    box: append identity rows with finite bounds around x0 (default: when P is not positive definite)."""
    rank = n if rank is None else rank
    box = (rank < n) if box is None else box
    P = _P(rng, B, n, rank)
    A = rng.standard_normal((B, m, n)) * (rng.random((B, m, n)) < density)
    if "zero_cols" in edges and n > 1:
        A[:, :, rng.integers(0, n)] = 0.0
    if "zero_rows" in edges and m > 2:
        A[:, rng.integers(0, m, 2), :] = 0.0
    kind = rng.integers(0, 5, (B, m))       # 0 two-sided, 1 equality, 2 upper only, 3 lower only, 4 free
    g = np.ones((B, m))                     # margin factor of a row
    if "row_scale" in edges:                # 1e+4 on any row (margin scaled with it), 1e-4 on inequality rows (margin kept)
        s = 10.0 ** rng.choice([-4.0, 0.0, 4.0], (B, m))
        s = np.where((s < 1) & (kind == 1), 1.0, s)
        A, g = A * s[:, :, None], np.maximum(s, 1.0)
    if "dup_rows" in edges and m > 3:
        A[:, m - 1], kind[:, m - 1] = A[:, 0], kind[:, 0]
        A[:, m - 2], kind[:, m - 2] = A[:, 1], kind[:, 1]
    x0 = rng.uniform(-1, 1, (B, n))
    Ax0 = np.einsum("bij,bj->bi", A, x0)
    lo = Ax0 - g * (0.1 + rng.random((B, m)))
    hi = Ax0 + g * (0.1 + rng.random((B, m)))
    if "dup_rows" in edges and m > 3:       # the same row twice with the same (consistent) bounds
        lo[:, m - 1], hi[:, m - 1] = lo[:, 0], hi[:, 0]
        lo[:, m - 2], hi[:, m - 2] = lo[:, 1], hi[:, 1]
    l = np.where(kind == 1, Ax0, np.where((kind == 2) | (kind == 4), -np.inf, lo))
    u = np.where(kind == 1, Ax0, np.where((kind == 3) | (kind == 4), np.inf, hi))
    zero = ~A.any(axis=2)                   # a zero row is feasible iff its box holds 0: margin 0.1 around it
    l = np.where(zero & np.isfinite(l), np.minimum(l, -0.1), l)
    u = np.where(zero & np.isfinite(u), np.maximum(u, 0.1), u)
    if "big_bounds" in edges:
        w = rng.random((B, m))
        l = np.where((w < 0.3) & ~np.isfinite(l), -1e20, l)
        u = np.where((w > 0.7) & ~np.isfinite(u), 1e20, u)
    if box:
        A = np.concatenate([A, np.broadcast_to(np.eye(n), (B, n, n))], axis=1)
        l = np.concatenate([l, x0 - 1.0], axis=1)
        u = np.concatenate([u, x0 + 1.0], axis=1)
    q = rng.standard_normal((B, n))
    return _colmajor(P), q, _colmajor(A), l, u


def infeasible(rng, B, n, m, rank=None, density=0.7, how="pair"):
    """A feasible family (m - 2 rows) plus two contradicting rows, or a zero row whose box [1, 2] misses 0."""
    P, q, A, l, u = feasible(rng, B, n, m - 2, rank=rank, density=density)
    mm = l.shape[1]
    A = np.transpose(A.reshape(B, n, mm), (0, 2, 1))
    if how == "pair":
        a = rng.standard_normal((B, 1, n))
        a /= np.abs(a).sum(axis=2, keepdims=True)
        A = np.concatenate([A, a, a], axis=1)
        l = np.concatenate([l, np.full((B, 1), -np.inf), np.ones((B, 1))], axis=1)
        u = np.concatenate([u, -np.ones((B, 1)), np.full((B, 1), np.inf)], axis=1)
    else:
        A = np.concatenate([A, np.zeros((B, 2, n))], axis=1)
        l = np.concatenate([l, np.ones((B, 1)), np.full((B, 1), -np.inf)], axis=1)
        u = np.concatenate([u, 2 * np.ones((B, 1)), np.full((B, 1), np.inf)], axis=1)
    return P, q, _colmajor(A), l, u


def unbounded(rng, B, n, m, rank=0, density=0.7):
    """P of rank < n (0: an LP), d in the null space of P with A d = 0 and q.d = -||d||_2, a feasible x0."""
    assert rank < n
    M = rng.standard_normal((B, n, max(rank, 1)))
    d = rng.standard_normal((B, n))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    proj = np.eye(n) - d[:, :, None] * d[:, None, :]
    M = proj @ M if rank > 0 else M * 0.0
    P = M @ np.transpose(M, (0, 2, 1))
    A = (rng.standard_normal((B, m, n)) * (rng.random((B, m, n)) < density)) @ proj
    x0 = rng.uniform(-1, 1, (B, n))
    Ax0 = np.einsum("bij,bj->bi", A, x0)
    kind = rng.integers(0, 4, (B, m))
    l = np.where(kind == 1, Ax0, np.where(kind == 2, -np.inf, Ax0 - 0.1 - rng.random((B, m))))
    u = np.where(kind == 1, Ax0, np.where(kind == 3, np.inf, Ax0 + 0.1 + rng.random((B, m))))
    q = rng.standard_normal((B, n))
    q -= (np.einsum("bj,bj->b", q, d) + 1.0)[:, None] * d
    return _colmajor(P), q, _colmajor(A), l, u


FAMILIES = {
    # name: (verdict, builder(rng, B, n, m))
    "pd_mixed": ("feasible", lambda r, B, n, m: feasible(r, B, n, m)),
    "pd_edges": ("feasible", lambda r, B, n, m: feasible(r, B, n, m, edges=EDGES)),
    "lp_boxed": ("feasible", lambda r, B, n, m: feasible(r, B, n, m, rank=0, edges=("zero_cols",))),
    "rankdef_scaled": ("feasible", lambda r, B, n, m: feasible(r, B, n, m, rank=max(1, n // 2), edges=("row_scale", "zero_rows"))),
    "infeasible_pair": ("infeasible", lambda r, B, n, m: infeasible(r, B, n, max(m, 3), how="pair")),
    "infeasible_zero_row": ("infeasible", lambda r, B, n, m: infeasible(r, B, n, max(m, 3), how="zero_row")),
    "unbounded_lp": ("unbounded", lambda r, B, n, m: unbounded(r, B, n, m, rank=0)),
    "unbounded_rankdef": ("unbounded", lambda r, B, n, m: unbounded(r, B, n, m, rank=max(1, n // 2)) if n > 1
                          else unbounded(r, B, n, m, rank=0)),
}


def build(name, B, n, m, seed):
    verdict, fn = FAMILIES[name]
    P, q, A, l, u = fn(np.random.default_rng(seed), B, n, m)
    return verdict, (P, q, A, l, u)


ROW_SCALED = ("pd_edges", "rankdef_scaled")   # families with rows scaled by 1e+-4


def verdict_ok(verdict, code, prm, family=None):
    """Codes a family's verdict admits; `verdict` may be one class or one per item.  With stop_check_iter < 2 no
    stopping check runs (qp_solver.hpp:465, :479 test iter % stop_check_iter == 1), so only max_iter can end the solve.
    Without scaling the verdict of a family with rows scaled by 1e+-4 is not asserted: the certificates of
    qp_solver.hpp:598-621 and :625-641 compare ||A'dy|| and A dx with eps_*_inf times the norms of the UNSCALED dy and
    dx, so a row of norm 1e-4 meets the primal infeasibility test with any dy on it, and a feasible family of that kind
    was called PrimalInfeasible (seen in the oracle, which follows those lines)."""
    code = np.asarray(code)
    if int(prm.stop_check_iter) < 2:
        return code == 4
    if not prm.scaling and family in ROW_SCALED:
        return np.ones(code.shape, bool)
    feas = np.broadcast_to(np.asarray(verdict), code.shape) == "feasible"
    return np.where(feas, (code != 2) & (code != 3), (code == 2) | (code == 3))


def linprog_confirms(P, q, A, l, u, n, m, code):
    """Oracle-free cross-check of one code-2 / code-3 verdict with scipy.optimize.linprog (HiGHS).
    Code 2: the least box violation min sum(s) s.t. l - s <= A x <= u + s, s >= 0 is > 0.
    Code 3: the recession LP min q.d s.t. P d = 0, A d in the recession cone of [l, u], |d| <= 1 has q.d < 0."""
    from scipy.optimize import linprog
    Pm = np.asarray(P).reshape(n, n).T
    Am = np.asarray(A).reshape(n, m).T
    big = 1e19
    if code == 2:
        c = np.r_[np.zeros(n), np.ones(m)]
        rows, rhs = [], []
        for i in range(m):
            if u[i] < big:
                rows.append(np.r_[Am[i], -np.eye(m)[i]]); rhs.append(u[i])
            if l[i] > -big:
                rows.append(np.r_[-Am[i], -np.eye(m)[i]]); rhs.append(-l[i])
        r = linprog(c, A_ub=np.array(rows), b_ub=np.array(rhs), bounds=[(None, None)] * n + [(0, None)] * m,
                    method="highs")
        return r.status == 0 and r.fun > 1e-6
    A_eq = [Pm] + [Am[i:i + 1] for i in range(m) if u[i] < big and l[i] > -big]
    A_ub = [Am[i:i + 1] for i in range(m) if u[i] < big and l[i] <= -big] + \
           [-Am[i:i + 1] for i in range(m) if l[i] > -big and u[i] >= big]
    r = linprog(q, A_eq=np.vstack(A_eq), b_eq=np.zeros(sum(a.shape[0] for a in A_eq)),
                A_ub=np.vstack(A_ub) if A_ub else None, b_ub=np.zeros(len(A_ub)) if A_ub else None,
                bounds=[(-1, 1)] * n, method="highs")
    return r.status == 0 and r.fun < -1e-6
