"""CPU reference of the swarm SQP solver ("Swarm SQP"): the law in numpy float64, in the summation orders the
law states, one agent at a time.  It restates the NEW code (pattern work, assembly, stopping test, ladder, line search), not
the QP solver: a QP is solved by the CPU oracle's dense solver on the densified QP with the same parameters.  Wave-reduced
quantities (v1, d.d, d.P d) have no fixed order on the device; here they are np.longdouble sums with the absolute terms next
to them, for the 4 (k + 2) eps slack of tests/qp_certify.py.  Also the test problems: a pattern zoo, HS71 and the
reference's double-integrator OCP as term tables of tests/ocpnlp_ref.py."""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
RUNNING, OPTIMAL, PRIMAL_INFEASIBLE, MAX_ITERATIONS, UNKNOWN = -1, 0, 1, 3, 5
INF = np.inf


def slack(k, absterms):
    return LD(4 * (k + 2)) * LD(EPS) * LD(absterms)


# ---------------------------------------------------------------------------------------------------------------------
# pattern work, restated through dense index matrices (nothing of the builder's counting passes)
# ---------------------------------------------------------------------------------------------------------------------
def qp_pattern_ref(n, m, Jp, Jj, Hp, Hi, xl, xu, gl, gu):
    Jp, Jj, Hp, Hi = [np.asarray(a, np.int64) for a in (Jp, Jj, Hp, Hi)]
    nnzJ, nnzH = int(Jp[m]), int(Hp[n])
    slotH = -np.ones((n, n), np.int64)       # Hessian slot of every entry of the symmetric matrix
    for c in range(n):
        for p in range(Hp[c], Hp[c + 1]):
            slotH[Hi[p], c] = slotH[c, Hi[p]] = p
    P_colptr, P_rowind, P_src, P_diag = [0], [], [], []
    for c in range(n):
        for r in range(n):
            if slotH[r, c] >= 0:
                if r == c:
                    P_diag.append(len(P_rowind))
                P_rowind.append(r)
                P_src.append(slotH[r, c])
        P_colptr.append(len(P_rowind))
    slotJ = -np.ones((max(m, 1), n), np.int64)
    for r in range(m):
        for p in range(Jp[r], Jp[r + 1]):
            slotJ[r, Jj[p]] = p
    Jc_colptr, Jc_row, Jc_pos = [0], [], []
    for c in range(n):
        for r in range(m):
            if slotJ[r, c] >= 0:
                Jc_row.append(r)
                Jc_pos.append(slotJ[r, c])
        Jc_colptr.append(len(Jc_row))
    bound_var = [j for j in range(n) if np.isfinite(xl[j]) or np.isfinite(xu[j])]
    nb = len(bound_var)
    A_rowptr = list(Jp[:m + 1]) + [nnzJ + i + 1 for i in range(nb)]
    A_colind = list(Jj[:nnzJ]) + bound_var
    i32 = lambda a: np.asarray(a, np.int32)                                         # noqa: E731
    return dict(nb=nb, A_rowptr=i32(A_rowptr), A_colind=i32(A_colind), P_colptr=i32(P_colptr), P_rowind=i32(P_rowind), P_src=i32(P_src),
                P_diag=i32(P_diag), Jc_colptr=i32(Jc_colptr), Jc_row=i32(Jc_row), Jc_pos=i32(Jc_pos), bound_var=i32(bound_var),
                nnzJ=nnzJ, nnzH=nnzH, nnzP=len(P_rowind))


class Problem:
    """Patterns and bounds shared by a swarm, with the reference's pattern work."""

    def __init__(self, n, m, Jp, Jj, Hp, Hi, xl, xu, gl, gu):
        self.n, self.m = int(n), int(m)
        self.Jp, self.Jj, self.Hp, self.Hi = [np.ascontiguousarray(a, np.int32) for a in (Jp, Jj, Hp, Hi)]
        self.xl, self.xu, self.gl, self.gu = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (xl, xu, gl, gu)]
        self.pat = qp_pattern_ref(self.n, self.m, self.Jp, self.Jj, self.Hp, self.Hi, self.xl, self.xu, self.gl, self.gu)
        self.nb, self.mq = self.pat["nb"], self.m + self.pat["nb"]
        self.nnzJ, self.nnzH, self.nnzP, self.nnzA = self.pat["nnzJ"], self.pat["nnzH"], self.pat["nnzP"], self.pat["nnzJ"] + self.pat["nb"]
        self.P_col = np.repeat(np.arange(self.n), np.diff(self.pat["P_colptr"]))
        self.A_row = np.repeat(np.arange(self.mq), np.diff(self.pat["A_rowptr"]))

    def args(self):
        return (self.n, self.m, self.Jp, self.Jj, self.Hp, self.Hi, self.xl, self.xu, self.gl, self.gu)


# ---------------------------------------------------------------------------------------------------------------------
# law 1: the QP of an agent
# ---------------------------------------------------------------------------------------------------------------------
def assemble_ref(pb, x, mu, df, g, dg, hess):
    """one agent -> Px [nnzP], q [n], Ax [nnzA], l, u [mq]: copies, one add on the diagonal, one subtraction per bound"""
    pat = pb.pat
    Px = np.asarray(hess, np.float64)[pat["P_src"]].copy()
    Px[pat["P_diag"]] = Px[pat["P_diag"]] + mu
    bv = pat["bound_var"]
    with np.errstate(invalid="ignore"):
        l = np.concatenate([pb.gl - g, pb.xl[bv] - x[bv]])
        u = np.concatenate([pb.gu - g, pb.xu[bv] - x[bv]])
    return Px, np.array(df, np.float64), np.concatenate([np.asarray(dg, np.float64), np.ones(pb.nb)]), l, u


def dense_qp(pb, Px, Ax):
    P = np.zeros((pb.n, pb.n))
    P[pb.pat["P_rowind"], pb.P_col] = Px
    A = np.zeros((pb.mq, pb.n))
    A[pb.A_row, pb.pat["A_colind"]] = Ax
    return P, A


# ---------------------------------------------------------------------------------------------------------------------
# law 4: the stopping test
# ---------------------------------------------------------------------------------------------------------------------
def _comp(mult, v, lo, hi):
    fl, fh = np.isfinite(lo), np.isfinite(hi)
    if fl and fh:
        return 0.0 if lo == hi else abs(mult) * min(v - lo, hi - v)
    if fl:
        return abs(mult) * (v - lo)
    if fh:
        return abs(mult) * (hi - v)
    return 0.0


def kkt_ref(pb, x, lam, z, df, g, dg):
    """one agent -> (r_stat, r_pri, r_comp) float64 in the law's order; (v1, sum of |terms|, terms) in longdouble"""
    pat = pb.pat
    rs = rp = rc = 0.0
    for c in range(pb.n):
        s = np.float64(df[c])
        for t in range(pat["Jc_colptr"][c], pat["Jc_colptr"][c + 1]):
            s = s + np.float64(dg[pat["Jc_pos"][t]]) * np.float64(lam[pat["Jc_row"][t]])
        s = s + np.float64(z[c])
        rs = np.fmax(rs, abs(s))
        rp = np.fmax(rp, np.fmax(pb.xl[c] - x[c], x[c] - pb.xu[c]))
        rc = np.fmax(rc, _comp(z[c], x[c], pb.xl[c], pb.xu[c]))
    for r in range(pb.m):
        rp = np.fmax(rp, np.fmax(pb.gl[r] - g[r], g[r] - pb.gu[r]))
        rc = np.fmax(rc, _comp(lam[r], g[r], pb.gl[r], pb.gu[r]))
    return float(rs), float(rp), float(rc)


def v1_ref(pb, g):
    g = np.asarray(g, LD)
    terms = np.maximum(LD(0), pb.gl.astype(LD) - g) + np.maximum(LD(0), g - pb.gu.astype(LD)) if pb.m else np.zeros(0, LD)
    return terms.sum(dtype=LD), np.abs(terms).sum(dtype=LD), 2 * pb.m


def judge_sums_ref(pb, Px, d):
    """d.d and d.P d (upper triangle, off-diagonal entries twice) in longdouble, with the sums of absolute terms and term counts"""
    d = np.asarray(d, LD)
    dd, k_dd = (d * d).sum(dtype=LD), pb.n
    r, c = pb.pat["P_rowind"], pb.P_col
    up = r <= c
    w = np.where(r == c, LD(1), LD(2))[up]
    terms = np.asarray(Px, LD)[up] * d[r[up]] * d[c[up]] * w
    return dd, dd, k_dd, terms.sum(dtype=LD), np.abs(terms).sum(dtype=LD), int(up.sum())


# ---------------------------------------------------------------------------------------------------------------------
# law 3: the step, as pure functions of one agent (solve_ref below calls them: there is one statement of the law)
# ---------------------------------------------------------------------------------------------------------------------
ARMIJO, HALVINGS = 1e-4, 10


def step_start_ref(pb, f, df, g, d, y, nu_prev):
    """the part of law 3 that does not depend on alpha -> (nu, phi0, D, dfd, absdfd, k): nu the running maximum over the m
    constraint rows of y (one multiply, one max), phi0 = f + nu v1(g), D = df.d - nu v1(g) in float64; df.d once more in
    longdouble with the sum of its absolute terms and its term count, for the slack of a wave-reduced sum"""
    nu = max(nu_prev, 1.1 * float(np.max(np.abs(np.asarray(y)[:pb.m]), initial=0.0)))
    v = float(v1_ref(pb, g)[0])
    terms = np.asarray(df, LD) * np.asarray(d, LD)
    return nu, f + nu * v, float(np.dot(df, d)) - nu * v, terms.sum(dtype=LD), np.abs(terms).sum(dtype=LD), pb.n


def trial_ref(pb, x, d, alpha):
    return np.fmin(np.fmax(x + alpha * d, pb.xl), pb.xu)


def accept_ref(pb, state, ft, gt, mu_first=1e-4):
    """one trial point of a searching agent.  state: x, lam, z, mu, nu, alpha, iter, status and, of the open search, d, y (the
    accepted QP solution, mq rows), phi0, D, halvings, searching.  -> the new state: committed (Armijo on the l1 merit; a merit
    that is not finite -- a NaN or infinite ft or entry of gt -- is a rejection), halved, or Unknown after the tenth halving
    was rejected too, with alpha left at 2^-10 and nothing else touched.  An agent that is not searching is returned as it is."""
    s = dict(state)
    if not s["searching"]:
        return s
    alpha = s["alpha"]
    with np.errstate(invalid="ignore", over="ignore"):
        phit = ft + s["nu"] * float(v1_ref(pb, gt)[0])
        ok = bool(np.isfinite(phit)) and bool(phit <= s["phi0"] + ARMIJO * alpha * s["D"])
    if ok:
        zq = np.zeros(pb.n)
        zq[pb.pat["bound_var"]] = np.asarray(s["y"])[pb.m:]
        s["x"] = trial_ref(pb, s["x"], s["d"], alpha)
        s["lam"] = s["lam"] + alpha * (np.asarray(s["y"])[:pb.m] - s["lam"])
        s["z"] = s["z"] + alpha * (zq - s["z"])
        s["mu"] = s["mu"] / 4.0 if s["mu"] > mu_first else 0.0
        s["iter"], s["searching"] = s["iter"] + 1, False
    elif s["halvings"] + 1 > HALVINGS:
        s["status"], s["searching"] = UNKNOWN, False
    else:
        s["halvings"], s["alpha"] = s["halvings"] + 1, alpha / 2.0
    return s


# ---------------------------------------------------------------------------------------------------------------------
# the whole law for one agent
# ---------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(tol=1e-6, max_iter=50, kappa=1e-8, mu_first=1e-4, mu_grow=8.0, mu_max=1e4)
QP_DEFAULTS = dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=10000)


def solve_ref(pb, evaluate, x0, oracle, lam0=None, z0=None, qp=None, history=None, **kw):
    """evaluate(x, lam, want_derivatives) for ONE agent -> (f, g) or (f, g, df, dg_val, hess_val).  -> dict of the final state.
    history (a list, optional) receives (iter, r_stat, r_pri, r_comp, mu, alpha, qp_solves) per direction call."""
    prm = dict(DEFAULTS, **kw)
    qprm = oracle.default_params(**dict(QP_DEFAULTS, **(qp or {})))
    n, m, mq = pb.n, pb.m, pb.mq
    x = np.array(x0, np.float64)
    lam = np.zeros(m) if lam0 is None else np.array(lam0, np.float64)
    z = np.zeros(n) if z0 is None else np.array(z0, np.float64)
    mu = nu = alpha = 0.0
    it, status, solves = 0, RUNNING, 0
    wd, wy = np.zeros(n), np.zeros(mq)
    res = (0.0, 0.0, 0.0)
    while True:
        f, g, df, dg, hess = evaluate(x, lam, True)
        res = kkt_ref(pb, x, lam, z, df, g, dg)                                     # law 4
        finite = np.all(np.isfinite(g)) and np.all(np.isfinite(x)) and np.isfinite(res[0])
        if history is not None:
            history.append((it, *res, mu, alpha, solves))
        if finite and max(res) <= prm["tol"]:
            status = OPTIMAL
            break
        if it >= prm["max_iter"]:
            status = MAX_ITERATIONS
            break
        rung = 0
        while True:                                                                 # laws 1 and 2
            Px, q, Ax, l, u = assemble_ref(pb, x, mu, df, g, dg, hess)
            P, A = dense_qp(pb, Px, Ax)
            r = oracle.qp_dense_solve_batch(oracle.colmajor(P)[None], q[None], oracle.colmajor(A)[None], l[None], u[None], params=qprm,
                                            warm_x=wd[None], warm_y=wy[None])
            solves += 1
            d, y, code = r["x"][0], r["y"][0], int(r["code"][0])
            ok = code == 0 and np.all(np.isfinite(d)) and np.all(np.isfinite(y))
            if ok and np.any(d != 0.0):
                dd, _, _, dPd, _, _ = judge_sums_ref(pb, Px, d)
                ok = bool(dPd >= LD(prm["kappa"]) * dd)
            if ok:
                break
            if code == 2 and rung == 0:
                status = PRIMAL_INFEASIBLE
                break
            mu = max(prm["mu_first"], prm["mu_grow"] * mu)
            if mu > prm["mu_max"]:
                status = UNKNOWN
                break
            rung += 1
        if status != RUNNING:
            break
        wd, wy = d.copy(), y.copy()
        nu, phi0, D = step_start_ref(pb, f, df, g, d, y, nu)[:3]                    # law 3
        st = dict(x=x, lam=lam, z=z, mu=mu, nu=nu, alpha=1.0, iter=it, status=RUNNING, d=d, y=y, phi0=phi0, D=D, halvings=0, searching=True)
        while st["searching"]:
            ft, gt = evaluate(trial_ref(pb, st["x"], d, st["alpha"]), lam, False)[:2]
            st = accept_ref(pb, st, ft, gt, prm["mu_first"])
        x, lam, z, mu, alpha, it, status = [st[k] for k in ("x", "lam", "z", "mu", "alpha", "iter", "status")]
        if status != RUNNING:
            break
    return dict(x=x, lam=lam, z=z, status=status, iter=it, r_stat=res[0], r_pri=res[1], r_comp=res[2], mu=mu, alpha=alpha, nu=nu,
                qp_solves=solves)


# ---------------------------------------------------------------------------------------------------------------------
# an independent KKT certificate in longdouble (nothing of kkt_ref's loops): the three residuals of a claimed solution
# ---------------------------------------------------------------------------------------------------------------------
def certify_kkt(pb, x, lam, z, df, g, dg):
    J = np.zeros((pb.m, pb.n), LD)
    rows = np.repeat(np.arange(pb.m), np.diff(pb.Jp))
    J[rows, pb.Jj] = np.asarray(dg, LD)
    x, lam, z, g = [np.asarray(a, LD) for a in (x, lam, z, g)]
    stat = np.max(np.abs(np.asarray(df, LD) + J.T @ lam + z), initial=LD(0))
    lo, hi = np.concatenate([pb.gl, pb.xl]).astype(LD), np.concatenate([pb.gu, pb.xu]).astype(LD)
    v, mult = np.concatenate([g, x]), np.concatenate([lam, z])
    pri = np.max(np.concatenate([[LD(0)], lo - v, v - hi]))
    with np.errstate(invalid="ignore"):
        dist = np.minimum(np.where(np.isfinite(lo), v - lo, LD(INF)), np.where(np.isfinite(hi), hi - v, LD(INF)))
    take = np.isfinite(dist) & (lo != hi)
    comp = np.max(np.abs(mult[take]) * dist[take], initial=LD(0))
    return float(stat), float(pri), float(comp)


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------
def dense_patterns(n, m):
    Jp = np.arange(0, m * n + 1, n, dtype=np.int32)
    Jj = np.tile(np.arange(n, dtype=np.int32), m)
    Hp = np.concatenate([[0], np.cumsum(np.arange(1, n + 1))]).astype(np.int32)
    Hi = np.concatenate([np.arange(c + 1) for c in range(n)]).astype(np.int32)
    return Jp, Jj, Hp, Hi


def random_problem(seed, n, m, jac_density=0.4, hess_density=0.3, bounded=0.5, empty_rows=(), empty_cols=()):
    """random patterns (every Hessian diagonal present) and bounds with infinite sides, equalities and ranges"""
    rng = np.random.default_rng(seed)
    Jmask = rng.random((m, n)) < jac_density
    Jmask[list(empty_rows), :] = False
    Jmask[:, list(empty_cols)] = False
    Hmask = np.triu(rng.random((n, n)) < hess_density) | np.eye(n, dtype=bool)
    Jp = np.concatenate([[0], np.cumsum(Jmask.sum(1))]).astype(np.int32)
    Jj = np.concatenate([np.nonzero(r)[0] for r in Jmask] + [np.zeros(0, np.int64)]).astype(np.int32)
    Hp = np.concatenate([[0], np.cumsum(Hmask.sum(0))]).astype(np.int32)
    Hi = np.concatenate([np.nonzero(Hmask[:, c])[0] for c in range(n)]).astype(np.int32)

    def bounds(k, share):
        lo, hi = -1.0 - rng.random(k), 1.0 + rng.random(k)
        kind = rng.random(k)
        lo[kind < 0.25], hi[(kind >= 0.25) & (kind < 0.5)] = -INF, INF
        eq = (kind >= 0.5) & (kind < 0.6)
        hi[eq] = lo[eq]
        free = rng.random(k) >= share
        lo[free], hi[free] = -INF, INF
        return lo, hi
    xl, xu = bounds(n, bounded)
    gl, gu = bounds(m, 0.9)
    return Problem(n, m, Jp, Jj, Hp, Hi, xl, xu, gl, gu)


def zoo():
    """(name, Problem): the sizes and corner cases of the issue -- n in {1, 4, 63, 64, 65, 130}, m = 0 with bounds, no bounds with
    m >= 1, every variable bounded, empty Jacobian rows, an empty column"""
    out = []
    for k, n in enumerate((1, 4, 63, 64, 65, 130)):
        out.append(("n%d" % n, random_problem(100 + k, n, max(1, n // 2))))
    out.append(("m0", random_problem(7, 9, 0, bounded=1.0)))
    out.append(("nb0", random_problem(8, 9, 5, bounded=0.0)))
    p = random_problem(9, 12, 6, bounded=1.0)
    p = Problem(p.n, p.m, p.Jp, p.Jj, p.Hp, p.Hi, np.where(np.isfinite(p.xl) | np.isfinite(p.xu), p.xl, -2.0), p.xu, p.gl, p.gu)
    out.append(("allbounded", p))
    out.append(("emptyrows", random_problem(10, 10, 7, empty_rows=(0, 3, 6))))
    out.append(("emptycol", random_problem(11, 10, 7, empty_cols=(0, 4, 9))))
    return out


# HS71: min x0 x3 (x0 + x1 + x2) + x2  s.t.  x0 x1 x2 x3 >= 25,  |x|^2 = 40,  1 <= x <= 5;  f* = 17.0140173
HS71_F = 17.0140173
HS71_START = np.array([1.0, 5.0, 5.0, 1.0])


def hs71_problem():
    Jp, Jj, Hp, Hi = dense_patterns(4, 2)
    return Problem(4, 2, Jp, Jj, Hp, Hi, np.full(4, 1.0), np.full(4, 5.0), [25.0, 40.0], [INF, 40.0])


def hs71_starts():
    """the standard start and 24 starts drawn uniformly within 0.1 (12) and 0.3 (12) of it, clipped to [1, 5] (seeded)"""
    rng = np.random.default_rng(71)
    out = [HS71_START]
    for radius in (0.1, 0.3):
        for _ in range(12):
            out.append(np.clip(HS71_START + rng.uniform(-radius, radius, 4), 1.0, 5.0))
    return np.array(out)


def hs71_eval(xp):
    """the HS71 model on the array module xp (numpy or torch): evaluate(x (B, 4), lam (B, 2), want) batched"""
    def evaluate(x, lam, want):
        x0, x1, x2, x3 = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
        s = x0 + x1 + x2
        f = x0 * x3 * s + x2
        g = xp.stack([x0 * x1 * x2 * x3, x0 * x0 + x1 * x1 + x2 * x2 + x3 * x3], 1)
        if not want:
            return f, g
        df = xp.stack([x3 * s + x0 * x3, x0 * x3, x0 * x3 + 1.0, x0 * s], 1)
        dg = xp.stack([x1 * x2 * x3, x0 * x2 * x3, x0 * x1 * x3, x0 * x1 * x2, 2 * x0, 2 * x1, 2 * x2, 2 * x3], 1)
        l0, l1 = lam[:, 0], lam[:, 1]
        two = 2.0 * l1
        # upper triangle, column by column: (0,0) | (0,1) (1,1) | (0,2) (1,2) (2,2) | (0,3) (1,3) (2,3) (3,3)
        hess = xp.stack([2.0 * x3 + two,
                         x3 + l0 * x2 * x3, two,
                         x3 + l0 * x1 * x3, l0 * x0 * x3, two,
                         2.0 * x0 + x1 + x2 + l0 * x1 * x2, x0 + l0 * x0 * x2, x0 + l0 * x0 * x1, two], 1)
        return f, g, df, dg, hess
    return evaluate


def single(evaluate_batched):
    """a batched numpy evaluate as the one-agent evaluate solve_ref takes"""
    def evaluate(x, lam, want):
        return tuple(a[0] for a in evaluate_batched(np.asarray(x)[None], np.asarray(lam)[None], want))
    return evaluate


# ---------------------------------------------------------------------------------------------------------------------
# The reference's Ipopt-test problem (test_ocp_ipopt.cpp): the double integrator from (1, 1) to (0, 0), theta = q, integrand
# |x|^2 + |u|^2, -1 <= u <= 1, ce = (tf, x0, xf), here with tf pinned to 5, on a two-interval mesh of degree 4.  As term tables of
# tests/ocpnlp_ref.py: rows (r, a, ka, b, kb, c, kc) over z = (t | x | u) resp. (tf | x0 | xf | q); kinds 0 = 1, 1 = z, 2 = z^2.
# ---------------------------------------------------------------------------------------------------------------------
OCP_K, OCP_TAU0, OCP_DIMS = np.array([4, 4], np.int32), np.array([0.0, 0.5]), (2, 1, 1, 1, 5)
OCP_BOUNDS = ([-1.0], [1.0], [5.0, 1.0, 1.0, 0.0, 0.0], [5.0, 1.0, 1.0, 0.0, 0.0])
OCP_BOUNDS_FREE = ([-1.0], [1.0], [3.0, 1.0, 1.0, 0.0, 0.0], [6.0, 1.0, 1.0, 0.0, 0.0])   # the reference's own scenario: tf in [3, 6]


def _terms(rows):
    return np.array([(r, a, k, 0, 0, 0, 0) for r, a, k in rows], np.int64), np.ones(len(rows))


def ocp_tables():
    t = {}
    for name, rows in (("f", [(0, 2, 1), (1, 3, 1)]), ("g", [(0, 1, 2), (0, 2, 2), (0, 3, 2)]), ("cr", [(0, 3, 1)]),
                       ("ce", [(r, r, 1) for r in range(5)]), ("theta", [(0, 5, 1)])):
        t["terms." + name], t["coef." + name] = _terms(rows)
    return t


def ocp_problem(free=False):
    import ocpnlp_ref as NR
    N = int(OCP_K.sum())
    vb, cb = NR.structure(N, OCP_DIMS)
    out = NR.nlp(OCP_K, OCP_TAU0, OCP_DIMS, ocp_tables(), np.ones(int(vb[4])), bounds=OCP_BOUNDS_FREE if free else OCP_BOUNDS, order=0)
    Jp, Jj = NR.dg_pattern(OCP_K, OCP_DIMS)
    Hp, Hi = NR.h_pattern(OCP_K, OCP_DIMS)
    return Problem(int(vb[4]), int(cb[4]), Jp, Jj, Hp, Hi, out["xl"], out["xu"], out["gl"], out["gu"])


def ocp_start():
    """tf = 5, q = 0, the straight line between the end states at the mesh's nodes, u = 0"""
    import meshfn_ref as MR
    import ocpnlp_ref as NR
    tau = MR.geometry(OCP_K, OCP_TAU0)[0]
    N = len(tau)
    vb, _ = NR.structure(N, OCP_DIMS)
    x = np.zeros(int(vb[4]))
    x[0] = 5.0
    s = np.append(tau, 1.0)
    x[vb[2]:vb[3]] = (np.array([1.0, 1.0])[None, :] * (1.0 - s)[:, None]).ravel()
    return x


def ocp_eval():
    """one-agent evaluate for solve_ref through tests/ocpnlp_ref.py"""
    import ocpnlp_ref as NR
    tables = ocp_tables()

    def evaluate(x, lam, want):
        o = NR.nlp(OCP_K, OCP_TAU0, OCP_DIMS, tables, x, lam, order=2 if want else 0)
        if not want:
            return o["f"], o["g"]
        return o["f"], o["g"], o["df"], o["dg"], o["d2f"] + o["d2g"]
    return evaluate


def ocp_starts():
    """the straight line, and two seeded perturbations of its states and inputs within 0.05 (tf and q as they are)"""
    rng = np.random.default_rng(6)
    x0 = ocp_start()
    out = [x0]
    for _ in range(2):
        x = x0.copy()
        x[2:] += rng.uniform(-0.05, 0.05, len(x0) - 2)
        out.append(x)
    return np.array(out)
