"""A plain float64 numpy restatement of flatten_ocp for the two example problems (examples/ocp_se2_model.h), sharing nothing
with the headers: groups as matrices, exp by a scaled Taylor series, dr_exp by its power series in ad, dr_expinv by solving with
it, J(+) as one full matrix, Ad from M hat(b) M^-1.  tests/flatten_gates.py measures it against the high-precision fixture; its
errors are the gates.  Elements are lists of parts: a matrix per group part, a vector per R^n part."""
import numpy as np

FD_STEP = 2.0 ** -26
DOF = dict(SE2=3, SO3=3, SE3=6)
PARTS = dict(SE2=[("SE2", 3)], SO3=[("SO3", 3)], SE3=[("SE3", 6)], X5=[("SE2", 3), ("R", 2)], X12B=[("SE3", 6), ("R", 6)])


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)


def hat(kind, a):
    if kind == "SE2":
        return np.array([[0, -a[2], a[0]], [a[2], 0, a[1]], [0, 0, 0]], dtype=np.float64)
    if kind == "SO3":
        return skew(a)
    M = np.zeros((4, 4)); M[:3, :3] = skew(a[3:]); M[:3, 3] = a[:3]
    return M


def vee(kind, M):
    if kind == "SE2":
        return np.array([M[0, 2], M[1, 2], M[1, 0]])
    if kind == "SO3":
        return np.array([M[2, 1], M[0, 2], M[1, 0]])
    return np.array([M[0, 3], M[1, 3], M[2, 3], M[2, 1], M[0, 2], M[1, 0]])


def ad_part(kind, a):
    if kind == "SE2":
        return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [0, 0, 0]], dtype=np.float64)
    if kind == "SO3":
        return skew(a)
    M = np.zeros((6, 6)); M[:3, :3] = skew(a[3:]); M[3:, 3:] = skew(a[3:]); M[:3, 3:] = skew(a[:3])
    return M


def expm(A):
    s = max(0, int(np.ceil(np.log2(max(np.linalg.norm(A, 1), 1e-300)))) + 3)
    A = A / 2.0 ** s
    out = np.eye(len(A)); term = np.eye(len(A))
    for k in range(1, 25):
        term = term @ A / k
        out = out + term
    for _ in range(s):
        out = out @ out
    return out


def rot_coefs(th2):
    """(1 - cos th) / th^2 and (th - sin th) / th^3"""
    th = np.sqrt(th2)
    if th < 0.1:
        B = 0.5 - th2 / 24 + th2 ** 2 / 720 - th2 ** 3 / 40320 + th2 ** 4 / 3628800
        C = 1.0 / 6 - th2 / 120 + th2 ** 2 / 5040 - th2 ** 3 / 362880 + th2 ** 4 / 39916800
        return B, C
    return 2 * np.sin(th / 2) ** 2 / th2, (th - np.sin(th)) / (th2 * th)


def log_part(kind, M):
    if kind == "SE2":
        th = np.arctan2(M[1, 0], M[0, 0])
        B, C = rot_coefs(th * th)
        V = np.array([[1 - C * th * th, -B * th], [B * th, 1 - C * th * th]])  # sin th / th = 1 - C th^2
        v = np.linalg.solve(V, M[:2, 2])
        return np.array([v[0], v[1], th])
    R = M[:3, :3]
    r = vee("SO3", (R - R.T) / 2)
    sn = np.linalg.norm(r)
    ang = np.arctan2(sn, (np.trace(R) - 1) / 2)
    w = r * (1 + sn * sn / 6) if sn < 1e-6 else r * (ang / sn)
    if kind == "SO3":
        return w
    B, C = rot_coefs(float(w @ w))
    W = skew(w)
    return np.concatenate([np.linalg.solve(np.eye(3) + B * W + C * W @ W, M[:3, 3]), w])


def blockdiag(parts, fn, a):
    T = sum(d for _, d in parts)
    out = np.zeros((T, T)); off = 0
    for kind, d in parts:
        out[off:off + d, off:off + d] = np.eye(d) if kind == "R" else fn(kind, a[off:off + d])
        off += d
    return out


def dr_exp_part(kind, a, terms=40):
    A = ad_part(kind, a)
    out = np.eye(len(A)); P = np.eye(len(A)); fact = 1.0
    for n in range(1, terms):
        P = P @ A; fact *= -(n + 1)
        out = out + P / fact
    return out


def dr_exp(parts, a):
    return blockdiag(parts, dr_exp_part, np.asarray(a, dtype=np.float64))


def ad(parts, a):
    out = blockdiag(parts, ad_part, np.asarray(a, dtype=np.float64))
    off = 0
    for kind, d in parts:
        if kind == "R":
            out[off:off + d, off:off + d] = 0.0
        off += d
    return out


def d_expinv_part(kind, e, w, terms=40):
    """d/de (J(e)^-1 w) = -J^-1 (dJ/de_j) J^-1 w, dJ/de_j termwise: d(ad^n) = sum_k ad^k ad(E_j) ad^(n-1-k)"""
    T = DOF[kind]
    A = ad_part(kind, e)
    J = dr_exp_part(kind, e, terms)
    y = np.linalg.solve(J, w)
    pw = [np.eye(T)]
    for n in range(1, terms):
        pw.append(pw[-1] @ A)
    out = np.zeros((T, T))
    for j in range(T):
        E = ad_part(kind, np.eye(T)[j])
        dJ = np.zeros((T, T)); fact = 1.0
        for n in range(1, terms):
            fact *= -(n + 1)
            if abs(fact) > 1e25:
                break
            dJ += sum(pw[k] @ E @ pw[n - 1 - k] for k in range(n)) / fact
        out[:, j] = -np.linalg.solve(J, dJ @ y)
    return out


def d_expinv(parts, e, w):
    e = np.asarray(e, dtype=np.float64); w = np.asarray(w, dtype=np.float64)
    T = sum(d for _, d in parts)
    out = np.zeros((T, T)); off = 0
    for kind, d in parts:
        if kind != "R":
            out[off:off + d, off:off + d] = d_expinv_part(kind, e[off:off + d], w[off:off + d])
        off += d
    return out


# ---- elements ----
def elem(parts, p):
    out = []; off = 0
    for kind, d in parts:
        if kind == "R":
            out.append(np.array(p[off:off + d], dtype=np.float64)); off += d
        elif kind == "SE2":
            x, y, c, s = p[off:off + 4]; off += 4
            out.append(np.array([[c, -s, x], [s, c, y], [0, 0, 1]], dtype=np.float64))
        else:
            px, py, pz, w, x, y, z = p[off:off + 7]; off += 7
            M = np.eye(4)
            M[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
            M[:3, 3] = [px, py, pz]
            out.append(M)
    return out


def rplus(parts, g, a):
    out = []; off = 0
    for (kind, d), gp in zip(parts, g):
        out.append(gp + a[off:off + d] if kind == "R" else gp @ expm(hat(kind, a[off:off + d])))
        off += d
    return out


def rminus(parts, a, b):
    return np.concatenate([ap - bp if kind == "R" else log_part(kind, np.linalg.solve(bp, ap)) for (kind, d), ap, bp in zip(parts, a, b)])


def identity(parts):
    return [np.zeros(d) if kind == "R" else np.eye(3 if kind != "SE3" else 4) for kind, d in parts]


def Ad_exp_neg(parts, e, b):
    """Ad_exp(-e) b = vee(M hat(b) M^-1), M = exp(-e), part by part"""
    out = []; off = 0
    for kind, d in parts:
        if kind == "R":
            out.append(b[off:off + d])
        else:
            M = expm(hat(kind, -e[off:off + d]))
            out.append(vee(kind, M @ hat(kind, b[off:off + d]) @ np.linalg.inv(M)))
        off += d
    return np.concatenate(out)


# ---- the problems ----
class SE2Problem:
    name = "se2"
    X, U = PARTS["X5"], [("R", 2)]
    nx, nu, nq, ncr, nce, EX = 5, 2, 1, 2, 6, 6

    def xdes(self, t):
        return [expm(hat("SE2", np.array([t, 0.0, 0.5 * t]))), np.array([1.0, 0.5])]

    def f(self, t, x, u):
        return np.array([x[1][0], 0.0, x[1][1], u[0][0], u[0][1]])

    def df(self, t, x, u):
        J = np.zeros((5, 8)); J[0, 4] = J[2, 5] = J[3, 6] = J[4, 7] = 1.0
        return J


DAMP = np.array([0.2, 0.3, 0.25, 0.4, 0.35, 0.5])


class SE3Problem:
    name = "se3"
    X, U = PARTS["X12B"], [("R", 6)]
    nx, nu, nq, ncr, nce, EX = 12, 6, 1, 6, 13, 13
    XI = np.array([0.8, 0.0, 0.15, 0.1, -0.05, 0.4])
    START = np.array([2.5, 0.0, 1.0, 0.3, -0.2, 1.5707963267948966])

    def xdes(self, t):
        return [expm(hat("SE3", self.START)) @ expm(hat("SE3", t * self.XI)), self.XI.copy()]

    def f(self, t, x, u):
        gb = x[0][:3, :3].T @ np.array([0.0, 0.0, -1.0])
        w = x[1]
        return np.concatenate([w, u[0] - DAMP * w + np.concatenate([gb, np.zeros(3)])])

    def df(self, t, x, u):
        J = np.zeros((12, 19))
        J[:6, 7:13] = np.eye(6); J[6:, 7:13] = -np.diag(DAMP); J[6:, 13:] = np.eye(6)
        J[6:9, 4:7] = skew(x[0][:3, :3].T @ np.array([0.0, 0.0, -1.0]))
        return J


PROBLEMS = dict(se2=SE2Problem(), se3=SE3Problem())


def flat_agent(P, row, tau, xa):
    """the node arrays of one agent (x [n], row [x0 | xi | u0 | du]) as the fixture lays them out"""
    N = len(tau)
    nx, nu, nq, ncr, nce = P.nx, P.nu, P.nq, P.ncr, P.nce
    nz, ne = 1 + nx + nu, 1 + 2 * nx + nq
    x0 = elem(P.X, row[:P.EX]); xi = np.asarray(row[P.EX:P.EX + nx]); u0 = np.asarray(row[P.EX + nx:P.EX + nx + nu]); du = np.asarray(row[P.EX + nx + nu:])
    xl = lambda t: rplus(P.X, x0, t * xi)
    ul = lambda t: [u0 + t * du]
    out = dict(Ff=np.zeros((N, nx)), dFf=np.zeros((N, nx, nz)), Fg=np.zeros((N, nq)), dFg=np.zeros((N, nq, nz)), Fcr=np.zeros((N, ncr)),
               dFcr=np.zeros((N, ncr, nz)))
    tf = xa[0]

    def integrand(t, x, u):
        a = rminus(P.X, x, P.xdes(t))
        return 0.5 * (a @ a + u[0] @ u[0])

    for i in range(N):
        t = tf * tau[i]
        e = xa[1 + nq + i * nx:1 + nq + (i + 1) * nx]
        v = xa[1 + nq + (N + 1) * nx + i * nu:1 + nq + (N + 1) * nx + (i + 1) * nu]
        x = rplus(P.X, xl(t), e); u = rplus(P.U, ul(t), v)
        Jp = np.zeros((nz, nz)); Jp[0, 0] = 1.0
        Jp[1:1 + nx, 1:1 + nx] = dr_exp(P.X, e); Jp[1 + nx:, 1 + nx:] = np.eye(nu)
        Jp[1:1 + nx, 0] = Ad_exp_neg(P.X, e, xi); Jp[1 + nx:, 0] = du
        fv = P.f(t, x, u); w = fv - xi
        Dinv = np.linalg.inv(dr_exp(P.X, e)); ade = ad(P.X, e)
        out["Ff"][i] = Dinv @ w + ade @ xi
        J = Dinv @ P.df(t, x, u) @ Jp
        J[:, 1:1 + nx] += d_expinv(P.X, e, w) - ad(P.X, xi)
        out["dFf"][i] = J
        g0 = integrand(t, x, u)
        out["Fg"][i, 0] = g0
        Jg = np.zeros((1, nz))
        Jg[0, 0] = (integrand(t + FD_STEP, x, u) - g0) / FD_STEP
        for c in range(nx):
            Jg[0, 1 + c] = (integrand(t, rplus(P.X, x, FD_STEP * np.eye(nx)[c]), u) - g0) / FD_STEP
        for c in range(nu):
            Jg[0, 1 + nx + c] = (integrand(t, x, rplus(P.U, u, FD_STEP * np.eye(nu)[c])) - g0) / FD_STEP
        out["dFg"][i] = Jg @ Jp
        out["Fcr"][i] = u[0]
        Jc = np.zeros((ncr, nz)); Jc[:, 1 + nx:] = np.eye(nu)
        out["dFcr"][i] = Jc @ Jp
    e0 = xa[1 + nq:1 + nq + nx]; ef = xa[1 + nq + N * nx:1 + nq + (N + 1) * nx]; q = xa[1:1 + nq]
    xs = rplus(P.X, xl(0.0), e0)
    lg = rminus(P.X, xs, identity(P.X))
    out["ce"] = np.concatenate([[tf], lg])
    Je = np.zeros((ne, ne)); Je[0, 0] = 1.0
    Je[1:1 + nx, 1:1 + nx] = dr_exp(P.X, e0); Je[1 + nx:1 + 2 * nx, 1 + nx:1 + 2 * nx] = dr_exp(P.X, ef)
    Je[1 + nx:1 + 2 * nx, 0] = Ad_exp_neg(P.X, ef, xi); Je[1 + 2 * nx:, 1 + 2 * nx:] = np.eye(nq)
    Jce = np.zeros((nce, ne)); Jce[0, 0] = 1.0
    Jce[1:, 1:1 + nx] = np.linalg.inv(dr_exp(P.X, lg))
    out["dce"] = Jce @ Je
    out["theta"] = tf + q[0]
    Jt = np.zeros((1, ne)); Jt[0, 0] = 1.0; Jt[0, ne - 1] = 1.0
    out["dtheta"] = (Jt @ Je)[0]
    return out


def flat_nodes(problem, tau, x, traj):
    """the restatement on agents x [B][n], traj [B][row]: dict of stacked arrays"""
    P = PROBLEMS[problem]
    rows = [flat_agent(P, traj[b], np.asarray(tau), np.asarray(x[b])) for b in range(len(x))]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}
