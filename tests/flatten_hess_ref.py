"""A plain float64 numpy restatement of the second derivatives of the flattened example problems, for the gates of
tests/flatten_hess_gates.py: it differences the Jacobians and values of tests/flatten_ref.py (matrix groups, power series, J(+) as
one full matrix -- nothing of the headers) with the same two steps as include/smooth_feedback_amd/ocp_flatten.hpp:
  f, cr, ce, theta   (J(z + h e_a) - J(z - h e_a)) / (2 h), h = 2^-17, contracted with the multipliers
  g                  the four-point second difference of the values at 2^-13
Upper triangles are computed and mirrored.  What it delivers against the high-precision fixture is what float64 delivers with
this law on these inputs."""
import numpy as np

import flatten_ref as FR

H_JAC = 2.0 ** -17
H_VAL = 2.0 ** -13


def agent_functions(P, row):
    """closures of one agent (row = [x0 | xi | u0 | du]): Jf(z), Jcr(z), g(z) with z = (t | e | v); Jce(ze), Jtheta(ze) with
    ze = (tf | e0 | ef | q).  The formulas of flatten_ref.flat_agent, one function at a time."""
    nx, nu, nq, ncr, nce = P.nx, P.nu, P.nq, P.ncr, P.nce
    nz, ne = 1 + nx + nu, 1 + 2 * nx + nq
    x0 = FR.elem(P.X, row[:P.EX]); xi = np.asarray(row[P.EX:P.EX + nx]); u0 = np.asarray(row[P.EX + nx:P.EX + nx + nu]); du = np.asarray(row[P.EX + nx + nu:])
    xl = lambda t: FR.rplus(P.X, x0, t * xi)
    ul = lambda t: [u0 + t * du]

    def split(z):
        t, e, v = z[0], z[1:1 + nx], z[1 + nx:]
        return t, e, FR.rplus(P.X, xl(t), e), FR.rplus(P.U, ul(t), v)

    def jplus(e):
        Jp = np.zeros((nz, nz)); Jp[0, 0] = 1.0
        Jp[1:1 + nx, 1:1 + nx] = FR.dr_exp(P.X, e); Jp[1 + nx:, 1 + nx:] = np.eye(nu)
        Jp[1:1 + nx, 0] = FR.Ad_exp_neg(P.X, e, xi); Jp[1 + nx:, 0] = du
        return Jp

    def Jf(z):
        t, e, x, u = split(z)
        w = P.f(t, x, u) - xi
        J = np.linalg.inv(FR.dr_exp(P.X, e)) @ P.df(t, x, u) @ jplus(e)
        J[:, 1:1 + nx] += FR.d_expinv(P.X, e, w) - FR.ad(P.X, xi)
        return J

    def Jcr(z):
        Jc = np.zeros((ncr, nz)); Jc[:, 1 + nx:] = np.eye(nu)
        return Jc @ jplus(z[1:1 + nx])

    def g(z):
        t, e, x, u = split(z)
        a = FR.rminus(P.X, x, P.xdes(t))
        return 0.5 * (a @ a + u[0] @ u[0])

    def jend(ze):
        tf, e0, ef = ze[0], ze[1:1 + nx], ze[1 + nx:1 + 2 * nx]
        Je = np.zeros((ne, ne)); Je[0, 0] = 1.0
        Je[1:1 + nx, 1:1 + nx] = FR.dr_exp(P.X, e0); Je[1 + nx:1 + 2 * nx, 1 + nx:1 + 2 * nx] = FR.dr_exp(P.X, ef)
        Je[1 + nx:1 + 2 * nx, 0] = FR.Ad_exp_neg(P.X, ef, xi); Je[1 + 2 * nx:, 1 + 2 * nx:] = np.eye(nq)
        return Je

    def Jce(ze):
        lg = FR.rminus(P.X, FR.rplus(P.X, xl(0.0), ze[1:1 + nx]), FR.identity(P.X))
        J = np.zeros((nce, ne)); J[0, 0] = 1.0
        J[1:, 1:1 + nx] = np.linalg.inv(FR.dr_exp(P.X, lg))
        return J @ jend(ze)

    def Jtheta(ze):
        J = np.zeros((1, ne)); J[0, 0] = 1.0; J[0, ne - 1] = 1.0
        return J @ jend(ze)

    return dict(Jf=Jf, Jcr=Jcr, g=g, Jce=Jce, Jtheta=Jtheta)


def square_from_jacobians(J, z, lam):
    """sum_r lam[r] H_r from central differences of J at H_JAC: rows from the diagonal on, mirrored"""
    n = len(z)
    out = np.zeros((n, n))
    for a in range(n):
        d = np.zeros(n); d[a] = H_JAC
        row = lam @ ((J(z + d) - J(z - d)) / (2 * H_JAC))
        out[a, a:] = row[a:]
        out[a:, a] = row[a:]
    return out


def square_from_values(f, z, lam):
    """lam times the four-point second differences of the scalar f at H_VAL, mirrored"""
    n = len(z)
    out = np.zeros((n, n))
    h = H_VAL
    for a in range(n):
        for b in range(a, n):
            da = np.zeros(n); db = np.zeros(n); da[a] = h; db[b] = h
            v = ((f(z + da + db) - f(z + da - db)) - (f(z - da + db) - f(z - da - db))) / (4 * h * h)
            out[a, b] = out[b, a] = lam * v
    return out


def flat_hess_agent(P, row, tau, xa, lam):
    """the five arrays of one agent (x [n], row, lam [N nx + nq + N ncr + nce]) as the fixture lays them out"""
    N = len(tau)
    nx, nu, nq, ncr = P.nx, P.nu, P.nq, P.ncr
    fn = agent_functions(P, np.asarray(row))
    out = dict(HLf=[], HLg=[], HLcr=[])
    for i in range(N):
        t = xa[0] * tau[i]
        z = np.concatenate([[t], xa[1 + nq + i * nx:1 + nq + (i + 1) * nx], xa[1 + nq + (N + 1) * nx + i * nu:1 + nq + (N + 1) * nx + (i + 1) * nu]])
        out["HLf"].append(square_from_jacobians(fn["Jf"], z, lam[i * nx:(i + 1) * nx]))
        out["HLg"].append(square_from_values(fn["g"], z, lam[N * nx]))
        out["HLcr"].append(square_from_jacobians(fn["Jcr"], z, lam[N * nx + nq + i * ncr:N * nx + nq + (i + 1) * ncr]))
    ze = np.concatenate([[xa[0]], xa[1 + nq:1 + nq + nx], xa[1 + nq + N * nx:1 + nq + (N + 1) * nx], xa[1:1 + nq]])
    out = {k: np.stack(v) for k, v in out.items()}
    out["d2theta"] = square_from_jacobians(fn["Jtheta"], ze, np.ones(1))
    out["d2ce_l"] = square_from_jacobians(fn["Jce"], ze, lam[N * nx + nq + N * ncr:])
    return out


def flat_hess_nodes(problem, tau, x, lam, traj):
    """the restatement on agents x [B][n], lam [B][m'], traj [B][row]: dict of stacked arrays"""
    P = FR.PROBLEMS[problem]
    rows = [flat_hess_agent(P, traj[b], np.asarray(tau), np.asarray(x[b]), np.asarray(lam[b])) for b in range(len(x))]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}
