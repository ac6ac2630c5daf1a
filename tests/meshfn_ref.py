"""Plain float64 numpy restatement of the functions over a collocation mesh (mesh_eval, mesh_integrate, mesh_dyn with first
and multiplier-weighted second derivatives) and of the fixture's integrands.  It shares nothing with the headers under
include/; the mesh (nodes, weights, differentiation matrices) is the restatement of tests/mesh_ref.py.  Used for the gates
(tests/meshfn_gates.py), for the patterns the tests compare exactly, and to evaluate the integrands for the model-free kernels.

Variables [t0 | tf | x_0 .. x_N | u_0 .. u_{N-1}].  Derivatives are returned as scipy-free CSR (rowptr, colind, val) with
ascending columns, second derivatives as the upper triangle in CSC (colptr, rowind, val)."""
import numpy as np

import mesh_ref as R


def phi(k, z):
    z = np.asarray(z, dtype=np.float64)
    one, zero = np.ones_like(z), np.zeros_like(z)
    return [(one, zero, zero), (z, one, zero), (z * z, 2 * z, 2 * one), (np.sin(z), np.cos(z), -np.sin(z)), (np.cos(z), -np.sin(z), -np.cos(z))][k]


def model(dims, terms, coef, t, xs, us):
    """the term-table integrand at N nodes: f (N, nf), J (N, nf, nv), H (N, nf, nv, nv); columns (t | x | u)"""
    nx, nu, nf = [int(v) for v in dims]
    N, nv = len(t), 1 + nx + nu
    z = np.column_stack([t, xs[:N].reshape(N, nx), us[:N].reshape(N, nu)])
    f, J, H = np.zeros((N, nf)), np.zeros((N, nf, nv)), np.zeros((N, nf, nv, nv))
    for (r, a, ka, b, kb), c in zip(terms, coef):
        A, B = phi(ka, z[:, a]), phi(kb, z[:, b])
        f[:, r] += c * A[0] * B[0]
        J[:, r, a] += c * A[1] * B[0]
        J[:, r, b] += c * A[0] * B[1]
        H[:, r, a, a] += c * A[2] * B[0]
        H[:, r, a, b] += c * A[1] * B[1]
        H[:, r, b, a] += c * A[1] * B[1]
        H[:, r, b, b] += c * A[0] * B[2]
    return f, J, H


def geometry(K, tau0):
    """nodes (N,), weights (N,), and per node (interval, index in it, first node of the interval)"""
    K = np.asarray(K, dtype=np.int64)
    where, M = [], 0
    for s, k in enumerate(K):
        where += [(s, j, M) for j in range(k)]
        M += k
    return R.all_nodes(K, tau0)[:-1], R.all_weights(K, tau0)[:-1], where


def eval_pattern(N, nx, nu, nf):
    per = 2 + nx + nu
    colind = np.zeros((N * nf, per), np.int32)
    for i in range(N):
        colind[i * nf:(i + 1) * nf] = np.concatenate([[0, 1], 2 + i * nx + np.arange(nx), 2 + (N + 1) * nx + i * nu + np.arange(nu)])
    return np.arange(N * nf + 1, dtype=np.int32) * per, colind.ravel()


def dyn_pattern(K, nx, nu):
    K = np.asarray(K, dtype=np.int64)
    N = int(K.sum())
    rowptr, colind, M = [0], [], 0
    for k in K:
        for j in range(k):
            for d in range(nx):
                cols = {0, 1} | {2 + (M + kk) * nx + d for kk in range(k + 1)} | {2 + (M + j) * nx + c for c in range(nx)}
                cols |= {2 + (N + 1) * nx + (M + j) * nu + c for c in range(nu)}
                colind += sorted(cols)
                rowptr.append(len(colind))
        M += k
    return np.array(rowptr, np.int32), np.array(colind, np.int32)


def integrate_pattern(N, nx, nu, nf):
    nv = 2 + nx * (N + 1) + nu * N
    return np.arange(nf + 1, dtype=np.int32) * nv, np.tile(np.arange(nv, dtype=np.int32), nf)


def d2_pattern(N, nx, nu):
    nv = 2 + nx * (N + 1) + nu * N
    colptr, rowind = [0], []
    for c in range(nv):
        if c < 2:
            rowind += list(range(c + 1))
        elif c < 2 + nx * N:
            i, j = divmod(c - 2, nx)
            rowind += [0, 1] + [2 + i * nx + r for r in range(j + 1)]
        elif c >= 2 + nx * (N + 1):
            i, j = divmod(c - 2 - nx * (N + 1), nu)
            rowind += [0, 1] + [2 + i * nx + r for r in range(nx)] + [2 + nx * (N + 1) + i * nu + r for r in range(j + 1)]
        colptr.append(len(rowind))
    return np.array(colptr, np.int32), np.array(rowind, np.int32)


def _dense_to(rowptr, colind, A):
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return A[rows, colind]


def _second(N, nx, nu, i, tau, s, wl, timed, Jr, Hr, Hs):
    """adds node i's part of one output's multiplier-weighted Hessian to the dense numVars x numVars Hs (upper blocks):
    s scales the Hessian blocks, wl the Jacobian blocks that only the time-scaled functions have"""
    mt = 1 - tau
    xd, ud = 2 + i * nx, 2 + (N + 1) * nx + i * nu
    X, U = slice(xd, xd + nx), slice(ud, ud + nu)
    tx, tu = slice(1, 1 + nx), slice(1 + nx, 1 + nx + nu)
    Hs[0, 0] += s * mt * mt * Hr[0, 0]
    Hs[0, 1] += s * mt * tau * Hr[0, 0]
    Hs[1, 1] += s * tau * tau * Hr[0, 0]
    Hs[0, X] += s * mt * Hr[0, tx]
    Hs[0, U] += s * mt * Hr[0, tu]
    Hs[1, X] += s * tau * Hr[0, tx]
    Hs[1, U] += s * tau * Hr[0, tu]
    Hs[X, X] += s * Hr[tx, tx]
    Hs[X, U] += s * Hr[tx, tu]
    Hs[U, U] += s * Hr[tu, tu]
    if timed:
        Hs[0, 0] += -2 * wl * mt * Jr[0]
        Hs[0, 1] += wl * (1 - 2 * tau) * Jr[0]
        Hs[1, 1] += 2 * wl * tau * Jr[0]
        Hs[0, X] += -wl * Jr[tx]
        Hs[0, U] += -wl * Jr[tu]
        Hs[1, X] += wl * Jr[tx]
        Hs[1, U] += wl * Jr[tu]


def _upper(N, nx, nu, Hs):
    colptr, rowind = d2_pattern(N, nx, nu)
    cols = np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))
    return Hs[rowind, cols]


def functions(K, tau0, dims, t0, tf, xs, f, J, H=None, lam=None, order=1):
    """{"eval.F": .., "eval.dF": .., "eval.d2F": .., "evals.*" (scaled), "integrate.*", "dyn.*" (when nf == nx)} from the
    integrand's values f (N, nf), Jacobians J (N, nf, nv) and Hessians H (N, nf, nv, nv) at the nodes; lam: {function: multipliers}"""
    nx, nu, nf = [int(v) for v in dims]
    tau, w, where = geometry(K, tau0)
    N, h = len(tau), tf - t0
    nv = 2 + nx * (N + 1) + nu * N
    out = {}
    for key in ("eval", "evals", "integrate") + (("dyn",) if nf == nx else ()):
        timed = key in ("integrate", "dyn")
        rows = nf if key == "integrate" else N * nf
        F, A = np.zeros(rows), np.zeros((rows, nv))
        Hs = np.zeros((nv, nv))
        for i in range(N):
            wi = 1.0 if key == "eval" else w[i]
            xd, ud = 2 + i * nx, 2 + (N + 1) * nx + i * nu
            for r in range(nf):
                row = r if key == "integrate" else i * nf + r
                if timed:
                    F[row] += wi * h * f[i, r]
                    A[row, 0] += -wi * f[i, r] + wi * h * (1 - tau[i]) * J[i, r, 0]
                    A[row, 1] += wi * f[i, r] + wi * h * tau[i] * J[i, r, 0]
                    A[row, xd:xd + nx] += wi * h * J[i, r, 1:1 + nx]
                    A[row, ud:ud + nu] += wi * h * J[i, r, 1 + nx:]
                else:
                    F[row] = wi * f[i, r]
                    A[row, 0] = wi * (1 - tau[i]) * J[i, r, 0]
                    A[row, 1] = wi * tau[i] * J[i, r, 0]
                    A[row, xd:xd + nx] = wi * J[i, r, 1:1 + nx]
                    A[row, ud:ud + nu] = wi * J[i, r, 1 + nx:]
                if order >= 2:
                    wl = wi * lam[key][row]
                    _second(N, nx, nu, i, tau[i], wl * h if timed else wl, wl, timed, J[i, r], H[i, r], Hs)
        if key == "dyn":
            X = np.asarray(xs, dtype=np.float64).reshape(N + 1, nx)
            Ds = [R.diffmat(np.asarray(K, dtype=np.int64), tau0, s) for s in range(len(K))]
            for i, (s, j, M) in enumerate(where):
                D = Ds[s]
                for k in range(int(K[s]) + 1):
                    F[i * nx:(i + 1) * nx] -= w[i] * D[k, j] * X[M + k]
                    A[np.arange(i * nx, (i + 1) * nx), 2 + (M + k) * nx + np.arange(nx)] -= w[i] * D[k, j]
        out[key + ".F"] = F
        if order >= 1:
            pat = integrate_pattern(N, nx, nu, nf) if key == "integrate" else dyn_pattern(K, nx, nu) if key == "dyn" else eval_pattern(N, nx, nu, nf)
            out[key + ".dF"] = _dense_to(pat[0], pat[1], A)
        if order >= 2:
            out[key + ".d2F"] = _upper(N, nx, nu, Hs)
    return out


def node_times(K, tau0, t0, tf):
    return t0 + (tf - t0) * geometry(K, tau0)[0]


def scaled_error(got, ref):
    return R.scaled_error(got, ref)
