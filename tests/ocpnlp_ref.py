"""Plain float64 numpy restatement of the collocation NLP of an optimal control problem over a ph mesh (ocp_to_nlp.hpp,
sfb_ocp_nlp_*).  It shares nothing with the headers under include/: it is the composition a caller had to write before --
mesh_dyn, mesh_integrate and the weight-scaled mesh_eval of tests/meshfn_ref.py on the variables [t0 | tf | X | U] with
t0 = 0, then the t0 column dropped, the variables re-ordered to [tf | q | X | U], everything scaled by ws, the -ws I block and
the end-constraint rows added -- done on dense matrices and read out through patterns built here from sets.  Used for the
gates (tests/ocpnlp_gates.py), for the patterns the tests compare exactly, and to evaluate the models for the model-free kernel.

Functions are term tables with three factors: output r = sum of coef phi_ka(z_a) phi_kb(z_b) phi_kc(z_c) over rows
(r, a, ka, b, kb, c, kc); z = (t | x | u) for f, g, cr and (tf | x0 | xf | q) for theta, ce."""
import numpy as np

import meshfn_ref as MR


def model(terms, coef, nf, Z):
    """a term table at the rows of Z (R, nv): f (R, nf), J (R, nf, nv), H (R, nf, nv, nv)"""
    Z = np.asarray(Z, dtype=np.float64)
    R, nv = Z.shape
    f, J, H = np.zeros((R, nf)), np.zeros((R, nf, nv)), np.zeros((R, nf, nv, nv))
    for (r, a, ka, b, kb, c, kc), co in zip(terms, coef):
        idx = (a, b, c)
        P = (MR.phi(ka, Z[:, a]), MR.phi(kb, Z[:, b]), MR.phi(kc, Z[:, c]))
        f[:, r] += co * P[0][0] * P[1][0] * P[2][0]
        for p, q, s in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            J[:, r, idx[p]] += co * P[p][1] * P[q][0] * P[s][0]
            H[:, r, idx[p], idx[p]] += co * P[p][2] * P[q][0] * P[s][0]
            H[:, r, idx[p], idx[q]] += co * P[p][1] * P[q][1] * P[s][0]
            H[:, r, idx[q], idx[p]] += co * P[p][1] * P[q][1] * P[s][0]
    return f, J, H


def structure(N, dims):
    nx, nu, nq, ncr, nce = [int(v) for v in dims]
    return np.cumsum([0, 1, nq, nx * (N + 1), nu * N]).astype(np.int64), np.cumsum([0, nx * N, nq, ncr * N, nce]).astype(np.int64)


def split(N, dims, x):
    """tf, q (nq,), X (N + 1, nx), U (N, nu) of the NLP variables"""
    vb, _ = structure(N, dims)
    x = np.asarray(x, dtype=np.float64)
    return float(x[0]), x[vb[1]:vb[2]], x[vb[2]:vb[3]].reshape(N + 1, int(dims[0])), x[vb[3]:vb[4]].reshape(N, int(dims[1]))


def w_scaling(K, tau0):
    return 1.0 / max(1e-6, float(np.max(MR.geometry(K, tau0)[1])))


def models(K, tau0, dims, tables, x):
    """what the model-free entry takes for one agent: {"f": (F, dF, H), "g": .., "cr": .., "ce": (ce, dce, Hce), "theta": ..}"""
    nx, nu, nq, ncr, nce = [int(v) for v in dims]
    tau = MR.geometry(K, tau0)[0]
    N = len(tau)
    tf, q, X, U = split(N, dims, x)
    Z = np.column_stack([tf * tau, X[:N], U])
    ze = np.concatenate([[tf], X[0], X[N], q])[None, :]
    out = {name: model(tables["terms." + name], tables["coef." + name], nf, Z) for name, nf in (("f", nx), ("g", nq), ("cr", ncr))}
    for name, nf in (("ce", nce), ("theta", 1)):
        f, J, H = model(tables["terms." + name], tables["coef." + name], nf, ze)
        out[name] = (f[0], J[0], H[0])
    return out


def dg_pattern(K, dims):
    nx, nu, nq, ncr, nce = [int(v) for v in dims]
    K = np.asarray(K, dtype=np.int64)
    N = int(K.sum())
    vb, _ = structure(N, dims)
    xs = lambda i: set(range(vb[2] + i * nx, vb[2] + (i + 1) * nx))                 # noqa: E731
    us = lambda i: set(range(vb[3] + i * nu, vb[3] + (i + 1) * nu))                 # noqa: E731
    rows, M = [], 0
    for k in K:
        for j in range(k):
            for d in range(nx):
                rows.append({0} | {vb[2] + (M + kk) * nx + d for kk in range(k + 1)} | xs(M + j) | us(M + j))
        M += k
    for r in range(nq):
        cols = {0, vb[1] + r}
        for i in range(N):
            cols |= xs(i) | us(i)
        rows.append(cols)
    for i in range(N):
        rows += [{0} | xs(i) | us(i)] * ncr
    rows += [{0} | set(range(vb[1], vb[2])) | xs(0) | xs(N)] * nce
    return np.cumsum([0] + [len(r) for r in rows]).astype(np.int32), np.array([c for r in rows for c in sorted(r)], np.int32)


def h_pattern(K, dims):
    nx, nu, nq, ncr, nce = [int(v) for v in dims]
    N = int(np.sum(K))
    vb, _ = structure(N, dims)
    groups = [[0] + list(range(vb[2] + i * nx, vb[2] + (i + 1) * nx)) + list(range(vb[3] + i * nu, vb[3] + (i + 1) * nu)) for i in range(N)]
    groups.append([0] + list(range(vb[1], vb[2])) + list(range(vb[2], vb[2] + nx)) + list(range(vb[2] + N * nx, vb[2] + (N + 1) * nx)))
    pairs = sorted({(c, r) for g in groups for r in g for c in g if r <= c})
    colptr = np.zeros(vb[4] + 1, np.int64)
    for c, _ in pairs:
        colptr[c + 1] += 1
    return np.cumsum(colptr).astype(np.int32), np.array([r for _, r in pairs], np.int32)


def _dense_csr(pat, val, cols):
    A = np.zeros((len(pat[0]) - 1, cols))
    A[np.repeat(np.arange(len(pat[0]) - 1), np.diff(pat[0])), pat[1]] = val
    return A


def nlp(K, tau0, dims, tables, x, lam=None, bounds=None, order=2):
    """{"f", "df", "d2f", "g", "dg", "d2g", "gl", "gu", "xl", "xu", "w_scaling"} in float64 (order 2 needs lam; bounds = (crl, cru, cel, ceu))"""
    nx, nu, nq, ncr, nce = [int(v) for v in dims]
    tau, w, _ = MR.geometry(K, tau0)
    N = len(tau)
    vb, cb = structure(N, dims)
    n, m = int(vb[4]), int(cb[4])
    tf, q, X, U = split(N, dims, x)
    ws = w_scaling(K, tau0)
    mv = models(K, tau0, dims, tables, x)
    old = 2 + nx * (N + 1) + nu * N                                                # [t0 | tf | X | U]
    to_new = np.concatenate([[-1, 0], vb[2] + np.arange(nx * (N + 1)), vb[3] + np.arange(nu * N)]).astype(np.int64)
    end_new = np.concatenate([[0], vb[2] + np.arange(nx), vb[2] + N * nx + np.arange(nx), vb[1] + np.arange(nq)]).astype(np.int64)
    lam = np.zeros(m) if lam is None else np.asarray(lam, dtype=np.float64)
    g, A, Hg = np.zeros(m), np.zeros((m, n)), np.zeros((n, n))
    for name, key, nf, seg in (("f", "dyn", nx, 0), ("g", "integrate", nq, 1), ("cr", "evals", ncr, 2)):
        if nf == 0:
            continue
        rows = slice(cb[seg], cb[seg + 1])
        f, J, H = mv[name]
        res = MR.functions(K, tau0, (nx, nu, nf), 0.0, tf, X, f, J, H, {k: np.concatenate([lam[rows], np.zeros(N * nf)]) for k in ("eval", "evals", "integrate", "dyn")}, order)
        g[rows] = ws * res[key + ".F"]
        if order >= 1:
            pat = MR.integrate_pattern(N, nx, nu, nf) if key == "integrate" else MR.dyn_pattern(K, nx, nu) if key == "dyn" else MR.eval_pattern(N, nx, nu, nf)
            A[rows][:, to_new[1:]] = ws * _dense_csr(pat, res[key + ".dF"], old)[:, 1:]
        if order >= 2:
            cp, ri = MR.d2_pattern(N, nx, nu)
            cols = np.repeat(np.arange(old), np.diff(cp))
            keep = (ri > 0) & (cols > 0)
            np.add.at(Hg, (to_new[ri[keep]], to_new[cols[keep]]), ws * res[key + ".d2F"][keep])
    if nq:
        g[cb[1]:cb[2]] -= ws * q
        A[np.arange(cb[1], cb[2]), vb[1] + np.arange(nq)] -= ws
    ce, dce, Hce = mv["ce"]
    g[cb[3]:] = ce
    for r in range(nce):
        A[cb[3] + r, end_new] = dce[r]
    th, dth, Hth = mv["theta"]

    def upper(Hend):
        out = np.zeros((n, n))
        for a, ca in enumerate(end_new):
            for b, cbb in enumerate(end_new):
                if ca <= cbb:
                    out[ca, cbb] = Hend[a, b]
        return out

    out = {"f": float(th[0]), "g": g, "w_scaling": ws}
    hp = h_pattern(K, dims)
    hcols = np.repeat(np.arange(n), np.diff(hp[0]))
    if order >= 1:
        df = np.zeros(n)
        df[end_new] = dth[0]
        pat = dg_pattern(K, dims)
        out["df"], out["dg"] = df, A[np.repeat(np.arange(m), np.diff(pat[0])), pat[1]]
    if order >= 2:
        for r in range(nce):
            Hg += lam[cb[3] + r] * upper(Hce[r])
        out["d2f"], out["d2g"] = upper(Hth[0])[hp[1], hcols], Hg[hp[1], hcols]
    if bounds is not None:
        crl, cru, cel, ceu = [np.asarray(b, dtype=np.float64) for b in bounds]
        out["gl"] = np.concatenate([np.zeros(cb[2]), (ws * w[:, None] * crl[None, :]).ravel(), cel])
        out["gu"] = np.concatenate([np.zeros(cb[2]), (ws * w[:, None] * cru[None, :]).ravel(), ceu])
        out["xl"] = np.concatenate([[0.0], np.full(n - 1, -np.inf)])
        out["xu"] = np.full(n, np.inf)
    return out
