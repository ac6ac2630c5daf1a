"""Generates tests/golden/ocpnlp_reference.npz: the collocation NLP of an optimal control problem over a ph mesh
(include/smooth_feedback_amd/ocp_to_nlp.hpp, sfb_ocp_nlp_* of include/sfb.h), every value computed with mpmath at 60 digits from
the definitions.  Nothing goes through the headers, tests/ocpnlp_ref.py or numpy arithmetic; the LGR nodes, weights and
differentiation matrices are those of make_golden_mesh.py next to this file (its Mesh class).

The problem: minimise theta(tf, x(0), x(tf), q) subject to x' = f(t, x, u), q = int_0^tf g, crl <= cr(t, x, u) <= cru,
cel <= ce(tf, x(0), x(tf), q) <= ceu.  On a mesh with nodes tau_i, weights w_i (i < N) and end point tau_N = 1 the NLP has
  y = [tf | q (nq) | x_0 .. x_N | u_0 .. u_{N-1}],   t_i = tf tau_i,   ws = 1 / max(1e-6, max_i w_i),
  c_dyn[i nx + d] = ws w_i (tf f_d(t_i, x_i, u_i) - sum_k D_s(k, j) x_{M_s + k, d})     node i = M_s + j of interval s, D_s its
                                                                                      differentiation matrix on [0, 1]
  c_int[r]        = ws (sum_i w_i tf g_r(t_i, x_i, u_i) - q_r)
  c_cr[i ncr + r] = ws w_i cr_r(t_i, x_i, u_i)
  c_ce            = ce(tf, x_0, x_N, q)
and objective theta(tf, x_0, x_N, q).  Every row is a scalar function of y; its gradient and Hessian follow from the chain
rule through z_i = (tf tau_i, x_i, u_i) (dz/dy is tau_i at (t, tf) and the identity on x_i, u_i) and the product with tf:
  grad (tf phi) = tf grad phi + phi e_tf,   hess (tf phi) = tf hess phi + e_tf grad phi' + grad phi e_tf'.
Stored per case: x, lambda, dims, the term tables, the bounds (crl, cru, cel, ceu), w_scaling, xl, xu, gl, gu, var_beg, con_beg,
the pattern of dg (CSR: the structural entries of every row, sorted by column -- an entry is structural when the row's
definition touches that variable, whatever its value) with the values dg, the upper-triangle pattern shared by d2f and d2g
(CSC: the union of what any row of c, or theta, touches twice) with the values d2f and d2g = hess (lambda' c), and f, df
(dense, n), g.  Functions are term tables: output r = sum of coef phi_ka(z_a) phi_kb(z_b) phi_kc(z_c) over rows
(r, a, ka, b, kb, c, kc), phi as in make_golden_meshfn.py; z = (t | x | u) for f, g, cr and (tf | x0 | xf | q) for theta, ce.

  bare   one interval, K = 1, dims (1, 0, 0, 0, 0): every segment but one is empty
  ref    the problem of the reference's tests/test_ocp_to_nlp.cpp on Mesh<3, 3> after refine_ph(0, 4) twice, dims (2, 1, 1, 4, 6)
  cross  as ref, with q x0 and q xf products in theta and ce
  mixed  Mesh<3, 6> with K = 3, 5, 3, 3 and unequal lengths (m36 of make_golden_meshfn.py), dims (3, 2, 2, 1, 3)
  k13    Mesh<13, 13>(2), dims (3, 2, 1, 3, 2)
Run by hand from the repository root (a few minutes):  python tests/golden/make_golden_ocpnlp.py"""
import importlib.util
import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_meshfn", os.path.join(HERE, "make_golden_meshfn.py"))
GF = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GF)
GM = GF.GM
assert mp.mp.dps == 60
f64, mpf, phi = GM.f64, GM.mpf, GF.phi

MESHES = {  # name: (Kmin, Kmax, n, k, ops)
    "k1": GF.MESHES["k1"],
    "r33": (3, 3, 1, 3, [(0, 0, 4), (0, 0, 4)]),
    "m36": GF.MESHES["m36"],
    "k13": GF.MESHES["k13"],
}

# z = (t, x1, x2, u) and (tf, x01, x02, xf1, xf2, q)
REF = {
    "f": [(0, 2, 1, 0, 0, 0, 0, 1.0), (0, 0, 1, 0, 0, 0, 0, 1.0), (1, 1, 1, 3, 2, 0, 0, 1.0)],
    "g": [(0, 0, 1, 0, 0, 0, 0, 1.0), (0, 0, 1, 1, 2, 0, 0, 1.0), (0, 0, 1, 2, 2, 0, 0, 1.0), (0, 3, 2, 0, 0, 0, 0, 1.0)],
    "cr": [(0, 0, 1, 0, 0, 0, 0, 1.0), (1, 0, 1, 1, 1, 3, 1, 1.0), (2, 0, 1, 2, 1, 3, 1, 1.0), (3, 3, 2, 0, 0, 0, 0, 1.0)],
    "theta": [(0, 0, 2, 0, 0, 0, 0, 1.0), (0, 0, 1, 0, 0, 0, 0, -4.0), (0, 0, 0, 0, 0, 0, 0, 4.0), (0, 1, 2, 3, 2, 0, 0, 1.0),
              (0, 2, 2, 4, 2, 0, 0, 1.0), (0, 3, 2, 0, 0, 0, 0, 1.0), (0, 4, 2, 0, 0, 0, 0, 1.0), (0, 5, 1, 0, 0, 0, 0, 1.0)],
    "ce": [(0, 0, 1, 0, 0, 0, 0, 1.0), (1, 1, 1, 3, 1, 0, 0, 1.0), (2, 2, 1, 4, 1, 0, 0, 1.0), (3, 3, 1, 0, 0, 0, 0, 1.0),
           (4, 4, 1, 0, 0, 0, 0, 1.0), (5, 5, 2, 0, 0, 0, 0, 1.0)],
}
CROSS = dict(REF)
CROSS["theta"] = REF["theta"] + [(0, 5, 1, 1, 1, 0, 0, 0.7), (0, 5, 1, 4, 1, 0, 0, -0.4)]
CROSS["ce"] = REF["ce"] + [(1, 5, 1, 2, 1, 0, 0, 0.3), (4, 5, 1, 3, 1, 0, 0, 0.6)]
BARE = {"f": [(0, 1, 1, 0, 0, 0, 0, -0.8), (0, 0, 2, 0, 0, 0, 0, 0.5), (0, 1, 3, 0, 4, 0, 0, 0.3)], "g": [], "cr": [],
        "theta": [(0, 0, 2, 0, 0, 0, 0, 1.0), (0, 1, 1, 2, 1, 0, 0, 0.5), (0, 2, 3, 0, 1, 0, 0, 0.25)], "ce": []}


def drawn_tables(rng, dims):
    """term tables drawn once: per output a linear term, a product of two and a product of three coordinates"""
    nx, nu, nq, ncr, nce = dims
    out = {}
    for name, nf, nv in (("f", nx, 1 + nx + nu), ("g", nq, 1 + nx + nu), ("cr", ncr, 1 + nx + nu), ("theta", 1, 1 + 2 * nx + nq), ("ce", nce, 1 + 2 * nx + nq)):
        rows = []
        for r in range(nf):
            c = np.round(rng.uniform(-1, 1, 4), 2)
            a = rng.integers(0, nv, 7)
            k = rng.integers(1, 5, 7)
            rows += [(r, int(a[0]), 1, 0, 0, 0, 0, float(c[0])), (r, int(a[1]), int(k[1]), int(a[2]), int(k[2]), 0, 0, float(c[1])),
                     (r, int(a[3]), int(k[3]), int(a[4]), 1, int(a[5]), int(k[5]), float(c[2])), (r, r % nv, 2, int(a[6]), 1, 0, 0, float(c[3]))]
        out[name] = rows
    return out


CASES = [  # name, mesh, dims, tables (None: drawn)
    ("bare", "k1", (1, 0, 0, 0, 0), BARE),
    ("ref", "r33", (2, 1, 1, 4, 6), REF),
    ("cross", "r33", (2, 1, 1, 4, 6), CROSS),
    ("mixed", "m36", (3, 2, 2, 1, 3), None),
    ("k13", "k13", (3, 2, 1, 3, 2), None),
]


def model(rows, nf, z):
    """f [nf], J [nf][nv], H [nf][nv][nv] of a term table at z (mpf)"""
    nv = len(z)
    f = [mp.mpf(0)] * nf
    J = [[mp.mpf(0)] * nv for _ in range(nf)]
    H = [[[mp.mpf(0)] * nv for _ in range(nv)] for _ in range(nf)]
    for r, a, ka, b, kb, c, kc, coef in rows:
        idx = (a, b, c)
        P = (phi(ka, z[a]), phi(kb, z[b]), phi(kc, z[c]))
        co = mpf(coef)
        f[r] += co * P[0][0] * P[1][0] * P[2][0]
        for p in range(3):
            o = [q for q in range(3) if q != p]
            J[r][idx[p]] += co * P[p][1] * P[o[0]][0] * P[o[1]][0]
            H[r][idx[p]][idx[p]] += co * P[p][2] * P[o[0]][0] * P[o[1]][0]
            for q in o:
                s = 3 - p - q
                H[r][idx[p]][idx[q]] += co * P[p][1] * P[q][1] * P[s][0]
    return f, J, H


class Row:
    """a scalar function of y: value, gradient {col: v}, Hessian {(row, col): v}, row <= col"""

    def __init__(self):
        self.v, self.g, self.h = mp.mpf(0), {}, {}

    def add(self, scale, cols, val, grad, hess):
        """+ scale phi, phi given on the local variables cols (hess None: linear, it touches nothing twice)"""
        self.v += scale * val
        for p, cp in enumerate(cols):
            self.g[cp] = self.g.get(cp, mp.mpf(0)) + scale * grad[p]
            for q, cq in enumerate(cols if hess is not None else ()):
                if cp <= cq:
                    self.h[(cp, cq)] = self.h.get((cp, cq), mp.mpf(0)) + scale * hess[p][q]


def through_node(tau, tf, f, J, H, timed):
    """value, gradient, Hessian on (tf, x_i, u_i) of z -> phi(z), z = (tf tau, x_i, u_i); timed: of tf phi"""
    nz = len(J)
    g = [tau * J[0]] + list(J[1:])
    h = [[(tau if p == 0 else 1) * (tau if q == 0 else 1) * H[p][q] for q in range(nz)] for p in range(nz)]
    if not timed:
        return f, g, h
    e = [mp.mpf(1)] + [mp.mpf(0)] * (nz - 1)
    return tf * f, [tf * g[p] + f * e[p] for p in range(nz)], [[tf * h[p][q] + e[p] * g[q] + g[p] * e[q] for q in range(nz)] for p in range(nz)]


def nlp(m, dims, tab, y, lam):
    nx, nu, nq, ncr, nce = dims
    S = len(m.iv)
    N = sum(m.K(s) for s in range(S))
    taus, wts = m.all(m.nodes), m.all(m.weights)
    ws = 1 / max([mpf(1e-6)] + wts[:N])
    qv, xv = 1, 1 + nq
    uv = xv + nx * (N + 1)
    n = uv + nu * N
    tf, q = y[0], y[qv:xv]
    X = [y[xv + i * nx:xv + (i + 1) * nx] for i in range(N + 1)]
    U = [y[uv + i * nu:uv + (i + 1) * nu] for i in range(N)]
    dyn, integ, run = [], [Row() for _ in range(nq)], []
    i = 0
    for s in range(S):
        D, M0 = m.diffmat(s), i
        for j in range(m.K(s)):
            cols = [0] + list(range(xv + i * nx, xv + (i + 1) * nx)) + list(range(uv + i * nu, uv + (i + 1) * nu))
            z = [tf * taus[i]] + list(X[i]) + list(U[i])
            for name, nf, rows, timed in (("f", nx, dyn, True), ("g", nq, integ, True), ("cr", ncr, run, False)):
                f, J, H = model(tab[name], nf, z)
                for r in range(nf):
                    v, g, h = through_node(taus[i], tf, f[r], J[r], H[r], timed)
                    if name == "g":
                        integ[r].add(ws * wts[i], cols, v, g, h)
                        continue
                    row = Row()
                    row.add(ws * wts[i], cols, v, g, h)
                    if name == "f":
                        for k in range(m.K(s) + 1):
                            c = xv + (M0 + k) * nx + r
                            row.add(-ws * wts[i] * D[k, j], [c], X[M0 + k][r], [mp.mpf(1)], None)
                    rows.append(row)
            i += 1
    for r in range(nq):
        integ[r].add(-ws, [qv + r], q[r], [mp.mpf(1)], None)
    ecols = [0] + list(range(xv, xv + nx)) + list(range(xv + N * nx, xv + (N + 1) * nx)) + list(range(qv, qv + nq))
    ze = [tf] + list(X[0]) + list(X[N]) + list(q)

    def end_rows(name, nf):
        f, J, H = model(tab[name], nf, ze)
        out = []
        for r in range(nf):
            row = Row()
            sym = [[H[r][p][p2] if ecols[p] <= ecols[p2] else H[r][p2][p] for p2 in range(len(ze))] for p in range(len(ze))]
            row.add(mp.mpf(1), ecols, f[r], J[r], sym)
            out.append(row)
        return out

    cons = dyn + integ + run + end_rows("ce", nce)
    theta = end_rows("theta", 1)[0]
    hkeys = set(theta.h)
    for row in cons:
        hkeys |= set(row.h)
    hkeys = sorted(hkeys, key=lambda rc: (rc[1], rc[0]))
    rowptr, colind, dg = [0], [], []
    for row in cons:
        for c in sorted(row.g):
            colind.append(c)
            dg.append(row.g[c])
        rowptr.append(len(colind))
    colptr = [0] * (n + 1)
    for _, c in hkeys:
        colptr[c + 1] += 1
    df = [theta.g.get(c, mp.mpf(0)) for c in range(n)]
    d2g = [mp.fsum(lam[k] * row.h[rc] for k, row in enumerate(cons) if rc in row.h) for rc in hkeys]
    return {"w_scaling": f64([ws])[0], "f": f64([theta.v])[0], "df": f64(df), "d2f": f64([theta.h.get(rc, mp.mpf(0)) for rc in hkeys]),
            "g": f64([row.v for row in cons]), "dg": f64(dg), "d2g": f64(d2g),
            "dg.rowptr": np.array(rowptr, np.int32), "dg.colind": np.array(colind, np.int32),
            "h.colptr": np.cumsum(colptr).astype(np.int32), "h.rowind": np.array([r for r, _ in hkeys], np.int32),
            "var_beg": np.array([0, qv, xv, uv, n], np.int64),
            "con_beg": np.cumsum([0, nx * N, nq, ncr * N, nce]).astype(np.int64)}, ws, wts[:N]


def main():
    rng = np.random.default_rng(20261)
    out = {"case.names": np.array([c[0] for c in CASES]), "mesh.names": np.array(sorted(MESHES))}
    for name, (kmin, kmax, n, k, ops) in MESHES.items():
        m = GM.Mesh(kmin, kmax, n, k).run(ops, [])
        pre = "mesh.%s." % name
        out[pre + "spec"] = np.array([kmin, kmax, n, k], dtype=np.int32)
        out[pre + "ops"] = np.array(ops, dtype=np.int32).reshape(-1, 3)
        out[pre + "K"] = np.array([m.K(i) for i in range(len(m.iv))], dtype=np.int32)
        out[pre + "tau0"] = f64([v[1] for v in m.iv])
    for name, mesh, dims, tab in CASES:
        kmin, kmax, n, k, ops = MESHES[mesh]
        m = GM.Mesh(kmin, kmax, n, k).run(ops, [])
        nx, nu, nq, ncr, nce = dims
        tab = tab or drawn_tables(rng, dims)
        N = sum(m.K(s) for s in range(len(m.iv)))
        nvar, ncon = 1 + nq + nx * (N + 1) + nu * N, nx * N + nq + ncr * N + nce
        y = rng.uniform(-1, 1, nvar)
        y[0] = np.round(rng.uniform(1.5, 3.0), 3)
        lam = rng.uniform(-1, 1, ncon)
        crl, cru = np.round(rng.uniform(-2, -1, ncr), 2), np.round(rng.uniform(1, 2, ncr), 2)
        cel, ceu = np.round(rng.uniform(-2, -1, nce), 2), np.round(rng.uniform(1, 2, nce), 2)
        if tab is REF or tab is CROSS:
            crl, cru, cel, ceu = -np.ones(ncr), np.ones(ncr), -np.ones(nce), np.ones(nce)
        pre = "case.%s." % name
        res, ws, wts = nlp(m, dims, tab, [mpf(v) for v in y], [mpf(v) for v in lam])
        inf = np.full(nvar, np.inf)
        xl = -inf
        xl[0] = 0.0
        gl = [mp.mpf(0)] * (nx * N + nq) + [ws * w * mpf(v) for w in wts for v in crl] + [mpf(v) for v in cel]
        gu = [mp.mpf(0)] * (nx * N + nq) + [ws * w * mpf(v) for w in wts for v in cru] + [mpf(v) for v in ceu]
        out.update({pre + "mesh": np.array(mesh), pre + "dims": np.array(dims, dtype=np.int32), pre + "x": y, pre + "lambda": lam,
                    pre + "crl": crl, pre + "cru": cru, pre + "cel": cel, pre + "ceu": ceu, pre + "xl": xl, pre + "xu": inf,
                    pre + "gl": f64(gl).reshape(-1), pre + "gu": f64(gu).reshape(-1)})
        for fn in ("f", "g", "cr", "theta", "ce"):
            out[pre + "terms." + fn] = np.array([r[:7] for r in tab[fn]], dtype=np.int32).reshape(-1, 7)
            out[pre + "coef." + fn] = np.array([r[7] for r in tab[fn]], dtype=np.float64)
        out.update({pre + key: v for key, v in res.items()})
        print(name, "n", nvar, "m", ncon, "nnz", len(res["dg"]), "hnnz", len(res["d2g"]))
    path = os.path.join(HERE, "ocpnlp_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
