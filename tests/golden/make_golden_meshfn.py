"""Generates tests/golden/meshfn_reference.npz: inputs and float64-rounded results of the functions over a collocation mesh
of include/smooth_feedback_amd/mesh_function.hpp (mesh_eval, mesh_integrate, mesh_dyn with first derivatives and
multiplier-weighted second derivatives), computed with mpmath at 60 digits.  Nothing goes through the headers,
tests/meshfn_ref.py or numpy arithmetic; the LGR nodes, weights and differentiation matrices are those of
make_golden_mesh.py next to this file (its Mesh class), numpy only draws the inputs and stores the rounded results.

Variables y = [t0 | tf | x_0 .. x_N | u_0 .. u_{N-1}], numVars = 2 + nx (N + 1) + nu N; node i has time
t_i = t0 + (tf - t0) tau_i, so with z = (t, x, u) the local variables (t0, tf, x_i, u_i) reach z through G = dz/dy_loc:
row t = (1 - tau_i, tau_i, 0 ..), identity on x_i and u_i.  With J_r and H_r the gradient and Hessian of output r of the
integrand in z, h = tf - t0 and grad h = (-1, 1, 0 ..):
  eval       F[i nf + r] = w f_r (w = the quadrature weight when scaled, else 1);  gradient w G' J_r;  Hessian w G' H_r G
  integrate  F[r] = sum_i w_i h f_r;  gradient sum_i w_i (h G' J_r + f_r grad h);
             Hessian sum_i w_i (h G' H_r G + grad h (G' J_r)' + (G' J_r) grad h')
  dyn        F[i nx + d] = w_i (h f_d - sum_k D(k, j) x_{M + k, d}) for node i = M + j of an interval with differentiation
             matrix D on [0, 1]; gradient and Hessian as one term of integrate, and -w_i D(k, j) at x_{M + k, d}
and d2F = sum_rows lambda_row Hessian_row.  Stored per case and function: F, the values dF of the gradient in the order of the
structural pattern sorted by (row, column) -- eval: row (i, r) has t0, tf, x_i, u_i; integrate: every column; dyn: row (i, d)
has t0, tf, column d of every x_{M + k}, all of x_i, u_i -- and d2F, the upper triangle sorted by (column, row) over the
structural pattern (t0, tf) x everything and the (x_i, u_i) blocks of every node.  eval is stored unscaled and scaled.

  mesh.*   the op scripts of the meshes: k1 one interval of one point; m36 Mesh<3, 6>(2, 3) with its second half split
           in three and one degree raised (K = 3, 5, 3, 3: mixed degrees, unequal lengths); m46 Mesh<4, 6> after
           refine_ph(0, 8), refine_ph(0, 5) (K = 5, 4); k13 Mesh<13, 13>(2); u13 Mesh<4, 4>(13), the MPC's 13 x 4.
  fn.*     the integrands as term tables: output r = sum of coef phi_ka(z_a) phi_kb(z_b) over rows (r, a, ka, b, kb),
           phi_0 = 1, phi_1 = z, phi_2 = z^2, phi_3 = sin z, phi_4 = cos z: poly (nx, nu, nf = 3, 2, 3; polynomial and bilinear),
           cost (3, 2, 1), scalar (1, 0, 1), trig (12, 2, 12), and vehicle: the example vehicle's dynamics on SE2 x R^3 with
           inputs R^2 written on its tangent coordinates (the pose does not enter, so every pose column of the
           right-Jacobian is zero); its states are stored in the harness's flat form (x, y, cos, sin, v) as xs_flat.
  case.*   (mesh, integrand) pairs: t0, tf, xs [N + 1][nx], us [N][nu], lambda per function (doubles, exact from there on).
           The trig integrand on u13 and the vehicle carry orders 0 and 1 only; nf != nx carries no dyn.
Run by hand from the repository root (about a minute):  python tests/golden/make_golden_meshfn.py"""
import importlib.util
import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_mesh", os.path.join(HERE, "make_golden_mesh.py"))
GM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GM)
assert mp.mp.dps == 60
f64, mpf = GM.f64, GM.mpf

MESHES = {  # name: (Kmin, Kmax, n, k, ops)
    "k1": (1, 2, 1, 1, []),
    "m36": (3, 6, 2, 3, [(0, 1, 7), (3, 1, 5)]),
    "m46": (4, 6, 1, 4, [(0, 0, 8), (0, 0, 5)]),
    "k13": (13, 13, 2, 13, []),
    "u13": (4, 4, 13, 4, []),
}


def _trig_terms():
    rows = []
    for p in range(6):
        a, b, nxt = 1 + 2 * p, 2 + 2 * p, 1 + (2 * p + 2) % 12
        rows += [(2 * p, b, 1, 0, 0, 1.0), (2 * p, a, 3, 0, 4, 0.1),
                 (2 * p + 1, a, 3, 0, 0, -1.0), (2 * p + 1, b, 1, nxt, 1, -0.2), (2 * p + 1, 13 + p % 2, 1, a, 4, 1.0), (2 * p + 1, 0, 1, b, 1, 0.05)]
    return rows


FNS = {  # name: (nx, nu, nf, rows (r, a, ka, b, kb, coef)); z index 0 = t, 1 .. nx = x, then u
    "poly": (3, 2, 3, [(0, 0, 1, 1, 1, 0.7), (0, 2, 1, 4, 1, 1.3), (0, 3, 2, 0, 0, 0.5), (0, 5, 2, 0, 0, -0.2), (0, 0, 0, 0, 0, 0.4),
                       (1, 1, 1, 2, 1, 1.0), (1, 5, 1, 0, 1, -0.6), (1, 0, 2, 0, 0, 0.3), (1, 3, 1, 4, 1, 0.9),
                       (2, 3, 1, 5, 1, -0.8), (2, 1, 2, 0, 1, 0.25), (2, 4, 1, 5, 1, 1.1), (2, 2, 1, 0, 0, -0.5)]),
    "cost": (3, 2, 1, [(0, 1, 2, 0, 0, 0.5), (0, 2, 2, 0, 0, 0.7), (0, 3, 2, 0, 0, 0.2), (0, 4, 2, 0, 0, 0.1), (0, 5, 2, 0, 0, 0.3),
                       (0, 1, 1, 5, 1, 0.4), (0, 0, 2, 4, 1, 0.3), (0, 0, 1, 2, 1, 0.05)]),
    "scalar": (1, 0, 1, [(0, 1, 1, 0, 0, -0.8), (0, 0, 2, 0, 0, 0.5), (0, 1, 3, 0, 4, 0.3)]),
    "trig": (12, 2, 12, _trig_terms()),
    "vehicle": (6, 2, 6, [(0, 4, 1, 0, 0, 1.0), (1, 5, 1, 0, 0, 1.0), (2, 6, 1, 0, 0, 1.0), (3, 4, 1, 0, 0, -0.2), (3, 7, 1, 0, 0, 1.0),
                          (5, 6, 1, 0, 0, -0.4), (5, 8, 1, 0, 0, 1.0)]),
}
CASES = [  # name, mesh, integrand, highest order
    ("poly_k1", "k1", "poly", 2), ("poly_m36", "m36", "poly", 2), ("poly_m46", "m46", "poly", 2), ("poly_k13", "k13", "poly", 2),
    ("poly_u13", "u13", "poly", 2),
    ("cost_k1", "k1", "cost", 2), ("cost_m36", "m36", "cost", 2), ("cost_m46", "m46", "cost", 2),
    ("scalar_k1", "k1", "scalar", 2), ("scalar_k13", "k13", "scalar", 2), ("scalar_u13", "u13", "scalar", 2),
    ("trig_m46", "m46", "trig", 2), ("trig_u13", "u13", "trig", 1),
    ("vehicle_m36", "m36", "vehicle", 1), ("vehicle_k13", "k13", "vehicle", 1),
]


def phi(k, z):
    return [(mp.mpf(1), mp.mpf(0), mp.mpf(0)), (z, mp.mpf(1), mp.mpf(0)), (z * z, 2 * z, mp.mpf(2)), (mp.sin(z), mp.cos(z), -mp.sin(z)),
            (mp.cos(z), -mp.sin(z), -mp.cos(z))][k]


def model(fn, z):
    """f [nf], J [nf][nv], H [nf][nv][nv] of the integrand at z = (t, x, u)"""
    nx, nu, nf, rows = FNS[fn]
    nv = 1 + nx + nu
    f = [mp.mpf(0)] * nf
    J = [[mp.mpf(0)] * nv for _ in range(nf)]
    H = [[[mp.mpf(0)] * nv for _ in range(nv)] for _ in range(nf)]
    for r, a, ka, b, kb, c in rows:
        c = mpf(c)
        A, B = phi(ka, z[a]), phi(kb, z[b])
        f[r] += c * A[0] * B[0]
        J[r][a] += c * A[1] * B[0]
        J[r][b] += c * A[0] * B[1]
        H[r][a][a] += c * A[2] * B[0]
        H[r][a][b] += c * A[1] * B[1]
        H[r][b][a] += c * A[1] * B[1]
        H[r][b][b] += c * A[0] * B[2]
    return f, J, H


def functions(m, fn, t0, tf, xs, us, lam, order):
    """{key: list} for the three functions on mesh m (make_golden_mesh.Mesh); xs, us, lam: mpf"""
    nx, nu, nf, _ = FNS[fn]
    S = len(m.iv)
    N = sum(m.K(s) for s in range(S))
    taus, wts = m.all(m.nodes), m.all(m.weights)
    h = tf - t0
    nloc = 2 + nx + nu
    u_base = 2 + nx * (N + 1)
    which = {"eval": nf, "evals": nf, "integrate": nf}
    if nf == nx:
        which["dyn"] = nx
    F = {k: [mp.mpf(0)] * (nf if k == "integrate" else N * nf) for k in which}
    dF = {k: {} for k in which}
    d2 = {k: {} for k in which}
    node_of = []
    for s in range(S):
        node_of += [(s, j) for j in range(m.K(s))]
    starts = np.cumsum([0] + [m.K(s) for s in range(S)])
    for i in range(N):
        s, j = node_of[i]
        tau, w = taus[i], wts[i]
        cols = [0, 1] + [2 + i * nx + c for c in range(nx)] + [u_base + i * nu + c for c in range(nu)]
        z = [t0 + h * tau] + list(xs[i]) + list(us[i])
        f, J, H = model(fn, z)
        G = [[mp.mpf(0)] * nloc for _ in range(1 + nx + nu)]   # dz / dy_loc
        G[0][0], G[0][1] = 1 - tau, tau
        for c in range(nx + nu):
            G[1 + c][2 + c] = mp.mpf(1)
        gh = [mp.mpf(-1), mp.mpf(1)] + [mp.mpf(0)] * (nx + nu)
        for r in range(nf):
            gJ = [mp.fsum(G[a][p] * J[r][a] for a in range(1 + nx + nu)) for p in range(nloc)]
            gH = None
            if order >= 2:
                HG = [[mp.fsum(H[r][a][b] * G[b][q] for b in range(1 + nx + nu)) for q in range(nloc)] for a in range(1 + nx + nu)]
                gH = [[mp.fsum(G[a][p] * HG[a][q] for a in range(1 + nx + nu)) for q in range(nloc)] for p in range(nloc)]
            for key in which:
                scaled = key != "eval"
                ww = w if scaled else mp.mpf(1)
                timed = key in ("integrate", "dyn")
                row = r if key == "integrate" else i * nf + r
                F[key][row] += ww * (h if timed else 1) * f[r]
                for p in range(nloc):
                    v = ww * ((h * gJ[p] + f[r] * gh[p]) if timed else gJ[p])
                    dF[key][(row, cols[p])] = dF[key].get((row, cols[p]), mp.mpf(0)) + v
                if order >= 2:
                    lm = lam[key][row]
                    for p in range(nloc):
                        for q in range(nloc):
                            if cols[p] > cols[q]:
                                continue
                            v = gH[p][q] * (h if timed else 1)
                            if timed:
                                v += gh[p] * gJ[q] + gJ[p] * gh[q]
                            d2[key][(cols[q], cols[p])] = d2[key].get((cols[q], cols[p]), mp.mpf(0)) + lm * ww * v
        if "dyn" in which:
            D = m.diffmat(s) if j == 0 else D    # noqa: F821  (one matrix per interval)
            M0 = int(starts[s])
            for d in range(nx):
                row = i * nx + d
                for k in range(m.K(s) + 1):
                    F["dyn"][row] -= w * D[k, j] * xs[M0 + k][d]
                    key = (row, 2 + (M0 + k) * nx + d)
                    dF["dyn"][key] = dF["dyn"].get(key, mp.mpf(0)) - w * D[k, j]
    if order >= 1:   # integrate's pattern is dense: the columns of x_N are structural zeros
        for r in range(nf):
            for c in range(nx):
                dF["integrate"][(r, 2 + N * nx + c)] = mp.mpf(0)
    out = {}
    for key in which:
        out[key + ".F"] = f64(F[key])
        if order >= 1:
            out[key + ".dF"] = f64([dF[key][k] for k in sorted(dF[key])])
        if order >= 2:
            out[key + ".d2F"] = f64([d2[key][k] for k in sorted(d2[key])])
    return out


def main():
    rng = np.random.default_rng(20260)
    out = {"mesh.names": np.array(sorted(MESHES)), "fn.names": np.array(sorted(FNS)), "case.names": np.array([c[0] for c in CASES])}
    for name, (kmin, kmax, n, k, ops) in MESHES.items():
        m = GM.Mesh(kmin, kmax, n, k).run(ops, [])
        pre = "mesh.%s." % name
        out[pre + "spec"] = np.array([kmin, kmax, n, k], dtype=np.int32)
        out[pre + "ops"] = np.array(ops, dtype=np.int32).reshape(-1, 3)
        out[pre + "K"] = np.array([m.K(i) for i in range(len(m.iv))], dtype=np.int32)
        out[pre + "tau0"] = f64([v[1] for v in m.iv])
    for name, (nx, nu, nf, rows) in FNS.items():
        pre = "fn.%s." % name
        out[pre + "dims"] = np.array([nx, nu, nf], dtype=np.int32)
        out[pre + "terms"] = np.array([r[:5] for r in rows], dtype=np.int32)
        out[pre + "coef"] = np.array([r[5] for r in rows], dtype=np.float64)
    for name, mesh, fn, order in CASES:
        kmin, kmax, n, k, ops = MESHES[mesh]
        m = GM.Mesh(kmin, kmax, n, k).run(ops, [])
        nx, nu, nf, _ = FNS[fn]
        N = sum(m.K(s) for s in range(len(m.iv)))
        t0, tf = np.round(rng.uniform(-0.5, 0.5), 3), np.round(rng.uniform(1.5, 3.0), 3)
        xs, us = rng.uniform(-1, 1, (N + 1, nx)), rng.uniform(-1, 1, (N, nu))
        pre = "case.%s." % name
        if fn == "vehicle":
            th = rng.uniform(-3, 3, N + 1)
            out[pre + "xs_flat"] = np.column_stack([rng.uniform(-2, 2, (N + 1, 2)), np.cos(th), np.sin(th), xs[:, 3:]])
            xs[:, :3] = 0.0   # tangent coordinates: the pose does not enter the dynamics
        lam = {key: rng.uniform(-1, 1, nf if key == "integrate" else N * nf) for key in ("eval", "evals", "integrate", "dyn")}
        lam["evals"] = lam["eval"]
        out.update({pre + "mesh": np.array(mesh), pre + "fn": np.array(fn), pre + "order": np.array(order, dtype=np.int32),
                    pre + "t0": np.array(t0), pre + "tf": np.array(tf), pre + "xs": xs, pre + "us": us})
        if order >= 2:
            out.update({pre + "lambda." + key: lam[key] for key in ("eval", "integrate", "dyn") if key != "dyn" or nf == nx})
        mx = [[mpf(v) for v in row] for row in xs]
        mu = [[mpf(v) for v in row] for row in us]
        ml = {key: [mpf(v) for v in lam[key]] for key in lam}
        res = functions(m, fn, mpf(t0), mpf(tf), mx, mu, ml, order)
        out.update({pre + key: v for key, v in res.items()})
        print(name, {key: v.shape for key, v in res.items()})
    path = os.path.join(HERE, "meshfn_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
