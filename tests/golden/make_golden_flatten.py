"""Writes tests/golden/flatten_reference.npz: high-precision values for flatten_ocp (include/smooth_feedback_amd/ocp_flatten.hpp).

Everything is computed on the MATRIX groups with mpmath's expm / logm and by differences of those, at 90 digits, and shares no
formula with lie.hpp or ocp_flatten.hpp:
  dr_exp(a)                 column j = d/dh log(exp(-a) exp(a + h e_j)) at h = 0, central difference at h = 1e-25 (error 1e-50)
  d/de (dr_expinv(e) w)     central differences at 1e-18 of dr_exp(e)^-1 w (error 1e-32)
  the flat functions        the two example problems of examples/ocp_se2_model.h restated on matrices; dynamics
                            dr_exp(e)^-1 (f(xl (+) e, ul (+) v) - dxl) + ad(e) dxl with ad from the matrix commutator
  their Jacobians           central differences at 1e-18 of the flat VALUES in (t | e | v) and (tf | e0 | ef | q): not the chain rule
Layout: agents of the harness (examples/flat_ocp_harness.h): x [A][n] = [tf | q | e_0 .. e_N | v_0 .. v_{N-1}] on N = 3 nodes
tau, traj [A][row] = [x0 | xi | u0 | du]; the node arrays as sfb_ocp_nlp_batch takes them.  Agent a has the rotation parts of
its e at level a: 0 (e = 0), 1e-9, 0.3, 1.0; tf alternates between two values.

    python tests/golden/make_golden_flatten.py
"""
import os

import numpy as np
from mpmath import mp, mpf, matrix, expm, logm, eye, zeros, lu_solve

mp.dps = 90
H1 = mpf(10) ** -25
H2 = mpf(10) ** -18
LEVELS = (0.0, 1e-9, 0.3, 1.0)


# ---- matrix groups: kind -> (dof, matrix size, hat) ----
def hat(kind, a):
    if kind == "SE2":
        return matrix([[0, -a[2], a[0]], [a[2], 0, a[1]], [0, 0, 0]])
    if kind == "SO3":
        return matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    if kind == "SE3":
        return matrix([[0, -a[5], a[4], a[0]], [a[5], 0, -a[3], a[1]], [-a[4], a[3], 0, a[2]], [0, 0, 0, 0]])
    raise KeyError(kind)


def vee(kind, M):
    if kind == "SE2":
        return [M[0, 2], M[1, 2], M[1, 0]]
    if kind == "SO3":
        return [M[2, 1], M[0, 2], M[1, 0]]
    if kind == "SE3":
        return [M[0, 3], M[1, 3], M[2, 3], M[2, 1], M[0, 2], M[1, 0]]
    raise KeyError(kind)


DOF = dict(SE2=3, SO3=3, SE3=6)


def gexp(kind, a):
    return expm(hat(kind, a))


def glog(kind, M):
    return vee(kind, logm(M))


def ad_matrix(kind, a):
    """column j = vee([hat a, hat e_j])"""
    T = DOF[kind]
    A = hat(kind, a)
    out = zeros(T, T)
    for j in range(T):
        E = hat(kind, [mpf(1) if k == j else mpf(0) for k in range(T)])
        c = vee(kind, A * E - E * A)
        for i in range(T):
            out[i, j] = c[i]
    return out


def dr_exp_part(kind, a):
    T = DOF[kind]
    a = [mpf(v) for v in a]
    Ainv = gexp(kind, [-v for v in a])
    out = zeros(T, T)
    for j in range(T):
        ap = list(a); am = list(a)
        ap[j] += H1; am[j] -= H1
        lp = glog(kind, Ainv * gexp(kind, ap)); lm = glog(kind, Ainv * gexp(kind, am))
        for i in range(T):
            out[i, j] = (lp[i] - lm[i]) / (2 * H1)
    return out


# a group is a list of parts (kind, dof); "R" parts are vectors
def parts_dof(parts):
    return sum(d for _, d in parts)


def blockdiag(parts, fn, a):
    T = parts_dof(parts)
    out = zeros(T, T)
    off = 0
    for kind, d in parts:
        blk = eye(d) if kind == "R" else fn(kind, a[off:off + d])
        for i in range(d):
            for j in range(d):
                out[off + i, off + j] = blk[i, j]
        off += d
    return out


def dr_exp(parts, a):
    return blockdiag(parts, dr_exp_part, a)


def ad(parts, a):
    T = parts_dof(parts)
    out = zeros(T, T)
    off = 0
    for kind, d in parts:
        if kind != "R":
            blk = ad_matrix(kind, [mpf(v) for v in a[off:off + d]])
            for i in range(d):
                for j in range(d):
                    out[off + i, off + j] = blk[i, j]
        off += d
    return out


def dr_expinv_times(parts, e, w):
    return list(lu_solve(dr_exp(parts, e), matrix(w)))


def d_expinv(parts, e, w):
    T = parts_dof(parts)
    e = [mpf(v) for v in e]; w = [mpf(v) for v in w]
    out = zeros(T, T)
    for j in range(T):
        ep = list(e); em = list(e)
        ep[j] += H2; em[j] -= H2
        vp = dr_expinv_times(parts, ep, w); vm = dr_expinv_times(parts, em, w)
        for i in range(T):
            out[i, j] = (vp[i] - vm[i]) / (2 * H2)
    return out


# elements: list per part, a matrix or a vector (list)
def elem_from_doubles(parts, p):
    out = []
    off = 0
    for kind, d in parts:
        if kind == "R":
            out.append([mpf(float(v)) for v in p[off:off + d]]); off += d
        elif kind == "SE2":
            x, y, c, s = [mpf(float(v)) for v in p[off:off + 4]]; off += 4
            nrm = mp.sqrt(c * c + s * s); c /= nrm; s /= nrm
            out.append(matrix([[c, -s, x], [s, c, y], [0, 0, 1]]))
        elif kind == "SE3":
            px, py, pz, w, x, y, z = [mpf(float(v)) for v in p[off:off + 7]]; off += 7
            nrm = mp.sqrt(w * w + x * x + y * y + z * z); w /= nrm; x /= nrm; y /= nrm; z /= nrm
            R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
            out.append(matrix([R[0] + [px], R[1] + [py], R[2] + [pz], [0, 0, 0, 1]]))
    return out


def rplus(parts, g, a):
    out = []
    off = 0
    for (kind, d), gp in zip(parts, g):
        seg = a[off:off + d]; off += d
        out.append([gp[i] + seg[i] for i in range(d)] if kind == "R" else gp * gexp(kind, seg))
    return out


def rminus(parts, a, b):
    out = []
    for (kind, d), ap, bp in zip(parts, a, b):
        out += [ap[i] - bp[i] for i in range(d)] if kind == "R" else glog(kind, bp ** -1 * ap)
    return out


def identity(parts):
    return [[mpf(0)] * d if kind == "R" else eye(3 if kind != "SE3" else 4) for kind, d in parts]


# ---- the two problems of examples/ocp_se2_model.h ----
class SE2Problem:
    name = "se2"
    X = [("SE2", 3), ("R", 2)]
    U = [("R", 2)]
    nx, nu, nq, ncr, nce, EX = 5, 2, 1, 2, 6, 6

    def xdes(self, t):
        return [gexp("SE2", [t * 1, mpf(0), t * mpf("0.5")]), [mpf(1), mpf("0.5")]]

    def f(self, t, x, u):
        return [x[1][0], mpf(0), x[1][1], u[0][0], u[0][1]]


DAMP = [mpf(s) for s in ("0.2", "0.3", "0.25", "0.4", "0.35", "0.5")]


class SE3Problem:
    name = "se3"
    X = [("SE3", 6), ("R", 6)]
    U = [("R", 6)]
    nx, nu, nq, ncr, nce, EX = 12, 6, 1, 6, 13, 13
    XI = [mpf(s) for s in ("0.8", "0.0", "0.15", "0.1", "-0.05", "0.4")]
    START = [mpf("2.5"), mpf(0), mpf(1), mpf("0.3"), mpf("-0.2"), mpf(1.5707963267948966)]

    def xdes(self, t):
        return [gexp("SE3", self.START) * gexp("SE3", [t * v for v in self.XI]), list(self.XI)]

    def f(self, t, x, u):
        R = x[0][0:3, 0:3]
        gb = R.T * matrix([0, 0, -1])
        w = x[1]
        return [w[i] for i in range(6)] + [u[0][i] - DAMP[i] * w[i] + (gb[i] if i < 3 else 0) for i in range(6)]


def integrand(P, t, x, u):
    a = rminus(P.X, x, P.xdes(t))
    return [(sum(v * v for v in a) + sum(v * v for v in u[0])) / 2]


def make_flat(P, row):
    """the flat functions of one agent: row = [x0 | xi | u0 | du] (float64)"""
    x0 = elem_from_doubles(P.X, row[:P.EX])
    xi = [mpf(float(v)) for v in row[P.EX:P.EX + P.nx]]
    u0 = [mpf(float(v)) for v in row[P.EX + P.nx:P.EX + P.nx + P.nu]]
    du = [mpf(float(v)) for v in row[P.EX + P.nx + P.nu:]]

    def xl(t):
        return rplus(P.X, x0, [t * v for v in xi])

    def ul(t):
        return [[u0[i] + t * du[i] for i in range(P.nu)]]

    def xu(z):
        t, e, v = z[0], z[1:1 + P.nx], z[1 + P.nx:]
        return t, e, rplus(P.X, xl(t), e), rplus(P.U, ul(t), v)

    def dyn(z):
        t, e, x, u = xu(z)
        w = [a - b for a, b in zip(P.f(t, x, u), xi)]
        first = dr_expinv_times(P.X, e, w)
        second = ad(P.X, e) * matrix(xi)
        return [first[i] + second[i] for i in range(P.nx)]

    def g(z):
        t, e, x, u = xu(z)
        return integrand(P, t, x, u)

    def cr(z):
        t, e, x, u = xu(z)
        return list(u[0])

    def ends(z):
        tf, e0, ef, q = z[0], z[1:1 + P.nx], z[1 + P.nx:1 + 2 * P.nx], z[1 + 2 * P.nx:]
        return tf, rplus(P.X, xl(mpf(0)), e0), rplus(P.X, xl(tf), ef), q

    def ce(z):
        tf, xa, xf, q = ends(z)
        return [tf] + rminus(P.X, xa, identity(P.X))

    def theta(z):
        tf, xa, xf, q = ends(z)
        return [tf + q[0]]

    return dict(f=dyn, g=g, cr=cr, ce=ce, theta=theta)


def jacobian(fn, z):
    z = [mpf(v) for v in z]
    cols = []
    for j in range(len(z)):
        zp = list(z); zm = list(z)
        zp[j] += H2; zm[j] -= H2
        fp = fn(zp); fm = fn(zm)
        cols.append([(a - b) / (2 * H2) for a, b in zip(fp, fm)])
    return [[cols[j][i] for j in range(len(z))] for i in range(len(cols[0]))]


def f64(v):
    return np.array(v, dtype=object).astype(np.float64) if not isinstance(v, matrix) else np.array(v.tolist(), dtype=object).astype(np.float64)


def tangent_at_level(rng, parts, level):
    """a tangent whose rotation parts have norm `level`, the other entries of order 1 (0 everywhere at level 0)"""
    out = []
    for kind, d in parts:
        a = rng.uniform(-0.8, 0.8, d)
        if level == 0.0:
            a[:] = 0.0
        elif kind == "SE2":
            a[2] = level
        elif kind == "SO3":
            a *= level / np.linalg.norm(a)
        elif kind == "SE3":
            a[3:] *= level / np.linalg.norm(a[3:])
        out += list(a)
    return np.array(out)


LIE_GROUPS = dict(SE2=[("SE2", 3)], SO3=[("SO3", 3)], SE3=[("SE3", 6)], X5=[("SE2", 3), ("R", 2)], X12B=[("SE3", 6), ("R", 6)])


def main():
    rng = np.random.default_rng(20240917)
    out = {}
    out["lie.names"] = np.array(list(LIE_GROUPS))
    for name, parts in LIE_GROUPS.items():
        T = parts_dof(parts)
        A, W, D, E = [], [], [], []
        for level in LEVELS:
            a = tangent_at_level(rng, parts, level)
            w = rng.uniform(-1.0, 1.0, T)
            A.append(a); W.append(w)
            D.append(f64(dr_exp(parts, [mpf(float(v)) for v in a])))
            E.append(f64(d_expinv(parts, [float(v) for v in a], [float(v) for v in w])))
            print("lie", name, level, flush=True)
        out["lie.%s.a" % name] = np.array(A); out["lie.%s.w" % name] = np.array(W)
        out["lie.%s.dr_exp" % name] = np.array(D); out["lie.%s.d_expinv" % name] = np.array(E)
    N = 3
    tau = np.array([0.0, 0.35, 0.8])
    out["tau"] = tau
    out["prob.names"] = np.array(["se2", "se3"])
    for P in (SE2Problem(), SE3Problem()):
        nz, ne = 1 + P.nx + P.nu, 1 + 2 * P.nx + P.nq
        n = 1 + P.nq + (N + 1) * P.nx + N * P.nu
        A = len(LEVELS)
        x = np.zeros((A, n)); traj = np.zeros((A, P.EX + P.nx + 2 * P.nu))
        res = {k: [] for k in ("Ff", "dFf", "Fg", "dFg", "Fcr", "dFcr", "ce", "dce", "theta", "dtheta")}
        for a, level in enumerate(LEVELS):
            # trajectories: the identity start for even agents, a turned start for odd ones (elements exact in float64 to 1e-17)
            if P.name == "se2":
                traj[a, :P.EX] = [0, 0, 1, 0, 0.3, -0.1] if a % 2 == 0 else [0.4, -0.3, 0.6, 0.8, 0.2, 0.1]
            else:
                traj[a, :P.EX] = [0, 0, 0, 1, 0, 0, 0] + [0.1] * 6 if a % 2 == 0 else [0.3, -0.2, 0.5, 0.8, 0, 0.6, 0] + list(rng.uniform(-0.3, 0.3, 6))
            traj[a, P.EX:] = rng.uniform(-0.5, 0.5, P.nx + 2 * P.nu)
            x[a, 0] = 1.7 if a % 2 == 0 else 3.1
            x[a, 1] = rng.uniform(0.1, 1.0)
            for i in range(N + 1):
                x[a, 1 + P.nq + i * P.nx:1 + P.nq + (i + 1) * P.nx] = tangent_at_level(rng, P.X, level)
            x[a, 1 + P.nq + (N + 1) * P.nx:] = rng.uniform(-0.5, 0.5, N * P.nu)
            fl = make_flat(P, traj[a])
            for i in range(N):
                t = float(x[a, 0]) * float(tau[i])  # the float64 product, as the front forms it
                z = [mpf(t)] + [mpf(float(v)) for v in x[a, 1 + P.nq + i * P.nx:1 + P.nq + (i + 1) * P.nx]] + \
                    [mpf(float(v)) for v in x[a, 1 + P.nq + (N + 1) * P.nx + i * P.nu:1 + P.nq + (N + 1) * P.nx + (i + 1) * P.nu]]
                for key, fn in (("f", "f"), ("g", "g"), ("cr", "cr")):
                    res["F" + key].append(f64(fl[fn](z))); res["dF" + key].append(f64(jacobian(fl[fn], z)))
                print(P.name, "agent", a, "node", i, flush=True)
            ze = [mpf(float(x[a, 0]))] + [mpf(float(v)) for v in x[a, 1 + P.nq:1 + P.nq + P.nx]] + \
                 [mpf(float(v)) for v in x[a, 1 + P.nq + N * P.nx:1 + P.nq + (N + 1) * P.nx]] + [mpf(float(x[a, 1]))]
            for key in ("ce", "theta"):
                res[key].append(f64(fl[key](ze))); res["d" + key].append(f64(jacobian(fl[key], ze)))
        pre = "prob.%s." % P.name
        out[pre + "x"] = x; out[pre + "traj"] = traj
        out[pre + "dims"] = np.array([P.nx, P.nu, P.nq, P.ncr, P.nce], dtype=np.int32)
        for key, nf in (("f", P.nx), ("g", P.nq), ("cr", P.ncr)):
            out[pre + "F" + key] = np.array(res["F" + key]).reshape(A, N, nf)
            out[pre + "dF" + key] = np.array(res["dF" + key]).reshape(A, N, nf, nz)
        out[pre + "ce"] = np.array(res["ce"]).reshape(A, P.nce); out[pre + "dce"] = np.array(res["dce"]).reshape(A, P.nce, ne)
        out[pre + "theta"] = np.array(res["theta"]).reshape(A); out[pre + "dtheta"] = np.array(res["dtheta"]).reshape(A, ne)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flatten_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
