"""Generates tests/golden/lie_reference.npz: inputs and float64-rounded results of the Lie operations of
include/smooth_feedback_amd/lie.hpp (R3, SE2, SO3, Bundle<SE2,R3> = X6, Bundle<SE2,R3,SE2,R3> = X12), computed with
mpmath at 60 digits FROM THE MATRIX GROUP, not from the closed forms of lie.hpp:

  exp / log      mpmath.expm / a matrix logarithm (inverse scaling and squaring + power series) of the 3x3 homogeneous matrix (SE2) or of the rotation matrix (SO3); every log is
                 checked by expm(hat(log)) == matrix; a rotation by exactly pi (no principal logarithm there) takes
                 pi * axis with the axis of (R + I) / 2 and the sign of the quaternion's own vector part
  product        matrix product
  ad             columns vee([hat(a), hat(e_i)])
  dr_expinv      Bernoulli series  sum_n B_n^+ ad(a)^n / n!, cross-checked here against the central difference of
                 h -> log(exp(a) exp(h)) with step 1e-15 at 60 digits (every fourth input; agreement to 1e-18 relative:
                 the logarithm next to pi loses digits to the conditioning of the square roots)
  rplus, rminus  g expm(hat(a)),  log(b^-1 a);  bundles part by part

Elements are stored as lie.hpp stores them (SE2: x, y, cos, sin; SO3: w, x, y, z; bundles: parts one after the other).
An element given as doubles is not exactly on the group: the reference takes the group element it normalises to
((cos, sin) / hypot, q / |q|).  A rotation matrix has two quaternions; the fixture stores the one with w >= 0 and the
tests compare up to that sign.

Every row carries the name of its input class (npz key "<group>.<op>.cls", index into "classes").
Run by hand from the repository root (about three minutes):  python tests/golden/make_golden_lie.py
tests/test_lie_host.py regenerates a sample through sample() when mpmath is importable."""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261016
CLASSES = ["random_1p5", "random_3", "sweep", "theta0", "near_pi", "trans_1e-6", "trans_1e6", "w_negative", "pi_exact"]
PI = float(mp.pi)
CROSS_CHECK = True   # dr_expinv against the central difference of log(exp(a) exp(h)); sample() switches it off


def f64(v):
    return [float(x) for x in v]


# ---------------------------------------------------------------- matrix forms
def se2_hat(a):
    return mp.matrix([[0, -a[2], a[0]], [a[2], 0, a[1]], [0, 0, 0]])


def se2_vee(M):
    return [M[0, 2], M[1, 2], M[1, 0]]


def se2_mat(e):
    x, y, c, s = [mp.mpf(v) for v in e]
    r = mp.sqrt(c * c + s * s)
    return mp.matrix([[c / r, -s / r, x], [s / r, c / r, y], [0, 0, 1]])


def se2_elem(M):
    return [M[0, 2], M[1, 2], M[0, 0], M[1, 0]]


def so3_hat(a):
    return mp.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def so3_vee(M):
    return [M[2, 1], M[0, 2], M[1, 0]]


def so3_mat(e):
    w, x, y, z = [mp.mpf(v) for v in e]
    n = mp.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def so3_elem(R):
    """quaternion of a rotation matrix (largest-pivot extraction), the representative with w >= 0"""
    t = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2]]
    k = max(range(4), key=lambda i: t[i])
    if k == 0:
        w = mp.sqrt(1 + t[0]) / 2
        q = [w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)]
    else:
        i = k - 1
        j, l = (i + 1) % 3, (i + 2) % 3
        v = mp.sqrt(1 + R[i, i] - R[j, j] - R[l, l]) / 2
        q = [0, 0, 0, 0]
        q[0] = (R[l, j] - R[j, l]) / (4 * v)
        q[1 + i] = v
        q[1 + j] = (R[j, i] + R[i, j]) / (4 * v)
        q[1 + l] = (R[l, i] + R[i, l]) / (4 * v)
    sign = -1 if (q[0] < 0 or (q[0] == 0 and next(c for c in q[1:] if c != 0) < 0)) else 1
    return [sign * c for c in q]


def mat_err(A, B):
    return max(abs(A[i, j] - B[i, j]) / (1 + abs(B[i, j])) for i in range(A.rows) for j in range(A.cols))


def sqrtm_db(M):
    """principal square root by the Denman-Beavers iteration (no eigenvalue of M on the closed negative real axis)"""
    Y, Z = M, mp.eye(M.rows)
    for _ in range(200):
        Yn, Zn = (Y + mp.inverse(Z)) / 2, (Z + mp.inverse(Y)) / 2
        d = max(abs(Yn[i, j] - Y[i, j]) / (1 + abs(Y[i, j])) for i in range(M.rows) for j in range(M.cols))
        Y, Z = Yn, Zn
        if d < mp.mpf(10) ** -(mp.mp.dps - 4):
            return Y
    raise ArithmeticError("Denman-Beavers did not converge")


def logm_iss(M, rot):
    """principal matrix logarithm by inverse scaling and squaring: square roots until the leading rot x rot (rotation)
    block is within 0.03 of the identity, then the power series of log(I + X).  (mpmath.logm returns a non-principal
    branch for rotations beyond pi / 2 and is not used.)"""
    k = 0
    while max(abs(M[i, j] - (1 if i == j else 0)) for i in range(rot) for j in range(rot)) > mp.mpf(3) / 100:
        M = sqrtm_db(M)
        k += 1
        assert k < 40
    X = M - mp.eye(M.rows)
    L, term = mp.zeros(M.rows, M.cols), mp.eye(M.rows)
    for n in range(1, 400):
        term = term * X
        L = L + term * (mp.mpf((-1) ** (n + 1)) / n)
        if max(abs(term[i, j]) for i in range(rot) for j in range(rot)) < mp.mpf(10) ** -(mp.mp.dps + 4):
            break
    return L * (2 ** k)


class Group:
    def __init__(self, name, hat, vee, mat, elem, T, E, rot):
        self.name, self.hat, self.vee, self.mat, self.elem, self.T, self.E, self.rot = name, hat, vee, mat, elem, T, E, rot
        self.checked = -1   # every fourth dr_expinv is cross-checked against the central difference

    def exp_m(self, a):
        return mp.expm(self.hat([mp.mpf(v) for v in a]))

    def log_m(self, M, hint=None):
        if self.name == "SO3" and abs(M[0, 0] + M[1, 1] + M[2, 2] + 1) < mp.mpf(10) ** -50:  # rotation by exactly pi
            S = (M + mp.eye(3)) / 2                                                       # = axis axis'
            k = max(range(3), key=lambda i: S[i, i])
            ax = [S[i, k] / mp.sqrt(S[k, k]) for i in range(3)]
            if hint is not None and sum(a * mp.mpf(h) for a, h in zip(ax, hint)) < 0:
                ax = [-a for a in ax]
            v = [mp.pi * a for a in ax]
        else:
            v = self.vee(logm_iss(M, self.rot))
        assert mat_err(mp.expm(self.hat(v)), M) < mp.mpf(10) ** -40, "log does not invert exp"
        return v

    def ad(self, a):
        a = [mp.mpf(v) for v in a]
        A = self.hat(a)
        cols = []
        for i in range(self.T):
            E = self.hat([mp.mpf(1 if j == i else 0) for j in range(self.T)])
            cols.append(self.vee(A * E - E * A))
        return mp.matrix([[cols[c][r] for c in range(self.T)] for r in range(self.T)])

    def dr_expinv(self, a):
        self.checked += 1
        A = self.ad(a)
        J, term, n = mp.eye(self.T), mp.eye(self.T), 0
        while True:
            n += 1
            term = term * A / n                                   # ad^n / n!
            b = mp.mpf(1) / 2 if n == 1 else mp.bernoulli(n)      # B_1^+ = +1/2
            if b != 0:
                J = J + b * term
            big = max(abs(term[i, j]) for i in range(self.T) for j in range(self.T))
            ref = max(abs(J[i, j]) for i in range(self.T) for j in range(self.T))
            if n > 4 and big * 2 < ref * mp.mpf(10) ** -58:      # |B_n| <= 4 n! / (2 pi)^n: geometric for |theta| < 2 pi
                break
            assert n < 2000
        if CROSS_CHECK and self.checked % 4 == 0:
            h = mp.mpf(10) ** -15
            Ea = self.exp_m(a)
            for c in range(self.T):
                e = [h if j == c else 0 for j in range(self.T)]
                lp = self.log_m(Ea * self.exp_m(e))
                lm = self.log_m(Ea * self.exp_m([-v for v in e]))
                for r in range(self.T):
                    d = (lp[r] - lm[r]) / (2 * h)
                    assert abs(d - J[r, c]) < mp.mpf(10) ** -18 * (1 + abs(J[r, c])), (self.name, a, r, c, d, J[r, c])
        return J

    def inv_m(self, M):
        return mp.inverse(M)


SE2 = Group("SE2", se2_hat, se2_vee, se2_mat, se2_elem, 3, 4, 2)
SO3 = Group("SO3", so3_hat, so3_vee, so3_mat, so3_elem, 3, 4, 3)


def colmajor(M):
    return [M[r, c] for c in range(M.cols) for r in range(M.rows)]


# ---------------------------------------------------------------- inputs
def tangents(group, rng):
    """(class, tangent) for the angle classes of the issue; SE2: (vx, vy, omega), SO3: angle * unit axis"""
    out = []

    def unit():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v)

    def add(cls, theta, trans=1.5, scale=1.0):
        if group == "SE2":
            out.append((cls, np.array([scale * rng.uniform(-trans, trans), scale * rng.uniform(-trans, trans), theta])))
        else:
            out.append((cls, theta * unit()))
    for _ in range(40):
        add("random_1p5", rng.uniform(-1.5, 1.5))
    for _ in range(40):
        add("random_3", rng.uniform(-3, 3), trans=3.0)
    for k in range(25):
        for sgn in (1.0, -1.0):
            add("sweep", sgn * 10.0 ** (-k / 2.0))
    for k in range(4):
        if group == "SE2":
            add("theta0", 0.0)
        else:
            out.append(("theta0", np.zeros(3)))
    for k in range(1, 13):
        add("near_pi", PI - 10.0 ** (-k))
        if k % 3 == 0:
            add("near_pi", -(PI - 10.0 ** (-k)))
    if group == "SE2":
        for _ in range(8):
            add("trans_1e-6", rng.uniform(-3, 3), trans=1.0, scale=1e-6)
        for _ in range(8):
            add("trans_1e6", rng.uniform(-3, 3), trans=1.0, scale=1e6)
        add("trans_1e6", 1e-5, trans=1.0, scale=1e6)
        add("trans_1e6", 1.1e-4, trans=1.0, scale=1e6)
        add("trans_1e-6", 0.0, trans=1.0, scale=1e-6)
    return out


def elements(G, tans):
    """the float64 elements exp(a) of the tangents (the reference is evaluated at these doubles)"""
    return [(cls, np.array(f64(G.elem(G.exp_m(a))))) for cls, a in tans]


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def so3_special_elements(rng):
    """quaternions on the w < 0 branch of SO3::log (products of two large rotations, negated random ones) and rotations
    by exactly pi (w == 0)"""
    out = []
    while len(out) < 24:
        a, b = rng.normal(size=3), rng.normal(size=3)
        a, b = rng.uniform(2.0, 3.0) * a / np.linalg.norm(a), rng.uniform(2.0, 3.0) * b / np.linalg.norm(b)
        qa, qb = np.array(f64(SO3.elem(SO3.exp_m(a)))), np.array(f64(SO3.elem(SO3.exp_m(b))))
        q = quat_mul(qa, qb)
        if q[0] < -1e-3:
            out.append(("w_negative", q / np.linalg.norm(q), qa, qb))
    for k in range(8):
        a = rng.uniform(-3, 3) * (lambda v: v / np.linalg.norm(v))(rng.normal(size=3))
        q = -np.array(f64(SO3.elem(SO3.exp_m(a))))
        out.append(("w_negative", q, None, None))
    for ax in ([1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0], [0.6, 0.8, 0.0], [0.0, -0.6, 0.8], [2.0 / 3, -1.0 / 3, 2.0 / 3]):
        out.append(("pi_exact", np.array([0.0] + list(ax)), None, None))
    return out


# ---------------------------------------------------------------- operations on one item -> list of mp values
def op_eval(G, op, row):
    E, T = G.E, G.T
    if op == "exp":
        return G.elem(G.exp_m(row))
    if op == "log":
        return G.log_m(G.mat(row), hint=row[1:4])
    if op == "mul":
        return G.elem(G.mat(row[:E]) * G.mat(row[E:]))
    if op == "ad":
        return colmajor(G.ad(row))
    if op == "dr_expinv":
        return colmajor(G.dr_expinv(row))
    if op == "rplus":
        return G.elem(G.mat(row[:E]) * G.exp_m(row[E:]))
    if op == "rminus":
        return G.log_m(G.inv_m(G.mat(row[E:])) * G.mat(row[:E]))
    if op == "rminus_rplus":
        g = G.mat(row[:E])
        return G.log_m(G.inv_m(g) * (g * G.exp_m(row[E:])))
    raise KeyError(op)


# bundles: parts as (group or None for R^3)
BUNDLES = {"R3": [None], "X6": [SE2, None], "X12": [SE2, None, SE2, None]}


def bundle_eval(parts, op, row):
    """part by part; R^3 parts: rplus = +, rminus = -, ad = 0, dr_expinv = I"""
    Es, Ts = [(p.E if p else 3) for p in parts], [3] * len(parts)
    E, T = sum(Es), sum(Ts)
    if op in ("ad", "dr_expinv"):
        M = mp.zeros(T, T)
        for i, p in enumerate(parts):
            a = row[3 * i:3 * i + 3]
            blk = (p.ad(a) if op == "ad" else p.dr_expinv(a)) if p else (mp.zeros(3, 3) if op == "ad" else mp.eye(3))
            for r in range(3):
                for c in range(3):
                    M[3 * i + r, 3 * i + c] = blk[r, c]
        return colmajor(M)
    first, second = row[:E], row[E:]
    out, eo, to = [], 0, 0
    for i, p in enumerate(parts):
        g = first[eo:eo + Es[i]]
        other = second[to:to + 3] if op != "rminus" else second[eo:eo + Es[i]]
        if p:
            out += op_eval(p, op, np.concatenate([g, other]))
        elif op == "rplus":
            out += [mp.mpf(a) + mp.mpf(b) for a, b in zip(g, other)]
        elif op == "rminus":
            out += [mp.mpf(a) - mp.mpf(b) for a, b in zip(g, other)]
        else:  # rminus(rplus(g, b), g) with the float64 sum NOT rounded in between: b
            out += [mp.mpf(b) for b in other]
        eo += Es[i]
        to += 3
    return out


def build_inputs():
    """{(group, op): (class names, input rows)}; deterministic"""
    rng = np.random.default_rng(SEED)
    cases = {}
    for G in (SE2, SO3):
        tans = tangents(G.name, rng)
        elems = elements(G, tans)
        special = so3_special_elements(rng) if G is SO3 else []
        cases[G.name, "exp"] = tans
        cases[G.name, "ad"] = tans
        cases[G.name, "dr_expinv"] = tans
        cases[G.name, "log"] = elems + [(c, q) for c, q, _, _ in special]
        mul = [(c, np.concatenate([e, elems[i - 1][1]])) for i, (c, e) in enumerate(elems)]   # with its neighbour
        mul += [(c, np.concatenate([qa, qb])) for c, _, qa, qb in special if qa is not None]
        cases[G.name, "mul"] = mul
        # rplus / rminus / rminus_rplus: fresh tangents of every class, each applied to an element of ITS OWN class (the next
        # one, cyclically): log(g^-1 (g exp(b))) with |g| = 1e6 and |b| = 1 loses ten digits in any arithmetic, which
        # would say nothing about the code under test
        small = tangents(G.name, rng)

        def mate(i, shift):
            same = [j for j, (c, _) in enumerate(tans) if c == small[i][0]]
            return elems[same[(same.index(i) + shift) % len(same)]][1]
        cases[G.name, "rplus"] = [(c, np.concatenate([mate(i, 1), a])) for i, (c, a) in enumerate(small)]
        cases[G.name, "rminus_rplus"] = [(c, np.concatenate([mate(i, 2), a])) for i, (c, a) in enumerate(small)]
        rm = []
        for i, (c, a) in enumerate(small):
            g = mate(i, 3)
            rm.append((c, np.concatenate([np.array(f64(G.elem(G.mat(g) * G.exp_m(a)))), g])))
        cases[G.name, "rminus"] = rm
    # bundles: SE2 parts from the SE2 classes (a thinned set), R^3 parts random
    se2_t = cases["SE2", "exp"]
    se2_e = cases["SE2", "log"]
    for name, parts in BUNDLES.items():
        n = 8 if name == "R3" else 48
        idx = np.linspace(0, len(se2_t) - 1, n).astype(int)
        tan_rows, elem_rows, other_rows, cls = [], [], [], []
        for k in idx:
            same = [j for j, (c, _) in enumerate(se2_t) if c == se2_t[k][0]]
            t, e, o = [], [], []
            for pi_, p in enumerate(parts):                        # every SE2 part from the row's class
                kk = same[(same.index(k) + pi_) % len(same)]
                t.append(se2_t[kk][1] if p else rng.uniform(-2, 2, 3))
                e.append(se2_e[same[(same.index(kk) + 1) % len(same)]][1] if p else rng.uniform(-2, 2, 3))
                o.append(se2_e[same[(same.index(kk) + 2) % len(same)]][1] if p else rng.uniform(-2, 2, 3))
            tan_rows.append(np.concatenate(t)); elem_rows.append(np.concatenate(e)); other_rows.append(np.concatenate(o))
            cls.append(se2_t[k][0] if name != "R3" else "random_3")
        cases[name, "ad"] = list(zip(cls, tan_rows))
        cases[name, "dr_expinv"] = list(zip(cls, tan_rows))
        cases[name, "rplus"] = [(c, np.concatenate([e, t])) for c, e, t in zip(cls, elem_rows, tan_rows)]
        cases[name, "rminus_rplus"] = cases[name, "rplus"]
        cases[name, "rminus"] = [(c, np.concatenate([o, e])) for c, o, e in zip(cls, other_rows, elem_rows)]
    return cases


def evaluate(group, op, row):
    if group in ("SE2", "SO3"):
        return f64(op_eval(SE2 if group == "SE2" else SO3, op, row))
    return f64(bundle_eval(BUNDLES[group], op, row))


def sample(every=25):
    """{key: (row indices, regenerated out rows)} for every `every`-th row of every case (tests/test_lie_host.py)"""
    global CROSS_CHECK
    CROSS_CHECK = False
    out = {}
    for (group, op), rows in sorted(build_inputs().items()):
        idx = list(range(0, len(rows), every))
        out["%s.%s" % (group, op)] = (idx, np.array([rows[i][1] for i in idx]), np.array([evaluate(group, op, rows[i][1]) for i in idx]))
    return out


def main():
    out = {"classes": np.array(CLASSES)}
    for (group, op), rows in sorted(build_inputs().items()):
        key = "%s.%s" % (group, op)
        out[key + ".in"] = np.array([r for _, r in rows])
        out[key + ".cls"] = np.array([CLASSES.index(c) for c, _ in rows], dtype=np.int8)
        out[key + ".out"] = np.array([evaluate(group, op, r) for _, r in rows])
        print(key, out[key + ".in"].shape, out[key + ".out"].shape, flush=True)
    path = os.path.join(HERE, "lie_reference.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
