"""Generates tests/golden/lie_se3_reference.npz: inputs and float64-rounded results of the SE(3) operations of
include/smooth_feedback_amd/lie.hpp (SE3, Bundle<SE3, Rn<6>> = X12B), computed with mpmath at 60 digits FROM THE 4x4
HOMOGENEOUS MATRIX GROUP, not from closed forms, with the machinery of make_golden_lie.py (imported, not copied):

  exp / log      mpmath.expm / the checked matrix logarithm (inverse scaling and squaring + power series) of the 4x4 matrix;
                 every log is checked by expm(hat(log)) == matrix.  A rotation by exactly pi has no principal logarithm:
                 omega = pi * axis with the axis of (R + I) / 2 and the sign of the quaternion's own vector part, and v from
                 the linear system  (int_0^1 expm(s hat(omega)) ds) v = p  in its exact form at pi
                 (I + 2 hat(omega) / pi^2 + hat(omega)^2 / pi^2), checked by the same expm(hat(log)) == matrix
  product        matrix product
  ad             columns vee([hat(a), hat(e_i)]), 6 x 6
  dr_expinv      Bernoulli series  sum_n B_n^+ ad(a)^n / n!, cross-checked against the central difference of
                 h -> log(exp(a) exp(h)) with step 1e-15 at 60 digits (every fourth input)
  rplus, rminus  g expm(hat(a)),  log(b^-1 a);  the bundle part by part

Elements are stored as lie.hpp stores them: SE3 (px, py, pz, w, x, y, z), X12B that followed by the six doubles of R^6.
Tangents (v0, v1, v2, w0, w1, w2).  A quaternion given as doubles is not exactly of unit length: the reference takes the
rotation it normalises to, and stores the quaternion with w >= 0; the tests compare up to that sign.

Input classes as in make_golden_lie.py, one name per row.  The sweep holds the rotation angles 10^(-k/2), k = 0..24, and
0.1 j, j = 1..31: every switch between a series and a closed form that lies in (0, 3.1) is crossed, wherever it is.
Run by hand from the repository root (several minutes):  python tests/golden/make_golden_lie_se3.py
tests/test_lie_se3_host.py regenerates a sample through sample() when mpmath is importable."""
import importlib.util
import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_lie", os.path.join(HERE, "make_golden_lie.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

mp.mp.dps = 60
SEED = 20261017
CLASSES = B.CLASSES
PI = B.PI
f64 = B.f64


# ---------------------------------------------------------------- matrix forms
def se3_hat(a):
    v, w = a[:3], a[3:6]
    return mp.matrix([[0, -w[2], w[1], v[0]], [w[2], 0, -w[0], v[1]], [-w[1], w[0], 0, v[2]], [0, 0, 0, 0]])


def se3_vee(M):
    return [M[0, 3], M[1, 3], M[2, 3], M[2, 1], M[0, 2], M[1, 0]]


def se3_mat(e):
    R = B.so3_mat(e[3:7])
    M = mp.eye(4)
    for i in range(3):
        for j in range(3):
            M[i, j] = R[i, j]
        M[i, 3] = mp.mpf(e[i])
    return M


def se3_elem(M):
    R = mp.matrix([[M[i, j] for j in range(3)] for i in range(3)])
    return [M[0, 3], M[1, 3], M[2, 3]] + B.so3_elem(R)


class SE3Group(B.Group):
    def log_m(self, M, hint=None):
        if abs(M[0, 0] + M[1, 1] + M[2, 2] + 1) < mp.mpf(10) ** -50:      # rotation by exactly pi
            R = mp.matrix([[M[i, j] for j in range(3)] for i in range(3)])
            w = B.SO3.log_m(R, hint=hint)
            W = B.so3_hat(w)
            V = mp.eye(3) + W * (2 / mp.pi ** 2) + W * W / mp.pi ** 2
            v = mp.lu_solve(V, mp.matrix([M[0, 3], M[1, 3], M[2, 3]]))
            out = [v[0], v[1], v[2]] + list(w)
        else:
            out = self.vee(B.logm_iss(M, self.rot))
        scale = 1 + max(abs(M[i, 3]) for i in range(3))
        assert B.mat_err(mp.expm(self.hat(out)), M) < mp.mpf(10) ** -40 * scale, "log does not invert exp"
        return out


SE3 = SE3Group("SE3", se3_hat, se3_vee, se3_mat, se3_elem, 6, 7, 3)


# ---------------------------------------------------------------- inputs
def tangents(rng):
    """(class, tangent (v, omega)) for the angle and translation classes"""
    out = []

    def unit():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v)

    def add(cls, theta, trans=1.5, scale=1.0):
        out.append((cls, np.concatenate([scale * rng.uniform(-trans, trans, 3), theta * unit()])))
    for _ in range(24):
        add("random_1p5", rng.uniform(-1.5, 1.5))
    for _ in range(24):
        add("random_3", rng.uniform(-3, 3), trans=3.0)
    for k in range(25):
        add("sweep", 10.0 ** (-k / 2.0))
    for j in range(1, 32):
        add("sweep", 0.1 * j)
    for k in range(3):
        out.append(("theta0", np.concatenate([rng.uniform(-1.5, 1.5, 3), np.zeros(3)])))
    for k in range(1, 13):
        add("near_pi", PI - 10.0 ** (-k))
        if k % 3 == 0:
            add("near_pi", -(PI - 10.0 ** (-k)))
    for _ in range(6):
        add("trans_1e-6", rng.uniform(-3, 3), trans=1.0, scale=1e-6)
    for _ in range(6):
        add("trans_1e6", rng.uniform(-3, 3), trans=1.0, scale=1e6)
    add("trans_1e6", 1e-5, trans=1.0, scale=1e6)
    add("trans_1e6", 1.1e-4, trans=1.0, scale=1e6)
    add("trans_1e-6", 0.0, trans=1.0, scale=1e-6)
    return out


def elements(tans):
    return [(cls, np.array(f64(SE3.elem(SE3.exp_m(a))))) for cls, a in tans]


def special_elements(rng):
    """poses whose quaternion is on the w < 0 branch of the logarithm, and rotations by exactly pi (w == 0); with the two
    factors where the element is a product"""
    out = []
    for cls, q, qa, qb in B.so3_special_elements(rng):
        p = rng.uniform(-1.5, 1.5, 3)
        if qa is None:
            out.append((cls, np.concatenate([p, q]), None, None))
        else:
            ga, gb = np.concatenate([rng.uniform(-1.5, 1.5, 3), qa]), np.concatenate([rng.uniform(-1.5, 1.5, 3), qb])
            g = np.array(f64(SE3.elem(SE3.mat(ga) * SE3.mat(gb))))
            g[3:] = q                              # the w < 0 representative the float64 quaternion product gives
            out.append((cls, g, ga, gb))
    return out[::2] + [s for s in out[1::2] if s[0] == "pi_exact"]


def op_eval(op, row):
    G, E = SE3, 7
    if op == "log":
        return G.log_m(G.mat(row), hint=row[4:7])
    if op == "exp":
        return G.elem(G.exp_m(row))
    if op == "mul":
        return G.elem(G.mat(row[:E]) * G.mat(row[E:]))
    return B.op_eval(G, op, row)


def bundle_eval(op, row):
    """X12B = SE3 x R^6; R^6: rplus = +, rminus = -, ad = 0, dr_expinv = I"""
    if op in ("ad", "dr_expinv"):
        M = mp.zeros(12, 12)
        blk = SE3.ad(row[:6]) if op == "ad" else SE3.dr_expinv(row[:6])
        for r in range(6):
            for c in range(6):
                M[r, c] = blk[r, c]
            if op == "dr_expinv":
                M[6 + r, 6 + r] = 1
        return B.colmajor(M)
    first, second = row[:13], row[13:]
    if op == "rminus":
        return op_eval(op, np.concatenate([first[:7], second[:7]])) + [mp.mpf(a) - mp.mpf(b) for a, b in zip(first[7:], second[7:])]
    out = op_eval(op, np.concatenate([first[:7], second[:6]]))
    if op == "rplus":
        return out + [mp.mpf(a) + mp.mpf(b) for a, b in zip(first[7:], second[6:])]
    return out + [mp.mpf(b) for b in second[6:]]    # rminus(rplus(g, b), g) with the sum not rounded in between: b


def build_inputs():
    """{(group, op): [(class name, input row)]}; deterministic"""
    rng = np.random.default_rng(SEED)
    cases = {}
    tans = tangents(rng)
    elems = elements(tans)
    special = special_elements(rng)
    cases["SE3", "exp"] = tans
    cases["SE3", "ad"] = tans
    cases["SE3", "dr_expinv"] = tans
    cases["SE3", "log"] = elems + [(c, g) for c, g, _, _ in special]
    mul = [(c, np.concatenate([e, elems[i - 1][1]])) for i, (c, e) in enumerate(elems)]
    mul += [(c, np.concatenate([ga, gb])) for c, _, ga, gb in special if ga is not None]
    cases["SE3", "mul"] = mul
    small = tangents(rng)      # fresh tangents, each applied to an element of its own class (make_golden_lie.py)

    def mate(i, shift):
        same = [j for j, (c, _) in enumerate(tans) if c == small[i][0]]
        return elems[same[(same.index(i) + shift) % len(same)]][1]
    cases["SE3", "rplus"] = [(c, np.concatenate([mate(i, 1), a])) for i, (c, a) in enumerate(small)]
    cases["SE3", "rminus_rplus"] = [(c, np.concatenate([mate(i, 2), a])) for i, (c, a) in enumerate(small)]
    rm = []
    for i, (c, a) in enumerate(small):
        g = mate(i, 3)
        rm.append((c, np.concatenate([np.array(f64(SE3.elem(SE3.mat(g) * SE3.exp_m(a)))), g])))
    rm += [(c, np.concatenate([g, elems[k][1]])) for k, (c, g, _, _) in enumerate(special)]   # w < 0 and pi against a random pose
    cases["SE3", "rminus"] = rm
    # the bundle: the SE3 part from a thinned set of the SE3 rows, the R^6 part random
    idx = np.linspace(0, len(tans) - 1, 40).astype(int)
    r6 = lambda: rng.uniform(-2, 2, 6)
    cases["X12B", "ad"] = [(tans[k][0], np.concatenate([tans[k][1], r6()])) for k in idx]
    cases["X12B", "dr_expinv"] = cases["X12B", "ad"]
    cases["X12B", "rplus"] = [(c, np.concatenate([row[:7], r6(), row[7:], r6()])) for c, row in (cases["SE3", "rplus"][k] for k in idx)]
    cases["X12B", "rminus_rplus"] = cases["X12B", "rplus"]
    cases["X12B", "rminus"] = [(c, np.concatenate([row[:7], r6(), row[7:], r6()])) for c, row in (cases["SE3", "rminus"][k] for k in idx)]
    return cases


def evaluate(group, op, row):
    return f64(op_eval(op, row) if group == "SE3" else bundle_eval(op, row))


def sample(every=25):
    """{key: (row indices, input rows, regenerated out rows)} for every `every`-th row of every case"""
    B.CROSS_CHECK = False
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
    path = os.path.join(HERE, "lie_se3_reference.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
