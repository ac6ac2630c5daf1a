"""Plain float64 transcription of the textbook closed forms of the SE(3) operations (pose = translation + unit quaternion,
tangent (v, omega)) and of SE(3) x R^6, written without reference to include/smooth_feedback_amd/lie.hpp, with the
comparison helpers of tests/test_lie_se3_host.py / test_lie_se3_gpu.py.  Same role and same rule as tests/lie_ref.py (whose
helpers it imports): its error against the 60-digit values of tests/golden/lie_se3_reference.npz is what float64 can be
expected to deliver; four times that error is the gate for lie.hpp.

Textbook forms (W = hat(omega), t = |omega|^2):
  exp        p = V v,  V = I + B W + C W^2,  B = (1 - cos th)/th^2,  C = (th - sin th)/th^3;  q = so3 exp
  log        omega = so3 log,  v = V^-1 p = (I - W/2 + k W^2) p
  product    (p + R(q) p', q q'),  R(q) the rotation matrix of the quaternion
  ad         [[W, hat(v)], [0, W]]
  dr_expinv  in powers of ad, through its minimal polynomial  ad (ad^2 + t)^2 = 0:
             sum_n B_n^+ ad^n / n! = I + ad/2 + a ad^2 + b ad^4,  a = k - t k',  b = -k'   (k' = dk/dt)
             (the even part of x / (1 - e^-x), interpolated with its derivative at the double eigenvalues +-i th)
Series next to the removable singularities, switched where truncation meets cancellation (eps = 1.1e-16):
  B          = sinc(th/2)^2 / 2: no cancellation, lie_ref._sinc bridges 0/0
  C          closed: 6 eps / t relative; seven terms: 1.7e-14 t^7 relative             -> t < 0.6
  k          lie_ref._k
  k'         closed (-1/t^2 + (1 + c^2)/(8 t) + c/(4 t th), c = cot(th/2)): 3 eps / t^2; twelve terms: 1.2e-21 t^12 -> t < 2"""
import math

import numpy as np

from lie_ref import OPS, _bernoulli, _hat3, _k, _sinc, per_class, so3_exp, so3_log, so3_mul  # noqa: F401

GROUP_PARTS = {"SE3": ("SE3",), "X12B": ("SE3", "R6")}
ELEM = {"SE3": 7, "R6": 6}
_DK_COEF = [float((n - 1) * abs(b) / math.factorial(2 * n)) for n, b in enumerate(_bernoulli(26)[::2]) if n >= 2]   # t^0 .. t^11


def _C(t):
    if t < 0.6:
        acc = 1.0 / math.factorial(15)          # Horner, alternating signs: 1/3! - t/5! + ... + t^6/15!
        for n in range(5, -1, -1):
            acc = 1.0 / math.factorial(2 * n + 3) - t * acc
        return acc
    th = math.sqrt(t)
    return (th - math.sin(th)) / (t * th)


def _dk(t):
    if t < 2.0:
        acc = 0.0
        for c in reversed(_DK_COEF):
            acc = acc * t + c
        return acc
    th = math.sqrt(t)
    c = 1.0 / math.tan(0.5 * th)
    return -1.0 / (t * t) + (1.0 + c * c) / (8.0 * t) + c / (4.0 * t * th)


def _rot(q):
    w, x, y, z = q
    n = w * w + x * x + y * y + z * z
    s = 2.0 / n
    return np.array([[1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
                     [s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)],
                     [s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)]])


def se3_exp(a):
    v, w = np.array(a[:3]), np.array(a[3:6])
    t = float(w @ w)
    W = _hat3(w)
    V = np.eye(3) + 0.5 * _sinc(0.5 * math.sqrt(t)) ** 2 * W + _C(t) * (W @ W)
    return list(V @ v) + so3_exp(list(w))


def se3_log(g):
    w = np.array(so3_log(list(g[3:7])))
    W = _hat3(w)
    Vi = np.eye(3) - 0.5 * W + _k(float(w @ w)) * (W @ W)
    return list(Vi @ np.array(g[:3])) + list(w)


def se3_mul(g, h):
    return list(np.array(g[:3]) + _rot(g[3:7]) @ np.array(h[:3])) + so3_mul(list(g[3:7]), list(h[3:7]))


def se3_inv(g):
    qi = [g[3], -g[4], -g[5], -g[6]]
    return list(-(_rot(qi) @ np.array(g[:3]))) + qi


def se3_ad(a):
    M = np.zeros((6, 6))
    M[:3, :3] = M[3:, 3:] = _hat3(a[3:6])
    M[:3, 3:] = _hat3(a[:3])
    return M


def se3_dr_expinv(a):
    t = float(np.dot(a[3:6], a[3:6]))
    A = se3_ad(a)
    A2 = A @ A
    dk = _dk(t)
    return np.eye(6) + 0.5 * A + (_k(t) - t * dk) * A2 - dk * (A2 @ A2)


def _se3(op, row):
    row = [float(v) for v in row]
    E = 7
    if op == "exp":
        return se3_exp(row)
    if op == "log":
        return se3_log(row)
    if op == "mul":
        return se3_mul(row[:E], row[E:])
    if op == "ad":
        return se3_ad(row)
    if op == "dr_expinv":
        return se3_dr_expinv(row)
    if op == "rplus":
        return se3_mul(row[:E], se3_exp(row[E:]))
    if op == "rminus":
        return se3_log(se3_mul(se3_inv(row[E:]), row[:E]))
    if op == "rminus_rplus":
        g = row[:E]
        return se3_log(se3_mul(se3_inv(g), se3_mul(g, se3_exp(row[E:]))))
    raise KeyError(op)


def widths(group, op):
    """(doubles in, doubles out) per item, or None when the group has no such operation"""
    E, T = (7, 6) if group == "SE3" else (13, 12)
    if op in ("exp", "log", "mul") and group != "SE3":
        return None
    return {"exp": (T, E), "log": (E, T), "mul": (2 * E, E), "ad": (T, T * T), "dr_expinv": (T, T * T), "rplus": (E + T, E),
            "rminus": (2 * E, T), "rminus_rplus": (E + T, T)}[op]


def transcription(group, op, inp):
    """the operation on every row of inp [count][win] -> [count][wout], laid out as examples/lie_eval.h lays it out"""
    out = []
    for row in np.asarray(inp, dtype=np.float64):
        if group == "SE3":
            r = _se3(op, row)
            out.append(r.T.reshape(-1) if op in ("ad", "dr_expinv") else np.array(r))
        elif op in ("ad", "dr_expinv"):
            M = np.zeros((12, 12))
            M[:6, :6] = _se3(op, row[:6])
            if op == "dr_expinv":
                M[6:, 6:] = np.eye(6)
            out.append(M.T.reshape(-1))
        else:
            first, second = row[:13], row[13:]
            if op == "rminus":
                res = _se3(op, np.concatenate([first[:7], second[:7]])) + [float(x) - float(y) for x, y in zip(first[7:], second[7:])]
            else:
                res = _se3(op, np.concatenate([first[:7], second[:6]]))
                x, y = [float(v) for v in first[7:]], [float(v) for v in second[6:]]
                res = res + ([p + q for p, q in zip(x, y)] if op == "rplus" else [(p + q) - p for p, q in zip(x, y)])
            out.append(np.array(res))
    return np.array(out)


def _blocks(group, op):
    """The output entries of (group, op) grouped by the quantity they belong to, each with ONE scale (the rule of
    lie_ref._blocks): the translation of a pose or tangent -- and the block of ad / dr_expinv that carries v -- apart from the
    rotation entries, the R^6 part of the bundle apart from the pose."""
    bundle = group == "X12B"
    T = 12 if bundle else 6
    kind = {"exp": "elem", "mul": "elem", "rplus": "elem", "log": "tan", "rminus": "tan", "rminus_rplus": "tan",
            "ad": "mat", "dr_expinv": "mat"}[op]
    if kind == "mat":
        at = lambda rows, cols: [r + c * T for c in cols for r in rows]
        blocks = [at(range(0, 3), range(3, 6)),                                               # carries v
                  at(range(0, 3), range(0, 3)) + at(range(3, 6), range(0, 6))]                # rotation blocks (and the zero block)
        if bundle:
            blocks += [at(range(6, 12), range(6, 12)), at(range(0, 6), range(6, 12)) + at(range(6, 12), range(0, 6))]
        return blocks
    blocks = [[0, 1, 2], list(range(3, 7 if kind == "elem" else 6))]
    if bundle:
        n = 7 if kind == "elem" else 6
        blocks.append(list(range(n, n + 6)))
    return blocks


def scaled_error(group, op, got, ref):
    """per row: max over the blocks of _blocks() of  max|got - ref| / (1 + max|ref|).  A pose is compared up to the sign of
    its quaternion (q and -q are the same rotation; the fixture holds the one with w >= 0)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)

    def one(g):
        return np.max([np.max(np.abs(g[:, b] - ref[:, b]), axis=1) / (1.0 + np.max(np.abs(ref[:, b]), axis=1)) for b in _blocks(group, op)],
                      axis=0)
    err = one(got)
    if op in ("exp", "mul", "rplus"):
        flipped = got.copy()
        flipped[:, 3:7] *= -1.0
        err = np.minimum(err, one(flipped))
    return np.where(np.all(np.isfinite(got), axis=1), err, np.inf)
