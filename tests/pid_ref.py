"""Plain float64 numpy restatement of the Lie-group PID law and of its closed-loop rollout, in MATRIX form: a pose is its
homogeneous matrix (SE2 3x3, SO3 3x3, SE3 4x4), rplus(g, a) = g @ exp(hat(a)), rminus(a, b) = vee(log(inv(b) @ a)), with exp
and log by the textbook formulas on matrices (Rodrigues; angle and axis from R - R' and the trace; the translation through
the linear system V v = p).  It shares nothing with include/smooth_feedback_amd (which works on quaternions and
(cos, sin) pairs) nor with tests/lie_ref*.py.  What it delivers against the 60-digit fixture tests/golden/pid_reference.npz
(make_golden_pid.py) is what float64 delivers on these inputs: the gates of tests/test_pid_*.py are four times that.

Element storage as the C-ABI: RN N values, SE2 (x, y, cos, sin), SO3 (w, x, y, z), SE3 (px, py, pz, w, x, y, z)."""
import numpy as np

ELEM = {"SE2": 4, "SO3": 4, "SE3": 7}
GROUPS = {"R2": [("RN", 2)], "SE2": [("SE2", 3)], "SO3": [("SO3", 3)], "SE3": [("SE3", 6)], "SE3R3": [("SE3", 6), ("RN", 3)],
          "SE2R1": [("SE2", 3), ("RN", 1)]}


def widths(parts):
    """doubles per element, per tangent"""
    return sum(d if k == "RN" else ELEM[k] for k, d in parts), sum(d for _, d in parts)


# ---------------------------------------------------------------- matrices
def _hat3(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _rot_of_quat(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _quat_of_rot(R):
    t = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], -R[0, 0] + R[1, 1] - R[2, 2], -R[0, 0] - R[1, 1] + R[2, 2]]
    k = int(np.argmax(t))
    r = 2.0 * np.sqrt(1.0 + t[k])
    if k == 0:
        q = [r / 4, (R[2, 1] - R[1, 2]) / r, (R[0, 2] - R[2, 0]) / r, (R[1, 0] - R[0, 1]) / r]
    elif k == 1:
        q = [(R[2, 1] - R[1, 2]) / r, r / 4, (R[0, 1] + R[1, 0]) / r, (R[0, 2] + R[2, 0]) / r]
    elif k == 2:
        q = [(R[0, 2] - R[2, 0]) / r, (R[0, 1] + R[1, 0]) / r, r / 4, (R[1, 2] + R[2, 1]) / r]
    else:
        q = [(R[1, 0] - R[0, 1]) / r, (R[0, 2] + R[2, 0]) / r, (R[1, 2] + R[2, 1]) / r, r / 4]
    q = np.array(q)
    q /= np.linalg.norm(q)
    return -q if q[0] < 0 else q


def _coefs(th):
    """sin th / th,  (1 - cos th) / th^2,  (th - sin th) / th^3"""
    t2 = th * th
    if abs(th) < 1e-4:
        return 1 - t2 / 6, 0.5 - t2 / 24, 1.0 / 6 - t2 / 120
    h = np.sin(0.5 * th) / (0.5 * th)
    if abs(th) > 0.3:
        c = (th - np.sin(th)) / th ** 3
    else:       # the difference cancels: its series, whose next term is below 1e-17 here
        c = 1.0 / 6 - t2 / 120 + t2 ** 2 / 5040 - t2 ** 3 / 362880 + t2 ** 4 / 39916800 - t2 ** 5 / 6227020800
    return np.sin(th) / th, 0.5 * h * h, c


def _rot_exp(W, th):
    """exp of a skew matrix W (2x2 or 3x3) of angle th, and V = int_0^1 exp(s W) ds"""
    A, B, Cc = _coefs(th)
    I, W2 = np.eye(len(W)), W @ W
    return I + A * W + B * W2, I + B * W + Cc * W2


def part_mat(kind, e):
    if kind == "SE2":
        c, s = np.array(e[2:4]) / np.hypot(e[2], e[3])
        return np.array([[c, -s, e[0]], [s, c, e[1]], [0.0, 0.0, 1.0]])
    if kind == "SO3":
        return _rot_of_quat(e)
    M = np.eye(4)
    M[:3, :3] = _rot_of_quat(e[3:7])
    M[:3, 3] = e[:3]
    return M


def part_elem(kind, M):
    if kind == "SE2":
        return np.array([M[0, 2], M[1, 2], M[0, 0], M[1, 0]])
    if kind == "SO3":
        return _quat_of_rot(M)
    return np.concatenate([M[:3, 3], _quat_of_rot(M[:3, :3])])


def part_exp(kind, a):
    a = np.asarray(a, dtype=np.float64)
    if kind == "SE2":
        R, V = _rot_exp(np.array([[0.0, -a[2]], [a[2], 0.0]]), a[2])
        M = np.eye(3)
        M[:2, :2], M[:2, 2] = R, V @ a[:2]
        return M
    if kind == "SO3":
        return _rot_exp(_hat3(a), np.linalg.norm(a))[0]
    R, V = _rot_exp(_hat3(a[3:]), np.linalg.norm(a[3:]))
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, V @ a[:3]
    return M


def _rot_log3(R):
    r = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])   # sin(th) * axis
    s = np.linalg.norm(r)
    th = np.arctan2(s, 0.5 * (np.trace(R) - 1.0))
    return r * (th / s if s > 1e-4 else 1.0 + s * s / 6.0 + 3.0 * s ** 4 / 40.0)


def part_log(kind, M):
    if kind == "SE2":
        th = np.arctan2(M[1, 0], M[0, 0])
        V = _rot_exp(np.array([[0.0, -th], [th, 0.0]]), th)[1]
        return np.concatenate([np.linalg.solve(V, M[:2, 2]), [th]])
    if kind == "SO3":
        return _rot_log3(M)
    w = _rot_log3(M[:3, :3])
    V = _rot_exp(_hat3(w), np.linalg.norm(w))[1]
    return np.concatenate([np.linalg.solve(V, M[:3, 3]), w])


def part_inv(kind, M):
    if kind == "SO3":
        return M.T
    d = len(M) - 1
    out = np.eye(d + 1)
    out[:d, :d] = M[:d, :d].T
    out[:d, d] = -M[:d, :d].T @ M[:d, d]
    return out


# ---------------------------------------------------------------- bundles: a state is a list of matrices / vectors
def load(parts, row):
    out, o = [], 0
    for k, d in parts:
        w = d if k == "RN" else ELEM[k]
        out.append(np.array(row[o:o + w], dtype=np.float64) if k == "RN" else part_mat(k, row[o:o + w]))
        o += w
    return out


def store(parts, g):
    return np.concatenate([gi if k == "RN" else part_elem(k, gi) for (k, _), gi in zip(parts, g)])


def rplus(parts, g, a):
    out, o = [], 0
    for (k, d), gi in zip(parts, g):
        out.append(gi + a[o:o + d] if k == "RN" else gi @ part_exp(k, a[o:o + d]))
        o += d
    return out


def rminus(parts, a, b):
    return np.concatenate([ai - bi if k == "RN" else part_log(k, part_inv(k, bi) @ ai) for (k, _), ai, bi in zip(parts, a, b)])


def matrix_rows(parts, X):
    """elements [B][elem] -> [B][entries of the parts' matrices]: the form in which elements are compared"""
    return np.array([np.concatenate([np.ravel(gi) for gi in load(parts, row)]) for row in np.atleast_2d(X)])


# ---------------------------------------------------------------- the law and the rollout
def law_row(parts, t, x, v, gd, vd, ad, kp, kd, ki, windup, t_last, ie):
    e = rminus(parts, gd, x)
    if t_last == t_last and t > t_last:
        ie = np.clip(ie + (t - t_last) * e, -windup, windup)
    return ad + kp * e + kd * (vd - v) + ki * ie, ie, e


def law(parts, t, x, v, gd, vd, ad, kp, kd, ki, windup, t_last, ie):
    """batched on flat arrays: -> u, i_err"""
    out = [law_row(parts, t, load(parts, x[b]), v[b], load(parts, gd[b]), vd[b], ad[b], kp[b], kd[b], ki[b], windup, t_last[b], ie[b])[:2]
           for b in range(len(x))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def integrate_row(parts, x, v, u, dt):
    return rplus(parts, x, dt * v + 0.5 * dt * dt * u), v + dt * u


def integrate(parts, x, v, u, dt):
    """the double-integrator step on flat arrays: -> x, v"""
    out = [integrate_row(parts, load(parts, x[b]), v[b], u[b], dt) for b in range(len(x))]
    return np.array([store(parts, o[0]) for o in out]), np.array([o[1] for o in out])


def traj(parts, kind, g0, w, t):
    if kind == 0:
        return rplus(parts, g0, t * w), w, np.zeros_like(w)
    return rplus(parts, g0, (t + 0.15 * t * t) * w), (1 + 0.3 * t) * w, 0.3 * w


def rollout(parts, kind, t0, dt, steps, x, v, g0, w, kp, kd, ki, windup, umax, t_last, ie):
    """batched on flat arrays; kind [B] selects the trajectory family per row.  -> dict x (matrix rows), v, ie, u, cost"""
    res = dict(x=[], v=[], ie=[], u=[], cost=[])
    for b in range(len(x)):
        xb, vb, ieb, tl, gb = load(parts, x[b]), np.array(v[b]), np.array(ie[b]), t_last[b], load(parts, g0[b])
        cost, u = 0.0, np.zeros_like(vb)
        for k in range(steps):
            t = t0 + k * dt
            gd, vd, ad = traj(parts, int(kind[b]), gb, w[b], t)
            u, ieb, e = law_row(parts, t, xb, vb, gd, vd, ad, kp[b], kd[b], ki[b], windup, tl, ieb)
            tl = t
            if umax is not None:
                u = np.clip(u, -umax, umax)
            xb, vb = integrate_row(parts, xb, vb, u, dt)
            cost += dt * float(e @ e)
        res["x"].append(np.concatenate([np.ravel(gi) for gi in xb])); res["v"].append(vb); res["ie"].append(ieb); res["u"].append(u)
        res["cost"].append(cost)
    return {k: np.array(val) for k, val in res.items()}


# ---------------------------------------------------------------- errors
def scaled_error(got, ref):
    """per row: max |got - ref| / (1 + max |ref|)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    got, ref = got.reshape(len(ref), -1), ref.reshape(len(ref), -1)
    return np.max(np.abs(got - ref), axis=1) / (1.0 + np.max(np.abs(ref), axis=1))


def per_class(err, cls, names):
    return {str(names[c]): float(err[cls == c].max()) for c in np.unique(cls)}
