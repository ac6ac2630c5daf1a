"""Generates tests/golden/pid_reference.npz: inputs and float64-rounded results of the Lie-group PID law
(include/smooth_feedback_amd/pid.hpp: pid_law, the PID<T, G> front), of the closed-loop rollout on the double integrator
(pid_rollout, sfb_pid_rollout_batch) and of the device swarm front's two trajectory families, computed with mpmath at 60
digits IN MATRIX FORM: a pose is its homogeneous matrix (SE2 3x3, SO3 3x3, SE3 4x4), exp is the power series of the matrix
exponential (scaling and squaring around it), log is the matrix logarithm (mpmath.logm, every result checked by
exp(log) == matrix), rplus(g, a) = g exp(hat(a)), rminus(a, b) = vee(log(b^-1 a)).  Nothing here goes through lie.hpp,
tests/lie_ref*.py or the closed forms of any group.  R^n parts are plain vectors; a bundle is evaluated part by part.

  law      g_err = g_des (-) x;  if t_last is set and t > t_last: i_err += (t - t_last) g_err, clamped to +-windup_limit;
           t_last = t;  u = a_des + kp o g_err + kd o (v_des - v) + ki o i_err                  (reference pid.hpp:74-87)
  tick k   t_k = t0 + k dt;  (g_des, v_des, a_des) = traj(t_k);  u = law;  u = clamp(u, +-u_max) if given;
           x <- x exp(hat(dt v + dt^2/2 u)),  v <- v + dt u;  cost += dt |g_err|^2
  traj     kind 0: g_des = g0 exp(hat(t w)), v_des = w, a_des = 0
           kind 1: g_des = g0 exp(hat(S(t) w)), v_des = s(t) w, a_des = s'(t) w,  s = 1 + 0.3 t,  S = t + 0.15 t^2

Element storage as lie.hpp / the C-ABI: RN N values, SE2 (x, y, cos, sin), SO3 (w, x, y, z), SE3 (px, py, pz, w, x, y, z);
quaternions and (cos, sin) given as doubles are normalised; quaternions are stored with w >= 0.

Groups: R2, SE2, SO3, SE3, SE3R3 = (SE3, R3), SE2R1 = (SE2, R1).  Case classes by the rotation angle of g_des (-) x at the
(first) call: "tiny" |th| <= 1e-9, "generic" |th| <= 1.5, "large" 2 <= |th| <= 3.  Sections of the fixture:
  step.<G>.*     one call at t = 1 with t_last unset (NaN), earlier (5 rows of 8), equal or later by row; results for windup_limit 0.5 and +inf
  seq.<G>.*      four calls of one controller at t = 0.1, 0.4, 0.4, 0.3 (unset, later, equal, earlier), windup_limit 0.5
  roll.<G>.*     rollouts from t0 = 0.25, dt = 0.05: A = 1 tick, B = 40 ticks, C = 40 ticks with the input clamp u_max
  swarm.SE3.*    40 ticks; rows with kind 0 track trajectory family 0, rows with kind 1 family 1
Run by hand from the repository root (a few minutes on 8 cores):  python tests/golden/make_golden_pid.py
tests/test_pid_host.py regenerates a sample through sample() when mpmath is importable."""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261018
CLASSES = ["tiny", "generic", "large"]
GROUPS = {"R2": [("RN", 2)], "SE2": [("SE2", 3)], "SO3": [("SO3", 3)], "SE3": [("SE3", 6)], "SE3R3": [("SE3", 6), ("RN", 3)],
          "SE2R1": [("SE2", 3), ("RN", 1)]}
ELEM = {"SE2": 4, "SO3": 4, "SE3": 7}
WINDUP = 0.5
T_STEP, T_LAST_KINDS = 1.0, [float("nan"), 0.7, 1.0, 0.4, 1.3, 0.7, 0.2, 0.5]     # unset, earlier, equal, later than t
SEQ_TIMES = [0.1, 0.4, 0.4, 0.3]
T0, DT = 0.25, 0.05
ROLL_SETS = {"A": (1, False), "B": (40, False), "C": (40, True)}
N_STEP, N_SEQ, N_ROLL, N_SWARM = 8, 4, 3, 4      # rows per (group, class)


def f64(xs):
    return [float(x) for x in xs]


# ---------------------------------------------------------------- matrix forms
def hat(kind, a):
    a = [mp.mpf(x) for x in a]
    if kind == "SE2":
        return mp.matrix([[0, -a[2], a[0]], [a[2], 0, a[1]], [0, 0, 0]])
    if kind == "SO3":
        return mp.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return mp.matrix([[0, -a[5], a[4], a[0]], [a[5], 0, -a[3], a[1]], [-a[4], a[3], 0, a[2]], [0, 0, 0, 0]])


def vee(kind, M):
    if kind == "SE2":
        return [M[0, 2], M[1, 2], M[1, 0]]
    if kind == "SO3":
        return [M[2, 1], M[0, 2], M[1, 0]]
    return [M[0, 3], M[1, 3], M[2, 3], M[2, 1], M[0, 2], M[1, 0]]


def rot_of_quat(q):
    w, x, y, z = [mp.mpf(c) for c in q]
    n = mp.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_of_rot(R):
    """unit quaternion with w >= 0 of a rotation matrix, from its largest diagonal combination"""
    t = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], -R[0, 0] + R[1, 1] - R[2, 2], -R[0, 0] - R[1, 1] + R[2, 2]]
    k = max(range(4), key=lambda i: t[i])
    r = mp.sqrt(1 + t[k]) * 2
    if k == 0:
        q = [r / 4, (R[2, 1] - R[1, 2]) / r, (R[0, 2] - R[2, 0]) / r, (R[1, 0] - R[0, 1]) / r]
    elif k == 1:
        q = [(R[2, 1] - R[1, 2]) / r, r / 4, (R[0, 1] + R[1, 0]) / r, (R[0, 2] + R[2, 0]) / r]
    elif k == 2:
        q = [(R[0, 2] - R[2, 0]) / r, (R[0, 1] + R[1, 0]) / r, r / 4, (R[1, 2] + R[2, 1]) / r]
    else:
        q = [(R[1, 0] - R[0, 1]) / r, (R[0, 2] + R[2, 0]) / r, (R[1, 2] + R[2, 1]) / r, r / 4]
    return [-c for c in q] if q[0] < 0 else q


def mat(kind, e):
    if kind == "SE2":
        x, y, c, s = [mp.mpf(v) for v in e]
        n = mp.sqrt(c * c + s * s)
        c, s = c / n, s / n
        return mp.matrix([[c, -s, x], [s, c, y], [0, 0, 1]])
    if kind == "SO3":
        return rot_of_quat(e)
    R = rot_of_quat(e[3:7])
    M = mp.eye(4)
    for i in range(3):
        for j in range(3):
            M[i, j] = R[i, j]
        M[i, 3] = mp.mpf(e[i])
    return M


def elem(kind, M):
    if kind == "SE2":
        return [M[0, 2], M[1, 2], M[0, 0], M[1, 0]]
    if kind == "SO3":
        return quat_of_rot(M)
    return [M[0, 3], M[1, 3], M[2, 3]] + quat_of_rot(mp.matrix([[M[i, j] for j in range(3)] for i in range(3)]))


def exp_series(A):
    """matrix exponential by its power series: A / 2^s with norm below 1/2, terms until they vanish at 60 digits, s squarings"""
    nrm = mp.norm(A, "inf")
    s = max(0, int(mp.ceil(mp.log(nrm * 2 + mp.mpf(10) ** -80, 2)))) if nrm > 0 else 0
    X = A / (2 ** s)
    n = A.rows
    term, out, k = mp.eye(n), mp.eye(n), 0
    while True:
        k += 1
        term = term * X / k
        out = out + term
        if mp.norm(term, "inf") < mp.mpf(10) ** -70:
            break
    for _ in range(s):
        out = out * out
    return out


def inv_rigid(kind, M):
    n = M.rows
    if kind == "SO3":
        return M.T
    d = n - 1
    R = mp.matrix([[M[i, j] for j in range(d)] for i in range(d)]).T
    p = R * mp.matrix([M[i, d] for i in range(d)])
    out = mp.eye(n)
    for i in range(d):
        for j in range(d):
            out[i, j] = R[i, j]
        out[i, d] = -p[i]
    return out


def log_matrix(kind, M):
    with mp.workdps(75):
        L = mp.logm(M)
        L = mp.matrix([[mp.re(L[i, j]) for j in range(L.cols)] for i in range(L.rows)])
        a = vee(kind, L)
        back = exp_series(hat(kind, a))
        scale = 1 + mp.norm(M, "inf")
        assert mp.norm(back - M, "inf") < mp.mpf(10) ** -55 * scale, "log does not invert exp"
    return [+c for c in a]


class Part:
    """one part of a bundle: a matrix for a Lie part, a list of mpf for an RN part"""

    def __init__(self, kind, dof):
        self.kind, self.dof, self.E = kind, dof, (dof if kind == "RN" else ELEM[kind])

    def load(self, e):
        return [mp.mpf(v) for v in e] if self.kind == "RN" else mat(self.kind, e)

    def store(self, g):
        return list(g) if self.kind == "RN" else elem(self.kind, g)

    def rplus(self, g, a):
        if self.kind == "RN":
            return [x + mp.mpf(y) for x, y in zip(g, a)]
        return g * exp_series(hat(self.kind, a))

    def rminus(self, a, b):
        if self.kind == "RN":
            return [x - y for x, y in zip(a, b)]
        return log_matrix(self.kind, inv_rigid(self.kind, b) * a)


def parts_of(group):
    return [Part(k, d) for k, d in GROUPS[group]]


def split(parts, row, what):
    out, o = [], 0
    for p in parts:
        w = p.E if what == "elem" else p.dof
        out.append(row[o:o + w])
        o += w
    return out


def load(parts, row):
    return [p.load(e) for p, e in zip(parts, split(parts, row, "elem"))]


def store(parts, g):
    return [c for p, gi in zip(parts, g) for c in p.store(gi)]


def rplus(parts, g, a):
    return [p.rplus(gi, ai) for p, gi, ai in zip(parts, g, split(parts, a, "tan"))]


def rminus(parts, a, b):
    return [c for p, ai, bi in zip(parts, a, b) for c in p.rminus(ai, bi)]


def mpv(xs):
    return [mp.mpf(float(x)) for x in xs]


# ---------------------------------------------------------------- the law and the rollout at 60 digits
def law(parts, t, x, v, gd, vd, ad, kp, kd, ki, windup, t_last, ie):
    """-> u, i_err, g_err (lists of mpf); t_last float (NaN unset)"""
    e = rminus(parts, gd, x)
    if t_last == t_last and t > t_last:
        h = mp.mpf(t) - mp.mpf(t_last)
        ie = [i + h * g for i, g in zip(ie, e)]
        if windup != float("inf"):
            w = mp.mpf(windup)
            ie = [min(max(i, -w), w) for i in ie]
    u = [a + p * g + d * (vdi - vi) + k * i for a, p, g, d, vdi, vi, k, i in zip(ad, kp, e, kd, vd, v, ki, ie)]
    return u, ie, e


def traj(parts, kind, g0, w, t):
    t = mp.mpf(t)
    if kind == 0:
        return rplus(parts, g0, [t * c for c in w]), list(w), [mp.mpf(0)] * len(w)
    s, S = 1 + mp.mpf("0.3") * t, t + mp.mpf("0.15") * t * t
    return rplus(parts, g0, [S * c for c in w]), [s * c for c in w], [mp.mpf("0.3") * c for c in w]


def rollout(parts, kind, steps, x, v, g0, w, kp, kd, ki, windup, umax, t_last, ie):
    dt = mp.mpf(DT)
    cost, u, worst = mp.mpf(0), [mp.mpf(0)] * len(v), mp.mpf(0)
    for k in range(steps):
        tk = mp.mpf(T0) + k * dt
        gd, vd, ad = traj(parts, kind, g0, w, tk)
        tkf = float(tk)
        u, ie, e = law(parts, tkf, x, v, gd, vd, ad, kp, kd, ki, windup, t_last, ie)
        t_last = tkf
        if umax is not None:
            u = [min(max(c, -m), m) for c, m in zip(u, umax)]
        x = rplus(parts, x, [dt * vi + dt * dt / 2 * ui for vi, ui in zip(v, u)])
        v = [vi + dt * ui for vi, ui in zip(v, u)]
        cost += dt * sum(c * c for c in e)
        worst = max(worst, rot_angle(parts, e))
    assert worst < mp.mpf("3.06"), "the error's rotation angle comes too close to pi: %s" % worst
    return x, v, ie, u, cost


def rot_angle(parts, e):
    out, o = mp.mpf(0), 0
    for p in parts:
        seg = e[o:o + p.dof]
        o += p.dof
        if p.kind == "SE2":
            out = max(out, abs(seg[2]))
        elif p.kind == "SO3":
            out = max(out, mp.sqrt(sum(c * c for c in seg)))
        elif p.kind == "SE3":
            out = max(out, mp.sqrt(sum(c * c for c in seg[3:])))
    return out


# ---------------------------------------------------------------- inputs
def class_tangent(rng, parts, cls, row):
    """a tangent whose rotation angle per Lie part lies in the class"""
    out = []
    for p in parts:
        if p.kind == "RN":
            out += list(rng.uniform(-1.5, 1.5, p.dof))
            continue
        if cls == "tiny":
            th = [0.0, 1e-9, -1e-10, 1e-12, 3e-15, -1e-16, 1e-11, 1e-13][row % 8]
        elif cls == "generic":
            th = rng.uniform(0.05, 1.5) * rng.choice([-1, 1])
        else:
            th = rng.uniform(2.0, 3.0) * rng.choice([-1, 1])
        if p.kind == "SE2":
            out += list(rng.uniform(-1.5, 1.5, 2)) + [th]
        else:
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            out += ([] if p.kind == "SO3" else list(rng.uniform(-1.5, 1.5, 3))) + list(th * ax)
    return np.array(out)


def random_element(rng, parts):
    """a generic element as doubles: identity (+) a random tangent, rounded"""
    a = []
    for p in parts:
        a += list(rng.uniform(-2, 2, p.dof))
    ident = [mp.eye(3) if p.kind in ("SE2", "SO3") else mp.eye(4) if p.kind == "SE3" else [mp.mpf(0)] * p.dof for p in parts]
    return np.array(f64(store(parts, rplus(parts, ident, a))))


def displaced(parts, g_row, a):
    """the element g (+) a, rounded to doubles"""
    return np.array(f64(store(parts, rplus(parts, load(parts, g_row), a))))


def gains(rng, D):
    return rng.uniform(0.5, 4.0, D), rng.uniform(0.5, 4.0, D), rng.uniform(0.1, 0.6, D) * rng.choice([-1, 1], D)


def build_inputs():
    """{section.group: dict of input arrays}; deterministic"""
    rng = np.random.default_rng(SEED)
    out = {}
    for group in GROUPS:
        parts = parts_of(group)
        D = sum(p.dof for p in parts)
        rows = dict(x=[], v=[], gd=[], vd=[], ad=[], kp=[], kd=[], ki=[], ie=[], t_last=[], cls=[])
        for ci, cls in enumerate(CLASSES):
            for r in range(N_STEP):
                x = random_element(rng, parts)
                kp, kd, ki = gains(rng, D)
                rows["x"].append(x); rows["gd"].append(displaced(parts, x, class_tangent(rng, parts, cls, r)))
                rows["v"].append(rng.uniform(-1, 1, D)); rows["vd"].append(rng.uniform(-1, 1, D)); rows["ad"].append(rng.uniform(-1, 1, D))
                rows["kp"].append(kp); rows["kd"].append(kd); rows["ki"].append(ki)
                rows["ie"].append(rng.uniform(-0.45, 0.45, D)); rows["t_last"].append(T_LAST_KINDS[r % 8]); rows["cls"].append(ci)
        out["step." + group] = {k: np.array(v) for k, v in rows.items()}

        rows = dict(x=[], v=[], gd=[], vd=[], ad=[], kp=[], kd=[], ki=[], cls=[])
        for ci, cls in enumerate(CLASSES):
            for r in range(N_SEQ):
                xs = [random_element(rng, parts) for _ in SEQ_TIMES]
                kp, kd, ki = gains(rng, D)
                rows["x"].append(xs); rows["gd"].append([displaced(parts, x, class_tangent(rng, parts, cls, r + 2 * k)) for k, x in enumerate(xs)])
                for key in ("v", "vd", "ad"):
                    rows[key].append(rng.uniform(-1, 1, (len(SEQ_TIMES), D)))
                rows["kp"].append(kp); rows["kd"].append(kd); rows["ki"].append(ki); rows["cls"].append(ci)
        out["seq." + group] = {k: np.array(v) for k, v in rows.items()}

        for section, n, kinds in (("roll." + group, N_ROLL, [0]),) + ((("swarm." + group, N_SWARM, [0, 1]),) if group == "SE3" else ()):
            rows = dict(x=[], v=[], g0=[], w=[], kp=[], kd=[], ki=[], ie=[], t_last=[], cls=[], kind=[])
            for kind in kinds:
                for ci, cls in enumerate(CLASSES):
                    for r in range(n):
                        g0 = random_element(rng, parts)
                        w = rng.uniform(-0.4, 0.4, D)
                        gd0, vd0, _ = traj(parts, kind, load(parts, g0), mpv(w), T0)
                        e = class_tangent(rng, parts, cls, r)
                        # x0 with g_des(t0) (-) x0 = e:  x0 = g_des(t0) exp(-e)
                        x0 = np.array(f64(store(parts, rplus(parts, gd0, [-c for c in mpv(e)]))))
                        kp, kd, ki = gains(rng, D)
                        # the large class starts at rest relative to the reference and well damped: the error's angle only shrinks
                        v0 = np.array(f64(vd0)) + (0.0 if cls == "large" else 1.0) * rng.uniform(-0.3, 0.3, D)
                        if cls == "large":
                            kd = np.maximum(kd, 2.0 * np.sqrt(kp))
                        rows["x"].append(x0); rows["v"].append(v0); rows["g0"].append(g0); rows["w"].append(w)
                        rows["kp"].append(kp); rows["kd"].append(kd); rows["ki"].append(ki)
                        rows["ie"].append(rng.uniform(-0.2, 0.2, D)); rows["t_last"].append([float("nan"), T0 - DT][r % 2])
                        rows["cls"].append(ci); rows["kind"].append(kind)
            d = {k: np.array(v) for k, v in rows.items()}
            d["umax"] = rng.uniform(0.8, 1.5, D)
            out[section] = d
    return out


# ---------------------------------------------------------------- evaluation, one row at a time (a job per row)
def eval_row(job):
    section, group, i, d = job
    parts = parts_of(group)
    kind = section.split(".")[0]
    if kind == "step":
        x, gd = load(parts, d["x"]), load(parts, d["gd"])
        res = {}
        for tag, W in (("w", WINDUP), ("inf", float("inf"))):
            u, ie, _ = law(parts, T_STEP, x, mpv(d["v"]), gd, mpv(d["vd"]), mpv(d["ad"]), mpv(d["kp"]), mpv(d["kd"]), mpv(d["ki"]), W,
                           float(d["t_last"]), mpv(d["ie"]))
            res["u_" + tag], res["ie_" + tag] = f64(u), f64(ie)
        return section, i, res
    if kind == "seq":
        ie, t_last, us, ies = [mp.mpf(0)] * len(d["kp"]), float("nan"), [], []
        for k, t in enumerate(SEQ_TIMES):
            u, ie, _ = law(parts, t, load(parts, d["x"][k]), mpv(d["v"][k]), load(parts, d["gd"][k]), mpv(d["vd"][k]), mpv(d["ad"][k]),
                           mpv(d["kp"]), mpv(d["kd"]), mpv(d["ki"]), WINDUP, t_last, ie)
            t_last = t
            us.append(f64(u)); ies.append(f64(ie))
        return section, i, dict(u=us, ie=ies)
    res = {}
    sets = ROLL_SETS if kind == "roll" else {"B": ROLL_SETS["B"]}
    for tag, (steps, clamp) in sets.items():
        x, v, ie, u, cost = rollout(parts, int(d["kind"]), steps, load(parts, d["x"]), mpv(d["v"]), load(parts, d["g0"]), mpv(d["w"]),
                                    mpv(d["kp"]), mpv(d["kd"]), mpv(d["ki"]), WINDUP, mpv(d["umax"]) if clamp else None,
                                    float(d["t_last"]), mpv(d["ie"]))
        res.update({"x_" + tag: f64(store(parts, x)), "v_" + tag: f64(v), "ie_" + tag: f64(ie), "u_" + tag: f64(u), "cost_" + tag: float(cost)})
    return section, i, res


def jobs(inputs, every=1):
    out = []
    for section, d in sorted(inputs.items()):
        group = section.split(".")[1]
        n = len(d["cls"])
        for i in range(0, n, every):
            out.append((section, group, i, {k: (v if k == "umax" else v[i]) for k, v in d.items()}))
    return out


def sample(every=9):
    """[(section, row, {name: regenerated values})] for every `every`-th row of every section -- rollouts of one tick only"""
    inputs = build_inputs()
    out = []
    for job in jobs(inputs, every):
        if job[0].startswith(("roll", "swarm")):
            continue
        out.append(eval_row(job))
    return inputs, out


def main():
    import multiprocessing
    inputs = build_inputs()
    todo = jobs(inputs)
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        done = pool.map(eval_row, todo, chunksize=1)
    out = {"classes": np.array(CLASSES)}
    for section, d in inputs.items():
        for k, v in d.items():
            out["%s.%s" % (section, k)] = v
    results = {}
    for section, i, res in done:
        for k, v in res.items():
            results.setdefault((section, k), {})[i] = v
    for (section, k), rows in results.items():
        out["%s.%s" % (section, k)] = np.array([rows[i] for i in range(len(rows))])
    path = os.path.join(HERE, "pid_reference.npz")
    np.savez_compressed(path, **out)
    sat = [np.mean(np.any(np.abs(out["step.%s.ie_w" % g]) >= WINDUP, axis=1)) for g in GROUPS]
    print("share of step rows with a saturated integral component, per group:", np.round(sat, 2))
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
