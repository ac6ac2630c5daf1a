"""Generates tests/golden/spline_reference.npz: inputs and float64-rounded results of the Lie-group splines of
include/smooth_feedback_amd/spline.hpp (the group adjoint Ad of lie.hpp, fit_spline_cubic, Spline<K, G>::operator(), the
PID rollout along a spline), computed with mpmath at 60 digits IN MATRIX FORM ONLY: a pose is its homogeneous matrix, exp is
the power series of the matrix exponential, log is mpmath.logm with every result checked by exp(log) == matrix, and
Ad_g a = vee(g hat(a) g^-1), ad(a) b = vee(hat(a) hat(b) - hat(b) hat(a)) are matrix products.  The matrix forms (hat, vee,
the conversions from and to the flat element storage, the series, the checked logarithm, the PID law) are those of
make_golden_pid.py, next to this file; nothing goes through lie.hpp, tests/lie_ref*.py or a closed form of any group.
pettni/smooth, whose Spline this mirrors, is not available: the curve is defined here.

  curve     segment i, u = (s - tk[i]) / h_i:  g = g_i exp(hat(B_1 v_i1)) ... exp(hat(B_K v_iK)),
            B_j(u) = sum_{l=j..K} C(K,l) u^l (1-u)^(K-l), derivatives term by term;
            vel <- Ad_{exp(-B_j v_j)} vel + B_j' v_j;  acc <- Ad_{exp(-B_j v_j)} acc + B_j' ad(vel) v_j + B_j'' v_j;
            vel /= h_i, acc /= h_i^2.  s < tk[0]: (g_0, 0, 0); s > tk[S]: (g_S, 0, 0); a knot belongs to the segment it
            starts, the last knot to the last segment.
  fit       D_i = log(g_i^-1 g_{i+1}), d_i = D_i / h_i; sigma from the natural-cubic system (dense LU here, per tangent
            coordinate); v_i1 = h_i sigma_i / 3, v_i3 = h_i sigma_{i+1} / 3, v_i2 = log(exp(-v_i1) g_i^-1 g_{i+1} exp(-v_i3)).
            Asserted: the rotation angle of v_i2 never exceeds 2.5.
  rollout   tick k at t_k = t0 + k dt tracks the curve at t_k - ts0 (law, clamp, double-integrator step of make_golden_pid.py)

Groups: R2, SE2, SO3, SE3, SE3R3 = (SE3, R3), SE2R1 = (SE2, R1).  Case classes by the rotation angle between consecutive
knots: "tiny" <= 1e-9, "generic" <= 1.2, "abelian" (even rows: pure body translations; odd rows: rotations about one axis).
Sections of the fixture (every array has one row per case; cls is the class index):
  Ad.<G>.*          g, a -> out = Ad_g a
  curve.<G>.S<S>.*  S = 1, 3 segments, uneven knot times: tk, gk -> V (the fit); (tk, gk, V as doubles), t -> g, vel, acc at times
                    before the start, at every knot, inside every segment, at the end and after it; rollouts of the spline
                    (tk, gk, V as doubles) from t0 = 0.25, dt = 0.05 with time origin ts0: A = 1 tick, B = 40 ticks, C = 40
                    ticks with the input clamp umax -- they start before the first knot and run past the last
  k2.<G>.*          a K = 2 spline of two segments from given control differences: tk, gk, V, t -> g, vel, acc
Run by hand from the repository root (a few minutes on 8 cores):  python tests/golden/make_golden_spline.py
tests/test_spline_host.py regenerates a sample through sample() when mpmath is importable."""
import importlib.util
import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_pid", os.path.join(HERE, "make_golden_pid.py"))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)          # sets mp.mp.dps = 60

SEED = 20261019
CLASSES = ["tiny", "generic", "abelian"]
GROUPS = P.GROUPS
WINDUP = 0.5
T0, DT = 0.25, 0.05
ROLL_SETS = {"A": (1, False), "B": (40, False), "C": (40, True)}
SEGMENTS = (1, 3)
KNOT_TIMES = {1: [0.3, 1.1], 3: [0.3, 0.9, 1.3, 2.0]}
TS0 = [0.0, 0.1]                     # per row of a class
N_AD, N_CURVE, N_K2 = 4, 4, 2        # rows per (group, class)
f64, mpv = P.f64, P.mpv


def ident(p):
    return [mp.mpf(0)] * p.dof if p.kind == "RN" else (mp.eye(4) if p.kind == "SE3" else mp.eye(3))


# ---------------------------------------------------------------- per part, matrix form
def p_exp(p, a):
    return p.rplus(ident(p), a)


def p_mul(p, g, h):
    return [x + y for x, y in zip(g, h)] if p.kind == "RN" else g * h


def p_inv(p, g):
    return [-x for x in g] if p.kind == "RN" else P.inv_rigid(p.kind, g)


def p_log(p, g):
    return list(g) if p.kind == "RN" else P.log_matrix(p.kind, g)


def p_Ad(p, g, a):
    """vee(g hat(a) g^-1)"""
    return list(a) if p.kind == "RN" else P.vee(p.kind, g * P.hat(p.kind, a) * P.inv_rigid(p.kind, g))


def p_ad(p, a, b):
    """vee([hat(a), hat(b)])"""
    if p.kind == "RN":
        return [mp.mpf(0)] * p.dof
    A, B = P.hat(p.kind, a), P.hat(p.kind, b)
    return P.vee(p.kind, A * B - B * A)


def p_angle(p, a):
    if p.kind == "SE2":
        return abs(a[2])
    if p.kind == "SO3":
        return mp.sqrt(sum(c * c for c in a))
    if p.kind == "SE3":
        return mp.sqrt(sum(c * c for c in a[3:]))
    return mp.mpf(0)


def basis(K, j, u):
    """B_j, B_j', B_j'' of degree K at u, from the definition, term by term"""
    B = dB = ddB = mp.mpf(0)
    for l in range(j, K + 1):
        c, m = mp.binomial(K, l), K - l
        def pw(x, n):
            return mp.mpf(0) if n < 0 else x ** n
        B += c * pw(u, l) * pw(1 - u, m)
        dB += c * (l * pw(u, l - 1) * pw(1 - u, m) - m * pw(u, l) * pw(1 - u, m - 1))
        ddB += c * (l * (l - 1) * pw(u, l - 2) * pw(1 - u, m) - 2 * l * m * pw(u, l - 1) * pw(1 - u, m - 1) + m * (m - 1) * pw(u, l) * pw(1 - u, m - 2))
    return B, dB, ddB


def p_curve(p, K, tk, gk, V, s):
    """one part: tk [S+1] mpf, gk [S+1] loaded, V [S][K] tangents (mpf lists) -> g, vel, acc at s"""
    S = len(tk) - 1
    zero = [mp.mpf(0)] * p.dof
    if s < tk[0]:
        return gk[0], zero, zero
    if s > tk[S]:
        return gk[S], zero, zero
    i = max(k for k in range(S) if tk[k] <= s)
    h = tk[i + 1] - tk[i]
    u = (s - tk[i]) / h
    g, vel, acc = gk[i], zero, zero
    for j in range(1, K + 1):
        B, dB, ddB = basis(K, j, u)
        vj = V[i][j - 1]
        g = p_mul(p, g, p_exp(p, [B * c for c in vj]))
        hinv = p_exp(p, [-B * c for c in vj])
        vel = [w + dB * c for w, c in zip(p_Ad(p, hinv, vel), vj)]
        acc = [z + dB * b + ddB * c for z, b, c in zip(p_Ad(p, hinv, acc), p_ad(p, vel, vj), vj)]
    return g, [c / h for c in vel], [c / (h * h) for c in acc]


def p_fit(p, tk, gk):
    """one part: the cubic's control differences [S][3]"""
    S = len(tk) - 1
    h = [tk[i + 1] - tk[i] for i in range(S)]
    rel = [p_mul(p, p_inv(p, gk[i]), gk[i + 1]) for i in range(S)]
    d = [[c / h[i] for c in p_log(p, rel[i])] for i in range(S)]
    A = mp.zeros(S + 1, S + 1)
    rhs = mp.zeros(S + 1, p.dof)
    A[0, 0], A[0, 1], A[S, S - 1], A[S, S] = 2, 1, 1, 2
    for k in range(p.dof):
        rhs[0, k], rhs[S, k] = 3 * d[0][k], 3 * d[S - 1][k]
    for i in range(1, S):
        A[i, i - 1], A[i, i], A[i, i + 1] = h[i], 2 * (h[i - 1] + h[i]), h[i - 1]
        for k in range(p.dof):
            rhs[i, k] = 3 * (h[i] * d[i - 1][k] + h[i - 1] * d[i][k])
    cols = [mp.lu_solve(A, rhs[:, k]) for k in range(p.dof)]
    sig = mp.matrix([[cols[k][i] for k in range(p.dof)] for i in range(S + 1)])
    out = []
    for i in range(S):
        v1 = [h[i] * sig[i, k] / 3 for k in range(p.dof)]
        v3 = [h[i] * sig[i + 1, k] / 3 for k in range(p.dof)]
        v2 = p_log(p, p_mul(p, p_mul(p, p_exp(p, [-c for c in v1]), rel[i]), p_exp(p, [-c for c in v3])))
        assert p_angle(p, v2) <= mp.mpf("2.5"), "the fit's closing log sees a rotation angle above 2.5"
        out.append([v1, v2, v3])
    return out


# ---------------------------------------------------------------- bundles: flat rows in, flat rows out
def split_V(parts, V):
    """V [S][K][D] -> per part [S][K] lists"""
    out, o = [], 0
    for p in parts:
        out.append([[list(vj[o:o + p.dof]) for vj in seg] for seg in V])
        o += p.dof
    return out


def curve(parts, K, tk, gk_rows, V, s):
    """flat doubles in -> g (per part), vel, acc (mpf lists over the bundle)"""
    tkm = [mp.mpf(float(t)) for t in tk]
    gk = [P.load(parts, row) for row in gk_rows]
    Vp = split_V(parts, [[mpv(vj) for vj in seg] for seg in V])
    g, vel, acc = [], [], []
    for pi, p in enumerate(parts):
        gi, v, a = p_curve(p, K, tkm, [gg[pi] for gg in gk], Vp[pi], mp.mpf(float(s)) if not isinstance(s, mp.mpf) else s)
        g.append(gi); vel += v; acc += a
    return g, vel, acc


def fit(parts, tk, gk_rows):
    """-> V [S][3][D] (mpf)"""
    tkm = [mp.mpf(float(t)) for t in tk]
    gk = [P.load(parts, row) for row in gk_rows]
    per = [p_fit(p, tkm, [gg[pi] for gg in gk]) for pi, p in enumerate(parts)]
    S = len(tk) - 1
    return [[[c for pp in per for c in pp[i][j]] for j in range(3)] for i in range(S)]


def rollout(parts, steps, tk, gk_rows, V, ts0, x, v, kp, kd, ki, umax, t_last, ie):
    dt = mp.mpf(DT)
    cost, u, worst = mp.mpf(0), [mp.mpf(0)] * len(v), mp.mpf(0)
    for k in range(steps):
        tkk = mp.mpf(T0) + k * dt
        gd, vd, ad = curve(parts, 3, tk, gk_rows, V, tkk - mp.mpf(float(ts0)))
        tf = float(tkk)
        u, ie, e = P.law(parts, tf, x, v, gd, vd, ad, kp, kd, ki, WINDUP, t_last, ie)
        t_last = tf
        if umax is not None:
            u = [min(max(c, -m), m) for c, m in zip(u, umax)]
        x = P.rplus(parts, x, [dt * vi + dt * dt / 2 * ui for vi, ui in zip(v, u)])
        v = [vi + dt * ui for vi, ui in zip(v, u)]
        cost += dt * sum(c * c for c in e)
        worst = max(worst, P.rot_angle(parts, e))
    assert worst < mp.mpf("3.0"), "the tracking error's rotation angle comes too close to pi: %s" % worst
    return x, v, ie, u, cost


# ---------------------------------------------------------------- inputs
def class_increment(rng, parts, cls, row, axes, scale=1.0):
    """a tangent g_{i+1} (-) g_i of the class; axes: the fixed rotation axis per part of an abelian odd row"""
    out = []
    for pi, p in enumerate(parts):
        if p.kind == "RN":
            out += list(rng.uniform(-1.0, 1.0, p.dof))
            continue
        nlin = {"SE2": 2, "SO3": 0, "SE3": 3}[p.kind]
        lin = list(rng.uniform(-1.0, 1.0, nlin))
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        if cls == "tiny":
            th = [1e-9, -1e-10, 0.0, 1e-12, 3e-15, -1e-16][int(rng.integers(6))]
        elif cls == "generic":
            th = scale * rng.uniform(0.2, 1.2) * rng.choice([-1, 1])
        elif row % 2 == 0:
            th = 0.0                                     # pure body translation (SO3: no motion at all would be void: one axis)
            if p.kind == "SO3":
                th, ax = scale * rng.uniform(0.2, 1.2) * rng.choice([-1, 1]), axes[pi]
        else:
            th, ax, lin = scale * rng.uniform(0.2, 1.2) * rng.choice([-1, 1]), axes[pi], [0.0] * nlin
        out += lin + ([th] if p.kind == "SE2" else list(th * ax))
    return np.array(out)


def knots(rng, parts, cls, row, n, scale=1.0):
    axes = []
    for p in parts:
        ax = rng.normal(size=3)
        axes.append(ax / np.linalg.norm(ax))
    g = [P.random_element(rng, parts)]
    for _ in range(n - 1):
        g.append(P.displaced(parts, g[-1], class_increment(rng, parts, cls, row, axes, scale)))
    return np.array(g)


def build_inputs():
    rng = np.random.default_rng(SEED)
    out = {}
    for group in GROUPS:
        parts = P.parts_of(group)
        D = sum(p.dof for p in parts)
        rows = dict(g=[], a=[], cls=[])
        for ci, cls in enumerate(CLASSES):
            for r in range(N_AD):
                axes = [a / np.linalg.norm(a) for a in rng.normal(size=(len(parts), 3))]
                e0 = np.array(f64(P.store(parts, [ident(p) for p in parts])))
                rows["g"].append(P.random_element(rng, parts) if cls == "generic" else P.displaced(parts, e0, class_increment(rng, parts, cls, r, axes)))
                rows["a"].append(rng.uniform(-1.5, 1.5, D)); rows["cls"].append(ci)
        out["Ad." + group] = {k: np.array(v) for k, v in rows.items()}
        for S in SEGMENTS:
            rows = dict(tk=[], gk=[], t=[], x=[], v=[], kp=[], kd=[], ki=[], ie=[], t_last=[], ts0=[], err=[], cls=[])
            for ci, cls in enumerate(CLASSES):
                for r in range(N_CURVE):
                    tk = np.array(KNOT_TIMES[S]) + np.concatenate([[0.0], rng.uniform(-0.03, 0.03, S)])
                    mid = [tk[i] + rng.uniform(0.2, 0.8) * (tk[i + 1] - tk[i]) for i in range(S)]
                    kp, kd, ki = P.gains(rng, D)
                    rows["tk"].append(tk); rows["gk"].append(knots(rng, parts, cls, r, S + 1))
                    rows["t"].append(np.array([tk[0] - 0.2] + list(tk) + mid + [tk[S] + 0.3]))
                    # the state starts next to the held start pose, at rest: err = g_0 (-) x0, its rotation angle in the class
                    rows["err"].append(class_increment(rng, parts, cls if cls != "abelian" else "generic", r, None, 0.4) * 0.5)
                    rows["v"].append(rng.uniform(-0.2, 0.2, D))
                    rows["kp"].append(kp); rows["kd"].append(np.maximum(kd, 1.5)); rows["ki"].append(ki)
                    rows["ie"].append(rng.uniform(-0.2, 0.2, D)); rows["t_last"].append([float("nan"), T0 - DT][r % 2])
                    rows["ts0"].append(TS0[r % 2]); rows["cls"].append(ci)
            d = {k: np.array(v) for k, v in rows.items()}
            d["x"] = np.array([P.displaced(parts, gk[0], -e) for gk, e in zip(d["gk"], d["err"])])
            del d["err"]
            d["umax"] = rng.uniform(2.0, 4.0, D) * (0.5 if S == 1 else 1.0)      # one segment asks for less: the clamp is to act there too
            out["curve.%s.S%d" % (group, S)] = d
        rows = dict(tk=[], gk=[], V=[], t=[], cls=[])
        for ci, cls in enumerate(CLASSES):
            for r in range(N_K2):
                tk = np.array([0.1, 0.8, 1.2]) + np.concatenate([[0.0], rng.uniform(-0.03, 0.03, 2)])
                axes = [a / np.linalg.norm(a) for a in rng.normal(size=(len(parts), 3))]
                V = np.array([[class_increment(rng, parts, cls, r, axes, 0.5) for _ in range(2)] for _ in range(2)])
                g = [P.random_element(rng, parts)]
                for i in range(2):
                    g.append(P.displaced(parts, P.displaced(parts, g[-1], V[i][0]), V[i][1]))
                mid = [tk[i] + rng.uniform(0.2, 0.8) * (tk[i + 1] - tk[i]) for i in range(2)]
                rows["tk"].append(tk); rows["gk"].append(np.array(g)); rows["V"].append(V)
                rows["t"].append(np.array([tk[0] - 0.2] + list(tk) + mid + [tk[2] + 0.3])); rows["cls"].append(ci)
        out["k2." + group] = {k: np.array(v) for k, v in rows.items()}
    return out


# ---------------------------------------------------------------- evaluation, one row at a time (a job per row)
def eval_times(parts, K, tk, gk, V, ts):
    g, vel, acc = [], [], []
    for s in ts:
        gi, v, a = curve(parts, K, tk, gk, V, s)
        g.append(f64(P.store(parts, gi))); vel.append(f64(v)); acc.append(f64(a))
    return dict(g=g, vel=vel, acc=acc)


def eval_row(job, rollouts=True):
    section, group, i, d = job
    parts = P.parts_of(group)
    kind = section.split(".")[0]
    if kind == "Ad":
        g, a, out = P.load(parts, d["g"]), mpv(d["a"]), []
        o = 0
        for p, gi in zip(parts, g):
            out += p_Ad(p, gi, a[o:o + p.dof])
            o += p.dof
        return section, i, dict(out=f64(out))
    if kind == "k2":
        return section, i, eval_times(parts, 2, d["tk"], d["gk"], d["V"], d["t"])
    V = np.array([[f64(vj) for vj in seg] for seg in fit(parts, d["tk"], d["gk"])])
    res = dict(V=V.tolist())
    res.update(eval_times(parts, 3, d["tk"], d["gk"], V, d["t"]))
    if rollouts:
        for tag, (steps, clamp) in ROLL_SETS.items():
            x, v, ie, u, cost = rollout(parts, steps, d["tk"], d["gk"], V, d["ts0"], P.load(parts, d["x"]), mpv(d["v"]), mpv(d["kp"]), mpv(d["kd"]),
                                        mpv(d["ki"]), mpv(d["umax"]) if clamp else None, float(d["t_last"]), mpv(d["ie"]))
            res.update({"x_" + tag: f64(P.store(parts, x)), "v_" + tag: f64(v), "ie_" + tag: f64(ie), "u_" + tag: f64(u), "cost_" + tag: float(cost)})
    return section, i, res


def jobs(inputs, every=1):
    out = []
    for section, d in sorted(inputs.items()):
        group = section.split(".")[1]
        for i in range(0, len(d["cls"]), every):
            out.append((section, group, i, {k: (v if k == "umax" else v[i]) for k, v in d.items()}))
    return out


def sample(every=7):
    """[(section, row, {name: regenerated values})] for every `every`-th row of every section, without the rollouts"""
    inputs = build_inputs()
    return inputs, [eval_row(job, rollouts=False) for job in jobs(inputs, every)]


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
    path = os.path.join(HERE, "spline_reference.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
