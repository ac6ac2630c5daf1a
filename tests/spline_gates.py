"""Shared by tests/test_spline_host.py, test_spline_gpu.py, test_pid_spline_gpu.py and test_pid_device_spline_gpu.py: the
fixture tests/golden/spline_reference.npz (60 digits, matrix form: tests/golden/make_golden_spline.py), the gates, and the
comparison.

Gate rule (as tests/pid_gates.py): tests/spline_ref.py is a plain float64 restatement in matrix form that shares nothing
with the fronts; its largest error against the 60-digit values, per case class, is what float64 delivers on these inputs,
and the gate of every comparison is FOUR times that.  A case class is (section, knot class): sections Ad (the group
adjoint), fit (the control differences of fit_spline_cubic), eval (pose, body velocity, body acceleration of the cubic at
times before, on, between and after the knots), k2 (the same for a K = 2 spline), rollA / rollB / rollC (1 tick, 40 ticks,
40 ticks with the input clamp, along the spline), steps40 (the 40 ticks of rollB done one call of the law at a time, the
desired triple evaluated tick by tick and the state handed on as flat doubles with the double-integrator step of
tests/pid_ref.py in between: stepwise_rollout below); knot classes tiny (rotation angle between consecutive knots <= 1e-9),
generic (<= 1.2), abelian (pure body translations, or rotations about one axis).  Errors are scaled per row and quantity:
max |got - ref| / (1 + max |ref|); elements are compared as their homogeneous matrices.  Measured by
test_spline_host.py::test_gate_is_four_times_the_float64_restatements_error, which prints the table and checks that the
restatement still delivers it.  Each (group, S, class) has four rows, so the worst of 48 rows per class is taken.  Worst over
the six groups and S = 1, 3, on the CPU this was written on:"""
import os

import numpy as np

import pid_ref as PR
import spline_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spline_reference.npz")
MARGIN = 4.0
MEASURED = {
    "Ad.tiny": 1.17e-16,  "Ad.generic": 8.49e-16,  "Ad.abelian": 1.45e-16,
    "fit.tiny": 2.39e-16,  "fit.generic": 2.79e-16,  "fit.abelian": 2.20e-16,
    "eval.tiny": 5.29e-16,  "eval.generic": 1.12e-15,  "eval.abelian": 1.10e-15,
    "k2.tiny": 5.06e-16,  "k2.generic": 3.18e-16,  "k2.abelian": 1.87e-16,
    "rollA.tiny": 6.54e-16,  "rollA.generic": 6.63e-16,  "rollA.abelian": 4.82e-16,
    "rollB.tiny": 1.44e-15,  "rollB.generic": 1.67e-15,  "rollB.abelian": 2.23e-15,
    "rollC.tiny": 1.42e-15,  "rollC.generic": 1.93e-15,  "rollC.abelian": 1.80e-15,
    "steps40.tiny": 7.71e-15,  "steps40.generic": 6.19e-15,  "steps40.abelian": 3.13e-15,
}
FX = np.load(FIXTURE)
CLASSES = list(FX["classes"])
GROUPS = R.GROUPS
SEGMENTS = (1, 3)
WINDUP = 0.5
T0, DT = 0.25, 0.05
ROLL_SETS = {"A": (1, False), "B": (40, False), "C": (40, True)}
SECTIONS = ("Ad", "fit", "eval", "k2", "rollA", "rollB", "rollC", "steps40")


def section(name):
    """the arrays of one section of the fixture ("Ad.SE3", "curve.SE3.S3", "k2.SE3"), without the prefix"""
    pre = name + "."
    return {k[len(pre):]: FX[k] for k in FX.files if k.startswith(pre) and "." not in k[len(pre):]}


def curve(group, S):
    return section("curve.%s.S%d" % (group, S))


def gate(sec, cls):
    return MARGIN * MEASURED["%s.%s" % (sec, cls)]


def errors(group, pairs, cls):
    """pairs: [(name, got, ref)]; a name starting with x or g holds elements (flat, any number per row, or already matrix
    rows when the width says so).  -> {class: worst scaled error over the quantities}"""
    parts = GROUPS[group]
    worst = np.zeros(len(cls))
    for name, got, ref in pairs:
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        if name[0] in "xg":
            E = R.widths(parts)[0]
            ref = R.matrix_rows(parts, ref.reshape(-1, E)).reshape(len(cls), -1)
            got = got.reshape(len(cls), -1)
            if got.shape != ref.shape:
                got = R.matrix_rows(parts, got.reshape(-1, E)).reshape(len(cls), -1)
        assert got.size == ref.size, (group, name, got.shape, ref.shape)
        assert np.all(np.isfinite(got)), (group, name)
        worst = np.maximum(worst, R.scaled_error(got, ref))
    return R.per_class(worst, np.asarray(cls), CLASSES)


def check(sec, group, pairs, cls, who):
    """every class of the section within its gate; the figures are printed first"""
    err = errors(group, pairs, cls)
    print("%-7s %-6s %-26s %s" % (sec, group, who, "  ".join("%s %.2e (gate %.2e)" % (c, e, gate(sec, c)) for c, e in sorted(err.items()))))
    bad = {c: e for c, e in err.items() if not e <= gate(sec, c)}
    assert not bad, "%s %s (%s): over the gate: %s" % (sec, group, who, {c: (e, gate(sec, c)) for c, e in bad.items()})
    return err


def eval_pairs(d, got):
    return [("g", got[0], d["g"]), ("vel", got[1], d["vel"]), ("acc", got[2], d["acc"])]


def roll_pairs(d, tag, got):
    """got: the dict of pid_rollout*_host (x, v, i_err, u_last, cost)"""
    return [(k, got[g], d["%s_%s" % (k, tag)]) for k, g in (("x", "x"), ("v", "v"), ("ie", "i_err"), ("u", "u_last"), ("cost", "cost"))]


def stepwise_rollout(group, S, law, evaluate):
    """the 40 ticks of set B as 40 calls of `evaluate(parts, tk, gk, V, t [n][1]) -> g, vel, acc` and of `law(parts, t, x, v, gd,
    vd, ad, kp, kd, ki, ie, t_last) -> u, ie, t_last` on flat arrays, with the double-integrator step and the cost by
    tests/pid_ref.py (numpy, matrix form) in between; the state travels from tick to tick as flat doubles.
    -> (cls, pairs) for check("steps40", ...)"""
    d = curve(group, S)
    parts = GROUPS[group]
    x, v, ie, tl = d["x"].copy(), d["v"].copy(), d["ie"].copy(), d["t_last"].copy()
    cost, u = np.zeros(len(x)), None
    for k in range(ROLL_SETS["B"][0]):
        t = T0 + k * DT
        gd, vd, ad = [a[:, 0] for a in evaluate(parts, d["tk"], d["gk"], d["V"], (t - d["ts0"])[:, None])]
        e = np.array([PR.rminus(parts, PR.load(parts, g), PR.load(parts, xx)) for g, xx in zip(gd, x)])
        u, ie, tl = law(parts, t, x, v, gd, vd, ad, d["kp"], d["kd"], d["ki"], ie, tl)
        x, v = PR.integrate(parts, x, v, u, DT)
        cost += DT * np.sum(e * e, axis=1)
    return d["cls"], [("x", x, d["x_B"]), ("v", v, d["v_B"]), ("ie", ie, d["ie_B"]), ("u", u, d["u_B"]), ("cost", cost, d["cost_B"])]


def restatement_law(parts, t, x, v, gd, vd, ad, kp, kd, ki, ie, t_last):
    u, ie = PR.law(parts, t, x, v, gd, vd, ad, kp, kd, ki, WINDUP, t_last, ie)
    return u, ie, np.full(len(x), t)


def restatement_pairs(group):
    """[(section key, cls, pairs)] of tests/spline_ref.py on every section of one group"""
    parts = GROUPS[group]
    a = section("Ad." + group)
    out = [("Ad", a["cls"], [("out", R.Ad(parts, a["g"], a["a"]), a["out"])])]
    k2 = section("k2." + group)
    out.append(("k2", k2["cls"], eval_pairs(k2, R.evaluate(parts, k2["tk"], k2["gk"], k2["V"], k2["t"]))))
    for S in SEGMENTS:
        d = curve(group, S)
        out.append(("fit", d["cls"], [("V", R.fit(parts, d["tk"], d["gk"]), d["V"])]))
        out.append(("eval", d["cls"], eval_pairs(d, R.evaluate(parts, d["tk"], d["gk"], d["V"], d["t"]))))
        for tag, (steps, clamp) in ROLL_SETS.items():
            r = R.rollout(parts, T0, DT, steps, d["x"], d["v"], d["tk"], d["gk"], d["V"], d["ts0"], d["kp"], d["kd"], d["ki"], WINDUP,
                          d["umax"] if clamp else None, d["t_last"], d["ie"])
            out.append(("roll" + tag, d["cls"], [(k, r[k], d["%s_%s" % (k, tag)]) for k in ("x", "v", "ie", "u", "cost")]))
        cls, pairs = stepwise_rollout(group, S, restatement_law, R.evaluate)
        out.append(("steps40", cls, pairs))
    return out


def measure():
    """{gate key: worst scaled error of the restatement over the groups and segment counts}"""
    worst = {}
    for group in GROUPS:
        for key, cls, pairs in restatement_pairs(group):
            for c, e in errors(group, pairs, cls).items():
                k = "%s.%s" % (key, c)
                worst[k] = max(worst.get(k, 0.0), e)
    return worst
