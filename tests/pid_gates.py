"""Shared by tests/test_pid_host.py, test_pid_gpu.py and test_pid_device_gpu.py: the fixture tests/golden/pid_reference.npz
(60 digits, matrix form: tests/golden/make_golden_pid.py), the gates, and the comparison.

Gate rule (as tests/test_lie_host.py and test_lie_se3_host.py): tests/pid_ref.py is a plain float64 restatement in matrix form
that shares nothing with the fronts; its largest error against the 60-digit values, per case class, is what float64 delivers
on these inputs, and the gate of every comparison is FOUR times that.  A case class is (section, angle class): sections
step (one call; windup 0.5 and +inf), seq (four calls of one controller), rollA / rollB / rollC (1 tick, 40 ticks, 40 ticks
with the input clamp), steps40 (the 40 ticks of rollB done one call of the law at a time, with the state handed from tick to
tick as flat doubles and the double-integrator step by tests/pid_ref.py in between: stepwise_rollout below -- every tick
rounds the pose to a quaternion and back, which the one-launch rollout does not, so the procedure has its own float64
error: with the restatement's own law it is 5.2e-15 on SE3 in the tiny class, where rollB has 9.2e-16),
swarm0 / swarm1 (40 ticks on the two trajectory families of the device swarm test); angle classes
tiny (|th| <= 1e-9), generic, large (2 <= |th| <= 3) by the rotation angle of g_des (-) x at the first call.  Errors are
scaled per row and quantity: max |got - ref| / (1 + max |ref|); elements are compared as their homogeneous matrices.
Measured by test_pid_host.py::test_gate_is_four_times_the_float64_restatements_error, which prints the table and checks that
the restatement still delivers it; worst over the six groups, on the CPU this was written on:"""
import os

import numpy as np

import pid_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pid_reference.npz")
MARGIN = 4.0
MEASURED = {
    "step.tiny": 5.44e-16,     "step.generic": 3.95e-16,   "step.large": 7.89e-16,
    "seq.tiny": 3.03e-16,      "seq.generic": 3.54e-16,    "seq.large": 8.76e-16,
    "rollA.tiny": 4.08e-16,    "rollA.generic": 4.37e-16,  "rollA.large": 7.69e-16,
    "rollB.tiny": 9.18e-16,    "rollB.generic": 2.08e-15,  "rollB.large": 1.35e-15,
    "rollC.tiny": 1.16e-15,    "rollC.generic": 2.17e-15,  "rollC.large": 2.33e-15,
    "steps40.tiny": 5.18e-15,  "steps40.generic": 3.43e-15, "steps40.large": 1.94e-15,
    "swarm0.tiny": 8.46e-16,   "swarm0.generic": 8.22e-16, "swarm0.large": 1.30e-15,
    "swarm1.tiny": 1.22e-15,   "swarm1.generic": 1.14e-15, "swarm1.large": 1.22e-15,
}
FX = np.load(FIXTURE)
CLASSES = list(FX["classes"])
GROUPS = R.GROUPS
WINDUP = 0.5
T_STEP = 1.0
SEQ_TIMES = [0.1, 0.4, 0.4, 0.3]
T0, DT = 0.25, 0.05
ROLL_SETS = {"A": (1, False), "B": (40, False), "C": (40, True)}


def section(name, group):
    """the arrays of one section of the fixture, without the prefix"""
    pre = "%s.%s." % (name, group)
    return {k[len(pre):]: FX[k] for k in FX.files if k.startswith(pre)}


def gate(sec, cls):
    return MARGIN * MEASURED["%s.%s" % (sec, cls)]


def errors(group, pairs, cls):
    """pairs: [(name, got, ref)]; a name starting with x holds elements (flat, or already matrix rows when the width says
    so).  -> {class: worst scaled error over the quantities}"""
    parts = GROUPS[group]
    worst = np.zeros(len(cls))
    for name, got, ref in pairs:
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        if name.startswith("x"):
            E = R.widths(parts)[0]
            ref = R.matrix_rows(parts, ref.reshape(-1, E)).reshape(len(cls), -1)
            got = got.reshape(len(cls), -1)
            if got.shape != ref.shape:
                got = R.matrix_rows(parts, got.reshape(-1, E)).reshape(len(cls), -1)
        assert np.all(np.isfinite(got)), (group, name)
        worst = np.maximum(worst, R.scaled_error(got, ref))
    return R.per_class(worst, np.asarray(cls), CLASSES)


def check(sec, group, pairs, cls, who):
    """every class of the section within its gate; the figures are printed first"""
    err = errors(group, pairs, cls)
    print("%-7s %-6s %-22s %s" % (sec, group, who, "  ".join("%s %.2e (gate %.2e)" % (c, e, gate(sec, c)) for c, e in sorted(err.items()))))
    bad = {c: e for c, e in err.items() if not e <= gate(sec, c)}
    assert not bad, "%s %s (%s): over the gate: %s" % (sec, group, who, {c: (e, gate(sec, c)) for c, e in bad.items()})
    return err


# ---------------------------------------------------------------- the float64 restatement on every section
def restatement_pairs(sec, group):
    """[(section key, cls, pairs)] of tests/pid_ref.py on one section and group"""
    parts = GROUPS[group]
    out = []
    if sec == "step":
        d = section("step", group)
        pairs = []
        for tag, W in (("w", WINDUP), ("inf", np.inf)):
            u, ie = R.law(parts, T_STEP, d["x"], d["v"], d["gd"], d["vd"], d["ad"], d["kp"], d["kd"], d["ki"], W, d["t_last"], d["ie"])
            pairs += [("u_" + tag, u, d["u_" + tag]), ("ie_" + tag, ie, d["ie_" + tag])]
        out.append(("step", d["cls"], pairs))
    elif sec == "seq":
        d = section("seq", group)
        n = len(d["cls"])
        ie, tl, us, ies = np.zeros_like(d["kp"]), np.full(n, np.nan), [], []
        for k, t in enumerate(SEQ_TIMES):
            u, ie = R.law(parts, t, d["x"][:, k], d["v"][:, k], d["gd"][:, k], d["vd"][:, k], d["ad"][:, k], d["kp"], d["kd"], d["ki"], WINDUP, tl, ie)
            tl = np.full(n, t)
            us.append(u); ies.append(ie)
        out.append(("seq", d["cls"], [("u", np.stack(us, 1), d["u"]), ("ie", np.stack(ies, 1), d["ie"])]))
    else:
        d = section(sec, group)
        for tag, (steps, clamp) in (ROLL_SETS.items() if sec == "roll" else [("B", ROLL_SETS["B"])]):
            r = R.rollout(parts, d["kind"], T0, DT, steps, d["x"], d["v"], d["g0"], d["w"], d["kp"], d["kd"], d["ki"], WINDUP,
                          d["umax"] if clamp else None, d["t_last"], d["ie"])
            pairs = [(k, r[k], d["%s_%s" % (k, tag)]) for k in ("x", "v", "ie", "u", "cost")]
            if sec == "roll":
                out.append(("roll" + tag, d["cls"], pairs))
            else:
                for kind in (0, 1):
                    m = d["kind"] == kind
                    out.append(("swarm%d" % kind, d["cls"][m], [(k, np.asarray(g)[m], np.asarray(rf)[m]) for k, g, rf in pairs]))
    return out


def stepwise_rollout(group, law):
    """the 40 ticks of the roll section's set B as 40 calls of `law(parts, t, x, v, gd, vd, ad, kp, kd, ki, ie, t_last) -> u, ie,
    t_last` on flat arrays, with the trajectory, the double-integrator step and the cost by tests/pid_ref.py (numpy, matrix
    form) in between; the state travels from tick to tick as flat doubles.  -> (cls, pairs) for check("steps40", ...)"""
    r = section("roll", group)
    parts = GROUPS[group]
    x, v, ie, tl = r["x"].copy(), r["v"].copy(), r["ie"].copy(), r["t_last"].copy()
    cost, u = np.zeros(len(x)), None
    for k in range(ROLL_SETS["B"][0]):
        t = T0 + k * DT
        gd = np.array([R.store(parts, R.traj(parts, 0, R.load(parts, g0), w, t)[0]) for g0, w in zip(r["g0"], r["w"])])
        e = np.array([R.rminus(parts, R.load(parts, g), R.load(parts, xx)) for g, xx in zip(gd, x)])
        u, ie, tl = law(parts, t, x, v, gd, r["w"], np.zeros_like(v), r["kp"], r["kd"], r["ki"], ie, tl)
        x, v = R.integrate(parts, x, v, u, DT)
        cost += DT * np.sum(e * e, axis=1)
    return r["cls"], [("x", x, r["x_B"]), ("v", v, r["v_B"]), ("ie", ie, r["ie_B"]), ("u", u, r["u_B"]), ("cost", cost, r["cost_B"])]


def restatement_law(parts, t, x, v, gd, vd, ad, kp, kd, ki, ie, t_last):
    u, ie = R.law(parts, t, x, v, gd, vd, ad, kp, kd, ki, WINDUP, t_last, ie)
    return u, ie, np.full(len(x), t)


def measure():
    """{gate key: worst scaled error of the restatement over the groups}"""
    worst = {}
    for group in GROUPS:
        for sec in ("step", "seq", "roll") + (("swarm",) if group == "SE3" else ()):
            for key, cls, pairs in restatement_pairs(sec, group):
                for c, e in errors(group, pairs, cls).items():
                    k = "%s.%s" % (key, c)
                    worst[k] = max(worst.get(k, 0.0), e)
        cls, pairs = stepwise_rollout(group, restatement_law)
        for c, e in errors(group, pairs, cls).items():
            worst["steps40.%s" % c] = max(worst.get("steps40.%s" % c, 0.0), e)
    return worst
