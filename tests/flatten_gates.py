"""Shared by tests/test_flatten_host.py and test_flatten_gpu.py: the fixture tests/golden/flatten_reference.npz (mpmath, 90 digits:
tests/golden/make_golden_flatten.py), the gates, and the comparison.

Gate rule (as tests/ocpnlp_gates.py): tests/flatten_ref.py is a plain float64 numpy restatement that shares nothing with the
headers; its largest error against the high-precision values, per class, is what float64 delivers on these inputs, and the gate of
every comparison is FOUR times that.  Errors are scaled per array: max |got - ref| / (1 + max |ref|).  Classes:
  dr_exp, d_expinv   the Lie operations, per group (SE2, SO3, SE3, X5, X12B)
  F, dF              flat values and Jacobians of the functions with analytic inner Jacobians (dynamics f, running constraint cr)
  F_fd, dF_fd        the integrand g: its inner Jacobian is by forward differences at 2^-26 on the group, in the headers and in
                     the restatement alike
  end, dend          ce and theta, and their Jacobians
Measured by test_flatten_host.py::test_gate_is_four_times_the_float64_restatements_error, which prints the table and checks
that the restatement still delivers it and that no fixture array is left out.  On the CPU this was written on:"""
import os

import numpy as np

import flatten_ref as FR
import mesh_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flatten_reference.npz")
MARGIN = 4.0
MEASURED = {"dr_exp": 1.11e-16, "d_expinv": 1.51e-16, "F": 7.97e-16, "dF": 1.05e-15, "F_fd": 2.38e-15, "dF_fd": 2.05e-07, "end": 1.62e-16, "dend": 2.78e-16}
FX = np.load(FIXTURE)
LIE = [str(n) for n in FX["lie.names"]]
PROBLEMS = [str(n) for n in FX["prob.names"]]
TAU = FX["tau"]
NODE_CLASS = dict(Ff="F", dFf="dF", Fcr="F", dFcr="dF", Fg="F_fd", dFg="dF_fd", ce="end", theta="end", dce="dend", dtheta="dend")


def problem(name):
    pre = "prob.%s." % name
    return {k[len(pre):]: FX[k] for k in FX.files if k.startswith(pre)}


def gate(key):
    return MARGIN * MEASURED[key]


def check(key, got, ref, who):
    """one array within the gate of its class; the figure is printed first"""
    err = R.scaled_error(np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel())
    print("%-8s %-34s %.2e (gate %.2e)" % (key, who, err, gate(key)))
    assert err <= gate(key), "%s (%s): %.3e over the gate %.3e" % (key, who, err, gate(key))
    return err


def lie_rows(fn):
    """[(class, who, got, ref)] of fn(group, op, a, w) -> [count][T][T] on the fixture's Lie points"""
    rows = []
    for g in LIE:
        a, w = FX["lie.%s.a" % g], FX["lie.%s.w" % g]
        rows.append(("dr_exp", g, fn(g, "dr_exp", a, w), FX["lie.%s.dr_exp" % g]))
        rows.append(("d_expinv", g, fn(g, "d_expinv", a, w), FX["lie.%s.d_expinv" % g]))
    return rows


def node_rows(fn):
    """[(class, who, got, ref)] of fn(problem, tau, x, traj) -> dict of node arrays on the fixture's agents, one row per
    (array, agent): the agents differ in the size of e, and each is held to the gate"""
    rows = []
    for name in PROBLEMS:
        p = problem(name)
        got = fn(name, TAU, p["x"], p["traj"])
        for k, cls in NODE_CLASS.items():
            for a in range(len(p["x"])):
                rows.append((cls, "%s %s agent %d" % (name, k, a), got[k][a], p[k][a]))
    return rows


def restatement_lie(group, op, a, w):
    parts = FR.PARTS[group]
    if op == "dr_exp":
        return np.stack([FR.dr_exp(parts, r) for r in a])
    return np.stack([FR.d_expinv(parts, r, v) for r, v in zip(a, w)])


def measure():
    """{class: worst scaled error of the restatement}, and the fixture keys it did not touch"""
    worst = {}
    for key, _, got, ref in lie_rows(restatement_lie) + node_rows(FR.flat_nodes):
        worst[key] = max(worst.get(key, 0.0), R.scaled_error(np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()))
    seen = {"lie.names", "prob.names", "tau"}
    seen |= {"lie.%s.%s" % (g, k) for g in LIE for k in ("a", "w", "dr_exp", "d_expinv")}
    seen |= {"prob.%s.%s" % (n, k) for n in PROBLEMS for k in tuple(NODE_CLASS) + ("x", "traj", "dims")}
    return worst, sorted(set(FX.files) - seen)
