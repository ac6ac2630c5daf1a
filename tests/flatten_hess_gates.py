"""For tests/test_flatten_hess_host.py: the fixture tests/golden/flatten_hess_reference.npz (mpmath,
90 digits, four-point differences of lambda . F at 1e-18: tests/golden/make_golden_flatten_hess.py), the gates, and the comparison.

Gate rule (as tests/flatten_gates.py): tests/flatten_hess_ref.py is a plain float64 numpy restatement that differences the
Jacobians and values of tests/flatten_ref.py with the two steps of the headers and shares no code with them; its largest error
against the high-precision values, per class, is what float64 delivers with this law on these inputs, and the gate of every
comparison is FOUR times that.  Errors are scaled per (array, agent): max |got - ref| / (1 + max |ref|), over the UPPER triangles
(r <= c), which is what the consumers read.  Classes:
  HL      HLf and HLcr: central differences of closed-form Jacobians at 2^-17
  HL_fd   HLg: the integrand carries no jacobian; four-point second differences of its flat values at 2^-13
  d2end   d2theta and d2ce_l: central differences of the end functions' Jacobians at 2^-17
Measured by test_flatten_hess_host.py::test_gate_is_four_times_the_float64_restatements_error, which prints the table and checks
that the restatement still delivers it and that no fixture array is left out.  On the CPU this was written on:"""
import os

import numpy as np

import flatten_hess_ref as HR
import mesh_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flatten_hess_reference.npz")
MARGIN = 4.0
MEASURED = {"HL": 8.84e-11, "HL_fd": 1.12e-07, "d2end": 3.39e-11}
FX = np.load(FIXTURE)
PROBLEMS = [str(n) for n in FX["prob.names"]]
TAU = FX["tau"]
HESS_CLASS = dict(HLf="HL", HLcr="HL", HLg="HL_fd", d2theta="d2end", d2ce_l="d2end")


def problem(name):
    pre = "prob.%s." % name
    return {k[len(pre):]: FX[k] for k in FX.files if k.startswith(pre)}


def gate(key):
    return MARGIN * MEASURED[key]


def upper(a):
    """the upper triangles (r <= c) of an array of squares [..., n, n], flattened"""
    a = np.asarray(a, dtype=np.float64)
    r, c = np.triu_indices(a.shape[-1])
    return a[..., r, c].ravel()


def error(got, ref):
    return R.scaled_error(upper(got), upper(ref))


def check(key, got, ref, who, scale=1.0):
    """the upper triangles of one array within the gate of its class (times `scale`); the figure is printed first"""
    err = error(got, ref)
    print("%-6s %-34s %.2e (gate %.2e)" % (key, who, err, scale * gate(key)))
    assert err <= scale * gate(key), "%s (%s): %.3e over the gate %.3e" % (key, who, err, scale * gate(key))
    return err


def hess_rows(fn):
    """[(class, who, got, ref)] of fn(problem, tau, x, lam, traj) -> dict of the five arrays on the fixture's agents, one row per
    (array, agent): the agents differ in the size of e, and each is held to the gate"""
    rows = []
    for name in PROBLEMS:
        p = problem(name)
        got = fn(name, TAU, p["x"], p["lam"], p["traj"])
        for k, cls in HESS_CLASS.items():
            for a in range(len(p["x"])):
                rows.append((cls, "%s %s agent %d" % (name, k, a), got[k][a], p[k][a]))
    return rows


def measure():
    """{class: worst scaled error of the restatement}, and the fixture keys it did not touch"""
    worst = {}
    for key, _, got, ref in hess_rows(HR.flat_hess_nodes):
        worst[key] = max(worst.get(key, 0.0), error(got, ref))
    seen = {"prob.names", "tau", "check"}
    seen |= {"prob.%s.%s" % (n, k) for n in PROBLEMS for k in tuple(HESS_CLASS) + ("x", "traj", "lam")}
    return worst, sorted(set(FX.files) - seen)
