"""Shared by tests/test_meshfn_host.py and test_meshfn_gpu.py: the fixture tests/golden/meshfn_reference.npz (60 digits:
tests/golden/make_golden_meshfn.py), the gates, and the comparison.

Gate rule (as tests/mesh_gates.py, pid_gates.py): tests/meshfn_ref.py is a plain float64 numpy restatement that shares
nothing with the headers; its largest error against the 60-digit values, per class, is what float64 delivers on these
inputs, and the gate of every comparison is FOUR times that.  Classes: eval.F / dF / d2F (unscaled and scaled by the
quadrature weights), integrate.F / dF / d2F, dyn.F / dF / d2F.  Errors are scaled per array: max |got - ref| / (1 + max |ref|).
Measured by test_meshfn_host.py::test_gate_is_four_times_the_float64_restatements_error, which prints the table and checks
that the restatement still delivers it and that no fixture array is left out.  On the CPU this was written on:"""
import os

import numpy as np

import meshfn_ref as MR
import mesh_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshfn_reference.npz")
MARGIN = 4.0
MEASURED = {
    "eval.F": 3.41e-14, "eval.dF": 3.20e-14, "eval.d2F": 1.27e-14,
    "integrate.F": 5.26e-14, "integrate.dF": 5.51e-14, "integrate.d2F": 4.12e-14,
    "dyn.F": 8.64e-13, "dyn.dF": 7.27e-13, "dyn.d2F": 6.41e-14,
}
FX = np.load(FIXTURE)
MESHES = [str(n) for n in FX["mesh.names"]]
FNS = [str(n) for n in FX["fn.names"]]
CASES = [str(n) for n in FX["case.names"]]
FUNCTIONS = ("eval", "evals", "integrate", "dyn")


def section(name):
    """the arrays of one section ("mesh.k1", "case.poly_k1"), without the prefix; deeper keys keep their dots"""
    pre = name + "."
    return {k[len(pre):]: FX[k] for k in FX.files if k.startswith(pre)}


def case(name):
    """one case with its mesh (K, tau0, spec, ops) and integrand (dims, terms, coef) resolved"""
    c = section("case." + name)
    c["name"] = name
    c["m"] = section("mesh." + str(c["mesh"]))
    c["f"] = section("fn." + str(c["fn"]))
    c["order"] = int(c["order"])
    c["t0"], c["tf"] = float(c["t0"]), float(c["tf"])
    c["lam"] = {k: c.get("lambda." + ("eval" if k == "evals" else k)) for k in FUNCTIONS}
    return c


def klass(key):
    """"evals.dF" -> "eval.dF": the scaled evaluation is gated with the unscaled one"""
    return key.replace("evals.", "eval.")


def gate(key):
    return MARGIN * MEASURED[klass(key)]


def check(key, got, ref, who):
    """one array within the gate of its class; the figure is printed first"""
    err = R.scaled_error(got, ref)
    print("%-14s %-30s %.2e (gate %.2e)" % (key, who, err, gate(key)))
    assert err <= gate(key), "%s (%s): %.3e over the gate %.3e" % (key, who, err, gate(key))
    return err


def model_values(c):
    """the integrand of a case at its nodes in float64: f (N, nf), J (N, nf, nv), H (N, nf, nv, nv)"""
    m, f = c["m"], c["f"]
    return MR.model(f["dims"], f["terms"], f["coef"], MR.node_times(m["K"], m["tau0"], c["t0"], c["tf"]), c["xs"], c["us"])


def result_keys(c):
    """the result arrays a case carries: "eval.F", "dyn.dF", ..."""
    return [k for k in c if k.split(".")[0] in FUNCTIONS and k.split(".")[-1] in ("F", "dF", "d2F") and not k.startswith("lambda")]


def restatement_rows():
    """[(key, who, got, ref)] of tests/meshfn_ref.py on every result of the fixture, and the fixture keys visited"""
    rows = []
    seen = {"mesh.names", "fn.names", "case.names"}
    for n in MESHES:
        seen |= {"mesh.%s.%s" % (n, q) for q in section("mesh." + n)}
    for n in FNS:
        seen |= {"fn.%s.%s" % (n, q) for q in section("fn." + n)}
    for name in CASES:
        c = case(name)
        f, J, H = model_values(c)
        got = MR.functions(c["m"]["K"], c["m"]["tau0"], c["f"]["dims"], c["t0"], c["tf"], c["xs"], f, J, H, c["lam"], c["order"])
        keys = result_keys(c)
        assert set(keys) == set(got), (name, sorted(set(keys) ^ set(got)))
        rows += [(k, name, got[k], c[k]) for k in keys]
        seen |= {"case.%s.%s" % (name, k) for k in keys}
        seen |= {"case.%s.%s" % (name, q) for q in ("mesh", "fn", "order", "t0", "tf", "xs", "us", "xs_flat") if q in c}
        seen |= {"case.%s.%s" % (name, q) for q in c if q.startswith("lambda.")}
    return rows, seen


def measure():
    """{class: worst scaled error of the restatement}, and the fixture keys it did not touch"""
    rows, seen = restatement_rows()
    worst = {}
    for key, _, got, ref in rows:
        worst[klass(key)] = max(worst.get(klass(key), 0.0), R.scaled_error(got, ref))
    return worst, sorted(set(FX.files) - seen)
