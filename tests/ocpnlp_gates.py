"""Shared by tests/test_ocpnlp_host.py and test_ocpnlp_gpu.py: the fixture tests/golden/ocpnlp_reference.npz (60 digits:
tests/golden/make_golden_ocpnlp.py), the gates, and the comparison.

Gate rule (as tests/meshfn_gates.py): tests/ocpnlp_ref.py is a plain float64 numpy restatement that shares nothing with the
headers; its largest error against the 60-digit values, per class, is what float64 delivers on these inputs, and the gate of
every comparison is FOUR times that.  Classes: f, df, d2f, g, dg, d2g, bounds (gl, gu and w_scaling; xl, xu, the patterns,
var_beg and con_beg compare exactly).  Errors are scaled per array: max |got - ref| / (1 + max |ref|).  Measured by
test_ocpnlp_host.py::test_gate_is_four_times_the_float64_restatements_error, which prints the table and checks that the
restatement still delivers it and that no fixture array is left out.  On the CPU this was written on:"""
import os

import numpy as np

import mesh_ref as R
import ocpnlp_ref as NR

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ocpnlp_reference.npz")
MARGIN = 4.0
MEASURED = {"f": 1.51e-16, "df": 1.01e-16, "d2f": 9.60e-17, "g": 7.49e-13, "dg": 1.05e-12, "d2g": 6.16e-14, "bounds": 1.78e-13}
FX = np.load(FIXTURE)
CASES = [str(n) for n in FX["case.names"]]
MESHES = [str(n) for n in FX["mesh.names"]]
CLASSES = ("f", "df", "d2f", "g", "dg", "d2g")
EXACT = ("xl", "xu", "dg.rowptr", "dg.colind", "h.colptr", "h.rowind", "var_beg", "con_beg")
INPUTS = ("mesh", "dims", "x", "lambda", "crl", "cru", "cel", "ceu")


def section(name):
    pre = name + "."
    return {k[len(pre):]: FX[k] for k in FX.files if k.startswith(pre)}


def case(name):
    """one case with its mesh (K, tau0, spec, ops) resolved; the term tables stay under "terms.*" / "coef.*" """
    c = section("case." + name)
    c["name"] = name
    c["m"] = section("mesh." + str(c["mesh"]))
    c["dims"] = tuple(int(v) for v in c["dims"])
    return c


def gate(key):
    return MARGIN * MEASURED[key]


def check(key, got, ref, who):
    """one array within the gate of its class; the figure is printed first"""
    err = R.scaled_error(np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel())
    print("%-8s %-34s %.2e (gate %.2e)" % (key, who, err, gate(key)))
    assert err <= gate(key), "%s (%s): %.3e over the gate %.3e" % (key, who, err, gate(key))
    return err


def restatement(c, x=None, lam=None, order=2):
    """tests/ocpnlp_ref.py on a case (on its own x, lambda unless others are given)"""
    return NR.nlp(c["m"]["K"], c["m"]["tau0"], c["dims"], c, c["x"] if x is None else x, c["lambda"] if lam is None else lam,
                  (c["crl"], c["cru"], c["cel"], c["ceu"]), order)


def restatement_rows():
    """[(class, who, got, ref)] of the restatement on every result of the fixture, and the fixture keys visited"""
    rows = []
    seen = {"case.names", "mesh.names"}
    for n in MESHES:
        seen |= {"mesh.%s.%s" % (n, q) for q in section("mesh." + n)}
    for name in CASES:
        c = case(name)
        got = restatement(c)
        K, dims = c["m"]["K"], c["dims"]
        exact = {"xl": got["xl"], "xu": got["xu"], "dg.rowptr": NR.dg_pattern(K, dims)[0], "dg.colind": NR.dg_pattern(K, dims)[1],
                 "h.colptr": NR.h_pattern(K, dims)[0], "h.rowind": NR.h_pattern(K, dims)[1], "var_beg": NR.structure(int(np.sum(K)), dims)[0],
                 "con_beg": NR.structure(int(np.sum(K)), dims)[1]}
        for k in EXACT:
            assert np.array_equal(exact[k], c[k]), (name, k)
        rows += [(k, name, got[k], c[k]) for k in CLASSES]
        rows += [("bounds", name + " " + k, got[k], c[k]) for k in ("gl", "gu", "w_scaling")]
        seen |= {"case.%s.%s" % (name, k) for k in CLASSES + EXACT + INPUTS + ("gl", "gu", "w_scaling")}
        seen |= {"case.%s.%s" % (name, k) for k in c if k.startswith("terms.") or k.startswith("coef.")}
    return rows, seen


def measure():
    """{class: worst scaled error of the restatement}, and the fixture keys it did not touch"""
    rows, seen = restatement_rows()
    worst = {}
    for key, _, got, ref in rows:
        worst[key] = max(worst.get(key, 0.0), R.scaled_error(np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()))
    return worst, sorted(set(FX.files) - seen)
