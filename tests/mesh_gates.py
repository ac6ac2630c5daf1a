"""Shared by tests/test_mesh_host.py and test_mesh_gpu.py: the fixture tests/golden/mesh_reference.npz (60 digits:
tests/golden/make_golden_mesh.py), the gates, and the comparison.

Gate rule (as tests/pid_gates.py, spline_gates.py): tests/mesh_ref.py is a plain float64 numpy restatement that shares
nothing with the headers; its largest error against the 60-digit values, per case class, is what float64 delivers on
these inputs, and the gate of every comparison is FOUR times that.  Case classes: lgr (nodes and weights, K = 1 .. 15),
mesh.tau0 / nodes / weights / diffmat / intmat (every mesh of the fixture; nodes also of the degree-raised meshes), eval.p0 / p1 / p2, resample (node samples
carried to the degree-raised mesh, states with and inputs without the value at 1), dynerr.exact / resolved / coarse
(the interval errors; the class is the one the fixture assigned by the size of the 60-digit error), flat.tiny /
flat.generic (flat_dynamics of the two example models, by |e|), audit (MPC::dyn_error of synthetic plans of the example MPCs).  Errors are scaled
per row: max |got - ref| / (1 + max |ref|).  Measured by
test_mesh_host.py::test_gate_is_four_times_the_float64_restatements_error, which prints the table and checks that the
restatement still delivers it and that no fixture row is left out.  On the CPU this was written on:"""
import os

import numpy as np

import mesh_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_reference.npz")
MARGIN = 4.0
MEASURED = {
    "lgr": 5.34e-14,
    "mesh.tau0": 6.17e-17,  "mesh.nodes": 2.22e-16,  "mesh.weights": 1.53e-14,  "mesh.diffmat": 1.44e-13,  "mesh.intmat": 4.03e-16,
    "eval.p0": 1.66e-11,  "eval.p1": 3.30e-11,  "eval.p2": 1.81e-10,
    "resample": 7.74e-16,
    "dynerr.exact": 5.58e-16,  "dynerr.resolved": 9.41e-17,  "dynerr.coarse": 4.72e-16,
    "flat.tiny": 8.14e-17,  "flat.generic": 1.60e-16,
    "audit": 8.41e-17,
}
FX = np.load(FIXTURE)
CLASSES = [str(c) for c in FX["classes"]]
MESHES = [str(n) for n in FX["mesh.names"]]
EVALS = [str(n) for n in FX["eval.names"]]
DYN = [str(n) for n in FX["dynerr.names"]]
FLAT = [str(n) for n in FX["flat.names"]]
FLAT_CLASSES = [str(c) for c in FX["flat.classes"]]
AUDIT = [str(n) for n in FX["audit.names"]]
AUDIT_VARIANT = {"vehicle6": 6, "vehicle12": 12, "rigid": 13}    # the harness's MPC variants
CLASS_BOUNDS = {"exact": (0.0, 1e-13), "resolved": (1e-10, 1e-4), "coarse": (1e-3, np.inf)}


def section(name):
    """the arrays of one section ("mesh.basic", "dynerr.ex_ref"), without the prefix"""
    pre = name + "."
    return {k[len(pre):]: FX[k] for k in FX.files if k.startswith(pre) and "." not in k[len(pre):]}


def mesh(name):
    return section("mesh." + name)


def dyn(name):
    d = section("dynerr." + name)
    d["base"] = mesh(str(d["mesh"]))
    d["cls_name"] = CLASSES[int(d["cls"])]
    return d


def gate(key):
    return MARGIN * MEASURED[key]


def check(key, got, ref, who):
    """one row within the gate of its class; the figure is printed first"""
    err = R.scaled_error(got, ref)
    print("%-16s %-34s %.2e (gate %.2e)" % (key, who, err, gate(key)))
    assert err <= gate(key), "%s (%s): %.3e over the gate %.3e" % (key, who, err, gate(key))
    return err


def mesh_rows(name, K, tau0, nodes, weights, diffmat, intmat):
    """[(key, got, ref)] of one mesh's quantities against the fixture; K is compared exactly"""
    m = mesh(name)
    assert np.array_equal(np.asarray(K, dtype=np.int64), m["K"].astype(np.int64)), (name, K, m["K"])
    return [("mesh." + q, g, m[q]) for q, g in (("tau0", tau0), ("nodes", nodes), ("weights", weights), ("diffmat", diffmat), ("intmat", intmat))]


def flat_rows(model, got):
    """[(key, who, got, ref)]: the rows of one model's flat_dynamics values, class by class"""
    d = section("flat." + model)
    return [("flat." + c, model, got[d["cls"] == i], d["out"][d["cls"] == i]) for i, c in enumerate(FLAT_CLASSES)]


def restatement_rows():
    """[(key, who, got, ref)] of tests/mesh_ref.py on every row of the fixture"""
    rows, seen = [], set()
    for K in range(1, 16):
        x, w = R.lgr(K)
        rows += [("lgr", "K=%d x" % K, x, FX["lgr.K%d.x" % K]), ("lgr", "K=%d w" % K, w, FX["lgr.K%d.w" % K])]
        seen |= {"lgr.K%d.x" % K, "lgr.K%d.w" % K}
    for name in MESHES:
        m = mesh(name)
        K, tau0 = R.run_script(m["spec"], m["ops"], m["opdata"])
        n = len(K)
        rows += [(k, name, g, r) for k, g, r in mesh_rows(
            name, K, tau0, R.all_nodes(K, tau0), R.all_weights(K, tau0),
            np.concatenate([R.diffmat(K, tau0, i).ravel() for i in range(n)]), np.concatenate([R.intmat(K, tau0, i).ravel() for i in range(n)]))]
        seen |= {"mesh.%s.%s" % (name, q) for q in m}
    for name in EVALS:
        m, e = mesh(name), section("eval." + name)
        for ei, extend in enumerate((True, False)):
            vals = e["vals"] if extend else e["vals"][:-1]
            for p in range(3):
                got = np.stack([R.evaluate(m["K"], m["tau0"], t, vals, p, extend) for t in e["t"]])
                rows.append(("eval.p%d" % p, "%s extend=%d" % (name, extend), got, e["out"][ei, p]))
        seen |= {"eval.%s.%s" % (name, q) for q in e}
    for name in MESHES:
        m, r = mesh(name), section("resample." + name)
        rows.append(("mesh.nodes", name + " raised", R.raised_nodes(m["K"], m["tau0"]), r["tau"]))
        rows += [("resample", name + " ext", R.resample(m["K"], m["tau0"], r["vals"], True), r["out_ext"]),
                 ("resample", name + " open", R.resample(m["K"], m["tau0"], r["vals"][:-1], False), r["out_open"])]
        seen |= {"resample.%s.%s" % (name, q) for q in r}
    for name in DYN:
        d = dyn(name)
        K, tau0 = d["base"]["K"], d["base"]["tau0"]
        X, U = R.resample(K, tau0, d["vals_x"], True), R.resample(K, tau0, d["vals_u"], False)
        rows += [("resample", name + " X", X, d["X"]), ("resample", name + " U", U, d["U"])]
        t = float(d["t0"]) + (float(d["tf"]) - float(d["t0"])) * R.raised_nodes(K, tau0)
        F = R.dynamics(int(d["fid"]), d["coef"], int(d["nu"]), t, X, U)
        rows.append(("dynerr." + d["cls_name"], name, R.dyn_error(K, tau0, float(d["tf"]) - float(d["t0"]), X, F), d["errs"]))
        seen |= {"dynerr.%s.%s" % (name, q) for q in section("dynerr." + name)}
    for model in FLAT:
        d = section("flat." + model)
        rows += flat_rows(model, R.flat_dynamics(model, d["xl"], d["dxl"], d["ul"], d["e"], d["v"]))
        seen |= {"flat.%s.%s" % (model, q) for q in d}
    for name in AUDIT:
        a = section("audit." + name)
        rows.append(("audit", name, R.audit_errors(str(a["model"]), int(a["K"]), float(a["tf"]), a["primal"]), a["errs"]))
        seen |= {"audit.%s.%s" % (name, q) for q in a}
    return rows, seen | {"classes", "mesh.names", "eval.names", "dynerr.names", "flat.names", "flat.classes", "audit.names"}


def measure():
    """{gate key: worst scaled error of the restatement}, and the fixture keys it did not touch"""
    rows, seen = restatement_rows()
    worst = {}
    for key, _, got, ref in rows:
        worst[key] = max(worst.get(key, 0.0), R.scaled_error(got, ref))
    return worst, sorted(set(FX.files) - seen)
