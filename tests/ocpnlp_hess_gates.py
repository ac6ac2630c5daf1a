"""Shared by tests/test_ocpnlp_hess_host.py and test_ocpnlp_hess_gpu.py: the class `d2l` next to the classes of
tests/ocpnlp_gates.py, for the Lagrangian Hessian sigma d2f + d2g(lambda) of the collocation NLP (OCPNLP::d2l_dx2,
sfb_ocp_nlp_hess_*).

The reference is sigma * d2f + d2g from the 60-digit fixture tests/golden/ocpnlp_reference.npz, with sigma drawn from SIGMAS:
powers of two, so the product is exact and the sum adds one rounding.  Gate rule as in ocpnlp_gates: tests/ocpnlp_ref.py
(NR.nlp(.., order=2), its d2f and d2g combined the same way) is what float64 delivers on these inputs; the gate is FOUR times
its worst scaled error over all cases and those sigmas.  Errors are scaled per array: max |got - ref| / (1 + max |ref|).
Measured by test_ocpnlp_hess_host.py::test_d2l_gate_is_four_times_the_float64_restatements_error, which prints the table
and checks that the restatement still delivers it.  On the CPU this was written on:"""
import numpy as np

import mesh_ref as R
import ocpnlp_gates as G

SIGMAS = (1.0, 0.0, 0.5, -2.0)
# worst per case: bare 6.5e-18, ref 2.0e-15, cross 1.5e-15, mixed 3.7e-16, k13 6.156e-14 at every sigma (k13's d2g part carries it: the
# figure equals the d2g class of ocpnlp_gates because the same entries are the worst ones, not because it was copied)
MEASURED = {"d2l": 6.16e-14}  # (kept here: ocpnlp_gates.MEASURED is compared with the fixture's own classes and stays as it is)


def gate(key="d2l"):
    return G.MARGIN * MEASURED[key]


def check(got, ref, who, key="d2l"):
    """one array within the gate of the class; the figure is printed first"""
    err = R.scaled_error(np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel())
    print("%-8s %-44s %.2e (gate %.2e)" % (key, who, err, gate(key)))
    assert err <= gate(key), "%s (%s): %.3e over the gate %.3e" % (key, who, err, gate(key))
    return err


def reference(c, sigma):
    """sigma d2f + d2g of one fixture case"""
    return sigma * c["d2f"] + c["d2g"]


def measure():
    """{(case, sigma): scaled error of the restatement}"""
    out = {}
    for name in G.CASES:
        c = G.case(name)
        got = G.restatement(c)
        for s in SIGMAS:
            out[(name, s)] = R.scaled_error(s * got["d2f"] + got["d2g"], reference(c, s))
    return out


def contracted(c, x, lam):
    """one agent's arrays of the model-free entry from tests/ocpnlp_ref.py: the Jacobians, and the model Hessians contracted with
    lambda in numpy"""
    import ocpnlp_ref as NR
    nx, nu, nq, ncr, nce = c["dims"]
    mv = NR.models(c["m"]["K"], c["m"]["tau0"], c["dims"], c, x)
    N = len(mv["f"][0])
    _, cb = NR.structure(N, c["dims"])
    lam = np.asarray(lam, dtype=np.float64)
    lf, lq, lcr, lce = lam[cb[0]:cb[1]].reshape(N, nx), lam[cb[1]:cb[2]], lam[cb[2]:cb[3]].reshape(N, ncr), lam[cb[3]:cb[4]]
    return {"dFf": mv["f"][1], "HLf": np.einsum("ij,ijab->iab", lf, mv["f"][2]), "dFg": mv["g"][1], "HLg": np.einsum("j,ijab->iab", lq, mv["g"][2]),
            "dFcr": mv["cr"][1], "HLcr": np.einsum("ij,ijab->iab", lcr, mv["cr"][2]), "d2theta": mv["theta"][2][0],
            "d2ce_l": np.einsum("r,rab->ab", lce, mv["ce"][2])}
