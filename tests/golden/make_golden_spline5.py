"""Generates tests/golden/spline5_reference.npz: 60-digit results for FIVE-knot cubic splines on SE3, the curves of the stream
contract's spline cases (tests/stream_contract.py).  Inputs: the four-knot curves of tests/golden/spline_reference.npz
(section curve.SE3.S3) with a fifth knot that repeats the last increment, g_4 = g_3 (+) (g_3 (-) g_2) at t_4 = t_3 + (t_3 - t_2)
(formed in float64 by tests/pid_ref.py: inputs are doubles either way), so every curve keeps its knot class.  Results: the fit V, the
evaluation (g, vel, acc) at the fixture's times and the rollouts A, B, C, computed by eval_row of make_golden_spline.py (mpmath, 60
digits, matrix form) and rounded to float64.  Run by hand from the repository root:  python tests/golden/make_golden_spline5.py"""
import importlib.util
import multiprocessing as mpc
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
GROUP = "SE3"


def inputs():
    import pid_ref as PR
    import spline_gates as G
    parts = G.GROUPS[GROUP]
    d = {k: np.array(v) for k, v in G.curve(GROUP, 3).items()}
    g4 = np.array([PR.store(parts, PR.rplus(parts, PR.load(parts, row[3]), PR.rminus(parts, PR.load(parts, row[3]), PR.load(parts, row[2])))) for row in d["gk"]])
    d["gk"] = np.concatenate([d["gk"], g4[:, None]], axis=1)
    d["tk"] = np.concatenate([d["tk"], (2 * d["tk"][:, 3] - d["tk"][:, 2])[:, None]], axis=1)
    return {k: d[k] for k in ("cls", "tk", "gk", "t", "ts0", "x", "v", "kp", "kd", "ki", "umax", "t_last", "ie")}


def _row(job):
    spec = importlib.util.spec_from_file_location("make_golden_spline", os.path.join(HERE, "make_golden_spline.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    return M.eval_row(job)


def main():
    d = inputs()
    jobs = [("curve.%s.S4" % GROUP, GROUP, i, {k: (v if k == "umax" else v[i]) for k, v in d.items()}) for i in range(len(d["cls"]))]
    with mpc.Pool(min(8, len(jobs))) as pool:
        rows = pool.map(_row, jobs)
    out = dict(d)
    for k in rows[0][2]:
        out[k] = np.array([r[2][k] for r in sorted(rows, key=lambda r: r[1])], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "spline5_reference.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
