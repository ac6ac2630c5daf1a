"""Generator of tests/golden/mpc_relin_reference.npz: start states of the planar vehicle (variant 6, K = 8: two mesh intervals,
tf = 2) off the desired trajectory, heading errors up to 1 rad, for which the numpy restatement tests/mpc_relin_ref.py -- passes
with the CPU oracle's sparse QP solver, Jacobians by central differences -- finds the audit's dynamics error FALLING at every one
of two re-linearisation passes, for every agent; with the restatement's errors after 0, 1 and 2 passes.

Candidates: heading error th on a grid over [-1, 1] without a neighbourhood of 0 (an agent that starts on the trajectory has no
error to lose), position and velocity errors drawn once from a fixed generator.  A candidate is kept when its error falls by at
least a tenth at each pass; the first 67 kept are the fixture (batches 1, 3 and 67 of the GPU test are its leading agents).

    python tests/golden/make_golden_mpc_relin.py      (CPU only; needs the built harness library for the pattern and P)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mpc_relin_ref as Q  # noqa: E402
from examples import models_lib as M  # noqa: E402
from oracle import loader as O  # noqa: E402

K, TF, B, PASSES = 8, 2.0, 67, 2


def main():
    rng = np.random.default_rng(20261021)
    C = 400
    th = np.linspace(-1.0, 1.0, C)
    th = th[np.abs(th) >= 0.2]
    C = len(th)
    dx0 = np.zeros((C, Q.NX))
    dx0[:, :2] = rng.uniform(-0.4, 0.4, (C, 2))
    dx0[:, 2] = th
    dx0[:, 3:] = rng.uniform(-0.2, 0.2, (C, 3))
    order = rng.permutation(C)                       # leading agents of every size of heading error
    dx0 = dx0[order]
    t = 0.025 * np.arange(C)
    pattern = M.mpc_pattern(6, K, TF)
    runs = Q.passes(O, pattern, K, TF, t, dx0, PASSES)
    err = np.stack([r["agent_max"] for r in runs])   # (3, C)
    code = np.stack([r["code"] for r in runs])
    ok = np.all(np.isin(code, Q.KEPT), axis=0) & (err[1] <= 0.9 * err[0]) & (err[2] <= 0.9 * err[1])
    print("%d of %d candidates fall at every pass" % (ok.sum(), C))
    keep = np.nonzero(ok)[0][:B]
    assert len(keep) == B, len(keep)
    assert np.abs(dx0[keep, 2]).max() > 0.9 and np.abs(dx0[keep[:3], 2]).min() >= 0.2
    print("errors after 0 / 1 / 2 passes: worst %.3e %.3e %.3e   median %.3e %.3e %.3e" % (*err[:, keep].max(axis=1), *np.median(err[:, keep], axis=1)))
    np.savez(os.path.join(HERE, "mpc_relin_reference.npz"), K=K, tf=TF, t=t[keep], dx0=dx0[keep], agent_max=err[:, keep], code=code[:, keep].astype(np.int32))


if __name__ == "__main__":
    main()
