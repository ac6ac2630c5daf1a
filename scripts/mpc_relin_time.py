"""Times of sequential convex MPC on the device: one warmed tick of MPCSwarmDeviceLin::step(.., passes) with
0 / 1 / 2 re-linearisation passes at 8 192 agents of the planar vehicle, between device events, and mpc_relinearise_kernel alone
(the least of ten warmed runs).  Agents start off the desired trajectory with heading errors up to 1 rad.  Nothing is asserted.

    python scripts/mpc_relin_time.py [--agents 8192] [--K 8 20]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples import models_lib as M  # noqa: E402
from examples import mpc_relin_lib as RL  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=8192)
    ap.add_argument("--K", type=int, nargs="+", default=[8, 20])
    ap.add_argument("--tf", type=float, default=2.0)
    a = ap.parse_args()
    B = a.agents
    rng = np.random.default_rng(1)
    dx0 = np.concatenate([rng.uniform(-0.4, 0.4, (B, 2)), rng.uniform(-1.0, 1.0, (B, 1)), rng.uniform(-0.2, 0.2, (B, 3))], axis=1)
    t = 0.025 * (np.arange(B) % 400)
    for K in a.K:
        d = M.mpc_dims(6, K)
        rd = RL.record_doubles(6, K)
        print("K %d: n %d m %d nnzA %d, record %d doubles, %d agents" % (K, d["n"], d["m"], d["nnzA"], rd, B))
        for passes in (0, 1, 2):
            r = RL.swarm(K, a.tf, t, dx0, passes, prune=1, ticks=3)
            kept = np.isin(r["code"], (0, 4, 5)).mean()
            print("  passes %d: tick %8.3f ms   iterations mean %.1f   plans kept %.4f   audit worst %.3e median %.3e" %
                  (passes, 1e3 * r["seconds"], r["iter"].mean(), kept, np.nanmax(r["agent_max"]), np.nanmedian(r["agent_max"])))
        k = RL.kernel(K, a.tf, t, dx0, reps=10)
        bytes_ = B * 8.0 * (rd + d["n"])
        print("  mpc_relinearise_kernel %8.3f ms   %.1f MB (record written, plan read once) -> %.0f GB/s" %
              (1e3 * k["seconds"], bytes_ / 1e6, bytes_ / k["seconds"] / 1e9))


if __name__ == "__main__":
    main()
