"""Wall-clock time of MPCSwarmDeviceLin::audit() next to the swarm tick it audits (README / DESIGN.md 6d):
python scripts/mpc_audit_time.py [agents] [K] [variant].  Two audit figures: the two launches alone between device events
(warmed, least of five) -- the one to hold against the memory system, whose least traffic is one read of the primal -- and the
whole audit() call end to end on the host clock (upload of the times, launches, download of 8 bytes per agent: PCIe and launch
latency included).  The tick figure is the host clock around the second tick of the same swarm, once with an audit before it
and once without."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples import models_lib as M  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
K = int(sys.argv[2]) if len(sys.argv) > 2 else 50
variant = int(sys.argv[3]) if len(sys.argv) > 3 else 12
nx = 6 if variant == 6 else 12
rng = np.random.default_rng(1)
t, dx0 = 0.025 * (np.arange(B) % 400), rng.uniform(-0.5, 0.5, (B, nx))
n = M.mpc_dims(variant, K)["n"]
for rep in range(3):
    a = M.mpc_swarm_devlin_audit(variant, K, 5.0, t, dx0, audit=True)
    p = M.mpc_swarm_devlin_audit(variant, K, 5.0, t, dx0, audit=False)
    print("rep %d: audit launches %.4f ms by device events (%.1f GB/s of the %.1f MB primal)   audit() end to end %.3f ms   "
          "tick after an audit %.3f ms   tick without %.3f ms   same bits: %s"
          % (rep, 1e3 * a["audit_kernel_seconds"], B * n * 8 / a["audit_kernel_seconds"] / 1e9, B * n * 8 / 1e6, 1e3 * a["audit_seconds"],
             1e3 * a["tick_seconds"], 1e3 * p["tick_seconds"], np.array_equal(a["u_next"], p["u_next"])))
print("agent_max: median %.3e  max %.3e   ival_max: %s   skipped %d" % (np.median(a["agent_max"]), a["agent_max"].max(),
                                                                        np.array2string(a["ival_max"], precision=3), a["skipped"]))
