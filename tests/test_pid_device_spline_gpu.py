"""PIDSwarmDevice (include/smooth_feedback_amd/pid_device.hpp) driven by SplineTrajectory<3, SE3> (spline.hpp) gives the
bits sfb_pid_rollout_spline_batch gives on the same data: both run pid_rollout over spline_eval per lane.  G is SE3, not a
bundle: the C-ABI sums a bundle's cost part by part (pid_device.hpp)."""
import numpy as np
import pytest

import spline_gates as G
from examples import models_lib as M

pytestmark = pytest.mark.gpu


def _tile(a, B):
    a = np.asarray(a)
    return a[np.arange(B) % len(a)]


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("S", G.SEGMENTS)
def test_swarm_on_a_spline_trajectory_is_the_rollout_kernel_bit_for_bit(sfb, S, shared):
    d, B = G.curve("SE3", S), 65
    a = {k: _tile(v, B) for k, v in d.items() if k != "umax"}
    tk, gk, V = (d["tk"][3], d["gk"][3], d["V"][3]) if shared else (a["tk"], a["gk"], a["V"])
    for clamp, ts0 in ((False, None), (True, a["ts0"])):
        um = d["umax"] if clamp else None
        ref = sfb.pid_rollout_spline_batch_host(G.GROUPS["SE3"], G.T0, G.DT, 40, a["x"], a["v"], tk, gk, V, a["kp"], a["kd"], a["ki"], a["ie"], a["t_last"],
                                                ts0=ts0, windup_limit=G.WINDUP, u_max=um)
        got = M.pid_swarm_spline_device(G.T0, G.DT, 40, a["x"], a["v"], a["ie"], a["t_last"], a["kp"], a["kd"], a["ki"], tk, gk, V, ts0=ts0,
                                        windup=G.WINDUP, u_max=um)
        for k, r in (("x", "x"), ("v", "v"), ("ie", "i_err"), ("u", "u_last"), ("cost", "cost")):
            assert np.array_equal(got[k], ref[r]), (k, clamp)
