"""PIDSwarmDevice<SE3, functor> (include/smooth_feedback_amd/pid_device.hpp, through examples/models_device.hip) against the
swarm section of tests/golden/pid_reference.npz: half of the agents track a constant twist (the family of
sfb_pid_rollout_batch), half a twist whose size changes with time (v_des(t), with the consistent a_des); gates of
tests/pid_gates.py.  On the constant-twist half the front returns the bits of the C-ABI rollout."""
import numpy as np
import pytest

import pid_gates as G
from examples import models_lib as M

pytestmark = pytest.mark.gpu


def _swarm(d, steps, u_max=None, rows=slice(None)):
    return M.pid_swarm_device(G.T0, G.DT, steps, d["x"][rows], d["v"][rows], d["ie"][rows], d["t_last"][rows], d["kp"][rows], d["kd"][rows],
                              d["ki"][rows], d["g0"][rows], d["w"][rows], d["kind"][rows], windup=G.WINDUP, u_max=u_max)


def test_swarm_front_on_both_trajectory_families():
    d = G.section("swarm", "SE3")
    assert set(d["kind"]) == {0, 1} and np.sum(d["kind"] == 0) == np.sum(d["kind"] == 1)
    got = _swarm(d, 40)
    for kind in (0, 1):
        m = d["kind"] == kind
        G.check("swarm%d" % kind, "SE3", [(k, got[k][m], d[k + "_B"][m]) for k in ("x", "v", "ie", "u", "cost")], d["cls"][m], "PIDSwarmDevice")


@pytest.mark.parametrize("clamp", [False, True])
def test_constant_twist_half_is_the_c_abi_rollout_bit_for_bit(sfb, clamp):
    d = G.section("swarm", "SE3")
    m = d["kind"] == 0
    um = d["umax"] if clamp else None
    got = _swarm(d, 40, u_max=um)
    ref = sfb.pid_rollout_batch_host(G.GROUPS["SE3"], G.T0, G.DT, 40, d["x"][m], d["v"][m], d["g0"][m], d["w"][m], d["kp"][m], d["kd"][m], d["ki"][m],
                                     d["ie"][m], d["t_last"][m], windup_limit=G.WINDUP, u_max=um)
    for k, r in (("x", "x"), ("v", "v"), ("ie", "i_err"), ("u", "u_last"), ("cost", "cost")):
        assert np.array_equal(got[k][m], ref[r]), k


def test_step_of_the_swarm_front_is_the_c_abi_step(sfb):
    """step(t) evaluates the functor at t: the same law on the same triple as sfb_pid_step_batch, bit for bit"""
    import pid_ref as R
    d = G.section("swarm", "SE3")
    m = d["kind"] == 0
    got = _swarm(d, 0, rows=m)
    parts = G.GROUPS["SE3"]
    roll1 = sfb.pid_rollout_batch_host(parts, G.T0, G.DT, 1, d["x"][m], d["v"][m], d["g0"][m], d["w"][m], d["kp"][m], d["kd"][m], d["ki"][m],
                                       d["ie"][m], d["t_last"][m], windup_limit=G.WINDUP)
    assert np.array_equal(got["u"], roll1["u_last"]) and np.array_equal(got["ie"], roll1["i_err"])      # the first tick's law
    assert np.array_equal(got["x"], d["x"][m]) and np.array_equal(got["v"], d["v"][m])                  # a step moves nothing
