"""The fused dynamics-error audit of MPC plans (include/smooth_feedback_amd/mesh_device.hpp: mpc_dyn_error_device, through
sfbx_mpc_audit_device of the example harness) and MPC::dyn_error of the host front, against the 60-digit fixture
tests/golden/mesh_reference.npz (audit.*: synthetic smooth plans, not QP solutions) within the gate of tests/mesh_gates.py
(four times the float64 numpy restatement's own error).  Agent counts 1, 65 and 130: less than a wave of (agent, interval,
point) lanes, a partly filled last block, several blocks; 2 and 13 intervals."""
import numpy as np
import pytest

import mesh_gates as G
from examples import models_lib as M

pytestmark = pytest.mark.gpu
OPTIMAL, POLISH_FAILED, PRIMAL_INFEASIBLE, MAX_ITERATIONS, MAX_TIME = 0, 1, 2, 4, 5


def _case(name):
    a = G.section("audit." + name)
    return a, G.AUDIT_VARIANT[str(a["model"])], int(a["K"]), float(a["tf"])


@pytest.mark.parametrize("B", [1, 65, 130])
@pytest.mark.parametrize("name", G.AUDIT)
def test_audit_kernel_against_the_fixture(name, B):
    a, variant, K, tf = _case(name)
    got = M.mpc_audit_device(variant, K, tf, float(a["t"]), np.tile(a["primal"], (B, 1)))
    for b in sorted({0, B // 2, B - 1}):
        G.check("audit", got["errs"][b], a["errs"], "%s kernel, B=%d agent %d" % (name, B, b))
    assert np.array_equal(got["errs"], np.tile(got["errs"][0], (B, 1)))
    assert np.array_equal(got["agent_max"], got["errs"].max(axis=1)) and np.array_equal(got["ival_max"], got["errs"].max(axis=0))
    assert got["skipped"] == 0


@pytest.mark.parametrize("name", G.AUDIT)
def test_audit_kernel_and_host_front_agree_within_the_gate(name):
    """not bit for bit: sin / cos of the two maths libraries and the summation order differ"""
    a, variant, K, tf = _case(name)
    scale = 1.0 + 0.25 * (np.arange(7) % 4)
    plans, t = a["primal"][None, :] * scale[:, None], 0.3 + 0.1 * np.arange(7)
    host = M.mpc_dyn_error_host(variant, K, tf, t, plans)
    dev = M.mpc_audit_device(variant, K, tf, t, plans)["errs"]
    G.check("audit", host[0], a["errs"], name + " host front")
    for b in range(7):
        G.check("audit", dev[b], host[b], "%s kernel against the host front, agent %d" % (name, b))
    assert len({tuple(r) for r in dev[:4]}) == 4                                   # the plans do differ


def test_summaries_leave_out_rejected_plans_and_plans_with_a_nan():
    a, variant, K, tf = _case("v6_13")
    B = 70
    plans = a["primal"][None, :] * (0.2 + 0.8 * np.random.default_rng(5).uniform(size=B))[:, None]
    code = np.full(B, OPTIMAL, np.int32)
    code[[3, 40]] = MAX_ITERATIONS, MAX_TIME                                       # kept, as the swarm keeps their plans
    code[[7, 41, 69]] = PRIMAL_INFEASIBLE, POLISH_FAILED, 6                        # left out
    plans[7] *= 6.0                                                                # the rejected plan with the largest error
    plans[20, 11] = np.nan                                                         # a NaN in the first interval of agent 20
    got = M.mpc_audit_device(variant, K, tf, 0.3, plans, code)
    errs = got["errs"]
    assert np.isnan(errs[20, 0]) and np.all(np.isfinite(np.delete(errs, 20, axis=0))) and np.all(np.isfinite(errs[20, 2:]))
    assert np.isnan(got["agent_max"][20]) and np.array_equal(np.delete(got["agent_max"], 20), np.delete(errs, 20, axis=0).max(axis=1))
    keep = np.ones(B, bool)
    keep[[7, 41, 69, 20]] = False
    assert got["skipped"] == 4 and np.array_equal(got["ival_max"], errs[keep].max(axis=0))
    assert errs[7].max() > got["ival_max"].max()                                   # ... and it would have shown
    # without codes every finite plan counts
    free = M.mpc_audit_device(variant, K, tf, 0.3, plans)
    assert free["skipped"] == 1 and np.array_equal(free["ival_max"], np.delete(errs, 20, axis=0).max(axis=0)) and np.array_equal(free["errs"], errs, equal_nan=True)


@pytest.mark.parametrize("variant,K,tf", [(6, 8, 2.0), (6, 50, 5.0), (13, 8, 2.0)])
def test_after_a_real_tick_far_starts_have_larger_errors_than_starts_on_the_trajectory(variant, K, tf):
    """MPC::dyn_error(t) of the host front after operator(): the plan solves the dynamics linearised around the desired
    trajectory, so an agent started on it is audited far better than one started away from it"""
    nx = 6 if variant == 6 else 12
    far = np.zeros(nx)
    far[:3] = [0.9, -0.7, 0.8]
    near_e, near_code = M.mpc_tick_dyn_error_host(variant, K, tf, 0.3, np.zeros(nx))
    far_e, far_code = M.mpc_tick_dyn_error_host(variant, K, tf, 0.3, far)
    print("variant %d K %d: near %.3e (code %d)  far %.3e (code %d)" % (variant, K, near_e.max(), near_code, far_e.max(), far_code))
    assert {near_code, far_code} <= {OPTIMAL, MAX_ITERATIONS, MAX_TIME}
    assert np.all(np.isfinite(near_e)) and np.all(np.isfinite(far_e))
    assert far_e.max() >= 10.0 * near_e.max()


@pytest.mark.parametrize("variant,K,tf,B", [(6, 8, 2.0, 70), (6, 50, 5.0, 70), (13, 8, 2.0, 33)])
def test_swarm_audit_after_a_real_tick(variant, K, tf, B):
    """MPCSwarmDeviceLin::audit() on the swarm's own solution: equal to MPC::dyn_error of the host front on the downloaded
    primal for every agent, summaries consistent, far starts audited worse than starts on the trajectory, and the next
    step() does not notice the audit"""
    nx = 6 if variant == 6 else 12
    t = 0.025 * np.arange(B)
    far = np.arange(B) % 2 == 1
    dx0 = np.zeros((B, nx))
    dx0[far, :3] = np.array([0.9, -0.7, 0.8]) * (1.0 + 0.004 * np.arange(B)[far, None])
    got = M.mpc_swarm_devlin_audit(variant, K, tf, t, dx0, audit=True, target=1e-3)
    kept = np.isin(got["code"], [OPTIMAL, MAX_ITERATIONS, MAX_TIME])
    assert kept.all(), got["code"]
    host = M.mpc_dyn_error_host(variant, K, tf, t, got["primal"])
    worst = max(G.check("audit", got["errs"][b], host[b], "variant %d K %d swarm agent %d against the host front" % (variant, K, b)) for b in range(B))
    print("worst agent: %.2e" % worst)
    assert np.array_equal(got["agent_max"], got["errs"].max(axis=1)) and np.array_equal(got["ival_max"], got["errs"].max(axis=0)) and got["skipped"] == 0
    print("agent_max: on the trajectory <= %.3e, away from it >= %.3e" % (got["agent_max"][~far].max(), got["agent_max"][far].min()))
    assert got["agent_max"][far].min() > got["agent_max"][~far].max()
    nivals = -(-K // 4)
    assert got["refined_ivals"] >= nivals and (got["refined_ivals"] > nivals) == bool((got["ival_max"] > 1e-3).any())
    plain = M.mpc_swarm_devlin_audit(variant, K, tf, t, dx0, audit=False)
    assert np.array_equal(plain["primal"], got["primal"]) and np.array_equal(plain["code"], got["code"])
    assert np.array_equal(plain["u_next"], got["u_next"])
