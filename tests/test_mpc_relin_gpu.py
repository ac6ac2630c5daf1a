"""Sequential convex MPC on the GPU (include/smooth_feedback_amd/mpc_device.hpp: mpc_relinearise_kernel and
MPCSwarmDeviceLin::step(.., passes) -> sfb_mpc_swarm_step_resident_flat) for the planar vehicle on the smallest transcription
with two mesh intervals (K = 8, Kmesh = 4), batches 1, 3 and 67 (less than a wave of (agent, node) lanes, a partly filled block,
several blocks), every agent with its own state and time: the leading agents of tests/golden/mpc_relin_reference.npz.
Against MPC::fill_flat_record and the host path (MPC::operator() with MPCParams::relin_passes), and for the audit against the
numpy restatement's errors in the fixture.  Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_relin_gates as G  # noqa: E402
import mpc_relin_ref as Q  # noqa: E402
from examples import models_lib as M  # noqa: E402
from examples import mpc_relin_lib as RL  # noqa: E402

pytestmark = pytest.mark.gpu
FX = G.fixture()
K, TF = FX["K"], FX["tf"]
BATCHES = [1, 3, 67]


@functools.lru_cache(maxsize=None)
def device(B, passes, prune=0):
    return RL.swarm(K, TF, FX["t"][:B], FX["dx0"][:B], passes, prune=prune, want_Ax=prune == 1)


@functools.lru_cache(maxsize=None)
def host(B, passes):
    return RL.tick_host(G.VARIANT, K, TF, FX["t"][:B], FX["dx0"][:B], passes)


@pytest.mark.parametrize("B", BATCHES)
def test_kernel_records_equal_fill_flat_record(B):
    """the flat records the kernel writes about the swarm's own pass-one plans, then about given plans with rotation parts up
    to 1 rad and an agent whose code the swarm does not keep (re-linearised about e = v = 0), entry by entry"""
    t, dx0 = FX["t"][:B], FX["dx0"][:B]
    own = RL.kernel(K, TF, t, dx0)
    assert np.all(np.isin(own["code"], G.KEPT))
    want = RL.flat_records(G.VARIANT, K, TF, t, dx0, own["plan"])
    err = np.max(np.abs(own["rec"] - want))
    print("B %d: own plans %.2e" % (B, err))
    assert err <= G.REC_TOL
    assert np.max(np.abs(want - RL.flat_records(G.VARIANT, K, TF, t, dx0))) > 1e-3      # ... and the plans are not zero
    n = own["plan"].shape[1]
    rng = np.random.default_rng(11 + B)
    plan = rng.uniform(-0.3, 0.3, (B, n))
    N = M.mpc_dims(G.VARIANT, K)["N"]
    for i in range(N + 1):
        plan[:, i * Q.NX + 2] = np.resize([1.0, -0.3, 1e-9], B) * (1 if i % 2 else -1)
    code = np.resize(np.array([0, 4, 5, 0, 2, 0, 1], np.int32), B)
    if B == 1:
        code[:] = 2
    given = RL.kernel(K, TF, t, dx0, plan=plan, code=code)
    assert np.array_equal(given["plan"], plan) and np.array_equal(given["code"], code)
    eff = np.where(np.isin(code, G.KEPT)[:, None], plan, 0.0)
    want = RL.flat_records(G.VARIANT, K, TF, t, dx0, eff)
    err = np.max(np.abs(given["rec"] - want))
    print("B %d: given plans %.2e" % (B, err))
    assert err <= G.REC_TOL


@pytest.mark.parametrize("B", BATCHES)
def test_no_pass_gives_the_bits_of_todays_step(B):
    today = M.mpc_swarm_devlin_audit(G.VARIANT, K, TF, FX["t"][:B], FX["dx0"][:B], audit=False)
    got = device(B, 0)
    assert np.array_equal(got["primal"], today["primal"]) and np.array_equal(got["code"], today["code"])
    assert np.array_equal(host(B, 0)["code"], got["code"])


@pytest.mark.parametrize("B", BATCHES)
def test_device_path_equals_host_path(B):
    dev, ref = device(B, 2), host(B, 2)
    assert np.array_equal(dev["code"], ref["code"]) and np.all(np.isin(dev["code"], G.KEPT))
    err, eu = np.max(np.abs(dev["primal"] - ref["primal"])), np.max(np.abs(dev["u0"] - ref["u0"]))
    print("B %d: primal %.2e u0 %.2e (gate %.0e); moved by the passes %.2e" % (B, err, eu, G.U_TOL, np.max(np.abs(dev["primal"] - device(B, 0)["primal"]))))
    assert err <= G.U_TOL and eu <= G.U_TOL
    assert np.max(np.abs(dev["primal"] - device(B, 0)["primal"])) > 1e-3          # the passes did act


def test_agents_on_the_trajectory_keep_their_plan():
    """agents that start on the desired trajectory stay near it (the plan gives way to the drag by 0.16 in the velocities,
    by 0.12 in the pose), where the pass-one linearisation is already good: a pass moves the plan by no more than the QP
    tolerance (the restatement: 8.6e-4 at the first pass, 2.3e-6 at the second)"""
    t, dx0 = FX["t"][:3], np.zeros((3, Q.NX))
    p = [RL.swarm(K, TF, t, dx0, k)["primal"] for k in range(3)]
    d1, d2 = np.max(np.abs(p[1] - p[0])), np.max(np.abs(p[2] - p[1]))
    print("plan moved by %.2e at the first pass, %.2e at the second (QP tolerance %.0e)" % (d1, d2, G.QP_EPS))
    assert d1 <= G.QP_EPS and d2 <= G.QP_EPS


def test_the_audit_falls_as_in_the_restatement():
    """heading errors up to 1 rad: the dynamics error of the GPU's plans after 0, 1, 2 passes within a factor of the
    restatement's (tests/mpc_relin_gates.py: four times the worst ratio host path / restatement, printed here), and no agent's
    error grows from pass 0 to pass 2"""
    B = 67
    ref = FX["agent_max"]
    dev = np.stack([device(B, p)["agent_max"] for p in range(3)])
    hst = np.stack([host(B, p)["agent_max"] for p in range(3)])
    ratio = lambda a: np.maximum(a / ref, ref / a)                                  # noqa: E731
    for p in range(3):
        print("pass %d: restatement worst %.3e median %.3e | host path ratio %.3f | device ratio %.3f" %
              (p, ref[p].max(), np.median(ref[p]), ratio(hst)[p].max(), ratio(dev)[p].max()))
    print("AUDIT_FACTOR_MEASURED = %.4f" % ratio(hst).max())
    gate = G.audit_factor()
    assert np.all(np.isfinite(dev)) and ratio(dev).max() <= gate, (ratio(dev).max(), gate)
    assert np.all(dev[2] <= dev[0])
    assert np.median(dev[1]) < 0.2 * np.median(dev[0])                              # ... and the first pass pays: the linearisation error goes


def test_side_stream_and_memory():
    B = 67
    r = RL.kernel(K, TF, FX["t"][:B], FX["dx0"][:B], side=True)
    assert np.all(np.isfinite(r["rec_side"])) and np.array_equal(r["rec"], r["rec_side"])
    two = RL.swarm(K, TF, FX["t"][:B], FX["dx0"][:B], 2, ticks=2)
    assert two["free_before"] == two["free_after"], (two["free_before"], two["free_after"])
    assert np.all(np.isin(two["code"], G.KEPT))


def test_sharded_swarm_forwards_the_passes():
    """MPCSwarmMultiDeviceLin::step(.., passes): two shards (on the one device) give what the one swarm gives"""
    B = 67
    one, two = device(B, 2), RL.swarm_multi(K, TF, FX["t"][:B], FX["dx0"][:B], 2, [0, 0])
    assert np.array_equal(two["code"], one["code"]) and np.array_equal(two["iter"], one["iter"])
    assert np.max(np.abs(two["u0"] - one["u0"])) <= G.U_TOL


def test_argument_errors_on_a_live_swarm(sfb):
    r = RL.kernel(K, TF, FX["t"][:3], FX["dx0"][:3], want_status=True)
    assert list(r["status"]) == [sfb._capi.SFB_ERR_INVALID_ARG] * 3


def test_pruned_plan_of_probe_relin():
    B = 67
    kd, kr = RL.probe(G.VARIANT, K, TF)
    pr, whole, today = device(B, 2, 1), device(B, 2, 2), device(B, 2, 0)
    assert pr["nnzA_kept"] == kr.sum() < pr["nnzA"] and today["nnzA_kept"] == kd.sum() and whole["nnzA_kept"] == whole["nnzA"]
    assert np.all(kr[np.any(pr["Ax"] != 0.0, axis=0)])                              # the last pass stayed inside the mask: no fallback
    for name, r in (("probe_relin", pr), ("today's probe (every pass on the fallback)", today)):
        err = np.max(np.abs(r["primal"] - whole["primal"]))
        print("%s: %.2e (gate %.0e)" % (name, err, G.PRUNED_TOL))
        assert np.array_equal(r["code"], whole["code"]) and err <= G.PRUNED_TOL
