"""The batched Lie-group PID kernels (smooth_feedback_amd/csrc/pid.hip through sfb_pid_step_batch_host and
sfb_pid_rollout_batch_host) against the 60-digit fixture tests/golden/pid_reference.npz, within the gates of
tests/pid_gates.py (four times the float64 restatement's own error per case class).  Batches of 1, 65 (a wavefront and a
lane) and 1000 are the fixture's rows repeated."""
import numpy as np
import pytest

import pid_gates as G
from examples import models_lib as M

pytestmark = pytest.mark.gpu
GROUP_NAMES = list(G.GROUPS)


def _tile(a, B):
    a = np.asarray(a)
    return a[np.arange(B) % len(a)]


def _step(sfb, group, d, B, windup, rows=None, **over):
    """the step section's rows repeated to a batch of B (or the given rows) through the kernel"""
    a = {k: (_tile(v, B) if rows is None else v[rows]) for k, v in d.items()}
    a.update(over)
    return sfb.pid_step_batch_host(G.GROUPS[group], G.T_STEP, a["x"], a["v"], a["gd"], a["vd"], a["ad"], a["kp"], a["kd"], a["ki"], a["ie"],
                                   a["t_last"], windup_limit=windup)


@pytest.mark.parametrize("B", [1, 65, 1000])
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_step_against_the_fixture(sfb, group, B):
    d = G.section("step", group)
    n = len(d["cls"])
    for tag, W in (("w", G.WINDUP), ("inf", np.inf)):
        u, ie, tl = _step(sfb, group, d, B, W)
        assert np.all(tl == G.T_STEP)                                     # t_last = t, always
        G.check("step", group, [("u", u, _tile(d["u_" + tag], B)), ("ie", ie, _tile(d["ie_" + tag], B))], _tile(d["cls"], B),
                "kernel B=%d windup %s" % (B, tag))
        no_int = ~(_tile(d["t_last"], B) < G.T_STEP)                      # unset, equal, later: the integral is untouched, bit for bit
        assert np.array_equal(ie[no_int], _tile(d["ie"], B)[no_int])
        if B >= n:                                                        # every t_last kind and class was in the batch
            assert set(np.unique(_tile(d["cls"], B))) == {0, 1, 2} and np.isnan(_tile(d["t_last"], B)).any()


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_shared_and_per_agent_arguments_agree_bit_for_bit(sfb, group):
    d = G.section("step", group)
    B = 65
    one = {k: np.repeat(d[k][3:4], B, axis=0) for k in ("gd", "vd", "ad", "kp", "kd", "ki")}
    per_agent = _step(sfb, group, d, B, G.WINDUP, **one)
    a = {k: _tile(v, B) for k, v in d.items()}
    shared = sfb.pid_step_batch_host(G.GROUPS[group], G.T_STEP, a["x"], a["v"], d["gd"][3], d["vd"][3], d["ad"][3], d["kp"][3], d["kd"][3],
                                     d["ki"][3], a["ie"], a["t_last"], windup_limit=G.WINDUP)
    for p, s in zip(per_agent, shared):
        assert np.array_equal(p, s)
    r = G.section("roll", group)
    ra = {k: _tile(v, B) for k, v in r.items() if k != "umax"}
    kw = dict(windup_limit=G.WINDUP, u_max=r["umax"])
    per_agent = sfb.pid_rollout_batch_host(G.GROUPS[group], G.T0, G.DT, 7, ra["x"], ra["v"], np.repeat(r["g0"][1:2], B, 0), np.repeat(r["w"][1:2], B, 0),
                                           np.repeat(r["kp"][1:2], B, 0), np.repeat(r["kd"][1:2], B, 0), np.repeat(r["ki"][1:2], B, 0), ra["ie"],
                                           ra["t_last"], **kw)
    shared = sfb.pid_rollout_batch_host(G.GROUPS[group], G.T0, G.DT, 7, ra["x"], ra["v"], r["g0"][1], r["w"][1], r["kp"][1], r["kd"][1], r["ki"][1],
                                        ra["ie"], ra["t_last"], **kw)
    for k in per_agent:
        assert np.array_equal(per_agent[k], shared[k], equal_nan=True), k


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_two_successive_step_calls_are_the_host_fronts_two_calls(sfb, group):
    d = G.section("seq", group)
    n = len(d["cls"])
    ie, tl, us, ies = np.zeros_like(d["kp"]), np.full(n, np.nan), [], []
    for k in range(2):
        u, ie, tl = sfb.pid_step_batch_host(G.GROUPS[group], G.SEQ_TIMES[k], d["x"][:, k], d["v"][:, k], d["gd"][:, k], d["vd"][:, k], d["ad"][:, k],
                                            d["kp"], d["kd"], d["ki"], ie, tl, windup_limit=G.WINDUP)
        us.append(u); ies.append(ie)
    u, ie = np.stack(us, 1), np.stack(ies, 1)
    G.check("seq", group, [("u", u, d["u"][:, :2]), ("ie", ie, d["ie"][:, :2])], d["cls"], "kernel, two calls")
    hu, hie = M.pid_host(group, G.SEQ_TIMES[:2], d["x"][:, :2], d["v"][:, :2], d["gd"][:, :2], d["vd"][:, :2], d["ad"][:, :2], d["kp"], d["kd"], d["ki"],
                         G.WINDUP)
    G.check("seq", group, [("u", hu, d["u"][:, :2]), ("ie", hie, d["ie"][:, :2])], d["cls"], "host front, two calls")


def _rollout(sfb, group, r, B, steps, clamp):
    a = {k: _tile(v, B) for k, v in r.items() if k != "umax"}
    return sfb.pid_rollout_batch_host(G.GROUPS[group], G.T0, G.DT, steps, a["x"], a["v"], a["g0"], a["w"], a["kp"], a["kd"], a["ki"], a["ie"],
                                      a["t_last"], windup_limit=G.WINDUP, u_max=r["umax"] if clamp else None)


@pytest.mark.parametrize("B", [1, 65, 1000])
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_rollout_against_the_fixture(sfb, group, B):
    r = G.section("roll", group)
    for tag, (steps, clamp) in G.ROLL_SETS.items():
        got = _rollout(sfb, group, r, B, steps, clamp)
        assert np.all(got["t_last"] == G.T0 + (steps - 1) * G.DT)
        G.check("roll" + tag, group, [(k, got[g], _tile(r["%s_%s" % (k, tag)], B)) for k, g in
                                     (("x", "x"), ("v", "v"), ("ie", "i_err"), ("u", "u_last"), ("cost", "cost"))], _tile(r["cls"], B),
                "kernel B=%d" % B)


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_rollout_is_forty_steps_and_the_double_integrator(sfb, group):
    """40 launches of the step kernel with the double-integrator step of tests/pid_ref.py (numpy, matrix form) in between
    (pid_gates.stepwise_rollout) against the fixture's 40-tick rollout.  The procedure hands the pose from tick to tick as
    flat doubles, a rounding per tick that the one-launch rollout does not have, so its gate is four times what the float64
    restatement delivers when its own law runs the same procedure (class steps40 of tests/pid_gates.py), not rollB's."""
    def law(parts, t, x, v, gd, vd, ad, kp, kd, ki, ie, tl):
        return sfb.pid_step_batch_host(parts, t, x, v, gd, vd, ad, kp, kd, ki, ie, tl, windup_limit=G.WINDUP)
    cls, pairs = G.stepwise_rollout(group, law)
    G.check("steps40", group, pairs, cls, "40 step launches")


@pytest.mark.parametrize("group", ["SE3R3", "SE2R1"])
def test_zero_steps_leave_everything_untouched(sfb, group):
    r = G.section("roll", group)
    got = _rollout(sfb, group, r, 65, 0, True)
    for k, src in (("x", "x"), ("v", "v"), ("i_err", "ie"), ("t_last", "t_last")):
        assert np.array_equal(got[k], _tile(r[src], 65), equal_nan=True), k


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_first_row_of_a_batch_of_65_is_the_batch_of_one(sfb, group):
    d, r = G.section("step", group), G.section("roll", group)
    for a, b in zip(_step(sfb, group, d, 1, G.WINDUP), _step(sfb, group, d, 65, G.WINDUP)):
        assert np.array_equal(a[0], b[0], equal_nan=True)
    one, many = _rollout(sfb, group, r, 1, 40, True), _rollout(sfb, group, r, 65, 40, True)
    for k in one:
        assert np.array_equal(one[k][0], many[k][0], equal_nan=True), k
