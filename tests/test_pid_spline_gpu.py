"""The PID rollout along cubic splines (pid_rollout_spline_kernel of smooth_feedback_amd/csrc/spline.hip through
sfb_pid_rollout_spline_batch_host) against the 60-digit fixture tests/golden/spline_reference.npz, within the gates of
tests/spline_gates.py, and against the other kernels: the step kernel fed by the evaluation kernel, and the constant-twist
rollout.  Batches of 1 and 65 are the fixture's rows repeated."""
import numpy as np
import pytest

import pid_gates as PG
import pid_ref as PR
import spline_gates as G

pytestmark = pytest.mark.gpu
GROUP_NAMES = list(G.GROUPS)


def _tile(a, B):
    a = np.asarray(a)
    return a[np.arange(B) % len(a)]


def _rollout(sfb, group, d, B, steps, clamp, **over):
    a = {k: _tile(v, B) for k, v in d.items() if k != "umax"}
    a.update(over)
    return sfb.pid_rollout_spline_batch_host(G.GROUPS[group], G.T0, G.DT, steps, a["x"], a["v"], a["tk"], a["gk"], a["V"], a["kp"], a["kd"], a["ki"],
                                             a["ie"], a["t_last"], ts0=a["ts0"], windup_limit=G.WINDUP, u_max=d["umax"] if clamp else None)


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("S", G.SEGMENTS)
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_rollout_against_the_fixture(sfb, group, S, B):
    d = G.curve(group, S)
    for tag, (steps, clamp) in G.ROLL_SETS.items():
        got = _rollout(sfb, group, d, B, steps, clamp)
        assert np.all(got["t_last"] == G.T0 + (steps - 1) * G.DT)
        G.check("roll" + tag, group, G.roll_pairs({k: _tile(v, B) for k, v in d.items() if k != "umax"}, tag, got), _tile(d["cls"], B),
                "kernel B=%d S=%d" % (B, S))


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_shared_and_per_agent_arguments_agree_bit_for_bit(sfb, group):
    d, B = G.curve(group, 3), 65
    rep = lambda a: np.repeat(a[4:5], B, axis=0)                                   # noqa: E731
    per_agent = _rollout(sfb, group, d, B, 40, True, tk=rep(d["tk"]), gk=rep(d["gk"]), V=rep(d["V"]), ts0=np.zeros(B))
    shared = _rollout(sfb, group, d, B, 40, True, tk=d["tk"][4], gk=d["gk"][4], V=d["V"][4], ts0=np.zeros(B))
    no_ts0 = _rollout(sfb, group, d, B, 40, True, tk=d["tk"][4], gk=d["gk"][4], V=d["V"][4], ts0=None)
    staggered = _rollout(sfb, group, d, B, 40, True, tk=d["tk"][4], gk=d["gk"][4], V=d["V"][4], ts0=np.linspace(-0.3, 0.3, B))
    for k in per_agent:
        assert np.array_equal(per_agent[k], shared[k], equal_nan=True), k
        assert np.array_equal(shared[k], no_ts0[k], equal_nan=True), k             # a ts0 of zeros is NULL
    assert not np.array_equal(staggered["x"], shared["x"])


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_first_row_of_a_batch_of_65_is_the_batch_of_one(sfb, group):
    for S in G.SEGMENTS:
        d = G.curve(group, S)
        one, many = _rollout(sfb, group, d, 1, 40, True), _rollout(sfb, group, d, 65, 40, True)
        for k in one:
            assert np.array_equal(one[k][0], many[k][0], equal_nan=True), k


@pytest.mark.parametrize("group", ["SE3R3", "SE2R1"])
def test_zero_steps_leave_everything_untouched(sfb, group):
    d = G.curve(group, 3)
    got = _rollout(sfb, group, d, 65, 0, True)
    for k, src in (("x", "x"), ("v", "v"), ("i_err", "ie"), ("t_last", "t_last")):
        assert np.array_equal(got[k], _tile(d[src], 65), equal_nan=True), k
    assert not got["u_last"].any() and not got["cost"].any()                       # the wrapper's zeros: nothing was written


@pytest.mark.parametrize("S", G.SEGMENTS)
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_rollout_is_forty_steps_of_the_step_and_evaluation_kernels(sfb, group, S):
    """40 launches of the step kernel, each fed by a launch of the evaluation kernel, with the double-integrator step of
    tests/pid_ref.py (numpy, matrix form) in between (spline_gates.stepwise_rollout) against the fixture's 40-tick rollout.
    The procedure hands the pose from tick to tick as flat doubles, so its gate is four times what the float64 restatement
    delivers when its own law and curve run the same procedure (class steps40 of tests/spline_gates.py)."""
    def law(parts, t, x, v, gd, vd, ad, kp, kd, ki, ie, tl):
        return sfb.pid_step_batch_host(parts, t, x, v, gd, vd, ad, kp, kd, ki, ie, tl, windup_limit=G.WINDUP)

    def evaluate(parts, tk, gk, V, t):
        return sfb.spline_eval_batch_host(parts, tk, gk, V, t)
    cls, pairs = G.stepwise_rollout(group, S, law, evaluate)
    G.check("steps40", group, pairs, cls, "40 eval + step launches S=%d" % S)


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_a_spline_along_a_constant_twist_tracks_like_the_constant_twist_rollout(sfb, group):
    """knots on g0 exp(t w) with v1 = v2 = v3 = h w / 3 on every segment: the spline IS the constant-twist curve (velocity w,
    acceleration 0) between its first and last knot, and the ticks stay inside.  The reference here is the constant-twist
    kernel's own output, so both kernels' errors add up; the rows are the PID fixture's small-error classes."""
    r = PG.section("roll", group)
    parts = G.GROUPS[group]
    m = r["cls"] != PG.CLASSES.index("large")
    r = {k: (v if k == "umax" else v[m]) for k, v in r.items()}
    n = len(r["x"])
    tk = np.array([0.0, 0.7, 1.5, 2.5])
    gk = np.array([[PR.store(parts, PR.rplus(parts, PR.load(parts, g0), t * w)) for t in tk] for g0, w in zip(r["g0"], r["w"])])
    V = np.array([[[h * w / 3.0] * 3 for h in np.diff(tk)] for w in r["w"]])
    for clamp in (False, True):
        kw = dict(windup_limit=PG.WINDUP, u_max=r["umax"] if clamp else None)
        ref = sfb.pid_rollout_batch_host(parts, PG.T0, PG.DT, 40, r["x"], r["v"], r["g0"], r["w"], r["kp"], r["kd"], r["ki"], r["ie"], r["t_last"], **kw)
        got = sfb.pid_rollout_spline_batch_host(parts, PG.T0, PG.DT, 40, r["x"], r["v"], np.tile(tk, (n, 1)), gk, V, r["kp"], r["kd"], r["ki"], r["ie"],
                                                r["t_last"], **kw)
        G.check("rollC" if clamp else "rollB", group, [(k, got[k], ref[k]) for k in ("x", "v", "i_err", "u_last", "cost")],
                np.full(n, G.CLASSES.index("generic")), "spline vs constant twist")
