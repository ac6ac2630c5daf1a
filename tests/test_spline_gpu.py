"""The batched Lie-group spline kernels (smooth_feedback_amd/csrc/spline.hip through sfb_spline_fit_cubic_batch_host and
sfb_spline_eval_batch_host) against the 60-digit fixture tests/golden/spline_reference.npz, within the gates of
tests/spline_gates.py (four times the float64 restatement's own error per case class).  Batches of 1 and 65 (a wavefront
and a lane in a second block) are the fixture's rows repeated; S = 1 and 3 segments, at most 9 times per agent."""
import ctypes as C

import numpy as np
import pytest

import spline_gates as G

pytestmark = pytest.mark.gpu
GROUP_NAMES = list(G.GROUPS)


def _tile(a, B):
    a = np.asarray(a)
    return a[np.arange(B) % len(a)]


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("S", G.SEGMENTS)
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_fit_and_evaluation_against_the_fixture(sfb, group, S, B):
    d = {k: _tile(v, B) for k, v in G.curve(group, S).items() if k != "umax"}
    V = sfb.spline_fit_cubic_batch_host(G.GROUPS[group], d["tk"], d["gk"])
    G.check("fit", group, [("V", V, d["V"])], d["cls"], "kernel B=%d S=%d" % (B, S))
    got = sfb.spline_eval_batch_host(G.GROUPS[group], d["tk"], d["gk"], d["V"], d["t"])
    G.check("eval", group, G.eval_pairs(d, got), d["cls"], "kernel B=%d S=%d" % (B, S))
    # held pose at rest before the first and after the last knot: exactly
    assert np.array_equal(got[0][:, 0], d["gk"][:, 0]) and np.array_equal(got[0][:, -1], d["gk"][:, -1])
    assert not got[1][:, [0, -1]].any() and not got[2][:, [0, -1]].any()


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_shared_and_per_agent_arguments_agree_bit_for_bit(sfb, group):
    d, B, parts = G.curve(group, 3), 65, G.GROUPS[group]
    rep = lambda a: np.repeat(a[3:4], B, axis=0)                                   # noqa: E731
    t = _tile(d["t"], B)
    per_agent = sfb.spline_eval_batch_host(parts, rep(d["tk"]), rep(d["gk"]), rep(d["V"]), t)
    shared = sfb.spline_eval_batch_host(parts, d["tk"][3], d["gk"][3], d["V"][3], t)
    zeros = sfb.spline_eval_batch_host(parts, d["tk"][3], d["gk"][3], d["V"][3], t, ts0=np.zeros(B))
    one_t = sfb.spline_eval_batch_host(parts, rep(d["tk"]), rep(d["gk"]), rep(d["V"]), d["t"][3])
    one_t_shared = sfb.spline_eval_batch_host(parts, d["tk"][3], d["gk"][3], d["V"][3], d["t"][3], batch=B)
    for a, b, c, e, f in zip(per_agent, shared, zeros, one_t, one_t_shared):
        assert np.array_equal(a, b) and np.array_equal(a, c)                      # one spline for all; a ts0 of zeros is NULL
        assert np.array_equal(e, f) and np.array_equal(e[3], a[3])                 # shared times
    tk = _tile(d["tk"], B)
    assert np.array_equal(sfb.spline_fit_cubic_batch_host(parts, rep(tk), _tile(d["gk"], B)),
                          sfb.spline_fit_cubic_batch_host(parts, d["tk"][3], _tile(d["gk"], B)))
    # a time origin shifts the curve: agent b at t - ts0[b] is the curve at those times
    ts0 = np.linspace(-0.4, 0.4, B)
    shifted = sfb.spline_eval_batch_host(parts, d["tk"][3], d["gk"][3], d["V"][3], t, ts0=ts0)
    direct = sfb.spline_eval_batch_host(parts, d["tk"][3], d["gk"][3], d["V"][3], t - ts0[:, None])
    for a, b in zip(shifted, direct):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_first_row_of_a_batch_of_65_is_the_batch_of_one(sfb, group):
    parts = G.GROUPS[group]
    for S in G.SEGMENTS:
        d = G.curve(group, S)
        one, many = [{k: _tile(d[k], B) for k in ("tk", "gk", "V", "t")} for B in (1, 65)]
        assert np.array_equal(sfb.spline_fit_cubic_batch_host(parts, one["tk"], one["gk"])[0], sfb.spline_fit_cubic_batch_host(parts, many["tk"], many["gk"])[0])
        for a, b in zip(sfb.spline_eval_batch_host(parts, one["tk"], one["gk"], one["V"], one["t"]),
                        sfb.spline_eval_batch_host(parts, many["tk"], many["gk"], many["V"], many["t"])):
            assert np.array_equal(a[0], b[0])


def test_no_times_write_nothing(sfb):
    d = G.curve("SE3R3", 3)
    grp = sfb.PIDGroup(G.GROUPS["SE3R3"])
    B, K = d["tk"].shape
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                          # noqa: E731
    tk, gk, V, t = [np.ascontiguousarray(d[k]) for k in ("tk", "gk", "V", "t")]
    g, vel, acc = np.full((B, 1, grp.elem), 7.0), np.full((B, 1, grp.dof), 7.0), np.full((B, 1, grp.dof), 7.0)
    rc = sfb._capi.lib.sfb_spline_eval_batch_host(C.byref(grp.c), B, K, p(tk), p(gk), p(V), 0, None, 0, p(t), 0, p(g), p(vel), p(acc))
    assert rc == sfb._capi.SFB_OK and np.all(g == 7.0) and np.all(vel == 7.0) and np.all(acc == 7.0)


@pytest.mark.parametrize("cls", ["generic", "abelian"])
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_the_kernels_fit_fed_to_the_kernels_evaluation_reproduces_the_knots(sfb, group, cls):
    parts, S = G.GROUPS[group], 3
    d = G.curve(group, S)
    m = d["cls"] == G.CLASSES.index(cls)
    tk, gk = _tile(d["tk"][m], 65), _tile(d["gk"][m], 65)
    V = sfb.spline_fit_cubic_batch_host(parts, tk, gk)
    t = np.concatenate([tk, np.nextafter(tk[:, 1:], -np.inf)], axis=1)             # every knot from its segment, and from the one before
    g, vel, _ = sfb.spline_eval_batch_host(parts, tk, gk, V, t)
    cl = np.full(65, G.CLASSES.index(cls))
    G.check("eval", group, [("g", g[:, :S + 1], gk)], cl, "fit -> eval, at the knots")
    G.check("eval", group, [("g", g[:, S + 1:], gk[:, 1:])], cl, "fit -> eval, segment ends")
    G.check("eval", group, [("vel", vel[:, S + 1:2 * S], vel[:, 1:S])], cl, "fit -> eval, one-sided velocities")
