"""SE(3) in include/smooth_feedback_amd/lie.hpp -- SE3 itself and X12B = Bundle<SE3, Rn<6>>, the state of
examples/rigid_body_model.h -- against tests/golden/lie_se3_reference.npz: 60-digit values computed from the 4x4 homogeneous
matrix group (tests/golden/make_golden_lie_se3.py), in the input classes of tests/test_lie_host.py (random tangents, a sweep
of the rotation angle across every series / closed-form switch, angle 0, angles next to pi, the w < 0 branch of the
logarithm, rotations by exactly pi, translations of 1e-6 and 1e6).  Host code, no GPU; tests/test_lie_se3_gpu.py runs the
same functions in device code against the same gates.  Also here: the C-ABI's layout checks for an SFB_LIE_SE3 part.

Tolerance: the rule of tests/test_lie_host.py, unchanged.  tests/lie_ref_se3.py holds a plain float64 transcription of the
textbook closed forms, independent of lie.hpp (dr_expinv in powers of ad there, in block form in lie.hpp).  Its worst error
against the 60-digit values (scaled as lie_ref_se3.scaled_error scales: 1 + |value| per quantity, translation apart from
rotation, each bundle part apart from the others) is what float64 delivers; the gate is FOUR times that, and never looser
than CAP = 1e-12.  Measured on the CPU this was written on:"""
import ctypes as C
import os

import numpy as np
import pytest

import lie_ref_se3 as LR
from examples import models_lib as M

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lie_se3_reference.npz")
CAP = 1e-12
MARGIN = 4.0
# worst scaled error of the float64 transcription per "<group>.<operation>"; the gate is MARGIN times it.
# 0: the operation is exact in float64 (ad copies entries) and must be reproduced exactly.
MEASURED = {
    "SE3.ad": 0.00e+00,              # gate 0.00e+00
    "SE3.dr_expinv": 2.89e-16,       # gate 1.16e-15
    "SE3.exp": 2.56e-16,             # gate 1.02e-15
    "SE3.log": 2.45e-16,             # gate 9.80e-16
    "SE3.mul": 9.95e-16,             # gate 3.98e-15
    "SE3.rminus": 3.91e-16,          # gate 1.56e-15
    "SE3.rminus_rplus": 5.24e-16,    # gate 2.10e-15
    "SE3.rplus": 3.95e-16,           # gate 1.58e-15
    "X12B.ad": 0.00e+00,             # gate 0.00e+00
    "X12B.dr_expinv": 2.02e-16,      # gate 8.08e-16
    "X12B.rminus": 3.41e-16,         # gate 1.36e-15
    "X12B.rminus_rplus": 4.58e-16,   # gate 1.83e-15
    "X12B.rplus": 3.95e-16,          # gate 1.58e-15
}
# lie.hpp on the host, worst scaled errors when this was written: dr_expinv 5.0e-16, mul 1.5e-15 (|p| = 1e6), everything else
# below 7e-16; every entry within 2.0 times the transcription's error.  A finding on the way: with the k(th) of SE2 / SO3
# (closed form from th^2 = 0.16 on) SE3::dr_expinv was at 1.0e-15, 3.6 times the transcription: in SE(3) k multiplies
# W V + V W, of size th |v|, where SE2 and SO3 only have W^2 -- hence detail::dr_expinv_coef_wide.


def load():
    fx = np.load(FIXTURE)
    keys = sorted(k[:-3] for k in fx.files if k.endswith(".in"))
    return fx, keys


def gate(key):
    return min(MARGIN * MEASURED[key], CAP)


def check(key, fx, evaluate, who):
    """errors per input class, printed; every class within the gate"""
    group, op = key.split(".")
    got = evaluate(group, op, fx[key + ".in"])
    err = LR.scaled_error(group, op, got, fx[key + ".out"])
    classes = LR.per_class(err, fx[key + ".cls"], fx["classes"])
    print("%-18s %-14s gate %.3g  worst %.3g  %s" % (key, who, gate(key), err.max(), "  ".join("%s %.2g" % kv for kv in sorted(classes.items()))))
    bad = {c: e for c, e in classes.items() if not e <= gate(key)}
    assert not bad, "%s (%s): classes over the gate %.3g: %s" % (key, who, gate(key), bad)
    return err


_FX, _KEYS = load()


def test_fixture_covers_every_group_and_operation():
    assert set(_KEYS) == set(MEASURED)
    for group in LR.GROUP_PARTS:
        for op in LR.OPS:
            key = "%s.%s" % (group, op)
            assert (LR.widths(group, op) is not None) == (key in _KEYS), key
            assert M.lie_eval_widths(group, op) == LR.widths(group, op), key
    names = set(_FX["classes"][np.unique(np.concatenate([_FX[k + ".cls"] for k in _KEYS]))])
    assert names == {"random_1p5", "random_3", "sweep", "theta0", "near_pi", "trans_1e-6", "trans_1e6", "w_negative", "pi_exact"}
    assert os.path.getsize(FIXTURE) < 512 * 1024


def test_sweep_crosses_every_switch():
    """the switches of lie.hpp's SE(3) code (th^2 = 1e-10 and 1e-8 next to 0/0, 0.16, 0.5, 2.0, 2.25) and of the transcription
    (1e-8, 0.19, 0.6, 2.0) each have sweep angles on both sides, in every operation that takes a tangent"""
    for key in ("SE3.exp", "SE3.dr_expinv", "SE3.rplus", "X12B.dr_expinv"):
        inp = _FX[key + ".in"][_FX[key + ".cls"] == list(_FX["classes"]).index("sweep")]
        w = inp[:, 3:6] if key.endswith(("exp", "dr_expinv")) else inp[:, -6 if key.startswith("SE3") else -12:][:, 3:6]
        t = np.sum(w * w, axis=1)
        for s in (1e-10, 1e-8, 0.16, 0.19, 0.5, 0.6, 2.0, 2.25):
            assert (t < s).any() and (t > s).any(), (key, s)


@pytest.mark.parametrize("key", _KEYS)
def test_transcription_is_as_accurate_as_recorded(key):
    """the table above is what the independent transcription really delivers (within the same margin), and no gate is
    looser than the cap"""
    check(key, _FX, LR.transcription, "transcription")
    assert MARGIN * MEASURED[key] <= CAP


@pytest.mark.parametrize("key", _KEYS)
def test_lie_hpp_on_the_host(key):
    check(key, _FX, lambda g, op, x: M.lie_eval(g, op, x), "lie.hpp host")


def test_batch_entry_point_is_item_by_item():
    for key in ("SE3.mul", "SE3.rminus", "X12B.dr_expinv", "X12B.rplus"):
        group, op = key.split(".")
        inp = _FX[key + ".in"][:7]
        whole = M.lie_eval(group, op, inp)
        for i in range(len(inp)):
            assert np.array_equal(M.lie_eval(group, op, inp[i:i + 1])[0], whole[i])


def test_fixture_regenerates():
    """a sample of the fixture, recomputed with mpmath from the generator's own inputs, is the committed fixture"""
    pytest.importorskip("mpmath")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_lie_se3", os.path.join(os.path.dirname(FIXTURE), "make_golden_lie_se3.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    sample = gen.sample(every=40)
    assert set(sample) == set(_KEYS)
    for key, (idx, inp, out) in sample.items():
        assert np.array_equal(_FX[key + ".in"][idx], inp), key
        assert np.array_equal(_FX[key + ".out"][idx], out), key


# ---- the small components of SE3::exp / log at small angles, component by component ----
# For a = (v, th e_k) the translation is  p = v + B th (e_k x v) + C th^2 e_k x (e_k x v)  with B th = (1 - cos th) / th and
# C th^2 = 1 - sin th / th: the component along e_k x v is 1e-6 of |v| at th = 1e-5 and would hide behind one scale per
# quantity.  Reference: the Taylor series of sin and cos in exact rational arithmetic (|th| <= 1e-2: twelve terms leave 1e-60).
# Measured with the transcription: exp, relative to each non-zero component, 2.2e-16; log of those poses back to v, relative
# to |v|, 1.5e-16; gates four times that.
SMALL_MEASURED = {"exp": 2.2e-16, "log": 1.5e-16}


def _small_angle_cases():
    from fractions import Fraction
    from math import factorial
    rows, ref, elems = [], [], []
    for k in range(4, 25, 2):
        for sgn in (1.0, -1.0):
            for axis in range(3):
                for v in ((0.0, 1e6, -2e5), (1e6, 0.0, 3.0), (0.5, -3.0, 0.0)):
                    th = sgn * 10.0 ** (-k / 2.0)
                    t = Fraction(th)
                    Bt = sum(Fraction((-1) ** n, factorial(2 * n + 2)) * t ** (2 * n + 1) for n in range(12))        # (1 - cos t) / t
                    Ct2 = sum(Fraction((-1) ** (n + 1), factorial(2 * n + 1)) * t ** (2 * n) for n in range(1, 12))  # 1 - sin t / t
                    vv = [Fraction(x) for x in np.roll(v, axis)]
                    e = [Fraction(int(i == axis)) for i in range(3)]
                    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
                    ev = cross(e, vv)
                    eev = cross(e, ev)
                    p = [float(vv[i] + Bt * ev[i] + Ct2 * eev[i]) for i in range(3)]
                    w = [th * float(x) for x in e]
                    rows.append([float(x) for x in vv] + w)
                    ref.append(p)
                    q = [np.cos(0.5 * th)] + [np.sin(0.5 * th) * float(x) for x in e]
                    elems.append(p + q)
    return np.array(rows), np.array(ref), np.array(elems)


@pytest.mark.parametrize("who", ["transcription", "lie.hpp host"])
def test_small_components_of_se3_exp_and_log(who):
    ev = LR.transcription if who == "transcription" else (lambda g, op, x: M.lie_eval(g, op, x))
    rows, ref, elems = _small_angle_cases()
    got = ev("SE3", "exp", rows)[:, :3]
    nz = ref != 0.0
    assert np.array_equal(got[~nz], ref[~nz])
    e_exp = np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))
    # log of the exact pose rounded to doubles: its translation part is v again
    big = np.abs(rows[:, :3]).max(axis=1, keepdims=True)
    e_log = np.max(np.abs(ev("SE3", "log", elems)[:, :3] - rows[:, :3]) / big)
    print("%s: small-angle SE3 exp component-wise %.3g (gate %.3g), log %.3g (gate %.3g)"
          % (who, e_exp, MARGIN * SMALL_MEASURED["exp"], e_log, MARGIN * SMALL_MEASURED["log"]))
    assert e_exp <= MARGIN * SMALL_MEASURED["exp"] and e_log <= MARGIN * SMALL_MEASURED["log"]


# ---- the C-ABI's layout checks for an SE(3) part (no device needed) ----
def _layout(sfb, parts, nx=12, nu=6, ncr=6, kmesh=4, nivals=2):
    return sfb.MPCLayout(nx, nu, ncr, kmesh, nivals, 5.0, np.full(nivals, float(nivals)), np.ones((kmesh + 1, kmesh)), parts=parts,
                         crl=-np.ones(ncr), cru=np.ones(ncr))


def test_layout_with_an_se3_part():
    import smooth_feedback_amd as sfb
    assert sfb.mpc.LIE_SE3 == 3
    L = _layout(sfb, [(sfb.mpc.LIE_SE3, 6), (sfb.LIE_RN, 6)])
    N, nx, nu, ncr = 8, 12, 6, 6
    assert L.record_doubles() == N * (2 * nx + nx * nx + nx * nu) + N * (ncr + ncr * nx + ncr * nu) + nx + nx * nx
    assert L.nnzA == N * nx * (4 + nx + nu) + N * ncr * (nx + nu) + nx * nx
    # the largest state the kernel takes: SE3 x SE3 x SE3 x SE3 (nx = 24, ad codes up to +-24 in an int8_t)
    L24 = _layout(sfb, [(3, 6)] * 4, nx=24)
    assert L24.record_doubles() > 0 and L24.nnzA > 0
    # the front's own layout of the rigid-body model names the same parts
    Lm = M.mpc_layout(13, 8)
    assert [(int(k), int(d)) for k, d in zip(Lm.kind, Lm.dof)] == [(3, 6), (0, 6)]
    assert (Lm.nx, Lm.nu, Lm.ncr, Lm.kmesh, Lm.nivals) == (12, 6, 6, 4, 2)
    assert Lm.record_doubles() == L.record_doubles() and Lm.nnzA == L.nnzA


@pytest.mark.parametrize("dof", [3, 5, 7, 12])
def test_se3_part_with_another_dof_is_an_invalid_argument(dof):
    import smooth_feedback_amd as sfb
    from smooth_feedback_amd import _capi
    good = _layout(sfb, [(3, 6), (0, 6)])
    bad = _layout(sfb, [(3, dof), (0, 12 - dof)] if dof < 12 else [(3, 12)])
    # sfb_mpc_assemble_batch checks the layout before it looks for a device: batch 0, no buffers
    call = lambda L: _capi.lib.sfb_mpc_assemble_batch(C.byref(L.c), 0, None, None, None, None, None, None)
    assert call(bad) == _capi.SFB_ERR_INVALID_ARG
    assert b"dof" in _capi.lib.sfb_last_error()
    assert call(good) in (_capi.SFB_OK, _capi.SFB_ERR_NO_DEVICE)
    assert bad_record_doubles(bad) == -1


def bad_record_doubles(L):
    from smooth_feedback_amd import _capi
    return _capi.lib.sfb_mpc_record_doubles(C.byref(L.c), 0)
