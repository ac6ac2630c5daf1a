"""Every operation of include/smooth_feedback_amd/lie.hpp, for every group the fronts use (R3, SE2, SO3, X6 = Bundle<SE2,R3>,
X12 = Bundle<SE2,R3,SE2,R3>), against tests/golden/lie_reference.npz: 60-digit values computed from the matrix groups
(tests/golden/make_golden_lie.py), at random tangents, angle sweeps across the series / closed-form switches, angle 0, angles
next to pi, the w < 0 branch of SO3::log, rotations by exactly pi and translations of 1e-6 and 1e6.  Host code, no GPU;
tests/test_lie_gpu.py runs the same functions in device code against the same gates.

Tolerance.  tests/lie_ref.py holds a plain float64 transcription of the textbook closed forms, independent of lie.hpp.  Its
worst error against the 60-digit values (scaled as lie_ref.scaled_error scales, 1 + |value| per quantity) is what float64
delivers for an operation; the gate is FOUR times that (another libm, another summation order).  Independent of it no
operation may be off by more than CAP = 1e-12 (1 + |value|), the tolerance the MPC records built from these operations are
held to (REC_TOL, tests/test_mpc_devlin_gpu.py).  Measured on the CPU this was written on:"""
import os

import numpy as np
import pytest

import lie_ref as LR
from examples import models_lib as M

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lie_reference.npz")
CAP = 1e-12
MARGIN = 4.0
# worst scaled error of the float64 transcription per "<group>.<operation>"; the gate is MARGIN times it.
# 0: the operation is exact in float64 (ad copies entries; R^3 adds once) and must be reproduced exactly.
MEASURED = {
    "R3.ad": 0.00e+00,               # gate 0.00e+00
    "R3.dr_expinv": 0.00e+00,        # gate 0.00e+00
    "R3.rminus": 0.00e+00,           # gate 0.00e+00
    "R3.rminus_rplus": 0.00e+00,     # gate 0.00e+00
    "R3.rplus": 0.00e+00,            # gate 0.00e+00
    "SE2.ad": 0.00e+00,              # gate 0.00e+00
    "SE2.dr_expinv": 2.06e-16,       # gate 8.23e-16
    "SE2.exp": 2.11e-16,             # gate 8.45e-16
    "SE2.log": 2.48e-16,             # gate 9.94e-16
    "SE2.mul": 3.81e-16,             # gate 1.52e-15
    "SE2.rminus": 4.01e-16,          # gate 1.60e-15
    "SE2.rminus_rplus": 8.02e-16,    # gate 3.21e-15
    "SE2.rplus": 2.54e-16,           # gate 1.02e-15
    "SO3.ad": 0.00e+00,              # gate 0.00e+00
    "SO3.dr_expinv": 1.59e-16,       # gate 6.36e-16
    "SO3.exp": 1.26e-16,             # gate 5.05e-16
    "SO3.log": 1.48e-16,             # gate 5.92e-16
    "SO3.mul": 6.92e-17,             # gate 2.77e-16
    "SO3.rminus": 1.92e-16,          # gate 7.69e-16
    "SO3.rminus_rplus": 2.28e-16,    # gate 9.14e-16
    "SO3.rplus": 1.40e-16,           # gate 5.62e-16
    "X12.ad": 0.00e+00,              # gate 0.00e+00
    "X12.dr_expinv": 2.03e-16,       # gate 8.12e-16
    "X12.rminus": 4.20e-16,          # gate 1.68e-15
    "X12.rminus_rplus": 5.75e-16,    # gate 2.30e-15
    "X12.rplus": 5.71e-16,           # gate 2.29e-15
    "X6.ad": 0.00e+00,               # gate 0.00e+00
    "X6.dr_expinv": 2.03e-16,        # gate 8.12e-16
    "X6.rminus": 3.32e-16,           # gate 1.33e-15
    "X6.rminus_rplus": 4.06e-16,     # gate 1.63e-15
    "X6.rplus": 1.81e-16,            # gate 7.24e-16
}
# Findings of these tests in lie.hpp as it was before them (fixed in the same change; worst scaled errors then):
#   SE2::exp / SE2::log   1.6e-12 (theta = 1e-5, |p| = 1e6): (1 - cos th) / th cancels just above the th^2 < 1e-10 switch
#   SE2 / SO3::dr_expinv  7.9e-09 just above the th^2 < 1e-8 switch (1/th^2 - ... subtracts two numbers of 1e8) and
#                         7.9e-09 at th = pi - 1e-12 ((1 + cos) / sin divides two vanishing numbers)
# Now: every entry within 2.7 times the transcription's error (dr_expinv 5.4e-16, everything else below 8.1e-16).


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
    """sfbx_lie_eval on a batch == on its items one at a time (strides of every width)"""
    for key in ("SE2.mul", "SO3.rminus", "X6.dr_expinv", "X12.rplus", "R3.rminus_rplus"):
        group, op = key.split(".")
        inp = _FX[key + ".in"][:7]
        whole = M.lie_eval(group, op, inp)
        for i in range(len(inp)):
            assert np.array_equal(M.lie_eval(group, op, inp[i:i + 1])[0], whole[i])


def test_fixture_regenerates():
    """a sample of the fixture, recomputed with mpmath from the generator's own inputs, is the committed fixture"""
    pytest.importorskip("mpmath")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_lie", os.path.join(os.path.dirname(FIXTURE), "make_golden_lie.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    sample = gen.sample()
    assert set(sample) == set(_KEYS)
    for key, (idx, inp, out) in sample.items():
        assert np.array_equal(_FX[key + ".in"][idx], inp), key
        assert np.array_equal(_FX[key + ".out"][idx], out), key


# ---- the small component of SE2::exp / log at small angles, component by component ----
# x = -(1 - cos th) / th * vy for a = (0, vy, th) is 1e-6 of y = sin th / th * vy at th = 1e-5; scaled with y (one scale per
# quantity, as above) any error in (1 - cos th) / th below 1e-10 relative would hide.  Reference: the Taylor series of sin and
# cos in exact rational arithmetic (|th| <= 1e-2: twelve terms leave 1e-60).  Measured with the transcription: exp, relative
# to each component, 2.2e-16; log of those elements back to (vx, vy), relative to |v|, 3.0e-16; gates four times that.
SMALL_MEASURED = {"exp": 2.2e-16, "log": 3.0e-16}


def _small_angle_cases():
    from fractions import Fraction
    from math import factorial
    rows, ref_exp = [], []
    for k in range(4, 25):
        for sgn in (1.0, -1.0):
            for v in ((0.0, 1e6), (1e6, 0.0), (0.0, -3.0)):
                th = sgn * 10.0 ** (-k / 2.0)
                t = Fraction(th)
                A = sum(Fraction((-1) ** n, factorial(2 * n + 1)) * t ** (2 * n) for n in range(12))       # sin t / t
                B = sum(Fraction((-1) ** n, factorial(2 * n + 2)) * t ** (2 * n + 1) for n in range(12))   # (1 - cos t) / t
                vx, vy = Fraction(v[0]), Fraction(v[1])
                rows.append([v[0], v[1], th])
                ref_exp.append([float(A * vx - B * vy), float(B * vx + A * vy)])
    return np.array(rows), np.array(ref_exp)


def _componentwise(got, ref):
    return np.max(np.abs(got - ref) / np.abs(ref))


@pytest.mark.parametrize("who", ["transcription", "lie.hpp host"])
def test_small_component_of_se2_exp_and_log(who):
    ev = LR.transcription if who == "transcription" else (lambda g, op, x: M.lie_eval(g, op, x))
    rows, ref = _small_angle_cases()
    e_exp = _componentwise(ev("SE2", "exp", rows)[:, :2], ref)
    # log of the exact element (p, cos th, sin th) rounded to doubles: its translation part is (vx, vy) again
    elem = np.column_stack([ref, np.cos(rows[:, 2]), np.sin(rows[:, 2])])
    big = np.abs(rows[:, :2]).max(axis=1, keepdims=True)
    e_log = np.max(np.abs(ev("SE2", "log", elem)[:, :2] - rows[:, :2]) / big)
    print("%s: small-angle SE2 exp component-wise %.3g (gate %.3g), log %.3g (gate %.3g)"
          % (who, e_exp, MARGIN * SMALL_MEASURED["exp"], e_log, MARGIN * SMALL_MEASURED["log"]))
    assert e_exp <= MARGIN * SMALL_MEASURED["exp"] and e_log <= MARGIN * SMALL_MEASURED["log"]
