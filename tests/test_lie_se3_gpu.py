"""The SE(3) operations of include/smooth_feedback_amd/lie.hpp evaluated IN DEVICE CODE (sfbx_lie_eval_device,
examples/models_device.hip: one GPU thread per item through the same functions, with the device maths library), against the
60-digit fixture and the gates of tests/test_lie_se3_host.py.  These are the functions the device-side linearisation of the
MPC (mpc_device.hpp) and the EKF (ekf_device.hpp) call for a state on SE(3).  The largest host-vs-device difference per
operation is printed, not asserted.  Needs an MI355X."""
import numpy as np
import pytest

from examples import models_lib as M
from test_lie_se3_host import _FX, _KEYS, check

pytestmark = pytest.mark.gpu

_FULL = {}


def _full(key):
    """the whole fixture of one operation through the device, once"""
    if key not in _FULL:
        group, op = key.split(".")
        _FULL[key] = M.lie_eval(group, op, _FX[key + ".in"], device=True)
    return _FULL[key]


@pytest.mark.parametrize("key", _KEYS)
def test_lie_hpp_on_the_device(key):
    group, op = key.split(".")
    check(key, _FX, lambda g, o, x: _full(key), "lie.hpp device")
    dev, host = _full(key), M.lie_eval(group, op, _FX[key + ".in"])
    print("%-18s host vs device: max |difference| %.3g, %d of %d entries differ" % (key, np.abs(dev - host).max(), (dev != host).sum(), dev.size))


@pytest.mark.parametrize("count", [1, 65])
@pytest.mark.parametrize("key", _KEYS)
def test_ragged_batches_on_the_device(key, count):
    """batches of 1 and 65 (one thread, one wavefront and a thread): the same values as in the full batch, within the gates"""
    group, op = key.split(".")
    inp = np.resize(_FX[key + ".in"], (count, _FX[key + ".in"].shape[1]))      # the first rows, repeated if fewer than 65
    ref = np.resize(_FX[key + ".out"], (count, _FX[key + ".out"].shape[1]))
    sub = {key + ".in": inp, key + ".out": ref, key + ".cls": np.resize(_FX[key + ".cls"], count), "classes": _FX["classes"]}
    got = check(key, sub, lambda g, o, x: M.lie_eval(g, o, x, device=True), "device, batch %d" % count)
    assert len(got) == count
    full = _full(key)
    assert np.array_equal(M.lie_eval(group, op, inp, device=True), np.resize(full, (count, full.shape[1])))
