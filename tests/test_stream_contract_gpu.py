"""The stream contract of every device-pointer entry of include/sfb.h (tests/stream_contract.py has the harness, the case
builders and the case table): on non-blocking side streams, behind a bounded spin, an entry reads its inputs behind the stream,
leaves every output and in-out buffer complete for the next work on the stream, and shares nothing between two caller streams.
The GPU cases need an MI355X; the coverage test runs anywhere."""
import importlib.util
import os

import numpy as np
import pytest

import stream_contract as SC

# Cases whose entry is allowed to return only after its stream has drained: (reason, source line that blocks).  Steps 3 and 4
# run for them all the same.  Empty: every entry of the table returned while the spin still held its stream.
BLOCKING = {}


def test_every_stream_entry_of_the_header_has_a_case():
    """an entry added to sfb.h with a `void *stream` parameter cannot go untested unnoticed"""
    declared = set(SC.header_stream_entries())
    covered = {c.entry for c in SC.CASES.values()}
    assert len(declared) >= 27
    assert declared - covered == set(), "entries of sfb.h that take a stream and have no case: %s" % sorted(declared - covered)
    assert covered <= declared, "cases for entries sfb.h does not declare with a stream: %s" % sorted(covered - declared)
    assert set(BLOCKING) <= set(SC.CASES)
    never = ("sfb_sparse_qp_solve_batch", "sfb_ekf_predict_batch", "sfb_ekf_update_batch", "sfb_ekf_predict_update_batch", "sfb_ekf_predict_stepper_batch",
             "sfb_ekf_predict_rk4_batch")
    for name in BLOCKING:                                                           # the header promises asynchrony for these
        assert SC.CASES[name].entry not in never, name
        assert not (SC.CASES[name].entry == "sfb_qp_dense_solve_batch" and not SC.CASES[name].knobs and "(3,203)" not in name), name


def test_five_knot_gate_is_four_times_the_restatements_error():
    """the spline cases run on five-knot curves with a 60-digit fixture of their own (tests/golden/spline5_reference.npz): prints what
    tests/spline_ref.py delivers against it per class next to the recorded figure the gates are built from; the restatement still
    delivers it (within the same margin, as tests/test_spline_host.py asks of the other fixture), and the fixture's inputs are the
    extension of the four-knot fixture's curves that its generator describes"""
    import spline_gates as G
    spec = importlib.util.spec_from_file_location("make_golden_spline5", os.path.join(os.path.dirname(SC.SPLINE5_FIXTURE), "make_golden_spline5.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d, want = SC._five_knot_curves(), gen.inputs()
    for k, v in want.items():
        assert np.array_equal(d[k], v, equal_nan=True), k
    assert d["tk"].shape[1] == 5 and (np.diff(d["tk"], axis=1) > 0).all()
    worst = SC.spline5_restatement_errors()
    for k in sorted(worst):
        print("%-16s restatement %.2e   recorded %.2e   gate %.2e" % (k, worst[k], SC.SPLINE5_MEASURED[k], G.MARGIN * SC.SPLINE5_MEASURED[k]))
    assert set(worst) == set(SC.SPLINE5_MEASURED)
    assert all(worst[k] <= G.MARGIN * SC.SPLINE5_MEASURED[k] for k in worst)
    assert all(0 < v < 1e-14 for v in SC.SPLINE5_MEASURED.values())


@pytest.mark.gpu
def test_side_streams_are_non_blocking_and_the_spin_is_calibrated(sfb):
    e = SC.env()
    assert SC.stream_flags(e.s1.cuda_stream) == SC.HIP_STREAM_NON_BLOCKING and SC.stream_flags(e.s2.cuda_stream) == SC.HIP_STREAM_NON_BLOCKING
    assert e.s1.cuda_stream != e.s2.cuda_stream and 0 not in (e.s1.cuda_stream, e.s2.cuda_stream)
    ms = SC._time_spin(e.torch, SC.SPIN_MIN_MS * e.cycles_per_ms)                   # the calibration holds: a 20 ms spin takes 20 ms
    print("a spin sized for %.0f ms took %.2f ms" % (SC.SPIN_MIN_MS, ms))
    # the spin counts shader-clock cycles, and the clock moves between the device's power states (about 0.5 to 2.4 GHz): a factor of
    # five either way is what a change of state between calibration and use can make of it, more is a broken calibration.  (A spin
    # that came out too short to gate a case is caught there, by `pending`.)
    assert SC.SPIN_MIN_MS / 5.0 <= ms <= 5.0 * SC.SPIN_MIN_MS


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SC.CASES))
def test_stream_contract(sfb, oracle, knobs, name):
    case = SC.CASES[name]
    knobs.set(**case.knobs)
    real, decoy = case.build(sfb, oracle)
    SC.run_case(real, decoy, blocking=name in BLOCKING, name=name)
