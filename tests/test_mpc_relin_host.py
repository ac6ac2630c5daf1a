"""The re-linearisation law on the host (include/smooth_feedback_amd/mpc_relin.hpp through MPC::fill_flat_record /
assemble_flat_record / probe_relin of mpc.hpp) against the numpy restatement tests/mpc_relin_ref.py; the argument errors of
sfb_mpc_swarm_step_resident_flat; the header as C99; the default of MPCParams::relin_passes; the fixture; the sanitizer build of
examples/mpc_relin_selftest.cpp.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as R  # noqa: E402
import mpc_relin_gates as G  # noqa: E402
import mpc_relin_ref as Q  # noqa: E402
from examples import models_lib as M  # noqa: E402
from examples import mpc_relin_lib as RL  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, TF = 8, 2.0          # the smallest transcription with two mesh intervals
EPS = np.finfo(float).eps
T = np.array([0.3, 1.05, 2.775])
DX0 = np.array([[0.3, -0.2, 1.0, 0.1, -0.05, 0.2], [-0.4, 0.1, -0.6, -0.2, 0.15, -0.1], [0.05, 0.3, 1e-9, 0.0, 0.1, 0.05]])


def _pattern():
    d, _, _, _, Ap, Aj = M.mpc_pattern(G.VARIANT, K, TF)
    return d, Ap, Aj


def test_dyn_and_cr_rows_of_the_flat_record_at_zero_are_pass_ones():
    """ebar = vbar = 0: the flat record describes the pass-one problem on the dyn and cr rows; its x0 rows pin e_0"""
    d, Ap, Aj = _pattern()
    ndc = int(Ap[d["m"] - Q.NX])                                     # stored entries of the dyn and cr rows
    mdc = d["m"] - Q.NX
    rec = RL.flat_records(G.VARIANT, K, TF, T, DX0)
    assert np.array_equal(rec, RL.flat_records(G.VARIANT, K, TF, T, DX0, np.zeros((3, d["n"]))))
    Af, lf, uf = RL.assemble_flat(G.VARIANT, K, TF, rec)
    A1, l1, u1 = RL.assemble(G.VARIANT, K, TF, T, DX0)
    for b in range(3):
        e0 = Q.initial_deviation(T[b], DX0[b])
        Ad, lo, hi = Q.rows(Q.linearise(None, K), K, TF, e0)
        vals, outside = Q.csr_values(Ad, Ap, Aj)
        assert outside == 0.0
        # what float64 delivers on these inputs: the restatement against the transcription of pass one
        measured = max(R.scaled_error(A1[b, :ndc], vals[:ndc]), R.scaled_error(l1[b, :mdc], lo[:mdc]), R.scaled_error(u1[b, :mdc], hi[:mdc]))
        gate = G.MARGIN * measured
        err = max(R.scaled_error(Af[b, :ndc], A1[b, :ndc]), R.scaled_error(lf[b, :mdc], l1[b, :mdc]), R.scaled_error(uf[b, :mdc], u1[b, :mdc]))
        print("agent %d: flat rows against pass one %.2e (restatement %.2e, gate %.2e)" % (b, err, measured, gate))
        assert err <= gate
        # x0 rows: I e_0 = log(xdes(t)^-1 x).  The exact value is dx0; the restatement's own round trip through the matrices
        # (never below one rounding of a double of that size) sets the gate
        assert np.array_equal(Af[b, ndc:].reshape(Q.NX, Q.NX), np.eye(Q.NX))
        assert np.array_equal(lf[b, mdc:], uf[b, mdc:])
        measured0 = max(R.scaled_error(e0, DX0[b]), EPS)
        err0 = max(R.scaled_error(lf[b, mdc:], e0), R.scaled_error(lf[b, mdc:], DX0[b]))
        print("         x0 rows %.2e (restatement %.2e, gate %.2e)" % (err0, measured0, G.MARGIN * measured0))
        assert err0 <= G.MARGIN * measured0
        rf = RL.split_record(G.VARIANT, K, rec[b])
        assert np.all(rf["dxdes"] == 0.0) and np.array_equal(rf["J"], np.eye(Q.NX))


@pytest.mark.parametrize("rot", [1e-9, 0.3, 1.0])
def test_flat_jacobians_against_central_differences_of_the_restatement(rot):
    """A_i, B_i, C_i, D_i of the flat record about a plan with rotation parts `rot` (the points of flatten_reference.npz),
    and f, c = value - Jacobian * plan"""
    d, _, _ = _pattern()
    N = d["N"]
    rng = np.random.default_rng(7)
    plan = rng.uniform(-0.3, 0.3, (3, d["n"]))
    for i in range(N + 1):
        plan[:, i * Q.NX + 2] = rot * np.where(np.arange(3) + i & 1, -1.0, 1.0)
    rec = RL.flat_records(G.VARIANT, K, TF, T, DX0, plan)
    worst = 0.0
    for b in range(3):
        rf = RL.split_record(G.VARIANT, K, rec[b])
        for i in range(N):
            e, v = plan[b, i * Q.NX:(i + 1) * Q.NX], plan[b, (N + 1) * Q.NX + i * Q.NU:(N + 1) * Q.NX + (i + 1) * Q.NU]
            for fn, Je, Jv, val in ((Q.F, rf["dfdx"][i], rf["dfdu"][i], rf["f"][i]), (Q.cr, rf["dcdx"][i], rf["dcdu"][i], rf["c"][i])):
                Jre, Jrv = Q.jacobians_fd(fn, e, v)
                J, Jr = np.hstack([Je, Jv]), np.hstack([Jre, Jrv])
                tol = Q.fd_tolerance(1.0 + np.abs(Jr).max())
                worst = max(worst, np.abs(J - Jr).max() / tol)
                assert np.abs(J - Jr).max() <= tol, (b, i, np.abs(J - Jr).max(), tol)
                # value - J plan in the order of the law: NX + NU products and as many roundings of sums of size <= scale
                want = fn(e, v) - Je @ e - Jv @ v
                scale = 1.0 + np.abs(fn(e, v)).max() + np.abs(J).max() * max(np.abs(e).max(), np.abs(v).max()) * (Q.NX + Q.NU)
                assert np.abs(val - want).max() <= 4 * (Q.NX + Q.NU) * EPS * scale, (b, i, np.abs(val - want).max())
    print("rotation part %g: worst Jacobian difference at %.3f of its tolerance" % (rot, worst))


def test_probe_relin_covers_the_flat_jacobians():
    d, Ap, Aj = _pattern()
    kd, kr = RL.probe(G.VARIANT, K, TF)
    assert np.all(kr[kd]) and kr.sum() > kd.sum()
    rng = np.random.default_rng(3)
    plan = rng.uniform(-0.5, 0.5, (3, d["n"]))
    Af, _, _ = RL.assemble_flat(G.VARIANT, K, TF, RL.flat_records(G.VARIANT, K, TF, T, DX0, plan))
    nz = np.any(Af != 0.0, axis=0)
    assert np.all(kr[nz])                  # a generic flat record stays inside the mask ...
    assert np.any(nz & ~kd)                # ... and leaves today's: the ad and dr_expinv terms fill the group block
    print("A_keep: %d entries today, %d with the flat Jacobians, %d stored" % (kd.sum(), kr.sum(), len(kd)))


def test_relin_passes_defaults_to_zero():
    assert M.lib().sfbx_mpc_relin_default_params() == 0


def test_argument_errors_come_before_the_device_check(sfb):
    """no swarm can exist without a device, so what a CPU can see is the first check: it answers before any HIP call"""
    lib = sfb._capi.lib
    prm = sfb._capi.SfbQPParams()
    lib.sfb_qp_params_default(C.byref(prm))
    du0, code = np.zeros(2), np.zeros(1, np.int32)
    assert lib.sfb_mpc_swarm_step_resident_flat(None, C.byref(prm), M._p(du0), None, M._p(code), None, None) == sfb._capi.SFB_ERR_INVALID_ARG
    assert "swarm is NULL" in lib.sfb_last_error().decode()
    assert lib.sfb_mpc_swarm_step_resident_flat(None, None, None, None, None, None, None) == sfb._capi.SFB_ERR_INVALID_ARG
    assert "swarm is NULL" in lib.sfb_last_error().decode()
    # the neighbouring entry answers the same way
    assert lib.sfb_mpc_swarm_step_resident(None, C.byref(prm), 1, M._p(du0), None, M._p(code), None, None) == sfb._capi.SFB_ERR_INVALID_ARG


def test_header_with_the_new_entry_is_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc"
    c = tmp_path / "abi.c"
    c.write_text("#include <sfb.h>\n"
                 "typedef sfb_status (*flat_fn)(sfb_mpc_swarm *, const sfb_qp_params *, double *, uint32_t *, int32_t *, double *, double *);\n"
                 "flat_fn entry(void) { return sfb_mpc_swarm_step_resident_flat; }\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o",
                    str(tmp_path / "abi.o")], check=True)


def test_fixture_is_what_the_generator_describes(oracle):
    fx = G.fixture()
    assert (fx["K"], fx["tf"]) == (K, TF) and fx["dx0"].shape == (67, Q.NX) and fx["agent_max"].shape == (3, 67)
    assert 0.9 < np.abs(fx["dx0"][:, 2]).max() <= 1.0 and np.abs(fx["dx0"][:, 2]).min() >= 0.2
    assert len(np.unique(fx["t"])) == 67
    assert np.all(np.isin(fx["code"], G.KEPT))
    e = fx["agent_max"]
    assert np.all(e[1] < e[0]) and np.all(e[2] < e[1])              # the restatement's error falls at every pass, for every agent
    # the restatement reproduces its fixture (the leading agents: a few seconds)
    runs = Q.passes(oracle, M.mpc_pattern(G.VARIANT, K, TF), K, TF, fx["t"][:3], fx["dx0"][:3], 2)
    got = np.stack([r["agent_max"] for r in runs])
    print("restatement again:", got.tolist(), "fixture:", e[:, :3].tolist())
    assert np.allclose(got, e[:, :3], rtol=1e-6, atol=0.0)


def test_sanitizer_selftest_builds_and_passes(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++"
    exe = str(tmp_path / "mpc_relin_selftest")
    subprocess.check_call([cxx, "-O0", "-std=c++20", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "examples"), os.path.join(ROOT, "examples", "mpc_relin_selftest.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
