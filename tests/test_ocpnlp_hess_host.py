"""The Lagrangian Hessian of the collocation NLP on the host (OCPNLP::d2l_dx2 of include/smooth_feedback_amd/ocp_to_nlp.hpp over
meshfn::ocp_nlp_hess_pattern / _value / _assemble of mesh_function.hpp) and the host-side behaviour of the C-ABI entries
sfb_ocp_nlp_hess_pattern / _batch / _batch_host, against sigma d2f + d2g of the 60-digit fixture tests/golden/ocpnlp_reference.npz
within the `d2l` gate of tests/ocpnlp_hess_gates.py.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_ref as R
import ocpnlp_gates as G
import ocpnlp_hess_gates as HG
import ocpnlp_ref as NR
from examples import models_lib as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _bounds(c):
    return (c["crl"], c["cru"], c["cel"], c["ceu"])


def _d2l(c, sigma, x=None, lam=None, numerical=False, calls=1):
    return M.ocp_nlp_hess_host(c["m"]["spec"], c["m"]["ops"], c["dims"], c, _bounds(c), c["x"] if x is None else x,
                               c["lambda"] if lam is None else lam, sigma, numerical=numerical, calls=calls)


def test_d2l_gate_is_four_times_the_float64_restatements_error():
    errs = HG.measure()
    for (name, s), v in errs.items():
        print("%-6s sigma %4.1f restatement %.2e" % (name, s, v))
    worst = max(errs.values())
    print("d2l      measured %.2e recorded %.2e gate %.2e" % (worst, HG.MEASURED["d2l"], HG.gate()))
    assert set(n for n, _ in errs) == set(G.CASES) and set(s for _, s in errs) == set(HG.SIGMAS)
    assert HG.SIGMAS == (1.0, 0.0, 0.5, -2.0)
    assert worst <= 2.0 * HG.MEASURED["d2l"] + 1e-18                                # the restatement still delivers what was recorded
    assert HG.gate() == 4.0 * HG.MEASURED["d2l"]


@pytest.mark.parametrize("name", G.CASES)
def test_patterns_of_the_c_abi_the_constructor_the_shared_builder_and_the_restatement_agree(sfb, name):
    c = G.case(name)
    K, dims = c["m"]["K"], c["dims"]
    mesh = sfb.PHMesh(K, c["m"]["tau0"])
    front = M.ocp_nlp_host(c["m"]["spec"], c["m"]["ops"], dims, c, _bounds(c), c["x"], c["lambda"], order=2)    # the constructor's map-based builder
    h = _d2l(c, 1.0)
    nnz = C.c_int64(-1)
    d = sfb._capi.SfbOcpDims(*dims)
    assert sfb._capi.lib.sfb_ocp_nlp_hess_pattern(C.byref(mesh.c), C.byref(d), None, None, C.byref(nnz)) == 0      # both arrays NULL: the count alone
    assert nnz.value == len(c["h.rowind"])
    for who, got in (("C-ABI", sfb.ocp_nlp_hess_pattern(mesh, dims)), ("constructor", (front["hcolptr"], front["hrowind"])),
                     ("d2l member", (h["hcolptr"], h["hrowind"])), ("shared builder", (h["hcolptr2"], h["hrowind2"])), ("restatement", NR.h_pattern(K, dims))):
        assert np.array_equal(got[0], c["h.colptr"]) and np.array_equal(got[1], c["h.rowind"]), who


@pytest.mark.parametrize("sigma", HG.SIGMAS)
@pytest.mark.parametrize("name", G.CASES)
def test_d2l_against_the_fixture(name, sigma):
    c = G.case(name)
    h = _d2l(c, sigma, calls=2)
    assert h["stable"]                                                              # a second call moves no output array
    assert h["d2l"].shape == c["d2f"].shape and np.all(np.isfinite(h["d2l"]))
    HG.check(h["d2l"], HG.reference(c, sigma), "%s sigma %g" % (name, sigma))


@pytest.mark.parametrize("sigma", HG.SIGMAS)
def test_cross_terms_between_q_and_the_end_states_are_kept(sigma):
    """theta and ce of `cross` have q x0 and q xf products: their second derivatives sit at (q, x0) and (q, xf)"""
    c = G.case("cross")
    h = _d2l(c, sigma)
    vb = c["var_beg"]
    N = (vb[3] - vb[2]) // 2 - 1
    cols = np.repeat(np.arange(vb[4]), np.diff(c["h.colptr"]))
    ref = HG.reference(c, sigma)
    for lo in (vb[2], vb[2] + 2 * N):                                               # the columns of x0, of xf
        sel = (c["h.rowind"] == vb[1]) & (cols >= lo) & (cols < lo + 2)
        assert sel.sum() == 2
        assert np.count_nonzero(ref[sel]) >= 1 and np.count_nonzero(h["d2l"][sel]) >= 1, lo
        assert np.array_equal(h["d2l"][sel] != 0, ref[sel] != 0)
        assert R.scaled_error(h["d2l"][sel], ref[sel]) <= HG.gate()


@pytest.mark.parametrize("name", G.CASES)
def test_sigma_zero_and_lambda_zero_give_exact_zeros(name):
    c = G.case(name)
    h = _d2l(c, 0.0, lam=np.zeros(len(c["lambda"])))
    assert np.all(h["d2l"] == 0.0)


@pytest.mark.parametrize("name", G.CASES)
def test_d2l_against_the_existing_members_on_a_second_draw(name):
    """d2f_dx2 and d2g_dx2 keep their code: on another x, lambda, sigma the one-pass value is sigma d2f + d2g within the gate"""
    c = G.case(name)
    rng = np.random.default_rng(7 + len(name))
    x = rng.uniform(-1, 1, len(c["x"]))
    x[0] = float(np.round(rng.uniform(0.5, 3.0), 2))
    lam = rng.uniform(-1, 1, len(c["lambda"]))
    front = M.ocp_nlp_host(c["m"]["spec"], c["m"]["ops"], c["dims"], c, _bounds(c), x, lam, order=2)
    for sigma in (1.0, -0.75):
        h = _d2l(c, sigma, x=x, lam=lam)
        HG.check(h["d2l"], sigma * front["d2f"] + front["d2g"], "%s second draw sigma %g" % (name, sigma))


@pytest.mark.parametrize("name", G.CASES)
def test_numerical_differentiation_against_analytic(name):
    """the tolerance tests/test_ocpnlp_host.py uses for second derivatives: 1e-3 relative in the Frobenius norm"""
    c = G.case(name)
    a, nu = _d2l(c, 0.5), _d2l(c, 0.5, numerical=True)
    err = np.linalg.norm(nu["d2l"] - a["d2l"]) / max(np.linalg.norm(a["d2l"]), 1e-300)
    print("%-5s d2l %.2e" % (name, err))
    assert err <= 1e-3, err


def test_argument_errors_come_in_the_stated_order_and_before_the_device_check(sfb):
    lib, E = sfb._capi.lib, sfb._capi
    K, tau0 = np.array([3, 5], np.int32), np.array([0.0, 0.5])
    buf = np.zeros(1 << 14)
    b = buf.ctypes.data
    NAMES = ("x", "lam", "sigma", "dFf", "HLf", "dFg", "HLg", "dFcr", "HLcr", "d2theta", "d2ce_l", "hess")

    def both(mesh, dims, batch, **null):
        m = C.byref(mesh) if mesh is not None else None
        d = C.byref(E.SfbOcpDims(*dims)) if dims is not None else None
        args = [None if k in null else b for k in NAMES]
        return {lib.sfb_ocp_nlp_hess_batch_host(m, d, batch, *args), lib.sfb_ocp_nlp_hess_batch(m, d, batch, *args, None)}

    def message():
        return lib.sfb_last_error().decode()

    good = sfb.PHMesh(K, tau0)
    wrong = sfb.PHMesh([3, 14], tau0)
    full = (2, 1, 1, 2, 3)
    inv = {E.SFB_ERR_INVALID_ARG}
    assert both(None, full, 1) == inv and both(E.SfbMesh(0, K.ctypes.data, tau0.ctypes.data), full, 1) == inv
    # the mesh before the batch, the batch before the dims, the dims before the sizes, the sizes before the NULL arrays
    assert both(wrong.c, (0, -1, 0, 0, 0), -1, x=1) == inv and "K" in message()
    assert both(good.c, (0, -1, 0, 0, 0), -1, x=1) == inv and "batch" in message()
    assert both(good.c, None, 1, x=1) == inv and "dims" in message()
    assert both(good.c, (0, 1, 1, 1, 1), 1, x=1) == inv and "nx" in message()
    for k in range(1, 5):
        dims = [1, 0, 0, 0, 0]
        dims[k] = -1
        assert both(good.c, dims, 1, x=1) == inv and "nu, nq, ncr or nce" in message()
    assert both(good.c, (1 << 20, 1 << 10, 0, 0, 0), 1, x=1) == inv and "32-bit" in message()
    assert both(good.c, (1, 1 << 14, 0, 0, 0), 1, x=1) == inv and "hessian" in message() and "32-bit" in message()     # N nz^2 alone is too large
    for k in ("x", "lam", "sigma", "dFf", "HLf", "dFg", "HLg", "HLcr", "d2theta", "d2ce_l", "hess"):
        assert both(good.c, full, 1, **{k: 1}) == inv and "NULL" in message(), k
    # empty segments take NULL arrays, and dFcr is never read; without a device such calls get as far as the device check
    if E.device_count() == 0:
        assert both(good.c, (2, 1, 0, 0, 0), 1, dFg=1, HLg=1, dFcr=1, HLcr=1, d2ce_l=1) == {E.SFB_ERR_NO_DEVICE}
        assert both(good.c, full, 1, dFcr=1) == {E.SFB_ERR_NO_DEVICE}
        assert both(good.c, full, 1) == {E.SFB_ERR_NO_DEVICE}
        with pytest.raises(E.SfbError) as e:
            sfb.ocp_nlp_hess_batch_host(good, (1, 0, 0, 0, 0), np.ones((2, 1 + 9)), np.ones((2, 8)), 1.0, np.zeros((2, 8, 1, 2)), np.zeros((2, 8, 2, 2)),
                                        None, None, None, None, np.zeros((2, 3, 3)), None)
        assert e.value.status == E.SFB_ERR_NO_DEVICE
    # a batch of zero: OK without a device, and nothing is written
    buf[:] = 7.0
    assert both(good.c, full, 0) == {E.SFB_OK} and both(good.c, (1, 0, 0, 0, 0), 0, dFg=1, HLg=1, dFcr=1, HLcr=1, d2ce_l=1) == {E.SFB_OK}
    assert both(good.c, full, 0, **{k: 1 for k in NAMES}) == {E.SFB_OK}
    assert np.all(buf == 7.0)
    # the host-only pattern entry: the same first checks, then its own arrays
    d, nnz = E.SfbOcpDims(*full), C.c_int64(-1)
    assert lib.sfb_ocp_nlp_hess_pattern(C.byref(wrong.c), C.byref(d), None, None, C.byref(nnz)) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_ocp_nlp_hess_pattern(C.byref(good.c), None, None, None, C.byref(nnz)) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_ocp_nlp_hess_pattern(C.byref(good.c), C.byref(d), b, None, C.byref(nnz)) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_ocp_nlp_hess_pattern(C.byref(good.c), C.byref(d), None, None, None) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_ocp_nlp_hess_pattern(C.byref(good.c), C.byref(d), None, None, C.byref(nnz)) == E.SFB_OK
    nx, nu, nq, N = 2, 1, 1, 8
    assert nnz.value == len(NR.h_pattern(K, full)[1]) == (1 + nq + nq * (nq + 1) // 2 + nx * (1 + nq) + 3 + (N - 1) * (nx + 3) + nx * (1 + nq + nx) + 3
                                                          + N * (nu * (1 + nx) + 1))


def test_sfb_h_with_the_hessian_entries_is_plain_c99(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    c = tmp_path / "abi.c"
    c.write_text("#include <sfb.h>\nint main(void) { sfb_mesh m; sfb_ocp_dims d; int64_t nnz = 0; m.nivals = 0; m.K = 0; m.tau0 = 0; "
                 "d.nx = 1; d.nu = d.nq = d.ncr = d.nce = 0; "
                 "return (int)(sfb_ocp_nlp_hess_pattern(&m, &d, 0, 0, &nnz) + sfb_ocp_nlp_hess_batch_host(&m, &d, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + "
                 "sfb_ocp_nlp_hess_batch(&m, &d, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)) * 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-c", str(c), "-o", str(tmp_path / "abi.o")], check=True)


def test_d2l_and_the_pattern_builder_under_address_and_ub_sanitizers(tmp_path):
    """examples/ocp_nlp_hess_selftest.cpp: d2l_dx2 and meshfn::ocp_nlp_hess_pattern on the bare and the reference shape, analytic and
    numerical, four sigmas, d2l == sigma d2f + d2g to 1e-12 relative, as a stand-alone executable (nothing is loaded into Python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "hess_selftest"
    build = subprocess.run(["g++", "-std=c++20", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, "-I", os.path.join(ROOT, "examples"),
                            os.path.join(ROOT, "examples", "ocp_nlp_hess_selftest.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime does not link here")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-3000:]
    assert run.stdout.count("hessian ok") == 2
