"""The collocation NLP front on the host (include/smooth_feedback_amd/ocp_to_nlp.hpp: detail::OCPNLP, ocp_to_nlp, nlpsol_to_ocpsol,
ocpsol_to_nlpsol; nlp.hpp) and the host-only entries of the C-ABI (sfb_ocp_nlp_structure / _pattern / _bounds) against the
60-digit fixture tests/golden/ocpnlp_reference.npz, within the gates of tests/ocpnlp_gates.py.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_gates as MG
import mesh_ref as R
import ocpnlp_gates as G
import ocpnlp_ref as NR
from examples import models_lib as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _host(c, order=2, numerical=False, calls=1, x=None, lam=None):
    return M.ocp_nlp_host(c["m"]["spec"], c["m"]["ops"], c["dims"], c, (c["crl"], c["cru"], c["cel"], c["ceu"]), c["x"] if x is None else x,
                          c["lambda"] if lam is None else lam, order=order, numerical=numerical, calls=calls)


def test_gate_is_four_times_the_float64_restatements_error():
    worst, left = G.measure()
    for k in sorted(worst):
        print("%-8s measured %.2e recorded %.2e gate %.2e" % (k, worst[k], G.MEASURED[k], G.gate(k)))
    assert not left, left                                                           # no fixture array is left unvisited
    assert set(worst) == set(G.MEASURED)
    for k, v in worst.items():                                                      # the restatement still delivers what was recorded
        assert v <= 2.0 * G.MEASURED[k] + 1e-18, (k, v)
        assert G.gate(k) == 4.0 * G.MEASURED[k]


def test_fixture_covers_what_the_issue_asks_for():
    assert G.CASES == ["bare", "ref", "cross", "mixed", "k13"]
    dims = {n: G.case(n)["dims"] for n in G.CASES}
    assert dims == {"bare": (1, 0, 0, 0, 0), "ref": (2, 1, 1, 4, 6), "cross": (2, 1, 1, 4, 6), "mixed": (3, 2, 2, 1, 3), "k13": (3, 2, 1, 3, 2)}
    assert [list(G.case(n)["m"]["K"]) for n in G.CASES] == [[1], [3, 3, 3], [3, 3, 3], [3, 5, 3, 3], [13, 13]]
    assert len(set(np.round(np.diff(np.append(G.case("mixed")["m"]["tau0"], 1.0)), 12))) > 1                    # unequal lengths
    bare = G.case("bare")
    assert len(bare["x"]) == 3 and len(bare["g"]) == 1
    for n in G.CASES:                                                               # nnz as the issue counts it
        c = G.case(n)
        nx, nu, nq, ncr, nce = c["dims"]
        K = c["m"]["K"].astype(np.int64)
        N = int(K.sum())
        assert len(c["dg"]) == int(np.sum(K * nx * (1 + K + nx + nu))) + nq * (2 + (nx + nu) * N) + ncr * N * (1 + nx + nu) + nce * (1 + nq + 2 * nx)
        assert np.all(np.diff(c["dg.colind"])[np.setdiff1d(np.arange(len(c["dg"]) - 1), c["dg.rowptr"][1:-1] - 1)] > 0)     # ascending in a row


@pytest.mark.parametrize("name", G.CASES)
def test_host_front_against_the_fixture(name):
    c = G.case(name)
    h = _host(c, order=2, calls=2)
    assert h["stable"]                                                              # a second call moves no output array
    assert np.array_equal(h["xl"], c["xl"]) and np.array_equal(h["xu"], c["xu"])
    for k in G.CLASSES:
        G.check(k, h[k], c[k], name)
    for k in ("gl", "gu", "w_scaling"):
        G.check("bounds", h[k], c[k], name + " " + k)
    for order in (0, 1):                                                            # the lower orders give the same bits
        lo = _host(c, order=order)
        assert lo["f"] == h["f"] and np.array_equal(lo["g"], h["g"])
        if order:
            assert np.array_equal(lo["df"], h["df"]) and np.array_equal(lo["dg"], h["dg"])


@pytest.mark.parametrize("name", G.CASES)
def test_patterns_of_the_c_abi_the_host_front_and_the_restatement_agree(sfb, name):
    c = G.case(name)
    K, dims = c["m"]["K"], c["dims"]
    mesh = sfb.PHMesh(K, c["m"]["tau0"])
    h = _host(c, order=2)
    rp, ci = sfb.ocp_nlp_pattern(mesh, dims)
    vb, cb = sfb.ocp_nlp_structure(mesh, dims)
    for got in ((rp, ci), (h["rowptr"], h["colind"]), NR.dg_pattern(K, dims)):
        assert np.array_equal(got[0], c["dg.rowptr"]) and np.array_equal(got[1], c["dg.colind"])
    for got in ((h["hcolptr"], h["hrowind"]), NR.h_pattern(K, dims)):
        assert np.array_equal(got[0], c["h.colptr"]) and np.array_equal(got[1], c["h.rowind"])
    assert np.array_equal(vb, c["var_beg"]) and np.array_equal(cb, c["con_beg"])
    assert (h["n"], h["m"]) == (vb[4], cb[4])
    xl, xu, gl, gu, ws = sfb.ocp_nlp_bounds(mesh, dims, c["crl"], c["cru"], c["cel"], c["ceu"])
    assert np.array_equal(xl, c["xl"]) and np.array_equal(xu, c["xu"])
    for k, v in (("gl", gl), ("gu", gu), ("w_scaling", ws)):
        G.check("bounds", v, c[k], name + " C-ABI " + k)


def test_cross_terms_between_q_and_the_end_states_are_kept():
    """theta and ce of `cross` have q x0 and q xf products; their second derivatives sit at (q, x0) and (q, xf), q before x"""
    c = G.case("cross")
    h = _host(c, order=2)
    vb = c["var_beg"]
    N = (vb[3] - vb[2]) // 2 - 1
    cols = np.repeat(np.arange(vb[4]), np.diff(c["h.colptr"]))
    for key in ("d2f", "d2g"):
        for lo in (vb[2], vb[2] + 2 * N):                                           # the columns of x0, of xf
            sel = (c["h.rowind"] == vb[1]) & (cols >= lo) & (cols < lo + 2)
            assert sel.sum() == 2
            assert np.count_nonzero(c[key][sel]) >= 1 and np.count_nonzero(h[key][sel]) >= 1, (key, lo)
            assert R.scaled_error(h[key][sel], c[key][sel]) <= G.gate(key)
    ref = G.case("ref")                                                             # without the products those entries are zero
    sel = (ref["h.rowind"] == vb[1]) & (cols >= vb[2])
    assert sel.sum() == 4 and not np.any(ref["d2f"][sel]) and not np.any(ref["d2g"][sel])


@pytest.mark.parametrize("name", G.CASES)
def test_numerical_differentiation_against_analytic(name):
    """the reference test's tolerances: 1e-4 relative for first, 1e-3 for second derivatives"""
    c = G.case(name)
    a, nu = _host(c, order=2), _host(c, order=2, numerical=True)
    assert nu["f"] == a["f"] and np.array_equal(nu["g"], a["g"])
    for k, tol in (("df", 1e-4), ("dg", 1e-4), ("d2f", 1e-3), ("d2g", 1e-3)):
        err = np.linalg.norm(nu[k] - a[k]) / max(np.linalg.norm(a[k]), 1e-300)
        print("%-5s %-6s %.2e" % (name, k, err))
        assert err <= tol, (k, err)


def test_reference_scenario_as_caller_code():
    assert M.test_ocp_to_nlp_api() == 0


@pytest.mark.parametrize("name", G.CASES)
def test_solution_conversions_there_and_back(name):
    """ocpsol_to_nlpsol(nlpsol_to_ocpsol(s)) samples the interpolants at the mesh's nodes: s.x and s.lambda again, within the
    gate of Mesh::eval (tests/mesh_gates.py, class eval.p0)"""
    c = G.case(name)
    h = _host(c, order=0)
    gate = MG.MARGIN * MG.MEASURED["eval.p0"]
    for k, ref in (("x_back", c["x"]), ("lambda_back", c["lambda"])):
        err = R.scaled_error(h[k], ref)
        print("%-6s %-12s %.2e (gate %.2e)" % (name, k, err, gate))
        assert err <= gate


def test_a_shape_the_harness_does_not_carry_is_refused():
    c = dict(G.case("ref"))
    c["m"] = G.case("mixed")["m"]
    with pytest.raises(LookupError):
        _host(c, order=0, x=np.zeros(1 + 1 + 2 * 15 + 14), lam=np.zeros(1))


def _need(*tools):
    for t in tools:
        if shutil.which(t) is None:
            pytest.skip("no %s" % t)


@pytest.mark.parametrize("header", ["nlp.hpp", "ocp_to_nlp.hpp"])
def test_forwarding_headers_compile_standalone(tmp_path, header):
    _need("g++")
    src = tmp_path / "one.cpp"
    src.write_text("#include <smooth/feedback/%s>\nint main() { smooth::feedback::NLPSolution s; return s.status == smooth::feedback::NLPSolution::Status::Unknown ? 0 : 1; }\n" % header)
    subprocess.run(["g++", "-std=c++20", "-Wall", "-fsyntax-only", "-I", INC, str(src)], check=True)


def test_sfb_h_with_the_nlp_entries_is_plain_c99(tmp_path):
    _need("gcc")
    c = tmp_path / "abi.c"
    c.write_text("#include <sfb.h>\nint main(void) { sfb_mesh m; sfb_ocp_dims d; int64_t nnz = 0, vb[5], cb[5]; m.nivals = 0; m.K = 0; m.tau0 = 0; "
                 "d.nx = 1; d.nu = d.nq = d.ncr = d.nce = 0; "
                 "return (int)(sfb_ocp_nlp_pattern(&m, &d, 0, 0, &nnz) + sfb_ocp_nlp_structure(&m, &d, vb, cb) + sfb_ocp_nlp_bounds(&m, &d, 0, 0, 0, 0, 0, 0, 0, 0, 0) + "
                 "sfb_ocp_nlp_batch_host(&m, &d, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + sfb_ocp_nlp_batch(&m, &d, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)) * 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-c", str(c), "-o", str(tmp_path / "abi.o")], check=True)


def test_argument_errors_come_in_the_stated_order_and_before_the_device_check(sfb):
    lib, E = sfb._capi.lib, sfb._capi
    K, tau0 = np.array([3, 5], np.int32), np.array([0.0, 0.5])
    buf = np.zeros(1 << 14)
    b = buf.ctypes.data
    NAMES = ("x", "Ff", "dFf", "Fg", "dFg", "Fcr", "dFcr", "ce", "dce", "g", "dg")

    def both(mesh, dims, batch, **null):
        m = C.byref(mesh) if mesh is not None else None
        d = C.byref(E.SfbOcpDims(*dims)) if dims is not None else None
        args = [None if k in null else b for k in NAMES]
        return {lib.sfb_ocp_nlp_batch_host(m, d, batch, *args), lib.sfb_ocp_nlp_batch(m, d, batch, *args, None)}

    def message():
        return lib.sfb_last_error().decode()

    good = sfb.PHMesh(K, tau0)
    wrong = sfb.PHMesh([3, 14], tau0)
    full = (2, 1, 1, 2, 3)
    inv = {E.SFB_ERR_INVALID_ARG}
    assert both(None, full, 1) == inv and both(E.SfbMesh(0, K.ctypes.data, tau0.ctypes.data), full, 1) == inv
    # the mesh before the batch, the batch before the dims, the dims before the sizes, the sizes before the NULL sets
    assert both(wrong.c, (0, -1, 0, 0, 0), -1, x=1, dFf=1) == inv and "K" in message()
    assert both(good.c, (0, -1, 0, 0, 0), -1, x=1, dFf=1) == inv and "batch" in message()
    assert both(good.c, None, 1, x=1, dFf=1) == inv and "dims" in message()
    assert both(good.c, (0, 1, 1, 1, 1), 1, x=1, dFf=1) == inv and "nx" in message()
    for k in range(1, 5):
        dims = [1, 0, 0, 0, 0]
        dims[k] = -1
        assert both(good.c, dims, 1, x=1, dFf=1) == inv and "nu, nq, ncr or nce" in message()
    assert both(good.c, (1 << 20, 1 << 10, 0, 0, 0), 1, x=1, dFf=1) == inv and "32-bit" in message()
    assert both(good.c, (1, 0, 0, 0, 1 << 30), 1, x=1, dFf=1) == inv and "32-bit" in message()
    for null in ({"dFf": 1}, {"dFg": 1}, {"dFcr": 1}, {"dce": 1}, {"dg": 1}, {"dFf": 1, "dFg": 1, "dFcr": 1}):
        assert both(good.c, full, 1, x=1, **null) == inv and "all or none" in message(), null
    assert both(good.c, (2, 1, 0, 0, 0), 1, dFg=1, dFcr=1, dce=1, x=1) == inv and "NULL" in message()          # empty segments: their Jacobians do not count
    for k in ("x", "Ff", "Fg", "Fcr", "ce", "g"):
        assert both(good.c, full, 1, **{k: 1}) == inv and "NULL" in message(), k
        assert both(good.c, full, 1, dFf=1, dFg=1, dFcr=1, dce=1, dg=1, **{k: 1}) == inv and "NULL" in message(), k
    # a batch of zero: OK without a device, and nothing is written
    buf[:] = 7.0
    assert both(good.c, full, 0) == {E.SFB_OK} and both(good.c, (1, 0, 0, 0, 0), 0, Fg=1, dFg=1, Fcr=1, dFcr=1, ce=1, dce=1) == {E.SFB_OK}
    assert np.all(buf == 7.0)
    # the host-only entries: the same first checks, then their own arrays
    d, nnz, vb = E.SfbOcpDims(*full), C.c_int64(-1), np.zeros(5, np.int64)
    assert lib.sfb_ocp_nlp_pattern(C.byref(wrong.c), C.byref(d), None, None, C.byref(nnz)) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_ocp_nlp_pattern(C.byref(good.c), None, None, None, C.byref(nnz)) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_ocp_nlp_pattern(C.byref(good.c), C.byref(d), b, None, C.byref(nnz)) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_ocp_nlp_pattern(C.byref(good.c), C.byref(d), None, None, None) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_ocp_nlp_pattern(C.byref(good.c), C.byref(d), None, None, C.byref(nnz)) == E.SFB_OK
    assert nnz.value == 3 * 2 * (1 + 3 + 2 + 1) + 5 * 2 * (1 + 5 + 2 + 1) + 1 * (2 + 3 * 8) + 2 * 8 * 4 + 3 * (1 + 1 + 4)
    assert lib.sfb_ocp_nlp_structure(C.byref(good.c), C.byref(d), None, vb.ctypes.data) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_ocp_nlp_structure(C.byref(good.c), C.byref(E.SfbOcpDims(0, 0, 0, 0, 0)), vb.ctypes.data, vb.ctypes.data) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_ocp_nlp_bounds(C.byref(good.c), C.byref(d), None, b, b, b, b, b, b, b, None) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_ocp_nlp_bounds(C.byref(good.c), C.byref(d), None, None, None, None, b, b, None, None, None) == E.SFB_OK     # xl, xu alone need no bounds
    if E.device_count() == 0:   # well-formed calls then fail for want of a device, never compute on the CPU
        assert both(good.c, full, 1) == {E.SFB_ERR_NO_DEVICE}
        assert both(good.c, full, 1, dFf=1, dFg=1, dFcr=1, dce=1, dg=1) == {E.SFB_ERR_NO_DEVICE}
        with pytest.raises(E.SfbError) as e:
            sfb.ocp_nlp_batch_host(good, (1, 0, 0, 0, 0), np.ones((2, 1 + 9)), np.zeros((2, 8, 1)), None, None, None, None, None, None, None)
        assert e.value.status == E.SFB_ERR_NO_DEVICE


def test_all_orders_and_the_conversions_under_address_and_ub_sanitizers(tmp_path):
    """examples/ocp_nlp_selftest.cpp: OCPNLP at orders 0, 1, 2, analytic and numerical, on the bare, the reference and the
    mixed-degree shape, plus nlpsol_to_ocpsol / ocpsol_to_nlpsol, as a stand-alone executable"""
    _need("g++")
    exe = tmp_path / "selftest"
    build = subprocess.run(["g++", "-std=c++20", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, "-I", os.path.join(ROOT, "examples"),
                            os.path.join(ROOT, "examples", "ocp_nlp_selftest.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime does not link here")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-3000:]
    assert run.stdout.count(" ok") == 3
