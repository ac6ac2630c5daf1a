"""The functions over a collocation mesh (include/smooth_feedback_amd/mesh_function.hpp: MeshValue, mesh_eval, mesh_integrate,
mesh_dyn at orders 0, 1, 2) through the host entries of examples/collocation.cpp, and the host-only pattern functions of the
C-ABI, against the 60-digit fixture tests/golden/meshfn_reference.npz within the gates of tests/meshfn_gates.py (four times the
float64 numpy restatement's own error per class).  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import meshfn_gates as G
import meshfn_ref as MR
from examples import models_lib as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HOST_FN = {"eval": ("eval", False), "evals": ("eval", True), "integrate": ("integrate", False), "dyn": ("dyn", False)}


def test_gate_is_four_times_the_float64_restatements_error():
    """prints what tests/meshfn_ref.py delivers against the 60-digit values per class, next to the recorded figure the gates
    are built from; the restatement still delivers it (within the same margin), every class has a figure, and no array of the
    fixture is left out"""
    worst, left_out = G.measure()
    for k in sorted(worst):
        print("%-14s restatement %.2e   recorded %.2e   gate %.2e" % (k, worst[k], G.MEASURED[k], G.MARGIN * G.MEASURED[k]))
    assert not left_out, left_out
    assert set(worst) == set(G.MEASURED)
    assert all(worst[k] <= G.MARGIN * G.MEASURED[k] for k in worst)
    assert all(0 < v < 1e-9 for v in G.MEASURED.values())


def test_fixture_covers_what_the_issue_asks_for():
    K = {n: G.section("mesh." + n)["K"].tolist() for n in G.MESHES}
    assert K == {"k1": [1], "m36": [3, 5, 3, 3], "m46": [5, 4], "k13": [13, 13], "u13": [4] * 13}
    assert len(set(np.round(np.diff(np.append(G.section("mesh.m36")["tau0"], 1.0)), 12))) > 1        # unequal lengths
    assert G.section("mesh.m46")["ops"].tolist() == [[0, 0, 8], [0, 0, 5]] and list(G.section("mesh.m46")["spec"][:2]) == [4, 6]
    dims = {n: tuple(G.section("fn." + n)["dims"].tolist()) for n in G.FNS}
    assert dims == {"poly": (3, 2, 3), "cost": (3, 2, 1), "scalar": (1, 0, 1), "trig": (12, 2, 12), "vehicle": (6, 2, 6)}
    assert {3, 4} <= set(G.section("fn.trig")["terms"][:, [2, 4]].ravel().tolist())                    # sines and cosines
    pairs = {(str(G.case(n)["mesh"]), str(G.case(n)["fn"])) for n in G.CASES}
    assert {(m, "poly") for m in G.MESHES} <= pairs and ("u13", "trig") in pairs and ("k13", "scalar") in pairs and ("k1", "cost") in pairs
    for n in G.CASES:
        c = G.case(n)
        want = {"eval", "evals", "integrate"} | ({"dyn"} if c["f"]["dims"][0] == c["f"]["dims"][2] else set())
        assert {k.split(".")[0] for k in G.result_keys(c)} == want
        assert {k.split(".")[1] for k in G.result_keys(c)} == set(["F", "dF", "d2F"][:c["order"] + 1])


def _host(c, key, deriv, **kw):
    fn, scale = HOST_FN[key]
    m, f = c["m"], c["f"]
    vehicle = str(c["fn"]) == "vehicle"
    shape = "vehicle" if vehicle else tuple(int(v) for v in f["dims"])
    return M.meshfn_host(m["spec"], m["ops"], None, fn, deriv, shape, f["terms"], f["coef"], c["t0"], c["tf"], c["xs_flat"] if vehicle else c["xs"],
                         c["us"], scale=scale, lam=c["lam"][key], **kw)


@pytest.mark.parametrize("name", G.CASES)
def test_host_front_against_the_fixture(name):
    """every function at every order the case carries; the values of a lower order are the same bits at a higher one, and a
    second call on an allocated MeshValue moves none of its arrays"""
    c = G.case(name)
    for key in G.FUNCTIONS:
        if key + ".F" not in c:
            continue
        if str(c["fn"]) == "vehicle" and key == "dyn":      # the defect needs a vector state: the harness carries no such call
            with pytest.raises(LookupError):
                _host(c, key, 0)
            continue
        got = [_host(c, key, d, calls=2) for d in range(c["order"] + 1)]
        for d, g in enumerate(got):
            assert g["stable"], (key, d)
            G.check(key + ".F", g["F"], c[key + ".F"], "%s order %d" % (name, d))
            assert np.array_equal(g["F"], got[0]["F"])
            if d >= 1:
                G.check(key + ".dF", g["val"], c[key + ".dF"], "%s order %d" % (name, d))
                assert np.array_equal(g["val"], got[1]["val"])
            if d >= 2:
                G.check(key + ".d2F", g["val2"], c[key + ".d2F"], name)


@pytest.mark.parametrize("name", G.CASES)
def test_patterns_of_the_c_abi_the_host_front_and_the_restatement_agree(sfb, name):
    c = G.case(name)
    nx, nu, nf = [int(v) for v in c["f"]["dims"]]
    K, tau0 = c["m"]["K"], c["m"]["tau0"]
    N = int(K.sum())
    mesh = sfb.PHMesh(K, tau0)
    vehicle = str(c["fn"]) == "vehicle"
    order = min(c["order"], 2)
    # eval
    rp, ci = sfb.mesh_eval_pattern(mesh, nx, nu, nf)
    want = MR.eval_pattern(N, nx, nu, nf)
    host = _host(c, "eval", order)
    assert np.array_equal(rp, want[0]) and np.array_equal(ci, want[1]) and np.array_equal(host["rowptr"], rp) and np.array_equal(host["colind"], ci)
    assert host["cols"] == 2 + nx * (N + 1) + nu * N
    # integrate: a dense row block
    host = _host(c, "integrate", order)
    want = MR.integrate_pattern(N, nx, nu, nf)
    assert np.array_equal(host["rowptr"], want[0]) and np.array_equal(host["colind"], want[1])
    last_state = (host["colind"] >= 2 + N * nx) & (host["colind"] < 2 + (N + 1) * nx)
    assert np.all(host["val"][last_state] == 0.0)
    if order >= 2:
        want = MR.d2_pattern(N, nx, nu)
        assert np.array_equal(host["colptr2"], want[0]) and np.array_equal(host["rowind2"], want[1])
        cols = np.repeat(np.arange(len(want[0]) - 1), np.diff(want[0]))
        assert np.all(want[1] <= cols)                                              # the upper triangle
    # dyn
    if nf == nx:
        rp, ci = sfb.mesh_dyn_pattern(mesh, nx, nu)
        want = MR.dyn_pattern(K, nx, nu)
        assert np.array_equal(rp, want[0]) and np.array_equal(ci, want[1])
        assert np.diff(rp).tolist() == [2 + k + nx + nu for k in K for _ in range(k * nx)]
        for r in range(len(rp) - 1):
            assert np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0)                          # columns ascend within each row
        if not vehicle:
            host = _host(c, "dyn", order)
            assert np.array_equal(host["rowptr"], rp) and np.array_equal(host["colind"], ci)
            if order >= 2:
                want = MR.d2_pattern(N, nx, nu)
                assert np.array_equal(host["colptr2"], want[0]) and np.array_equal(host["rowind2"], want[1])


def _is_approx(a, b, prec):
    """Eigen's isApprox: |a - b| <= prec min(|a|, |b|) in the Frobenius norm"""
    return np.linalg.norm(a - b) <= prec * min(np.linalg.norm(a), np.linalg.norm(b))


@pytest.mark.parametrize("name", ["poly_m46", "poly_k13", "cost_m36", "scalar_u13", "trig_m46", "vehicle_m36"])
def test_numerical_differentiation_against_analytic(name):
    """DT = Numerical against DT = Analytic at the reference test's tolerance (relative 1e-3 in the sense of isApprox)"""
    c = G.case(name)
    for key in G.FUNCTIONS:
        if key + ".F" not in c or (str(c["fn"]) == "vehicle" and key == "dyn"):
            continue
        a, n = _host(c, key, c["order"]), _host(c, key, c["order"], numerical=True)
        assert np.array_equal(a["F"], n["F"])
        assert np.array_equal(a["colind"], n["colind"])
        print(key, np.linalg.norm(a["val"] - n["val"]) / np.linalg.norm(a["val"]))
        assert _is_approx(n["val"], a["val"], 1e-3), key
        if c["order"] >= 2:
            print(key, "d2F", np.linalg.norm(a["val2"] - n["val2"]) / np.linalg.norm(a["val2"]))
            assert _is_approx(n["val2"], a["val2"], 1e-3), key


def test_reference_trajectory_scenarios_as_caller_code():
    """x = 0.1 t^2 - 0.4 t + 0.2 and x = 1.5 exp(-t) on Mesh<5, 5> after refine_ph(0, 40), t0 = 3, tf = 5: max |mesh_dyn.F| <= 1e-8,
    the integrals within 1e-4 of 0.217333 + 0.2 and of 0.00273752"""
    assert M.test_mesh_function_api() == 0


def test_a_shape_or_order_the_harness_does_not_carry_is_refused():
    c = G.case("cost_k1")
    with pytest.raises(LookupError):
        _host(c, "dyn", 1)                     # nf != nx
    v = G.case("vehicle_m36")
    with pytest.raises(LookupError):
        _host(v, "eval", 2)                    # order 2 needs Rn state and input


def _need(*tools):
    for t in tools:
        if shutil.which(t) is None:
            pytest.skip("no %s" % t)


def test_forwarding_header_compiles_standalone(tmp_path):
    _need("g++")
    src = tmp_path / "one.cpp"
    src.write_text("#include <smooth/feedback/collocation/mesh_function.hpp>\n"
                   "int main() { smooth::feedback::MeshValue<2> v; smooth::feedback::set_zero(v); return v.allocated ? 1 : 0; }\n")
    subprocess.run(["g++", "-std=c++20", "-Wall", "-fsyntax-only", "-I", INC, str(src)], check=True)


def test_sfb_h_with_the_mesh_function_entries_is_plain_c99(tmp_path):
    _need("gcc")
    c = tmp_path / "abi.c"
    c.write_text("#include <sfb.h>\nint main(void) { sfb_mesh m; int64_t nnz = 0; m.nivals = 0; m.K = 0; m.tau0 = 0; "
                 "return (int)(sfb_mesh_dyn_pattern(&m, 1, 0, 0, 0, &nnz) + sfb_mesh_dyn_batch_host(&m, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0)) * 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-c", str(c), "-o", str(tmp_path / "abi.o")], check=True)


def test_argument_errors_come_before_the_device_check(sfb):
    lib, E = sfb._capi.lib, sfb._capi
    K, tau0 = np.array([3, 5], np.int32), np.array([0.0, 0.5])
    buf = np.zeros(4096)
    p = lambda a: a.ctypes.data                                                     # noqa: E731
    b = p(buf)

    def every(mesh, batch, nx, nu, nf, t0=b, F=b, dF=b, out=b, dout=b, X=b):
        m = C.byref(mesh) if mesh is not None else None
        return {lib.sfb_mesh_eval_batch_host(m, batch, nx, nu, nf, 0, t0, b, F, dF, out, dout), lib.sfb_mesh_eval_batch(m, batch, nx, nu, nf, 0, t0, b, F, dF, out, dout, None),
                lib.sfb_mesh_integrate_batch_host(m, batch, nx, nu, nf, t0, b, F, dF, out, dout), lib.sfb_mesh_integrate_batch(m, batch, nx, nu, nf, t0, b, F, dF, out, dout, None),
                lib.sfb_mesh_dyn_batch_host(m, batch, nx, nu, t0, b, X, F, dF, out, dout), lib.sfb_mesh_dyn_batch(m, batch, nx, nu, t0, b, X, F, dF, out, dout, None)}

    def message():
        return lib.sfb_last_error().decode()

    good = sfb.PHMesh(K, tau0)
    wrong = [sfb.PHMesh([3, 13 + 1], tau0), sfb.PHMesh([0, 3], tau0), sfb.PHMesh(K, [0.1, 0.5]), sfb.PHMesh(K, [0.0, 0.0]), sfb.PHMesh(K, [0.0, 1.0])]
    bad = [(None, 1, 1, 1, 1), (E.SfbMesh(2, None, p(tau0)), 1, 1, 1, 1), (E.SfbMesh(0, p(K), p(tau0)), 1, 1, 1, 1)] + [(m.c, 1, 1, 1, 1) for m in wrong]
    bad += [(good.c, -1, 1, 1, 1), (good.c, 1, -1, 1, 1), (good.c, 1, 1, -1, 1)]
    for args in bad:
        assert every(*args) == {E.SFB_ERR_INVALID_ARG}, args[1:]
    # the stated order: the mesh before the batch, the batch before the sizes, the sizes before the arrays
    assert every(wrong[0].c, -1, -1, -1, 1, t0=None) == {E.SFB_ERR_INVALID_ARG} and "K" in message()
    assert every(good.c, -1, -1, 1, 1, t0=None) == {E.SFB_ERR_INVALID_ARG} and "batch" in message()
    assert every(good.c, 1, -1, -1, 1, t0=None) == {E.SFB_ERR_INVALID_ARG} and "nx" in message()
    assert every(good.c, 1, 1, -1, 1, t0=None) == {E.SFB_ERR_INVALID_ARG} and "nu" in message()
    assert lib.sfb_mesh_eval_batch_host(C.byref(good.c), 1, 1, 1, -1, 0, b, b, b, b, b, b) == E.SFB_ERR_INVALID_ARG and "nf" in message()
    assert every(good.c, 1, 1, 1, 1, dF=None) == {E.SFB_ERR_INVALID_ARG} and "both or neither" in message()     # dF without its output
    assert every(good.c, 1, 1, 1, 1, dout=None) == {E.SFB_ERR_INVALID_ARG}
    assert every(good.c, 1, 1, 1, 1, t0=None) == {E.SFB_ERR_INVALID_ARG} and "NULL" in message()
    assert every(good.c, 1, 1, 1, 1, out=None) == {E.SFB_ERR_INVALID_ARG}
    assert lib.sfb_mesh_dyn_batch_host(C.byref(good.c), 1, 1, 1, b, b, None, b, b, b, b) == E.SFB_ERR_INVALID_ARG
    # the pattern functions: host only, the same mesh checks, and a size query with NULL arrays
    nnz = C.c_int64(-1)
    assert lib.sfb_mesh_dyn_pattern(C.byref(wrong[0].c), 1, 1, None, None, C.byref(nnz)) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_mesh_eval_pattern(C.byref(good.c), 1, -1, 1, None, None, C.byref(nnz)) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_mesh_eval_pattern(C.byref(good.c), 1, 1, 1, b, None, C.byref(nnz)) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_mesh_eval_pattern(C.byref(good.c), 1, 1, 1, None, None, None) == E.SFB_ERR_INVALID_ARG
    assert lib.sfb_mesh_dyn_pattern(C.byref(good.c), 2, 1, None, None, C.byref(nnz)) == E.SFB_OK and nnz.value == 3 * 2 * (2 + 3 + 2 + 1) + 5 * 2 * (2 + 5 + 2 + 1)
    assert lib.sfb_mesh_eval_pattern(C.byref(good.c), 2, 1, 3, None, None, C.byref(nnz)) == E.SFB_OK and nnz.value == 8 * 3 * (2 + 2 + 1)
    if E.device_count() == 0:   # well-formed calls then fail for want of a device, never compute on the CPU
        assert every(good.c, 1, 1, 1, 1) == {E.SFB_ERR_NO_DEVICE}
        assert every(good.c, 1, 1, 0, 1, dF=None, dout=None) == {E.SFB_ERR_NO_DEVICE}            # values only, no inputs
        with pytest.raises(E.SfbError) as e:
            sfb.mesh_dyn_batch_host(good, 1, 0.0, 1.0, np.zeros((2, 9, 2)), np.zeros((2, 8, 2)), np.zeros((2, 8, 2, 4)))
        assert e.value.status == E.SFB_ERR_NO_DEVICE


SANITIZED_MAIN = r"""
#include <smooth/feedback/collocation/mesh_function.hpp>
#include <cstdio>
namespace F = smooth::feedback;
// f = (x0 x1 + t u0, sin(x0) + u0^2) with its derivatives in closed form
struct Fn {
  F::Vec<2> operator()(double t, const F::Rn<2> & x, const F::Rn<1> & u) const { return {x.v[0] * x.v[1] + t * u.v[0], std::sin(x.v[0]) + u.v[0] * u.v[0]}; }
  void jacobian(double t, const F::Rn<2> & x, const F::Rn<1> & u, F::Mat<2, 4> & J) const
  {
    J = F::Mat<2, 4>::Zero();
    J(0, 0) = u.v[0]; J(0, 1) = x.v[1]; J(0, 2) = x.v[0]; J(0, 3) = t;
    J(1, 1) = std::cos(x.v[0]); J(1, 3) = 2 * u.v[0];
  }
  void hessian(double, const F::Rn<2> & x, const F::Rn<1> &, F::Mat<4, 8> & H) const
  {
    H = F::Mat<4, 8>::Zero();
    H(1, 2) = H(2, 1) = 1; H(0, 3) = H(3, 0) = 1;
    H(1, 4 + 1) = -std::sin(x.v[0]); H(3, 4 + 3) = 2;
  }
};
template<unsigned char D, F::diff::Type DT, class M>
static int three(const M & m, const std::vector<F::Rn<2>> & X, const std::vector<F::Rn<1>> & U)
{
  Fn f;
  F::MeshValue<D> e, i, d;
  for (int call = 0; call < 3; ++call) {   // the second and third call reuse what the first allocated
    if constexpr (D == 2) {
      e.lambda.assign(2 * m.N_colloc(), 0.5);
      i.lambda.assign(2, -0.25);
      d.lambda.assign(2 * m.N_colloc(), 1.5);
    }
    F::mesh_eval<D, DT>(e, m, f, 0.25, 1.75, X, U, call == 1);
    F::mesh_integrate<D, DT>(i, m, f, 0.25, 1.75, X, U);
    F::mesh_dyn<D, DT>(d, m, f, 0.25, 1.75, X, U);
    if (!e.allocated || !i.allocated || !d.allocated) return 1;
    if (e.F.size() != 2 * m.N_colloc() || i.F.size() != 2 || d.F.size() != 2 * m.N_colloc()) return 2;
    for (const double v : d.F)
      if (!(v == v)) return 3;
    if constexpr (D >= 1)
      if (d.dF.val.size() != (std::size_t)d.dF.rowptr.back() || i.dF.val.size() != 2 * (std::size_t)i.dF.cols) return 4;
    if constexpr (D >= 2)
      if (d.d2F.val.size() != (std::size_t)d.d2F.colptr.back() || e.d2F.colptr.size() != (std::size_t)e.d2F.cols + 1) return 5;
  }
  return 0;
}
template<class M>
static int drive(M m, int rounds)
{
  unsigned s = 2463534242u;
  auto next = [&s] { return s = s * 1664525u + 1013904223u, s >> 8; };
  for (int r = 0; r < rounds; ++r) {
    const std::size_t i = next() % m.N_ivals();
    switch (next() % 4) {
    case 0: m.refine_ph(i, M::Kmin + next() % (3 * M::Kmax)); break;
    case 1: m.increase_degrees(); break;
    case 2: m.decrease_degrees(); break;
    default: m.set_N_colloc_ival(i, M::Kmin + next() % (M::Kmax + 2 - M::Kmin)); break;
    }
    if (m.N_ivals() > 60) m = M();
    std::vector<F::Rn<2>> X(m.N_colloc() + 1);
    std::vector<F::Rn<1>> U(m.N_colloc());
    for (auto & x : X) x.v = {1e-3 * (next() % 2000) - 1, 1e-3 * (next() % 2000) - 1};
    for (auto & u : U) u.v = {1e-3 * (next() % 2000) - 1};
    int rc = three<0, F::diff::Type::Default>(m, X, U);
    if (!rc) rc = three<1, F::diff::Type::Analytic>(m, X, U);
    if (!rc) rc = three<2, F::diff::Type::Analytic>(m, X, U);
    if (!rc) rc = three<1, F::diff::Type::Numerical>(m, X, U);
    if (!rc && r % 8 == 0) rc = three<2, F::diff::Type::Numerical>(m, X, U);
    if (rc) return rc;
  }
  return 0;
}
int main()
{
  const int rc = drive(F::Mesh<3, 6>(), 60) + 10 * drive(F::Mesh<1, 2>(), 60);
  std::printf("rc %d\n", rc);
  return rc;
}
"""


def test_all_functions_and_orders_under_address_and_ub_sanitizers(tmp_path):
    """a stand-alone program (its own main, run directly) drives the three functions at the three orders, analytic and by
    differences, over random refinement sequences, with every MeshValue reused across calls"""
    _need("g++")
    src, exe = tmp_path / "drive.cpp", tmp_path / "drive"
    src.write_text(SANITIZED_MAIN)
    build = subprocess.run(["g++", "-std=c++20", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, str(src), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and any(lib in build.stderr for lib in ("-lasan", "-lubsan", "libasan", "libubsan")):
        pytest.skip("the sanitizer runtime does not link here")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
