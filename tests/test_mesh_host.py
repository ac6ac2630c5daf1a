"""The ph collocation mesh (include/smooth_feedback_amd/mesh.hpp: Mesh<Kmin, Kmax>), the collocation dynamics-error
estimate and the flattened dynamics (dyn_error.hpp) through the host entries of examples/collocation.cpp, against the
60-digit fixture tests/golden/mesh_reference.npz within the gates of tests/mesh_gates.py (four times the float64 numpy
restatement's own error per case class).  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_gates as G
import mesh_ref as R
from examples import models_lib as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_gate_is_four_times_the_float64_restatements_error():
    """prints what tests/mesh_ref.py delivers against the 60-digit values per case class, next to the recorded figure the
    gates are built from; the restatement still delivers it (within the same margin), every class has a figure, and no
    array of the fixture is left out"""
    worst, left_out = G.measure()
    for k in sorted(worst):
        print("%-16s restatement %.2e   recorded %.2e   gate %.2e" % (k, worst[k], G.MEASURED[k], G.MARGIN * G.MEASURED[k]))
    assert not left_out, left_out
    assert set(worst) == set(G.MEASURED)
    assert all(worst[k] <= G.MARGIN * G.MEASURED[k] for k in worst)
    assert all(0 < v < 1e-9 for v in G.MEASURED.values())


def test_fixture_covers_what_the_issue_asks_for():
    assert [len(G.FX["lgr.K%d.x" % K]) for K in range(1, 16)] == list(range(1, 16))
    basic = G.mesh("basic")
    assert list(basic["spec"]) == [5, 10, 1, 5]
    assert basic["ops"].tolist() == [[0, 0, 50], [0, 1, 10], [0, 1, 13], [0, 2, 27], [0, 7, 33], [0, 9, 22]]
    assert G.mesh("k3567")["K"].tolist() == [3, 5, 6, 7] and list(G.mesh("k3567")["spec"][:2]) == [3, 6]
    assert G.mesh("u13")["K"].tolist() == [4] * 13 and list(G.mesh("u13")["spec"]) == [4, 4, 13, 4]
    # dyn-error classes: at least four cases each, and the 60-digit errors themselves lie inside the class bounds
    count = {c: 0 for c in G.CLASSES}
    shapes, sizes = set(), set()
    for name in G.DYN:
        d = G.dyn(name)
        lo, hi = G.CLASS_BOUNDS[d["cls_name"]]
        assert lo <= d["errs"].max() <= hi, (name, d["errs"].max())
        count[d["cls_name"]] += 1
        shapes.add(tuple(d["base"]["K"].tolist()))
        sizes.add((int(d["nx"]), int(d["nu"])))
    assert all(v >= 4 for v in count.values()), count
    assert {(4,), (4, 4), (4,) * 13, (5, 5, 5), (3, 5, 6), (5,) * 16, (13, 13)} <= shapes and max(map(max, shapes)) == 13    # K + 1 = 14: the kernels' limit
    assert {n for n, _ in sizes} == {1, 2, 12} and {n for _, n in sizes} == {0, 1, 2}
    ref = G.dyn("ex_ref")    # the reference's known answer
    assert ref["coef"].tolist() == [[0.2, -0.4, 0.1, 0.0]] and (float(ref["t0"]), float(ref["tf"])) == (3.0, 5.0) and int(ref["nu"]) == 0
    for e in G.EVALS:
        s, m = G.section("eval." + e), G.mesh(e)
        t = s["t"]
        assert t.min() < 0 and t.max() > 1 and 0.0 in t and 1.0 in t and m["tau0"][1] in t and s["out"].shape[:2] == (2, 3)
    assert {(str(G.section("audit." + n)["model"]), -(-int(G.section("audit." + n)["K"]) // 4)) for n in G.AUDIT} == {
        ("vehicle6", 2), ("vehicle6", 13), ("vehicle12", 2), ("rigid", 2)}
    for model in G.FLAT:
        d = G.section("flat." + model)
        n = np.linalg.norm(d["e"], axis=1)
        assert np.all(n[d["cls"] == 0] <= 1e-9) and np.all(n[d["cls"] == 1] <= 1.2) and min(np.sum(d["cls"] == 0), np.sum(d["cls"] == 1)) >= 4


@pytest.mark.parametrize("K", range(1, 16))
def test_lgr_nodes_and_weights(K):
    """lgr_nodes through a one-interval mesh of K points on [0, 1]: tau = (x + 1) / 2, weights / 2"""
    for kmin, kmax in ((5, 10), (3, 6), (8, 8), (4, 4), (5, 5)):
        if kmin <= K <= kmax + 1:
            got = M.mesh_script((kmin, kmax, 1, K))
            G.check("lgr", 2 * got["nodes"][:-1] - 1, G.FX["lgr.K%d.x" % K], "K=%d nodes" % K)
            G.check("lgr", 2 * got["weights"][:-1], G.FX["lgr.K%d.w" % K], "K=%d weights" % K)
            return
    # degrees no harness instantiation reaches come from the uniform mesh (the same lgr_nodes)
    nodes, w, _ = M.mesh(1, K)
    G.check("lgr", 2 * nodes[:-1] - 1, G.FX["lgr.K%d.x" % K], "K=%d nodes" % K)
    G.check("lgr", 2 * w[:-1], G.FX["lgr.K%d.w" % K], "K=%d weights" % K)


@pytest.mark.parametrize("name", G.MESHES)
def test_mesh_scripts_against_the_fixture(name):
    m = G.mesh(name)
    got = M.mesh_script(m["spec"], m["ops"], m["opdata"])
    for key, g, r in G.mesh_rows(name, got["K"], got["tau0"], got["nodes"], got["weights"], np.concatenate([d.ravel() for d in got["diffmat"]]),
                                 np.concatenate([i.ravel() for i in got["intmat"]])):
        G.check(key, g, r, name)


@pytest.mark.parametrize("name", G.EVALS)
def test_eval_against_the_fixture(name):
    m, e = G.mesh(name), G.section("eval." + name)
    want_found = [R.find(m["tau0"], t) for t in e["t"]]
    for ei, extend in enumerate((True, False)):
        for p in range(3):
            got = M.mesh_script(m["spec"], m["ops"], m["opdata"], t=e["t"], vals=e["vals"] if extend else e["vals"][:-1], p=p, extend=extend)
            G.check("eval.p%d" % p, got["eval"], e["out"][ei, p], "%s extend=%d" % (name, extend))
            assert got["found"].tolist() == want_found


@pytest.mark.parametrize("name", G.DYN)
def test_mesh_dyn_error_against_the_fixture(name):
    d = G.dyn(name)
    b = d["base"]
    got = M.mesh_dyn_error_host(b["spec"], b["ops"], b["opdata"], int(d["fid"]), d["coef"], float(d["t0"]), float(d["tf"]), d["vals_x"], d["vals_u"])
    assert got.shape == d["errs"].shape
    G.check("dynerr." + d["cls_name"], got, d["errs"], name)


@pytest.mark.parametrize("model", G.FLAT)
def test_flat_dynamics_against_the_fixture(model):
    d = G.section("flat." + model)
    got = M.flat_dynamics_host(G.FLAT.index(model), d["xl"], d["dxl"], d["ul"], d["e"], d["v"])
    for key, who, g, r in G.flat_rows(model, got):
        G.check(key, g, r, who)


@pytest.mark.parametrize("name", G.AUDIT)
def test_mpc_dyn_error_of_given_plans_against_the_fixture(name):
    a = G.section("audit." + name)
    got = M.mpc_dyn_error_host(G.AUDIT_VARIANT[str(a["model"])], int(a["K"]), float(a["tf"]), float(a["t"]), a["primal"])
    G.check("audit", got[0], a["errs"], name + " host front")
    # the desired trajectories' velocities and inputs are constant in time: so is the audit of one plan
    later = M.mpc_dyn_error_host(G.AUDIT_VARIANT[str(a["model"])], int(a["K"]), float(a["tf"]), 1.7, a["primal"])
    G.check("audit", later[0], a["errs"], name + " host front, another time")
    # ... and where the desired trajectory is one of the dynamics (the rigid body's is, the vehicles' are not: their
    # desired input leaves the damping unanswered), the plan of zeros obeys them
    if str(a["model"]) == "rigid":
        assert M.mpc_dyn_error_host(13, int(a["K"]), float(a["tf"]), 0.0, np.zeros_like(a["primal"])).max() <= 1e-15


@pytest.mark.parametrize("name", G.MESHES)
def test_raised_nodes_of_the_c_abi_against_the_fixture(sfb, name):
    """sfb_mesh_raised_nodes (host only): where the caller of the batched estimate evaluates its dynamics"""
    m = G.mesh(name)
    G.check("mesh.nodes", sfb.PHMesh(m["K"], m["tau0"]).raised_nodes(), G.section("resample." + name)["tau"], name + " raised")


def test_reference_scenarios_as_caller_code():
    assert M.test_collocation_api() == 0


def test_structural_properties_on_fresh_meshes():
    for spec, ops in (((5, 10, 1, 5), [(0, 0, 50), (0, 1, 13), (0, 2, 27)]), ((3, 6, 7, 4), [(1, 0, 0)]), ((4, 4, 13, 4), [])):
        got = M.mesh_script(spec, ops)
        assert np.all(np.diff(got["nodes"]) >= 0) and got["nodes"][0] == 0.0 and got["nodes"][-1] == 1.0
        assert abs(got["weights"].sum() - 1.0) <= 1e-14
    # a cubic on <8,8> split in 5: [x_1 .. x_K] = x_0 + xdot I and xdot = x D
    got = M.mesh_script((8, 8, 1, 8), [(0, 0, 40)])
    assert got["K"].tolist() == [8] * 5
    x = lambda t: 1 + 2 * t + 3 * t ** 2 + 4 * t ** 3                              # noqa: E731
    dx = lambda t: 2 + 6 * t + 12 * t ** 2                                           # noqa: E731
    ends = np.append(got["tau0"][1:], 1.0)
    for i in range(5):
        tau = np.append(got["nodes"][8 * i:8 * i + 8], ends[i])
        assert np.allclose(x(tau) @ got["diffmat"][i], dx(tau[:-1]), rtol=0, atol=1e-11)
        assert np.allclose(x(tau[0]) + dx(tau[:-1]) @ got["intmat"][i], x(tau[1:]), rtol=0, atol=1e-13)


def test_refine_errors_leaves_the_references_case_unsplit():
    d = G.dyn("ex_ref")
    b = d["base"]
    errs = M.mesh_dyn_error_host(b["spec"], b["ops"], b["opdata"], 0, d["coef"], 3.0, 5.0, d["vals_x"], d["vals_u"])
    assert errs.shape == (16,) and errs.max() <= 1e-8
    ops = np.concatenate([b["ops"].reshape(-1, 3), [[4, 0, 0]]])
    got = M.mesh_script(b["spec"], ops, np.concatenate([[1e-8], errs]))
    assert got["K"].tolist() == [5] * 16 and np.array_equal(got["tau0"], M.mesh_script(b["spec"], b["ops"])["tau0"])
    # ... while errors above the target do refine: a higher degree, then a split
    got = M.mesh_script(b["spec"], ops, np.concatenate([[1e-8], np.where(np.arange(16) == 3, 1.0, errs)]))
    assert len(got["K"]) > 16


def test_an_instantiation_the_harness_does_not_carry_is_refused():
    with pytest.raises(LookupError):
        M.mesh_script((2, 9, 1, 2))


def _need(*tools):
    for t in tools:
        if shutil.which(t) is None:
            pytest.skip("no %s" % t)


@pytest.mark.parametrize("header", ["smooth/feedback/collocation/mesh.hpp", "smooth/feedback/collocation/dyn_error.hpp"])
def test_forwarding_headers_compile_standalone(tmp_path, header):
    _need("g++")
    src = tmp_path / "one.cpp"
    src.write_text("#include <%s>\nint main() { smooth::feedback::Mesh<5, 10> m; m.refine_ph(0, 50); return (int)m.N_ivals() - 10; }\n" % header)
    subprocess.run(["g++", "-std=c++20", "-Wall", "-fsyntax-only", "-I", INC, str(src)], check=True)
    # the old include path keeps working, with the uniform mesh the MPC path uses
    old = tmp_path / "old.cpp"
    old.write_text("#include <smooth/feedback/mesh.hpp>\nint main() { smooth::feedback::Mesh m(2, 5); smooth::feedback::UniformMesh u = m; "
                   "return u.K - 5; }\n")
    subprocess.run(["g++", "-std=c++20", "-Wall", "-fsyntax-only", "-I", INC, str(old)], check=True)


def test_sfb_h_with_the_mesh_entries_is_plain_c99(tmp_path):
    _need("gcc")
    c = tmp_path / "abi.c"
    c.write_text("#include <sfb.h>\nint main(void) { sfb_mesh m; m.nivals = 0; m.K = 0; m.tau0 = 0; "
                 "return (int)sfb_mesh_resample_batch_host(&m, 0, 0, 1, 0, 0) * 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-c", str(c), "-o", str(tmp_path / "abi.o")], check=True)


def test_argument_errors_come_before_the_device_check(sfb):
    lib, E = sfb._capi.lib, sfb._capi
    K, tau0 = np.array([3, 5], np.int32), np.array([0.0, 0.5])
    buf = np.zeros(64)
    p = lambda a: a.ctypes.data                                                     # noqa: E731

    def both(mesh, batch, dim, vals=p(buf), out=p(buf)):
        m = C.byref(mesh) if mesh is not None else None
        return {lib.sfb_mesh_resample_batch_host(m, batch, dim, 1, vals, out), lib.sfb_mesh_resample_batch(m, batch, dim, 1, vals, out, None),
                lib.sfb_mesh_dyn_error_batch_host(m, batch, dim, p(buf), vals, vals, out), lib.sfb_mesh_dyn_error_batch(m, batch, dim, p(buf), vals, vals, out, None)}

    good = sfb.PHMesh(K, tau0)
    # K + 1 > 14, K < 1, starts not at 0 / not increasing / not below 1 (the objects keep their arrays alive)
    wrong = [sfb.PHMesh([3, 13 + 1], tau0), sfb.PHMesh([0, 3], tau0), sfb.PHMesh(K, [0.1, 0.5]), sfb.PHMesh(K, [0.0, 0.0]), sfb.PHMesh(K, [0.0, 1.0])]
    bad = [(None, 1, 1), (E.SfbMesh(2, None, p(tau0)), 1, 1), (E.SfbMesh(0, p(K), p(tau0)), 1, 1)] + [(m.c, 1, 1) for m in wrong]
    bad += [(good.c, -1, 1), (good.c, 1, -1)]
    for mesh, batch, dim in bad:
        assert both(mesh, batch, dim) == {E.SFB_ERR_INVALID_ARG}, (batch, dim)
    assert both(good.c, 1, 1, vals=None) == {E.SFB_ERR_INVALID_ARG}
    assert "K" in lib.sfb_last_error().decode() or "NULL" in lib.sfb_last_error().decode()
    if E.device_count() == 0:   # well-formed calls then fail for want of a device, never compute on the CPU
        assert both(good.c, 1, 1) == {E.SFB_ERR_NO_DEVICE}
        with pytest.raises(E.SfbError) as e:
            sfb.mesh_resample_batch_host(good, np.zeros((2, 9, 3)))
        assert e.value.status == E.SFB_ERR_NO_DEVICE


SANITIZED_MAIN = r"""
#include <smooth/feedback/collocation/dyn_error.hpp>
#include <smooth/feedback/collocation/mesh.hpp>
#include <cstdio>
namespace F = smooth::feedback;
template<class M>
static int drive(M m, int rounds)
{
  unsigned s = 12345;
  auto next = [&s] { return s = s * 1664525u + 1013904223u, s >> 8; };
  for (int r = 0; r < rounds; ++r) {
    const std::size_t i = next() % m.N_ivals();
    switch (next() % 5) {
    case 0: m.refine_ph(i, M::Kmin + next() % (3 * M::Kmax)); break;
    case 1: m.increase_degrees(); break;
    case 2: m.decrease_degrees(); break;
    case 3: m.set_N_colloc_ival(i, M::Kmin + next() % (M::Kmax + 2 - M::Kmin)); break;
    default: {
      std::vector<double> e(m.N_ivals());
      for (auto & v : e) v = 1e-9 * (1 + next() % 5000);
      m.refine_errors(e, 1e-6);
    }
    }
    if (m.N_ivals() > 400) m = M();
    const auto nodes = m.all_nodes(), w = m.all_weights();
    if (nodes.size() != m.N_colloc() + 1 || w.size() != nodes.size()) return 1;
    std::vector<F::Vec<2>> vals(nodes.size());
    for (std::size_t k = 0; k < nodes.size(); ++k) vals[k] = {nodes[k], 1.0};
    const std::vector<F::Vec<2>> open(vals.begin(), vals.end() - 1);
    for (const double t : {-0.5, 0.0, 0.3, nodes[nodes.size() / 2], 1.0, 1.5})
      for (std::size_t p = 0; p < 3; ++p) {
        const auto a = m.template eval<2>(t, vals, p, true), b = m.template eval<2>(t, open, p, false);
        if (!(a[0] == a[0]) || !(b[0] == b[0])) return 2;
      }
    const auto D = m.interval_diffmat(i % m.N_ivals());
    const auto I = m.interval_intmat(i % m.N_ivals());
    if (D.rows != I.rows + 1 || m.interval_find(nodes[nodes.size() / 3]) >= m.N_ivals()) return 3;
  }
  return 0;
}
int main()
{
  const int rc = drive(F::Mesh<5, 10>(), 60) + 10 * drive(F::Mesh<3, 6>(), 60) + 100 * drive(F::Mesh<4, 4>(13), 40) + 1000 * drive(F::Mesh<1, 2>(), 40);
  std::printf("rc %d\n", rc);
  return rc;
}
"""


def test_refinement_sequences_and_eval_under_address_and_ub_sanitizers(tmp_path):
    """a stand-alone program (its own main, run directly) drives random refinement sequences and eval"""
    _need("g++")
    src, exe = tmp_path / "drive.cpp", tmp_path / "drive"
    src.write_text(SANITIZED_MAIN)
    build = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, str(src),
                            "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and any(lib in build.stderr for lib in ("-lasan", "-lubsan", "libasan", "libubsan")):
        pytest.skip("the sanitizer runtime does not link here")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
