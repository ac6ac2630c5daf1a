"""flatten_ocp on the host (include/smooth_feedback_amd/ocp_flatten.hpp, dr_exp of lie.hpp) against the high-precision fixture
tests/golden/flatten_reference.npz, within the gates of tests/flatten_gates.py; the flattened problems through ocp_to_nlp; the
scenarios of sfbx_test_flatten_api; the sanitizer build of examples/flat_ocp_selftest.cpp."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flatten_gates as G  # noqa: E402
import mesh_ref as R  # noqa: E402
from examples import models_lib as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gate_is_four_times_the_float64_restatements_error():
    worst, left = G.measure()
    assert left == [], left
    assert set(worst) == set(G.MEASURED)
    for key in sorted(worst):
        print("%-9s restatement %.2e  recorded %.2e  gate %.2e" % (key, worst[key], G.MEASURED[key], G.gate(key)))
        # the recorded figure is what this restatement delivers: within a factor of two either way on another libm
        assert 0.5 * G.MEASURED[key] <= worst[key] <= 2.0 * G.MEASURED[key], key


def test_lie_operations_within_their_gates():
    for key, who, got, ref in G.lie_rows(lambda g, op, a, w: M.flat_lie_eval(g, op, a, w)):
        G.check(key, got, ref, who)


def test_flat_node_arrays_within_their_gates():
    rows = G.node_rows(lambda name, tau, x, traj: M.flat_ocp_nodes(name, tau, x, traj))
    assert len(rows) == 2 * 10 * 4
    for key, who, got, ref in rows:
        G.check(key, got, ref, who)


def test_e_block_of_the_dynamics_at_e_zero():
    """agent 0 of each problem has e = 0: there the e block of the flat dynamics' Jacobian is df/dx - ad(f + dxl) / 2"""
    import flatten_ref as FR
    for name in G.PROBLEMS:
        p = G.problem(name)
        P = FR.PROBLEMS[name]
        nx, nu, nq, N = P.nx, P.nu, P.nq, len(G.TAU)
        xa, row = p["x"][0], p["traj"][0]
        assert not np.any(xa[1 + nq:1 + nq + (N + 1) * nx])
        got = M.flat_ocp_nodes(name, G.TAU, xa[None], row[None])
        x0 = FR.elem(P.X, row[:P.EX]); xi = row[P.EX:P.EX + nx]; u0 = row[P.EX + nx:P.EX + nx + nu]; du = row[P.EX + nx + nu:]
        for i in range(N):
            t = xa[0] * G.TAU[i]
            x = FR.rplus(P.X, x0, t * xi)
            u = [u0 + t * du + xa[1 + nq + (N + 1) * nx + i * nu:1 + nq + (N + 1) * nx + (i + 1) * nu]]
            want = P.df(t, x, u)[:, 1:1 + nx] - 0.5 * FR.ad(P.X, P.f(t, x, u) + xi)
            G.check("dF", got["dFf"][0, i][:, 1:1 + nx], want, "%s node %d: df/dx - ad(f + dxl)/2" % (name, i))
            G.check("dF", p["dFf"][0, i][:, 1:1 + nx], want, "%s node %d: the fixture" % (name, i))


@pytest.mark.parametrize("name", G.PROBLEMS)
def test_ocpnlp_of_the_flattened_problem_is_the_model_free_loop_over_the_node_arrays(name):
    """one law: OCPNLP::g / dg_dx of the flattened problem, bit for bit meshfn::ocp_nlp_assemble over the host node arrays"""
    s = M.flat_ocp_mesh(name)
    d = M.flat_ocp_sizes(name, s["N"])
    rng = np.random.default_rng(5)
    B = 3
    x = rng.uniform(-0.4, 0.4, (B, s["n"])); x[:, 0] = [1.3, 2.0, 0.7]
    x[1, 1 + d["nq"]:1 + d["nq"] + (s["N"] + 1) * d["nx"]] = 0.0
    traj = np.tile(G.problem(name)["traj"][1], (B, 1)); traj[:, d["row"] - d["nx"] - 2 * d["nu"]:] += rng.uniform(-0.2, 0.2, (B, d["nx"] + 2 * d["nu"]))
    out = M.flat_ocp_nlp_host(name, x, traj)
    assert np.all(np.isfinite(out["g"])) and np.all(np.isfinite(out["dg"])) and np.all(np.isfinite(out["df"]))
    assert np.array_equal(out["differing"], np.zeros(B, np.int64)), out["differing"]
    nodes = M.flat_ocp_nodes(name, s["taus"][:-1], x, traj)
    assert np.array_equal(out["f"], nodes["theta"]) and np.array_equal(out["df"], nodes["dtheta"])


def test_flatten_api_scenarios():
    """a flattened Rn problem against its original, the unflatten round trip, d2l_dx2 against differences of the gradient, a
    Spline adapted as a trajectory"""
    code, fig = M.test_flatten_api()
    print("Rn problem: |g| %.2e |dg| %.2e |f| %.2e   round trip %.2e   d2l %.2e (max |H| %.2e)   spline velocity %.2e" % tuple(fig[:7]))
    assert code == 0, code


def test_sanitizer_selftest_builds_and_passes(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++"
    exe = str(tmp_path / "flat_ocp_selftest")
    subprocess.check_call([cxx, "-O0", "-std=c++20", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "examples"),
                           os.path.join(ROOT, "examples", "flat_ocp_selftest.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
