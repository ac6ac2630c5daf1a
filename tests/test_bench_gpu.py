"""bench.py contract on a GPU box: one JSON line with the required keys (N = 1), and the N > 1 code path
(barrier, gather of the small outputs, max-over-ranks timing) with two ranks sharing cuda:0 over gloo
(SFB_BENCH_SHARE_DEVICE=1; the driver runs the real thing over RCCL on 8 GPUs)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline"}


def _last_json(out):
    lines = [l for l in out.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_single_gpu_line_has_roofline_and_cpu_baseline():
    out = subprocess.run([sys.executable, "bench.py", "--workload", "qp_dense", "--batch", "8192", "--steps", "2",
                          "--warmup", "1", "--full"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    assert KEYS <= set(d) and {"cpu_baseline", "parity_vs_oracle"} <= set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["dtype"] == "f64" and d["value"] > 0
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(d["roofline"])
    assert {"value", "unit", "cores", "kind", "sample"} <= set(d["cpu_baseline"])
    assert d["parity_vs_oracle"]["code_mismatches"] == 0 and d["parity_vs_oracle"]["iter_mismatches"] == 0
    assert d["parity_vs_oracle"]["max_abs_dx"] <= 1e-8


def test_plain_line_is_the_headline_and_dumps_the_last_step(tmp_path):
    """Without --full the line carries the headline only; --dump-outputs writes what the last timed step returned, as
    float64, and equals the oracle's solution of the same seeded QPs."""
    import numpy as np
    out = subprocess.run([sys.executable, "bench.py", "--workload", "qp_dense", "--batch", "4096", "--steps", "3",
                          "--warmup", "1", "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    assert KEYS <= set(d) and d["steps"] == 3 and d["ms_per_step"] > 0
    assert not {"cpu_baseline", "parity_vs_oracle", "secondary", "pipelined", "closed_loop"} & set(d)
    got = {k: np.load(tmp_path / (k + ".npy")) for k in ("x", "y", "obj", "iter", "code")}
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(k + ".npy" for k in got)
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["x"].shape == (4096, 10) and got["y"].shape == (4096, 20) and got["iter"].shape == (4096,)
    sys.path.insert(0, ROOT)
    import smooth_feedback_amd as sfb
    from oracle import loader as O
    P, q, A, l, u = sfb.random_qp_batch(5, 4096, 20, 10, 1.0)  # rank 0's batch of the bench's dense workload
    S = 256
    ref = O.qp_dense_solve_batch(P[:S], q[:S], A[:S], l[:S], u[:S], nthreads=4,
                                 params=O.default_params(eps_abs=1e-6, eps_rel=1e-6, polish=1, max_iter=10000, scaling=0))
    assert np.array_equal(got["code"][:S], ref["code"]) and np.array_equal(got["iter"][:S], ref["iter"])
    fin = np.isfinite(ref["x"]).all(axis=1)
    assert np.abs(got["x"][:S] - ref["x"])[fin].max(initial=0.0) <= 1e-8


@pytest.mark.parametrize("workload,batch,port", [("qp_dense", 4096, 29533), ("mpc", 96, 29541), ("ekf", 70000, 29549)])
def test_two_ranks_code_path(workload, batch, port):
    """Every workload through the N > 1 path: per-rank shard, barrier, ONE gather of the small per-item outputs per
    step (for mpc: u_0, code, iter sliced out of the solution), max-over-ranks timing; rank 0 checks that its own
    rows come back from the gather unchanged and that the other rank's rows reproduce that rank's checksum."""
    env = dict(os.environ, SFB_BENCH_SHARE_DEVICE="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2",
                          "--workload", workload, "--batch", str(batch), "--steps", "2", "--warmup", "1"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    assert KEYS <= set(d)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 2 * batch and d["config"]["per_gpu_batch"] == batch
    assert d["value"] > 0 and "cpu_baseline" not in d and "secondary" not in d
    assert d["gather_check"] == {"own_rows_intact": True, "peer_rows_received": True, "peer_rows_differ_from_own": True,
                                 "gathered_rows": 2 * batch, "ranks_checked": 2}


def test_eight_ranks_mpc_code_path():
    """The shape of BASELINE configs[3] (8 ranks, one shard of MPC agents each, ONE gather of u_0 / code / iter per
    step) with all ranks on cuda:0 over gloo: sharding.shard_range over the job's batch, rank-derived seeds, host assembly threads divided among the
    ranks, the gather checked against per-rank checksums that travel by a separate all_reduce."""
    env = dict(os.environ, SFB_BENCH_SHARE_DEVICE="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8",
                          "--master-addr", "127.0.0.1", "--master-port", "29557", "bench.py", "--gpus", "8",
                          "--workload", "mpc", "--batch", "64", "--steps", "2", "--warmup", "1"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    assert d["n_gpus"] == 8 and d["scaling"] == "weak" and d["config"]["global_batch"] == 8 * 64
    assert d["gather_check"] == {"own_rows_intact": True, "peer_rows_received": True, "peer_rows_differ_from_own": True,
                                 "gathered_rows": 8 * 64, "ranks_checked": 8}


def test_default_line_carries_the_secondary_workloads():
    """The driver's command with --full: headline = BASELINE configs[2], plus the other two configurations under
    `secondary`, each with its own roofline, CPU baseline and parity figures; the dense one with the FP64-VALU view."""
    out = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--full"], cwd=ROOT, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    assert d["config"]["workload"].startswith("mpc_qp_nx12_nu2_K50_b8192")
    assert set(d["secondary"]) == {"qp_dense", "ekf", "qp_dense_sizes"}
    sizes = d["secondary"].pop("qp_dense_sizes")
    assert {(r["n"], r["m"]) for r in sizes} == {(10, 20), (16, 32), (20, 40), (32, 32), (32, 64), (40, 60), (64, 64)}
    for r in sizes:   # every size of the north star's class: measured, and bit-identical to the oracle on its sample
        assert r["qp_per_s"] > 0 and r["parity_vs_oracle"] == {"sample": r["parity_vs_oracle"]["sample"], "code_mismatches": 0,
                                                                "iter_mismatches": 0, "max_abs_dx": 0.0}
    for k, v in d["secondary"].items():
        assert v["value"] > 0 and {"bound", "achieved", "peak", "frac", "traffic", "kernel_ms"} <= set(v["roofline"])
        assert "cpu_baseline" in v and "parity_vs_oracle" in v
    assert d["secondary"]["qp_dense"]["roofline_alt"]["bound"] == "fp64_valu"
    assert d["secondary"]["ekf"]["parity_vs_oracle"]["P_bit_identical"]
    assert d["parity_vs_oracle"]["iter_mismatches"] == 0 and d["parity_vs_oracle"]["max_abs_dx"] == 0.0
    assert d["cpu_baseline"]["single_core"]["cores"] == 1
    # what a user of MPC::operator() sees (end-to-end incl. H2D), driver-timed in the same run
    cl = d["closed_loop"]
    assert cl["end_to_end"]["results_identical_to_device_resident"] and cl["end_to_end"]["value"] > 0
    assert cl["swarm_tick"]["agents"] == 8192 and cl["swarm_tick"]["ms_per_tick"] > 0 and cl["swarm_tick"]["optimal_fraction_last_tick"] == 1.0
    assert cl["single_agent"]["cold_ms"] > 0 and cl["single_agent"]["warm_iterations"] <= cl["single_agent"]["cold_iterations"]
    ekf_cpu = d["secondary"]["ekf"]["cpu_baseline"]
    assert ekf_cpu["single_core"]["cores"] == 1 and d["secondary"]["ekf"]["parity_vs_oracle"].get("all_cores_P_bit_identical", True)


@pytest.mark.parametrize("workload,batch,dtype,port", [("mpc", 96, "float64", 29565), ("qp_dense", 4096, "int32", 29573)])
def test_rccl_carries_the_collectives_of_the_n_gpu_path(workload, batch, dtype, port):
    """The `nccl` (= RCCL) branch of bench.py on the one GPU there is: one rank under torch.distributed.run, process group on
    RCCL with the device bound, and every collective of the N > 1 path issued for real (SFB_BENCH_FORCE_COLLECTIVES=1: the
    world-of-one shortcut of sharding.gather_small_outputs is bypassed) -- all_gather of the small per-item outputs (float64
    (batch, 4) rows of u0 / code / iter for mpc, int32 (batch, 2) for the dense QPs), the int64 checksum all_reduce, the
    barrier, the float64 MAX all_reduce of the elapsed time.  What an 8-GPU run adds is peers, not code."""
    env = dict(os.environ, SFB_BENCH_FORCE_COLLECTIVES="1")
    env.pop("SFB_BENCH_SHARE_DEVICE", None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "1",
                          "--workload", workload, "--batch", str(batch), "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                          "--no-pipelined", "--no-secondary", "--no-closed-loop"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    assert d["n_gpus"] == 1 and d["value"] > 0
    assert d["gather_check"] == {"own_rows_intact": True, "peer_rows_received": True, "peer_rows_differ_from_own": True,
                                 "gathered_rows": batch, "ranks_checked": 1, "backend": "nccl", "gathered_dtype": dtype,
                                 "checksum_via_all_reduce_matches": True}


def _run_rccl_ranks(world, B, port, timeout=240):
    """tests/helpers/rccl_ranks.py under torch.distributed.run in a session of its own (a hung rendezvous is ended by killing
    exactly that process group)."""
    import signal
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.Popen([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                          "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "helpers", "rccl_ranks.py"), str(B)],
                         cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = p.communicate(timeout=timeout)
        timed_out = False
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, err = p.communicate()
        timed_out = True
    rows = [json.loads(ln[len("RCCL_RANKS "):]) for ln in out.splitlines() if ln.startswith("RCCL_RANKS ")]
    return rows, timed_out, err


def _record(name, payload):
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", name), "w") as f:
        json.dump(payload, f, indent=1)


def test_rccl_unequal_shards_through_the_padding_path():
    """sharding.gather_small_outputs(force=True) on RCCL with total = 2 B + 1 rows: the padded all_gather and the trimming of
    sharding.py:27-31 on the real backend (one rank on the one GPU: its shard is the whole odd-sized batch), plus the checksum
    and MAX all_reduce of bench.py."""
    rows, timed_out, err = _run_rccl_ranks(1, 48, 29581)
    _record("rccl_one_rank_unequal.json", {"rows": rows, "timed_out": timed_out, "stderr_tail": err[-1500:]})
    assert not timed_out and len(rows) == 1, err[-2000:]
    r = rows[0]
    assert "error" not in r, r
    assert r["gathered_rows"] == 97 and r["gather_exact"] and r["checksum_ok"] and r["max_ok"]


def test_rccl_two_ranks_one_device():
    """TWO ranks, both bound to cuda:0, process group on nccl: more than one RCCL peer on the hardware there is.  RCCL may refuse
    duplicate devices (NCCL does: "Duplicate GPU detected"); then the refusal's text is the record (gpurun_out/
    rccl_two_ranks_one_device.json, quoted in DESIGN section 7) and the gloo variants (tests/test_sharding_gloo.py, the 2- and
    8-rank bench runs on one device above) stay the coverage of N > 1.  If it accepts them: shards of 49 and 48 rows through
    the padded all_gather, the checksum and the MAX all_reduce must be exact on both ranks."""
    rows, timed_out, err = _run_rccl_ranks(2, 48, 29583)
    refused = timed_out or len(rows) < 2 or any("error" in r for r in rows)
    _record("rccl_two_ranks_one_device.json", {"accepted": not refused, "rows": rows, "timed_out": timed_out, "stderr_tail": err[-3000:]})
    if refused:
        text = " ".join(r.get("error", "") for r in rows) + err
        # a refusal must be RCCL's own (duplicate device / invalid usage / a rendezvous that never completes), not a bug of ours
        assert timed_out or any(k in text for k in ("Duplicate GPU", "duplicate", "invalid usage", "ncclInvalidUsage", "NCCL error",
                                                    "ncclUnhandledCudaError", "ncclSystemError", "DistBackendError")), text[-3000:]
        return
    assert sorted(r["shard_rows"] for r in rows) == [48, 49]
    for r in rows:
        assert r["gathered_rows"] == 97 and r["gather_exact"] and r["checksum_ok"] and r["max_ok"], r
