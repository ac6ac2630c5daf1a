"""Time of FlatOCPSwarmDevice::eval (include/smooth_feedback_amd/ocp_flatten_device.hpp) against the path it replaces
(DESIGN.md 6h): python scripts/flat_ocp_time.py [agents] [problem] [reps] [threads].
Default: 8 192 agents of the planar vehicle on Bundle<SE2, Rn<2>> (examples/ocp_se2_model.h) on the 13 x 4 mesh, every agent
around its own trajectory.  The two halves of eval() are timed apart between device events, warmed, the least of `reps` runs each:
flat_ocp_nodes_kernel (model and change of variables at the nodes) and sfb_ocp_nlp_batch (the model-free assembly).  The
comparison is the host front on `threads` threads (16) filling the same node arrays (wall clock, the least of three), followed
by sfb_ocp_nlp_batch_host, which stages them through PCIe (wall clock, the least of three).  The kernel's bandwidth is its
algorithmic traffic -- x and the trajectory rows read once, every node array written once -- over its time.  Needs a device."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    a = [int(v) if v.isdigit() else v for v in sys.argv[1:]]
    a += [8192, "se2", 10, 16][len(a):]
    B, name, reps, threads = a
    import smooth_feedback_amd as sfb
    from examples import models_lib as M
    if sfb._capi.device_count() < 1:
        raise RuntimeError("flat_ocp_time.py needs a HIP device")
    s = M.flat_ocp_mesh(name, 1)
    d = M.flat_ocp_sizes(name, s["N"])
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.3, 0.3, (B, s["n"])); x[:, 0] = rng.uniform(1.0, 3.0, B)
    EX = d["row"] - d["nx"] - 2 * d["nu"]
    traj = rng.uniform(-0.5, 0.5, (B, d["row"]))
    if name == "se2":
        th = rng.uniform(-3, 3, B); traj[:, 2], traj[:, 3] = np.cos(th), np.sin(th)
    else:
        q = rng.normal(size=(B, 4)); traj[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    dev = M.flat_ocp_front_device(name, x, traj, mesh_kind=1, reps=reps)
    t_nodes, t_nlp = [float(v) for v in dev["seconds"]]
    N, nz, ne = s["N"], d["nz"], d["ne"]
    nf = d["nx"] + d["nq"] + d["ncr"]
    bytes_nodes = 8 * B * (s["n"] + d["row"] + N * nf * (1 + nz) + (d["nce"] + 1) * (1 + ne))
    host_nodes, host_nlp = [], []
    dims = (d["nx"], d["nu"], d["nq"], d["ncr"], d["nce"])
    mesh = sfb.PHMesh.uniform(13, 4)
    for _ in range(3):
        t0 = time.perf_counter()
        hn = M.flat_ocp_nodes(name, s["taus"][:-1], x, traj, threads=threads)
        t1 = time.perf_counter()
        g, dg = sfb.mesh.ocp_nlp_batch_host(mesh, dims, x, *[hn[k] for k in M.FLAT_NODE_KEYS[:8]])
        t2 = time.perf_counter()
        host_nodes.append(t1 - t0); host_nlp.append(t2 - t1)
    import mesh_ref as R
    err = R.scaled_error(dev["g"].ravel(), g.ravel())
    out = dict(agents=B, problem=name, mesh="13x4", n=s["n"], m=s["m"], nnz=s["nnz"], node_kernel_ms=1e3 * t_nodes, nlp_batch_ms=1e3 * t_nlp,
               eval_ms=1e3 * (t_nodes + t_nlp), node_kernel_bytes=bytes_nodes, node_kernel_GBps=bytes_nodes / t_nodes / 1e9,
               host_nodes_ms=1e3 * min(host_nodes), host_threads=threads, host_nlp_batch_ms=1e3 * min(host_nlp),
               host_path_ms=1e3 * (min(host_nodes) + min(host_nlp)), g_device_vs_host_scaled_error=err)
    print("agents %d  %s  mesh 13 x 4  n %d  m %d  nnz %d" % (B, name, s["n"], s["m"], s["nnz"]))
    print("device: node kernel %.3f ms (%.1f MB, %.0f GB/s)  sfb_ocp_nlp_batch %.3f ms  eval %.3f ms" %
          (out["node_kernel_ms"], bytes_nodes / 1e6, out["node_kernel_GBps"], out["nlp_batch_ms"], out["eval_ms"]))
    print("host:   node arrays on %d threads %.1f ms  sfb_ocp_nlp_batch_host %.1f ms  together %.1f ms" %
          (threads, out["host_nodes_ms"], out["host_nlp_batch_ms"], out["host_path_ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    main()
