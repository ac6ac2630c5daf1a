"""Times the batched PID kernels on one GPU (HIP events, median and min-max of 15 launches after warm-up):
  step     sfb_pid_step_batch at AGENTS SE3 agents: time, bytes moved / time
  rollout  sfb_pid_rollout_batch at AGENTS SE3 agents x TICKS ticks: time, agent-ticks per second
  unfused  the same TICKS ticks on a SAMPLE-agent sample as TICKS step launches with the double-integrator step on the host
           in between (numpy, tests/pid_ref.py), host clock: what the fused launch saves
Usage: python scripts/pid_time.py [--agents N] [--ticks T] [--sample S] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1 << 20)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--sample", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import smooth_feedback_amd as sfb
    import pid_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("pid_time.py needs a GPU")
    parts = [("SE3", 6)]
    rng = np.random.default_rng(0)
    B = a.agents

    def poses(n):
        q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
        return np.concatenate([rng.uniform(-2, 2, (n, 3)), q], axis=1)
    host = dict(x=poses(B), v=rng.uniform(-0.3, 0.3, (B, 6)), g0=poses(B), w=rng.uniform(-0.4, 0.4, (B, 6)), a=np.zeros((B, 6)),
                kp=rng.uniform(0.5, 4, (B, 6)), kd=rng.uniform(2, 4, (B, 6)), ki=rng.uniform(0.1, 0.5, (B, 6)), ie=np.zeros((B, 6)),
                tl=np.full(B, np.nan), u=np.zeros((B, 6)), cost=np.zeros(B))
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    p = {k: v.data_ptr() for k, v in dev.items()}
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))

    res = dict(agents=B, ticks=a.ticks, device=torch.cuda.get_device_name(0))
    step = lambda: sfb.pid_step_batch_device(parts, B, 1.0, p["x"], p["v"], p["g0"], p["w"], p["a"], 0, p["kp"], p["kd"], p["ki"], 0, 0.5, p["ie"],
                                             p["tl"], p["u"], stream)
    res["step"] = timed(step)
    step_bytes = B * 8 * (7 + 6 + 7 + 6 + 6 + 18 + 6 + 1 + 6 + 1 + 6)        # read x v g_des v_des a_des gains i_err t_last, write i_err t_last u
    res["step"]["bytes"] = step_bytes
    res["step"]["TB_per_s"] = step_bytes / (res["step"]["median_ms"] * 1e-3) / 1e12
    x0, v0 = dev["x"].clone(), dev["v"].clone()

    def roll():
        dev["x"].copy_(x0); dev["v"].copy_(v0); dev["ie"].zero_(); dev["tl"].fill_(float("nan"))
    def rollout():
        sfb.pid_rollout_batch_device(parts, B, 0.0, 0.05, a.ticks, p["x"], p["v"], p["g0"], p["w"], 0, p["kp"], p["kd"], p["ki"], 0, 0.5, 0, p["ie"],
                                     p["tl"], p["u"], p["cost"], stream)
    ms = []
    for rep in range(a.reps + 2):                      # the state is restored outside the timed window
        roll()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); rollout(); e1.record()
        torch.cuda.synchronize()
        if rep >= 2:
            ms.append(e0.elapsed_time(e1))
    res["rollout"] = dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))
    res["rollout"]["agent_ticks_per_s"] = B * a.ticks / (res["rollout"]["median_ms"] * 1e-3)
    assert bool(torch.isfinite(dev["cost"]).all())

    S = a.sample
    hs = {k: v[:S].copy() for k, v in host.items()}
    t0 = time.perf_counter()
    x, v, ie, tl = hs["x"], hs["v"], hs["ie"], hs["tl"]
    for k in range(a.ticks):
        t = 0.05 * k
        gd = np.array([R.store(parts, R.rplus(parts, R.load(parts, g), t * w)) for g, w in zip(hs["g0"], hs["w"])])
        u, ie, tl = sfb.pid_step_batch_host(parts, t, x, v, gd, hs["w"], hs["a"], hs["kp"], hs["kd"], hs["ki"], ie, tl, windup_limit=0.5)
        x, v = R.integrate(parts, x, v, u, 0.05)
    res["unfused_sample"] = dict(agents=S, seconds=time.perf_counter() - t0)
    fused = sfb.pid_rollout_batch_host(parts, 0.0, 0.05, a.ticks, hs["x"], hs["v"], hs["g0"], hs["w"], hs["kp"], hs["kd"], hs["ki"], hs["ie"], hs["tl"],
                                       windup_limit=0.5)
    t1 = time.perf_counter()
    sfb.pid_rollout_batch_host(parts, 0.0, 0.05, a.ticks, hs["x"], hs["v"], hs["g0"], hs["w"], hs["kp"], hs["kd"], hs["ki"], hs["ie"], hs["tl"], windup_limit=0.5)
    res["fused_sample"] = dict(agents=S, seconds=time.perf_counter() - t1, max_dv_vs_unfused=float(np.max(np.abs(fused["v"] - v))))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
