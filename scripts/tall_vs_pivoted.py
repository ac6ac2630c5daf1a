"""Times sfb_qp_dense_solve_batch (the pivoted route) and sfb_qp_dense_tall_solve_batch (the reduced-KKT route) on the SAME
device buffers, in one run, with HIP events after warm-up:
    (3, 203) polish = false at batch 1, 2 048, 8 192 and (4, 301) with default parameters at 2 048.
Prints per point the median and the min-max range of REPS timed launches of each route, the ratio of the medians, and whether
the two ranges are disjoint.  Usage: python scripts/tall_vs_pivoted.py [--reps 15] [--only-tall N M B]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import smooth_feedback_amd as sfb  # noqa: E402
import qp_families as QF  # noqa: E402


def buffers(n, m, B, seed=1):
    _, (P, q, A, l, u) = QF.build("pd_mixed", B, n, m, seed=seed)
    dev = torch.device("cuda:0")
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (P, q, A, l, u)]
    out = [torch.empty((B, n), dtype=torch.float64, device=dev), torch.empty((B, m), dtype=torch.float64, device=dev),
           torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
           torch.empty(B, dtype=torch.int32, device=dev)]
    return d, out


def time_route(fn, B, n, m, d, out, prm, reps, warmup=3):
    st = torch.cuda.current_stream().cuda_stream
    args = [B, n, m, *[a.data_ptr() for a in d], *[a.data_ptr() for a in out]]
    for _ in range(warmup):
        fn(*args, prm, stream=st)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*args, prm, stream=st)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return np.asarray(ms), out[3].cpu().numpy().astype(np.int64), out[4].cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only-tall", type=int, nargs=3, metavar=("N", "M", "B"), help="one point, the new route only (for a profiler)")
    a = ap.parse_args()
    if a.only_tall:
        n, m, B = a.only_tall
        d, out = buffers(n, m, B)
        ms, it, code = time_route(sfb.solve_qp_tall_batch_device, B, n, m, d, out, sfb.QPSolverParams(polish=False), a.reps)
        print("tall (%d, %d) x %d: median %.3f ms" % (n, m, B, np.median(ms)))
        return
    print("| n, m | batch | parameters | pivoted route ms (median, min-max) | reduced-KKT route ms (median, min-max) | ratio | ranges disjoint | mean iterations (pivoted / reduced) |")
    print("|---|---|---|---|---|---|---|---|")
    for n, m, B, polish in ((3, 203, 1, False), (3, 203, 2048, False), (3, 203, 8192, False), (4, 301, 2048, True)):
        prm = sfb.QPSolverParams(polish=polish)
        d, out = buffers(n, m, B)
        o_ms, o_it, o_code = time_route(sfb.solve_qp_batch_device, B, n, m, d, out, prm, a.reps)
        t_ms, t_it, t_code = time_route(sfb.solve_qp_tall_batch_device, B, n, m, d, out, prm, a.reps)
        print("| %d, %d | %d | %s | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.1fx | %s | %.1f / %.1f |" % (
            n, m, B, "defaults" if polish else "polish = false", np.median(o_ms), o_ms.min(), o_ms.max(), np.median(t_ms), t_ms.min(),
            t_ms.max(), np.median(o_ms) / np.median(t_ms), "yes" if t_ms.max() < o_ms.min() else "NO", o_it.mean(), t_it.mean()), flush=True)
        assert np.array_equal(o_code, t_code), "status codes of the two routes differ"


if __name__ == "__main__":
    main()
