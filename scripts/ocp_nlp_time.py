"""Time of the fused sfb_ocp_nlp_batch against the composition it replaces:
python scripts/ocp_nlp_time.py [agents] [intervals] [K] [nx] [nu] [nq] [ncr] [nce].
Default: 8 192 agents on the MPC's 13 x 4 mesh, nx = 12, nu = 2, nq = 1, ncr = 2, nce = 12.  Device tensors between device
events, warmed; each of five windows holds ten calls, and the least window is reported per call.  The two are timed alternately
in the same process: the fused entry, and the composition available before it -- sfb_mesh_dyn_batch, the weight-scaled
sfb_mesh_eval_batch and sfb_mesh_integrate_batch with t0 = 0, then a torch gather through a precomputed index (which drops the
t0 entries and re-orders; one per segment of the pattern, because the segments are contiguous runs of dg with one source array
each), the product with ws, and the -ws and ce entries written with torch.  The spread is the largest minus the least window of each; the fused call has to win by more than both.  The whole thing
is repeated in three fresh processes (this script starts them one after the other and touches no device itself).  The bandwidth
is the least possible traffic of the fused call -- every input read once, every output written once, the per-mesh tables not
counted -- over its time.  NLP_AGENTS=k in the environment sets the library's knob SFB_NLP_AGENTS (agents a lane walks with one
decoded item) for an A/B run."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(B, nivals, K, nx, nu, nq, ncr, nce):
    import numpy as np
    import torch

    import smooth_feedback_amd as sfb

    if os.environ.get("NLP_AGENTS"):
        sfb.debug_set("SFB_NLP_AGENTS", os.environ["NLP_AGENTS"])
    mesh = sfb.PHMesh.uniform(nivals, K)
    dims = (nx, nu, nq, ncr, nce)
    N, nz = mesh.N, 1 + nx + nu
    vb, cb = sfb.ocp_nlp_structure(mesh, dims)
    n, m = int(vb[4]), int(cb[4])
    rowptr, colind = sfb.ocp_nlp_pattern(mesh, dims)
    nnz = len(colind)
    ws = sfb.ocp_nlp_bounds(mesh, dims, np.zeros(ncr), np.zeros(ncr), np.zeros(nce), np.zeros(nce))[4]
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.rand(*s, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1    # noqa: E731
    x = rnd(B, n)
    x[:, 0] = 2.0 + 0.1 * x[:, 0]
    Ff, dFf, Fg, dFg, Fcr, dFcr = rnd(B, N, nx), rnd(B, N, nx, nz), rnd(B, N, nq), rnd(B, N, nq, nz), rnd(B, N, ncr), rnd(B, N, ncr, nz)
    ce, dce = rnd(B, nce), rnd(B, nce, 1 + 2 * nx + nq)
    g = torch.empty((B, m), dtype=torch.float64, device="cuda")
    dg = torch.empty((B, nnz), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr() if t.numel() else 0                                  # noqa: E731

    def fused():
        sfb.ocp_nlp_batch_device(mesh, dims, B, p(x), p(Ff), p(dFf), p(Fg), p(dFg), p(Fcr), p(dFcr), p(ce), p(dce), p(g), p(dg), stream=stream)

    # ---- the composition: per segment of the pattern (its rows are [dyn | integrals | running | end], so every segment's entries
    # are one contiguous run of dg with one source array) a gather through a precomputed index and the product with the scale
    old = 2 + nx * (N + 1) + nu * N
    to_new = np.concatenate([[-1, 0], vb[2] + np.arange(nx * (N + 1)), vb[3] + np.arange(nu * N)])
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    seg_of = np.searchsorted(cb[1:4], rows, side="right")                           # 0 dyn, 1 integrals, 2 running, 3 end
    dyn_rp, dyn_ci = sfb.mesh_dyn_pattern(mesh, nx, nu)
    ev_rp, ev_ci = sfb.mesh_eval_pattern(mesh, nx, nu, ncr) if ncr else (np.zeros(1, np.int32), np.zeros(0, np.int32))
    where = [{}, {}, {}, {}]
    for r in range(N * nx):
        for e in range(dyn_rp[r], dyn_rp[r + 1]):
            where[0][(r, to_new[dyn_ci[e]])] = e
    for r in range(nq):
        for c in range(old):
            where[1][(cb[1] + r, to_new[c])] = r * old + c
        where[1][(cb[1] + r, vb[1] + r)] = r * old                                 # (the t0 entry's slot: any finite number, the scale is set below)
    for r in range(N * ncr):
        for e in range(ev_rp[r], ev_rp[r + 1]):
            where[2][(cb[2] + r, to_new[ev_ci[e]])] = e
    end_new = np.concatenate([[0], vb[2] + np.arange(nx), vb[2] + N * nx + np.arange(nx), vb[1] + np.arange(nq)])
    for r in range(nce):
        for k, c in enumerate(end_new):
            where[3][(cb[3] + r, c)] = r * len(end_new) + k
    segs = []
    for sgm in range(4):
        sel = np.nonzero(seg_of == sgm)[0]
        if len(sel) == 0:
            continue
        idx = np.array([where[sgm][(rows[e], colind[e])] for e in sel], dtype=np.int64)
        sc = np.full(len(sel), 1.0 if sgm == 3 else ws)
        isq = (colind[sel] >= vb[1]) & (colind[sel] < vb[2]) if sgm == 1 else np.zeros(len(sel), bool)
        segs.append((sgm, int(sel[0]), int(sel[-1]) + 1, torch.from_numpy(idx).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(np.nonzero(isq)[0]).cuda()))
    t0, tf = torch.zeros(B, dtype=torch.float64, device="cuda"), x[:, 0].contiguous()
    X = x[:, vb[2]:vb[3]].contiguous()
    new = lambda k: torch.empty((B, k), dtype=torch.float64, device="cuda")          # noqa: E731
    F_dyn, F_ev, F_int, d_dyn, d_ev, d_int = new(N * nx), new(N * ncr), new(nq), new(len(dyn_ci)), new(len(ev_ci)), new(nq * old)
    g2, dg2 = new(m), new(nnz)
    dce_flat = dce.reshape(B, -1)

    def composed():
        sfb.mesh_dyn_batch_device(mesh, B, nx, nu, p(t0), p(tf), p(X), p(Ff), p(dFf), p(F_dyn), p(d_dyn), stream=stream)
        if ncr:
            sfb.mesh_eval_batch_device(mesh, B, nx, nu, ncr, True, p(t0), p(tf), p(Fcr), p(dFcr), p(F_ev), p(d_ev), stream=stream)
        if nq:
            sfb.mesh_integrate_batch_device(mesh, B, nx, nu, nq, p(t0), p(tf), p(Fg), p(dFg), p(F_int), p(d_int), stream=stream)
        for sgm, lo, hi, idx, sc, isq in segs:
            src = (d_dyn, d_int, d_ev, dce_flat)[sgm]
            torch.mul(torch.index_select(src, 1, idx), sc, out=dg2[:, lo:hi])
            if sgm == 1:
                dg2[:, lo + isq] = -ws
        g2[:, :cb[1]] = ws * F_dyn
        g2[:, cb[1]:cb[2]] = ws * (F_int - x[:, vb[1]:vb[2]])
        g2[:, cb[2]:cb[3]] = ws * F_ev
        g2[:, cb[3]:] = ce

    def window(call, calls=10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    for _ in range(5):
        fused()
        composed()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(dg).all())
    err = max(float((g - g2).abs().max()), float((dg - dg2).abs().max()))
    assert err < 1e-9, err                                                          # the two compute the same thing
    wf, wc = [], []
    for _ in range(5):                                                              # alternating
        wf.append(window(fused))
        wc.append(window(composed))
    read = 8 * sum(t.numel() for t in (x, Ff, dFf, Fg, dFg, Fcr, dFcr, ce, dce))
    written = 8 * (g.numel() + dg.numel())
    ms, msc = min(wf), min(wc)
    print("agents %d  mesh %d x %d  dims %s  n %d  m %d  nnz %d" % (B, nivals, K, dims, n, m, nnz))
    print("  fused    %.4f ms per call (windows %s, spread %.4f)   read %.1f MB  written %.1f MB   %.0f GB/s"
          % (ms, " ".join("%.4f" % w for w in wf), max(wf) - ms, read / 1e6, written / 1e6, (read + written) / ms / 1e6))
    print("  composed %.4f ms per call (windows %s, spread %.4f)   fused is %.4f ms less, %.2fx;  largest difference of the two results %.1e"
          % (msc, " ".join("%.4f" % w for w in wc), max(wc) - msc, msc - ms, msc / ms, err), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*[int(v) for v in sys.argv[2:10]])
    else:
        a = [int(v) for v in sys.argv[1:9]]
        a += [8192, 13, 4, 12, 2, 1, 2, 12][len(a):]
        for rep in range(3):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(v) for v in a], check=True, timeout=300)
