"""Time of the fused sfb_ocp_nlp_hess_batch against what a caller can write in torch without it:
python scripts/ocp_nlp_hess_time.py [agents] [intervals] [K] [nx] [nu] [nq] [ncr] [nce].
Default: 8 192 agents on the MPC's 13 x 4 mesh, nx = 12, nu = 2, nq = 1, ncr = 2, nce = 12.  Device tensors between device
events, warmed; each of five windows holds ten calls, and the least window is reported per call.  The two are timed alternately
in the same process: the fused entry, and the torch baseline -- index maps precomputed from the same gather records (entry ->
node and position in its (t | x | u) block, entry -> position in the end block), the node blocks scaled in torch (w h, the
powers of tau of the tf row and column, ws), the JL = sum_j lambda_j dF(j, c) contraction with einsum added to the tf row, the
end blocks sigma d2theta + d2ce_l, and both added into the value array with index_add_.  The spread is the largest minus the
least window of each.  The whole thing is repeated in three fresh processes (this script starts them one after the other and
touches no device itself).  The bandwidth is the least possible traffic of the fused call -- every array it reads read once
in full (tf of x, lambda, sigma, dFf, dFg, the three HL, the two end blocks), every output written once, the per-mesh tables
not counted -- over its time.  NLP_HESS_AGENTS=k in the environment sets the library's knob SFB_NLP_HESS_AGENTS (agents a lane
walks with one decoded record) for an A/B run; --one runs a single process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def records(np, colptr, rowind, vb, N, nx, nu, nq):
    """per entry of the pattern: its node (-1 none, -2 all), the flat position a nz + b in a node's block, the flat position in
    the (tf | x0 | xf | q) block (-1 none) -- the gather records of meshfn::ocp_nlp_hess_pattern, rebuilt from the pattern"""
    nz, ne = 1 + nx + nu, 1 + 2 * nx + nq

    def node_pos(v):                                                                # variable -> (node, position in z) or None
        if v == 0:
            return (-2, 0)
        if vb[2] <= v < vb[2] + nx * N:
            return ((v - vb[2]) // nx, 1 + (v - vb[2]) % nx)
        if v >= vb[3]:
            return ((v - vb[3]) // nu, 1 + nx + (v - vb[3]) % nu)
        return None

    def end_pos(v):
        if v == 0:
            return 0
        if vb[1] <= v < vb[2]:
            return 1 + 2 * nx + v - vb[1]
        if vb[2] <= v < vb[2] + nx:
            return 1 + v - vb[2]
        if vb[2] + nx * N <= v < vb[3]:
            return 1 + nx + v - vb[2] - nx * N
        return None

    cols = np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))
    node, pos, end = [], [], []
    for r, c in zip(rowind, cols):
        a, b = node_pos(int(r)), node_pos(int(c))
        i = -1
        if a is not None and b is not None and (a[0] == b[0] or a[0] == -2):
            i = b[0]
        node.append(i)
        pos.append(a[1] * nz + b[1] if i != -1 else 0)
        ea, eb = end_pos(int(r)), end_pos(int(c))
        end.append(ea * ne + eb if ea is not None and eb is not None else -1)
    return np.array(node), np.array(pos), np.array(end)


def child(B, nivals, K, nx, nu, nq, ncr, nce):
    import numpy as np
    import torch

    import smooth_feedback_amd as sfb

    if os.environ.get("NLP_HESS_AGENTS"):
        sfb.debug_set("SFB_NLP_HESS_AGENTS", os.environ["NLP_HESS_AGENTS"])
    mesh = sfb.PHMesh.uniform(nivals, K)
    dims = (nx, nu, nq, ncr, nce)
    N, nz, ne = mesh.N, 1 + nx + nu, 1 + 2 * nx + nq
    vb, cb = sfb.ocp_nlp_structure(mesh, dims)
    n, m = int(vb[4]), int(cb[4])
    colptr, rowind = sfb.ocp_nlp_hess_pattern(mesh, dims)
    nnz = len(rowind)
    ws = sfb.ocp_nlp_bounds(mesh, dims, np.zeros(ncr), np.zeros(ncr), np.zeros(nce), np.zeros(nce))[4]
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.rand(*s, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1    # noqa: E731
    x = rnd(B, n)
    x[:, 0] = 2.0 + 0.1 * x[:, 0]
    lam, sigma = rnd(B, m), rnd(B)
    dFf, dFg, dFcr = rnd(B, N, nx, nz), rnd(B, N, nq, nz), rnd(B, N, ncr, nz)
    HLf, HLg, HLcr = rnd(B, N, nz, nz), rnd(B, N, nz, nz) if nq else rnd(B, 0), rnd(B, N, nz, nz) if ncr else rnd(B, 0)
    d2theta, d2ce = rnd(B, ne, ne), rnd(B, ne, ne) if nce else rnd(B, 0)
    hess = torch.empty((B, nnz), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr() if t.numel() else 0                                  # noqa: E731

    def fused():
        sfb.ocp_nlp_hess_batch_device(mesh, dims, B, p(x), p(lam), p(sigma), p(dFf), p(HLf), p(dFg), p(HLg), p(dFcr), p(HLcr), p(d2theta), p(d2ce),
                                      p(hess), stream=stream)

    # ---- the torch baseline.  The node times and weights come from the tests' float64 restatement of the mesh (tests/meshfn_ref.py)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import meshfn_ref as MR
    tau, w, _ = MR.geometry(mesh.K, mesh.tau0)
    node, pos, end = records(np, colptr, rowind, vb, N, nx, nu, nq)
    dest_n, src_n = [], []
    for e in range(nnz):
        if node[e] == -2:
            dest_n += [e] * N
            src_n += [i * nz * nz + pos[e] for i in range(N)]
        elif node[e] >= 0:
            dest_n.append(e)
            src_n.append(node[e] * nz * nz + pos[e])
    dev = lambda a, t=np.int64: torch.from_numpy(np.asarray(a, dtype=t)).cuda()     # noqa: E731
    dest_n, src_n = dev(dest_n), dev(src_n)
    dest_e, src_e = dev(np.nonzero(end >= 0)[0]), dev(end[end >= 0])
    pw = np.ones((N, nz, nz))                                                       # w_i and the powers of tau of the tf row
    pw[:, 0, :] *= tau[:, None]
    pw[:, 0, 0] *= tau
    Cw = dev(ws * w[:, None, None] * pw, np.float64)
    Jw = np.ones((N, nz))
    Jw[:, 0] = 2 * tau
    Jw = dev(ws * w[:, None] * Jw, np.float64)
    hess2 = torch.empty_like(hess)

    def baseline():
        h = x[:, 0].reshape(B, 1, 1, 1)
        blk = HLf + HLg if nq else HLf
        blk = h * Cw * blk
        if ncr:
            blk = blk + Cw * HLcr
        J = torch.einsum("bij,bijc->bic", lam[:, :cb[1]].reshape(B, N, nx), dFf)
        if nq:
            J = J + torch.einsum("bj,bijc->bic", lam[:, cb[1]:cb[2]], dFg)
        blk[:, :, 0, :] += Jw * J
        hess2.zero_()
        hess2.index_add_(1, dest_n, blk.reshape(B, -1).index_select(1, src_n))
        endb = sigma.reshape(B, 1, 1) * d2theta
        if nce:
            endb = endb + d2ce
        hess2.index_add_(1, dest_e, endb.reshape(B, -1).index_select(1, src_e))

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
        baseline()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(hess).all())
    err = float((hess - hess2).abs().max()) / (1.0 + float(hess.abs().max()))
    assert err < 1e-9, err                                                          # the two compute the same thing
    wf, wc = [], []
    for _ in range(5):                                                              # alternating
        wf.append(window(fused))
        wc.append(window(baseline))
    read = 8 * (B + sum(t.numel() for t in (lam, sigma, dFf, dFg, HLf, HLg, HLcr, d2theta, d2ce)))
    written = 8 * hess.numel()
    ms, msc = min(wf), min(wc)
    print("agents %d  mesh %d x %d  dims %s  n %d  m %d  nnzH %d  agents per lane %s" % (B, nivals, K, dims, n, m, nnz, os.environ.get("NLP_HESS_AGENTS", "default")))
    print("  fused    %.4f ms per call (windows %s, spread %.4f)   read %.1f MB  written %.1f MB   %.0f GB/s"
          % (ms, " ".join("%.4f" % v for v in wf), max(wf) - ms, read / 1e6, written / 1e6, (read + written) / ms / 1e6))
    print("  baseline %.4f ms per call (windows %s, spread %.4f)   fused is %.4f ms less, %.2fx;  largest scaled difference of the two results %.1e"
          % (msc, " ".join("%.4f" % v for v in wc), max(wc) - msc, msc - ms, msc / ms, err), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*[int(v) for v in sys.argv[2:10]])
    else:
        one = "--one" in sys.argv
        a = [int(v) for v in sys.argv[1:] if v != "--one"][:8]
        a += [8192, 13, 4, 12, 2, 1, 2, 12][len(a):]
        for rep in range(1 if one else 3):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(v) for v in a], check=True, timeout=300)
