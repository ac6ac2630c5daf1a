"""Time of sfb_mesh_dyn_batch with derivatives: python scripts/mesh_dyn_time.py [agents] [intervals] [K] [nx] [nu].
Default: 8 192 agents on the MPC's 13 x 4 mesh, nx = 12, nu = 2.  The two launches of one call (values, CSR values) on device
tensors between device events, warmed; each of five windows holds ten calls, and the least window is reported per call.  The
whole thing is repeated in three fresh processes (this script starts them one after the other and touches no device itself).
The bandwidth is the least possible traffic -- every input read once, every output written once, the per-mesh tables not
counted -- over that time."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(B, nivals, K, nx, nu):
    import torch

    import smooth_feedback_amd as sfb

    mesh = sfb.PHMesh.uniform(nivals, K)
    N = mesh.N
    nnz = len(sfb.mesh_dyn_pattern(mesh, nx, nu)[1])
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.rand(*s, dtype=torch.float64, device="cuda", generator=g) * 2 - 1      # noqa: E731
    t0, tf, X, F, dF = rnd(B) * 0.1, 2.0 + rnd(B) * 0.1, rnd(B, N + 1, nx), rnd(B, N, nx), rnd(B, N, nx, 1 + nx + nu)
    out_F = torch.empty((B, N * nx), dtype=torch.float64, device="cuda")
    out_dF = torch.empty((B, nnz), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        sfb.mesh_dyn_batch_device(mesh, B, nx, nu, t0.data_ptr(), tf.data_ptr(), X.data_ptr(), F.data_ptr(), dF.data_ptr(), out_F.data_ptr(),
                                  out_dF.data_ptr(), stream=stream)

    for _ in range(5):
        call()
    torch.cuda.synchronize()
    windows, calls = [], 10
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            call()
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) / calls)
    assert bool(torch.isfinite(out_F).all()) and bool(torch.isfinite(out_dF).all())
    read = 8 * (2 * B + X.numel() + F.numel() + dF.numel())
    written = 8 * (out_F.numel() + out_dF.numel())
    ms = min(windows)
    print("agents %d  mesh %d x %d  nx %d  nu %d  nnz %d: %.4f ms per call (windows %s)   read %.1f MB  written %.1f MB   %.0f GB/s"
          % (B, nivals, K, nx, nu, nnz, ms, " ".join("%.4f" % w for w in windows), read / 1e6, written / 1e6, (read + written) / ms / 1e6), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*[int(v) for v in sys.argv[2:7]])
    else:
        a = [int(v) for v in sys.argv[1:6]]
        a += [8192, 13, 4, 12, 2][len(a):]
        for rep in range(3):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(v) for v in a], check=True, timeout=300)
