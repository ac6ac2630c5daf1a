"""The HIP EKF covariance kernels (csrc/ekf.hip, detail/ekf_lane.hpp) against the 60-digit fixture tests/golden/ekf_reference.npz,
within the gates of tests/ekf_gates.py: non-symmetric P, Q and R, cond(P) of 1e1, 1e6 and 1e10.  Needs an MI355X.

Every bucket is run at batches of 1, 65 and 130 with the fixture's draws tiled (filter b carries draw b mod ndraws) and per-filter
Q / R / dt, and asserts: every filter within the bucket's gate; filters that carry the same draw give the same bits; the bits are
the oracle's on these inputs (the existing parity tests feed the update a symmetric P only); info == 0.

What ekf_launch can reach, and where it runs here:
  ekf_kernel<N, M> (SFB_EKF_CASE)     (2,1) (2,2) (2,3) (3,1) (3,2) (3,3) (4,1) (4,2) (4,3) (6,1) (6,2) (6,3) (6,6) (4,4) (7,1) (7,2)
                                      (7,3): test_update_fused_and_chain[N-M], update alone, fused, three fused ticks; predict alone
                                      at dof 2, 3, 4, 6, 7: test_predict[dof]
  ekf_kernel<8, 1> predict only       test_predict[8] (the dof-8 register kernel), and the predict half of the fused (8, M) steps
  ekf_update_wide_kernel<N, M>        (8,1) (8,2) (8,3) (9,1) (9,2) (9,3) (10,1) (10,2) (10,3): test_update_fused_and_chain[N-M]
  ekf_generic_kernel, N < M solve     (3,10) (5,9): test_update_fused_and_chain
  ekf_generic_kernel, N >= M solve    (5,5) (9,4) (11,3) (16,16), and (1,1): test_update_fused_and_chain; predict at dof 1, 9, 11, 16
  ekf_rk4_kernel<N>                   dof 2, 3, 4, 6: test_predict[dof], classes rk4 (one A) and rk4_tv (A, A_mid, A_end)
  runge_kutta4 in the generic kernel  dof 1, 7, 8, 9, 11, 16: test_predict[dof], rk4 and rk4_tv
  ekf_fused_persistent_kernel<6, M>   M = 1, 2, 3: test_persistent_fused_step[M], 4 * 1024 * 64 + 37 filters
  sfb_ekf_predict_update_batch        device pointers, (6,3) at batch 65: test_device_pointer_entry_gives_the_host_entrys_bits
"""
import numpy as np
import pytest

import ekf_gates as G

pytestmark = pytest.mark.gpu

BATCHES = (1, 65, 130)


def _tile(a, B):
    return np.ascontiguousarray(a[np.arange(B) % len(a)])


def _bucket(k, who, got, want_bits, ref):
    """got (B, w) of the kernel; want_bits (D, w) of the oracle on the D draws; ref (D, w) of the fixture"""
    B, D = len(got), len(ref)
    assert np.array_equal(got, _tile(want_bits, B)), "%s (%s): not the oracle's bits (nor, then, the same bits for the same draw)" % (k, who)
    assert np.array_equal(got, got[np.arange(B) % D])                               # same draw, same bits
    G.check(k, got, _tile(ref, B), who)


@pytest.mark.parametrize("dof", G.PREDICT_DOFS)
def test_predict(sfb, oracle, dof):
    for L in G.levels(dof):
        s = G.state(dof, L)
        want = {"euler": oracle.ekf_predict_batch(s["A"], s["Q"], s["dt"], s["P"]),
                "rk4": oracle.ekf_predict_batch(s["A"], s["Q"], s["dt"], s["P"], stepper="rk4"),
                "rk4_tv": oracle.ekf_predict_batch(s["A"], s["Q"], s["dt"], s["P"], stepper="rk4", A_mid=s["Am"], A_end=s["Ae"])}
        for B in BATCHES:
            P, A, Q, dt, Am, Ae = (_tile(s[k], B) for k in ("P", "A", "Q", "dt", "Am", "Ae"))
            got = {"euler": sfb.ekf_predict_batch_host(P, dof, A, Q, dt, stepper="euler"),
                   "rk4": sfb.ekf_predict_batch_host(P, dof, A, Q, dt, stepper="rk4"),
                   "rk4_tv": sfb.ekf_predict_batch_host(P, dof, A, Q, dt, stepper="rk4", A_mid=Am, A_end=Ae)}
            for c in G.PREDICT_CLASSES:
                _bucket(G.key(c, dof, None, L), "B=%d" % B, got[c], want[c], s[c])
            step, _, _ = sfb.ekf_step_batch_host(P, dof, A=A, Q=Q, dt=dt)           # the fused entry with the predict half alone
            assert np.array_equal(step, got["euler"])


def _oracle_fused(oracle, s, p, n, Q, P):
    return oracle.ekf_update_batch(p["H"], p["R"], p["r"], oracle.ekf_predict_batch(s["A"], Q, s["dt"], P), n)


@pytest.mark.parametrize("dof,ny", G.PAIRS, ids=["%d-%d" % nm for nm in G.PAIRS])
def test_update_fused_and_chain(sfb, oracle, dof, ny):
    for L in G.levels(dof):
        s, p = G.state(dof, L), G.pair(dof, ny, L)
        Pu, du, iu = oracle.ekf_update_batch(p["H"], p["R"], p["r"], s["P"], dof)
        Pf, df, jf = _oracle_fused(oracle, s, p, dof, s["Q"], s["P"])
        assert (iu == 0).all() and (jf == 0).all()
        if L in G.CHAIN:
            Pt = s["P"]
            for _ in range(3):
                Pt, dk, jt = _oracle_fused(oracle, s, p, dof, s["Qc"], Pt)
                assert (jt == 0).all()
        for B in BATCHES:
            who = "B=%d" % B
            P, A, Q, Qc, dt = (_tile(s[k], B) for k in ("P", "A", "Q", "Qc", "dt"))
            H, R, r = (_tile(p[k], B) for k in ("H", "R", "r"))
            gP, gd, info = sfb.ekf_step_batch_host(P, dof, H=H, R=R, r=r)
            assert (info == 0).all()
            _bucket(G.key("update_P", dof, ny, L), who, gP, Pu, p["update_P"])
            _bucket(G.key("update_delta", dof, ny, L), who, gd, du, p["update_delta"])
            gP, gd, info = sfb.ekf_step_batch_host(P, dof, A=A, Q=Q, dt=dt, H=H, R=R, r=r)
            assert (info == 0).all()
            _bucket(G.key("fused_P", dof, ny, L), who, gP, Pf, p["fused_P"])
            _bucket(G.key("fused_delta", dof, ny, L), who, gd, df, p["fused_delta"])
            if L in G.CHAIN:                                                        # three ticks, P fed back
                gP = P
                for _ in range(3):
                    gP, gd, info = sfb.ekf_step_batch_host(gP, dof, A=A, Q=Qc, dt=dt, H=H, R=R, r=r)
                    assert (info == 0).all()
                _bucket(G.key("ticks_P", dof, ny, L), who, gP, Pt, p["ticks_P"])
                _bucket(G.key("ticks_delta", dof, ny, L), who, gd, dk, p["ticks_delta"])


@pytest.mark.parametrize("ny", [1, 2, 3])
def test_persistent_fused_step(sfb, oracle, knobs, ny):
    """4 * 1024 * 64 + 37 fused steps at dof 6 -- the batch the persistent kernel takes (test_ekf_gpu.py's persistent test) -- with the
    draws of all three levels tiled: filter b carries draw b mod (3 ndraws).  Gates per level, the oracle's bits, and the bits of the
    one-tile-per-wave kernel."""
    dof, B = 6, 4 * 1024 * 64 + 37
    D = G.DRAWS[dof]
    cat = lambda k, src: np.concatenate([src(L)[k] for L in G.LEVELS])
    sall = {k: cat(k, lambda L: G.state(dof, L)) for k in ("P", "A", "Q", "dt")}
    pall = {k: cat(k, lambda L: G.pair(dof, ny, L)) for k in ("H", "R", "r", "fused_P", "fused_delta")}
    Pf, df, jf = _oracle_fused(oracle, sall, pall, dof, sall["Q"], sall["P"])
    assert (jf == 0).all()
    P, A, Q, dt = (_tile(sall[k], B) for k in ("P", "A", "Q", "dt"))
    H, R, r = (_tile(pall[k], B) for k in ("H", "R", "r"))
    gP, gd, info = sfb.ekf_step_batch_host(P, dof, A=A, Q=Q, dt=dt, H=H, R=R, r=r)
    assert (info == 0).all()
    assert np.array_equal(gP, _tile(Pf, B)) and np.array_equal(gd, _tile(df, B))   # the oracle's bits, hence the same for the same draw
    idx = np.arange(B) % (3 * D)
    for i, L in enumerate(G.LEVELS):
        mine = (idx >= i * D) & (idx < (i + 1) * D)                                 # in b order these carry draws 0 .. D-1 in turn
        p = G.pair(dof, ny, L)
        G.check(G.key("fused_P", dof, ny, L), gP[mine], _tile(p["fused_P"], int(mine.sum())), "persistent")
        G.check(G.key("fused_delta", dof, ny, L), gd[mine], _tile(p["fused_delta"], int(mine.sum())), "persistent")
    knobs.set(SFB_EKF_PERSISTENT=0)
    P0, d0, i0 = sfb.ekf_step_batch_host(P, dof, A=A, Q=Q, dt=dt, H=H, R=R, r=r)
    assert np.array_equal(gP, P0) and np.array_equal(gd, d0) and np.array_equal(info, i0)


def test_device_pointer_entry_gives_the_host_entrys_bits(sfb):
    import torch
    dof, ny, B, L = 6, 3, 65, "c10"
    s, p = G.state(dof, L), G.pair(dof, ny, L)
    P, A, Q, dt = (_tile(s[k], B) for k in ("P", "A", "Q", "dt"))
    H, R, r = (_tile(p[k], B) for k in ("H", "R", "r"))
    hP, hd, hi = sfb.ekf_step_batch_host(P, dof, A=A, Q=Q, dt=dt, H=H, R=R, r=r)
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dP, dA, dQ, ddt, dH, dR, dr = (T(a) for a in (P, A, Q, dt, H, R, r))
    dd = torch.empty((B, dof), dtype=torch.float64, device=dev)
    di = torch.full((B,), -1, dtype=torch.int32, device=dev)
    sfb.ekf_predict_update_batch_device(B, dof, ny, dA.data_ptr(), dQ.data_ptr(), 0, ddt.data_ptr(), 0, dH.data_ptr(), dR.data_ptr(), 0,
                                        dr.data_ptr(), dP.data_ptr(), dd.data_ptr(), dinfo=di.data_ptr(),
                                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(dP.cpu().numpy(), hP) and np.array_equal(dd.cpu().numpy(), hd) and np.array_equal(di.cpu().numpy(), hi)
    assert (hi == 0).all()
    G.check(G.key("fused_P", dof, ny, L), hP, _tile(p["fused_P"], B), "device pointers")
    G.check(G.key("fused_delta", dof, ny, L), hd, _tile(p["fused_delta"], B), "device pointers")
