"""The rigid body on SE(3) x R^6 (examples/rigid_body_model.h, MPC variant 13: nx 12, nu 6, ncr 6) through the device side of
the MPC: sfb_mpc_assemble_batch with an SFB_LIE_SE3 part, the swarm linearised on the GPU (MPCSwarmDeviceLin) against the
host-linearised MPCSwarm, and the ASI filter on the same state group.  Needs an MI355X."""
import numpy as np
import pytest

import qp_certify as QC
from examples import models_lib as M
from test_mpc_devlin_gpu import REC_TOL, U_TOL

pytestmark = pytest.mark.gpu

VARIANT, K = 13, 8          # kmesh 4, nivals 2


def _assemble_on_device(L, rec, shared=None):
    import torch
    B = rec.shape[0]
    d_rec = torch.from_numpy(np.ascontiguousarray(rec)).cuda()
    d_sh = torch.from_numpy(shared).cuda() if shared is not None else None
    dA = torch.full((B, L.nnzA), np.nan, dtype=torch.float64, device="cuda")
    dl = torch.full((B, L.m), np.nan, dtype=torch.float64, device="cuda")
    du = torch.full((B, L.m), np.nan, dtype=torch.float64, device="cuda")
    L.assemble_batch_device(B, d_rec.data_ptr(), dA.data_ptr(), dl.data_ptr(), du.data_ptr(),
                            d_sh.data_ptr() if d_sh is not None else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dl.cpu().numpy(), du.cpu().numpy()


def _packed_layout(sfb, L, rec):
    parts = [(int(k), int(d)) for k, d in zip(L.kind, L.dof)]
    return sfb.MPCLayout(L.nx, L.nu, L.ncr, L.kmesh, L.nivals, L.tf, L.alpha, L.D, parts=parts, crl=L.crl, cru=L.cru, jac_keep=L.jac_keep_of(rec))


# hat of the basis vectors of se(3), tangent order (v, w); ad from the commutator of 4x4 matrices, not from any table
_E = np.zeros((6, 4, 4))
for _i in range(3):
    _E[_i, _i, 3] = 1.0
_E[3, 2, 1], _E[3, 1, 2] = 1.0, -1.0
_E[4, 0, 2], _E[4, 2, 0] = 1.0, -1.0
_E[5, 1, 0], _E[5, 0, 1] = 1.0, -1.0


def _ad_se3(a):
    A = np.einsum("i,ijk->jk", a, _E)
    cols = []
    for i in range(6):
        X = A @ _E[i] - _E[i] @ A
        cols.append([X[0, 3], X[1, 3], X[2, 3], X[2, 1], X[0, 2], X[1, 0]])
    return np.array(cols).T


@pytest.mark.parametrize("batch", [1, 5])
def test_assembly_with_an_se3_part_is_bit_identical_to_the_host_transcription(sfb, batch):
    """direct form, table form (Jacobians shared: the model's do not depend on the agent) and packed records; five agents
    cross the four-agents-per-thread grouping of the table form"""
    Av, l, u = M.mpc_assemble_batch(VARIANT, K, batch, seed=9)
    L, rec = M.mpc_records(VARIANT, K, batch, seed=9)
    assert (L.kmesh, L.nivals) == (4, 2) and [(int(k), int(d)) for k, d in zip(L.kind, L.dof)] == [(3, 6), (0, 6)]
    A2, l2, u2 = _assemble_on_device(L, rec)
    assert np.array_equal(A2, Av) and np.array_equal(l2, l) and np.array_equal(u2, u)
    own, shared = L.split_shared(rec)
    A3, l3, u3 = _assemble_on_device(L, own, shared)
    assert np.array_equal(A3, Av) and np.array_equal(l3, l) and np.array_equal(u3, u)
    Lp = _packed_layout(sfb, L, rec)
    packed = Lp.pack_records(rec)
    assert packed.shape[1] == Lp.record_doubles() < L.record_doubles()
    A4, l4, u4 = _assemble_on_device(Lp, packed)
    assert np.array_equal(A4, Av) and np.array_equal(l4, l) and np.array_equal(u4, u)
    # the own-node x-block of the dynamics rows, restated:  0 + tf dfdx;  += (-tf/2) ad(f + dxdes);  -= alpha D(i, i) on the
    # diagonal.  Every entry of ad is ONE signed component of f + dxdes (the commutator only adds zeros to it), so the
    # same three float64 operations produce it and the comparison is exact.
    N, nx, nu, km = L.N, L.nx, L.nu, L.kmesh
    f, dx, dfx = rec[:, :N * nx].reshape(batch, N, nx), rec[:, N * nx:2 * N * nx].reshape(batch, N, nx), rec[:, 2 * N * nx:2 * N * nx + N * nx * nx].reshape(batch, N, nx, nx)
    rowlen = km + nx + nu
    dyn = A2[:, :N * nx * rowlen].reshape(batch, N, nx, rowlen)
    for b in range(batch):
        for node in range(N):
            s, i = divmod(node, km)
            ad = np.zeros((nx, nx))
            ad[:6, :6] = _ad_se3((f[b, node] + dx[b, node])[:6])
            assert np.count_nonzero(ad) >= 12
            want = 0.0 + L.tf * dfx[b, node]
            want = want + (-L.tf / 2) * ad
            want[np.arange(nx), np.arange(nx)] -= L.alpha[s] * L.D[i, i]
            assert np.array_equal(dyn[b, node, :, i:i + nx], want), (b, node)


_RUNS = {}


def _devlin(batch, ticks):
    if (batch, ticks) not in _RUNS:
        _RUNS[batch, ticks] = M.mpc_swarm_devlin_step(VARIANT, K, batch, ticks, seed=1)
    return _RUNS[batch, ticks]


@pytest.mark.parametrize("batch", [3, 65])
def test_device_linearised_swarm_against_the_host_linearised_one(sfb, batch):
    """two ticks, cold then warm: records within REC_TOL of MPC::fill_record, codes equal, inputs within U_TOL; and the QPs
    the device-written records describe, solved by the same swarm kernels, pass the optimality certificates"""
    L, host = M.mpc_records(VARIANT, K, batch, seed=1)
    one = _devlin(batch, 1)
    Lp = M.mpc_layout(VARIANT, K)
    Lp.jac_keep = Lp.jac_keep_of(host)
    want = Lp.pack_records(host) if one["packed"] else host
    assert want.shape == one["records"].shape and np.max(np.abs(one["records"] - want)) <= REC_TOL
    d, Pp, Pi, Pv, Ap, Aj = M.mpc_pattern(VARIANT, K)
    plan = sfb.SparseQPPlan(d["n"], d["m"], Pp, Pi, Ap, Aj, stage=M.mpc_stage(VARIANT, K))
    Lq = _packed_layout(sfb, L, host) if one["packed"] else L
    swarm = sfb.MPCSwarm(plan, Lq, Pv, np.zeros(d["n"]), batch)
    if one["packed"]:
        swarm._rec_doubles = Lq.record_doubles()
    prm = QC.Params(max_iter=None)
    Px, q = np.tile(Pv, (batch, 1)), np.zeros((batch, d["n"]))
    udes = np.array([0.2, 0.3, 0.25, 0.4, 0.35, 0.5]) * np.array([0.8, 0.0, 0.15, 0.1, -0.05, 0.4])
    for ticks in (1, 2):
        r = _devlin(batch, ticks)
        u_ref, c_ref, _ = M.mpc_swarm_step(VARIANT, K, batch, ticks, seed=1)
        assert np.array_equal(r["code"], c_ref) and np.all(r["code"] == 0)
        assert np.max(np.abs(r["u0"] - u_ref)) <= U_TOL
        assert np.all(np.abs(r["u0"]) <= 0.5 + 1e-6)
        du0, code, it, x, y = swarm.step_host(r["records"], prm.sfb(sfb), full=True)      # warm from the previous tick at ticks = 2
        assert np.array_equal(code, r["code"]) and np.max(np.abs(du0 + udes - r["u0"])) <= U_TOL
        Ax, l, u = _assemble_on_device(Lq, r["records"])
        prob = QC.Problem.sparse(Pp, Pi, Px, q, Ap, Aj, Ax, l, u)
        obj = 0.5 * np.einsum("bi,bi->b", x, _psym_mv(Pp, Pi, Pv, x)) + np.einsum("bi,bi->b", q, x)
        rep = QC.certify(prob, dict(code=code, iter=it, x=x, y=y, obj=obj), prm)
        print("B %d tick %d: %s" % (batch, ticks, rep))
        assert rep.passed, str(rep)
    swarm.close()


def _psym_mv(Pp, Pi, Pv, x):
    """P x for the upper triangle (CSC) of a symmetric P"""
    out = np.zeros_like(x)
    for j in range(len(Pp) - 1):
        for p in range(Pp[j], Pp[j + 1]):
            i = Pi[p]
            out[:, i] += Pv[p] * x[:, j]
            if i != j:
                out[:, j] += Pv[p] * x[:, i]
    return out


def test_device_resident_swarm_front_on_the_rigid_body():
    """MPCSwarmDevice (host linearisation, device assembly with the SE3 table) == MPCSwarm (host assembly), three ticks"""
    u_h, c_h, i_h = M.mpc_swarm_step(VARIANT, K, 5, 3)
    u_d, c_d, i_d = M.mpc_swarm_step(VARIANT, K, 5, 3, device=True)
    assert np.array_equal(c_h, c_d) and np.array_equal(i_h, i_d) and np.array_equal(u_h, u_d)
    assert (c_d == 0).all() and u_d.shape == (5, 6)


def test_multi_device_swarm_on_the_rigid_body():
    r = M.mpc_swarm_devlin_step_multi(VARIANT, K, 5, 2, [0, 0], seed=1)
    one = M.mpc_swarm_devlin_step(VARIANT, K, 5, 2, seed=1, want_records=False)
    assert np.array_equal(r["code"], one["code"]) and np.max(np.abs(r["u0"] - one["u0"])) <= U_TOL


def test_asi_filter_on_the_rigid_body():
    """ASIFilter<Bundle<SE3, R6>, R6> on the host front and ASIFSwarmDevice on the same agents: Optimal, the QP's rows hold at
    the solution, and both fronts return the same inputs (the device assembles with its own maths library)"""
    u_dev, codes = M.asif_rigid_body_swarm_device(5)
    assert (codes == 0).all()
    for b in range(5):
        u, code, slack = M.asif_rigid_body(b)
        assert code == 0 and slack >= -5e-3
        assert np.all(np.abs(u[:6]) <= 0.5 + 1e-3)
        assert np.max(np.abs(u - u_dev[b])) <= U_TOL
