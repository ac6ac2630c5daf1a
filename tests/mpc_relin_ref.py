"""A plain float64 numpy restatement of the re-linearisation passes of include/smooth_feedback_amd/mpc_relin.hpp for the
planar vehicle (examples/vehicle_model.h, variant 6: SE2 x R^3, U = R^2), sharing nothing with the headers.  It sits next to the
other restatements of the MPC transcription (mesh_ref.py: mesh, flat dynamics, audit; flatten_ref.py: the groups as matrices):
  F(e, v), cr(e, v)         the flat dynamics in the tangent deviations (mesh_ref.audit_flat: dr_expinv by its Bernoulli series in
                            ad on homogeneous matrices) and the input box cr = udes (+) v
  jacobians_fd              central differences of those
  jacobians_zero            the closed form at e = v = 0: df/dx - ad(f + dxdes) / 2, df/du
  rows                      the QP rows of a linearisation (A_i, B_i, f0_i, C_i, D_i, c0_i) on the LGR mesh as a DENSE matrix:
                            sum_j D(j, i) e_j = tf (A_i e_i + B_i v_i + f0_i),  crl <= C_i e_i + D_i v_i + c0_i <= cru,  e_0 pinned
  passes                    solve, re-linearise by central differences about the plan, solve again warm-started, with the oracle's
                            sparse QP solver; the audit (mesh_ref.audit_errors) after every pass
The vehicle's desired trajectory has the constant body velocity (1, 0, 0.4 | 0, 0, 0) and udes = 0, so F does not depend on time."""
import numpy as np

import flatten_ref as FR
import mesh_ref as R

NX, NU, NCR, KMESH = 6, 2, 2, 4
TWIST = np.array([1.0, 0.0, 0.4])
DXDES = np.array([1.0, 0.0, 0.4, 0.0, 0.0, 0.0])
CRL, CRU = np.array([-0.5, -0.5]), np.array([0.5, 0.5])
FD_H = 2.0 ** -17          # eps^(1/3): balances the truncation h^2 |F'''| / 6 of a central difference against its rounding eps |F| / h
KEPT = (0, 4, 5)           # Optimal, MaxIterations, MaxTime: the plans a controller keeps


def F(e, v):
    return R.audit_flat("vehicle6", np.asarray(e, dtype=np.float64)[None, :], np.asarray(v, dtype=np.float64)[None, :])[0]


def cr(e, v):
    return np.asarray(v, dtype=np.float64).copy()


def jacobians_fd(fn, e, v, h=FD_H):
    """(d fn / de, d fn / dv) by central differences"""
    e, v = np.asarray(e, dtype=np.float64), np.asarray(v, dtype=np.float64)
    cols = []
    for c in range(NX + NU):
        d = np.zeros(NX + NU); d[c] = h
        cols.append((fn(e + d[:NX], v + d[NX:]) - fn(e - d[:NX], v - d[NX:])) / (2 * h))
    J = np.stack(cols, axis=1)
    return J[:, :NX], J[:, NX:]


def fd_tolerance(scale):
    """of a comparison with jacobians_fd, scaled by 1 + max |J|: rounding 16 eps / h (the differences of 1 + NX + NU values of
    size <= scale, a few roundings each) and truncation h^2 |F'''| / 6 with |F'''| <= 60 on |e| <= 1.5 (the cubic terms of the
    dr_expinv series times the twist)"""
    return (16 * np.finfo(float).eps / FD_H + 10 * FD_H ** 2) * scale


def jacobians_zero():
    """A, B, f0 at e = v = 0 in closed form"""
    vel = TWIST
    f = np.concatenate([vel, [-0.2 * vel[0], 0.0, -0.4 * vel[2]]])
    dfdx = np.zeros((NX, NX)); dfdx[0, 3] = dfdx[1, 4] = dfdx[2, 5] = 1.0; dfdx[3, 3] = -0.2; dfdx[5, 5] = -0.4
    dfdu = np.zeros((NX, NU)); dfdu[3, 0] = dfdu[5, 1] = 1.0
    adm = np.zeros((NX, NX)); adm[:3, :3] = FR.ad_part("SE2", (f + DXDES)[:3])
    return dfdx - adm / 2, dfdu, f - DXDES


def mesh(K):
    n = -(-int(K) // KMESH)
    return np.full(n, KMESH), np.arange(n) / n


def linearise(plan, K, fd=True):
    """per node (A, B, f0, C, D, c0) about plan = [e_0 .. e_N | v_0 .. v_{N-1}] (None: about zero, closed form)"""
    N = KMESH * len(mesh(K)[0])
    out = []
    for i in range(N):
        if plan is None:
            A, B, f0 = jacobians_zero()
            out.append((A, B, f0, np.zeros((NCR, NX)), np.eye(NCR, NU), np.zeros(NCR)))
            continue
        e, v = plan[i * NX:(i + 1) * NX], plan[(N + 1) * NX + i * NU:(N + 1) * NX + (i + 1) * NU]
        A, B = jacobians_fd(F, e, v)
        C, D = jacobians_fd(cr, e, v)
        out.append((A, B, F(e, v) - A @ e - B @ v, C, D, cr(e, v) - C @ e - D @ v))
    return out


def rows(lin, K, tf, e0):
    """dense A (m, n), l, u of the QP: rows [dyn | cr | x0], columns [e_0 .. e_N | v_0 .. v_{N-1}]"""
    Km, tau0 = mesh(K)
    N = int(Km.sum())
    n, m = NX * (N + 1) + NU * N, NX * N + NCR * N + NX
    A, lo, hi = np.zeros((m, n)), np.zeros(m), np.zeros(m)
    for s in range(len(Km)):
        D = R.diffmat(Km, tau0, s)                                     # (KMESH + 1, KMESH): d/dtau, tau in [0, 1]
        for i in range(KMESH):
            node = s * KMESH + i
            Ai, Bi, f0, Ci, Di, c0 = lin[node]
            r = slice(node * NX, (node + 1) * NX)
            for j in range(KMESH + 1):
                cj = (s * KMESH + j) * NX
                A[r, cj:cj + NX] -= D[j, i] * np.eye(NX)
            A[r, node * NX:(node + 1) * NX] += tf * Ai
            A[r, NX * (N + 1) + node * NU:NX * (N + 1) + (node + 1) * NU] += tf * Bi
            lo[r] = hi[r] = -tf * f0
            rc = slice(NX * N + node * NCR, NX * N + (node + 1) * NCR)
            A[rc, node * NX:(node + 1) * NX] = Ci
            A[rc, NX * (N + 1) + node * NU:NX * (N + 1) + (node + 1) * NU] = Di
            lo[rc], hi[rc] = CRL - c0, CRU - c0
    r0 = slice(NX * N + NCR * N, m)
    A[r0, :NX] = np.eye(NX)
    lo[r0] = hi[r0] = e0
    return A, lo, hi


def xdes_pose(t):
    g0 = np.array([[0.0, -1.0, 2.5], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])      # SE2::FromAngle(pi / 2, 2.5, 0)
    return g0 @ FR.expm(FR.hat("SE2", t * TWIST))


def initial_deviation(t, dx0):
    """e_0 = log(xdes(t)^-1 x) of the state x = xdes(t) (+) dx0, through the matrices"""
    Xd = xdes_pose(t)
    X = Xd @ FR.expm(FR.hat("SE2", dx0[:3]))
    return np.concatenate([FR.log_part("SE2", np.linalg.solve(Xd, X)), dx0[3:]])


def csr_values(Ad, Ap, Aj):
    """the stored entries of the transcription's pattern out of a dense A, and what lies outside the pattern"""
    vals = np.concatenate([Ad[r, Aj[Ap[r]:Ap[r + 1]]] for r in range(len(Ap) - 1)])
    rest = Ad.copy()
    for r in range(len(Ap) - 1):
        rest[r, Aj[Ap[r]:Ap[r + 1]]] = 0.0
    return vals, float(np.abs(rest).max())


def passes(oracle, pattern, K, tf, t, dx0, npass, params=None):
    """The passes for agents (t [B], dx0 [B][NX]) with the oracle's sparse solver on the transcription's pattern (d, Pp, Pi, Pv, Ap,
    Aj of examples.models_lib.mpc_pattern(6, K, tf)).  Returns per pass the plans [B][n], codes [B] and audit errors agent_max [B]."""
    d, Pp, Pi, Pv, Ap, Aj = pattern
    B = len(t)
    prm = params if params is not None else oracle.default_params()
    e0 = np.stack([initial_deviation(t[b], dx0[b]) for b in range(B)])
    Px, q = np.tile(Pv, (B, 1)), np.zeros((B, d["n"]))
    plan, dual, code = [None] * B, np.zeros((B, d["m"])), np.full(B, -1)
    out = []
    for p in range(npass + 1):
        Av, lo, hi = np.zeros((B, d["nnzA"])), np.zeros((B, d["m"])), np.zeros((B, d["m"]))
        for b in range(B):
            Ad, lo[b], hi[b] = rows(linearise(plan[b] if code[b] in KEPT else None, K), K, tf, e0[b])
            Av[b], outside = csr_values(Ad, Ap, Aj)
            assert outside == 0.0
        warm = p > 0
        wx = np.stack([plan[b] if plan[b] is not None else np.zeros(d["n"]) for b in range(B)]) if warm else None
        r = oracle.qp_sparse_solve_batch(Pp, Pi, Px, q, Ap, Aj, Av, lo, hi, params=prm, warm_x=wx, warm_y=dual.copy() if warm else None, nthreads=4)
        for b in range(B):
            if r["code"][b] in KEPT or p == 0:
                plan[b], dual[b], code[b] = r["x"][b].copy(), r["y"][b], r["code"][b]
        plans = np.stack(plan)
        out.append(dict(plan=plans, code=code.copy(), agent_max=np.array([R.audit_errors("vehicle6", K, tf, plans[b]).max() for b in range(B)])))
    return out
