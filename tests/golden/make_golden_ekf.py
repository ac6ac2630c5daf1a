"""Writes tests/golden/ekf_reference.npz: the matrix part of smooth::feedback::EKF (reference include/smooth/feedback/ekf.hpp:84-102
predict, :119-138 update) evaluated with mpmath at 60 digits on inputs that make every convention of those lines visible.  Written
from those lines alone: nothing here comes from oracle/ekf_oracle.c or from the project's headers.

    python tests/golden/make_golden_ekf.py            (under a minute; needs mpmath, which no test needs)

What is computed (symU(M): the upper triangle of M mirrored, Eigen's selfadjointView<Upper>):
  euler    P + dt symU(A P + P A' + Q)                                  (:88 with odeint's euler, the default stepper :30)
  rk4      odeint's runge_kutta4 on dP/dt = symU(A P + P A' + Q): k1 = f(P), k2 = f(P + dt/2 k1), k3 = f(P + dt/2 k2),
           k4 = f(P + dt k3), P + dt/6 (k1 + 2 k2 + 2 k3 + k4), with one A
  rk4_tv   the same with A at t for k1, A_mid at t + dt/2 for k2 and k3, A_end at t + dt for k4
  update   S = symU(H symU(P) H' + R), K = (S^-1 H P)', delta = K r, P <- symU((I - K H) P)      (:129-138)
  fused    update after euler
  ticks    three fused steps with the same A, Q_chain, dt, H, R, r, P fed back; the third tick's P and delta are stored

Inputs (stored as the float64 values the kernels are fed; matrices column-major flat):
  P      V diag(lambda) V' with lambda log-spaced from 1 down to 1/cond, cond = 1e1 (c1), 1e6 (c6), 1e10 (c10), V a random
         orthogonal matrix; formed at 60 digits and rounded; then the strictly lower triangle is moved by 0.1 lambda_min u
         so that P(i,j) != P(j,i): S reads the upper triangle, H P and (I - K H) P read all of P
  Q      s (I + 0.5 u), non-symmetric (only its upper triangle counts); s is the power of two nearest lambda_min
  R      s (1 + 0.5 u) on the diagonal, 0.1 s u above it, unrelated u of order one below it (never read)
  H, A, A_mid, A_end, r   u;    dt in [0.005, 0.1]
  Q_chain   qchain Q with qchain a power of two (stored; the product is exact) that brings Q to about n/3.  An explicit Euler step
         keeps P positive definite only where dt Q outweighs dt^2 A P A'; with Q of the order of lambda_min the predicted P is
         indefinite at c6 from the first tick on, S with it, the recursion diverges (eigenvalues of P of -300 by the third tick
         were seen), and how well a diagonally pivoted LDL' without 2x2 blocks does on an indefinite S is Eigen's own matter,
         not this formula's: the single fused step keeps the small Q, and with it an ill-conditioned S; the chain, which is there
         for P fed back through three ticks, runs where the filter does
u is uniform on the multiples of 2^-10 in [-1, 1]: such inputs compress, and the results, which do not, are what fills the file.

Coverage: every pair ekf_launch dispatches to a register kernel (SFB_EKF_CASE, SFB_EKF_WIDE in csrc/ekf.hip) and the generic
kernel on both of its solve branches, N < M: (3,10), (5,9); N >= M: (5,5), (9,4), (11,3), (16,16); and (1,1).  The pairs of one dof
share that dof's P, A, Q, dt draws (the predict results are keyed by dof on the same draws); H, R, r are the pair's own.

Size: the fixture may not exceed the largest one already committed (meshfn_reference.npz, 389 597 bytes), and the results are
float64 roundings of 60-digit numbers, which do not compress.  Eight draws per (pair, level) for all 33 pairs would be about
119 000 such values, 1.1 MB, however they are packed; so the draws are trimmed, never the coverage: the symmetric results are
stored as packed upper triangles, the pairs of one dof share one set of P, A, Q, dt draws, only the chain's last tick is kept, and
DRAWS below falls with the dof (a result has dof^2 entries) from 8 to 2 per (pair, level).  This writes 381 368 bytes.
Levels c1 and c10 only where dof or ny exceeds 10; the chain at c1 and c6 only.
"""
import os
import sys

import mpmath as mp
import numpy as np

mp.mp.dps = 60
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ekf_reference.npz")

CASE = [(2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (3, 3), (4, 1), (4, 2), (4, 3), (6, 1), (6, 2), (6, 3), (6, 6), (4, 4), (7, 1), (7, 2), (7, 3)]
WIDE = [(8, 1), (8, 2), (8, 3), (9, 1), (9, 2), (9, 3), (10, 1), (10, 2), (10, 3)]
GENERIC = [(3, 10), (5, 9), (5, 5), (9, 4), (11, 3), (16, 16), (1, 1)]
PAIRS = CASE + WIDE + GENERIC
PREDICT_DOFS = [1, 2, 3, 4, 6, 7, 8, 9, 11, 16]
LEVELS = {"c1": 1e1, "c6": 1e6, "c10": 1e10}
CHAIN = ("c1", "c6")
DRAWS = {1: 8, 2: 8, 3: 6, 4: 6, 5: 4, 6: 4, 7: 3, 8: 2, 9: 2, 10: 2, 11: 2, 16: 2}   # per (dof, level); see "Size" above
GRID = 1024


def levels(n):
    return ("c1", "c10") if n > 10 else ("c1", "c6", "c10")


def u(rng, *shape):
    return rng.integers(-GRID, GRID + 1, shape).astype(np.float64) / GRID


def M(flat, rows, cols):
    """column-major flat float64 -> mp.matrix, exactly"""
    return mp.matrix([[mp.mpf(float(flat[i + j * rows])) for j in range(cols)] for i in range(rows)])


def flat(X):
    return np.array([float(X[i, j]) for j in range(X.cols) for i in range(X.rows)])


def packed(X):
    """upper triangle, column by column"""
    return np.array([float(X[i, j]) for j in range(X.cols) for i in range(j + 1)])


def symU(X):
    n = X.rows
    return mp.matrix([[X[min(i, j), max(i, j)] for j in range(n)] for i in range(n)])


def cov_rhs(A, P, Q):
    return symU(A * P + P * A.T + Q)


def euler(P, A, Q, dt):
    return P + dt * cov_rhs(A, P, Q)


def rk4(P, A0, Am, Ae, Q, dt):
    k1 = cov_rhs(A0, P, Q)
    k2 = cov_rhs(Am, P + (dt / 2) * k1, Q)
    k3 = cov_rhs(Am, P + (dt / 2) * k2, Q)
    k4 = cov_rhs(Ae, P + dt * k3, Q)
    return P + (dt / 6) * (k1 + 2 * k2 + 2 * k3 + k4)


def update(P, H, R, r):
    S = symU(H * symU(P) * H.T + R)
    K = (mp.inverse(S) * (H * P)).T
    return symU((mp.eye(P.rows) - K * H) * P), K * r


def make_P(rng, n, cond):
    lam = [mp.mpf(cond) ** (-mp.mpf(i) / max(n - 1, 1)) for i in range(n)]
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Vm = mp.matrix(V.tolist())
    P = Vm * mp.diag(lam) * Vm.T
    P = np.array([[float((P[i, j] + P[j, i]) / 2) for j in range(n)] for i in range(n)])
    P += np.tril(u(rng, n, n), -1) * 0.1 * float(lam[-1])
    return np.ascontiguousarray(P.T).ravel(), 2.0 ** round(np.log2(float(lam[-1])))          # column-major flat; the scale of Q and R


def main():
    rng = np.random.default_rng(20261019)
    dofs = sorted({n for n, _ in PAIRS})
    out = {k: [] for k in ("state.P", "state.A", "state.Q", "state.dt", "state.qchain", "predict.Am", "predict.Ae", "predict.euler", "predict.rk4",
                           "predict.rk4_tv", "update.H", "update.R", "update.r", "update.P", "update.delta", "fused.P", "fused.delta",
                           "ticks.P", "ticks.delta")}
    state = {}
    for n in dofs:
        for L in levels(n):
            rows = []
            for d in range(DRAWS[n]):
                P, lmin = make_P(rng, n, LEVELS[L])
                A = u(rng, n * n)
                Q = lmin * (np.eye(n).ravel() + 0.5 * u(rng, n * n))
                dt = 0.005 + 0.095 * float(rng.integers(0, GRID + 1)) / GRID
                qchain = 2.0 ** int(np.ceil(np.log2(max(1.0, n / 3.0)))) / lmin
                rows.append((P, A, Q, dt, lmin, qchain))
                for k, v in zip(("state.P", "state.A", "state.Q", "state.dt", "state.qchain"), (P, A, Q, [dt], [qchain])):
                    out[k].append(np.asarray(v, dtype=np.float64))
                if n in PREDICT_DOFS:
                    Am, Ae = u(rng, n * n), u(rng, n * n)
                    Pm, A0, Qm, dtm = M(P, n, n), M(A, n, n), M(Q, n, n), mp.mpf(dt)
                    out["predict.Am"].append(Am); out["predict.Ae"].append(Ae)
                    out["predict.euler"].append(flat(euler(Pm, A0, Qm, dtm)))
                    out["predict.rk4"].append(flat(rk4(Pm, A0, A0, A0, Qm, dtm)))
                    out["predict.rk4_tv"].append(flat(rk4(Pm, A0, M(Am, n, n), M(Ae, n, n), Qm, dtm)))
            state[n, L] = rows
        print("state", n, file=sys.stderr)
    for n, m in PAIRS:
        for L in levels(n):
            for P, A, Q, dt, lmin, qchain in state[n, L]:
                H, r = u(rng, m * n), u(rng, m)
                Ru = u(rng, m, m)
                R = np.triu(Ru, 1) * 0.1 * lmin + np.tril(Ru, -1) + np.diag(lmin * (1.0 + 0.5 * u(rng, m)))
                R = np.ascontiguousarray(R.T).ravel()
                for k, v in zip(("update.H", "update.R", "update.r"), (H, R, r)):
                    out[k].append(v)
                Pm, Am, Qm, dtm, Hm, Rm, rm = M(P, n, n), M(A, n, n), M(Q, n, n), mp.mpf(dt), M(H, m, n), M(R, m, m), M(r, m, 1)
                Pu, du = update(Pm, Hm, Rm, rm)
                out["update.P"].append(packed(Pu)); out["update.delta"].append(flat(du))
                Pf, df = update(euler(Pm, Am, Qm, dtm), Hm, Rm, rm)
                out["fused.P"].append(packed(Pf)); out["fused.delta"].append(flat(df))
                if L in CHAIN:
                    Qc, Pf = M(qchain * Q, n, n), Pm
                    for _ in range(3):
                        Pf, df = update(euler(Pf, Am, Qc, dtm), Hm, Rm, rm)
                    out["ticks.P"].append(packed(Pf)); out["ticks.delta"].append(flat(df))
        print("pair", n, m, file=sys.stderr)
    arrays = {k: np.concatenate(v) for k, v in out.items()}
    arrays["pairs"] = np.array(PAIRS, dtype=np.int32)
    arrays["dofs"] = np.array(dofs, dtype=np.int32)
    arrays["predict_dofs"] = np.array(PREDICT_DOFS, dtype=np.int32)
    arrays["draws"] = np.array([DRAWS[n] for n in dofs], dtype=np.int32)
    arrays["level.names"] = np.array(list(LEVELS))
    arrays["level.cond"] = np.array(list(LEVELS.values()))
    arrays["chain.levels"] = np.array(CHAIN)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")
    for k in sorted(arrays):
        print("  %-16s %8d values" % (k, arrays[k].size))


if __name__ == "__main__":
    main()
