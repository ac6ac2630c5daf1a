"""Plain float64 numpy restatement of the matrix part of smooth::feedback::EKF, from the reference's ekf.hpp:84-102 (predict) and
:119-138 (update) and odeint's euler and runge_kutta4 tableaux.  Test infrastructure: it shares nothing with oracle/ekf_oracle.c or
the project's headers, and its error against the 60-digit fixture (tests/golden/make_golden_ekf.py) is what tests/ekf_gates.py
takes as "what float64 delivers on these inputs".  Matrices are ordinary (rows, cols) arrays here; the callers unflatten.

The two `wrong_*` switches of update() are the negative controls of tests/test_ekf_reference_host.py, not conventions."""
import numpy as np


def symU(X):
    """Eigen's selfadjointView<Upper>: the upper triangle mirrored"""
    U = np.triu(X)
    return U + np.triu(X, 1).T


def cov_rhs(A, P, Q):
    return symU(A @ P + P @ A.T + Q)                                   # ekf.hpp:88


def euler(P, A, Q, dt):
    return P + dt * cov_rhs(A, P, Q)


def rk4(P, A, Q, dt, A_mid=None, A_end=None):
    """runge_kutta4; A_mid, A_end: the linearisation at t + dt/2 and t + dt (cov_ode re-linearises at every stage time)"""
    Am = A if A_mid is None else A_mid
    Ae = A if A_end is None else A_end
    k1 = cov_rhs(A, P, Q)
    k2 = cov_rhs(Am, P + 0.5 * dt * k1, Q)
    k3 = cov_rhs(Am, P + 0.5 * dt * k2, Q)
    k4 = cov_rhs(Ae, P + dt * k3, Q)
    return P + (dt / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


def update(P, H, R, r, wrong_hp=False, wrong_r=False):
    """(P_new, delta).  S = symU(H symU(P) H' + R); K = (S^-1 H P)'; delta = K r; P_new = symU((I - K H) P)"""
    Rm = np.tril(R) + np.tril(R, -1).T if wrong_r else R
    S = symU(H @ symU(P) @ H.T + Rm)                                   # :129-130
    HP = H @ (symU(P) if wrong_hp else P)
    K = np.linalg.solve(S, HP).T                                        # :133-134
    return symU((np.eye(P.shape[0]) - K @ H) @ P), K @ r               # :137-138


def fused(P, A, Q, dt, H, R, r):
    return update(euler(P, A, Q, dt), H, R, r)


def ticks(P, A, Q, dt, H, R, r, count=3):
    delta = None
    for _ in range(count):
        P, delta = fused(P, A, Q, dt, H, R, r)
    return P, delta
