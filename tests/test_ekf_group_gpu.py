"""The group-valued EKF -- host front EKF<X6> (include/smooth_feedback_amd/ekf.hpp) and the device-resident swarm
(ekf_device.hpp) -- against a numpy restatement of the reference's predict / update (ekf.hpp:79-139) for the vehicle
filter of examples/vehicle_model.h.  The restatement shares nothing with the fronts:

  * group arithmetic in MATRIX form (3x3 homogeneous SE(2) matrices, exp by its power series, ad from the commutator),
    not through lie.hpp;
  * ANALYTIC Jacobians: A = -blockdiag(ad_SE2(f_0..2), 0) + df/dx (:86-87), H = [R(theta) 0; e_v0] (:119);
  * the order of :94-97 (covariance first, then the state), the substep rule `while (t + dt < tau)` and the remainder
    (:93-102), the upper-triangle symmetrisations of :88, :130 and :138, the update through a solve with S (:133-134);
  * Euler and runge_kutta4, the covariance stages re-linearised at t, t + h/2, t + h at the frozen estimate, the state
    stepped on the group with the same tableau.

Tolerance.  Both fronts differentiate by forward differences with step sqrt(eps) and cannot meet an analytic restatement at
rounding level.  The restatement is therefore run a second time with the same forward differences (float64): the gate is
ten times the largest difference between the two restatements over the inputs of this module,

    largest |analytic - forward-difference| restatement difference, all cases below:  1.38e-08   (states 1.38e-08, P 3.3e-09)
    GATE = 1.4e-07

which stays below the 1e-6 the host-vs-device test already allows (tests/test_ekf_device_gpu.py).
test_gate_is_ten_times_the_restatements_difference re-measures it without a GPU.  The front-vs-forward-difference
restatement differences are printed, not asserted."""
import numpy as np
import pytest

from examples import models_lib as M

GATE = 1.4e-07
FD = 1.4901161193847656e-08   # sqrt(DBL_EPSILON): the step of both fronts

MODES = [0, 1, 2, 3]                                   # 0: predict + update; 1, 2, 3: the fused step() variants
STEPPERS = [(0, 0.0), (0, 0.03), (1, 0.0), (1, 0.04)]  # (rk4, dt)
BATCHES = [1, 65, 1000]
STEPS = [1, 5]
TAU = 0.1

# hat of the basis vectors of se(2), tangent order (vx, vy, omega)
_E = np.zeros((3, 3, 3))
_E[0, 0, 2] = 1.0
_E[1, 1, 2] = 1.0
_E[2, 1, 0], _E[2, 0, 1] = 1.0, -1.0


def _hat(a):
    return np.einsum("bi,ijk->bjk", a, _E)


def _vee(X):
    return np.stack([X[:, 0, 2], X[:, 1, 2], X[:, 1, 0]], axis=1)


def _expm(X):
    out, term = np.tile(np.eye(3), (len(X), 1, 1)), np.tile(np.eye(3), (len(X), 1, 1))
    for n in range(1, 40):                        # |X| stays below 3 here: 3^40 / 40! = 1.5e-29
        term = term @ X / n
        out = out + term
    return out


def _ad_se2(a):
    """ad(a) e_i = vee([hat(a), hat(e_i)])"""
    A = _hat(a)
    return np.stack([_vee(A @ _E[i] - _E[i] @ A) for i in range(3)], axis=2)


def _rplus(x, a):
    g, v = x
    return g @ _expm(_hat(a[:, :3])), v + a[:, 3:]


def _f(t, x):
    """VehicleEkfDyn: body velocity of the pose, first-order lags driven by the known input"""
    _, v = x
    u0, u1 = 0.3 * np.cos(2.0 * t), 0.2 * np.sin(3.0 * t)
    return np.stack([v[:, 0], v[:, 1], v[:, 2], -0.2 * v[:, 0] + u0, np.zeros(len(v)), -0.4 * v[:, 2] + u1], axis=1)


def _h(x):
    """VehicleEkfMeas: position and forward speed"""
    g, v = x
    return np.stack([g[:, 0, 2], g[:, 1, 2], v[:, 0]], axis=1)


def _Q():
    Q = np.diag(0.02 + 0.01 * np.arange(6))
    Q[0, 1] = Q[1, 0] = 0.004
    Q[3, 5] = Q[5, 3] = -0.003
    return Q


def _R():
    R = np.diag([0.1, 0.12, 0.05])
    R[0, 1] = R[1, 0] = 0.01
    return R


def _symU(X):
    U = np.triu(X)
    return U + np.transpose(np.triu(X, 1), (0, 2, 1))


def _lin_dyn(t, x, fd):
    """A = -ad(f) + d^r f / dx at x (:86-87)"""
    B = len(x[1])
    fv = _f(t, x)
    if fd:
        dr = np.zeros((B, 6, 6))
        for c in range(6):
            e = np.zeros((B, 6))
            e[:, c] = FD
            dr[:, :, c] = (_f(t, _rplus(x, e)) - fv) / FD
    else:
        dr = np.zeros((B, 6, 6))
        dr[:, 0, 3] = dr[:, 1, 4] = dr[:, 2, 5] = 1.0
        dr[:, 3, 3], dr[:, 5, 5] = -0.2, -0.4
    A = dr.copy()
    A[:, :3, :3] -= _ad_se2(fv[:, :3])
    return A, fv


def _lin_meas(x, fd):
    """H = d^r h / dx (:119): the position moves by R(theta) (a_0, a_1), the speed by a_3"""
    B = len(x[1])
    H = np.zeros((B, 3, 6))
    if fd:
        h0 = _h(x)
        for c in range(6):
            e = np.zeros((B, 6))
            e[:, c] = FD
            H[:, :, c] = (_h(_rplus(x, e)) - h0) / FD
    else:
        H[:, :2, :2] = x[0][:, :2, :2]
        H[:, 2, 3] = 1.0
    return H


def _cov_rhs(A, P, Q):
    return _symU(A @ P + P @ np.transpose(A, (0, 2, 1)) + Q)          # :88


def _predict(x, P, tau, dt, rk4, fd):
    Q = _Q()

    def step(t, h):
        nonlocal x, P
        A0, k1 = _lin_dyn(t, x, fd)
        if not rk4:
            P = P + h * _cov_rhs(A0, P, Q)                              # covariance first (:94-96) ...
            x = _rplus(x, h * k1)                                       # ... then the state (:97)
            return
        Am, _ = _lin_dyn(t + 0.5 * h, x, fd)                            # cov_ode linearises at the frozen estimate
        Ae, _ = _lin_dyn(t + h, x, fd)
        c1 = _cov_rhs(A0, P, Q)
        c2 = _cov_rhs(Am, P + 0.5 * h * c1, Q)
        c3 = _cov_rhs(Am, P + 0.5 * h * c2, Q)
        c4 = _cov_rhs(Ae, P + h * c3, Q)
        P = P + h / 6.0 * c1 + h / 3.0 * c2 + h / 3.0 * c3 + h / 6.0 * c4
        k2 = _f(t + 0.5 * h, _rplus(x, 0.5 * h * k1))
        k3 = _f(t + 0.5 * h, _rplus(x, 0.5 * h * k2))
        k4 = _f(t + h, _rplus(x, h * k3))
        x = _rplus(x, h * (k1 / 6.0 + k2 / 3.0 + k3 / 3.0 + k4 / 6.0))

    t, dt_v = 0.0, (dt if dt > 0 else 2 * tau)                          # :91-92
    while t + dt_v < tau:                                               # :93
        step(t, dt_v)
        t += dt_v
    step(t, tau - t)                                                    # :101-102
    return x, P


def _update(x, P, y, fd):
    R = _R()
    H = _lin_meas(x, fd)
    Ht = np.transpose(H, (0, 2, 1))
    S = _symU(H @ _symU(P) @ Ht + R)                                    # :129-130, used as selfadjointView<Upper>
    K = np.transpose(np.linalg.solve(S, H @ P), (0, 2, 1))              # :133-134
    delta = np.einsum("bij,bj->bi", K, y - _h(x))
    x = _rplus(x, delta)                                                # :137
    P = _symU((np.eye(6) - K @ H) @ P)                                  # :138
    return x, P


def restate(states, P0, y, tau, dt, rk4, fd):
    """len(y) rounds of predict(Q, tau, dt) + update(y[k], R); states [B][7] = (x, y, cos, sin, v0, v1, v2), P [B][36]"""
    B = len(states)
    g = np.zeros((B, 3, 3))
    g[:, 0, 0], g[:, 0, 1], g[:, 0, 2] = states[:, 2], -states[:, 3], states[:, 0]
    g[:, 1, 0], g[:, 1, 1], g[:, 1, 2] = states[:, 3], states[:, 2], states[:, 1]
    g[:, 2, 2] = 1.0
    x = (g, states[:, 4:7].copy())
    P = np.transpose(P0.reshape(B, 6, 6), (0, 2, 1)).copy()            # column-major in, row-major here
    for k in range(len(y)):
        x, P = _predict(x, P, tau, dt, rk4, fd)
        x, P = _update(x, P, y[k], fd)
    g, v = x
    st = np.concatenate([g[:, 0, 2:3], g[:, 1, 2:3], g[:, 0, 0:1], g[:, 1, 0:1], v], axis=1)
    return st, np.transpose(P, (0, 2, 1)).reshape(B, 36)


def _inputs(batch, steps):
    return M.ekf_swarm_inputs(batch, steps, seed=100 + batch + steps)


def _effective_dt(mode, dt):
    return 0.0 if mode else dt      # step() is ONE substep of length tau, whatever dt says (ekf_device.hpp)


def test_gate_is_ten_times_the_restatements_difference():
    """no GPU: the gate comes from the restatement alone, and stays within the host-vs-device tolerance 1e-6"""
    worst_s = worst_p = 0.0
    for batch in BATCHES:
        for steps in STEPS:
            st, P0, y = _inputs(batch, steps)
            for rk4, dt in STEPPERS:
                a = restate(st, P0, y, TAU, dt, rk4, fd=False)
                b = restate(st, P0, y, TAU, dt, rk4, fd=True)
                worst_s = max(worst_s, np.abs(a[0] - b[0]).max())
                worst_p = max(worst_p, np.abs(a[1] - b[1]).max())
    print("analytic vs forward-difference restatement: states %.3g  P %.3g  -> gate %.3g" % (worst_s, worst_p, 10 * max(worst_s, worst_p)))
    assert GATE <= 1e-6
    assert 10 * max(worst_s, worst_p) <= GATE * 1.05 and GATE <= 12 * max(worst_s, worst_p)


@pytest.mark.gpu
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("rk4,dt", STEPPERS)
@pytest.mark.parametrize("mode", MODES)
def test_device_swarm_matches_the_restatement(mode, rk4, dt, batch, steps):
    st, P0, y = _inputs(batch, steps)
    dev = M.ekf_swarm_device(st, P0, y, tau=TAU, dt=dt, rk4=bool(rk4), fused=mode)
    ref_s, ref_p = restate(st, P0, y, TAU, _effective_dt(mode, dt), rk4, fd=False)
    fd_s, fd_p = restate(st, P0, y, TAU, _effective_dt(mode, dt), rk4, fd=True)
    ds, dp = np.abs(dev["states"] - ref_s).max(), np.abs(dev["P"] - ref_p).max()
    print("device mode %d rk4 %d dt %.2f B %d steps %d: vs analytic restatement states %.3g P %.3g | vs forward-difference "
          "restatement states %.3g P %.3g" % (mode, rk4, dt, batch, steps, ds, dp, np.abs(dev["states"] - fd_s).max(),
                                              np.abs(dev["P"] - fd_p).max()))
    assert np.all(dev["info"] == 0)
    assert ds <= GATE and dp <= GATE, (ds, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("rk4,dt", STEPPERS)
def test_host_filters_match_the_restatement(rk4, dt, batch, steps):
    """one host EKF<X6> per filter (the covariance algebra of the host object runs on the device, too)"""
    st, P0, y = _inputs(batch, steps)
    host = M.ekf_swarm_host(st, P0, y, tau=TAU, dt=dt, rk4=bool(rk4))
    ref_s, ref_p = restate(st, P0, y, TAU, dt, rk4, fd=False)
    fd_s, fd_p = restate(st, P0, y, TAU, dt, rk4, fd=True)
    ds, dp = np.abs(host["states"] - ref_s).max(), np.abs(host["P"] - ref_p).max()
    print("host rk4 %d dt %.2f B %d steps %d: vs analytic restatement states %.3g P %.3g | vs forward-difference restatement "
          "states %.3g P %.3g" % (rk4, dt, batch, steps, ds, dp, np.abs(host["states"] - fd_s).max(), np.abs(host["P"] - fd_p).max()))
    assert ds <= GATE and dp <= GATE, (ds, dp)
