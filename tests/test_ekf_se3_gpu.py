"""The EKF on SE(3) -- host front EKF<SE3> (include/smooth_feedback_amd/ekf.hpp) and the device-resident swarm
(ekf_device.hpp) on the pose filter of examples/rigid_body_model.h (Dof 6, known body twist, position measured, Ny 3) --
against a numpy restatement of the reference's predict / update (ekf.hpp:79-139).  The restatement shares nothing with the
fronts, as in tests/test_ekf_group_gpu.py for the vehicle:

  * group arithmetic in MATRIX form (4x4 homogeneous matrices, exp by its power series, ad from the commutator), not through
    lie.hpp; the quaternion of the result is read off the rotation matrix (largest eigenvector of its symmetric 4x4 form) and
    compared up to its sign, q and -q being the same rotation;
  * ANALYTIC Jacobians: the twist does not depend on the pose, so A = -ad(f) (:86-87); p(g exp(a)) = p + R a_v + O(a^2), so
    H = [R 0] (:119);
  * the order of :94-97 (covariance first, then the state), the substep rule `while (t + dt < tau)` and the remainder
    (:93-102), the upper-triangle symmetrisations of :88, :130 and :138, the update through a solve with S (:133-134);
  * Euler and runge_kutta4, the covariance stages re-linearised at t, t + h/2, t + h at the frozen estimate, the state
    stepped on the group with the same tableau.

Tolerance.  Both fronts differentiate by forward differences with step sqrt(eps).  The restatement is therefore run a second
time with the same forward differences (float64): the gate is ten times the largest difference between the two restatements
over the inputs of this module,

    largest |analytic - forward-difference| restatement difference, all cases below:  1.34e-08   (states 1.34e-08, P 5.2e-09)
    GATE = 1.34e-07

which stays below the 1e-6 the host-vs-device test already allows (tests/test_ekf_device_gpu.py).
test_gate_is_ten_times_the_restatements_difference re-measures it without a GPU.  The front-vs-forward-difference
restatement differences are printed, not asserted."""
import numpy as np
import pytest

from examples import models_lib as M

GATE = 1.34e-07
FD = 1.4901161193847656e-08   # sqrt(DBL_EPSILON): the step of both fronts

MODES = [0, 1, 2, 3]                                   # 0: predict + update; 1, 2, 3: the fused step() variants
STEPPERS = [(0, 0.0), (0, 0.03), (1, 0.0), (1, 0.04)]  # (rk4, dt)
BATCHES = [1, 65, 1000]
STEPS = [1, 5]
TAU = 0.1

# hat of the basis vectors of se(3), tangent order (v0, v1, v2, w0, w1, w2)
_E = np.zeros((6, 4, 4))
for _i in range(3):
    _E[_i, _i, 3] = 1.0
_E[3, 2, 1], _E[3, 1, 2] = 1.0, -1.0
_E[4, 0, 2], _E[4, 2, 0] = 1.0, -1.0
_E[5, 1, 0], _E[5, 0, 1] = 1.0, -1.0


def _hat(a):
    return np.einsum("bi,ijk->bjk", a, _E)


def _vee(X):
    return np.stack([X[:, 0, 3], X[:, 1, 3], X[:, 2, 3], X[:, 2, 1], X[:, 0, 2], X[:, 1, 0]], axis=1)


def _expm(X):
    out, term = np.tile(np.eye(4), (len(X), 1, 1)), np.tile(np.eye(4), (len(X), 1, 1))
    for n in range(1, 40):                        # |X| stays below 3 here: 3^40 / 40! = 1.5e-29
        term = term @ X / n
        out = out + term
    return out


def _ad(a):
    """ad(a) e_i = vee([hat(a), hat(e_i)])"""
    A = _hat(a)
    return np.stack([_vee(A @ _E[i] - _E[i] @ A) for i in range(6)], axis=2)


def _rplus(g, a):
    return g @ _expm(_hat(a))


def _f(t, g):
    """PoseEkfDyn: the known body twist"""
    one = np.ones(len(g))
    return np.stack([(0.8 + 0.3 * np.cos(2.0 * t)) * one, 0.1 * np.sin(t) * one, 0.15 * one, 0.1 * one,
                     (-0.05 + 0.2 * np.sin(3.0 * t)) * one, 0.4 * one], axis=1)


def _h(g):
    """PoseEkfMeas: the position"""
    return g[:, :3, 3]


def _Q():
    Q = np.diag(0.02 + 0.01 * np.arange(6))
    Q[0, 1] = Q[1, 0] = 0.004
    Q[2, 4] = Q[4, 2] = -0.003
    return Q


def _R():
    R = np.diag([0.1, 0.12, 0.08])
    R[0, 1] = R[1, 0] = 0.01
    return R


def _symU(X):
    U = np.triu(X)
    return U + np.transpose(np.triu(X, 1), (0, 2, 1))


def _lin_dyn(t, g, fd):
    """A = -ad(f) + d^r f / dx at g (:86-87)"""
    B = len(g)
    fv = _f(t, g)
    dr = np.zeros((B, 6, 6))
    if fd:
        for c in range(6):
            e = np.zeros((B, 6))
            e[:, c] = FD
            dr[:, :, c] = (_f(t, _rplus(g, e)) - fv) / FD
    return dr - _ad(fv), fv


def _lin_meas(g, fd):
    """H = d^r h / dx (:119): the position moves by R a_v"""
    B = len(g)
    H = np.zeros((B, 3, 6))
    if fd:
        h0 = _h(g)
        for c in range(6):
            e = np.zeros((B, 6))
            e[:, c] = FD
            H[:, :, c] = (_h(_rplus(g, e)) - h0) / FD
    else:
        H[:, :, :3] = g[:, :3, :3]
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


def _rot_of_quat(q):
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def _quat_of_rot(R):
    """unit quaternion (w, x, y, z) of a rotation matrix, w >= 0: the dominant eigenvector of the symmetric 4x4 form"""
    K = np.zeros((len(R), 4, 4))
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    K[:, 0, 0] = tr
    K[:, 0, 1] = K[:, 1, 0] = R[:, 2, 1] - R[:, 1, 2]
    K[:, 0, 2] = K[:, 2, 0] = R[:, 0, 2] - R[:, 2, 0]
    K[:, 0, 3] = K[:, 3, 0] = R[:, 1, 0] - R[:, 0, 1]
    for i in range(3):
        K[:, 1 + i, 1 + i] = 2 * R[:, i, i] - tr
        for j in range(i + 1, 3):
            K[:, 1 + i, 1 + j] = K[:, 1 + j, 1 + i] = R[:, i, j] + R[:, j, i]
    q = np.linalg.eigh(K)[1][:, :, -1]
    return q * np.where(q[:, :1] < 0, -1.0, 1.0)


def restate(states, P0, y, tau, dt, rk4, fd):
    """len(y) rounds of predict(Q, tau, dt) + update(y[k], R); states [B][7] = (px, py, pz, w, x, y, z), P [B][36]"""
    B = len(states)
    g = np.tile(np.eye(4), (B, 1, 1))
    g[:, :3, :3] = _rot_of_quat(states[:, 3:7])
    g[:, :3, 3] = states[:, :3]
    P = np.transpose(P0.reshape(B, 6, 6), (0, 2, 1)).copy()            # column-major in, row-major here
    for k in range(len(y)):
        g, P = _predict(g, P, tau, dt, rk4, fd)
        g, P = _update(g, P, y[k], fd)
    st = np.concatenate([g[:, :3, 3], _quat_of_rot(g[:, :3, :3])], axis=1)
    return st, np.transpose(P, (0, 2, 1)).reshape(B, 36)


def state_difference(a, b):
    """largest difference of two sets of poses (p, q), the quaternions up to their sign"""
    s = np.where(np.sum(a[:, 3:] * b[:, 3:], axis=1, keepdims=True) < 0, -1.0, 1.0)
    return max(np.abs(a[:, :3] - b[:, :3]).max(), np.abs(a[:, 3:] - s * b[:, 3:]).max())


_INPUTS = {}


def _inputs(batch, steps):
    """poses with random rotations and positions of a few metres, SPD covariances, measurements near the positions"""
    if (batch, steps) not in _INPUTS:
        rng = np.random.default_rng(300 + batch + steps)
        q = rng.normal(size=(batch, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        st = np.concatenate([rng.uniform(-3, 3, (batch, 3)), q], axis=1)
        G = rng.uniform(-1, 1, (batch, 6, 6))
        P0 = (np.eye(6)[None] * 0.5 + G @ G.transpose(0, 2, 1) / 12).reshape(batch, 36)
        y = st[None, :, :3] + rng.normal(0, 0.2, (steps, batch, 3))
        _INPUTS[batch, steps] = (np.ascontiguousarray(st), np.ascontiguousarray(P0), np.ascontiguousarray(y))
    return _INPUTS[batch, steps]


_REF = {}


def _restated(batch, steps, dt, rk4, fd):
    key = (batch, steps, dt, rk4, fd)
    if key not in _REF:
        _REF[key] = restate(*_inputs(batch, steps), TAU, dt, rk4, fd)
    return _REF[key]


def _effective_dt(mode, dt):
    return 0.0 if mode else dt      # step() is ONE substep of length tau, whatever dt says (ekf_device.hpp)


def test_restatement_round_trips_the_quaternion():
    st, _, _ = _inputs(65, 1)
    q = _quat_of_rot(_rot_of_quat(st[:, 3:7]))
    assert state_difference(st, np.concatenate([st[:, :3], q], axis=1)) < 1e-14


def test_gate_is_ten_times_the_restatements_difference():
    """no GPU: the gate comes from the restatement alone, and stays within the host-vs-device tolerance 1e-6"""
    worst_s = worst_p = 0.0
    for batch in BATCHES:
        for steps in STEPS:
            for rk4, dt in STEPPERS:
                for d in {dt, 0.0}:
                    a = _restated(batch, steps, d, rk4, False)
                    b = _restated(batch, steps, d, rk4, True)
                    worst_s = max(worst_s, state_difference(a[0], b[0]))
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
    dev = M.pose_ekf_swarm_device(st, P0, y, tau=TAU, dt=dt, rk4=bool(rk4), fused=mode)
    ref_s, ref_p = _restated(batch, steps, _effective_dt(mode, dt), rk4, False)
    fd_s, fd_p = _restated(batch, steps, _effective_dt(mode, dt), rk4, True)
    ds, dp = state_difference(dev["states"], ref_s), np.abs(dev["P"] - ref_p).max()
    print("device mode %d rk4 %d dt %.2f B %d steps %d: vs analytic restatement states %.3g P %.3g | vs forward-difference "
          "restatement states %.3g P %.3g" % (mode, rk4, dt, batch, steps, ds, dp, state_difference(dev["states"], fd_s),
                                              np.abs(dev["P"] - fd_p).max()))
    assert np.all(dev["info"] == 0)
    assert ds <= GATE and dp <= GATE, (ds, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("rk4,dt", STEPPERS)
def test_host_filters_match_the_restatement(rk4, dt, batch, steps):
    """one host EKF<SE3> per filter (the covariance algebra of the host object runs on the device, too)"""
    st, P0, y = _inputs(batch, steps)
    host = M.pose_ekf_swarm_host(st, P0, y, tau=TAU, dt=dt, rk4=bool(rk4))
    ref_s, ref_p = _restated(batch, steps, dt, rk4, False)
    fd_s, fd_p = _restated(batch, steps, dt, rk4, True)
    ds, dp = state_difference(host["states"], ref_s), np.abs(host["P"] - ref_p).max()
    print("host rk4 %d dt %.2f B %d steps %d: vs analytic restatement states %.3g P %.3g | vs forward-difference restatement "
          "states %.3g P %.3g" % (rk4, dt, batch, steps, ds, dp, state_difference(host["states"], fd_s), np.abs(host["P"] - fd_p).max()))
    assert ds <= GATE and dp <= GATE, (ds, dp)
