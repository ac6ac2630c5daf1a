"""Generates tests/golden/mesh_reference.npz: inputs and float64-rounded results of the ph collocation mesh of
include/smooth_feedback_amd/mesh.hpp (Mesh<Kmin, Kmax>) and of the dynamics-error estimate of dyn_error.hpp, computed with
mpmath at 60 digits.  Nothing goes through the headers, tests/mesh_ref.py or numpy arithmetic: numpy only supplies start
values for the node search and stores the rounded results.

  lgr       K = 1 .. 15: the K Legendre-Gauss-Radau nodes on [-1, 1) (-1 and the roots of P_{K-1} + P_K, each polished by
            mpmath.findroot and checked: residual, order, the weights sum to 2) and weights
            w_0 = 2 / K^2, w_i = (1 - x_i) / (K P_{K-1}(x_i))^2.
  mesh.*    meshes made by op scripts (spec = Kmin, Kmax, n, k of the constructor; ops rows (code, a, b): 0 refine_ph(a, b),
            1 increase_degrees, 2 decrease_degrees, 3 set_N_colloc_ival(a, b), 4 refine_errors, which takes its target and
            its errors, in this order, from opdata): K, tau0, all nodes, all weights, and per interval the (K + 1) x K
            differentiation matrix D(j, i) = l_j'(tau_i) (2 / width) over the K + 1 points and the K x K integration matrix
            inverse(D[1:, :]) (mpmath.inverse), both row-major and concatenated.
  eval.*    p = 0, 1, 2 (derivative with respect to the interval's own variable u in [-1, 1], as the reference's eval), at
            times below 0, at 0, interior, exactly on an interval start, at 1 and above 1, with the values extended by the
            one at 1 and not (the last interval then uses its own K points): out [2][3][nt][dim], out[0] is extend = true.
  resample.* per mesh: the degree-raised mesh's points tau [R]; node values vals [N + 1][3] (doubles) and the mesh polynomials
            through them at those points, out_ext [R][3] from all N + 1 values and out_open [R][3] from the first N (the last interval then uses
            its own K points), R = sum (K + 2), interval by interval with both end points.
  dynerr.*  per case: a base mesh (by name), t0, tf, node samples vals_x [N + 1][nx] and vals_u [N][nu] ROUNDED TO DOUBLE and
            from there on exact, the mesh polynomials through them at the degree-raised mesh's points X, U [R][.], the
            dynamics F there, and errs [nivals] (the estimate of dyn_error.hpp on the raised mesh).  Dynamics: fid 0 time
            only, f_d(t) = d/dt sum_k c_dk t^k with the samples from the same polynomial (degree <= 3: class exact);
            fid 1 harmonic pairs (x2, -x1) with samples (sin(t + p), cos(t + p)) (class resolved); fid 2 a pendulum with
            input, (x2, -sin x1 + u_{pair mod nu}), audited on the same harmonic samples (class coarse).  cls is decided
            by the largest interval error: exact <= 1e-13, resolved in [1e-10, 1e-4], coarse >= 1e-3; asserted here.
  flat.*    flat_dynamics (dyn_error.hpp; the reference's FlatDyn::operator()) of the two example models, vehicle = SE2 x R^3
            with inputs R^2 and rigid = SE3 x R^6 with inputs R^6, IN MATRIX FORM (hat, vee, the power series of the matrix
            exponential: those of make_golden_pid.py next to this file): x = xl exp(hat(e)), u = ul + v,
            out = J (f(x, u) - dxl) + ad(e) dxl per part with ad(a) b = vee(hat(a) hat(b) - hat(b) hat(a)) and
            J = d^r exp^-1(e) = sum_n (-1)^n B_n / n! ad(e)^n (Bernoulli numbers, summed until the terms vanish at 60 digits).
            Classes by |e|: tiny <= 1e-9, generic <= 1.2; six rows each.
  audit.*   MPC::dyn_error on synthetic smooth plans (not QP solutions) of the example MPCs: the primal [dx_0 .. dx_N | du_0 ..
            du_{N-1}] (doubles) on Mesh<4, 4>(nivals), e(tau) / v(tau) the mesh polynomials through it (x extended by the
            value at 1, u not), the dynamics flat_dynamics around the model's desired trajectory -- whose body velocity,
            velocity part and input are constant in time for all three models, so the time of the tick does not enter --
            audited on the mesh raised by one degree over the horizon tf: errs [nivals].  Models: vehicle6 (SE2 x R^3),
            vehicle12 (two such vehicles on one input pair), rigid (SE3 x R^6).
Run by hand from the repository root (a few seconds):  python tests/golden/make_golden_mesh.py"""
import importlib.util
import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_pid", os.path.join(HERE, "make_golden_pid.py"))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)          # the matrix forms; sets mp.mp.dps = 60
assert mp.mp.dps == 60
CLASSES = ["exact", "resolved", "coarse"]


def f64(x):
    """mpmath numbers (nested lists, or a matrix) rounded to float64"""
    return np.array(x.tolist() if isinstance(x, mp.matrix) else x, dtype=object).astype(np.float64)


def mpf(x):
    return mp.mpf(float(x))


_LGR = {}


def lgr(K):
    if K in _LGR:
        return _LGR[K]
    c = np.zeros(K + 1)
    c[K] = 1.0
    c[K - 1] = 1.0
    guess = sorted(np.polynomial.legendre.legroots(c).real)
    g = lambda t: mp.legendre(K - 1, t) + mp.legendre(K, t)                     # noqa: E731
    x = [mp.mpf(-1)]
    for s in guess[1:]:
        r = mp.findroot(g, mp.mpf(float(s)))
        assert abs(g(r)) < mp.mpf(10) ** -50 and abs(r - s) < 1e-6
        x.append(r)
    assert all(a < b for a, b in zip(x, x[1:])) and x[-1] < 1
    w = [mp.mpf(2) / K ** 2] + [(1 - xi) / (K * mp.legendre(K - 1, xi)) ** 2 for xi in x[1:]]
    assert abs(sum(w) - 2) < mp.mpf(10) ** -50
    _LGR[K] = (x, w)
    return _LGR[K]


def lagrange(x, u, p):
    """d^p/du^p of every Lagrange basis polynomial through the points x, at u"""
    n, W = len(x), []
    for j in range(n):
        den = mp.fprod(x[j] - x[k] for k in range(n) if k != j)
        o = [k for k in range(n) if k != j]
        if p == 0:
            num = mp.fprod(u - x[k] for k in o)
        elif p == 1:
            num = mp.fsum(mp.fprod(u - x[k] for k in o if k != m) for m in o)
        else:
            num = mp.fsum(mp.fprod(u - x[k] for k in o if k not in (m, l)) for m in o for l in o if l != m)
        W.append(num / den)
    return W


class Mesh:
    def __init__(self, kmin, kmax, n, k):
        self.kmin, self.kmax = kmin, kmax
        self.iv = [[k, mp.mpf(0)]] if n < 2 else [[k, mp.mpf(i) / n] for i in range(n)]

    def end(self, i):
        return self.iv[i + 1][1] if i + 1 < len(self.iv) else mp.mpf(1)

    def refine_ph(self, i, D):
        if D > self.kmax or self.iv[i][0] > self.kmax:
            n = max(2, -(-D // self.kmin))
            t0, tf = self.iv[i][1], self.end(i)
            self.iv[i + 1:i + 1] = [[self.kmin, t0 + (tf - t0) * j / n] for j in range(1, n)]
        elif D >= self.iv[i][0]:
            self.iv[i][0] = D

    def refine_errors(self, errs, target):
        for i in reversed(range(len(self.iv))):
            K = self.iv[i][0]
            if errs[i] > target:
                self.refine_ph(i, K + int(mp.nint(mp.log(errs[i] / target) / mp.log(K) + 1)))

    def run(self, ops, opdata):
        at = 0
        for code, a, b in ops:
            if code == 0:
                self.refine_ph(a, b)
            elif code == 1:
                for v in self.iv:
                    v[0] = min(v[0] + 1, self.kmax + 1)
            elif code == 2:
                for v in self.iv:
                    v[0] = max(v[0] - 1, self.kmin)
            elif code == 3:
                self.iv[a][0] = b
            else:
                n = len(self.iv)
                self.refine_errors([mpf(e) for e in opdata[at + 1:at + 1 + n]], mpf(opdata[at]))
                at += 1 + n
        return self

    def K(self, i):
        return self.iv[i][0]

    def nodes(self, i):
        x = lgr(self.K(i))[0] + [mp.mpf(1)]
        t0, al = self.iv[i][1], (self.end(i) - self.iv[i][1]) / 2
        return [t0 + al * (v + 1) for v in x]

    def weights(self, i):
        al = (self.end(i) - self.iv[i][1]) / 2
        return [al * v for v in lgr(self.K(i))[1] + [mp.mpf(0)]]

    def all(self, f):
        out = []
        for i in range(len(self.iv)):
            v = f(i)
            out += v if i + 1 == len(self.iv) else v[:-1]
        return out

    def diffmat(self, i):
        K = self.K(i)
        x = lgr(K)[0] + [mp.mpf(1)]
        al = 2 / (self.end(i) - self.iv[i][1])
        D = mp.zeros(K + 1, K)
        for c in range(K):
            W = lagrange(x, x[c], 1)
            for j in range(K + 1):
                D[j, c] = al * W[j]
        return D

    def intmat(self, i):
        D = self.diffmat(i)
        return mp.inverse(D[1:, :])

    def find(self, t):
        if t < 0:
            return 0
        if t > 1:
            return len(self.iv) - 1
        return max(i for i in range(len(self.iv)) if self.iv[i][1] <= t)

    def eval(self, t, vals, p, extend):
        return self.eval_in(self.find(t), t, vals, extend, p)

    def eval_in(self, i, t, vals, extend, p=0):
        """the polynomial of interval i at t (also at the interval's end point, where find() moves on)"""
        K = self.K(i)
        u = 2 * (t - self.iv[i][1]) / (self.end(i) - self.iv[i][1]) - 1
        before = sum(self.K(s) for s in range(i))
        closed = extend or i + 1 < len(self.iv)
        x = lgr(K)[0] + ([mp.mpf(1)] if closed else [])
        W = lagrange(x, u, p)
        return [mp.fsum(W[j] * vals[before + j][d] for j in range(len(x))) for d in range(len(vals[0]))] if len(vals[0]) else []

    def raised(self):
        m = Mesh(self.kmin, self.kmax, 1, 1)
        m.iv = [[k + 1, t] for k, t in self.iv]
        return m


MESHES = {  # name: (Kmin, Kmax, n, k, ops, opdata)
    "basic": (5, 10, 1, 5, [(0, 0, 50), (0, 1, 10), (0, 1, 13), (0, 2, 27), (0, 7, 33), (0, 9, 22)], []),
    "k3567": (3, 6, 4, 3, [(3, 1, 4), (3, 2, 5), (3, 3, 6), (1, 0, 0), (3, 0, 3)], []),
    "u13": (4, 4, 13, 4, [], []),
    "ref16": (5, 5, 1, 5, [(0, 0, 80)], []),
    "one4": (4, 4, 1, 4, [], []),
    "two4": (4, 4, 2, 4, [], []),
    "three5": (5, 5, 3, 5, [], []),
    "mixed": (3, 6, 3, 3, [(3, 1, 5), (3, 2, 6)], []),
    "updown": (8, 8, 1, 8, [(0, 0, 40), (1, 0, 0), (1, 0, 0), (2, 0, 0)], []),
    "k13": (13, 13, 2, 13, [], []),
    "errs": (5, 10, 4, 5, [(4, 0, 0), (1, 0, 0)], [1e-6, 1e-9, 3e-5, 2e-6, 0.5]),
}


def build(name):
    kmin, kmax, n, k, ops, opdata = MESHES[name]
    return Mesh(kmin, kmax, n, k).run(ops, opdata)


def mesh_section(name):
    kmin, kmax, n, k, ops, opdata = MESHES[name]
    m = build(name)
    pre = "mesh.%s." % name
    N = len(m.iv)
    return {
        pre + "spec": np.array([kmin, kmax, n, k], dtype=np.int32),
        pre + "ops": np.array(ops, dtype=np.int32).reshape(-1, 3),
        pre + "opdata": np.array(opdata, dtype=np.float64),
        pre + "K": np.array([m.K(i) for i in range(N)], dtype=np.int32),
        pre + "tau0": f64([v[1] for v in m.iv]),
        pre + "nodes": f64(m.all(m.nodes)),
        pre + "weights": f64(m.all(m.weights)),
        pre + "diffmat": np.concatenate([f64(m.diffmat(i)).ravel() for i in range(N)]),
        pre + "intmat": np.concatenate([f64(m.intmat(i)).ravel() for i in range(N)]),
    }


def eval_section(name):
    m = build(name)
    nodes = f64(m.all(m.nodes))
    vals = np.stack([np.sin(3 * nodes) + nodes ** 2, np.cos(2 * nodes) - 0.5 * nodes], axis=1)
    b1, b2 = float(f64([m.iv[1][1]])[0]), float(f64([m.iv[len(m.iv) // 2][1]])[0])
    t = np.array([-0.25, 0.0, 0.013, 0.37, b1, b2, 0.77, 0.999, 1.0, 1.3])
    V = [[mpf(v) for v in row] for row in vals]
    out = np.zeros((2, 3, len(t), 2))
    for e, extend in enumerate((True, False)):
        for p in range(3):
            for k, tk in enumerate(t):
                out[e, p, k] = f64(m.eval(mpf(tk), V if extend else V[:-1], p, extend))
    pre = "eval.%s." % name
    return {pre + "t": t, pre + "vals": vals, pre + "out": out}


def resample_section(name):
    m = build(name)
    nodes = f64(m.all(m.nodes))
    vals = np.stack([np.sin(3 * nodes) + nodes ** 2, np.cos(2 * nodes) - 0.5 * nodes, 1.0 + nodes - 2 * nodes ** 3], axis=1)
    V = [[mpf(v) for v in row] for row in vals]
    up = m.raised()
    taus = [t for i in range(len(up.iv)) for t in up.nodes(i)]
    ivals = [i for i in range(len(up.iv)) for _ in up.nodes(i)]
    pre = "resample.%s." % name
    return {pre + "vals": vals, pre + "tau": f64(taus), pre + "out_ext": f64([m.eval_in(i, t, V, True) for i, t in zip(ivals, taus)]),
            pre + "out_open": f64([m.eval_in(i, t, V[:-1], False) for i, t in zip(ivals, taus)])}


# ---------------------------------------------------------------- dynamics-error cases
def dyn_f(fid, coef, nu, t, x, u):
    if fid == 0:
        return [mp.fsum(k * coef[d][k] * t ** (k - 1) for k in range(1, len(coef[d]))) for d in range(len(x))]
    out = []
    for p in range(len(x) // 2):
        x1, x2 = x[2 * p], x[2 * p + 1]
        out += [x2, -x1] if fid == 1 else [x2, -mp.sin(x1) + u[p % nu]]
    return out


def samples(fid, coef, nx, t):
    if fid == 0:
        return [mp.fsum(coef[d][k] * t ** k for k in range(len(coef[d]))) for d in range(nx)]
    return [(mp.sin if d % 2 == 0 else mp.cos)(t + mp.mpf(d // 2) / 3) for d in range(nx)]


def input_samples(nu, t):
    return [mp.mpf(3) / 10 * mp.cos(2 * t + d) for d in range(nu)]


REF_COEF = [[0.2, -0.4, 0.1, 0.0]]
DYN_CASES = [  # name, mesh, fid, nx, nu, t0, tf
    ("ex_ref", "ref16", 0, 1, 0, 3.0, 5.0),
    ("ex_one4", "one4", 0, 2, 1, 0.0, 1.5),
    ("ex_u13", "u13", 0, 12, 2, -1.0, 2.0),
    ("ex_mixed", "mixed", 0, 2, 0, 0.5, 2.5),
    ("ex_three5", "three5", 0, 1, 1, 0.0, 1.0),
    ("re_two4", "two4", 1, 2, 0, 0.0, 1.0),
    ("re_u13", "u13", 1, 2, 1, 0.0, 2.0),
    ("re_u13x12", "u13", 1, 12, 2, 0.0, 2.0),
    ("re_three5", "three5", 1, 2, 0, 0.0, 1.0),
    ("re_mixed", "mixed", 1, 2, 2, 0.0, 0.6),
    ("co_one4", "one4", 2, 2, 1, 0.0, 1.0),
    ("co_two4", "two4", 2, 2, 1, 0.0, 1.0),
    ("co_three5", "three5", 2, 12, 2, 0.0, 1.0),
    ("co_mixed", "mixed", 2, 2, 2, 0.0, 1.0),
    ("co_u13", "u13", 2, 2, 1, 0.0, 2.0),
    ("ex_k13", "k13", 0, 2, 0, 0.0, 1.5),        # the largest degree the kernels take: K + 1 = 14 raised points
    ("co_k13", "k13", 2, 12, 2, 0.0, 2.0),
    ("co_basic", "basic", 2, 2, 1, 0.0, 6.0),    # 27 intervals of K = 5 and 10
]


def case_coef(name, nx):
    if name == "ex_ref":
        return REF_COEF
    rng = np.random.default_rng(sum(map(ord, name)))
    return np.round(rng.uniform(-1, 1, (nx, 4)), 3).tolist()


def dyn_section(case):
    name, mesh_name, fid, nx, nu, t0, tf = case
    base = build(mesh_name)
    coef = case_coef(name, nx) if fid == 0 else []
    C = [[mpf(c) for c in row] for row in coef]
    T0, TF = mpf(t0), mpf(tf)
    tn = [T0 + (TF - T0) * v for v in base.all(base.nodes)]
    vals_x = f64([samples(fid, C, nx, t) for t in tn])
    vals_u = f64([input_samples(nu, t) for t in tn[:-1]]).reshape(len(tn) - 1, nu)
    VX = [[mpf(v) for v in row] for row in vals_x]
    VU = [[mpf(v) for v in row] for row in vals_u]
    up = base.raised()
    X, U, F, errs = [], [], [], []
    for i in range(len(up.iv)):
        taus = up.nodes(i)
        Xi = [base.eval(tau, VX, 0, True) for tau in taus]
        Ui = [base.eval(tau, VU, 0, False) if nu else [] for tau in taus]
        Fi = [dyn_f(fid, C, nu, T0 + (TF - T0) * tau, x, u) for tau, x, u in zip(taus, Xi, Ui)]
        Ke, I = up.K(i), up.intmat(i)
        est = [[Xi[0][d] + (TF - T0) * mp.fsum(Fi[r][d] * I[r, j - 1] for r in range(Ke)) for d in range(nx)] for j in range(1, Ke + 1)]
        e = [mp.sqrt(mp.fsum((est[j - 1][d] - Xi[j][d]) ** 2 for d in range(nx))) for j in range(1, Ke + 1)]
        xn = max(mp.sqrt(mp.fsum(v ** 2 for v in Xi[j])) for j in range(1, Ke + 1))
        errs.append(max(e) / (1 + xn))
        X += Xi
        U += Ui
        F += Fi
    worst = max(errs)
    cls = 0 if worst <= mp.mpf("1e-13") else (1 if mp.mpf("1e-10") <= worst <= mp.mpf("1e-4") else (2 if worst >= mp.mpf("1e-3") else -1))
    assert cls == ("ex", "re", "co").index(name[:2]), (name, mp.nstr(worst, 5))
    print("%-10s %-7s nx %2d nu %d  worst interval error %s -> %s" % (name, mesh_name, nx, nu, mp.nstr(worst, 4), CLASSES[cls]))
    R = len(X)
    pre = "dynerr.%s." % name
    return {
        pre + "mesh": np.array(mesh_name), pre + "fid": np.int32(fid), pre + "coef": np.array(coef, dtype=np.float64).reshape(-1, 4),
        pre + "nx": np.int32(nx), pre + "nu": np.int32(nu), pre + "t0": np.float64(t0), pre + "tf": np.float64(tf), pre + "cls": np.int32(cls),
        pre + "vals_x": vals_x, pre + "vals_u": vals_u,
        pre + "X": f64(X).reshape(R, nx), pre + "U": f64(U).reshape(R, nu) if nu else np.zeros((R, 0)), pre + "F": f64(F).reshape(R, nx),
        pre + "errs": f64(errs),
    }


# ---------------------------------------------------------------- flattened dynamics, matrix form
FLAT_CLASSES = ["tiny", "generic"]
FLAT_MODELS = {"vehicle": ("SE2", 3, 2), "rigid": ("SE3", 6, 6)}     # pose kind, pose dof (= velocity count), inputs
RIGID_DAMPING = [0.2, 0.3, 0.25, 0.4, 0.35, 0.5]


def model_f(model, vel, u):
    """the example models' dynamics: (pose rate, velocity rate) from the body velocities and the inputs"""
    if model == "vehicle":
        return list(vel) + [mpf(-0.2) * vel[0] + u[0], mp.mpf(0), mpf(-0.4) * vel[2] + u[1]]
    return list(vel) + [u[i] - mpf(RIGID_DAMPING[i]) * vel[i] for i in range(6)]


def ad_apply(kind, a, b):
    A, B = P.hat(kind, a), P.hat(kind, b)
    return P.vee(kind, A * B - B * A)


def dr_expinv_apply(kind, a, d):
    out, term, n = list(d), list(d), 0
    while True:
        n += 1
        term = ad_apply(kind, a, term)                         # ad(a)^n d
        c = (-1) ** n * mp.bernoulli(n) / mp.factorial(n)
        out = [o + c * t for o, t in zip(out, term)]
        if n > 4 and max(abs(t) for t in term) * (abs(c) if c else mp.mpf(10) ** -30) < mp.mpf(10) ** -70:
            return out
        assert n < 400


def flat_section(model):
    kind, D, Nu = FLAT_MODELS[model]
    rng = np.random.default_rng(31 + D)
    rows = {k: [] for k in ("xl", "dxl", "ul", "e", "v", "out", "cls")}
    for ci, cls in enumerate(FLAT_CLASSES):
        for _ in range(6):
            th = rng.uniform(-3, 3)
            if kind == "SE2":
                pose = [rng.uniform(-2, 2), rng.uniform(-2, 2), np.cos(th), np.sin(th)]
            else:
                q = rng.normal(size=4)
                q = q / np.linalg.norm(q) * np.sign(q[0])
                pose = list(rng.uniform(-2, 2, 3)) + list(q)
            xl = np.array(pose + list(rng.uniform(-1, 1, D)))
            dxl, ul, v = rng.uniform(-1, 1, 2 * D), rng.uniform(-0.5, 0.5, Nu), rng.uniform(-0.3, 0.3, Nu)
            e = rng.normal(size=2 * D)
            e = e / np.linalg.norm(e) * (rng.uniform(1e-10, 1e-9) if cls == "tiny" else rng.uniform(0.3, 1.2))
            E = [mpf(c) for c in e]
            vel = [mpf(a) + b for a, b in zip(xl[-D:], E[D:])]                      # the R^D part of xl (+) e
            f = model_f(model, vel, [mpf(a) + mpf(b) for a, b in zip(ul, v)])
            d = [a - mpf(b) for a, b in zip(f, dxl)]
            pose_out = [a + b for a, b in zip(dr_expinv_apply(kind, E[:D], d[:D]), ad_apply(kind, E[:D], [mpf(c) for c in dxl[:D]]))]
            out = pose_out + d[D:]                                                  # R^D: J = 1, ad = 0
            for k, val in (("xl", xl), ("dxl", dxl), ("ul", ul), ("e", e), ("v", v), ("out", f64(out)), ("cls", ci)):
                rows[k].append(val)
    pre = "flat.%s." % model
    return {pre + k: np.array(val, dtype=np.int32 if k == "cls" else np.float64) for k, val in rows.items()}


# ---------------------------------------------------------------- MPC plans audited against the flattened dynamics
# model: [(pose kind, dof, desired body velocity, damping on (v_0, v_2) or on every velocity)], inputs
AUDIT_MODELS = {
    "vehicle6": ([("SE2", 3, [1.0, 0.0, 0.4], [0.2, 0.4])], 2),
    "vehicle12": ([("SE2", 3, [1.0, 0.0, 0.4], [0.2, 0.4]), ("SE2", 3, [0.8, 0.0, 0.3], [0.3, 0.5])], 2),
    "rigid": ([("SE3", 6, [0.8, 0.0, 0.15, 0.1, -0.05, 0.4], RIGID_DAMPING)], 6),
}
AUDIT_CASES = [("v6_2", "vehicle6", 8, 2.0), ("v6_13", "vehicle6", 50, 5.0), ("v12_2", "vehicle12", 8, 2.0), ("rigid_2", "rigid", 8, 2.0)]


def audit_flat(model, e, v):
    """flat_dynamics of the model around its desired trajectory at deviation e, input deviation v (lists of mpf)"""
    blocks, nu = AUDIT_MODELS[model]
    out, o = [], 0
    for kind, D, twist, damp in blocks:
        tw = [mpf(c) for c in twist]
        vel = [a + b for a, b in zip(tw, e[o + D:o + 2 * D])]
        if kind == "SE2":   # udes = 0: u = v
            acc = [-mpf(damp[0]) * vel[0] + v[0], mp.mpf(0), -mpf(damp[1]) * vel[2] + v[1]]
        else:               # udes = damping * twist
            acc = [mpf(damp[i]) * tw[i] + v[i] - mpf(damp[i]) * vel[i] for i in range(D)]
        d = [a - b for a, b in zip(vel, tw)]                                   # f_pose - dxl_pose
        ep = e[o:o + D]
        out += [a + b for a, b in zip(dr_expinv_apply(kind, ep, d), ad_apply(kind, ep, tw))] + acc   # dxl_vel = 0
        o += 2 * D
    return out


def audit_section(case):
    name, model, K, tf = case
    blocks, nu = AUDIT_MODELS[model]
    nx = sum(2 * b[1] for b in blocks)
    nivals = -(-K // 4)
    base = Mesh(4, 4, nivals, 4)
    nodes = f64(base.all(base.nodes))
    N = len(nodes) - 1
    dx = np.stack([0.25 / (1 + d % 3) * np.sin((1.5 + 0.3 * d) * tf * nodes + 0.7 * d) for d in range(nx)], axis=1)
    du = np.stack([0.2 * np.cos((2.0 + d) * tf * nodes[:-1] + d) for d in range(nu)], axis=1)
    primal = np.concatenate([dx.ravel(), du.ravel()])
    VX = [[mpf(c) for c in row] for row in dx]
    VU = [[mpf(c) for c in row] for row in du]
    up, errs, TF = base.raised(), [], mpf(tf)
    for i in range(nivals):
        taus = up.nodes(i)
        Xi = [base.eval_in(i, tau, VX, True) for tau in taus]
        Fi = [audit_flat(model, x, base.eval_in(i, tau, VU, False)) for tau, x in zip(taus[:-1], Xi)]
        Ke, I = up.K(i), up.intmat(i)
        est = [[Xi[0][d] + TF * mp.fsum(Fi[r][d] * I[r, j - 1] for r in range(Ke)) for d in range(nx)] for j in range(1, Ke + 1)]
        e = [mp.sqrt(mp.fsum((est[j - 1][d] - Xi[j][d]) ** 2 for d in range(nx))) for j in range(1, Ke + 1)]
        errs.append(max(e) / (1 + max(mp.sqrt(mp.fsum(c ** 2 for c in Xi[j])) for j in range(1, Ke + 1))))
    print("%-8s %-9s K %2d: interval errors %s .. %s" % (name, model, K, mp.nstr(min(errs), 3), mp.nstr(max(errs), 3)))
    pre = "audit.%s." % name
    return {pre + "model": np.array(model), pre + "K": np.int32(K), pre + "tf": np.float64(tf), pre + "t": np.float64(0.3),
            pre + "primal": primal, pre + "errs": f64(errs)}


def main():
    fx = {"classes": np.array(CLASSES), "mesh.names": np.array(list(MESHES)), "dynerr.names": np.array([c[0] for c in DYN_CASES]),
          "eval.names": np.array(["basic", "k3567"])}
    for K in range(1, 16):
        x, w = lgr(K)
        fx["lgr.K%d.x" % K], fx["lgr.K%d.w" % K] = f64(x), f64(w)
    for name in MESHES:
        fx.update(mesh_section(name))
    for name in ("basic", "k3567"):
        fx.update(eval_section(name))
    for name in MESHES:
        fx.update(resample_section(name))
    for case in DYN_CASES:
        fx.update(dyn_section(case))
    fx["flat.classes"], fx["flat.names"] = np.array(FLAT_CLASSES), np.array(list(FLAT_MODELS))
    for model in FLAT_MODELS:
        fx.update(flat_section(model))
    fx["audit.names"] = np.array([c[0] for c in AUDIT_CASES])
    for case in AUDIT_CASES:
        fx.update(audit_section(case))
    path = os.path.join(HERE, "mesh_reference.npz")
    np.savez_compressed(path, **fx)
    print("wrote %s: %d arrays, %d bytes" % (path, len(fx), os.path.getsize(path)))


if __name__ == "__main__":
    main()
