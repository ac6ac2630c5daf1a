"""The batched mesh-function kernels (smooth_feedback_amd/csrc/mesh.hip through sfb_mesh_eval_batch*, sfb_mesh_integrate_batch*
and sfb_mesh_dyn_batch*) against the 60-digit fixture tests/golden/meshfn_reference.npz, within the gates of
tests/meshfn_gates.py (four times the float64 numpy restatement's own error per class).  The kernels are model-free: the
integrand's values and Jacobians at the nodes come from tests/meshfn_ref.py in float64.  In a batch the even agents carry the
fixture's case and are compared with the fixture; the odd agents carry one of three other draws of times, states and inputs and
are compared with the host front on the same draw, within the same gate.  Batches of 1, 3 and 67: one lane per output double,
so the lane index crosses agents and 256-lane blocks at non-multiples of 64 for every shape here.  Shapes: nu = 0 (scalar),
nf != nx (cost), K = 1 (k1), K = 13 (k13), mixed degrees (m36, m46), 13 x 4 with nx = 12, nu = 2 (trig_u13)."""
import numpy as np
import pytest

import meshfn_gates as G
import meshfn_ref as MR
from examples import models_lib as M

pytestmark = pytest.mark.gpu
BATCHES = [1, 3, 67]
_DRAWS = {}


def _dims(c):
    return [int(v) for v in c["f"]["dims"]]


def _draws(name):
    """[fixture draw, three others] of one case (once): dict t0, tf, xs, us, f, J, and for the others the host front's results"""
    if name in _DRAWS:
        return _DRAWS[name]
    c = G.case(name)
    m, fn = c["m"], c["f"]
    nx, nu, nf = _dims(c)
    vehicle = str(c["fn"]) == "vehicle"
    rng = np.random.default_rng(len(name) + 7 * len(G.CASES))
    draws = []
    for v in range(4):
        if v == 0:
            d = {"t0": c["t0"], "tf": c["tf"], "xs": c["xs"], "us": c["us"]}
        else:
            d = {"t0": float(np.round(rng.uniform(-1, 0), 2)), "tf": float(np.round(rng.uniform(1, 2), 2)), "xs": rng.uniform(-1, 1, c["xs"].shape),
                 "us": rng.uniform(-1, 1, c["us"].shape)}
            if vehicle:
                d["xs"][:, :3] = 0.0
        d["f"], d["J"], _ = MR.model(fn["dims"], fn["terms"], fn["coef"], MR.node_times(m["K"], m["tau0"], d["t0"], d["tf"]), d["xs"], d["us"])
        if v > 0 and not vehicle:       # (the harness runs the vehicle on the group, where mesh_dyn does not apply)
            shape = tuple(_dims(c))
            for key, (hf, scale) in {"eval": ("eval", False), "evals": ("eval", True), "integrate": ("integrate", False), "dyn": ("dyn", False)}.items():
                if key == "dyn" and nf != nx:
                    continue
                h = M.meshfn_host(m["spec"], m["ops"], None, hf, 1, shape, fn["terms"], fn["coef"], d["t0"], d["tf"], d["xs"], d["us"], scale=scale)
                d[key + ".F"], d[key + ".dF"] = h["F"], h["val"]
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        draws.append(d)
    _DRAWS[name] = (c, draws)
    return _DRAWS[name]


def _batch(draws, B, vehicle):
    """agent b -> draw: the fixture's for even b, the others in turn for odd b (the vehicle has no other draws to compare)"""
    which = [0 if b % 2 == 0 or vehicle else 1 + (b // 2) % 3 for b in range(B)]
    stack = lambda k: np.stack([np.asarray(draws[w][k]) for w in which])            # noqa: E731
    return which, stack("t0"), stack("tf"), stack("xs"), stack("f"), stack("J")


def _run(sfb, key, mesh, nx, nu, t0, tf, X, F, dF, device):
    """one function through the host-pointer entry or, on torch tensors, the device-pointer entry -> (out_F, out_dF) as numpy"""
    if device:
        import torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None     # noqa: E731
        if key == "dyn":
            out = sfb.mesh_dyn_batch(mesh, nu, dev(t0), dev(tf), dev(X), dev(F), dev(dF))
        elif key == "integrate":
            out = sfb.mesh_integrate_batch(mesh, nx, nu, dev(t0), dev(tf), dev(F), dev(dF))
        else:
            out = sfb.mesh_eval_batch(mesh, nx, nu, dev(t0), dev(tf), dev(F), dev(dF), scale=key == "evals")
        torch.cuda.synchronize()
        return [o.cpu().numpy() if o is not None else None for o in out]
    if key == "dyn":
        return sfb.mesh_dyn_batch_host(mesh, nu, t0, tf, X, F, dF)
    if key == "integrate":
        return sfb.mesh_integrate_batch_host(mesh, nx, nu, t0, tf, F, dF)
    return sfb.mesh_eval_batch_host(mesh, nx, nu, t0, tf, F, dF, scale=key == "evals")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", G.CASES)
def test_kernels_against_the_fixture_and_the_host_front(sfb, name, B):
    c, draws = _draws(name)
    nx, nu, nf = _dims(c)
    mesh = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
    which, t0, tf, X, F, dF = _batch(draws, B, str(c["fn"]) == "vehicle")
    for key in G.FUNCTIONS:
        if key + ".F" not in c:
            continue
        host = _run(sfb, key, mesh, nx, nu, t0, tf, X, F, dF, device=False)
        dev = _run(sfb, key, mesh, nx, nu, t0, tf, X, F, dF, device=True)
        vals = _run(sfb, key, mesh, nx, nu, t0, tf, X, F, None, device=False)
        assert vals[1] is None and np.array_equal(vals[0], host[0])                 # Deriv = 0: the same bits
        assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])  # the two entries run the same kernels
        assert np.all(np.isfinite(host[0])) and np.all(np.isfinite(host[1]))
        for b in sorted({0, 1, 2, B // 2, B - 2, B - 1} & set(range(B))):
            ref = c if which[b] == 0 else draws[which[b]]
            who = "%s B=%d agent %d %s" % (name, B, b, "fixture" if which[b] == 0 else "host front")
            G.check(key + ".F", host[0][b].ravel(), ref[key + ".F"], who)
            G.check(key + ".dF", host[1][b].ravel(), ref[key + ".dF"], who)
        for b in range(B):                                                          # equal draws give equal bits, wherever they sit
            first = which.index(which[b])
            assert np.array_equal(host[0][b], host[0][first]) and np.array_equal(host[1][b], host[1][first]), b


def test_batch_of_zero_writes_nothing(sfb):
    import torch
    c, draws = _draws("poly_m36")
    nx, nu, nf = _dims(c)
    mesh = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
    N = mesh.N
    seven = lambda n: torch.full((n,), 7.0, dtype=torch.float64, device="cuda")      # noqa: E731
    t0, tf, X, F, dF = seven(1), seven(1), seven((N + 1) * nx), seven(N * nf), seven(N * nf * (1 + nx + nu))
    oF, odF = seven(N * nf), seven(N * nf * (2 + 14 + nx + nu))
    p = lambda t: t.data_ptr()                                                       # noqa: E731
    sfb.mesh_eval_batch_device(mesh, 0, nx, nu, nf, True, p(t0), p(tf), p(F), p(dF), p(oF), p(odF))
    sfb.mesh_integrate_batch_device(mesh, 0, nx, nu, nf, p(t0), p(tf), p(F), p(dF), p(oF), p(odF))
    sfb.mesh_dyn_batch_device(mesh, 0, nx, nu, p(t0), p(tf), p(X), p(F), p(dF), p(oF), p(odF))
    torch.cuda.synchronize()
    assert bool((oF == 7.0).all()) and bool((odF == 7.0).all())
    lib, C = sfb._capi.lib, __import__("ctypes")
    hF, hdF = np.full(N * nf, 7.0), np.full(N * nf * (2 + 14 + nx + nu), 7.0)
    q = lambda a: a.ctypes.data                                                      # noqa: E731
    assert lib.sfb_mesh_eval_batch_host(C.byref(mesh.c), 0, nx, nu, nf, 1, q(hF), q(hF), q(hF), q(hdF), q(hF), q(hdF)) == 0
    assert lib.sfb_mesh_integrate_batch_host(C.byref(mesh.c), 0, nx, nu, nf, q(hF), q(hF), q(hF), q(hdF), q(hF), q(hdF)) == 0
    assert lib.sfb_mesh_dyn_batch_host(C.byref(mesh.c), 0, nx, nu, q(hF), q(hF), q(hF), q(hF), q(hdF), q(hF), q(hdF)) == 0
    assert np.all(hF == 7.0) and np.all(hdF == 7.0)


def test_two_meshes_used_alternately_keep_their_own_tables(sfb):
    """... and the same mesh with another (nx, nu) has tables of its own"""
    runs = []
    for name in ("poly_m36", "poly_k13", "cost_m36", "scalar_k13", "trig_m46", "poly_m46"):
        c, draws = _draws(name)
        nx, nu, nf = _dims(c)
        mesh = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
        which, t0, tf, X, F, dF = _batch(draws, 5, False)
        key = "dyn" if nf == nx else "evals"
        runs.append((name, key, lambda key=key, mesh=mesh, nx=nx, nu=nu, a=(t0, tf, X, F, dF): _run(sfb, key, mesh, nx, nu, *a, device=False)))
    first = [r[2]() for r in runs]
    for rounds in range(2):
        for (name, key, call), want in zip(runs, first):
            got = call()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    for (name, key, _), want in zip(runs, first):
        G.check(key + ".dF", want[1][0], G.case(name)[key + ".dF"], name)


def test_more_meshes_than_a_device_keeps_are_dropped_and_rebuilt_with_the_same_tables(sfb):
    """70 distinct two-interval meshes through sfb_mesh_dyn_batch_host (it reads every table: nodes, weights, differentiation
    matrices, the entry -> row table): a device keeps 64 sets of tables, so the cache is emptied on the way whatever it held
    before.  Meshes 0, 1 and 69 called again give the bits of their first run, and mesh 0 stays within the gates against
    the restatement."""
    K, nx, nu, B = np.array([2, 3]), 2, 1, 3
    tau0 = [np.array([0.0, 0.30 + 0.005 * i]) for i in range(70)]
    rng = np.random.default_rng(64)
    t0, tf = rng.uniform(-1, 0, B), rng.uniform(1, 2, B)
    X, F, dF = rng.uniform(-1, 1, (B, 6, nx)), rng.uniform(-1, 1, (B, 5, nx)), rng.uniform(-1, 1, (B, 5, nx, 1 + nx + nu))
    meshes = [sfb.PHMesh(K, t) for t in tau0]
    first = [sfb.mesh_dyn_batch_host(m, nu, t0, tf, X, F, dF) for m in meshes]
    for i in (0, 1, 69):
        again = sfb.mesh_dyn_batch_host(meshes[i], nu, t0, tf, X, F, dF)
        assert np.array_equal(again[0], first[i][0]) and np.array_equal(again[1], first[i][1]), i
    assert len({f[0].tobytes() + f[1].tobytes() for f in first}) == 70              # every mesh had tables of its own
    for b in range(B):
        want = MR.functions(K, tau0[0], (nx, nu, nx), t0[b], tf[b], X[b], F[b], dF[b], order=1)
        G.check("dyn.F", first[0][0][b], want["dyn.F"], "mesh 0 of 70, agent %d" % b)
        G.check("dyn.dF", first[0][1][b], want["dyn.dF"], "mesh 0 of 70, agent %d" % b)


def _se2_exp(a, b, th):
    s, c = np.sin(th), np.cos(th)
    A, Bc = (s / th, (1 - c) / th) if abs(th) > 1e-9 else (1.0, 0.0)
    return A * a - Bc * b, Bc * a + A * b, c, s


def _xdes_flat(t):
    """VehicleModel6::xdes(t) in the harness's flat storage (x, y, cos, sin, v)"""
    x, y, c, s = _se2_exp(t * 1.0, 0.0, t * 0.4)
    return np.array([2.5 - y, x, -s, c, 1.0, 0.0, 0.4])                              # SE2(pi / 2, 2.5, 0) * exp


def test_defects_of_a_swarm_tick_end_to_end(sfb):
    """the primal of one MPCSwarmDeviceLin tick on 8 vehicles (as the swarm's solution accessor hands it on), lifted on the
    host to the deviations e_i, v_i from the desired trajectory; the model is the flattened vehicle dynamics around it,
    evaluated by the harness, its Jacobian by differences; then sfb_mesh_dyn_batch: finite, and equal to the host front on the
    same numbers within the gate"""
    B, K, tf, nx, nu = 8, 8, 2.0, 6, 2
    t = 0.025 * np.arange(B)
    dx0 = np.zeros((B, nx))
    dx0[1::2, :3] = [0.3, -0.2, 0.25]
    got = M.mpc_swarm_devlin_audit(6, K, tf, t, dx0, audit=True)
    assert np.isin(got["code"], [0, 4, 5]).all(), got["code"]
    mesh = sfb.PHMesh.uniform(2, 4)
    N = mesh.N
    E = got["primal"][:, :nx * (N + 1)].reshape(B, N + 1, nx)
    V = got["primal"][:, nx * (N + 1):].reshape(B, N, nu)
    tau = MR.geometry(mesh.K, mesh.tau0)[0]
    dxl = np.array([1.0, 0.0, 0.4, 0.0, 0.0, 0.0])

    def flat(b, e, v):   # rows: the nodes of agent b
        xl = np.stack([_xdes_flat(t[b] + tf * ta) for ta in tau])
        return M.flat_dynamics_host(0, xl, np.tile(dxl, (N, 1)), np.zeros((N, nu)), e, v)

    F, dF, h = np.zeros((B, N, nx)), np.zeros((B, N, nx, 1 + nx + nu)), 1e-7
    for b in range(B):
        F[b] = flat(b, E[b, :N], V[b])
        for k in range(nx + nu):
            e, v = E[b, :N].copy(), V[b].copy()
            (e if k < nx else v)[:, k if k < nx else k - nx] += h
            dF[b, :, :, 1 + k] = (flat(b, e, v) - F[b]) / h
    out_F, out_dF = sfb.mesh_dyn_batch_host(mesh, nu, t, t + tf, E, F, dF)
    assert np.all(np.isfinite(out_F)) and np.all(np.isfinite(out_dF))
    worst = 0.0
    for b in range(B):
        table = np.concatenate([F[b].reshape(N, nx), dF[b].reshape(N, -1)], axis=1)
        host = M.meshfn_host((4, 4, 2, 4), [], None, "dyn", 1, "table", np.zeros((0, 5)), table, t[b], t[b] + tf, E[b], V[b])
        worst = max(worst, G.check("dyn.F", out_F[b], host["F"], "agent %d against the host front" % b))
        G.check("dyn.dF", out_dF[b], host["val"], "agent %d against the host front" % b)
    print("defects: largest %.3e; kernel against host front %.2e" % (np.abs(out_F).max(), worst))
