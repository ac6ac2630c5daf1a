"""The fused collocation-NLP kernel (smooth_feedback_amd/csrc/mesh.hip through sfb_ocp_nlp_batch*) against the 60-digit fixture
tests/golden/ocpnlp_reference.npz, within the gates of tests/ocpnlp_gates.py (four times the float64 numpy restatement's own
error per class).  The kernel is model-free: the values and Jacobians of f, g, cr at the nodes and of ce come from
tests/ocpnlp_ref.py in float64.  In a batch the even agents carry the fixture's x and are compared with the fixture; the odd
agents carry one of three other seeded draws, each with its own tf, and are compared with the host front (detail::OCPNLP through
the harness) on the same draw, within the same gates.  Batches of 1, 3 and 67: a lane walks eight agents with one decoded item,
so 67 leaves a last group of three, and the m + nnz items of every case are no multiple of a wave or a block (bare: 1 + 3 items,
every segment but one empty; k13: 159 + 2098 items over nine blocks)."""
import ctypes as C

import numpy as np
import pytest

import ocpnlp_gates as G
import ocpnlp_ref as NR
from examples import models_lib as M

pytestmark = pytest.mark.gpu
BATCHES = [1, 3, 67]
NAMES = ("Ff", "dFf", "Fg", "dFg", "Fcr", "dFcr", "ce", "dce")
_DRAWS = {}


def _inputs(c, x):
    """one agent's model arrays in the order of the entry's arguments"""
    mv = NR.models(c["m"]["K"], c["m"]["tau0"], c["dims"], c, x)
    return {"Ff": mv["f"][0], "dFf": mv["f"][1], "Fg": mv["g"][0], "dFg": mv["g"][1], "Fcr": mv["cr"][0], "dFcr": mv["cr"][1],
            "ce": mv["ce"][0], "dce": mv["ce"][1]}


def _draws(name):
    """[fixture draw, three others] of one case (once): x, the model arrays, and the reference g / dg (fixture or host front)"""
    if name in _DRAWS:
        return _DRAWS[name]
    c = G.case(name)
    rng = np.random.default_rng(len(name) + 11 * len(G.CASES))
    draws = []
    for v in range(4):
        if v == 0:
            d = {"x": c["x"], "g": c["g"], "dg": c["dg"]}
        else:
            x = rng.uniform(-1, 1, len(c["x"]))
            x[0] = float(np.round(rng.uniform(0.5, 3.0), 2))
            h = M.ocp_nlp_host(c["m"]["spec"], c["m"]["ops"], c["dims"], c, (c["crl"], c["cru"], c["cel"], c["ceu"]), x, order=1)
            assert np.array_equal(h["colind"], c["dg.colind"])
            d = {"x": x, "g": h["g"], "dg": h["dg"]}
        d.update(_inputs(c, d["x"]))
        for a in d.values():
            a.setflags(write=False)
        draws.append(d)
    _DRAWS[name] = (c, draws)
    return _DRAWS[name]


def _batch(draws, B):
    which = [0 if b % 2 == 0 else 1 + (b // 2) % 3 for b in range(B)]
    return which, {k: np.stack([draws[w][k] for w in which]) for k in ("x",) + NAMES}


def _run(sfb, mesh, dims, a, deriv=True, device=False):
    args = [a[k] if (deriv or not k.startswith("d")) else None for k in NAMES]
    if device:
        import torch
        dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda() if v is not None else None     # noqa: E731
        out = sfb.ocp_nlp_batch(mesh, dims, dev(a["x"]), *[dev(v) for v in args])
        torch.cuda.synchronize()
        return [o.cpu().numpy() if o is not None else None for o in out]
    return sfb.ocp_nlp_batch_host(mesh, dims, a["x"], *args)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", G.CASES)
def test_kernel_against_the_fixture_and_the_host_front(sfb, name, B):
    c, draws = _draws(name)
    mesh = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
    which, a = _batch(draws, B)
    host = _run(sfb, mesh, c["dims"], a)
    dev = _run(sfb, mesh, c["dims"], a, device=True)
    vals = _run(sfb, mesh, c["dims"], a, deriv=False)
    assert vals[1] is None and np.array_equal(vals[0], host[0])                     # values only: the same bits of g
    assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])      # the two entries run the same kernel
    assert np.all(np.isfinite(host[0])) and np.all(np.isfinite(host[1]))
    assert host[0].shape == (B, len(c["g"])) and host[1].shape == (B, len(c["dg"]))
    for b in range(B):
        ref = draws[which[b]]
        who = "%s B=%d agent %d %s" % (name, B, b, "fixture" if which[b] == 0 else "host front")
        G.check("g", host[0][b], ref["g"], who)
        G.check("dg", host[1][b], ref["dg"], who)
        first = which.index(which[b])                                               # equal draws give equal bits, wherever they sit
        assert np.array_equal(host[0][b], host[0][first]) and np.array_equal(host[1][b], host[1][first]), b


@pytest.mark.parametrize("name", G.CASES)
def test_fused_output_against_the_composition_of_the_three_mesh_functions(sfb, name):
    """what a caller composed before: sfb_mesh_dyn_batch, the weight-scaled sfb_mesh_eval_batch and sfb_mesh_integrate_batch on
    [t0 | tf | X | U] with t0 = 0, then in numpy the t0 column dropped, the variables re-ordered, the product with ws, -ws at the
    integral rows' q entry and the end rows"""
    c, draws = _draws(name)
    nx, nu, nq, ncr, nce = c["dims"]
    K, tau0 = c["m"]["K"], c["m"]["tau0"]
    mesh = sfb.PHMesh(K, tau0)
    N, B = mesh.N, 5
    which, a = _batch(draws, B)
    g, dg = _run(sfb, mesh, c["dims"], a)
    vb, cb = NR.structure(N, c["dims"])
    ws = NR.w_scaling(K, tau0)
    old = 2 + nx * (N + 1) + nu * N
    to_new = np.concatenate([[0], vb[2] + np.arange(nx * (N + 1)), vb[3] + np.arange(nu * N)])
    t0, tf = np.zeros(B), a["x"][:, 0].copy()
    X = a["x"][:, vb[2]:vb[3]].reshape(B, N + 1, nx)
    A, want = np.zeros((B, cb[4], vb[4])), np.zeros((B, cb[4]))
    F, dF = sfb.mesh_dyn_batch_host(mesh, nu, t0, tf, X, a["Ff"], a["dFf"])
    pat = sfb.mesh_dyn_pattern(mesh, nx, nu)
    dense = np.zeros((B, N * nx, old))
    dense[:, np.repeat(np.arange(N * nx), np.diff(pat[0])), pat[1]] = dF
    want[:, :cb[1]], A[:, :cb[1], to_new] = ws * F, ws * dense[:, :, 1:]
    if nq:
        F, dF = sfb.mesh_integrate_batch_host(mesh, nx, nu, t0, tf, a["Fg"], a["dFg"])
        want[:, cb[1]:cb[2]] = ws * (F - a["x"][:, vb[1]:vb[2]])
        A[:, cb[1]:cb[2], to_new] = ws * dF[:, :, 1:]
        A[:, np.arange(cb[1], cb[2]), vb[1] + np.arange(nq)] = -ws
    if ncr:
        F, dF = sfb.mesh_eval_batch_host(mesh, nx, nu, t0, tf, a["Fcr"], a["dFcr"], scale=True)
        pat = sfb.mesh_eval_pattern(mesh, nx, nu, ncr)
        dense = np.zeros((B, N * ncr, old))
        dense[:, np.repeat(np.arange(N * ncr), np.diff(pat[0])), pat[1]] = dF
        want[:, cb[2]:cb[3]], A[:, cb[2]:cb[3], to_new] = ws * F, ws * dense[:, :, 1:]
    if nce:
        end_new = np.concatenate([[0], vb[2] + np.arange(nx), vb[2] + N * nx + np.arange(nx), vb[1] + np.arange(nq)])
        want[:, cb[3]:] = a["ce"]
        A[:, cb[3]:, end_new] = a["dce"]
    rows = np.repeat(np.arange(cb[4]), np.diff(c["dg.rowptr"]))
    for b in range(B):
        G.check("g", g[b], want[b], "%s agent %d against the composition" % (name, b))
        G.check("dg", dg[b], A[b, rows, c["dg.colind"]], "%s agent %d against the composition" % (name, b))


def test_batch_of_zero_writes_nothing(sfb):
    import torch
    c, _ = _draws("mixed")
    mesh = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
    big = len(c["dg"]) + 64
    seven = lambda: torch.full((big,), 7.0, dtype=torch.float64, device="cuda")     # noqa: E731
    ins, g, dg = [seven() for _ in range(9)], seven(), seven()
    sfb.ocp_nlp_batch_device(mesh, c["dims"], 0, *[t.data_ptr() for t in ins], g.data_ptr(), dg.data_ptr())
    torch.cuda.synchronize()
    assert bool((g == 7.0).all()) and bool((dg == 7.0).all())
    h = np.full(big, 7.0)
    d = sfb._capi.SfbOcpDims(*c["dims"])
    p = h.ctypes.data
    assert sfb._capi.lib.sfb_ocp_nlp_batch_host(C.byref(mesh.c), C.byref(d), 0, *([p] * 11)) == 0
    assert np.all(h == 7.0)


def test_more_meshes_than_a_device_keeps_are_dropped_and_rebuilt_with_the_same_tables(sfb):
    """70 distinct two-interval meshes with the dims of "bare" through sfb_ocp_nlp_batch_host, values and Jacobian: a device keeps
    64 sets of decode tables, so the cache is emptied on the way whatever it held before.  Meshes 0, 1 and 69 called again give
    the bits of their first run, and mesh 0 stays within the gates against the restatement."""
    c = G.case("bare")
    K, dims, B = np.array([2, 3]), c["dims"], 3
    tau0 = [np.array([0.0, 0.30 + 0.005 * i]) for i in range(70)]
    x = np.random.default_rng(64).uniform(-1, 1, (B, int(NR.structure(5, dims)[0][4])))
    x[:, 0] = [0.75, 1.5, 2.25]
    runs = []
    for t in tau0:
        per = [_inputs({**c, "m": {"K": K, "tau0": t}}, xb) for xb in x]
        a = {k: np.stack([p[k] for p in per]) for k in NAMES}
        a["x"] = x
        runs.append((sfb.PHMesh(K, t), a))
    first = [_run(sfb, mesh, dims, a) for mesh, a in runs]
    for i in (0, 1, 69):
        again = _run(sfb, runs[i][0], dims, runs[i][1])
        assert np.array_equal(again[0], first[i][0]) and np.array_equal(again[1], first[i][1]), i
    assert len({f[0].tobytes() + f[1].tobytes() for f in first}) == 70              # every mesh had tables of its own
    for b in range(B):
        want = NR.nlp(K, tau0[0], dims, c, x[b], order=1)
        G.check("g", first[0][0][b], want["g"], "mesh 0 of 70, agent %d" % b)
        G.check("dg", first[0][1][b], want["dg"], "mesh 0 of 70, agent %d" % b)


def test_two_meshes_and_dims_used_alternately_keep_their_own_decode_tables(sfb):
    """... and the same mesh with other dims has tables of its own (ref and cross share mesh and dims: one table)"""
    runs = []
    for name in ("ref", "k13", "mixed", "bare", "cross"):
        c, draws = _draws(name)
        mesh = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
        _, a = _batch(draws, 5)
        runs.append((name, lambda mesh=mesh, dims=c["dims"], a=a: _run(sfb, mesh, dims, a)))
    c, draws = _draws("mixed")                                                      # the m36 mesh with the dims of k13
    k13 = G.case("k13")
    N = int(np.sum(c["m"]["K"]))
    n13 = int(NR.structure(N, k13["dims"])[0][4])
    x = np.random.default_rng(3).uniform(0.5, 1.5, (2, n13))
    mv = NR.models(c["m"]["K"], c["m"]["tau0"], k13["dims"], k13, x[0])
    one = {"Ff": mv["f"][0], "dFf": mv["f"][1], "Fg": mv["g"][0], "dFg": mv["g"][1], "Fcr": mv["cr"][0], "dFcr": mv["cr"][1], "ce": mv["ce"][0],
           "dce": mv["ce"][1]}
    x[1] = x[0]
    other = {k: np.stack([one[k]] * 2) for k in NAMES}
    other["x"] = x
    mesh36 = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
    runs.append(("m36 with the dims of k13", lambda: _run(sfb, mesh36, k13["dims"], other)))
    first = [r[1]() for r in runs]
    for rounds in range(2):
        for (name, call), want in zip(runs, first):
            got = call()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    for (name, _), want in zip(runs[:5], first):
        G.check("dg", want[1][0], G.case(name)["dg"], name)
    ref = NR.nlp(c["m"]["K"], c["m"]["tau0"], k13["dims"], k13, x[0], order=1)
    G.check("dg", first[5][1][0], ref["dg"], "m36 with the dims of k13 against the restatement")
