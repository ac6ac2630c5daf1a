"""The Lagrangian-Hessian kernel of the collocation NLP (ocp_nlp_hess_kernel of smooth_feedback_amd/csrc/mesh.hip through
sfb_ocp_nlp_hess_batch*) against sigma d2f + d2g of the 60-digit fixture tests/golden/ocpnlp_reference.npz, within the `d2l` gate
of tests/ocpnlp_hess_gates.py (four times the float64 numpy restatement's own error).  The kernel is model-free: the Jacobians
and the model Hessians at the nodes come from tests/ocpnlp_ref.py in float64, contracted with lambda in numpy.  Cases and batch
scheme of tests/test_ocpnlp_gpu.py: in a batch the even agents carry the fixture's x and lambda (sigma cycling through the gate's
four values) and are compared with the fixture; the odd agents carry one of three other seeded draws, each with its own tf,
lambda and sigma, and are compared with the host front (OCPNLP::d2l_dx2 through the harness).  Batches of 1, 3 and 67: a lane walks
four agents with one decoded record, so 67 leaves a last group of three.  bare (n = 3, nnzH = 6: every optional segment empty,
x_0 and x_N adjacent), k13 (nnzH = 547 over three blocks, no multiple of a wave), cross (the transposed q blocks)."""
import ctypes as C

import numpy as np
import pytest

import ocpnlp_gates as G
import ocpnlp_hess_gates as HG
import ocpnlp_ref as NR
import test_ocpnlp_gpu as FIRST
from examples import models_lib as M

pytestmark = pytest.mark.gpu
BATCHES = [1, 3, 67]
NAMES = ("x", "lam", "sigma", "dFf", "HLf", "dFg", "HLg", "dFcr", "HLcr", "d2theta", "d2ce_l")
_DRAWS = {}


def _draws(name):
    """{(draw, sigma): arrays and the reference} of one case (once): draw 0 is the fixture's x and lambda at each of the gate's sigmas,
    draws 1 .. 3 are seeded, each with its own tf, lambda and sigma, and have the host front as reference"""
    if name in _DRAWS:
        return _DRAWS[name]
    c = G.case(name)
    rng = np.random.default_rng(len(name) + 13 * len(G.CASES))
    draws = {}
    fix = HG.contracted(c, c["x"], c["lambda"])
    for s in HG.SIGMAS:
        draws[(0, s)] = dict(fix, x=c["x"], lam=c["lambda"], sigma=np.float64(s), ref=HG.reference(c, s))
    for v in (1, 2, 3):
        x = rng.uniform(-1, 1, len(c["x"]))
        x[0] = float(np.round(rng.uniform(0.5, 3.0), 2))
        lam = rng.uniform(-1, 1, len(c["lambda"]))
        s = float(np.round(rng.uniform(-2, 2), 2))
        h = M.ocp_nlp_hess_host(c["m"]["spec"], c["m"]["ops"], c["dims"], c, (c["crl"], c["cru"], c["cel"], c["ceu"]), x, lam, s)
        assert np.array_equal(h["hrowind"], c["h.rowind"])
        draws[(v, s)] = dict(HG.contracted(c, x, lam), x=x, lam=lam, sigma=np.float64(s), ref=h["d2l"])
    for d in draws.values():
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    _DRAWS[name] = (c, draws)
    return _DRAWS[name]


def _batch(draws, B):
    odd = [k for k in draws if k[0] > 0]
    which = [(0, HG.SIGMAS[(b // 2) % 4]) if b % 2 == 0 else odd[(b // 2) % 3] for b in range(B)]
    return which, {k: np.stack([np.asarray(draws[w][k]) for w in which]) for k in NAMES}


def _run(sfb, mesh, dims, a, device=False):
    args = [a[k] for k in NAMES]
    if device:
        import torch
        dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()            # noqa: E731
        out = sfb.ocp_nlp_hess_batch(mesh, dims, *[dev(v) for v in args])
        torch.cuda.synchronize()
        return out.cpu().numpy()
    return sfb.ocp_nlp_hess_batch_host(mesh, dims, *args)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", G.CASES)
def test_kernel_against_the_fixture_and_the_host_front(sfb, name, B):
    c, draws = _draws(name)
    mesh = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
    which, a = _batch(draws, B)
    host = _run(sfb, mesh, c["dims"], a)
    dev = _run(sfb, mesh, c["dims"], a, device=True)
    assert np.array_equal(dev, host)                                                # the two entries run the same kernel
    assert np.all(np.isfinite(host)) and host.shape == (B, len(c["h.rowind"]))
    for b in range(B):
        who = "%s B=%d agent %d %s" % (name, B, b, "fixture" if which[b][0] == 0 else "host front")
        HG.check(host[b], draws[which[b]]["ref"], who)
        assert np.array_equal(host[b], host[which.index(which[b])]), b              # equal draws give equal bits, wherever they sit
    if name == "cross":                                                             # the transposed q blocks hold something
        vb = c["var_beg"]
        sel = (c["h.rowind"] == vb[1]) & (np.repeat(np.arange(vb[4]), np.diff(c["h.colptr"])) >= vb[2])
        assert sel.sum() == 4 and np.count_nonzero(host[0][sel]) >= 2


def test_batch_of_zero_writes_nothing(sfb):
    import torch
    c, _ = _draws("mixed")
    mesh = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
    big = len(c["h.rowind"]) + 64
    seven = lambda: torch.full((big,), 7.0, dtype=torch.float64, device="cuda")     # noqa: E731
    ins, hess = [seven() for _ in range(11)], seven()
    sfb.ocp_nlp_hess_batch_device(mesh, c["dims"], 0, *[t.data_ptr() for t in ins], hess.data_ptr())
    torch.cuda.synchronize()
    assert bool((hess == 7.0).all())
    h = np.full(big, 7.0)
    d = sfb._capi.SfbOcpDims(*c["dims"])
    p = h.ctypes.data
    assert sfb._capi.lib.sfb_ocp_nlp_hess_batch_host(C.byref(mesh.c), C.byref(d), 0, *([p] * 12)) == 0
    assert np.all(h == 7.0)


def test_two_meshes_and_dims_used_alternately_with_first_order_calls_keep_their_own_tables(sfb):
    """the Hessian's records live in the cache entry of the first-order tables and are built on first use: calls of both kinds on
    several (mesh, dims) pairs, alternating, give the same bits every round (ref and cross share mesh and dims: one entry)"""
    runs = []
    for name in ("ref", "k13", "mixed", "bare", "cross"):
        c, draws = _draws(name)
        mesh = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
        _, a = _batch(draws, 5)
        _, a1 = FIRST._batch(FIRST._draws(name)[1], 5)
        if name in ("ref", "bare"):                                                 # first order first here, the Hessian first elsewhere
            runs.append((name + " first order", lambda mesh=mesh, dims=c["dims"], a1=a1: FIRST._run(sfb, mesh, dims, a1)[1]))
        runs.append((name, lambda mesh=mesh, dims=c["dims"], a=a: _run(sfb, mesh, dims, a)))
        if name not in ("ref", "bare"):
            runs.append((name + " first order", lambda mesh=mesh, dims=c["dims"], a1=a1: FIRST._run(sfb, mesh, dims, a1)[1]))
    c, _ = _draws("mixed")                                                          # the m36 mesh with the dims of k13
    k13 = G.case("k13")
    N = int(np.sum(c["m"]["K"]))
    vb, cb = NR.structure(N, k13["dims"])
    rng = np.random.default_rng(3)
    x, lam = rng.uniform(0.5, 1.5, int(vb[4])), rng.uniform(-1, 1, int(cb[4]))
    mixed13 = dict(k13, m=c["m"])
    one = dict(HG.contracted(mixed13, x, lam), x=x, lam=lam, sigma=np.float64(0.5))
    other = {k: np.stack([np.asarray(one[k])] * 2) for k in NAMES}
    mesh36 = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
    runs.append(("m36 with the dims of k13", lambda: _run(sfb, mesh36, k13["dims"], other)))
    first = [r[1]() for r in runs]
    for rounds in range(2):
        for (name, call), want in zip(runs, first):
            assert np.array_equal(call(), want), name
    for (name, _), want in zip(runs, first):
        if name in G.CASES:
            HG.check(want[0], HG.reference(G.case(name), 1.0), name)                 # agent 0: the fixture at sigma 1
        elif name.endswith("first order"):
            G.check("dg", want[0], G.case(name.split()[0])["dg"], name)
    ref = NR.nlp(c["m"]["K"], c["m"]["tau0"], k13["dims"], k13, x, lam, order=2)
    HG.check(first[-1][0], 0.5 * ref["d2f"] + ref["d2g"], "m36 with the dims of k13 against the restatement")
