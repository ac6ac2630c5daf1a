"""The batched ph-mesh kernels (smooth_feedback_amd/csrc/mesh.hip through sfb_mesh_resample_batch* and
sfb_mesh_dyn_error_batch*) against the 60-digit fixture tests/golden/mesh_reference.npz, within the gates of
tests/mesh_gates.py (four times the float64 numpy restatement's own error per case class).  Batches of 1, 63, 65 and 130
(less than a wave of (agent, interval) pairs, a partly filled last block, several blocks) are the fixture's rows repeated;
every mesh of the fixture is covered by the resampling, and the estimate runs on uniform and mixed degrees, 1 to 27 intervals,
K from 3 to 13 (K + 1 = 14 raised points: the kernels' limit, the last rows of their LDS tiles and tables)."""
import ctypes as C

import numpy as np
import pytest

import mesh_gates as G
import mesh_ref as R

pytestmark = pytest.mark.gpu
BATCHES = [1, 63, 65, 130]
_SAMPLES = {}


def _tile(a, B):
    return np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))


def _samples(name):
    """what the restatement computes for one dyn-error case (once): X, U, F at the raised points"""
    if name not in _SAMPLES:
        d = G.dyn(name)
        K, tau0 = d["base"]["K"], d["base"]["tau0"]
        X, U = R.resample(K, tau0, d["vals_x"], True), R.resample(K, tau0, d["vals_u"], False)
        t = float(d["t0"]) + (float(d["tf"]) - float(d["t0"])) * R.raised_nodes(K, tau0)
        F = R.dynamics(int(d["fid"]), d["coef"], int(d["nu"]), t, X, U)
        for a in (X, U, F):
            a.setflags(write=False)
        _SAMPLES[name] = (d, X, U, F)
    return _SAMPLES[name]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", G.MESHES)
def test_resample_against_the_fixture(sfb, name, B):
    m, r = G.mesh(name), G.section("resample." + name)
    mesh = sfb.PHMesh(m["K"], m["tau0"])
    ext = sfb.mesh_resample_batch_host(mesh, _tile(r["vals"], B), True)
    opn = sfb.mesh_resample_batch_host(mesh, _tile(r["vals"][:-1], B), False)
    assert ext.shape == opn.shape == (B, mesh.R, 3)
    for b in sorted({0, B // 2, B - 1}):
        G.check("resample", ext[b], r["out_ext"], "%s B=%d agent %d, extended" % (name, B, b))
        G.check("resample", opn[b], r["out_open"], "%s B=%d agent %d, open" % (name, B, b))
    assert np.array_equal(ext, _tile(ext[0], B)) and np.array_equal(opn, _tile(opn[0], B))
    # only the last interval sees the difference
    last = mesh.R - (int(m["K"][-1]) + 2)
    assert np.array_equal(ext[:, :last], opn[:, :last])


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", G.DYN)
def test_dyn_error_against_the_fixture(sfb, name, B):
    d, X, U, F = _samples(name)
    mesh = sfb.PHMesh(d["base"]["K"], d["base"]["tau0"])
    gx = sfb.mesh_resample_batch_host(mesh, _tile(d["vals_x"], B), True)
    G.check("resample", gx[B - 1], d["X"], "%s B=%d X" % (name, B))
    if int(d["nu"]):
        gu = sfb.mesh_resample_batch_host(mesh, _tile(d["vals_u"], B), False)
        G.check("resample", gu[B - 1], d["U"], "%s B=%d U" % (name, B))
    errs = sfb.mesh_dyn_error_batch_host(mesh, float(d["tf"]) - float(d["t0"]), _tile(X, B), _tile(F, B))
    assert errs.shape == (B, mesh.nivals)
    for b in sorted({0, B // 2, B - 1}):
        G.check("dynerr." + d["cls_name"], errs[b], d["errs"], "%s B=%d agent %d" % (name, B, b))
    assert np.array_equal(errs, _tile(errs[0], B))


def test_agents_are_independent_and_a_nan_stays_in_its_own_interval(sfb):
    d, X, U, F = _samples("co_three5")                       # nx = 12, three intervals of 5
    mesh, B = sfb.PHMesh(d["base"]["K"], d["base"]["tau0"]), 65
    scale = 1.0 + np.arange(B) % 7
    Xb, Fb = _tile(X, B) * scale[:, None, None], _tile(F, B) * scale[:, None, None]
    h = np.full(B, float(d["tf"]) - float(d["t0"]))
    errs = sfb.mesh_dyn_error_batch_host(mesh, h, Xb, Fb)
    for b in (0, 1, 6, 64):                                  # each agent alone gives the same bits
        assert np.array_equal(sfb.mesh_dyn_error_batch_host(mesh, h[b:b + 1], Xb[b:b + 1], Fb[b:b + 1])[0], errs[b])
    assert len({tuple(e) for e in errs}) == 7
    Fb = Fb.copy()
    Fb[33, 7 + 2, 5] = np.nan                                # agent 33, second interval (rows 7 .. 13), third point
    bad = sfb.mesh_dyn_error_batch_host(mesh, h, Xb, Fb)
    assert np.isnan(bad[33, 1]) and np.array_equal(np.delete(bad.ravel(), 33 * 3 + 1), np.delete(errs.ravel(), 33 * 3 + 1))
    # F at an interval's end point is never read
    Fb = _tile(F, B) * scale[:, None, None]
    Fb[:, [6, 13, 20]] = np.nan
    assert np.array_equal(sfb.mesh_dyn_error_batch_host(mesh, h, Xb, Fb), errs)
    # the horizon is per agent
    h2 = h * (1.0 + (np.arange(B) == 5))
    other = sfb.mesh_dyn_error_batch_host(mesh, h2, Xb, Fb)
    assert not np.array_equal(other[5], errs[5]) and np.array_equal(np.delete(other, 5, axis=0), np.delete(errs, 5, axis=0))


def test_zero_widths_and_empty_batches(sfb):
    m = G.mesh("mixed")
    mesh = sfb.PHMesh(m["K"], m["tau0"])
    lib, p = sfb._capi.lib, lambda a: a.ctypes.data                               # noqa: E731
    out = np.full(8, 7.0)
    assert lib.sfb_mesh_resample_batch_host(C.byref(mesh.c), 5, 0, 1, None, p(out)) == sfb._capi.SFB_OK and np.all(out == 7.0)
    assert lib.sfb_mesh_resample_batch_host(C.byref(mesh.c), 0, 3, 1, p(out), p(out)) == sfb._capi.SFB_OK and np.all(out == 7.0)
    assert sfb.mesh_resample_batch_host(mesh, np.zeros((4, mesh.N, 0)), False).shape == (4, mesh.R, 0)
    # no state coordinates: nothing to be wrong about
    errs = sfb.mesh_dyn_error_batch_host(mesh, 1.0, np.zeros((4, mesh.R, 0)), np.zeros((4, mesh.R, 0)))
    assert errs.shape == (4, 3) and not errs.any()
    errs = np.full(3, 7.0)
    assert lib.sfb_mesh_dyn_error_batch_host(C.byref(mesh.c), 0, 2, p(out), p(out), p(out), p(errs)) == sfb._capi.SFB_OK and np.all(errs == 7.0)


def test_more_meshes_than_a_device_keeps_are_dropped_and_rebuilt_with_the_same_lists(sfb):
    """70 distinct two-interval meshes through sfb_mesh_dyn_error_batch_host (the entry that reads the interval widths): a
    device keeps 64 interval lists, so the cache is emptied on the way whatever it held before.  Meshes 0, 1 and 69 called
    again give the bits of their first run, and mesh 0 stays within the gate against the restatement (random X, F: the
    errors are of order one, the fixture's "coarse" class)."""
    K = np.array([2, 3])
    tau0 = [np.array([0.0, 0.30 + 0.005 * i]) for i in range(70)]
    rng = np.random.default_rng(64)
    h, X, F = rng.uniform(0.5, 1.5, 3), rng.uniform(-1, 1, (3, 9, 2)), rng.uniform(-1, 1, (3, 9, 2))
    meshes = [sfb.PHMesh(K, t) for t in tau0]
    first = [sfb.mesh_dyn_error_batch_host(m, h, X, F) for m in meshes]
    for i in (0, 1, 69):
        assert np.array_equal(sfb.mesh_dyn_error_batch_host(meshes[i], h, X, F), first[i]), i
    assert len({e.tobytes() for e in first}) == 70                                 # every mesh had a list of its own
    for b in range(3):
        want = R.dyn_error(K, tau0[0], h[b], X[b], F[b])
        assert want.min() > G.CLASS_BOUNDS["coarse"][0]
        G.check("dynerr.coarse", first[0][b], want, "mesh 0 of 70, agent %d" % b)


@pytest.mark.parametrize("name", ["co_three5", "re_u13x12", "ex_mixed"])
def test_device_pointer_entries_equal_the_host_entries_bit_for_bit(sfb, name):
    import torch
    d, X, U, F = _samples(name)
    mesh, B = sfb.PHMesh(d["base"]["K"], d["base"]["tau0"]), 65
    nx = int(d["nx"])
    vals, Xb, Fb = _tile(d["vals_x"], B), _tile(X, B), _tile(F, B)
    h = np.linspace(0.5, 1.5, B)
    want_x, want_e = sfb.mesh_resample_batch_host(mesh, vals, True), sfb.mesh_dyn_error_batch_host(mesh, h, Xb, Fb)
    dev = lambda a: torch.from_numpy(a).cuda()                                     # noqa: E731
    dv, dX, dF, dh = dev(vals), dev(Xb), dev(Fb), dev(h)
    dout = torch.full((B, mesh.R, nx), 7.0, dtype=torch.float64, device="cuda")
    derr = torch.full((B, mesh.nivals), 7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    sfb.mesh_resample_batch_device(mesh, B, nx, True, dv.data_ptr(), dout.data_ptr(), stream)
    sfb.mesh_dyn_error_batch_device(mesh, B, nx, dh.data_ptr(), dX.data_ptr(), dF.data_ptr(), derr.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), want_x) and np.array_equal(derr.cpu().numpy(), want_e)
    # resample -> dyn_error chained on the device, without a copy in between, on the kernel's own X
    sfb.mesh_dyn_error_batch_device(mesh, B, nx, dh.data_ptr(), dout.data_ptr(), dF.data_ptr(), derr.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(derr.cpu().numpy(), sfb.mesh_dyn_error_batch_host(mesh, h, want_x, Fb))
