"""mpc_assemble_kernel over the layout zoo (tests/mpc_layout_zoo.py), in both of its forms, against the dense reference
tests/mpc_assembly_ref.py:

  * the DIRECT form (sfb_mpc_assemble_batch): every layout x packing, full / shared-Jacobian / packed-layout-with-shared
    records, batches 1, 3, 4, 5, 9, finite and non-finite special values, outputs pre-filled with NaN and a sentinel tail
    behind Ax, l, u; and the seam of its launch loop at 65 535 grid rows;
  * the TABLE form (every swarm tick): the same layouts, packings and batches through one tick of an MPCSwarm, read back
    with sfb_mpc_swarm_debug_buffers and compared with the reference AND with the direct form; with shared Jacobians;
    after sfb_mpc_swarm_set_jac_keep to another packing and back; the seam at 4 * 65 535 agents;
  * the FLAT table of re-linearisation passes (sfb_mpc_swarm_step_resident_flat): commutative, unpacked assembly whatever
    the layout and the swarm's packing.

Equality is on the uint64 view of the doubles, NaN matched to NaN: every entry of every agent, no tolerance.  Needs an
MI355X."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_assembly_ref as AR  # noqa: E402
import mpc_layout_zoo as Z  # noqa: E402
from stream_contract import hip_runtime  # noqa: E402

pytestmark = pytest.mark.gpu

TAIL = 32                                                     # sentinel doubles behind every output
SENTINEL = 0x7FF8C0DEC0DEC0DE                                 # a NaN with a payload of its own
PREFILL = 0x7FF800000000BEEF                                  # another: what the kernel must overwrite
TICK = dict(max_iter=3, polish=False)


# ---------------------------------------------------------------------------------------------------- device plumbing
def _hip():
    import torch
    torch.cuda.init()
    lib = hip_runtime()
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return lib


def _d2h(ptr, shape):
    out = np.empty(shape)
    rc = _hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2)
    assert rc == 0, "hipMemcpy D2H: %d" % rc
    return out


def _h2d(ptr, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    rc = _hip().hipMemcpy(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, 1)
    assert rc == 0, "hipMemcpy H2D: %d" % rc


def _direct(Ls, rec, shared=None):
    """sfb_mpc_assemble_batch on device copies of the records; the outputs start as NaN and end in a sentinel tail"""
    import torch
    rec = np.ascontiguousarray(rec)
    B = rec.shape[0]
    assert rec.shape[1] == Ls.record_doubles(shared is not None)
    d_rec = torch.from_numpy(rec).cuda()
    d_sh = torch.from_numpy(np.ascontiguousarray(shared)).cuda() if shared is not None else None

    def buf(cnt):
        h = np.full(cnt + TAIL, PREFILL, dtype=np.uint64)
        h[cnt:] = SENTINEL
        return torch.from_numpy(h.view(np.float64)).cuda()

    outs = [buf(B * Ls.nnzA), buf(B * Ls.m), buf(B * Ls.m)]
    Ls.assemble_batch_device(B, d_rec.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                             d_sh.data_ptr() if d_sh is not None else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = []
    for o, width in zip(outs, (Ls.nnzA, Ls.m, Ls.m)):
        h = o.cpu().numpy()
        assert (h[B * width:].view(np.uint64) == SENTINEL).all(), "the kernel wrote behind its output"
        res.append(h[:B * width].reshape(B, width))
    return tuple(res)


def _buffers(sw, B):
    Ls = sw.layout
    pa, pl, pu = sw.debug_buffers()
    return _d2h(pa, (B, Ls.nnzA)), _d2h(pl, (B, Ls.m)), _d2h(pu, (B, Ls.m))


def _check(got, want, what):
    for nm, g, w in zip(("Ax", "l", "u"), got, want):
        w = w[:len(g)]
        ok = AR.same_bits(g, w)
        if not ok.all():
            b, k = np.argwhere(~ok)[0]
            raise AssertionError("%s: %s differs in %d places, first at agent %d entry %d: got %r (%#x), want %r (%#x)" % (
                what, nm, int((~ok).sum()), b, k, g[b, k], g[b, k].view(np.uint64), w[b, k], w[b, k].view(np.uint64)))


# ------------------------------------------------------------------------------- records and references, computed once
_CASES = {}


def _case(name, which, special):
    """(full records [9, R], flags, what goes to the device, reference (Ax, l, u)) of a layout x packing x special set"""
    key = (name, which, special)
    if key not in _CASES:
        L, keep = Z.get(name), Z.packing(name, which)
        recs = Z.records(name, max(Z.BATCHES), seed=11, keep=keep, special=special)
        dev = recs if keep is None else AR.pack(L, keep, recs)
        _CASES[key] = (recs, keep, np.ascontiguousarray(dev), AR.assemble_batch(L, recs))
    return _CASES[key]


def _shared_case(name, special):
    """records that share the Jacobians of agent 0: (own [9, R'], shared, reference of the records they stand for)"""
    key = (name, "shared", special)
    if key not in _CASES:
        L = Z.get(name)
        own, shared, full = Z.shared_of(L, _case(name, "none", special)[0])
        _CASES[key] = (own, shared, AR.assemble_batch(L, full))
    return _CASES[key]


# ------------------------------------------------------------------------------------------------------ the direct form
@pytest.mark.parametrize("name", Z.NAMES)
def test_direct_form_equals_the_reference(sfb, name):
    cases = 0
    for special in ("finite", "nonfinite"):
        for which in Z.PACKINGS:
            recs, keep, dev, want = _case(name, which, special)
            Ls = Z.to_sfb(sfb, name, keep)
            for B in Z.BATCHES:
                _check(_direct(Ls, dev[:B]), want, "%s/%s/%s/B=%d" % (name, which, special, B))
                cases += 1
        own, shared, want = _shared_case(name, special)
        for which in ("none", "random"):                       # a packed layout with a shared record: the flags are ignored
            Ls = Z.to_sfb(sfb, name, Z.packing(name, which))
            for B in Z.BATCHES:
                _check(_direct(Ls, own[:B], shared), want, "%s/shared+%s/%s/B=%d" % (name, which, special, B))
                cases += 1
    print("direct form, %s: %d cases" % (name, cases))


def test_direct_form_across_the_seam_of_its_launch_loop(sfb):
    """gridDim.y ends at 65 535: agent 65 535 starts the second launch of mpc_assemble_launch.  Distinct records per agent,
    every agent compared."""
    B = 65537
    L, Ls = Z.get("minimal"), Z.to_sfb(sfb, "minimal")
    recs = Z.records("minimal", B, seed=12)
    assert len(np.unique(recs[:, 0])) == B
    want = AR.assemble_batch(L, recs)
    t0 = time.perf_counter()
    got = _direct(Ls, recs)
    print("direct form, seam: %d agents, %.3f s wall (copies included)" % (B, time.perf_counter() - t0))
    _check(got, want, "minimal/seam")
    for b in (65534, 65535, 65536):
        assert all(AR.all_same_bits(g[b], w[b]) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------------- the table form
def _plan(sfb, L):
    Ap, Aj = AR.pattern(L)
    return sfb.SparseQPPlan(L.n, L.m, np.arange(L.n + 1), np.arange(L.n), Ap, Aj)       # P = identity


def _swarm(sfb, plan, Ls, B):
    return sfb.MPCSwarm(plan, Ls, np.ones(Ls.n), np.zeros(Ls.n), B)


@pytest.mark.parametrize("name", Z.NAMES)
def test_table_form_equals_the_reference_and_the_direct_form(sfb, name):
    """One tick per record form; the solver's codes are not asserted (three iterations on numbers chosen to test the
    assembly, not to be solved).  Only the finite special set goes through a tick."""
    L = Z.get(name)
    plan = _plan(sfb, L)
    prm = sfb.QPSolverParams(**TICK)
    own, shared, want_sh = _shared_case(name, "finite")
    cases = 0
    for at, which in enumerate(Z.PACKINGS):
        recs, keep, dev, want = _case(name, which, "finite")
        other = Z.PACKINGS[(at + 1) % len(Z.PACKINGS)]
        _, keep_o, dev_o, want_o = _case(name, other, "finite")
        Ls = Z.to_sfb(sfb, name, keep)
        direct = _direct(Ls, dev)
        _check(direct, want, "%s/%s direct" % (name, which))
        for B in Z.BATCHES:
            tag = "%s/%s/B=%d" % (name, which, B)
            sw = _swarm(sfb, plan, Ls, B)
            sw.step_host(dev[:B], prm)
            got = _buffers(sw, B)
            _check(got, want, tag + " table")
            _check(got, direct, tag + " table against direct")
            sw.step_host(own[:B], prm, shared_jac=shared)                    # the flags of the swarm's layout are ignored
            _check(_buffers(sw, B), want_sh, tag + " shared table")
            assert sw.set_jac_keep(keep_o) == AR.record_doubles(L, keep_o)   # another packing ...
            sw.step_host(dev_o[:B], prm)
            _check(_buffers(sw, B), want_o, tag + " table after set_jac_keep(%s)" % other)
            assert sw.set_jac_keep(keep) == AR.record_doubles(L, keep)       # ... and back
            sw.step_host(dev[:B], prm)
            _check(_buffers(sw, B), want, tag + " table after set_jac_keep back")
            sw.close()
            cases += 4
    print("table form, %s: %d ticks compared" % (name, cases))


@pytest.mark.parametrize("name", ["so3", "se3x2"])
@pytest.mark.parametrize("which", ["none", "edges"])
def test_flat_table_is_commutative_and_unpacked_whatever_the_swarm(sfb, name, which):
    L = Z.get(name)
    plan = _plan(sfb, L)
    prm = sfb.QPSolverParams(**TICK)
    _, keep, dev, want = _case(name, which, "finite")
    Ls = Z.to_sfb(sfb, name, keep)
    for B in Z.BATCHES:
        sw = _swarm(sfb, plan, Ls, B)
        sw.step_host(dev[:B], prm)
        _check(_buffers(sw, B), want, "%s/%s/B=%d first tick" % (name, which, B))
        ptr, rd = sw.device_records()
        assert rd == AR.record_doubles(L, keep)
        flat = Z.records(name, B, seed=13, special="finite")                 # FULL records, whatever the swarm's packing
        _h2d(ptr, flat)
        sw.step_resident_flat(prm)
        got = _buffers(sw, B)
        _check(got, AR.assemble_batch(L, flat, flat=True), "%s/%s/B=%d flat" % (name, which, B))
        with_ad = AR.assemble_batch(L, flat)
        assert not AR.all_same_bits(got[0], with_ad[0])                      # (the ad term would have shown)
        sw.close()


def test_table_form_across_the_seam_of_its_launch_loop(sfb):
    """Four agents per thread and 65 535 grid rows: agent 4 * 65 535 starts the second launch.  Distinct records per agent,
    every agent compared.  (The tick of these 262 141 three-variable QPs takes 0.03 s of wall time on an MI355X; printed.)"""
    B = 4 * 65535 + 1
    L, Ls = Z.get("minimal"), Z.to_sfb(sfb, "minimal")
    recs = Z.records("minimal", B, seed=14)
    assert len(np.unique(recs[:, 0])) == B
    want = AR.assemble_batch(L, recs)
    sw = _swarm(sfb, _plan(sfb, L), Ls, B)
    t0 = time.perf_counter()
    sw.step_host(recs, sfb.QPSolverParams(**TICK))
    print("table form, seam: %d agents, tick %.3f s wall" % (B, time.perf_counter() - t0))
    got = _buffers(sw, B)
    sw.close()
    _check(got, want, "minimal/table seam")
    for b in (4 * 65535 - 1, 4 * 65535):
        assert all(AR.all_same_bits(g[b], w[b]) for g, w in zip(got, want))
