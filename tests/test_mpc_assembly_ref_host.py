"""CPU checks of the assembly reference (tests/mpc_assembly_ref.py) and of the layout zoo (tests/mpc_layout_zoo.py) that the
GPU tests of mpc_assemble_kernel stand on: the reference equals the C++ host transcription bit for bit on the example
models, stays within a derived rounding bound of exact rational arithmetic on the zoo, agrees with the C-ABI on every size,
and the zoo's records tell every deliberate mistake of the reference's switchboard from the truth.  No GPU."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_assembly_ref as AR  # noqa: E402
import mpc_layout_zoo as Z  # noqa: E402
from examples import models_lib as M  # noqa: E402


# ------------------------------------------------------------------------------------- reference against the host front
@pytest.mark.parametrize("variant,K", [(6, 10), (12, 20), (13, 8)])
def test_reference_equals_the_host_transcription(variant, K):
    B = 3
    Av, l, u = M.mpc_assemble_batch(variant, K, B, seed=4)
    Ls, rec = M.mpc_records(variant, K, B, seed=4)
    L = AR.Layout.of(Ls)
    assert L.noncommutative
    d, _, _, _, Ap, Aj = M.mpc_pattern(variant, K)
    Ap2, Aj2 = AR.pattern(L)
    assert (L.n, L.m, AR.nnzA(L)) == (d["n"], d["m"], d["nnzA"])
    assert np.array_equal(Ap2, Ap) and np.array_equal(Aj2, Aj)
    A2, l2, u2 = AR.assemble_batch(L, rec)
    assert AR.all_same_bits(A2, Av) and AR.all_same_bits(l2, l) and AR.all_same_bits(u2, u)
    # the shared-Jacobian form and a packing carry the same information
    own, shared = AR.split_shared(L, rec[0])
    assert np.array_equal(AR.merge_shared(L, own, shared), rec[0])
    keep = Ls.jac_keep_of(rec)
    assert np.array_equal(AR.unpack(L, keep, AR.pack(L, keep, rec[1])), rec[1])


# ------------------------------------------------------------------------------------ reference against exact arithmetic
def _frac(a):
    out = np.empty(np.shape(a), dtype=object)
    flat = out.reshape(-1)
    for i, v in enumerate(np.asarray(a, dtype=np.float64).reshape(-1)):
        flat[i] = Fraction(float(v))
    return out


def _hat_exact(w):
    z = Fraction(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=object)


def _ad_exact(L, s):
    out = np.full((L.nx, L.nx), Fraction(0), dtype=object)
    off = 0
    for kind, dof in L.parts:
        a = s[off:off + dof]
        if kind == AR.SE2:
            blk = np.full((3, 3), Fraction(0), dtype=object)
            blk[0, 1], blk[1, 0] = -a[2], a[2]              # -w, w
            blk[0, 2], blk[1, 2] = a[1], -a[0]              # vy, -vx
            out[off:off + 3, off:off + 3] = blk
        elif kind == AR.SO3:
            out[off:off + 3, off:off + 3] = _hat_exact(a)
        elif kind == AR.SE3:
            out[off:off + 3, off:off + 3] = _hat_exact(a[3:])
            out[off + 3:off + 6, off + 3:off + 6] = _hat_exact(a[3:])
            out[off:off + 3, off + 3:off + 6] = _hat_exact(a[:3])
        off += dof
    return out


def _exact(L, rec):
    """(A, l, u) in rationals and, entry by entry, the sum S of the magnitudes of the terms that make it up"""
    p = {k: _frac(v) for k, v in AR.split(L, rec).items()}
    xcol, ucol, dyn, cr, ce = AR._blocks(L)
    zero = Fraction(0)
    A, SA = np.full((L.m, L.n), zero, dtype=object), np.full((L.m, L.n), zero, dtype=object)
    lo, hi, Sl, Su = (np.full(L.m, zero, dtype=object) for _ in range(4))
    tf, alpha, D, crl, cru = Fraction(L.tf), _frac(L.alpha), _frac(L.D), _frac(L.crl), _frac(L.cru)
    ab = np.vectorize(abs, otypes=[object])
    idx = np.arange(L.nx)
    for s in range(L.nivals):
        M0 = s * L.kmesh
        for i in range(L.kmesh):
            node = M0 + i
            f, dx = p["f"][node], p["dx"][node]
            A[dyn(node), xcol(node)] += tf * p["dfdx"][node]
            SA[dyn(node), xcol(node)] += ab(tf * p["dfdx"][node])
            A[dyn(node), ucol(node)] += tf * p["dfdu"][node]
            SA[dyn(node), ucol(node)] += ab(tf * p["dfdu"][node])
            if L.noncommutative:
                A[dyn(node), xcol(node)] += (-tf / 2) * _ad_exact(L, f + dx)
                SA[dyn(node), xcol(node)] += (tf / 2) * ab(_ad_exact(L, ab(f) + ab(dx)))
            for j in range(L.kmesh + 1):
                A[dyn(node), xcol(M0 + j)][idx, idx] -= alpha[s] * D[j, i]
                SA[dyn(node), xcol(M0 + j)][idx, idx] += abs(alpha[s] * D[j, i])
            lo[dyn(node)] = -tf * (f - dx)
            hi[dyn(node)] = lo[dyn(node)]
            Sl[dyn(node)] = tf * (ab(f) + ab(dx))
            Su[dyn(node)] = Sl[dyn(node)]
    for node in range(L.N):
        if L.ncr:
            A[cr(node), xcol(node)] = p["dcdx"][node]
            A[cr(node), ucol(node)] = p["dcdu"][node]
            lo[cr(node)] = crl - p["c"][node]
            hi[cr(node)] = cru - p["c"][node]
            Sl[cr(node)] = ab(crl) + ab(p["c"][node])
            Su[cr(node)] = ab(cru) + ab(p["c"][node])
    A[ce, xcol(0)] = p["J"][0]
    lo[ce] = -p["e"]
    hi[ce] = lo[ce]
    Sl[ce] = ab(p["e"])
    Su[ce] = Sl[ce]
    SA = np.where(SA == zero, ab(A), SA)            # (the copied entries of the cr and ce rows: their own magnitude)
    return (AR.gather(L, A), lo, hi), (AR.gather(L, SA), Sl, Su)


@pytest.mark.parametrize("name", Z.NAMES)
def test_reference_is_within_a_rounding_bound_of_exact_arithmetic(name):
    """An entry of A is ((0.0 + tf j) + (-tf / 2)(+-(f_k + dx_k))) - alpha D: at most six roundings (two products, the sum
    f_k + dx_k, two sums, the product alpha D), each at most 2^-53 relative on a quantity of magnitude at most
    S = |tf j| + |tf / 2| (|f_k| + |dx_k|) + |alpha D| (times 1 + a few 2^-53); a dynamics bound is two roundings on at most
    |tf| (|f| + |dx|).  8 * 2^-53 * S covers the six and their compounding.  Derived, not measured."""
    L = Z.get(name)
    rec = Z.records(name, 1, seed=3)[0]
    got = AR.assemble(L, rec)
    want, S = _exact(L, rec)
    bound = Fraction(8, 2 ** 53)
    for g, w, s in zip(got, want, S):
        assert np.isfinite(g).all()
        for x, y, t in zip(g, w, s):
            assert abs(Fraction(float(x)) - y) <= bound * t
    worst = max(float(abs(Fraction(float(x)) - y) / t) for g, w, s in zip(got, want, S) for x, y, t in zip(g, w, s) if t != 0)
    print(name, "worst error / S = %.3g (bound %.3g)" % (worst, float(bound)))


# ----------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("name", Z.NAMES)
def test_sizes_of_the_c_abi_equal_the_reference_counts(sfb, name):
    L = Z.get(name)
    for which in Z.PACKINGS:
        keep = Z.packing(name, which)
        Ls = Z.to_sfb(sfb, name, keep)
        assert (Ls.n, Ls.m) == (L.n, L.m)
        assert Ls.nnzA == AR.nnzA(L) == Z.counts(Z.SPECS[name][0])[0]
        assert Ls.record_doubles() == AR.record_doubles(L, keep)
        assert Ls.record_doubles(True) == AR.record_doubles(L, keep, shared=True) == AR.record_doubles(L, None, shared=True)
        assert Ls.shared_jac_doubles == AR.shared_jac_doubles(L)
        assert AR.record_doubles(L) == AR.record_doubles(L, None, shared=True) + AR.shared_jac_doubles(L)
        rec = Z.records(name, 2, seed=1, keep=keep)
        if keep is not None:                                   # the package's own packer agrees with the reference's
            assert np.array_equal(Ls.pack_records(rec), np.array([AR.pack(L, keep, x) for x in rec]))
            assert AR.pack(L, keep, rec[0]).size == Ls.record_doubles()
            assert np.array_equal(AR.unpack(L, keep, AR.pack(L, keep, rec[1])), rec[1])


def test_edges_packing_has_its_edges():
    for name in Z.NAMES:
        L = Z.get(name)
        km = AR.split_keep(L, Z.packing(name, "edges"))
        for blk, k in km.items():
            rows, cols = k.shape
            if blk == "dcdu":
                assert not k.any()
            elif rows >= 2:
                assert (~k).all(axis=1).any() and k.all(axis=1).any() and k[:, cols - 1].any()
            elif rows == 1:
                assert k[0, cols - 1]
        if L.noncommutative:
            assert (Z.ad_support(L) & ~km["dfdx"]).any()       # the table's src = -1 with a non-zero ad code
        rnd = Z.packing(name, "random")
        assert rnd.size == AR.jac_flags(L)
    assert AR.split_keep(Z.get("limits"), Z.packing("limits", "edges"))["dfdu"][:, 31].any()   # mask bit 31


# ------------------------------------------------------------------------------------ the zoo can tell the mistakes apart
def _differs(name, mistake):
    L = Z.get(name)
    for which in ("none", "edges", "random"):
        keep = Z.packing(name, which)
        for special in (None, "finite"):
            for rec in Z.records(name, 2, seed=5, keep=keep, special=special):
                truth = AR.assemble(L, rec)
                if mistake == "popcount_inclusive":
                    if keep is None:
                        continue
                    wrong = AR.assemble(L, AR.unpack(L, keep, AR.pack(L, keep, rec), mistakes=(mistake,)))
                else:
                    wrong = AR.assemble(L, rec, mistakes=(mistake,))
                if not all(AR.all_same_bits(a, b) for a, b in zip(truth, wrong)):
                    return True
    return False


@pytest.mark.parametrize("mistake", AR.MISTAKES)
def test_zoo_tells_the_mistake_from_the_truth(mistake):
    """Each mistake, switched on in the reference alone, changes the bits of some output on some zoo layout's records: a
    kernel that made it could not pass the GPU tests.  (The small layouts come first; the search stops at the first hit.)"""
    order = sorted(Z.NAMES, key=lambda nm: Z.get(nm).m * Z.get(nm).n)
    hits = []
    for name in order:
        if _differs(name, mistake):
            hits.append(name)
            break
    print(mistake, "seen on", hits)
    assert hits, "no zoo layout can see the mistake '%s'" % mistake


def test_mistake_free_reference_is_deterministic_and_flat_drops_only_ad():
    L = Z.get("so3")
    rec = Z.records("so3", 1, seed=2, special="finite")[0]
    a, b = AR.assemble(L, rec), AR.assemble(L, rec)
    assert all(AR.all_same_bits(x, y) for x, y in zip(a, b))
    flat, no_ad = AR.assemble(L, rec, flat=True), AR.assemble(L, rec, mistakes=("no_ad",))
    assert all(AR.all_same_bits(x, y) for x, y in zip(flat, no_ad))
    assert not AR.all_same_bits(flat[0], a[0])
    Lc = Z.get("commutative")
    rc = Z.records("commutative", 1, seed=2)[0]
    assert all(AR.all_same_bits(x, y) for x, y in zip(AR.assemble(Lc, rc), AR.assemble(Lc, rc, flat=True)))
