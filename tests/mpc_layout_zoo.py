"""A zoo of MPC layouts, record packings and records for the assembly kernel (tests/mpc_assembly_ref.py is the reference):
sizes at the kernel's block edges and at every limit check_layout admits, non-commutative parts at every tangent offset,
and numbers chosen so that no two terms of an entry can be confused:

  * D is a random (kmesh + 1, kmesh) matrix: no LGR matrix, neither symmetric nor banded;
  * alpha differs from interval to interval, crl != cru, tf is no power of two;
  * records are seeded; for a packing they carry exact zeros outside its flags.

No GPU and no library needed here."""
import zlib

import numpy as np

import mpc_assembly_ref as AR

RN, SE2, SO3, SE3 = AR.RN, AR.SE2, AR.SO3, AR.SE3

#        name          (nx, nu, ncr, kmesh, nivals)   parts (kind, dof)
SPECS = {
    "minimal":     ((1, 1, 0, 1, 1), ()),                                                   # smallest QP: n = 3, m = 2
    "commutative": ((5, 3, 1, 3, 2), ()),
    "rn_parts":    ((5, 3, 1, 3, 2), ((RN, 2), (RN, 3))),                                   # parts given, no ad
    "so3":         ((3, 3, 2, 5, 2), ((SO3, 3),)),                                          # nnzA + m = 512
    "mixed":       ((9, 2, 2, 1, 3), ((RN, 2), (SO3, 3), (SE2, 3), (RN, 1))),               # nnzA + m = 513, kmesh = 1
    "edge255":     ((3, 2, 0, 3, 3), ((SE2, 3),)),                                          # nnzA + m = 255
    "a_edge":      ((8, 2, 0, 4, 1), ((SE2, 3), (RN, 2), (SO3, 3))),                        # nnzA = 512
    "se3x2":       ((16, 4, 2, 4, 2), ((RN, 1), (SE3, 6), (SE3, 6), (SE2, 3))),             # SE3 off offset 0, twice
    "limits":      ((24, 32, 16, 8, 2), ((SE3, 6), (SO3, 3), (SE2, 3), (SE3, 6), (RN, 6))),  # every per-node limit
    "ivals":       ((2, 1, 1, 1, 128), ()),                                                 # every alpha slot
    "km8":         ((3, 2, 1, 8, 3), ((SO3, 3),)),                                          # widest D
}
NAMES = tuple(SPECS)
PACKINGS = ("none", "all", "random", "edges")
BATCHES = (1, 3, 4, 5, 9)

FINITE = (-0.0, 0.0, 5e-324 * 2 ** 30, 1e300)           # (a subnormal: 2^-1044)
NONFINITE = (np.inf, -np.inf, np.nan)
SPECIALS = {"finite": FINITE, "nonfinite": NONFINITE}


def _rng(*key):
    return np.random.default_rng([zlib.crc32(str(k).encode()) for k in key])


def counts(sizes):
    """(nnzA, m, n) from the closed forms of include/sfb.h"""
    nx, nu, ncr, kmesh, nivals = sizes
    N = kmesh * nivals
    return N * nx * (kmesh + nx + nu) + N * ncr * (nx + nu) + nx * nx, N * nx + N * ncr + nx, nx * (N + 1) + nu * N


# the block edges the sizes were chosen for (256 threads per block, one per entry of A and per row of l, u)
assert counts(SPECS["minimal"][0]) == (4, 2, 3)
assert sum(counts(SPECS["so3"][0])[:2]) == 512
assert sum(counts(SPECS["mixed"][0])[:2]) == 513
assert sum(counts(SPECS["edge255"][0])[:2]) == 255
assert counts(SPECS["a_edge"][0])[0] == 512
assert counts(SPECS["limits"][0])[1:] == (664, 920)


def layout(name):
    """AR.Layout of a zoo entry, with its seeded tf, alpha, D, crl, cru"""
    (nx, nu, ncr, kmesh, nivals), parts = SPECS[name]
    r = _rng("layout", name)
    tf = float(r.uniform(2.1, 3.9))                              # inside (2, 4): no power of two
    alpha = r.uniform(0.5, 2.0, nivals)
    assert len(set(alpha.tolist())) == nivals
    D = r.normal(size=(kmesh + 1, kmesh)) + 0.25 * r.choice([-1.0, 1.0], (kmesh + 1, kmesh))    # no entry near zero
    crl = -r.uniform(0.5, 1.5, ncr)
    cru = r.uniform(1.6, 2.5, ncr)
    L = AR.Layout(nx, nu, ncr, kmesh, nivals, tf, alpha, D, parts, crl, cru)
    assert sum(d for _, d in parts) in (0, nx)
    assert (AR.nnzA(L), L.m, L.n) == counts(SPECS[name][0])
    return L


_LAYOUTS = {}


def get(name):
    if name not in _LAYOUTS:
        _LAYOUTS[name] = layout(name)
    return _LAYOUTS[name]


def ad_support(L):
    """bool (nx, nx): where ad of the bundle can be non-zero"""
    s = np.arange(1.0, L.nx + 1.0)
    return AR.ad(L, s) != 0.0


def packing(name, which):
    """flags [dfdx | dfdu | dcdx | dcdu | J] of a packing of a zoo layout, None for "none" """
    L = get(name)
    if which == "none":
        return None
    nflags = AR.jac_flags(L)
    if which == "all":
        return np.ones(nflags, np.uint8)
    r = _rng("packing", name, which)
    if which == "random":
        return (r.random(nflags) < 0.4).astype(np.uint8)
    assert which == "edges"
    shp = AR.field_shapes(L)
    sup = ad_support(L)
    out = []
    for blk in AR.JAC_BLOCKS:
        rows, cols = shp[blk][1:]
        k = r.random((rows, cols)) < 0.5
        if blk == "dcdu" and rows > 0:
            k[:] = False                                          # one whole block empty
        elif rows >= 2:
            # the empty row: in dfdx one that crosses the support of ad (a dropped entry whose ad term is not zero)
            empty = int(np.argmax(sup.any(axis=1))) if (blk == "dfdx" and sup.any()) else int(r.integers(rows))
            full = (empty + 1 + int(r.integers(rows - 1))) % rows
            k[empty, :] = False
            k[full, :] = True                                     # (keeps the last column: bit cols - 1 of the row mask)
        elif rows == 1:
            k[:] = False
            k[0, cols - 1] = True                                 # only the last column
        out.append(k.ravel())
    keep = np.concatenate(out).astype(np.uint8)
    if sup.any():
        assert (sup & ~AR.split_keep(L, keep)["dfdx"]).any()
    return keep


def records(name, batch, seed=0, keep=None, special=None):
    """[batch][full record]: seeded normal values of mixed scale; zeros (+0.0) outside `keep`; with `special` ("finite" /
    "nonfinite") the values of that set at seeded spots of f, dxdes, every Jacobian block (kept entries only), c and e"""
    L = get(name)
    shp = AR.field_shapes(L)
    km = AR.split_keep(L, keep) if keep is not None else None
    r = _rng("records", name, seed, special)
    p = {}
    for k in AR.FIELDS:
        full = (batch,) + shp[k]
        v = r.normal(size=full) * np.exp2(r.integers(-3, 4, size=full))
        spots = np.ones(shp[k], dtype=bool)
        if km is not None and k in AR.JAC_BLOCKS:
            v[..., ~km[k]] = 0.0
            spots[:, ~km[k]] = False
        where = np.flatnonzero(spots.ravel())
        if special is not None and where.size:
            vals = SPECIALS[special]
            # per agent: a quarter of the field's places, at least two rounds of the set where the field has room for them
            cnt = min(where.size, max(2 * len(vals), where.size // 4))
            pick = where[r.random((batch, where.size)).argsort(axis=1)[:, :cnt]]
            put = r.permuted(np.tile(np.resize(vals, cnt), (batch, 1)), axis=1)
            v.reshape(batch, -1)[np.arange(batch)[:, None], pick] = put
        p[k] = v
    return AR.join(p, lead=(batch,))


def shared_of(L, recs):
    """([batch][record without Jacobians], shared Jacobian record of agent 0, the full records this stands for)"""
    own, jac = AR.split_shared(L, recs)
    shared = np.ascontiguousarray(jac[0])
    return np.ascontiguousarray(own), shared, AR.merge_shared(L, own, shared)


def to_sfb(sfb, name, keep=None):
    """smooth_feedback_amd.MPCLayout of a zoo entry"""
    L = get(name)
    return sfb.MPCLayout(L.nx, L.nu, L.ncr, L.kmesh, L.nivals, L.tf, L.alpha, L.D, parts=L.parts, crl=L.crl, cru=L.cru,
                         jac_keep=keep)
