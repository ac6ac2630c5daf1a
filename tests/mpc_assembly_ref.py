"""Independent numpy restatement of the numeric fill of the MPC QP: ocp_to_qp_update_dyn, _cr and _ce
(ocp_to_qp.hpp:240-373), from the agents' full (unpacked) linearisation records (include/sfb.h, sfb_mpc_layout).

It works on a dense m x n float64 matrix per agent with the block operations of those lines, in their order, in plain
double arithmetic (numpy's elementwise products and sums are rounded one by one: no fused multiply-add):

    1. A = 0.0
    2. A[dyn rows of the node, x_node] += tf * dfdx,   A[.., u_node] += tf * dfdu
    3. A[dyn rows of the node, x_node] += (-tf / 2) * ad(f + dxdes)          (bundle with a non-commutative part)
    4. A[row d, component d of x_{M+j}] -= alpha_s * D(j, i),  j = 0..kmesh
    l = u = -tf * (f - dxdes);   cr rows: A = [dcdx | dcdu], l = crl - c, u = cru - c;   ce rows: A = J, l = u = 0.0 - e

and only then gathers the values in the CSR order of the pattern (pattern(), built from a dense boolean mask of the same
blocks).  Nothing here computes the place of a stored entry from its index, which is what mpc_assemble_kernel and
mpc_build_table do.  ad is a dense matrix from the definitions of the groups, part by part at its tangent offset.
Every function takes one record [R] or a batch [B, R]: the agents are a leading axis of the same block operations.

MISTAKES is a switchboard of deliberate errors for tests/test_mpc_assembly_ref_host.py: each is a slip the kernel could make,
and the layout zoo must be able to tell every one of them from the truth."""
from dataclasses import dataclass, field

import numpy as np

RN, SE2, SO3, SE3 = 0, 1, 2, 3

MISTAKES = ("alpha0", "D_transposed", "no_ad", "ad_sign", "ad_offset", "so3_as_se2", "se3_no_upper_right", "bound_plus_dxdes",
            "cr_swapped", "J_transposed", "dfdu_stride_nx", "no_zero_plus", "popcount_inclusive")


@dataclass
class Layout:
    """The numbers of sfb_mpc_layout (no ctypes): D[j, i] of shape (kmesh + 1, kmesh), parts = [(kind, dof), ...]."""
    nx: int
    nu: int
    ncr: int
    kmesh: int
    nivals: int
    tf: float
    alpha: np.ndarray
    D: np.ndarray
    parts: tuple = ()
    crl: np.ndarray = field(default_factory=lambda: np.zeros(0))
    cru: np.ndarray = field(default_factory=lambda: np.zeros(0))

    @classmethod
    def of(cls, L):
        """from a smooth_feedback_amd.MPCLayout"""
        return cls(L.nx, L.nu, L.ncr, L.kmesh, L.nivals, L.tf, np.array(L.alpha), np.array(L.D).reshape(L.kmesh + 1, L.kmesh),
                   tuple((int(k), int(d)) for k, d in zip(L.kind, L.dof)), np.array(L.crl), np.array(L.cru))

    @property
    def N(self):
        return self.kmesh * self.nivals

    @property
    def n(self):
        return self.nx * (self.N + 1) + self.nu * self.N

    @property
    def m(self):
        return self.N * self.nx + self.N * self.ncr + self.nx

    @property
    def noncommutative(self):
        return any(k != RN for k, _ in self.parts)


# ---------------------------------------------------------------------------------------------------------- the record
FIELDS = ("f", "dx", "dfdx", "dfdu", "c", "dcdx", "dcdu", "e", "J")
OWN, SHARED = ("f", "dx", "c", "e", "J"), ("dfdx", "dfdu", "dcdx", "dcdu")
JAC_BLOCKS = ("dfdx", "dfdu", "dcdx", "dcdu", "J")       # the order of the flags of sfb_mpc_layout::jac_keep


def field_shapes(L):
    """shape of every field of the full record, in the record's order (matrices row-major (d, c))"""
    N, nx, nu, ncr = L.N, L.nx, L.nu, L.ncr
    return dict(f=(N, nx), dx=(N, nx), dfdx=(N, nx, nx), dfdu=(N, nx, nu), c=(N, ncr), dcdx=(N, ncr, nx), dcdu=(N, ncr, nu),
                e=(nx,), J=(1, nx, nx))


def _cut(L, rec, names):
    """rec [.., doubles of the named fields] -> {field: [.., its shape]} (views)"""
    shp = field_shapes(L)
    out, o = {}, 0
    for k in names:
        cnt = int(np.prod(shp[k]))
        out[k] = rec[..., o:o + cnt].reshape(rec.shape[:-1] + shp[k])
        o += cnt
    assert o == rec.shape[-1], "not a record of this layout"
    return out


def split(L, rec):
    """full record(s) -> {field: array of its shape}"""
    return _cut(L, rec, FIELDS)


def join(parts, names=FIELDS, lead=()):
    """{field: [lead.., its shape]} -> record(s) [lead.., doubles]"""
    return np.concatenate([np.asarray(parts[k], dtype=np.float64).reshape(tuple(lead) + (-1,)) for k in names], axis=-1)


def split_keep(L, keep):
    """flags [dfdx | dfdu | dcdx | dcdu | J] -> {block: bool (rows, cols)}"""
    shp = field_shapes(L)
    out, o = {}, 0
    keep = np.asarray(keep).astype(bool)
    for k in JAC_BLOCKS:
        r, c = shp[k][1:]
        out[k] = keep[o:o + r * c].reshape(r, c)
        o += r * c
    assert o == keep.size
    return out


def jac_flags(L):
    return 2 * L.nx * L.nx + L.nx * L.nu + L.ncr * L.nx + L.ncr * L.nu


def record_doubles(L, keep=None, shared=False):
    """doubles of one agent's record: full, packed by `keep`, or without the Jacobians it shares (flags ignored)"""
    shp = field_shapes(L)
    total = 0
    for k in (OWN if shared else FIELDS):
        if k in JAC_BLOCKS and keep is not None and not shared:
            total += shp[k][0] * int(split_keep(L, keep)[k].sum())
        else:
            total += int(np.prod(shp[k]))
    return total


def shared_jac_doubles(L):
    shp = field_shapes(L)
    return sum(int(np.prod(shp[k])) for k in SHARED)


def nnzA(L):
    return int(pattern(L)[0][-1])


def pack(L, keep, rec):
    """full record(s) -> packed: per node (J: once) the flagged entries of every Jacobian block, row by row"""
    p, km = split(L, rec), split_keep(L, keep)
    return join({k: (p[k][..., km[k]] if k in JAC_BLOCKS else p[k]) for k in FIELDS}, lead=rec.shape[:-1])


def unpack(L, keep, packed, mistakes=()):
    """packed record (one agent) -> full record with 0.0 outside the flags.  mistakes: "popcount_inclusive" reads every kept
    entry from the place its mask gives when bit c itself is counted: one further, inside the record."""
    shp, km = field_shapes(L), split_keep(L, keep)
    out, o = {}, 0
    for k in FIELDS:
        if k in JAC_BLOCKS:
            blocks, cnt = shp[k][0], int(km[k].sum())
            full = np.zeros(shp[k])
            src = o + (1 if "popcount_inclusive" in mistakes else 0)
            full[:, km[k]] = np.resize(packed, packed.size + 1)[src:src + blocks * cnt].reshape(blocks, cnt)
            out[k] = full
            o += blocks * cnt
        else:
            cnt = int(np.prod(shp[k]))
            out[k] = packed[o:o + cnt]
            o += cnt
    assert o == packed.size, "not a packed record of this layout and these flags"
    return join(out)


def split_shared(L, rec):
    """full record(s) -> (record(s) without [dfdx | dfdu | dcdx | dcdu], those four as Jacobian record(s))"""
    p = split(L, rec)
    return join(p, OWN, rec.shape[:-1]), join(p, SHARED, rec.shape[:-1])


def merge_shared(L, own, shared):
    """the full record(s) that `own` [.., R'] stands for when the Jacobians come from the ONE record `shared`"""
    p = _cut(L, own, OWN)
    for k, v in _cut(L, shared, SHARED).items():
        p[k] = np.broadcast_to(v, own.shape[:-1] + v.shape)
    return join(p, lead=own.shape[:-1])


# --------------------------------------------------------------------------------------------------------- the pattern
def _blocks(L):
    """rows and columns of the QP: constraint rows [dyn | cr | ce], variables [x_0 .. x_N | u_0 .. u_{N-1}]"""
    N, nx, nu, ncr = L.N, L.nx, L.nu, L.ncr
    xcol = lambda node: slice(node * nx, (node + 1) * nx)
    ucol = lambda node: slice(nx * (N + 1) + node * nu, nx * (N + 1) + (node + 1) * nu)
    dyn = lambda node: slice(node * nx, (node + 1) * nx)
    cr = lambda node: slice(N * nx + node * ncr, N * nx + (node + 1) * ncr)
    ce = slice(N * (nx + ncr), N * (nx + ncr) + nx)
    return xcol, ucol, dyn, cr, ce


def pattern(L):
    """(Ap, Aj) of A in CSR, columns ascending: the pattern of ocp_to_qp_allocate as include/sfb.h states it"""
    xcol, ucol, dyn, cr, ce = _blocks(L)
    mask = np.zeros((L.m, L.n), dtype=bool)
    eye = np.eye(L.nx, dtype=bool)
    for s in range(L.nivals):
        M = s * L.kmesh
        for i in range(L.kmesh):
            node = M + i
            mask[dyn(node), xcol(node)] = True
            mask[dyn(node), ucol(node)] = True
            for j in range(L.kmesh + 1):
                mask[dyn(node), xcol(M + j)] |= eye
    for node in range(L.N):
        mask[cr(node), xcol(node)] = True
        mask[cr(node), ucol(node)] = True
    mask[ce, xcol(0)] = True
    rows, cols = np.nonzero(mask)        # row-major: rows ascending, columns ascending inside a row
    Ap = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int32)
    return Ap, cols.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ ad
def hat(w):
    """w [.., 3] -> [.., 3, 3]"""
    out = np.zeros(w.shape[:-1] + (3, 3))
    out[..., 0, 1], out[..., 0, 2] = -w[..., 2], w[..., 1]
    out[..., 1, 0], out[..., 1, 2] = w[..., 2], -w[..., 0]
    out[..., 2, 0], out[..., 2, 1] = -w[..., 1], w[..., 0]
    return out


def ad_part(kind, a, mistakes=()):
    """ad(a) of one part, a [.., dof] its tangent components.  SE2 (vx, vy, w), SO3 (w), SE3 (v, w)."""
    dof = a.shape[-1]
    out = np.zeros(a.shape[:-1] + (dof, dof))
    if kind == SE2:                                      # [[0, -w, vy], [w, 0, -vx], [0, 0, 0]]
        out[..., 0, 1], out[..., 0, 2] = -a[..., 2], a[..., 1]
        out[..., 1, 0], out[..., 1, 2] = a[..., 2], -a[..., 0]
    elif kind == SO3:
        out = hat(a)
        if "so3_as_se2" in mistakes:
            out[..., 2, :] = 0.0
    elif kind == SE3:                                    # [[hat(w), hat(v)], [0, hat(w)]]
        out[..., :3, :3] = hat(a[..., 3:])
        out[..., 3:, 3:] = hat(a[..., 3:])
        if "se3_no_upper_right" not in mistakes:
            out[..., :3, 3:] = hat(a[..., :3])
    return out


def ad(L, s, mistakes=()):
    """dense ad(s) of the bundle, s [.., nx]: the parts' ad matrices on the diagonal, each at its tangent offset"""
    out = np.zeros(s.shape[:-1] + (L.nx, L.nx))
    off = 0
    for kind, dof in L.parts:
        a = s[..., 0:dof] if "ad_offset" in mistakes else s[..., off:off + dof]
        out[..., off:off + dof, off:off + dof] = ad_part(kind, a, mistakes)
        off += dof
    return out


# ------------------------------------------------------------------------------------------------------------ assembly
def assemble_dense(L, recs, flat=False, mistakes=()):
    """(A [B, m, n] dense, l [B, m], u [B, m]) from FULL records [B, R].  flat: no ad term, whatever the parts."""
    recs = np.asarray(recs, dtype=np.float64)
    B = recs.shape[0]
    p = split(L, recs)
    xcol, ucol, dyn, cr, ce = _blocks(L)
    tf, nx, nu, km = L.tf, L.nx, L.nu, L.kmesh
    A = np.zeros((B, L.m, L.n))
    lo, hi = np.zeros((B, L.m)), np.zeros((B, L.m))
    Dm = np.asarray(L.D).reshape(km + 1, km)
    diag = np.arange(nx)
    dfdu_all = p["dfdu"]
    if "dfdu_stride_nx" in mistakes:                     # entry (d, c) of a node read at (node nx + d) nx + c behind dfdu's start
        tail = join(p, FIELDS[3:], (B,))
        tail = np.concatenate([tail] * (1 + nx * nx * L.N // max(1, tail.shape[1])), axis=1)
        at = ((np.arange(L.N)[:, None, None] * nx + np.arange(nx)[None, :, None]) * nx + np.arange(nu)[None, None, :])
        dfdu_all = tail[:, at]
    with np.errstate(all="ignore"):
        for s in range(L.nivals):
            M = s * km
            alpha = L.alpha[0] if "alpha0" in mistakes else L.alpha[s]
            for i in range(km):
                node = M + i
                f, dx = p["f"][:, node], p["dx"][:, node]
                if "no_zero_plus" in mistakes:
                    A[:, dyn(node), xcol(node)] = tf * p["dfdx"][:, node]
                    A[:, dyn(node), ucol(node)] = tf * dfdu_all[:, node]
                else:
                    A[:, dyn(node), xcol(node)] += tf * p["dfdx"][:, node]                                # :258
                    A[:, dyn(node), ucol(node)] += tf * dfdu_all[:, node]                                 # :259
                if L.noncommutative and not flat and "no_ad" not in mistakes:                             # :262-264
                    adm = ad(L, f + dx, mistakes)
                    A[:, dyn(node), xcol(node)] += ((tf / 2) if "ad_sign" in mistakes else (-tf / 2)) * adm
                for j in range(km + 1):                                                                   # :266-270
                    Dji = Dm.ravel()[i * km + j] if "D_transposed" in mistakes else Dm[j, i]
                    blk = A[:, dyn(node), xcol(M + j)]
                    blk[:, diag, diag] -= alpha * Dji
                lo[:, dyn(node)] = -tf * ((f + dx) if "bound_plus_dxdes" in mistakes else (f - dx))       # :272
                hi[:, dyn(node)] = lo[:, dyn(node)]                                                       # :273
        crl, cru = (L.cru, L.crl) if "cr_swapped" in mistakes else (L.crl, L.cru)
        for node in range(L.N):                                                                           # :320-322
            A[:, cr(node), xcol(node)] = p["dcdx"][:, node]
            A[:, cr(node), ucol(node)] = p["dcdu"][:, node]
            lo[:, cr(node)] = crl - p["c"][:, node]
            hi[:, cr(node)] = cru - p["c"][:, node]
        J = p["J"][:, 0]
        A[:, ce, xcol(0)] = J.transpose(0, 2, 1) if "J_transposed" in mistakes else J                     # :368
        lo[:, ce] = -p["e"] if "no_zero_plus" in mistakes else 0.0 - p["e"]                               # :371
        hi[:, ce] = lo[:, ce]                                                                             # :372
    return A, lo, hi


_PATTERNS = {}


def gather(L, A):
    """values of the dense A [.., m, n] in the CSR order of pattern(L)"""
    key = (L.nx, L.nu, L.ncr, L.kmesh, L.nivals)
    if key not in _PATTERNS:
        Ap, Aj = pattern(L)
        _PATTERNS[key] = (np.repeat(np.arange(L.m), np.diff(Ap)), Aj)
    rows, cols = _PATTERNS[key]
    return A[..., rows, cols]


def assemble_batch(L, recs, flat=False, mistakes=(), chunk=4096):
    """(Ax [B, nnzA], l [B, m], u [B, m]) from FULL records [B, R]"""
    out = []
    for b0 in range(0, len(recs), chunk):
        A, lo, hi = assemble_dense(L, recs[b0:b0 + chunk], flat, mistakes)
        out.append((gather(L, A), lo, hi))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def assemble(L, rec, flat=False, mistakes=()):
    """(Ax [nnzA], l [m], u [m]) of one agent from its FULL record"""
    return tuple(v[0] for v in assemble_batch(L, rec[None], flat, mistakes))


# ------------------------------------------------------------------------------------------------------- bit equality
def same_bits(a, b):
    """elementwise: the same uint64 pattern, or NaN on both sides"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def all_same_bits(a, b):
    return bool(same_bits(a, b).all())
