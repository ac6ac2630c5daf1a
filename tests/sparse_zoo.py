"""Named structured sparsity patterns that pin every regime of the sparse plan (csrc/sparse_plan.cpp; DESIGN.md "Regimes of the
sparse plan"): numeric engine (unit / supernodal), LDS budget, segment mix (closed subtrees / open top runs) and sweep encoding.

Plain Python and numpy.  get(name) returns a dict with n, m, Pp, Pi (CSC of P), Ap, Aj (CSR of A), ordering, user_perm, stage,
keep and seeded values Px (positive diagonal), Ax in [-1, 1], q, l, u (one-sided, two-sided and a few equality rows); batch(name, B)
stacks B items whose values differ.  write_file(path, names) writes what tests/sparse_plan_check.cpp reads.

EXPECT[name] = (k, nnzL, units, lds_doubles, idx_scale, closed segments, open segments) of the plan's default engine, measured with
tests/sparse_plan_check.cpp; a pruned plan's whole-pattern fallback (built with the kernel plan's perm and LDS, as
sfb_sparse_qp_plan_create_pruned builds it) is the entry NAME + ".fallback".
"""
import struct
import zlib

import numpy as np

EXPECT = {
    #                            k     nnzL  units  lds  idx_scale closed open
    "clique53":                  (54, 1431, 1, 1536, 8, 1, 0),      # nnzL + k + 3 = 1488 <= kLdsSmall: the whole factor on chip
    "clique54":                  (55, 1485, 1, 2048, 8, 1, 0),      # 1543 > kLdsSmall: second attempt with kLdsTarget
    "clique62":                  (63, 1953, 1, 2048, 8, 1, 0),      # first column: 63 own + 1953 outside + 3 = 2019 <= 2048
    "clique63":                  (64, 2016, 0, 2048, 8, 1, 1),      # 64 + 2016 + 3 > 2048: no unit plan; panel of 64 rows
    "clique64":                  (65, 2080, 0, 2048, 8, 0, 1),      # panel rows 65 > 64: eliminated in LDS, no closed segment
    "clique100":                 (101, 5050, 0, 2048, 8, 0, 1),     # maxcol 100
    "chain8125":                 (8125, 8124, 1, 8128, 8, 1, 2),    # 65 024 bytes of LDS: the last size with 16-bit unit offsets
    "chain8127":                 (8127, 8126, 0, 8192, 8, 1, 2),    # LDS bytes = 2^16: supernodal engine, sweeps still in byte offsets
    "chain8189":                 (8189, 8188, 0, 8192, 8, 1, 2),
    "chain8191":                 (8191, 8190, 0, 8256, 1, 1, 2),    # (k + 1) * 8 = 2^16: element indices
    "chain399":                  (399, 398, 1, 832, 8, 1, 0),
    "arrow800":                  (800, 1597, 1, 1536, 8, 1, 2),
    "blockdiag400":              (400, 320, 1, 768, 8, 0, 1),       # 10 units for the 40 blocks together
    "rand200":                   (200, 2506, 1, 1536, 8, 4, 6),
    "tiny2":                     (2, 1, 1, 64, 8, 0, 1),
    "emptyrow":                  (9, 8, 1, 64, 8, 1, 1),
    "mpc6_10_pruned":            (204, 1117, 1, 1344, 8, 1, 0),
    "mpc6_10_pruned.fallback":   (204, 3315, 1, 1344, 8, 3, 1),     # lds_hint = the kernel plan's 1344 instead of kLdsSmall
}

# entries every consumer iterates over, in this order (the chained fallback entry follows its plan in the checker's file)
NAMES = ("clique53", "clique54", "clique62", "clique63", "clique64", "clique100", "chain8125", "chain8127", "chain8189", "chain8191",
         "chain399", "arrow800", "blockdiag400", "rand200", "tiny2", "emptyrow", "mpc6_10_pruned")
# the three boundary pairs of the issue: LDS budget, engine by column size, engine / encoding by the size of the work vector
BOUNDARY = ("clique53", "clique54", "clique62", "clique63", "chain8125", "chain8127", "chain8189", "chain8191")


def _diag_P(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)


def _csr(rows, n):
    Ap = np.zeros(len(rows) + 1, np.int32)
    Ap[1:] = np.cumsum([len(r) for r in rows])
    Aj = np.array([c for r in rows for c in sorted(r)], dtype=np.int32).reshape(-1)
    assert Aj.size == 0 or (Aj.min() >= 0 and Aj.max() < n)
    return Ap, Aj


def _chain_rows(n):
    return [(i, i + 1) for i in range(n - 1)]


def _pattern(name):
    """-> n, rows of A, (Pp, Pi), ordering, user_perm"""
    if name.startswith("clique"):    # P diagonal, one dense row of A eliminated first: its n columns become a clique
        n = int(name[6:])
        return n, [tuple(range(n))], _diag_P(n), 1, np.concatenate([[n], np.arange(n)]).astype(np.int32)
    if name.startswith("chain"):     # P diagonal, rows of A = {i, i + 1}, minimum degree: k = 2 n - 1
        k = int(name[5:])
        n = (k + 1) // 2
        return n, _chain_rows(n), _diag_P(n), 1, None
    if name == "arrow800":           # a chain plus one dense row
        n = 400
        return n, _chain_rows(n) + [tuple(range(n))], _diag_P(n), 1, None
    if name == "blockdiag400":       # 40 independent blocks of 6 unknowns and 4 rows; a block is a path of 7 unknowns of the KKT
        n = 240                      # system and one of 3: every subtree is smaller than the 8 columns a closed segment needs
        return n, [(6 * b + i, 6 * b + j) for b in range(40) for i, j in ((0, 1), (1, 2), (2, 3), (4, 5))], _diag_P(n), 1, None
    if name == "rand200":            # (n, m, density) = (80, 120, 0.05), P upper triangular with the same density
        n, m = 80, 120
        rng = np.random.default_rng(200)
        mask = rng.random((m, n)) < 0.05
        rows = [tuple(np.nonzero(r)[0]) for r in mask]
        pm = np.triu(rng.random((n, n)) < 0.05) | np.eye(n, dtype=bool)
        Pi = np.concatenate([np.nonzero(pm[:, c])[0] for c in range(n)]).astype(np.int32)
        Pp = np.concatenate([[0], np.cumsum(pm.sum(0))]).astype(np.int32)
        return n, rows, (Pp, Pi), 1, None
    if name == "tiny2":
        return 1, [(0,)], _diag_P(1), 1, None
    if name == "emptyrow":           # an A row with no entry (and a column of P without a stored diagonal)
        n = 5
        Pp, Pi = np.array([0, 1, 2, 2, 4, 5], np.int32), np.array([0, 1, 1, 3, 4], np.int32)
        return n, [(0, 1), (), (2, 4), (1, 2, 3)], (Pp, Pi), 1, None
    raise KeyError(name)


def _values(name, n, m, Pp, Pi, Ap, Aj, B):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    cols = np.repeat(np.arange(n), np.diff(Pp))
    Px = rng.uniform(-0.2, 0.2, (B, Pi.size))
    Px[:, Pi == cols] = rng.uniform(1.0, 2.0, (B, int((Pi == cols).sum())))
    Ax = rng.uniform(-1.0, 1.0, (B, Aj.size))
    q = rng.uniform(-1.0, 1.0, (B, n))
    lo, up = -rng.uniform(0.2, 1.0, (B, m)), rng.uniform(0.2, 1.0, (B, m))
    kind = rng.random(m)              # shared by the batch: 20 % lower only, 20 % upper only, 10 % equality, the rest two-sided
    l = np.where(kind[None] < 0.2, lo, np.where((kind[None] >= 0.2) & (kind[None] < 0.4), -np.inf, lo))
    u = np.where(kind[None] < 0.2, np.inf, up)
    eq = (kind >= 0.4) & (kind < 0.5)
    mid = rng.uniform(-0.1, 0.1, (B, m))
    l = np.where(eq[None], mid, l)
    u = np.where(eq[None], mid, u)
    return Px, Ax, q, l, u


def batch(name, B=1):
    if name == "mpc6_10_pruned":
        return _mpc(B)
    n, rows, (Pp, Pi), ordering, user_perm = _pattern(name)
    m = len(rows)
    Ap, Aj = _csr(rows, n)
    Px, Ax, q, l, u = _values(name, n, m, Pp, Pi, Ap, Aj, B)
    return dict(name=name, n=n, m=m, Pp=Pp, Pi=Pi, Ap=Ap, Aj=Aj, ordering=ordering, user_perm=user_perm, stage=None, keep=None,
                Px=Px, Ax=Ax, q=q, l=l, u=u)


def get(name):
    z = batch(name, 1)
    for key in ("Px", "Ax", "q", "l", "u"):
        z[key] = z[key][0]
    return z


def _mpc(B):
    """the MPC pattern of variant 6, K = 10 with the entries that are zero in every agent declared zero (the pruned plan of
    test_oracle_qp_sparse.py); values of the assembled agents"""
    from examples import models_lib as M
    d, Pp, Pi, Pv, Ap, Aj = M.mpc_pattern(6, 10)
    Av, l, u = M.mpc_assemble_batch(6, 10, max(B, 4), seed=3)
    keep = np.any(Av != 0.0, axis=0)
    Av, l, u = Av[:B], l[:B], u[:B]
    n, m = int(d["n"]), int(d["m"])
    return dict(name="mpc6_10_pruned", n=n, m=m, Pp=np.asarray(Pp, np.int32), Pi=np.asarray(Pi, np.int32), Ap=np.asarray(Ap, np.int32),
                Aj=np.asarray(Aj, np.int32), ordering=1, user_perm=None, stage=np.asarray(M.mpc_stage(6, 10), np.int32), keep=keep,
                Px=np.tile(np.asarray(Pv, float), (B, 1)), Ax=np.ascontiguousarray(Av), q=np.zeros((B, n)), l=l, u=u)


def dense_kkt(z, sigma=1e-6, rho=0.1, Ax=None):
    """[P + sigma I, A'; A, -1/rho I] of the upper-stored part of P, dense, caller's numbering: the float64 entries the kernel
    forms (P_ii + sigma and -1 / rho rounded to float64)"""
    n, m = z["n"], z["m"]
    K = np.zeros((n + m, n + m), np.float64)
    cols = np.repeat(np.arange(n), np.diff(z["Pp"]))
    for r, c, v in zip(z["Pi"], cols, z["Px"]):
        if r <= c:
            K[r, c] = K[c, r] = v
    rows = np.repeat(np.arange(m), np.diff(z["Ap"]))
    for r, c, v in zip(rows, z["Aj"], z["Ax"] if Ax is None else Ax):
        K[n + r, c] = K[c, n + r] = v
    K[np.arange(n), np.arange(n)] += sigma
    K[n + np.arange(m), n + np.arange(m)] = -1.0 / rho
    return K


def rhs(z):
    """the two right-hand sides the checker solves for (caller's numbering)"""
    k = z["n"] + z["m"]
    return np.random.default_rng(zlib.crc32(z["name"].encode()) + 1).uniform(-1.0, 1.0, (2, k))


def _entry_bytes(name, z, Aj, Ap, Ax, chain):
    n, m = z["n"], z["m"]
    i32 = lambda a: np.ascontiguousarray(a, dtype="<i4").tobytes()                       # noqa: E731
    f64 = lambda a: np.ascontiguousarray(a, dtype="<f8").tobytes()                       # noqa: E731
    perm, stage = z["user_perm"], z["stage"]
    nm = name.encode()
    out = struct.pack("<i", len(nm)) + nm
    out += struct.pack("<8i", n, m, z["ordering"], perm is not None, stage is not None, chain, len(z["Pi"]), len(Aj))
    out += i32(z["Pp"]) + i32(z["Pi"]) + i32(Ap) + i32(Aj)
    if perm is not None:
        out += i32(perm)
    if stage is not None:
        out += i32(stage)
    return out + f64(z["Px"]) + f64(Ax) + f64(rhs(z))


def file_entries(names=NAMES):
    """(entry name, zoo entry, A pattern and values as the checker sees them) -- a pruned entry comes as the kernel plan on the kept
    entries followed by its chained whole-pattern fallback"""
    out = []
    for name in names:
        z = get(name)
        if z["keep"] is None:
            out.append((name, z, z["Ap"], z["Aj"], z["Ax"], 0))
        else:
            keep = np.asarray(z["keep"], bool)
            rows = np.repeat(np.arange(z["m"]), np.diff(z["Ap"]))
            Ap2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=z["m"]))]).astype(np.int32)
            out.append((name, z, Ap2, z["Aj"][keep], z["Ax"][keep], 0))
            out.append((name + ".fallback", z, z["Ap"], z["Aj"], z["Ax"], 1))
    return out


def write_file(path, names=NAMES):
    entries = file_entries(names)
    with open(path, "wb") as f:
        f.write(b"SFBZOO1\0" + struct.pack("<i", len(entries)))
        for name, z, Ap, Aj, Ax, chain in entries:
            f.write(_entry_bytes(name, z, Aj, Ap, Ax, chain))
    return entries
