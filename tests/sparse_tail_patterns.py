"""Patterns for the column tail of the forward sweep (csrc/sparse_plan.h "COLUMN TAIL") beyond those of tests/sparse_zoo.py, shared
by tests/test_sparse_plan_tail_host.py (layout, CPU) and tests/test_sparse_lat_tail_gpu.py (register tail of the LAT form).

"twoclique60": the dense-trailing pattern of the zoo's cliques (P diagonal, a dense row of A eliminated first) with trailing entries
removed -- two rows of A over the columns 0 .. 49 and 40 .. 59, eliminated first: columns 12 .. 39 reach the rows up to 49 only, so
the trailing 48 x 48 block of L lacks the entries (50 .. 59, 12 .. 39).
"headline": the benchmark's model (variant 12, K = 50: n = m = 740) pruned the way bench.py prunes it."""
import numpy as np

import sparse_zoo as Z


def twoclique60(B=1):
    n = 60
    rows = [tuple(range(0, 50)), tuple(range(40, 60))]
    Pp, Pi = Z._diag_P(n)
    Ap, Aj = Z._csr(rows, n)
    Px, Ax, q, l, u = Z._values("twoclique60", n, len(rows), Pp, Pi, Ap, Aj, B)
    perm = np.concatenate([[n, n + 1], np.arange(n)]).astype(np.int32)
    return dict(name="twoclique60", n=n, m=len(rows), Pp=Pp, Pi=Pi, Ap=Ap, Aj=Aj, ordering=1, user_perm=perm, stage=None, keep=None,
                Px=Px, Ax=Ax, q=q, l=l, u=u)


def headline(B=16, seed=3):
    from examples import models_lib as M
    d, Pp, Pi, Pv, Ap, Aj = M.mpc_pattern(12, 50)
    Av, l, u = M.mpc_assemble_batch(12, 50, max(B, 64), seed=seed)
    keep = np.any(Av[:: max(1, Av.shape[0] // 64)] != 0.0, axis=0)
    Av, l, u = Av[:B], l[:B], u[:B]
    n, m = int(d["n"]), int(d["m"])
    return dict(name="headline", n=n, m=m, Pp=np.asarray(Pp, np.int32), Pi=np.asarray(Pi, np.int32), Ap=np.asarray(Ap, np.int32),
                Aj=np.asarray(Aj, np.int32), ordering=1, user_perm=None, stage=np.asarray(M.mpc_stage(12, 50), np.int32), keep=keep,
                Px=np.tile(np.asarray(Pv, float), (B, 1)), Ax=np.ascontiguousarray(Av), q=np.zeros((B, n)), l=l, u=u)


def batch(name, B):
    if name == "twoclique60":
        return twoclique60(B)
    if name == "headline":
        return headline(B)
    return Z.batch(name, B)


def one(name):
    z = batch(name, 1)
    for key in ("Px", "Ax", "q", "l", "u"):
        z[key] = z[key][0]
    return z


def zoo_entry_bytes(name):
    """the entry as tests/sparse_zoo.py writes one (a pruned plan: its kept entries)"""
    z = one(name)
    Ap, Aj, Ax = z["Ap"], z["Aj"], z["Ax"]
    if z["keep"] is not None:
        keep = np.asarray(z["keep"], bool)
        rows = np.repeat(np.arange(z["m"]), np.diff(Ap))
        Ap = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=z["m"]))]).astype(np.int32)
        Aj, Ax = Aj[keep], Ax[keep]
    return Z._entry_bytes(name, z, Aj, Ap, Ax, 0)

