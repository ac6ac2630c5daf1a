"""The early exits of the sparse kernel's stopping check (csrc/qp_sparse.hip, sp_check_stopping, EARLY EXIT): the passes that form
|A'dy|_inf (primal infeasibility) and |P dx|_inf (dual infeasibility) stop at the first group of rows that settles the side of
the threshold -- a probe of one row per lane (rows 0..63), then groups of 64 rows (A'dy, standard form), 384 rows (A'dy, LAT form)
or 512 rows (P dx, both forms).  Every result here is compared BIT FOR BIT with the sparse CPU oracle, which forms every row:
code, iteration count, primal and dual.  Needs an MI355X.

Shapes, the smallest at which the groups exist: n = 136 (standard form: probe, rows 64..127, rows 128..135) and n = 584 (LAT
form of A'dy: probe, 64..447, 448..583; P dx: probe, 64..575, 576..583); m = 100.  The pattern is shared by every item: P
diagonal, row i of A has one entry in the first group (column i % 8), one in a middle group (64 + i % 60) and one in the last
(n - 8 + i % 7); the item KINDS zero some of them, which places the only columns of A'dy that can exceed the threshold:

  all / early / mid / late   feasible (bounds of one sign around A x0, so that the certificate sum is negative and the A'dy pass
                             runs), the deciding column in every group / the first / a middle one / the last one only
  pinf                       an all-zero row of A with the box [1, 2]: PrimalInfeasible, A'dy = 0 in every column: the full pass
  dinf_first / dinf_last     P_jj = 0, q_j = -1 and a zero column of A for j = 10 / j = n - 1: DualInfeasible, the full P dx pass
  nonfinite                  an infinity or a NaN in a value of A or in q

The threshold edge of the dual test (`fabs(row) > thr`, not `>=`) has a batch of its own, with dyadic data (see its test).
"""
import numpy as np
import pytest

from test_qp_dense_gpu import _oracle_params

pytestmark = pytest.mark.gpu

M_ROWS = 100
SHAPES = (136, 584)
KINDS = ("all", "early", "mid", "late", "pinf", "dinf_first", "dinf_last", "nonfinite")
FORMS = {"lat": {"SFB_SP_FORCE_LAT": 1}, "standard": {"SFB_SP_LAT": 0}}  # (the LAT form for the whole launch / never)


def pattern(n, m=M_ROWS):
    """-> Pp, Pi (CSC, diagonal), Ap, Aj (CSR, three entries per row: first group, a middle group, last group)."""
    Pp, Pi = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    i = np.arange(m)
    Aj = np.stack([i % 8, 64 + i % 60, n - 8 + i % 7], axis=1).astype(np.int32).ravel()
    Ap = (3 * np.arange(m + 1)).astype(np.int32)
    return Pp, Pi, Ap, Aj


def batch(n, per_kind=4, seed=5, m=M_ROWS):
    """per_kind items of every kind, in the order of KINDS -> kinds, Px, q, Ax, l, u."""
    rng = np.random.default_rng(seed + n)
    kinds = [k for k in KINDS for _ in range(per_kind)]
    B = len(kinds)
    _, _, _, Aj = pattern(n, m)
    Aj = Aj.reshape(m, 3)
    Px = 0.5 + rng.random((B, n))
    q = rng.standard_normal((B, n))
    Ax = rng.uniform(0.5, 1.5, (B, m, 3)) * rng.choice([-1.0, 1.0], (B, m, 3))
    l, u = np.empty((B, m)), np.empty((B, m))
    for b, kind in enumerate(kinds):
        keep = {"early": (1, 0, 0), "mid": (0, 1, 0), "late": (0, 0, 1)}.get(kind, (1, 1, 1))
        Ax[b] *= np.asarray(keep, dtype=np.float64)
        x0 = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
        Ax0 = (Ax[b] * x0[Aj]).sum(axis=1)
        Ax0 = np.where(np.abs(Ax0) < 0.5, np.nan, Ax0)  # rows rescaled so that A x0 = +-(1 .. 2): bounds of one sign
        tgt = rng.uniform(1.0, 2.0, m) * rng.choice([-1.0, 1.0], m)
        sc = np.where(np.isnan(Ax0), 1.0, tgt / np.where(np.isnan(Ax0), 1.0, Ax0))
        Ax[b] *= sc[:, None]
        Ax0 = (Ax[b] * x0[Aj]).sum(axis=1)
        l[b], u[b] = Ax0 - 0.3, Ax0 + 0.3
        free = rng.random(m) < 0.2  # one-sided rows (the certificate sum's break to +inf, the row conditions' one-sided forms)
        l[b] = np.where(free & (Ax0 > 0), -np.inf, l[b])
        u[b] = np.where(free & (Ax0 < 0), np.inf, u[b])
        if kind == "pinf":
            r = int(rng.integers(m))
            Ax[b, r], l[b, r], u[b, r] = 0.0, 1.0, 2.0
        if kind.startswith("dinf"):
            j = 10 if kind == "dinf_first" else n - 1  # (columns no row of A touches)
            Px[b, j], q[b, j] = 0.0, -1.0
        if kind == "nonfinite":
            w = b % 4
            if w == 0: Ax[b, 3, 2] = np.inf
            elif w == 1: Ax[b, 5, 0] = np.nan
            elif w == 2: q[b, n - 2] = np.nan
            else: q[b, 70] = -np.inf
    return kinds, Px, q, Ax.reshape(B, -1), l, u


def edge_batch(n, m=M_ROWS):
    """Threshold edge of the dual test.  Dyadic data, no scaling, eps_dual_inf = 2^-30: the variable j moves alone (q = -e_j, column
    j of A is zero, every other variable stays at exactly 0 between bounds that hold 0; P_jj is far below sigma, so x_j grows by
    about 1 / sigma per iteration), so row j of P dx is P_jj dx_j and thr = 2^-30 |dx_j| exactly.  P_jj = 2^-30: the row EQUALS
    thr, `>` does not fire, the full pass runs, the test goes on and the reference calls the item DualInfeasible at its first
    check; P_jj = 2^-30 (1 + 2^-52): the product rounds to the next double above thr or the one after, the row decides (in the
    probe for j = 10, in the last group for j = n - 1) at every check and the item iterates on to max_iter: a pass that dropped
    its later groups would call the fourth item DualInfeasible.
    Those four do not tell `>` from `>=` in the ballot: with every other row at 0, a ballot that fired on the row equal to thr would
    stop with the partial maximum thr, and !(Pdx_n <= thr) would still be false.  `>=` is wrong only where a row EQUAL to thr lies
    in an earlier group than a row ABOVE it; the fifth item has that.  Its variable 10 moves as in the first item (P = 2^-30, row 10
    of P dx equals thr, in the probe), and the variable n - 1 (last group) moves half as fast: q = -1/2, P = 2^-28, a zero column
    of A.  dx_(n-1) is just under dx_10 / 2, so |dx|_inf stays |dx_10| and row n - 1 of P dx is just under 2 thr: the reference
    iterates on to max_iter, and an exit on `>=` in the probe would report DualInfeasible at the first check.
    -> Px, q, Ax, l, u, prm-kwargs."""
    _, _, _, Aj = pattern(n, m)
    js = (10, n - 1, 10, n - 1, 10)
    B = len(js)
    Px, q = np.ones((B, n)), np.zeros((B, n))
    Ax = np.tile(np.where(Aj % 2 == 0, 1.0, -0.5), (B, 1))
    l, u = np.full((B, m), -1.0), np.full((B, m), 1.0)
    for b, j in enumerate(js):
        Px[b, j] = 2.0 ** -30 * (1.0 + 2.0 ** -52 if b in (2, 3) else 1.0)
        q[b, j] = -1.0
    Px[4, n - 1], q[4, n - 1] = 2.0 ** -28, -0.5
    return Px, q, Ax, l, u, dict(scaling=False, eps_dual_inf=2.0 ** -30, max_iter=60, stop_check_iter=5, polish=False)


_cache = {}


def case(sfb, oracle, n):
    """Plan, data and the oracle's results for a shape: computed once, shared, never modified."""
    if n not in _cache:
        Pp, Pi, Ap, Aj = pattern(n)
        plan = sfb.SparseQPPlan(n, M_ROWS, Pp, Pi, Ap, Aj)
        kinds, *data = batch(n)
        prm = sfb.QPSolverParams(max_iter=1500, stop_check_iter=5)
        ref = oracle.qp_sparse_solve_batch(Pp, Pi, data[0], data[1], Ap, Aj, *data[2:], perm=plan.perm, forder=plan.factor_order(),
                                           params=_oracle_params(oracle, prm), nthreads=8)
        *edata, ekw = edge_batch(n)
        eprm = sfb.QPSolverParams(**ekw)
        eref = oracle.qp_sparse_solve_batch(Pp, Pi, edata[0], edata[1], Ap, Aj, *edata[2:], perm=plan.perm, forder=plan.factor_order(),
                                            params=_oracle_params(oracle, eprm), nthreads=4)
        for r in (ref, eref):
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _cache[n] = dict(plan=plan, kinds=np.asarray(kinds), data=data, prm=prm, ref=ref, edata=edata, eprm=eprm, eref=eref)
    return _cache[n]


def same_bits(r, ref, sel=slice(None)):
    assert np.array_equal(r.code[sel], ref["code"][sel]), (r.code[sel], ref["code"][sel])
    assert np.array_equal(r.iter[sel], ref["iter"][sel]), (r.iter[sel], ref["iter"][sel])
    assert np.array_equal(r.primal[sel], ref["x"][sel], equal_nan=True) and np.array_equal(r.dual[sel], ref["y"][sel], equal_nan=True)


def check_oracle_verdicts(c):
    """What the inputs are built for, established on the oracle alone."""
    code, it, kinds = c["ref"]["code"], c["ref"]["iter"], c["kinds"]
    for k in ("all", "early", "mid", "late"):
        assert (code[kinds == k] == 0).all() and (it[kinds == k] > 5).all(), (k, code[kinds == k], it[kinds == k])
    assert (code[kinds == "pinf"] == 2).all() and (it[kinds == "pinf"] > 1).all() and (it[kinds == "pinf"] < 1500).all()
    for k in ("dinf_first", "dinf_last"):
        assert (code[kinds == k] == 3).all() and (it[kinds == k] < 1500).all(), (k, code[kinds == k])
    ecode, eit = c["eref"]["code"], c["eref"]["iter"]
    assert (ecode[:2] == 3).all() and (eit[:2] == 2).all() and (ecode[2:] == 4).all() and (eit[2:] == 60).all(), (ecode, eit)  # (item 4: iterates on)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("n", SHAPES)
def test_every_kind_matches_the_oracle_bit_for_bit(sfb, oracle, knobs, n, form):
    """Feasible items whose deciding column of A'dy lies in the first, a middle or the last group only, primal infeasible items
    (the full A'dy pass must still conclude, at the oracle's iteration), dual infeasible ones (the full P dx pass), non-finite data:
    codes, iteration counts, x and y identical to the oracle, in the standard and in the LAT form."""
    c = case(sfb, oracle, n)
    check_oracle_verdicts(c)
    knobs.set(**FORMS[form])
    r = c["plan"].solve_batch_host(*c["data"], c["prm"])
    for k in KINDS:
        same_bits(r, c["ref"], c["kinds"] == k)
    print(n, form, "codes", np.bincount(r.code, minlength=7), "iterations", r.iter.min(), r.iter.max())


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("n", SHAPES)
def test_threshold_edge_of_the_dual_test(sfb, oracle, knobs, n, form):
    """A row of P dx that equals thr exactly does not decide (`>`), the next double above does, and a row equal to thr in the probe
    does not hide a row above thr in the last group: see edge_batch."""
    c = case(sfb, oracle, n)
    check_oracle_verdicts(c)
    knobs.set(**FORMS[form])
    r = c["plan"].solve_batch_host(*c["edata"], c["eprm"])
    same_bits(r, c["eref"])
    assert (r.code[:2] == 3).all() and (r.code[2:] != 3).all()


@pytest.mark.parametrize("n", SHAPES)
def test_launch_variants_give_the_same_bits(sfb, oracle, knobs, n):
    """The same batch through tiny grids (time slicing; the launch in predicted order with the LAT loop launch), polishers on and
    off, both pause settings, the standard-form loop launch and the single launch: identical to the plain launch and the oracle."""
    c = case(sfb, oracle, n)
    plain = c["plan"].solve_batch_host(*c["data"], c["prm"])
    same_bits(plain, c["ref"])
    for kn in ({"SFB_SP_GRID": 3, "SFB_SP_SLICE": 10}, {"SFB_SP_GRID": 12}, {"SFB_SP_GRID": 12, "SFB_SP_POLISHERS": 0},
               {"SFB_SP_GRID": 12, "SFB_SP_POLISHERS": 2}, {"SFB_SP_GRID": 12, "SFB_SP_PAUSE": 2}, {"SFB_SP_GRID": 12, "SFB_SP_PAUSE": 27},
               {"SFB_SP_GRID": 12, "SFB_SP_LAT": 0}, {"SFB_SP_GRID": 12, "SFB_SP_PREDICT": 0}):
        knobs.set(**kn)
        r = c["plan"].solve_batch_host(*c["data"], c["prm"])
        knobs.clear(*kn)
        assert np.array_equal(r.code, plain.code) and np.array_equal(r.iter, plain.iter), kn
        assert np.array_equal(r.primal, plain.primal, equal_nan=True) and np.array_equal(r.dual, plain.dual, equal_nan=True), kn
        assert np.array_equal(r.objective, plain.objective, equal_nan=True), kn
