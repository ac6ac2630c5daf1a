"""One scenario for the bookkeeping of the MPC swarm, shared by tests/test_mpc_swarm_ref_host.py (the model alone, with the
CPU oracle as the solver) and tests/test_mpc_swarm_state_gpu.py (sfb.MPCSwarm against the model).

Layouts of tests/mpc_layout_zoo.py whose n, m, nu make 64-lane trips of every kind (CASES), a diagonal P with distinct
entries and a q that is non-zero everywhere (an empty P on `minimal`), and ten steps (SCRIPT):

    1 tick A   2 pass A1   3 pass A2   4 tick B   5 pass B1   6 tick C, no warm start   7 pass C1
    8 reset_warmstart()   9 tick A   10 pass A1

A refusal is injected as one +inf in the agent's record of that step, at a place that puts an upper bound at -inf (`c` where
the layout has running constraints, else `f`): the pre-check's PrimalInfeasible at iteration 0 (qp_solver.hpp:361-374).
The agent's index mod 6 is its role (ROLE_REFUSED).

What a pre-check refusal returns: the solver leaves at iteration 0 with its starting point, scaled and scaled back -- the
warm start up to an ulp per entry, exact zeros from a zero start.  So the refused solve of roles 2, 3 and 5 differs from
the plan they hold in last bits only (enough for a comparison bit for bit, which is what both tests make), and that of
roles 1 (at step 1) and 4 (always) is zero like the state it would overwrite.  NATURAL is therefore a second, short script
on the empty-P `minimal` layout in which the refusals are the solver's own: with P = 0 and q != 0 the problem is an
unbounded LP, which the solver calls DualInfeasible at its second or third stopping check (iteration 27 or 52 from a warm
start), far from the plan the agent holds; a step with max_iter = 1 ends before any check with MaxIterations, which a
controller keeps (the same on `minimal_emptyP`, where the injected script must not meet a refusal of the solver's own).
There a wrong branch moves every number.  No GPU needed here."""
import numpy as np

import mpc_assembly_ref as AR
import mpc_layout_zoo as Z
import mpc_swarm_ref as SR

# --------------------------------------------------------------------------------------------------------- the scripts
#          step  kind    records  warm start asked for   max_iter (None: the case's)
SCRIPT = ((1, "tick", "A", True, None), (2, "pass", "A1", None, None), (3, "pass", "A2", None, None), (4, "tick", "B", True, None),
          (5, "pass", "B1", None, None), (6, "tick", "C", False, None), (7, "pass", "C1", None, None), (8, "reset", None, None, None),
          (9, "tick", "A", True, None), (10, "pass", "A1", None, None))
SOLVES = tuple(s[0] for s in SCRIPT if s[1] != "reset")
ROLE_REFUSED = {0: (), 1: (1,), 2: (2,), 3: (2, 3), 4: SOLVES, 5: (4, 5)}
ROLE_TEXT = {0: "never refused", 1: "refused at tick 1 only", 2: "refused at pass 2, accepted at pass 3",
             3: "refused at both passes after an accepted tick", 4: "refused at every step", 5: "refused at tick 4 and pass 5"}

# no injection: every agent is refused (DualInfeasible, by the solver) at the steps that iterate up to the stopping check
NATURAL = ((1, "tick", "A", True, 1), (2, "pass", "A1", None, 102), (3, "pass", "A2", None, 1), (4, "tick", "B", True, 102),
           (5, "pass", "B1", None, 1), (6, "pass", "B2", None, 102), (7, "tick", "C", False, 1), (8, "pass", "C1", None, 1))
NATURAL_REFUSED = (2, 4, 6)

#        id              layout         B  empty P  max_iter  seed  script
# (seed and max_iter: the first of seeds 0..15, max_iter 60, 40, 26 with which tests/test_mpc_swarm_ref_host.py holds -- no
# refusal of the solver's own across the script, and the last bits of the refused solves tell in every role; `ivals` needs
# max_iter = 26, before the second stopping check, where its equality-heavy QPs start to be called infeasible)
CASES = {
    "commutative":    ("commutative", 12, False, 60, 1, "main"),      # n = 53 < 64
    "so3":            ("so3",         12, False, 60, 2, "main"),      # n = 63: one short of a trip; tick with ad, pass flat
    "km8":            ("km8",         12, False, 60, 2, "main"),      # n = 123: no multiple of 64
    "ivals":          ("ivals",       12, False, 26, 3, "main"),      # n = m = 386, nu = 1
    "limits":         ("limits",       4, False, 60, 0, "main"),      # n = 920, nu = 32: the nu limit
    "minimal_emptyP": ("minimal",     12, True,   1, 6, "main"),      # nnzP = 0: the len == 0 return of the replicate launch
    "so3_single":     ("so3",          1, False, 60, 3, "main"),      # B = 1
    "natural":        ("minimal",      5, True,   1, 0, "natural"),   # the solver's own refusals, far from the plan
}
SIZES = {"commutative": (53, 41, 3), "so3": (63, 53, 3), "km8": (123, 99, 2), "ivals": (386, 386, 1), "limits": (920, 664, 32),
         "minimal": (3, 2, 1)}
POLISH = False


def role(b):
    return b % 6


def field_offset(L, name):
    shp, o = AR.field_shapes(L), 0
    for k in AR.FIELDS:
        if k == name:
            return o
        o += int(np.prod(shp[k]))
    raise KeyError(name)


def inject(L, recs, agents):
    """+inf in the first entry of c (of f where the layout has no running constraint) of the given agents' records"""
    at = field_offset(L, "c" if L.ncr >= 1 else "f")
    recs[list(agents), at] = np.inf


class Case:
    """everything of one case that does not depend on who solves: layout, patterns, Px, q, and per step the full records
    (refusals injected) with the QP values the reference assembly makes of them and the refusals the script expects"""

    def __init__(self, cid, seed=None, max_iter=None):
        name, B, empty, mi, sd, script = CASES[cid]
        seed, mi = (sd if seed is None else seed), (mi if max_iter is None else max_iter)
        self.id, self.name, self.B, self.emptyP, self.max_iter, self.polish, self.script = cid, name, B, empty, mi, POLISH, script
        L = self.L = Z.get(name)
        assert (L.n, L.m, L.nu) == SIZES[name]
        self.n, self.m, self.nu, self.uoff = L.n, L.m, L.nu, L.nx * (L.N + 1)
        self.Ap, self.Aj = AR.pattern(L)
        r = Z._rng("swarm scenario", cid)
        if empty:
            self.Pp, self.Pi, self.Px = np.zeros(L.n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0)
        else:
            self.Pp, self.Pi = np.arange(L.n + 1, dtype=np.int32), np.arange(L.n, dtype=np.int32)
            self.Px = r.uniform(0.5, 2.0, L.n)
            assert len(set(self.Px.tolist())) == L.n
        self.q = r.normal(size=L.n)
        assert np.all(self.q != 0.0) and len(set(self.q.tolist())) == L.n
        self.steps = []
        for no, kind, tag, warm, smi in (SCRIPT if script == "main" else NATURAL):
            if kind == "reset":
                self.steps.append(dict(no=no, kind=kind))
                continue
            recs = Z.records(name, B, seed="swarm %s %d" % (tag, seed))
            if script == "main":
                refused = np.array([no in ROLE_REFUSED[role(b)] for b in range(B)])
                inject(L, recs, np.flatnonzero(refused))
            else:
                refused = np.full(B, no in NATURAL_REFUSED)
            with np.errstate(all="ignore"):
                Ax, lo, hi = AR.assemble_batch(L, recs, flat=(kind == "pass"))
            assert np.isfinite(Ax).all()                                         # (the +inf reaches the bounds only)
            self.steps.append(dict(no=no, kind=kind, warm=warm, recs=recs, Ax=Ax, l=lo, u=hi, refused=refused,
                                   max_iter=mi if smi is None else smi))

    def model(self, mistakes=()):
        return SR.Swarm(self.B, self.n, self.m, self.uoff, self.nu, self.Px, self.q, mistakes=mistakes)


_CASES = {}


def case(cid):
    if cid not in _CASES:
        _CASES[cid] = Case(cid)
    return _CASES[cid]


# ---------------------------------------------------------------------------------------------- the oracle as the solver
class OracleSolver:
    """solve(case, step, rows, Px, q, warm): the CPU oracle on the given agents of a step, with the plan's elimination and
    summation orders.  params_of(max_iter) makes the oracle's parameters."""

    def __init__(self, oracle, params_of, perm, forder, nthreads=8):
        self.oracle, self.params_of, self.perm, self.forder, self.nthreads = oracle, params_of, perm, forder, nthreads

    def __call__(self, cs, st, rows, Px, q, warm):
        rows = np.asarray(rows)
        wx, wy = (None, None) if warm is None else (warm[0][rows], warm[1][rows])
        Pxr = Px[rows] if Px.shape[1] else np.zeros((len(rows), 0))
        r = self.oracle.qp_sparse_solve_batch(cs.Pp, cs.Pi, Pxr, q[rows], cs.Ap, cs.Aj, st["Ax"][rows], st["l"][rows], st["u"][rows],
                                              perm=self.perm, forder=self.forder, params=self.params_of(st["max_iter"]),
                                              warm_x=wx, warm_y=wy, nthreads=self.nthreads)
        return SR.Solve(r["x"], r["y"], r["code"], r["iter"])


def start_of(cs, warm):
    """a cold start as the all-zero warm start it is (qp_solver.hpp:436-445)"""
    return (np.zeros((cs.B, cs.n)), np.zeros((cs.B, cs.m))) if warm is None else warm


def drive(cs, solver, mistakes=(), truth=None):
    """The script on a model with the given mistakes.  Returns the log: per step dict(no, kind, warm, sol, ret, Px, q) with the
    warm start the solve began from, the solve, and what the step returned.  truth: the log of the mistake-free run; an agent
    whose solve has the same inputs there (bit for bit) takes that solve instead of a new one."""
    mdl = cs.model(mistakes)
    log = []
    for at, st in enumerate(cs.steps):
        if st["kind"] == "reset":
            mdl.reset_warmstart()
            log.append(dict(no=st["no"], kind="reset"))
            continue
        is_pass = st["kind"] == "pass"
        warm = mdl.warm(warmstart=bool(st["warm"]), is_pass=is_pass)
        rows = np.arange(cs.B)
        sol = None
        if truth is not None:
            t = truth[at]
            (ax, ay), (bx, by) = start_of(cs, warm), start_of(cs, t["warm"])
            same = (AR.same_bits(ax, bx).all(axis=1) & AR.same_bits(ay, by).all(axis=1) & AR.same_bits(mdl.q, t["q"]).all(axis=1)
                    & AR.same_bits(mdl.Px, t["Px"]).all(axis=1))
            sol = SR.Solve(t["sol"].x, t["sol"].y, t["sol"].code, t["sol"].iter)
            rows = np.flatnonzero(~same)
        if len(rows):
            new = solver(cs, st, rows, mdl.Px, mdl.q, warm)
            if sol is None:
                sol = new
            else:
                sol.x[rows], sol.y[rows], sol.code[rows], sol.iter[rows] = new.x, new.y, new.code, new.iter
        if is_pass:
            mdl.relin_pass(sol)
        else:
            mdl.tick(sol, warmstart=bool(st["warm"]))
        log.append(dict(no=st["no"], kind=st["kind"], warm=warm, sol=sol, ret=mdl.returned(), Px=mdl.Px.copy(), q=mdl.q.copy()))
    return log


OBSERVABLES = ("du0", "code", "iter", "x", "y")


def first_difference(log, truth):
    """(step, observable) of the first returned value that differs between two logs, None if none does"""
    for a, b in zip(log, truth):
        if a["kind"] == "reset":
            continue
        for nm, u, v in zip(OBSERVABLES, a["ret"], b["ret"]):
            same = AR.same_bits(u, v) if u.dtype == np.float64 else (u == v)
            if not same.all():
                return a["no"], nm
    return None
