"""The per-agent bookkeeping of the device-resident MPC swarm (sfb_mpc_swarm_*, csrc/capi_mpc.hip) as a plain numpy state
machine: what an agent holds between two solves, and which solve it starts the next one from.  It solves nothing: every
transition is handed the result (x, y, code, iter) of a solve that somebody else made.

The rule, with its sources:

  * a controller stores a solution as the warm start of the next solve only if it asked for warm starts AND the verdict is
    Optimal, MaxTime or MaxIterations (mpc.hpp:510-516 of the reference; include/smooth_feedback_amd/mpc.hpp:833-836 here);
    the input it returns is the first input of the solve it just made, whatever the verdict (:518 / :837);
  * a re-linearisation pass solves from the stored solution; a solve with one of those three verdicts replaces the plan and
    the stored solution, any other leaves both (MPC::relin_pass, include/smooth_feedback_amd/mpc.hpp:847-861);
  * on the device: mpc_store_kernel after a tick (du0 from the new solve; wx, wy overwritten under `store && kept`),
    mpc_accept_kernel after a pass (kept: x, y, code, iter, wx, wy := the new solve; else nothing moves, and du0 is read from
    the plan the agent held), mpc_replicate_kernel at creation (every agent gets the one Px and the one q) --
    all three in csrc/mpc_assemble.hip; sfb_mpc_swarm_reset_warmstart zeroes wx, wy (an all-zero warm start IS the cold
    start of qp_solver.hpp:436-445).

State per agent: the plan (x, y, code, iter), the warm start (wx, wy), the first input du0.  wx, wy start as zeros; the
plan and du0 are undefined until the first tick, and the model refuses to hand them out or to make a pass before it.

MISTAKES is a switchboard of deliberate errors for tests/test_mpc_swarm_ref_host.py: each is a slip one of the three
kernels (or the entry around them) could make, and the scenario of tests/mpc_swarm_scenario.py must be able to tell every
one of them from the truth.  No GPU and no library needed here; nothing is imported from the code under test."""
import numpy as np

KEPT = (0, 4, 5)            # Optimal, MaxIterations, MaxTime: the verdicts whose solve a controller keeps
POLISH_FAILED, MAX_ITERATIONS = 1, 4

MISTAKES = ("accept_all", "refuse_all", "du0_from_new_when_refused", "du0_stale_when_refused", "warm_from_refused_tick",
            "warm_from_refused_pass", "store_ignores_flag", "pass_starts_cold", "code_without_iter", "polish_failed_kept",
            "max_iterations_refused", "q_rotated", "px_first_entry_for_all")


class Undefined(RuntimeError):
    """the plan was asked for (or a pass was made) before the first tick"""


class Solve:
    """the result of one batched solve: x [B, n], y [B, m], code [B], iter [B]"""

    def __init__(self, x, y, code, iter):
        self.x = np.array(x, dtype=np.float64)
        self.y = np.array(y, dtype=np.float64)
        self.code = np.array(code, dtype=np.int32)
        self.iter = np.array(iter, dtype=np.uint32)
        assert self.x.ndim == 2 and self.y.ndim == 2 and self.code.shape == self.iter.shape == (len(self.x),)


class Swarm:
    def __init__(self, B, n, m, uoff, nu, Px=(), q=None, mistakes=()):
        assert all(k in MISTAKES for k in mistakes), mistakes
        assert 0 <= uoff and uoff + nu <= n
        self.B, self.n, self.m, self.uoff, self.nu, self.mistakes = B, n, m, uoff, nu, tuple(mistakes)
        self.x, self.y = np.full((B, n), np.nan), np.full((B, m), np.nan)
        self.code, self.iter = np.full(B, -1, np.int32), np.zeros(B, np.uint32)
        self.du0 = np.full((B, nu), np.nan)
        self.wx, self.wy = np.zeros((B, n)), np.zeros((B, m))
        self.defined = np.zeros(B, dtype=bool)               # the mask of "undefined": plan and du0 before the first tick
        # mpc_replicate_kernel: the one Px [nnzP] and the one q [n], for every agent
        Px = np.asarray(Px, dtype=np.float64).reshape(-1)
        q = np.zeros(n) if q is None else np.asarray(q, dtype=np.float64)
        assert q.shape == (n,)
        self.Px, self.q = np.tile(Px, (B, 1)), np.tile(q, (B, 1))
        if "q_rotated" in self.mistakes:
            self.q = np.roll(self.q, 1, axis=1)
        if "px_first_entry_for_all" in self.mistakes and Px.size:
            self.Px[:] = Px[0]

    # ------------------------------------------------------------------------------------------------- the verdicts
    def _kept(self, code):
        kept = set(KEPT)
        if "polish_failed_kept" in self.mistakes:
            kept.add(POLISH_FAILED)
        if "max_iterations_refused" in self.mistakes:
            kept.discard(MAX_ITERATIONS)
        return np.isin(code, sorted(kept))

    def _check(self, sol):
        assert isinstance(sol, Solve) and sol.x.shape == (self.B, self.n) and sol.y.shape == (self.B, self.m)

    # --------------------------------------------------------------------------------------------- the transitions
    def tick(self, sol, warmstart=True):
        """mpc_store_kernel: the plan is the new solve whatever its verdict, so is du0; the warm start only under
        `warmstart and kept`"""
        self._check(sol)
        self.x, self.y, self.code, self.iter = sol.x.copy(), sol.y.copy(), sol.code.copy(), sol.iter.copy()
        self.defined[:] = True
        self.du0 = sol.x[:, self.uoff:self.uoff + self.nu].copy()
        store = self._kept(sol.code) if (warmstart or "store_ignores_flag" in self.mistakes) else np.zeros(self.B, bool)
        if "warm_from_refused_tick" in self.mistakes and warmstart:
            store = np.ones(self.B, bool)
        self.wx[store], self.wy[store] = sol.x[store], sol.y[store]

    def relin_pass(self, sol):
        """mpc_accept_kernel: kept agents take the new solve as plan and warm start, the others keep everything; du0 of the
        plan held afterwards"""
        if not self.defined.all():
            raise Undefined("a re-linearisation pass before the first tick")
        self._check(sol)
        ok = self._kept(sol.code)
        if "accept_all" in self.mistakes:
            ok = np.ones(self.B, bool)
        if "refuse_all" in self.mistakes:
            ok = np.zeros(self.B, bool)
        before = self.du0.copy()
        self.x[ok], self.y[ok], self.code[ok] = sol.x[ok], sol.y[ok], sol.code[ok]
        if "code_without_iter" not in self.mistakes:
            self.iter[ok] = sol.iter[ok]
        warm = np.ones(self.B, bool) if "warm_from_refused_pass" in self.mistakes else ok
        self.wx[warm], self.wy[warm] = sol.x[warm], sol.y[warm]
        self.du0 = self.x[:, self.uoff:self.uoff + self.nu].copy()
        if "du0_from_new_when_refused" in self.mistakes:
            self.du0[~ok] = sol.x[~ok, self.uoff:self.uoff + self.nu]
        if "du0_stale_when_refused" in self.mistakes:
            self.du0[~ok] = before[~ok]

    def reset_warmstart(self):
        self.wx[:], self.wy[:] = 0.0, 0.0

    # ------------------------------------------------------------------------------------------------ what is read
    def warm(self, warmstart=True, is_pass=False):
        """(wx, wy) the next solve starts from, None for a cold start: a tick without warm start.  A pass always starts
        from the stored solution."""
        if is_pass and not self.defined.all():
            raise Undefined("a re-linearisation pass before the first tick")
        if is_pass and "pass_starts_cold" in self.mistakes:
            return None
        if not is_pass and not warmstart:
            return None
        return self.wx.copy(), self.wy.copy()

    def returned(self):
        """(du0, code, iter, x, y) as a step of the swarm returns them"""
        if not self.defined.all():
            raise Undefined("the plan before the first tick")
        return self.du0.copy(), self.code.copy(), self.iter.copy(), self.x.copy(), self.y.copy()
