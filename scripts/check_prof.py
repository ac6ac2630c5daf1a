"""Where a stopping check of the sparse kernel spends its time, and how often its parts run (profiling build:
PROF_DEFS=-DSFB_PROF_CHECK scripts/build_prof.sh, then SFB_LIB_PATH=smooth_feedback_amd/libsfb_prof.so scripts/check_prof.py;
add -DSFB_CHECK_FULL_PASSES for the check without the early exits of the infeasibility passes).
Cases: the headline batch (8 192 cold QPs: first launch in the standard form, loop launch in the LAT form), 512 QPs (LAT form
as a whole) and warm ticks of the swarm (TICKS=0 skips them; the swarm front links libsfb.so by that name, so for the ticks the
profiling build has to be installed as smooth_feedback_amd/libsfb.so of a scratch copy of the tree).  Counters are sums over all
checks of a case, per form."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import smooth_feedback_amd as sfb
from smooth_feedback_amd import _capi
from examples import models_lib as M

NAMES = ["checks", "optimal", "dual_residual_pass", "ordered_cert_sum", "pass2_Atdy", "primal_infeasible", "pass3_Pdx", "qdx_chain",
         "Adx_row_conditions", "dual_infeasible"]
CYC = ["optimality(pass 1)", "certificate sum", "pass 2 (A'dy)", "pass 3 (P dx)", "rest (dx staging, q'dx, A dx rows)"]
L = C.CDLL(_capi.LIB_PATH)
if not hasattr(L, "sfb_debug_check_prof"):
    sys.exit("not a profiling build: PROF_DEFS=-DSFB_PROF_CHECK scripts/build_prof.sh, SFB_LIB_PATH=.../libsfb_prof.so")


def counters(reset=True):
    out = np.zeros((2, 48), np.uint64)
    assert L.sfb_debug_check_prof(out.ctypes.data_as(C.c_void_p), int(reset)) == 0
    return out


def report(title):
    c = counters()
    print("== %s" % title)
    for f, form in enumerate(("standard form", "LAT form")):
        v = c[f].astype(np.float64)
        if v[0] == 0:
            continue
        print("  %s: %d checks" % (form, v[0]))
        print("    " + ", ".join("%s %d (%.1f %%)" % (NAMES[i], v[i], 100.0 * v[i] / v[0]) for i in range(1, 10)))
        tot = v[10:15].sum()
        print("    cycles per check %.0f: " % (tot / v[0]) + ", ".join("%s %.0f" % (CYC[i], v[10 + i] / v[0]) for i in range(5)))
        for base, name, ran in ((16, "pass 2", v[4]), (32, "pass 3", v[6])):
            if ran:
                print("    %s, cycles when it runs %.0f; group of 64 rows of the first deciding row (last: none): %s"
                      % (name, v[12 + (base == 32)] / ran, " ".join("%d" % x for x in c[f][base:base + 16])))


variant, K = int(os.environ.get("VARIANT", 12)), int(os.environ.get("K", 50))
d, Pp, Pi, Pv, Ap, Aj = M.mpc_pattern(variant, K)
for B in (8192, 512):
    Av, l, u = M.mpc_assemble_batch(variant, K, B, seed=3, threads=16)
    keep = np.any(Av[:: max(1, B // 64)] != 0.0, axis=0)
    plan = sfb.SparseQPPlan(d["n"], d["m"], Pp, Pi, Ap, Aj, stage=M.mpc_stage(variant, K), keep=keep)
    counters()
    r = plan.solve_batch_host(np.tile(Pv, (B, 1)), np.zeros((B, d["n"])), Av, l, u, sfb.QPSolverParams())
    report("%d cold QPs, n = %d, m = %d: mean iterations %.1f, codes %s" % (B, d["n"], d["m"], r.iter.mean(), np.bincount(r.code, minlength=5)))

ticks = int(os.environ.get("TICKS", 4))
if ticks:
    B = 8192
    u0 = np.zeros((B, 2)); codes = np.zeros(B, np.int32); iters = np.zeros(B, np.uint32)
    step = lambda nt: M.lib().sfbx_mpc_swarm_step(variant, K, C.c_double(5.0), C.c_int64(B), C.c_uint64(1), nt, u0.ctypes.data_as(C.c_void_p),
                                                  codes.ctypes.data_as(C.c_void_p), iters.ctypes.data_as(C.c_void_p))
    counters()
    assert step(ticks) == 0
    if counters(reset=False).sum() == 0:
        sys.exit("the ticks ran through another library than %s: the swarm front links smooth_feedback_amd/libsfb.so by name -- install "
                 "the profiling build under that name in a scratch copy of the tree (or TICKS=0)" % _capi.LIB_PATH)
    report("%d ticks of a swarm of %d (one cold, the others warm): last tick mean iterations %.1f" % (ticks, B, iters.mean()))
