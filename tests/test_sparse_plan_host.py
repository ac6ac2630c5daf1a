"""Every regime of the sparse plan (csrc/sparse_plan.cpp) on the CPU: tests/sparse_plan_check.cpp -- a stand-alone program of
sparse_plan.cpp + knobs.cpp, built with AddressSanitizer and UBSan and run directly -- checks the structural invariants of every
schedule of every pattern of tests/sparse_zoo.py, executes the schedules as qp_sparse.hip does and compares L, D and two solutions
bit for bit with a plain left-looking LDL' and textbook triangular solves, for the default engine and for SFB_PLAN_UNITS=0.
No GPU, no libsfb.so in the checker.

Sanity of the checker's plain reference (zoo entries with k <= 400): backward error
    eta(x) = |K x - b|_inf / (|K|_inf |x|_inf + |b|_inf),   accumulated in np.longdouble on the dense K this module builds itself,
against GATE_MULTIPLE * max(eta(np.linalg.solve(K, b)), k 2^-52).  Measured at the commit that introduced this test (x86-64):
    eta(checker) between 1.8e-17 (clique100) and 8.4e-17 (mpc6_10_pruned), eta(numpy) between 3.5e-18 and 8.4e-17: the floor
    decides every gate.  Largest eta(checker) / max(eta(numpy), k 2^-52): 0.056 (tiny2: eta(checker) 2.50e-17, eta(numpy)
    4.72e-18, floor 2 * 2^-52 = 4.44e-16); next emptyrow 0.012 (2.31e-17 against 2.00e-15), every other entry <= 0.003
    (rand200: 5.13e-17, numpy 8.37e-17, floor 4.44e-14; chain399: 3.64e-17, numpy 2.51e-17, floor 8.86e-14).
    GATE_MULTIPLE = 2^-3 = 0.125: the smallest power of two that leaves a factor >= 2 (here 2.2) above the largest measured ratio.
    Both engines print the same x (asserted), so the figures hold for both.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import sparse_zoo as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smooth_feedback_amd", "csrc")
GATE_MULTIPLE = 0.125

# The regimes named in the issue, as (entry, engine) -> the fields that make the regime.  Deleting a zoo entry fails this list.
REGIMES = [
    ("unit engine, lds = kLdsSmall (1536)",                        "clique53",  "default", dict(units=1, lds_doubles=1536)),
    ("unit engine, lds = kLdsTarget (2048), first size",           "clique54",  "default", dict(units=1, lds_doubles=2048)),
    ("unit engine, lds = kLdsTarget (2048), last size",            "clique62",  "default", dict(units=1, lds_doubles=2048)),
    ("supernodal by column size, closed + open",                   "clique63",  "default", dict(units=0, lds_doubles=2048, closed=1, open=1)),
    ("supernodal, one open segment, R > 64 in LDS",                "clique64",  "default", dict(units=0, closed=0, open=1, maxR=65)),
    ("supernodal, panel rows far beyond 64",                       "clique100", "default", dict(units=0, maxcol=100, maxR=101)),
    ("unit engine on 8128 doubles (65 024 B), closed + 2 open",    "chain8125", "default", dict(units=1, lds_doubles=8128, closed=1, open=2, idx_scale=8)),
    ("supernodal because LDS bytes >= 2^16, byte offsets",         "chain8127", "default", dict(units=0, lds_doubles=8192, idx_scale=8)),
    ("the same at the last k with byte offsets",                   "chain8189", "default", dict(units=0, lds_doubles=8192, idx_scale=8)),
    ("element indices in the sweeps",                              "chain8191", "default", dict(units=0, idx_scale=1)),
    ("one closed segment, lds = k + 2 rounded up",                 "chain399",  "default", dict(units=1, lds_doubles=832, closed=1, open=0)),
    ("closed + open with outside accumulators at kLdsSmall",       "arrow800",  "default", dict(units=1, lds_doubles=1536, closed=1, open=2)),
    ("a single open segment with units",                           "blockdiag400", "default", dict(units=1, closed=0, open=1)),
    ("many segments, closed and open mixed",                       "rand200",   "default", dict(units=1, closed=4, open=6)),
    ("smallest plan",                                              "tiny2",     "default", dict(k=2, nnzL=1)),
    ("empty row of A, missing diagonal of P",                      "emptyrow",  "default", dict(k=9)),
    ("pruned plan",                                                "mpc6_10_pruned", "default", dict(units=1)),
    ("whole-pattern fallback built with the kernel plan's LDS",    "mpc6_10_pruned.fallback", "default", dict()),
    ("supernodal engine forced on a unit plan, on-chip segments",  "arrow800",  "supernodal", dict(units=0, lds_doubles=2048, closed=1, open=2)),
]


def _need(*tools):
    for t in tools:
        if shutil.which(t) is None:
            pytest.skip("no %s" % t)


@pytest.fixture(scope="module")
def checker(tmp_path_factory, sfb):
    """the stand-alone program (its own main, run directly: no preloading of anything) and the zoo file"""
    _need("g++")
    tmp = tmp_path_factory.mktemp("sparse_plan_check")
    exe, zoo = str(tmp / "sparse_plan_check"), str(tmp / "zoo.bin")
    cxx = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]
    srcs = [os.path.join(ROOT, "tests", "sparse_plan_check.cpp"), os.path.join(CSRC, "sparse_plan.cpp"), os.path.join(CSRC, "knobs.cpp")]
    objs = [str(tmp / ("tu%d.o" % i)) for i in range(len(srcs))]
    jobs = [subprocess.Popen(cxx + ["-c", s, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for s, o in zip(srcs, objs)]
    for job in jobs:    # (the three translation units side by side: the sanitized compile is most of this module's time)
        out = job.communicate()[0]
        assert job.returncode == 0, out
    build = subprocess.run(cxx + objs + ["-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and any(lib in build.stderr for lib in ("-lasan", "-lubsan", "libasan", "libubsan")):
        pytest.skip("the sanitizer runtime does not link here")
    assert build.returncode == 0, build.stderr
    entries = Z.write_file(zoo)
    return exe, zoo, entries


@pytest.fixture(scope="module")
def report(checker):
    """one run over the whole zoo: {(entry, engine): JSON line}"""
    exe, zoo, entries = checker
    run = subprocess.run([exe, zoo], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    for word in ("AddressSanitizer", "runtime error", "LeakSanitizer", "VIOLATION"):
        assert word not in run.stderr, run.stderr[-4000:]
    lines = [json.loads(ln) for ln in run.stdout.splitlines() if ln.startswith("{")]
    rep = {(ln["name"], ln["engine"]): ln for ln in lines}
    assert len(rep) == len(lines) == 2 * len(entries)
    return rep


def _tuple(ln):
    return (ln["k"], ln["nnzL"], ln["units"], ln["lds_doubles"], ln["idx_scale"], ln["closed"], ln["open"])


def test_every_plan_of_the_zoo_passes_and_has_the_expected_regime(report, checker):
    names = [e[0] for e in checker[2]]
    assert set(names) == set(Z.EXPECT), sorted(set(names) ^ set(Z.EXPECT))
    assert set(Z.NAMES) <= set(names) and len(Z.NAMES) >= 17
    for name in names:
        print("%-26s %s   supernodal: %s" % (name, _tuple(report[name, "default"]), _tuple(report[name, "supernodal"])))
    for name in names:
        assert _tuple(report[name, "default"]) == Z.EXPECT[name], name
        forced = report[name, "supernodal"]
        assert forced["units"] == 0 and forced["nunits"] == 0 and (forced["k"], forced["nnzL"]) == Z.EXPECT[name][:2]


def test_the_zoo_covers_every_regime(report):
    for what, name, engine, fields in REGIMES:
        assert (name, engine) in report, "%s: the zoo has no %s" % (what, name)
        got = {f: report[name, engine][f] for f in fields}
        assert got == fields, (what, name, got)
    # the boundaries are boundaries: neighbours differ in exactly the choice they pin
    d = lambda n: report[n, "default"]                                                   # noqa: E731
    assert d("clique53")["lds_doubles"] < d("clique54")["lds_doubles"] and d("clique62")["units"] != d("clique63")["units"]
    assert d("chain8125")["units"] != d("chain8127")["units"] and d("chain8189")["idx_scale"] != d("chain8191")["idx_scale"]
    assert Z.EXPECT["chain8125"][0] == 8125 and Z.EXPECT["chain8191"][0] == 8191
    # the fallback of the pruned plan runs with at least the kernel plan's LDS (sfb_sparse_qp_plan_create_pruned)
    assert d("mpc6_10_pruned.fallback")["lds_doubles"] >= d("mpc6_10_pruned")["lds_doubles"]
    assert d("mpc6_10_pruned.fallback")["nnzL"] > d("mpc6_10_pruned")["nnzL"]


def _eta(K, x, b):
    K, x, b = (np.asarray(a, np.longdouble) for a in (K, x, b))
    return float(np.abs(K @ x - b).max() / (np.abs(K).sum(1).max() * np.abs(x).max() + np.abs(b).max()))


def test_backward_error_of_the_plain_reference(report, checker):
    """the checker's solution (its emulation and its reference agree bit for bit) solves the system this module builds"""
    done = 0
    for name, z, Ap, Aj, Ax, chain in checker[2]:
        k = z["n"] + z["m"]
        if k > 400:
            assert "x" not in report[name, "default"]
            continue
        K = Z.dense_kkt(dict(z, Ap=Ap, Aj=Aj), Ax=Ax)
        b = Z.rhs(z)[0]
        floor = k * 2.0 ** -52
        eta_np = _eta(K, np.linalg.solve(K, b), b)
        for engine in ("default", "supernodal"):
            x = np.array(report[name, engine]["x"])
            eta = _eta(K, x, b)
            print("%-26s %-10s k %4d  eta(checker) %.2e  eta(numpy) %.2e  floor %.2e  ratio %.3f" % (name, engine, k, eta, eta_np, floor, eta / max(eta_np, floor)))
            assert eta <= GATE_MULTIPLE * max(eta_np, floor), (name, engine, eta, eta_np, floor)
        assert report[name, "default"]["x"] == report[name, "supernodal"]["x"]
        done += 1
    assert done >= 11


@pytest.mark.parametrize("family,array", [("sweep", "fidx"), ("ustream", "uomap"), ("supernodal", "rab"), ("kmap", "Kmap")])
def test_a_corrupted_schedule_is_reported(checker, family, array):
    """one corrupted entry per schedule family: two forward-sweep slots of different steps exchanged, one outside accumulator of a
    unit segment redirected, the row pairs of two trailing slots exchanged, the accumulators of two KKT entries exchanged"""
    exe, zoo, _ = checker
    for name in ("arrow800", "rand200"):
        run = subprocess.run([exe, zoo, "--only", name, "--mutate", family], capture_output=True, text=True)
        assert run.returncode == 1, (run.returncode, run.stderr[-2000:])
        msg = [ln for ln in run.stderr.splitlines() if ln.startswith("VIOLATION")]
        assert len(msg) == 1 and msg[0].startswith("VIOLATION %s/" % name) and array in msg[0].split(":")[1], run.stderr[-2000:]
        assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
    ok = subprocess.run([exe, zoo, "--only", "arrow800"], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr[-2000:]


def test_the_checker_names_pattern_array_and_index(checker):
    exe, zoo, _ = checker
    run = subprocess.run([exe, zoo, "--only", "rand200", "--mutate", "sweep"], capture_output=True, text=True)
    assert run.returncode == 1
    import re
    assert re.search(r"^VIOLATION rand200/default: fidx\[\d+\]: ", run.stderr, re.M), run.stderr[-2000:]
