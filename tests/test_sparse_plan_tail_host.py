"""The column tail of the forward sweep schedule (csrc/sparse_plan.h "COLUMN TAIL", built by csrc/sparse_plan.cpp) on the CPU, for
every pattern of tests/sparse_zoo.py plus the headline model's pruned pattern and a pattern whose trailing block is not dense
(tests/sparse_tail_patterns.py).  tests/sparse_plan_tail_dump.cpp -- a stand-alone program of sparse_plan.cpp + knobs.cpp -- prints
the layout; that the schedules are VALID (dependencies, per-target order, masks, bit-identical solutions) is what
tests/test_sparse_plan_host.py checks with tests/sparse_plan_check.cpp on the same planner.

The tail units are ordinary units under that checker's rules: the c slots of a unit occupy the leading ceil(c / 2) lanes, both
halves, wherever the bank-aware placement puts them, and the value load is masked to those lanes.  A layout with row r in lane
r - c0, half 0 (one column spread over up to 49 lanes) cannot satisfy that rule -- a unit with one slot must have it in lane 0 --
so a reader that wants the tail by (row, column) goes through the plan's map `ftpos` instead, and this test pins that map.

TODAY: funits of the schedules of the commit before the tail was introduced (the list scheduler alone), measured once with that
commit's sparse_plan.cpp through tests/sparse_plan_check.cpp; the new layout may never need more units."""
import json
import os
import shutil
import struct
import subprocess

import pytest

import sparse_tail_patterns as TP
import sparse_zoo as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smooth_feedback_amd", "csrc")
TAIL_MAX = 48  # SparsePlanHost::kSweepTailMax

TODAY = {"clique53": 56, "clique54": 56, "clique62": 64, "clique63": 64, "clique64": 64, "clique100": 104, "chain8125": 8128,
         "chain8127": 8128, "chain8189": 8192, "chain8191": 8192, "chain399": 400, "arrow800": 800, "blockdiag400": 8, "rand200": 80,
         "tiny2": 8, "emptyrow": 8, "mpc6_10_pruned": 48, "mpc6_10_pruned.fallback": 88, "headline": 168}
EXTRA = ("twoclique60", "headline")


@pytest.fixture(scope="module")
def layouts(tmp_path_factory, sfb):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("sparse_plan_tail")
    exe, zoo = str(tmp / "sparse_plan_tail_dump"), str(tmp / "zoo.bin")
    srcs = [os.path.join(ROOT, "tests", "sparse_plan_tail_dump.cpp"), os.path.join(CSRC, "sparse_plan.cpp"), os.path.join(CSRC, "knobs.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off"] + srcs + ["-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    entries = Z.file_entries()
    with open(zoo, "wb") as f:
        f.write(b"SFBZOO1\0" + struct.pack("<i", len(entries) + len(EXTRA)))
        for name, z, Ap, Aj, Ax, chain in entries:
            f.write(Z._entry_bytes(name, z, Aj, Ap, Ax, chain))
        for name in EXTRA:
            f.write(TP.zoo_entry_bytes(name))
    run = subprocess.run([exe, zoo], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    out = {}
    for ln in run.stdout.splitlines():
        d = json.loads(ln)
        out[d["name"]] = d
    assert set(out) == set(TODAY) | set(EXTRA)
    return out


def test_tail_units_hold_one_column_each_in_ascending_order(layouts):
    with_tail = 0
    for name, d in layouts.items():
        k, T, t0 = d["k"], d["ftail"], d["ftail0"]
        print("%-26s k %5d funits %5d ftail0 %5d ftail %2d" % (name, k, d["funits"], t0, T))
        assert d["funits"] % 8 == 0 and t0 % 8 == 0 and T % 8 == 0 and 0 <= T <= TAIL_MAX
        if T == 0:
            assert t0 == 0 and d["tail"] == []
            continue
        with_tail += 1
        assert d["idx_scale"] == 8 and T <= k - 1 and t0 + T == d["funits"]      # the tail ends the schedule
        c0 = k - 1 - T
        assert len(d["tail"]) == T and len(d["lcols"]) == T + 1 and d["lcols"][T] == 0
        for i, (unit, pos) in enumerate(zip(d["tail"], d["ftpos"])):
            piv = c0 + i                                                        # consecutive pivots c0 .. k - 2
            assert len(unit) == d["lcols"][i] == d["counts"][t0 + i], (name, i)  # the whole column, nothing else
            rows = sorted(s[0] for s in unit)
            assert all(s[1] == piv for s in unit) and len(set(rows)) == len(rows)
            assert all(piv < r <= k - 1 for r in rows)
            lanes = max(1, (len(unit) + 1) // 2)
            want = [-1] * 64
            for r, _, lane, half in unit:
                assert 0 <= lane < lanes and half in (0, 1)                      # leading lanes, as in every unit
                want[r - c0] = lane * 2 + half
            assert pos == want, (name, i)                                        # the map of the register tail
    assert with_tail >= 10


def test_the_layout_never_needs_more_units_than_the_list_scheduler(layouts):
    for name, today in TODAY.items():
        assert layouts[name]["funits"] <= today, (name, layouts[name]["funits"], today)


def test_which_plans_have_a_tail(layouts):
    d = layouts
    assert (d["headline"]["funits"], d["headline"]["ftail0"], d["headline"]["ftail"]) == (168, 120, 48)
    assert d["headline"]["lcols"][:3] == [24, 35, 34] and d["headline"]["lcols"][24:26] == [12, 23]   # (dense: 48, 47, 46 ...) not dense
    assert d["mpc6_10_pruned"]["ftail"] == 8 and d["mpc6_10_pruned"]["ftail0"] == 40   # the smallest tail
    assert d["clique53"]["ftail"] == TAIL_MAX and d["clique53"]["lcols"][:-1] == list(range(48, 0, -1))   # dense
    assert d["arrow800"]["ftail"] == TAIL_MAX
    two = d["twoclique60"]
    assert two["ftail"] == TAIL_MAX and two["lcols"][0] == 38 and two["lcols"][28:30] == [10, 19]   # dense would be 48 and 20, 19: the columns up to 39 lack the rows 50 .. 59
    for name in ("tiny2", "blockdiag400", "chain8191"):                          # too small / would cost units / element indices
        assert d[name]["ftail"] == 0, name
    assert d["chain8191"]["idx_scale"] == 1
