"""The dense route table (csrc/qp_dense_route.h) on the CPU: tests/dense_route_check.cpp -- a stand-alone program of the header
alone, built with AddressSanitizer and UBSan and run directly -- prints dense_route(k, time_limited, big_off) at every boundary
of the routing, and the whole table is compared with literals written from the rule:

    k <= 32 and no time limit                       Four
    otherwise k <= 128                              Mid
    otherwise k <= 1024 and SFB_QP_DENSE_BIG != 0   Big
    otherwise                                       FullPattern

No GPU, no libsfb.so.  Workspace bytes and launch of every route go through this one function (csrc/capi.hip)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smooth_feedback_amd", "csrc")

# k -> routes at (time_limited, big_off) = (0, 0), (0, 1), (1, 0), (1, 1)
EXPECTED = {
    1:     ("Four", "Four", "Mid", "Mid"),
    16:    ("Four", "Four", "Mid", "Mid"),
    17:    ("Four", "Four", "Mid", "Mid"),
    32:    ("Four", "Four", "Mid", "Mid"),
    33:    ("Mid", "Mid", "Mid", "Mid"),
    48:    ("Mid", "Mid", "Mid", "Mid"),
    64:    ("Mid", "Mid", "Mid", "Mid"),
    65:    ("Mid", "Mid", "Mid", "Mid"),
    128:   ("Mid", "Mid", "Mid", "Mid"),          # the knob does not move sizes up to 128
    129:   ("Big", "FullPattern", "Big", "FullPattern"),
    1024:  ("Big", "FullPattern", "Big", "FullPattern"),
    1025:  ("FullPattern", "FullPattern", "FullPattern", "FullPattern"),
    19198: ("FullPattern", "FullPattern", "FullPattern", "FullPattern"),
}


def test_route_table_at_every_boundary(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "dense_route_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(ROOT, "tests", "dense_route_check.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and any(lib in build.stderr for lib in ("-lasan", "-lubsan", "libasan", "libubsan")):
        pytest.skip("the sanitizer runtime does not link here")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    got = {}
    for line in run.stdout.split("\n"):
        if line:
            k, tl, bo, route = line.split()
            got[(int(k), int(tl), int(bo))] = route
    want = {(k, tl, bo): routes[2 * tl + bo] for k, routes in EXPECTED.items() for tl in (0, 1) for bo in (0, 1)}
    assert len(want) == 13 * 2 * 2 and got == want, {key: (got.get(key), want[key]) for key in want if got.get(key) != want[key]}
