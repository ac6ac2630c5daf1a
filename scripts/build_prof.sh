#!/bin/bash
# Profiling build of libsfb.so: the sparse kernel prints the cycles it spends in the phases of the numeric
# factorisation (SFB_PROF_LDL).  Use with SFB_LIB_PATH=smooth_feedback_amd/libsfb_prof.so scripts/ldl_prof.py
# PROF_DEFS=-DSFB_SP_TIMELINE: per-item wall-clock stamps instead (scripts/timeline.py)
# PROF_DEFS=-DSFB_PROF_CHECK: counters and cycles of the parts of a stopping check (scripts/check_prof.py); with
#   -DSFB_CHECK_FULL_PASSES the infeasibility passes run to their end (the check before the early exits; alone: an A/B build)
# PROF_OUT: name of the library (default libsfb_prof.so), PROF_DIR: its object directory (default build_prof)
set -e
cd "$(dirname "$0")/../smooth_feedback_amd/csrc"
make -s
D=${PROF_DIR:-build_prof}
mkdir -p "$D"
cp build/*.o "$D"/
FLAGS="--offload-arch=gfx950 -O3 -std=c++20 -fPIC -ffp-contract=off -fno-fast-math ${PROF_DEFS:--DSFB_PROF_LDL}"
/opt/rocm/bin/hipcc $FLAGS -c qp_sparse.hip -o "$D"/qp_sparse.o
# the same guard as the Makefile's: numbers from a build whose sweeps spill or touch in-flight registers mean nothing
/opt/rocm/bin/hipcc $FLAGS -S --cuda-device-only qp_sparse.hip -o "$D"/qp_sparse.s 2> /dev/null
python3 check_sweep_spills.py "$D"/qp_sparse.s > "$D"/qp_sparse.spills || (cat "$D"/qp_sparse.spills; rm -f "$D"/qp_sparse.o; false)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../"${PROF_OUT:-libsfb_prof.so}" "$D"/*.o -Wl,-rpath,/opt/rocm/lib
