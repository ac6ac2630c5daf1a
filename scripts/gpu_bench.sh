#!/bin/bash
# the full bench line (headline + CPU baseline, parity, closed loop, secondary workloads) and a digest of it; files under $1
cd ${GRAFT_REPO_ROOT:-.}
OUT=${1:-bench_out}
mkdir -p $OUT
SECONDS=0; timeout 900 python bench.py --full 2> $OUT/bench_default.err | tail -1 > $OUT/bench_default.json; echo "bench.py wall $SECONDS s"
tail -3 $OUT/bench_default.err
python - $OUT/bench_default.json <<'PY'
import json, sys
r = json.load(open(sys.argv[1]))
def show(name, d):
    print(name, "value %.4g %s" % (d["value"], d["unit"]), "kernel_ms %.3f" % d["roofline"]["kernel_ms"], "frac %.3g" % d["roofline"]["frac"],
          "traffic", d["roofline"].get("traffic"), d["roofline"].get("traffic_source"), "alt", d.get("roofline_alt", {}).get("frac"))
    print("   cpu", {k: (v if not isinstance(v, dict) else v) for k, v in d.get("cpu_baseline", {}).items() if k != "sample"})
    print("   parity", d.get("parity_vs_oracle"))
show("headline", r)
for k, v in r.get("secondary", {}).items():
    if isinstance(v, dict) and "roofline" in v: show(k, v)
    else: print(k, json.dumps(v)[:1500])
print("pipelined", r.get("pipelined", {}).get("value"))
PY
