#!/bin/bash
# The driver's N = 1 bench line (--full: with the roofline, the gmres() call and the CPU baseline) and the
# rocprofv3 --kernel-trace --stats summary of the same command (profiles/rNN/).
# usage: bench_profile.sh TAG      -> $OUT/bench_TAG.json, $OUT/bench_TAG_kernel_stats.csv (OUT defaults to build/profile)
TAG=${1:-r03}
OUT=${OUT:-build/profile}
mkdir -p "$OUT"
cd /tmp 2>/dev/null && export TMPDIR=/tmp && cd - >/dev/null
python3 bench.py --full --steps 8 --warmup 2 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -5 $OUT/bench_$TAG.err; exit 1; }
rm -rf $OUT/prof_$TAG
rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -- python3 bench.py --full --steps 4 --warmup 1 --no-cpu-baseline > $OUT/bench_${TAG}_profiled.json 2> $OUT/bench_${TAG}_profiled.err
DB=$(find $OUT/prof_$TAG -name "*_results.db" | head -1)
python3 profiles/tools/kernel_stats_from_db.py "$DB" $OUT/bench_${TAG}_kernel_stats.csv
rm -rf $OUT/prof_$TAG
python3 - <<PY
import json
d = json.load(open("$OUT/bench_$TAG.json"))
print({k: d[k] for k in ("value", "ms_per_step", "n_gpus")}, d["gmres_call"]["value"], d["config"]["setup_seconds"])
r = d["roofline"]
print(r["kernel"], r["achieved"], r["frac"], r["traffic"], r["measured_streams"], r.get("reference_ordering"))
print({k: (v["achieved"], v["kernel"]) for k, v in r["single_operators"].items()})
PY
