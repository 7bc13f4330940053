#!/bin/bash
# Alternating runs of the headline command (bench.py --gpus 1) with several builds of libschwz_hip.so in one visit
# (the protocol of profiles/r07_cg_driver_ab.txt): ROUNDS rounds, one run per library and round, then per library the
# median, the fastest and the slowest run.
#   ROUNDS=7 LIBS="parent=/path/to/parent/libschwz_hip.so new=schwarz-lib_amd/lib/libschwz_hip.so" bash tools/bench_ab.sh [bench.py arguments]
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/out/bench_ab.txt}
mkdir -p "$(dirname $OUT)"
: > $OUT
for i in $(seq ${ROUNDS:-7}); do
    for E in $LIBS; do
        name=${E%%=*}; F=${E#*=}; case $F in /*) ;; *) F=$ROOT/$F;; esac
        line=$(SCHWZ_HIP_LIB=$F timeout -k 10 300 python3 $ROOT/bench.py --gpus 1 --steps ${STEPS:-30} --warmup ${WARMUP:-3} "$@" 2>/dev/null) || { echo "bench.py failed with $F"; exit 1; }
        echo "$name $(echo "$line" | python3 -c 'import json,sys; print("%.4f" % json.loads(sys.stdin.read())["ms_per_step"])')" >> $OUT
    done
done
python3 - $OUT <<'EOF'
import sys, statistics
runs = {}
for l in open(sys.argv[1]):
    k, v = l.split()
    runs.setdefault(k, []).append(float(v))
for k, v in runs.items():
    print("  %-8s median %.4f  min %.4f  max %.4f   runs %s" % (k, statistics.median(v), min(v), max(v), " ".join("%.4f" % t for t in v)))
EOF
