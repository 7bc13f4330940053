#!/bin/bash
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=${OUT:-$ROOT/out}
mkdir -p $OUT
python -m pytest tests/ -x -q -m gpu > $OUT/r03_gputests_j.txt 2>&1
echo "pytest rc=$?"
tail -3 $OUT/r03_gputests_j.txt
python3 $ROOT/bench.py --full > $OUT/r03_bench_j.json 2> $OUT/r03_bench_j.err
echo "bench rc=$?"
