#!/bin/bash
# Launch timeline of the walk kernels (tools/walk_timeline.py) for one or more measurement builds:
#   make -C schwarz-lib_amd variant NAME=stamp DEFS=-DSCHWZ_WITH_PROBES
#   LIBS="libschwz_hip_stamp.so" bash tools/walk_timeline.sh
# Per library: a rocprofv3 --kernel-trace run of the solves (kernel durations), then the stamped run on its own.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/out/walk_timeline}
mkdir -p $OUT
for L in ${LIBS:-libschwz_hip_stamp.so}; do
    export SCHWZ_HIP_LIB=$ROOT/schwarz-lib_amd/lib/$L
    T=$OUT/trace_${L%.so}
    rm -rf $T
    timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d $T -- python3 $ROOT/tools/walk_timeline.py --no-stamps --solves 6 > $OUT/trace_${L%.so}.log 2>&1 || exit 1
    timeout -k 10 240 python3 $ROOT/tools/walk_timeline.py --solves ${SOLVES:-3} --trace $T 2> $OUT/stamps_${L%.so}.err | tee $OUT/timeline_${L%.so}.txt || exit 2
done
