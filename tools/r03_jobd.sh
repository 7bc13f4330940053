#!/bin/bash
# round 3: whole GPU suite, then the default bench line with its new legs
OUT=${OUT:-out}
mkdir -p $OUT
python -m pytest tests/ -x -q -m gpu > $OUT/r03_gputests_d.txt 2>&1
echo "pytest rc=$?" >> $OUT/r03_gputests_d.txt
tail -4 $OUT/r03_gputests_d.txt
( time python bench.py --full ) > $OUT/r03_bench_d.json 2> $OUT/r03_bench_d.err
echo "bench rc=$?"
tail -c 600 $OUT/r03_bench_d.err
