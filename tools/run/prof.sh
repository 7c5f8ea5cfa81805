#!/bin/bash
# GPU box: rocprofv3 kernel trace of the bench (outputs under $OUT/prof)
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/out}          # where logs and traces go
export OUT
mkdir -p $OUT && cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_bench.log 2>&1
tail -1 $OUT/prof_bench.log | cut -c1-300
find $OUT/prof -name "*kernel_stats.csv" | head
