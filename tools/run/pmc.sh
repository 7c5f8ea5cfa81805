#!/bin/bash
# GPU box: HBM-side byte counters of the bench kernels.  FETCH_SIZE (3 TCC slots) and WRITE_SIZE
# (2 slots) do not fit one pass: two runs, --pmc with --kernel-trace only.
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/out}          # where logs and traces go
export OUT
mkdir -p $OUT && cd /tmp && export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/pmc_$c
  timeout -k 10 240 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/pmc_$c -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/pmc_$c.log 2>&1 || { tail -5 $OUT/pmc_$c.log | cut -c1-300; exit 1; }
  echo "$c done"
done
find $OUT/pmc_* -name "*.csv" | head
