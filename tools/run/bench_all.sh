#!/bin/bash
# GPU box: the RCCL / two-rank tests, then the default bench line (all legs)
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/out}          # where logs and traces go
export OUT
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests/test_gpu_rccl.py -x -q > $OUT/rccl_t.log 2>&1; rc=$?
tail -30 $OUT/rccl_t.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 900 python bench.py --full > $OUT/bench_default.log 2>&1; rc=$?
tail -c 6000 $OUT/bench_default.log
exit $rc
