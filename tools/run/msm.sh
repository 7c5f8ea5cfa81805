#!/bin/bash
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/out}          # where logs and traces go
export OUT
mkdir -p $OUT
timeout -k 10 600 python -m pytest tests/test_gpu_msm.py tests/test_gpu_api.py -x -q > $OUT/t.log 2>&1; rc=$?; tail -5 $OUT/t.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/b.log 2>&1 || { tail -20 $OUT/b.log; exit 1; }
tail -1 $OUT/b.log | cut -c1-200
