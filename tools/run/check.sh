#!/bin/bash
# GPU box: full -m gpu suite, then a bench line and per-kernel timings (outputs under $OUT/)
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/out}          # where logs and traces go
export OUT
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/t.log 2>&1; rc=$?; tail -5 $OUT/t.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $OUT/b.log 2>&1 || { tail -20 $OUT/b.log; exit 1; }
tail -1 $OUT/b.log
timeout -k 10 120 python tools/time_kernels.py > $OUT/tk.log 2>&1; tail -30 $OUT/tk.log
