#!/bin/bash
# GPU box: every k-means / sharded-step test, then the k-means timings and a bench line
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/out}          # where logs and traces go
export OUT
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests/test_gpu_kmeans_filter.py tests/test_gpu_kmeans.py tests/test_gpu_kmeans_fit.py tests/test_gpu_configs.py tests/test_gpu_rccl.py tests/test_gpu_api.py -x -q > $OUT/t.log 2>&1; rc=$?; tail -8 $OUT/t.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python tools/time_kmeans_filter.py > $OUT/kmf_time.log 2>&1; tail -7 $OUT/kmf_time.log
timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extra-legs > $OUT/b.log 2>&1 || { tail -20 $OUT/b.log; exit 1; }
tail -1 $OUT/b.log | cut -c1-400; tail -1 $OUT/b.log | grep -o '"stages_ms": {[^}]*}'
