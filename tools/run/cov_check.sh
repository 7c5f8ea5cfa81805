#!/bin/bash
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/out}          # where logs and traces go
export OUT
mkdir -p $OUT
timeout -k 10 180 python -m pytest tests/test_gpu_tica.py tests/test_gpu_configs.py -x -q > $OUT/cov_t.log 2>&1; rc=$?
tail -5 $OUT/cov_t.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 120 python tools/time_kernels.py 2>&1 | grep -E "lagged_moments|project|tica_solve" || exit 1
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/pmc_cov
timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_cov -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extra-legs > $OUT/pmc_cov.log 2>&1 || { tail -3 $OUT/pmc_cov.log; exit 1; }
cd $R && python tools/pmc_summary.py $OUT/pmc_cov | grep -E "cov_fused|kernel \|" | cut -c1-200
