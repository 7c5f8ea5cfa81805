#!/bin/bash
# GPU box: round-2 evidence.  (1) kernel trace + stats of the bench step, (2) HBM-side byte counters (two passes:
# FETCH_SIZE and WRITE_SIZE do not fit one), (3) matrix-pipe / LDS counters.  --pmc only ever with --kernel-trace.
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/out}          # where logs and traces go
export OUT
mkdir -p $OUT && cd /tmp && export TMPDIR=/tmp
BENCH="python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-extra-legs"
rm -rf $OUT/prof_r02 $OUT/pmc_r02_*
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_r02 -- $BENCH > $OUT/prof_r02_bench.log 2>&1 || { tail -5 $OUT/prof_r02_bench.log | cut -c1-300; exit 1; }
tail -1 $OUT/prof_r02_bench.log | cut -c1-200
rocprofv3 -L > $OUT/counters.txt 2>&1
pick() { for c in "$@"; do grep -q -w "$c" $OUT/counters.txt && printf "%s " "$c"; done; }
SETS=("FETCH_SIZE" "WRITE_SIZE" "$(pick SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_ACTIVE_INST_LDS GRBM_GUI_ACTIVE)" "$(pick SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_VALU_MFMA_COEXEC_CYCLES)")
i=0
for s in "${SETS[@]}"; do
  [ -z "$s" ] && continue
  echo "pmc set $i: $s"
  timeout -k 10 300 rocprofv3 --pmc $s --kernel-trace --output-format csv -d $OUT/pmc_r02_$i -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extra-legs > $OUT/pmc_r02_$i.log 2>&1 || { echo "set $i failed"; tail -3 $OUT/pmc_r02_$i.log | cut -c1-300; }
  i=$((i+1))
done
find $OUT/prof_r02 $OUT/pmc_r02_* -name "*.csv" | head -20
