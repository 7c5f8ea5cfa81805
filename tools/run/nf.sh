#!/bin/bash
# GPU box: k-means parity tests and a bench line (used when trying kernel variants)
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/out}          # where logs and traces go
export OUT
mkdir -p $OUT
timeout -k 10 400 python -m pytest tests/test_gpu_kmeans.py tests/test_gpu_kmeans_fit.py tests/test_gpu_configs.py -x -q 2>&1 | tail -3 || exit 1
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/b_nf.log 2>&1 || { tail -5 $OUT/b_nf.log; exit 1; }
python - <<'PY'
import json
import os
o = json.loads([l for l in open(os.path.join(os.environ["OUT"], "b_nf.log")) if l.startswith("{")][-1])
print(o["ms_per_step"], o["value"] / 1e6, o["roofline"]["launch_ms"], o["roofline"]["frac"], o["parity"]["counts_bit_exact"],
      o["parity"]["labels_bit_exact_given_centres"])
PY
