#!/usr/bin/env python3
"""Time msm_autocorr_lagscan with HIP events: tools/time_autocorr.py [n] [F] [f64|f32] [n_seg] [--host]

The lags are the ten that derive_taus gives for one split of n frames.  Prints the median over the timed calls,
the algorithmic traffic (3 passes over X for means, variances and the tile itself, plus one partner pass per lag
that is longer than a tile) and what fraction of the 8 TB/s HBM peak that is.  --host also times the numpy
restatement of the same passes (tests/_diagnostics_ref.py, float64 sums) on this machine's CPU."""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from pmarlo_amd.analysis.diagnostics import derive_taus  # noqa: E402
from pmarlo_amd.device import Engine  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 1_000_000
F = int(args[1]) if len(args) > 1 else 10
dtype = np.float32 if len(args) > 2 and args[2] == "f32" else np.float64
n_seg = int(args[3]) if len(args) > 3 else 1
rng = np.random.default_rng(0)
x = np.cumsum(rng.standard_normal((n, F)), axis=0).astype(dtype)
lags = derive_taus([n // n_seg])
stops = (np.arange(1, n_seg + 1) * (n // n_seg)).astype(np.int64)
starts = stops - n // n_seg
tile_rows = 4096 // F
far = sum(1 for t in lags if t >= tile_rows)
eng = Engine(0)
xd = eng.to_device(x)
for _ in range(3):
    eng.autocorr_lagscan(xd, lags, starts=starts, stops=stops)
eng.sync()
times = []
for _ in range(20):
    e0, e1 = eng.event().record(), None
    out = eng.autocorr_lagscan(xd, lags, starts=starts, stops=stops)
    e1 = eng.event().record()
    times.append(e0.elapsed_ms(e1))
ms = float(np.median(times))
traffic = (3 + far) * x.nbytes
print(f"autocorr_lagscan n={n} F={F} {np.dtype(dtype).name} n_seg={n_seg} lags={lags}")
print(f"  median {ms * 1e3:.1f} us (min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f}) over 20 calls")
print(f"  algorithmic traffic (3 + {far} far lags) x {x.nbytes / 1e6:.0f} MB = {traffic / 1e6:.0f} MB "
      f"-> {traffic / ms / 1e9:.2f} TB/s = {traffic / ms / 1e9 / 8.0:.2f} of the 8 TB/s HBM peak")
print("  values[0] =", out[0].to_host()[0])
if "--host" in sys.argv:
    from tests._diagnostics_ref import autocorr_lagscan_ref
    t0 = time.perf_counter()
    ref, _ = autocorr_lagscan_ref(x, starts, stops, lags, acc=np.float64)
    print(f"  numpy restatement on this host: {time.perf_counter() - t0:.3f} s; max |device - numpy| = "
          f"{np.nanmax(np.abs(ref - out[0].to_host())):.2e}")
eng.close()
