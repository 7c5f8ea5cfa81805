#!/usr/bin/env python3
"""Time msm_superpose with HIP events: tools/time_superpose.py [--small]

For (n, A, S) = (1 M, 22, 10), (1 M, 138, 10) and (20 000, 3350, 223): the launch with full output (24 A n bytes: xyz
read once, written once), the rmsd-only launch (12 S n bytes: the selected atoms alone) and msm_memcpy_d2d of the same
xyz buffer in the same process.  One warm-up, then the median of 7 runs each.  The copy is the yardstick: the
full-output launch moves exactly the copy's bytes, so its time over the copy's is the figure to read; the GB/s columns
are those byte counts over the measured times.  A fourth row, (2000, 6000, 6000), is the streamed launch (A above the LDS
limit) with every atom selected: the shape where one wave gathers for the whole workgroup.  --small runs 1/50 of the frames (a rehearsal, not a measurement)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from pmarlo_amd._lib import check, lib  # noqa: E402
from pmarlo_amd.device import Engine  # noqa: E402

SHAPES = [(1_000_000, 22, 10), (1_000_000, 138, 10), (20_000, 3350, 223), (2_000, 6000, 6000)]
RUNS = 7


def timed(eng, call):
    call()
    eng.sync()
    times = []
    for _ in range(RUNS):
        e0 = eng.event().record()
        call()
        e1 = eng.event().record()
        eng.sync()
        times.append(e0.elapsed_ms(e1) * 1e3)
    return float(np.median(times))


eng = Engine(0)
print(f"{'n':>8} {'A':>5} {'S':>4} | {'copy us':>9} {'GB/s':>7} | {'full us':>9} {'GB/s':>7} {'copy/full':>9} | "
      f"{'rmsd us':>9} {'GB/s':>7}")
for n, A, S in SHAPES:
    if "--small" in sys.argv:
        n = max(4, n // 50)
    rng = np.random.default_rng(A)
    base = rng.standard_normal((A, 3)).astype(np.float32)
    # one frame's worth of structure, jittered per frame on the host in slabs to keep the host side cheap
    xyz = np.empty((n, A, 3), np.float32)
    for lo in range(0, n, 50_000):
        hi = min(n, lo + 50_000)
        xyz[lo:hi] = base + 0.05 * rng.standard_normal((hi - lo, A, 3), dtype=np.float32) + \
            rng.uniform(-3, 3, (hi - lo, 1, 3)).astype(np.float32)
    sel = np.sort(rng.permutation(A)[:S]).astype(np.int32)
    xd, od = eng.to_device(xyz), eng.empty((n, A, 3), np.float32)
    sd, rd, md = eng.to_device(sel), eng.to_device(base[sel]), eng.empty((n,), np.float32)
    h = eng.handle
    t_copy = timed(eng, lambda: check(lib.msm_memcpy_d2d(h, od.ptr, xd.ptr, xd.nbytes), h))
    t_full = timed(eng, lambda: check(lib.msm_superpose(h, xd.ptr, n, A, sd.ptr, S, rd.ptr, od.ptr, md.ptr), h))
    t_rmsd = timed(eng, lambda: check(lib.msm_superpose(h, xd.ptr, n, A, sd.ptr, S, rd.ptr, None, md.ptr), h))
    full_b, rmsd_b = 24 * A * n, 12 * S * n
    print(f"{n:>8} {A:>5} {S:>4} | {t_copy:9.1f} {full_b / t_copy / 1e3:7.0f} | {t_full:9.1f} {full_b / t_full / 1e3:7.0f} "
          f"{t_copy / t_full:9.2f} | {t_rmsd:9.1f} {rmsd_b / t_rmsd / 1e3:7.0f}")
    print(f"         bytes: full {full_b} (24 A n), rmsd-only {rmsd_b} (12 S n); rmsd[0..2] = {md.to_host()[:3]}")
    for a in (xd, od, sd, rd, md):
        a.free()
eng.close()
