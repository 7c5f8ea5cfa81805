#!/usr/bin/env python3
"""Time msm_featurize_spec with HIP events: tools/time_featurize_spec.py [--small]

n = 1 M frames, A = 22 atoms, 45 distances + 3 angles + 2 dihedrals (F = 50 columns) into one [n, 50] matrix:
  three   the three per-kind launches (msm_featurize_distances / _angles / _dihedrals) timed as one window: the path
          without this entry point
  fused   one msm_featurize_spec launch, no box, no record flagged; its output is compared bit for bit with `three`
  round   one launch, every record flagged, one box per frame, mic = round
  search  the same with mic = search (27 images for every bond vector not provably the shortest already)
One warm-up, then the median of 7 windows each.  GB/s is the algorithmic traffic over the measured time: 12 A + 4 F
bytes per frame, plus 36 for the frame's box in the flagged runs.  --small runs 1/50 of the frames (a rehearsal, not
a measurement)."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from pmarlo_amd._lib import MIC_ROUND, MIC_SEARCH, check, lib  # noqa: E402
from pmarlo_amd.device import Engine  # noqa: E402

RUNS = 7
n, A = 1_000_000, 22
if "--small" in sys.argv:
    n //= 50


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


rng = np.random.default_rng(22)
base = np.cumsum(rng.standard_normal((A, 3)) * 0.12, axis=0).astype(np.float32)
xyz = np.empty((n, A, 3), np.float32)
for lo in range(0, n, 50_000):
    hi = min(n, lo + 50_000)
    xyz[lo:hi] = base + 0.03 * rng.standard_normal((hi - lo, A, 3), dtype=np.float32) + \
        rng.uniform(-3, 3, (hi - lo, 1, 3)).astype(np.float32)
ca = np.arange(0, A, 2)[:10]
pairs = np.array([(ca[i], ca[j]) for i in range(10) for j in range(i + 1, 10)], np.int32)
triplets = np.array([[0, 4, 8], [4, 8, 12], [8, 12, 16]], np.int32)
quads = np.array([[4, 6, 8, 14], [6, 8, 14, 16]], np.int32)
P, Tn, Q = len(pairs), len(triplets), len(quads)
F = P + Tn + Q
cells = np.tile([3.0, 3.2, 3.4, 80.0, 95.0, 70.0], (n, 1)) * (1.0 + 0.02 * rng.uniform(-1, 1, (n, 1)))
cells[:, 3:] = [80.0, 95.0, 70.0]

eng = Engine(0)
h = eng.handle
xd, box = eng.to_device(xyz), eng.box_from_cell(cells)
dp, dt, dq = eng.to_device(pairs), eng.to_device(triplets), eng.to_device(quads)
off = eng.feature_table(pairs=pairs, triplets=triplets, quads=quads, periodic=False)
on = eng.feature_table(pairs=pairs, triplets=triplets, quads=quads, periodic=True)
o3, o1 = eng.empty((n, F), np.float32), eng.empty((n, F), np.float32)


def three():
    check(lib.msm_featurize_distances(h, xd.ptr, n, A, dp.ptr, P, o3.ptr, F, 0), h)
    check(lib.msm_featurize_angles(h, xd.ptr, n, A, dt.ptr, Tn, o3.ptr, F, P), h)
    check(lib.msm_featurize_dihedrals(h, xd.ptr, n, A, dq.ptr, Q, 0, o3.ptr, F, P + Tn), h)


def spec(table, dbox, n_box, mic):     # the library call itself, as `three` makes them: no host-side checks in the window
    check(lib.msm_featurize_spec(h, xd.ptr, n, A, dbox, n_box, table.rec.ptr, table.param.ptr, F, F, mic, o1.ptr, F, 0), h)


t_three = timed(eng, three)
t_fused = timed(eng, lambda: spec(off, None, 0, MIC_ROUND))
same = bool(np.array_equal(o3.to_host(), o1.to_host()))
t_round = timed(eng, lambda: spec(on, box.ptr, n, MIC_ROUND))
t_search = timed(eng, lambda: spec(on, box.ptr, n, MIC_SEARCH))
finite = bool(np.isfinite(o1.to_host()).all())
plain, boxed = (12 * A + 4 * F) * n, (12 * A + 36 + 4 * F) * n
print(f"n = {n}, A = {A}, F = {F} ({P} distances, {Tn} angles, {Q} dihedrals); bytes: {plain} without boxes, {boxed} with")
for name, t, b in (("three", t_three, plain), ("fused", t_fused, plain), ("round", t_round, boxed),
                   ("search", t_search, boxed)):
    print(f"{name:>7} {t:9.1f} us {b / t / 1e3:7.0f} GB/s   x{t / t_three:5.2f} of three")
print(f"fused output bit-identical to the three launches: {same}; flagged output finite: {finite}")
eng.close()
