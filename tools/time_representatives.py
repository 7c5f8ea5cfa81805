"""Representative picking at the bench shape: 1 M frames x 10 features, k-means labels (k given on the command
line, default 500 then 100).  Per phase: one warm-up, then the median of 5 HIP-event timings.  Beside it the
numpy restatement (tests/_representatives_ref.py) on the host; its medoid is timed on a few states and scaled by
sum n_s^2, and says so.

Usage: python tools/time_representatives.py [n_frames] [k ...]"""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmarlo_amd import _lib  # noqa: E402
from pmarlo_amd.conformations import RepresentativePicker  # noqa: E402
from pmarlo_amd.conformations.representative_picker import DeviceStateGroups  # noqa: E402
from pmarlo_amd.device import get_engine  # noqa: E402
from tests import _gen, _representatives_ref as R  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12   # MI355X, vector fp64 FLOP/s (spec)


def med_ms(eng, fn, reps=5):
    fn()
    eng.sync()
    out = []
    for _ in range(reps):
        a, b = eng.event().record(), None
        fn()
        b = eng.event().record()
        eng.sync()
        out.append(a.elapsed_ms(b))
    return float(np.median(out))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    ks = [int(a) for a in sys.argv[2:]] or [500, 100]
    d = 10
    eng = get_engine()
    X = _gen.correlated_series(n, d, seed=1000).astype(np.float64)
    xd = eng.to_device(X)
    for k in ks:
        centers, _ = eng.kmeans_fit(xd, k, seed=0, max_iter=10)
        labels = eng.kmeans_assign(xd, centers).to_host()
        g = DeviceStateGroups(X, labels, k)
        sizes = np.diff(g.offsets)
        states = [s for s in range(k) if sizes[s] > 0]
        pairs = float(np.sum(sizes.astype(np.float64) ** 2))
        print(f"\nn = {n}, d = {d}, k = {k}: {len(states)} occupied states, n_s min / median / max = "
              f"{sizes.min()} / {int(np.median(sizes))} / {sizes.max()}, sum n_s^2 = {pairs:.3e}", flush=True)
        t_group = med_ms(eng, lambda: eng.group_by_label(g.labels, k))
        t_cen = med_ms(eng, lambda: eng.state_centroids(g.x, g.d_offsets, g.members, None))
        t_cs = med_ms(eng, g.centroid_scores)
        t_med = med_ms(eng, lambda: g.medoid_scores(states))
        launches = 0
        first, tot = True, 0
        for s in states:   # the launch cut of msm_state_scores: 2^36 (i, j, feature) products per launch
            for i0 in range(0, int(sizes[s]), _lib.REP_TILE_I):
                c = _lib.REP_TILE_I * int(sizes[s]) * d
                if first or tot + c > (1 << 36):
                    launches, tot, first = launches + 1, 0, False
                tot += c
        flops = 3.0 * d * pairs + 3.0 * pairs   # sub, fma per feature; sqrt, mul, add per pair
        print(f"  group_by_label      {t_group:9.3f} ms")
        print(f"  state_centroids     {t_cen:9.3f} ms")
        print(f"  centroid scores     {t_cs:9.3f} ms")
        print(f"  medoid scores       {t_med:9.3f} ms   {launches} launches, {flops / t_med / 1e9:8.2f} TFLOP/s fp64 = "
              f"{100 * flops / (t_med * 1e-3) / FP64_VECTOR_PEAK:5.1f} % of the vector peak (sub + fma count 3 of the 4 "
              f"flops two FMAs would)")
        cs, ms = g.centroid_scores(), g.medoid_scores(states)
        for n_reps in (1, 5):
            t_a = med_ms(eng, lambda: g.select(cs, states, n_reps))
            t_b = med_ms(eng, lambda: g.select(ms, states, n_reps))
            t_c = med_ms(eng, lambda: g.select(cs, states, n_reps, diverse=True))
            print(f"  select n_reps = {n_reps}:  smallest (centroid) {t_a:8.3f} ms   smallest (medoid) {t_b:8.3f} ms   "
                  f"diverse {t_c:8.3f} ms")
        picker = RepresentativePicker()
        for method in R.METHODS:
            for n_reps in (1, 5):
                t0 = time.perf_counter()
                picker.pick_representatives(X, [labels], states, n_reps=n_reps, method=method)
                print(f"  pick_representatives {method:20s} n_reps = {n_reps}: {1e3 * (time.perf_counter() - t0):9.1f} ms "
                      f"end to end (upload of {X.nbytes >> 20} MiB included)", flush=True)
        # the host restatement
        for method, n_reps in (("closest_to_centroid", 1), ("diverse", 5)):
            t0 = time.perf_counter()
            R.pick(X, [labels], states, None, n_reps, method)
            print(f"  numpy {method:20s} n_reps = {n_reps}: {1e3 * (time.perf_counter() - t0):9.1f} ms")
        sub = states[:: max(1, len(states) // 3)][:3]
        t0 = time.perf_counter()
        R.pick(X, [labels], sub, None, 1, "true_medoid")
        dt = time.perf_counter() - t0
        sub_pairs = float(np.sum(sizes[sub].astype(np.float64) ** 2))
        print(f"  numpy true_medoid on {len(sub)} states (sum n_s^2 = {sub_pairs:.3e}): {dt:.2f} s -> scaled by sum n_s^2 "
              f"to all states: {dt * pairs / sub_pairs:.1f} s (extrapolated)", flush=True)


if __name__ == "__main__":
    main()
