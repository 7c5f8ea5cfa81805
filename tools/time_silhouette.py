"""Silhouette samples at trajectory scale: msm_silhouette_samples against the single-launch msm_silhouette at the one
shape both take (200 000 x 10, k = 20), alternating, HIP-event timings; then one run each at 1 M x 10 with k = 20
and k = 500.  Labels come from a short k-means fit.  flops = (3 d + 3) per pair: sub and fma per feature; sqrt, add
and the share of the division per pair.

Usage: python tools/time_silhouette.py [n_shared] [n_large]     (n_large = 0 skips the large runs)"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmarlo_amd.device import get_engine  # noqa: E402
from tests import _gen  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12   # MI355X, vector fp64 FLOP/s (spec)


def timed_ms(eng, fn):
    a = eng.event().record()
    out = fn()
    b = eng.event().record()
    eng.sync()
    return a.elapsed_ms(b), out


def rate(n, d, ms):
    pairs = float(n) * float(n)
    return f"{pairs / ms / 1e9:7.1f} G pairs/s, {(3 * d + 3) * pairs / ms / 1e9:6.2f} TFLOP/s fp64 = " \
           f"{100 * (3 * d + 3) * pairs / (ms * 1e-3) / FP64_VECTOR_PEAK:4.1f} % of the vector peak"


def labelled(eng, n, d, k):
    X = _gen.correlated_series(n, d, seed=1000).astype(np.float64)
    xd = eng.to_device(X)
    centers, _ = eng.kmeans_fit(xd, k, seed=0, max_iter=10)
    return X, xd, eng.kmeans_assign(xd, centers)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    n_large = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    d, k = 10, 20
    eng = get_engine()
    X, xd, lab = labelled(eng, n, d, k)
    h_lab = lab.to_host()
    order = np.argsort(h_lab, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(h_lab, minlength=k))])
    xs = eng.to_device(X[order])
    new = lambda: eng.silhouette_samples(xd, lab, k)          # noqa: E731
    old = lambda: eng.silhouette(xs, offsets)                  # noqa: E731
    (s_new, v_new), (s_old, v_old) = new(), old()              # warm-up, and the two must agree
    diff = float(np.abs(v_new.to_host()[order] - v_old.to_host()).max())
    print(f"n = {n}, d = {d}, k = {k}: score {s_new:.15f} (samples) vs {s_old:.15f} (single launch), "
          f"max |s_i difference| = {diff:.2e}", flush=True)
    t_new, t_old = [], []
    for _ in range(5):
        t_new.append(timed_ms(eng, new)[0])
        t_old.append(timed_ms(eng, old)[0])
    for name, t in (("msm_silhouette_samples", t_new), ("msm_silhouette        ", t_old)):
        print(f"  {name}  median {np.median(t):9.2f} ms  (min {min(t):.2f}, max {max(t):.2f}; 5 runs, alternating)  "
              f"{rate(n, d, float(np.median(t)))}", flush=True)
    if n_large <= 0:
        return
    for k in (20, 500):
        _, xd, lab = labelled(eng, n_large, d, k)
        cut, v_cut = eng.silhouette_samples(xd, lab, k, max_products=1 << 32)     # the warm-up run, cut 16 times finer
        ms, (score, v) = timed_ms(eng, lambda: eng.silhouette_samples(xd, lab, k))
        same = cut == score and v_cut.to_host().tobytes() == v.to_host().tobytes()
        print(f"n = {n_large}, d = {d}, k = {k}: {ms / 1e3:8.3f} s (one run after one warm-up run), score {score:.6f}, "
              f"same bytes under a 2^32 cut: {same}  {rate(n_large, d, ms)}", flush=True)


if __name__ == "__main__":
    main()
