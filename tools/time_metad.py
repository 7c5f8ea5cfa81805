"""Metadynamics kernels at scale: msm_metad_bias at n = 1 M frames, H = 10 000 hills, d = 2 (value only, then with the
gradient; HIP events, one warm-up call, median of 7), and msm_metad_grid_scan at G = 300 x 300, H = 10 000, with
M = H + 1 checkpoints and with one (wall clock around the call, which waits for the stream itself; median of 4).  One
frame against all H hills, the MD step of MetadynamicsCVBias, value and gradient (HIP events around 20 calls).
Beside each time: the distance tests and the exp calls actually executed (counted on the host from the same inputs: a
test per frame-hill pair the frame sees, an exp per pair inside the cutoff; the scan adds two exps per grid point and
checkpoint), and the numpy restatement (tests/_metad_ref.py) on a slice, scaled.
The hills follow a random walk in [-1.5, 1.5] x [-0.5, 2.5] with sigma = 0.1, as a metadynamics run deposits them; the
frames see the hills deposited before them (count = frame index * H / n).
Usage: python tools/time_metad.py [--once]"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmarlo_amd.device import get_engine  # noqa: E402
from tests import _metad_ref as R  # noqa: E402


def main():
    once = "--once" in sys.argv
    n, H, d = 1_000_000, 10_000, 2
    rng = np.random.default_rng(0)
    lo, hi = np.array([-1.5, -0.5]), np.array([1.5, 2.5])
    walk = np.cumsum(rng.normal(scale=0.03, size=(n, d)), axis=0)
    u = (walk + 0.5 * (hi - lo)) % (2 * (hi - lo))
    cv = np.ascontiguousarray(lo + np.where(u > hi - lo, 2 * (hi - lo) - u, u))      # reflected into the box
    centers = cv[(np.arange(H) * (n // H))]
    packed = R.pack(centers, 0.1, 0.5)
    counts = (np.arange(n) // (n // H)).astype(np.int32)
    eng = get_engine()
    cvd, hills, cd = eng.to_device(cv), eng.to_device(packed), eng.to_device(counts)
    bias, grad = eng.empty((n,), np.float64), eng.empty((n, d), np.float64)

    def timed(call):
        ts = []
        for _ in range(1 if once else 8):
            a, b = eng.event(), eng.event()
            a.record()
            call()
            b.record()
            eng.sync()
            ts.append(a.elapsed_ms(b))
        return float(np.median(ts[1:] or ts))

    out = {"n": n, "H": H, "d": d, "plan": eng.metad_plan(n, H, d)}
    kw = dict(kernel="stretched-gaussian", counts=cd, bias=bias)
    out["bias_value_ms"] = timed(lambda: eng.metad_bias(cvd, hills, H, **kw))
    out["bias_value_grad_ms"] = timed(lambda: eng.metad_bias(cvd, hills, H, grad=True, grad_out=grad, **kw))
    one, b1, g1 = cvd.view((1, d), offset_elems=(n - 1) * d), eng.empty((1,), np.float64), eng.empty((1, d), np.float64)

    def md_steps():
        for _ in range(20):
            eng.metad_bias(one, hills, H, kernel="stretched-gaussian", grad=True, bias=b1, grad_out=g1)

    out["one_frame_value_grad_ms"] = timed(md_steps) / 20
    # executed work: a workgroup walks the hills up to its largest count, a lane tests the hills up to its own
    m = 500
    rows = np.linspace(0, n - 1, m).astype(np.int64)
    t0 = time.perf_counter()
    ref = R.bias(cv[rows], packed, counts[rows], kernel="stretched-gaussian")
    out["numpy_bias_ms_scaled_to_n"] = (time.perf_counter() - t0) * 1e3 * n / m
    term = R.hill_terms(cv[rows], packed, kernel="stretched-gaussian")[0]
    seen = np.arange(H)[None, :] < counts[rows][:, None]
    out["distance_tests"] = float(counts.astype(np.float64).sum())
    out["exp_calls"] = float(((term != 0) & seen).sum() * (n / m))
    out["max_abs_diff_vs_numpy_on_slice"] = float(np.max(np.abs(bias.to_host()[rows] - ref["bias"])))

    bins = np.array([300, 300], np.int32)
    glo, step, gb = R.grid_spec(lo, hi, bins)
    ck = np.arange(H + 1, dtype=np.int32)

    def scan():
        eng.metad_grid_scan(hills, H, glo, step, gb, ck, 1.0, 0.0, kernel="stretched-gaussian")

    t0 = time.perf_counter()
    scan()
    out["scan_first_call_wall_ms"] = (time.perf_counter() - t0) * 1e3
    ts = []
    for _ in range(1 if once else 4):
        t0 = time.perf_counter()
        scan()                      # the call waits for the stream itself (heights check, table upload)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["scan_wall_ms"] = float(np.median(ts))
    ck1 = np.array([H], np.int32)
    ts = []
    for _ in range(1 if once else 4):
        t0 = time.perf_counter()
        eng.metad_grid_scan(hills, H, glo, step, gb, ck1, 1.0, 0.0, kernel="stretched-gaussian")
        ts.append((time.perf_counter() - t0) * 1e3)
    out["scan_one_checkpoint_wall_ms"] = float(np.median(ts))
    G = int(np.prod(bins))
    pts = R.grid_points(glo, step, gb)
    sub = pts[:: max(1, G // 1500)]
    inside = float((R.hill_terms(sub, packed, kernel="stretched-gaussian")[0] != 0).sum()) * G / sub.shape[0]
    out["scan_distance_tests"] = float(G) * H
    out["scan_exp_calls"] = inside + 2.0 * G * (H + 1)
    t0 = time.perf_counter()
    R.scan(packed[:50], glo, step, gb, np.arange(51), 1.0, 0.0, kernel="stretched-gaussian")
    out["numpy_scan_ms_scaled_to_H"] = (time.perf_counter() - t0) * 1e3 * H / 50
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
