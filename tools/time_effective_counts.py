"""Effective counts at the C4 shape (k = 200 microstates, 1e5 frames, lags 1 / 10 / 50): device time of
Engine.effective_counts vs the numpy / Python-int restatement the tests use (tests/_effective_ref.py), on the same
box.  Usage: python tools/time_effective_counts.py [k] [frames]"""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmarlo_amd.device import get_engine  # noqa: E402
from tests import _effective_ref as R  # noqa: E402
from tools.time_its import chain  # noqa: E402


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
    eng = get_engine()
    trajs = [chain(k, n // 4, s) for s in range(4)]
    labels = np.concatenate(trajs).astype(np.int32)
    lens = np.array([len(t) for t in trajs], np.int64)
    stops = np.cumsum(lens)
    starts = stops - lens
    d_labels = eng.to_device(labels)
    eng.effective_counts(d_labels, k, 1, starts=starts, stops=stops)   # warm-up
    for lag in (1, 10, 50):
        eng.sync()
        t0 = time.perf_counter()
        ceff, si, C, trunc = eng.effective_counts(d_labels, k, lag, starts=starts, stops=stops)
        eng.sync()
        dev = time.perf_counter() - t0
        launches = eng.last_effective_launches
        t0 = time.perf_counter()
        want = R.effective_reference(trajs, k, lag)
        host = time.perf_counter() - t0
        C_h, trunc_h = C.to_host(), trunc.to_host()
        same = np.array_equal(C_h, want[2]) and np.array_equal(trunc_h, want[3])
        err = np.max(np.abs(ceff.to_host() - want[0]) / np.maximum(want[0], 1e-300), where=want[0] > 0, initial=0.0)
        print(f"lag {lag:3d} k={k} n={labels.size}: device {dev * 1e3:9.2f} ms ({launches} inefficiency launch(es)), "
              f"host restatement {host * 1e3:9.1f} ms; cells {np.count_nonzero(C_h)}, largest truncation lag "
              f"{trunc_h.max()}, integers equal: {same}, max rel. difference of Ceff {err:.2e}", flush=True)


if __name__ == "__main__":
    main()
