"""MBAR at N = 1 M frames, K = 32 rungs, fp64: the time of one msm_mbar_pass with and without the Gram update (HIP
events around the two launches, two warm-up calls, 7 timed), the full solve of reweight.mbar (wall clock, one warm-up,
5 timed) and the numpy restatement's pass (tests/_mbar_ref.py) on the same box; beside them the byte floor
K N 8 + 8 N at the 8 TB/s HBM peak.  Usage: python tools/time_mbar.py [top temperature of the ladder, default 330]"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmarlo_amd import reweight  # noqa: E402
from pmarlo_amd._lib import MSM_F64, check, lib  # noqa: E402
from pmarlo_amd.device import get_engine  # noqa: E402
from tests import _mbar_ref as R  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    K, n_per = 32, 1_000_000 // 32
    top = float(sys.argv[1]) if len(sys.argv) > 1 else 330.0
    T = np.linspace(300.0, top, K)
    E, _ = R.ladder_energies(np.random.default_rng(0), T, n_per)
    N = E.size
    eng = get_engine()
    u = eng.mbar_reduced_potentials(eng.to_device(E), 1.0 / (R.KB * T))
    N_k = np.full(K, n_per, np.int64)
    lnN = eng.to_device(np.log(N_k.astype(np.float64)))
    out = {"K": K, "N": N, "ladder_K": [300.0, top], "plan": eng.mbar_plan(K, N)}

    solves = []
    for _ in range(6):
        eng.sync()
        t0 = time.perf_counter()
        res = reweight.mbar(u, N_k, engine=eng)
        eng.sync()
        solves.append((time.perf_counter() - t0) * 1e3)
    out.update(solve_ms=float(np.median(solves[1:])), solve_passes=res.n_passes, solve_iterations=res.n_iterations,
               residual=res.residual)

    f = eng.to_device(res.f_k)
    s, G, obj = eng.empty((K,), np.float64), eng.empty((K, K), np.float64), eng.empty((1,), np.float64)
    status, logden = eng.zeros((1,), np.int32), eng.empty((N,), np.float64)

    def one_pass(gram):
        ts = []
        for _ in range(9):
            a, b = eng.event(), eng.event()
            a.record()
            check(lib.msm_mbar_pass(eng.handle, u.ptr, MSM_F64, K, N, N, f.ptr, lnN.ptr, gram, 0, logden.ptr, s.ptr,
                                    G.ptr if gram else None, obj.ptr, status.ptr), eng.handle)
            b.record()
            eng.sync()
            ts.append(a.elapsed_ms(b))
        return float(np.median(ts[2:]))

    floor_bytes = K * N * 8 + 8 * N
    out["floor_us_at_hbm_peak"] = floor_bytes / HBM_PEAK * 1e6
    for name, gram in (("pass_gram", 1), ("pass_no_gram", 0)):
        ms = one_pass(gram)
        out[name + "_ms"] = ms
        out[name + "_fraction_of_hbm_peak"] = floor_bytes / (ms * 1e-3) / HBM_PEAK

    uh = u.to_host()
    t0 = time.perf_counter()
    ref = R.mbar_pass(uh, N_k, res.f_k)
    out["numpy_pass_ms"] = (time.perf_counter() - t0) * 1e3
    out["s_max_abs_diff_to_numpy"] = float(np.abs(s.to_host() - ref["s"]).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
