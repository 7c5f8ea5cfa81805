"""TRAM at N = 1 M frames, K = 32 ensembles, m = 500 Markov states, fp64: the time of one msm_tram_pass (both
launches), of one msm_tram_rows launch, of one full iteration inside a check interval (msm_tram_iterations over 16
iterations, divided by 16) and, as the yardstick, of msm_mbar_pass(want_gram = 0) on the same u in the same process
(HIP events, one warm-up call, median of 7); beside them the numpy restatement's pass (tests/_tram_ref.py) on the same
box and the byte floor K N 8 + 8 N at the 8 TB/s HBM peak.  The count matrices are banded (a state exchanges with its
three neighbours on either side), as real ones are sparse; `--dense` fills them.
Usage: python tools/time_tram.py [--dense]"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmarlo_amd._lib import MSM_F64, TRAM_ROWS_COUNTS, check, lib  # noqa: E402
from pmarlo_amd.device import get_engine  # noqa: E402
from tests import _tram_ref as R  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    K, m, N = 32, 500, 1_000_000
    dense = "--dense" in sys.argv
    rng = np.random.default_rng(0)
    state = np.sort(rng.integers(m, size=N))
    thermo = rng.integers(K, size=N)
    centre = np.linspace(-1.0, 1.0, K)
    x = (state / m * 2 - 1) + 0.05 * rng.standard_normal(N)
    u = 8.0 * (x[None, :] - centre[:, None]) ** 2
    Nki = np.zeros((K, m))
    np.add.at(Nki, (thermo, state), 1.0)
    i = np.arange(m)
    band = (np.abs(i[:, None] - i[None, :]) <= 3) | dense
    C = rng.integers(1, 20, size=(K, m, m)) * band[None] * (Nki[:, :, None] > 0) * (Nki[:, None, :] > 0)
    C = C * np.minimum(1.0, (Nki / np.maximum(C.sum(axis=1), 1)).min(axis=1))[:, None, None]
    prob = R.problem(C, u, state, thermo)
    f, v = R.start(prob)

    eng = get_engine()
    off = np.concatenate([[0], np.cumsum(np.bincount(state, minlength=m))])
    tables = eng.tram_tables(off)
    u_d = eng.to_device(u)
    S, Nd, col = eng.to_device(prob["S"]), eng.to_device(prob["N"]), eng.to_device(prob["col"])
    f_d, v_d = eng.to_device(f), eng.to_device(v)
    g_d = eng.to_device(R.log_multipliers(f, v))
    _, g1 = eng.tram_rows(S, g_d, f_d, Nd, col, "multipliers")
    Rk, tab = eng.tram_rows(S, g1, f_d, Nd, col, "counts")
    s, logden, status = eng.empty((K, m), np.float64), eng.empty((N,), np.float64), eng.zeros((1,), np.int32)
    work, err = eng.empty((5, K, m), np.float64), eng.empty((1,), np.float64)
    out = {"K": K, "m": m, "N": N, "dense_counts": dense, "nonzeros_per_S_row": float((prob["S"] != 0).sum() / (K * m)),
           "plan": eng.tram_plan(K, off)}

    def timed(call, per=1):
        ts = []
        for _ in range(8):
            a, b = eng.event(), eng.event()
            a.record()
            call()
            b.record()
            eng.sync()
            ts.append(a.elapsed_ms(b) / per)
        return float(np.median(ts[1:]))

    tabs = (tables["offsets"].ptr, tables["unit_ptr"].ptr, tables["unit_state"].ptr, tables["units"])
    out["pass_ms"] = timed(lambda: check(lib.msm_tram_pass(eng.handle, u_d.ptr, MSM_F64, K, m, N, N, *tabs, tab.ptr, 0,
                                                           logden.ptr, s.ptr, status.ptr), eng.handle))
    out["pass_no_logden_ms"] = timed(lambda: check(lib.msm_tram_pass(eng.handle, u_d.ptr, MSM_F64, K, m, N, N, *tabs,
                                                                     tab.ptr, 0, None, s.ptr, status.ptr), eng.handle))
    out["rows_ms"] = timed(lambda: check(lib.msm_tram_rows(eng.handle, K, m, S.ptr, g1.ptr, f_d.ptr, Nd.ptr, col.ptr,
                                                           TRAM_ROWS_COUNTS, Rk.ptr, tab.ptr), eng.handle))
    out["iteration_ms"] = timed(lambda: check(lib.msm_tram_iterations(
        eng.handle, u_d.ptr, MSM_F64, K, m, N, N, *tabs, S.ptr, Nd.ptr, col.ptr, f_d.ptr, v_d.ptr, work.ptr, 16, 0,
        logden.ptr, err.ptr, status.ptr), eng.handle), per=16)
    out["err_after_timing"] = float(err.to_host()[0])

    fk, lnN = eng.zeros((K,), np.float64), eng.to_device(np.log(np.maximum(np.bincount(thermo, minlength=K), 1.0)))
    sk, obj = eng.empty((K,), np.float64), eng.empty((1,), np.float64)
    out["mbar_pass_no_gram_ms"] = timed(lambda: check(lib.msm_mbar_pass(
        eng.handle, u_d.ptr, MSM_F64, K, N, N, fk.ptr, lnN.ptr, 0, 0, logden.ptr, sk.ptr, None, obj.ptr, status.ptr),
        eng.handle))
    out["pass_over_mbar_pass"] = out["pass_ms"] / out["mbar_pass_no_gram_ms"]
    out["status"] = int(status.to_host()[0])
    floor_bytes = K * N * 8 + 8 * N
    out["floor_us_at_hbm_peak"] = floor_bytes / HBM_PEAK * 1e6
    out["pass_fraction_of_hbm_peak"] = floor_bytes / (out["pass_ms"] * 1e-3) / HBM_PEAK
    out["rows_bytes"] = K * m * m * 8

    # the numpy pass, and the device against it, at the table the timed pass used
    Rk2, tab2 = eng.tram_rows(S, g1, eng.to_device(f), Nd, col, "counts")
    r = eng.tram_pass(u_d, tables, tab2)
    t0 = time.perf_counter()
    ref = R.frame_pass(u, state, tab2.to_host(), m)
    out["numpy_pass_ms"] = (time.perf_counter() - t0) * 1e3
    out["s_max_rel_diff_to_numpy"] = float((np.abs(r["s"].to_host() - ref["s"]) / np.maximum(ref["s"], 1e-300)).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
