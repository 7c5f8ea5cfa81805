"""HMM at N = 1 M frames, one trajectory, k = 500 symbols: per EM iteration the time of the E-step (msm_hmm_estep: the
chunk products, the boundary scan, the chunk pass and the folds), of the emission sums (msm_hmm_emissions), of the
update (msm_hmm_mstep), of a whole iteration inside msm_hmm_iterations (8 iterations, divided by 8) and of
msm_hmm_viterbi (HIP events, one warm-up call, median of 7), for lag 10 with n = 4, lag 1 with n = 4 (a single
sequence: the worst case of the one-group boundary scan) and lag 10 with n = 16.  Beside them the traffic floor of an
iteration at the 8 TB/s HBM peak (labels read by the products and the pass, gamma written once and gathered once) and
the sequential fp64 numpy restatement (tests/_hmm_ref.py) on the first 20 000 frames, scaled to N.
The split of the E-step into its phases comes from a kernel trace of `--once` (one E-step of every shape, no
repeats): the kernels are hmm_product_kernel, hmm_boundary_kernel, hmm_pass_kernel, hmm_fold_*_kernel.
Usage: python tools/time_hmm.py [--once] [--shape 0|1|2]"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmarlo_amd._lib import check, lib  # noqa: E402
from pmarlo_amd.device import get_engine  # noqa: E402
from pmarlo_amd.markov_state_model.hmm import lag_observations  # noqa: E402
from tests import _hmm_ref as R  # noqa: E402

HBM_PEAK = 8.0e12


def model(n, k, rng):
    A = np.full((n, n), 0.02 / max(n - 1, 1)) + np.eye(n) * (0.98 - 0.02 / max(n - 1, 1))
    B = rng.random((n, k)) ** 4 + 1e-3
    return A / A.sum(axis=1, keepdims=True), B / B.sum(axis=1, keepdims=True), np.full(n, 1.0 / n)


def main():
    once = "--once" in sys.argv
    N, k = 1_000_000, 500
    rng = np.random.default_rng(0)
    eng = get_engine()
    shapes = ((10, 4), (1, 4), (10, 16))
    if "--shape" in sys.argv:
        shapes = (shapes[int(sys.argv[sys.argv.index("--shape") + 1])],)
    for lag, n in shapes:
        A, B, p0 = model(n, k, rng)
        hidden = np.cumsum(rng.random(N) < 0.02) % n              # dwell times of about 50 frames
        cdf = np.cumsum(B, axis=1)
        traj = np.minimum((rng.random(N)[:, None] > cdf[hidden]).sum(axis=1), k - 1).astype(np.int32)
        labels, table = lag_observations([traj], lag, k)
        t = eng.hmm_tables(eng.to_device(labels), k, table)
        dA, dB, dp = eng.to_device(A), eng.to_device(B), eng.to_device(p0)
        out = {"N": N, "k": k, "n": n, "lag": lag, "sequences": t["Q"], "plan": eng.hmm_plan(n, t["n_chunks"], t["Q"])}
        work = eng.empty((int(lib.msm_hmm_workspace_bytes(n, t["n_chunks"], t["Q"], t["units"])),), np.uint8)
        vwork = eng.empty((int(lib.msm_hmm_viterbi_workspace_bytes(n, k, t["n_chunks"], t["Q"])),), np.uint8)
        gamma = eng.zeros((N, n), np.float64)
        C, g0, logL = eng.empty((n, n), np.float64), eng.empty((n,), np.float64), eng.empty((t["Q"],), np.float64)
        E, part = eng.empty((n, k), np.float64), eng.empty((max(t["units"], 1), n), np.float64)
        total, hist, pi = eng.empty((1,), np.float64), eng.empty((8,), np.float64), eng.empty((n,), np.float64)
        path, logp, status = eng.empty((N,), np.int32), eng.empty((t["Q"],), np.float64), eng.zeros((1,), np.int32)
        seqs = (t["sequences"].ptr, t["Q"], t["chunk_ptr"].ptr, t["chunk_seq"].ptr, t["n_chunks"])
        groups = (t["offsets"].ptr, t["members"].ptr, t["unit_ptr"].ptr, t["unit_state"].ptr, t["units"])

        def estep():
            check(lib.msm_hmm_estep(eng.handle, t["labels"].ptr, N, k, n, *seqs, dA.ptr, dB.ptr, dp.ptr, 0, work.ptr,
                                    gamma.ptr, C.ptr, g0.ptr, logL.ptr, total.ptr, status.ptr), eng.handle)

        def emissions():
            check(lib.msm_hmm_emissions(eng.handle, gamma.ptr, N, n, k, *groups, 0, part.ptr, E.ptr), eng.handle)

        def timed(call, per=1):
            ts = []
            for _ in range(1 if once else 8):
                a, b = eng.event(), eng.event()
                a.record()
                call()
                b.record()
                eng.sync()
                ts.append(a.elapsed_ms(b) / per)
            return float(np.median(ts[1:] or ts))

        out["estep_ms"] = timed(estep)
        out["emissions_ms"] = timed(emissions)
        if not once:
            A2, B2, p2 = eng.to_device(A), eng.to_device(B), eng.to_device(p0)
            out["mstep_ms"] = timed(lambda: check(lib.msm_hmm_mstep(
                eng.handle, n, k, t["Q"], C.ptr, E.ptr, g0.ptr, 1, 0, 100_000, 1e-8, A2.ptr, B2.ptr, p2.ptr, pi.ptr,
                status.ptr), eng.handle))
            A3, B3, p3 = eng.to_device(A), eng.to_device(B), eng.to_device(p0)
            out["iteration_ms"] = timed(lambda: check(lib.msm_hmm_iterations(
                eng.handle, t["labels"].ptr, N, k, n, *seqs, *groups, 1, 0, 100_000, 1e-8, 8, 0, work.ptr, A3.ptr,
                B3.ptr, p3.ptr, pi.ptr, gamma.ptr, C.ptr, E.ptr, g0.ptr, logL.ptr, hist.ptr, status.ptr), eng.handle),
                per=8)
        out["viterbi_ms"] = timed(lambda: check(lib.msm_hmm_viterbi(
            eng.handle, t["labels"].ptr, N, k, n, *seqs, dA.ptr, dB.ptr, dp.ptr, 0, vwork.ptr, path.ptr, logp.ptr,
            status.ptr), eng.handle))
        out["status"] = int(status.to_host()[0])
        out["logL"] = float(total.to_host()[0])
        floor_bytes = 2 * 4 * N + 8 * n * N + 8 * n * N + 4 * N     # labels twice, gamma out, gamma in, members
        out["floor_us_at_hbm_peak"] = floor_bytes / HBM_PEAK * 1e6
        if not once:
            m = 20_000
            t0 = time.perf_counter()
            ref = R.estep(A, B, p0, labels[:m], R.single_rows([m]), k)
            R.mstep(ref["C"], ref["E"], ref["gamma0"], 1)
            out["numpy_iteration_ms_scaled_to_N"] = (time.perf_counter() - t0) * 1e3 * N / m
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
