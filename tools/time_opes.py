"""OPES kernels at scale: the replay of T = 10 000 deposits (d = 2) into the journal by msm_opes_deposit in bounded
launches of 256 deposits (wall clock around the launches and one sync; median of 3), msm_opes_bias in its journal form
at n = 1 M frames against those T versions (value only, then with the gradient, then without tile skipping; HIP events,
one warm-up call, median of 7), and one frame against the live kernels, the MD step of OPESCVBias, value and gradient
(HIP events around 20 calls).  Beside each time: the live-kernel count, the versions a frame's life-span test lets
through (counted on the host from the journal), and the numpy restatement (tests/_opes_ref.py, fp64) on a slice, scaled.
The deposits follow a random walk reflected into [-1.5, 1.5] x [-0.5, 2.5] with sigma0 = 0.1, as an OPES run makes them;
a frame sees the deposits made before it (count = frame index * T / n).
Usage: python tools/time_opes.py [--once]"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmarlo_amd.device import get_engine  # noqa: E402
from pmarlo_amd.reweight import OPESLedger  # noqa: E402
from tests import _opes_ref as O  # noqa: E402


def main():
    once = "--once" in sys.argv
    n, T, d = 1_000_000, 10_000, 2
    kT, barrier, sigma0 = 1.0, 10.0, 0.1
    rng = np.random.default_rng(0)
    lo, hi = np.array([-1.5, -0.5]), np.array([1.5, 2.5])
    walk = np.cumsum(rng.normal(scale=0.03, size=(n, d)), axis=0)
    u = (walk + 0.5 * (hi - lo)) % (2 * (hi - lo))
    cv = np.ascontiguousarray(lo + np.where(u > hi - lo, 2 * (hi - lo) - u, u))      # reflected into the box
    centers = np.ascontiguousarray(cv[(np.arange(T) * (n // T))])
    counts = (np.arange(n) // (n // T)).astype(np.int32)
    eng = get_engine()
    out = {"n": n, "T": T, "d": d, "plan": eng.opes_plan(n, T, d)}

    def ledger():
        return OPESLedger(d, kT, barrier=barrier, sigma0=sigma0, capacity=T, max_steps=256, engine=eng)

    cd = eng.to_device(centers)
    ts = []
    for _ in range(1 if once else 4):
        led = ledger()
        led.device_ledger()
        eng.sync()
        t0 = time.perf_counter()
        led.deposit(cd, np.arange(float(T)))
        eng.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    out["deposit_online_ms"] = float(np.median(ts[1:] or ts))
    state = led.state()
    out["live_kernels"], out["status"] = state["live"], state["status"]
    J = led.journal()

    cvd, cntd = eng.to_device(cv), eng.to_device(counts)
    bias, grad = eng.empty((n,), np.float64), eng.empty((n, d), np.float64)
    dev, par = led.device_ledger(), led.params()

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

    kw = dict(counts=cntd, bias=bias)
    out["bias_value_ms"] = timed(lambda: eng.opes_bias(cvd, dev, par, T, **kw))
    out["bias_value_grad_ms"] = timed(lambda: eng.opes_bias(cvd, dev, par, T, grad=True, grad_out=grad, **kw))
    got = bias.to_host()
    out["bias_value_no_skip_ms"] = timed(lambda: eng.opes_bias(cvd, dev, par, T, skip=False, **kw))
    out["skip_changes_bits"] = bool((bias.to_host() != got).any())
    one, b1, g1 = cvd.view((1, d), offset_elems=(n - 1) * d), eng.empty((1,), np.float64), eng.empty((1, d), np.float64)

    def md_steps():
        for _ in range(20):
            eng.opes_bias(one, dev, par, live=True, grad=True, bias=b1, grad_out=g1)

    out["one_frame_value_grad_ms"] = timed(md_steps) / 20
    # executed work: a lane tests the life span of every version before its count and evaluates those that live
    m = 300
    rows = np.linspace(0, n - 1, m).astype(np.int64)
    death = np.where(J["death"] >= T, O.ALIVE, J["death"])
    alive = (np.arange(T)[None, :] < counts[rows][:, None]) & (death[None, :] >= counts[rows][:, None])
    out["life_span_tests"] = float(counts.astype(np.float64).sum())
    out["distance_tests"] = float(alive.sum() * (n / m))
    refpar = O.Params(d, kT, barrier, sigma0=np.full(d, sigma0))
    t0 = time.perf_counter()
    ref = O.bias(None, refpar, cv[rows], counts[rows], dtype=np.float64, journal=J["kernels"], death=death, W=J["W"], Z=J["Z"])
    out["numpy_bias_ms_scaled_to_n"] = (time.perf_counter() - t0) * 1e3 * n / m
    out["max_abs_diff_vs_numpy_on_slice"] = float(np.max(np.abs(got[rows] - ref["bias"])))
    t0 = time.perf_counter()
    O.replay(refpar, centers[:300], dtype=np.float64)
    out["numpy_deposit_ms_for_300"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
