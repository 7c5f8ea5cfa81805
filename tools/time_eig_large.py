#!/usr/bin/env python3
"""Time msm_eigh and msm_tica_solve across the switch to the device-wide solver: tools/time_eig_large.py [--small]

Orders 256 (the one-workgroup Jacobi of eig.hip, global-memory path: the figure every earlier commit had), 320, 512,
1024 and 2048 (the block Jacobi of eig_large.h).  msm_eigh: a random symmetric matrix X + X', eigenvectors wanted.
msm_tica_solve: C00 = G G' + I / 10 (full rank), C0t = G diag(lambda) G' with lambda spread over (-0.5, 0.95), no
mean, no scale, kinetic map on.  HIP events around the whole call (the solve is one stream-ordered sequence of
launches, the host never waits inside it); one warm-up, then the median of 5 runs.  `sweeps` is what msm_eigh
reports; `x 256` is the time over the order-256 time of the same entry.  The yardstick: a solver that uses the chip
must stay below 8 x at order 512 (cubic scaling from the single compute unit that solves order 256).
--small stops at 512 (a rehearsal)."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from pmarlo_amd.device import Engine  # noqa: E402

ORDERS = [256, 320, 512, 1024, 2048]
RUNS = 5


def timed(eng, call):
    call()
    eng.sync()
    times = []
    for _ in range(RUNS):
        e0 = eng.event().record()
        call()
        e1 = eng.event().record()
        eng.sync()
        times.append(e0.elapsed_ms(e1))
    return float(np.median(times))


def tica_moments(n, rng):
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    lam = np.linspace(0.95, -0.5, n)
    C00 = G @ G.T + 0.1 * np.eye(n)
    C0t = (G * lam[None, :]) @ G.T
    # raw moments for T = 0.5 (w = 1): C00 = sym(M00), C0t = M0t + M0t'
    return np.concatenate([C00.ravel(), (0.5 * C0t).ravel(), np.zeros(2 * n), [0.5]])


eng = Engine(0)
orders = [n for n in ORDERS if n <= 512] if "--small" in sys.argv else ORDERS
print(f"{'order':>6} | {'eigh ms':>10} {'x 256':>7} {'sweeps':>6} | {'tica ms':>10} {'x 256':>7}")
base = {}
for n in orders:
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, n))
    a = eng.to_device(X + X.T)
    mom = eng.to_device(tica_moments(n, rng))
    out = (eng.empty((n,), np.float64), eng.empty((n, n), np.float64), eng.empty((n,), np.float64),
           eng.empty((1,), np.int32))
    sweeps = [0]

    def run_eigh():
        sweeps[0] = eng.eigh(a)[2]

    t_eigh = timed(eng, run_eigh)
    t_tica = timed(eng, lambda: eng.tica_solve(mom, n, out=out))
    base.setdefault("eigh", t_eigh)
    base.setdefault("tica", t_tica)
    print(f"{n:>6} | {t_eigh:10.2f} {t_eigh / base['eigh']:7.2f} {int(sweeps[0].to_host()[0]):>6} | "
          f"{t_tica:10.2f} {t_tica / base['tica']:7.2f}   rank {int(out[3].to_host()[0])}")
eng.close()
