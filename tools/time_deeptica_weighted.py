#!/usr/bin/env python3
"""Time one DeepTICA training step with and without per-pair weights: tools/time_deeptica_weighted.py [--unweighted]

The widest network of the test recipes (tests/_deeptica_ref.py, case "wide") at batch 256 over 4096 resident frames:
msm_mlp_loss_grad[_weighted] + msm_adamw_step called back to back through the C ABI with no host synchronisation
in between, HIP events around 20 steps, the median of 7 such runs after 3 warm steps.  --unweighted times the
unweighted step alone and touches no weighted symbol, so the same file runs against a library that has none."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

BATCH, N_FRAMES, STEPS, REPS = 256, 4096, 20, 7


def main(weighted: bool) -> None:
    from pmarlo_amd import _lib
    from pmarlo_amd._lib import check, lib
    from pmarlo_amd.device import Engine, _dtype_code
    from pmarlo_amd.features.deeptica import DeepTICAModel
    from pmarlo_amd.features.deeptica.model import dropout_sites
    from tests import _deeptica_ref as R

    c = R.case("wide")
    F = c["X"].shape[1]
    rng = np.random.default_rng(0)
    x = (c["mean"] + c["std"] * rng.standard_normal((N_FRAMES, F))).astype(c["X"].dtype)
    eng = Engine(0)
    xd = eng.to_device(np.ascontiguousarray(x))
    model = DeepTICAModel.from_arrays(c["config"], c["params"], c["mean"], c["std"])
    spec = model.spec
    widths = np.ascontiguousarray(spec.widths, np.int32)
    n_linear = len(widths) - 1
    flags = (int(spec.ln_in), int(spec.ln_hidden), int(spec.head_activation))
    drop = np.ascontiguousarray(dropout_sites(model.config, n_linear), np.float64)
    params, mean, scale = eng._mlp_on_device(spec)
    it = rng.integers(0, N_FRAMES - 5, size=BATCH)
    itd, itaud = eng.to_device(it), eng.to_device(it + 5)
    wd = eng.to_device(np.exp(1.5 * rng.standard_normal(BATCH)))
    sizer = lib.msm_mlp_train_weighted_workspace if weighted else lib.msm_mlp_train_workspace
    work = eng.empty((int(sizer(BATCH, n_linear, widths.ctypes.data, *flags)) // 8,), np.float64)
    stats, out = eng.empty((_lib.VAMP2_STATS,), np.float64), eng.empty((4,), np.float64)
    grad = eng.empty((params.size,), np.float64)
    mom, var = eng.zeros((params.size,), np.float64), eng.zeros((params.size,), np.float64)
    head = (eng.handle, xd.ptr, _dtype_code(xd.dtype), N_FRAMES, F, F, mean.ptr, scale.ptr, n_linear, widths.ctypes.data,
            spec.activation, *flags, params.ptr, params.size, itd.ptr, itaud.ptr)

    def step(k: int, with_weights: bool) -> None:
        tail = (BATCH, drop.ctypes.data, 0, k, 1e-3, 1e-6, 0.15, 1e-4, work.ptr, work.nbytes, stats.ptr, grad.ptr, None,
                int(widths[-1]))
        if with_weights:
            check(lib.msm_mlp_loss_grad_weighted(*head, wd.ptr, *tail), eng.handle)
        else:
            check(lib.msm_mlp_loss_grad(*head, *tail), eng.handle)
        check(lib.msm_adamw_step(eng.handle, params.ptr, grad.ptr, mom.ptr, var.ptr, params.size, k, 3e-4, 0.9, 0.999,
                                 1e-8, 1e-4, 1.0, out.ptr), eng.handle)

    print(f"wide network {tuple(int(w) for w in widths)}, batch {BATCH}, dropout {drop.tolist()}")
    for with_weights in ((False, True) if weighted else (False,)):
        for k in range(1, 4):
            step(k, with_weights)
        eng.sync()
        times = []
        for rep in range(REPS):
            e0 = eng.event().record()
            for k in range(STEPS):
                step(100 + k, with_weights)
            e1 = eng.event().record()
            eng.sync()
            times.append(e0.elapsed_ms(e1) / STEPS)
        assert np.isfinite(stats.to_host()[0])
        print(f"{'weighted  ' if with_weights else 'unweighted'}: {np.median(times) * 1e3:7.1f} us per step "
              f"(min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f})", flush=True)
    eng.close()


if __name__ == "__main__":
    main("--unweighted" not in sys.argv)
