"""DeepTICA inference at the scale of a long trajectory: 1 M frames x 64 float32 features through
64 -> (128, 64) -> 3, gelu, both LayerNorms.  Kernel time of msm_mlp_forward from device events and
DeepTICAModel.transform host to host, rounds interleaved in one process (median and minimum), against the two
floors of the kernel and against the numpy restatement of the same law on the same box.

    python tools/time_deeptica.py [n_frames] [rounds] [activation]

Another activation (relu, tanh, ...) in place of gelu shows how much of the kernel is the activation itself.
"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmarlo_amd.device import get_engine  # noqa: E402
from pmarlo_amd.features.deeptica import DeepTICAModel  # noqa: E402
from tests import _deeptica_ref as R  # noqa: E402

FP64_MATRIX_PEAK = 78.6e12     # flop/s, v_mfma_f64 on the whole chip
HBM_ACHIEVABLE = 6.3e12        # bytes/s, measured streaming rate (8.0e12 is the specification)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    activation = sys.argv[3] if len(sys.argv) > 3 else "gelu"
    F, hidden, n_out = 64, (128, 64), 3
    config = {"n_out": n_out, "hidden": list(hidden), "activation": activation, "layer_norm_in": True,
              "layer_norm_hidden": True, "linear_head": False, "hidden_dropout": [0.1, 0.1]}
    rng = np.random.default_rng(7)
    params = {}
    for key, shape in R.key_layout(config, F):
        if len(shape) == 2:
            v = rng.normal(size=shape) * (1.3 / np.sqrt(shape[1]))
        else:
            v = rng.uniform(0.5, 1.5, size=shape) if key.endswith("weight") else rng.normal(size=shape) * 0.3
        params[key] = v.astype(np.float32)
    mean, std = rng.normal(size=F), rng.uniform(0.5, 2.0, size=F)
    X = (mean + std * rng.standard_normal((n, F), dtype=np.float32)).astype(np.float32)
    model = DeepTICAModel.from_arrays(config, params, mean, std)
    widths = model.spec.widths
    flop = 2.0 * n * sum(a * b for a, b in zip(widths[:-1], widths[1:]))
    nbytes = float(X.nbytes + n * n_out * 8)

    eng = get_engine()
    xd = eng.to_device(X)
    out = eng.empty((n, n_out), np.float64)
    e0, e1 = eng.event(), eng.event()
    kernel_ms, transform_ms = [], []
    for r in range(rounds + 2):                      # two warm-up rounds
        e0.record()
        eng.mlp_forward(xd, model.spec, out=out)
        e1.record()
        eng.sync()
        k = e0.elapsed_ms(e1)
        t0 = time.perf_counter()
        y = model.transform(X)
        t = (time.perf_counter() - t0) * 1e3
        if r >= 2:
            kernel_ms.append(k)
            transform_ms.append(t)
    t0 = time.perf_counter()
    ref = R.forward(config, params, mean, std, X)
    numpy_ms = (time.perf_counter() - t0) * 1e3

    def line(what, v):
        print(f"{what:34s} median {statistics.median(v):9.3f} ms   min {min(v):9.3f} ms   ({len(v)} rounds)", flush=True)

    print(f"n = {n}, widths {widths}, {activation}, {flop / n / 1e3:.1f} kflop and {nbytes / n:.0f} bytes per frame")
    line("msm_mlp_forward (device events)", kernel_ms)
    line("transform, host to host", transform_ms)
    print(f"{'numpy restatement (fp64, host)':34s}        {numpy_ms:9.1f} ms   (once)")
    floor_mm, floor_hbm = flop / FP64_MATRIX_PEAK * 1e3, nbytes / HBM_ACHIEVABLE * 1e3
    km = statistics.median(kernel_ms)
    print(f"fp64 matrix floor {floor_mm:.3f} ms -> kernel / floor = {km / floor_mm:.1f};   "
          f"HBM floor ({nbytes / 1e6:.0f} MB at {HBM_ACHIEVABLE / 1e12:.1f} TB/s) {floor_hbm:.3f} ms -> "
          f"kernel / floor = {km / floor_hbm:.1f}")
    print(f"max |device - numpy| = {np.max(np.abs(y - ref)):.3e} at output scale {np.max(np.abs(ref)):.2f}")


if __name__ == "__main__":
    main()
