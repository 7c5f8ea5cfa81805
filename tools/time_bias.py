#!/usr/bin/env python3
"""Time msm_bias_energy_forces with HIP events: tools/time_bias.py [--small]

  step     one MD step: n = 1, 12 atoms / 23 features (the table of tests/golden/pbc.json), one box, replayed from a
           captured graph (three kernel nodes); the median of 7 windows of 200 replays each, per replay
  batch    n = 65 536 frames of the same system, one box per frame, device-resident, one call = three launches
  ca       n = 65 536 frames of 138 atoms with the 45 distances between 10 C-alpha atoms (chignolin's C-alpha pairs),
           no box
The network is 23 -> 32 -> 16 -> 3 (45 -> 32 -> 16 -> 3 for `ca`) with input and hidden LayerNorm and gelu.  One
warm-up, then the median of 7 windows.  Per part: the three kernels timed apart through the C ABI.  GB/s of the adjoint
is its algorithmic traffic (12 A + 8 F bytes read, 24 A written per frame, plus 36 for a frame's box) over its time;
GF/s of the network part is 4 sum w_l w_{l+1} fp64 flops per frame (forward and backward products) over its time.
--small runs 1/16 of the frames (a rehearsal, not a measurement)."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from pmarlo_amd._lib import MIC_ROUND, check, lib  # noqa: E402
from pmarlo_amd.device import Engine  # noqa: E402
from pmarlo_amd.features.deeptica import MLPSpec  # noqa: E402
from pmarlo_amd.features.deeptica.ts_feature_extractor import canonicalize_feature_spec  # noqa: E402

RUNS = 7
N = 65_536 // (16 if "--small" in sys.argv else 1)
K = 10.0


def timed(eng, call, reps=1):
    call()
    eng.sync()
    times = []
    for _ in range(RUNS):
        e0 = eng.event().record()
        for _ in range(reps):
            call()
        e1 = eng.event().record()
        eng.sync()
        times.append(e0.elapsed_ms(e1) * 1e3 / reps)
    return float(np.median(times))


def network(F, rng):
    widths = (F, 32, 16, 3)
    parts = [rng.uniform(0.5, 1.5, F), rng.normal(size=F) * 0.3]
    for i in range(3):
        parts += [rng.normal(size=(widths[i + 1], widths[i])) / np.sqrt(widths[i]), rng.normal(size=widths[i + 1]) * 0.3]
        if i < 2:
            parts += [rng.uniform(0.5, 1.5, widths[i + 1]), rng.normal(size=widths[i + 1]) * 0.3]
    return MLPSpec(widths, 1, True, True, True, np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32),
                   rng.normal(size=F), rng.uniform(0.5, 2.0, size=F))


def parts(eng, xd, table, spec, bd, n_box):
    """Microseconds of the three kernels of one call, each through its own entry point."""
    n, A, _ = xd.shape
    F = table.width
    widths = np.ascontiguousarray(spec.widths, np.int32)
    params, mean, scale = eng._mlp_on_device(spec)
    feats, gfeat = eng.empty((n, F), np.float32), eng.empty((n, F), np.float64)
    energy, force = eng.empty((n,), np.float64), eng.empty((n, A, 3), np.float64)
    need = int(lib.msm_mlp_vjp_workspace(n, 3, widths.ctypes.data, 1, 1, 1))
    work = eng.empty((need // 8,), np.float64)
    ptr, inc = table.incidence(A)
    h, box = eng.handle, (bd.ptr if bd is not None else None)
    t_f = timed(eng, lambda: check(lib.msm_featurize_spec(h, xd.ptr, n, A, box, n_box, table.rec.ptr, table.param.ptr,
                                                          table.n_features, F, MIC_ROUND, feats.ptr, F, 0), h))
    t_n = timed(eng, lambda: check(lib.msm_mlp_vjp(h, feats.ptr, 0, n, F, F, mean.ptr, scale.ptr, 3, widths.ctypes.data, 1,
                                                   1, 1, 1, params.ptr, params.size, None, 0, K, energy.ptr, None, 3,
                                                   gfeat.ptr, F, work.ptr, work.nbytes), h))
    t_a = timed(eng, lambda: check(lib.msm_featurize_spec_vjp(h, xd.ptr, n, A, box, n_box, table.rec.ptr, table.param.ptr,
                                                              table.n_features, F, MIC_ROUND, gfeat.ptr, F, 0, ptr.ptr,
                                                              inc.ptr, -1.0, force.ptr), h))
    return t_f, t_n, t_a


def main():
    rng = np.random.default_rng(23)
    eng = Engine(0)
    spec12 = canonicalize_feature_spec(json.loads((ROOT / "tests" / "golden" / "pbc.json").read_text())["spec"])
    table = eng.feature_table(spec12)
    net = network(23, rng)
    chain = np.cumsum(rng.standard_normal((12, 3)) * 0.09, axis=0)
    xyz = (chain + 0.02 * rng.standard_normal((N, 12, 3)) + rng.uniform(0, 2, (N, 1, 3))).astype(np.float32)
    cells = np.tile([2.4, 2.6, 2.9, 75.0, 98.0, 62.0], (N, 1))
    cells[:, :3] *= 1.0 + 0.02 * rng.uniform(-1, 1, (N, 1))
    xd, bd = eng.to_device(xyz), eng.box_from_cell(cells)
    out = {}

    # one MD step from a graph
    x1, b1 = eng.to_device(xyz[:1]), eng.to_device(np.ascontiguousarray(bd.to_host()[:1]))
    res = eng.bias_energy_forces(x1, table, net, K, box=b1)
    eng.graph_begin()
    try:
        eng.bias_energy_forces(x1, table, net, K, box=b1, energy=res["energy"], cv=res["cv"], force=res["force"],
                               work=res["work"])
    finally:
        graph = eng.graph_end()
    out["step_graph_replay_us"] = timed(eng, lambda: eng.graph_launch(graph), reps=200)
    out["step_eager_us"] = timed(eng, lambda: eng.bias_energy_forces(
        x1, table, net, K, box=b1, energy=res["energy"], cv=res["cv"], force=res["force"], work=res["work"]), reps=200)
    eng.graph_destroy(graph)

    # the batch, device-resident
    res = eng.bias_energy_forces(xd, table, net, K, box=bd, chunk=N)
    call = lambda: eng.bias_energy_forces(xd, table, net, K, box=bd, chunk=N, energy=res["energy"], cv=res["cv"],   # noqa: E731
                                          force=res["force"], work=res["work"])
    t = timed(eng, call)
    t_f, t_n, t_a = parts(eng, xd, table, net, bd, N)
    flops = 4 * (23 * 32 + 32 * 16 + 16 * 3)
    out["batch"] = {"n": N, "atoms": 12, "features": 23, "call_us": t, "frames_per_s": N / t * 1e6, "launches": 3,
                    "featurize_us": t_f, "network_us": t_n, "adjoint_us": t_a,
                    "adjoint_GBps": (12 * 12 + 8 * 23 + 24 * 12 + 36) * N / t_a / 1e3,
                    "network_GFps": flops * N / t_n / 1e3}
    assert np.isfinite(res["force"].to_host()).all()

    # 138 atoms, 45 C-alpha distances
    ca = np.arange(2, 138, 14)[:10]
    pairs = np.array([(ca[i], ca[j]) for i in range(10) for j in range(i + 1, 10)], np.int32)
    table_ca = eng.feature_table(pairs=pairs, periodic=False)
    net_ca = network(45, rng)
    big = np.cumsum(rng.standard_normal((138, 3)) * 0.09, axis=0)
    xyz_ca = (big + 0.02 * rng.standard_normal((N, 138, 3), dtype=np.float32)).astype(np.float32)
    xc = eng.to_device(xyz_ca)
    res = eng.bias_energy_forces(xc, table_ca, net_ca, K, chunk=N)
    call = lambda: eng.bias_energy_forces(xc, table_ca, net_ca, K, chunk=N, energy=res["energy"], cv=res["cv"],   # noqa: E731
                                          force=res["force"], work=res["work"])
    t = timed(eng, call)
    t_f, t_n, t_a = parts(eng, xc, table_ca, net_ca, None, 0)
    flops = 4 * (45 * 32 + 32 * 16 + 16 * 3)
    out["ca"] = {"n": N, "atoms": 138, "features": 45, "call_us": t, "frames_per_s": N / t * 1e6, "launches": 3,
                 "featurize_us": t_f, "network_us": t_n, "adjoint_us": t_a,
                 "adjoint_GBps": (12 * 138 + 8 * 45 + 24 * 138) * N / t_a / 1e3, "network_GFps": flops * N / t_n / 1e3}
    assert np.isfinite(res["force"].to_host()).all()
    print(json.dumps(out, indent=1))
    eng.close()


if __name__ == "__main__":
    main()
