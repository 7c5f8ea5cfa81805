"""Regenerate tests/golden/deeptica.npz / deeptica.json from the reference implementation.

Run in the build container only (the reference tree does not travel):

    PYTHONPATH=<reference checkout>/src python tests/golden/make_golden_deeptica.py

For every case of tests/_deeptica_ref.py the reference network is built with build_network, its state_dict keys and
shapes are checked against the recipe's, the recipe's arrays are loaded with strict=True, the model goes through the
reference's own DeepTICAModel.save / load, and transform and the raw network are run.  The inputs and parameters
come from the seeded recipes and are NOT stored; the files hold the key names, the reference's raw and final
outputs, and `ref_dev`: the largest distance of the reference's fp32 evaluation from the fp64 restatement, which is
the yardstick of the GPU tests.  A case whose ref_dev exceeds 1e-4 of its output scale (an ill-conditioned LayerNorm
row: a test that would show nothing) is refused.  No reference source text is stored.
"""

from __future__ import annotations

import json
import sys
import tempfile
import warnings
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from pmarlo.features.deeptica._full import DeepTICAConfig, DeepTICAModel  # noqa: E402
from pmarlo.features.deeptica.core.model import build_network  # noqa: E402
from sklearn.preprocessing import StandardScaler  # noqa: E402

from tests import _deeptica_ref as R  # noqa: E402

warnings.filterwarnings("ignore")


def run_case(name: str, tmp: Path):
    c = R.case(name)
    cfg = DeepTICAConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in c["config"].items()})
    scaler = StandardScaler(with_mean=True, with_std=True)
    scaler.mean_, scaler.scale_ = c["mean"].copy(), c["std"].copy()
    scaler.n_features_in_ = int(c["mean"].shape[0])
    net = build_network(cfg, scaler, seed=0)
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    want = R.key_layout(c["config"], c["X"].shape[1])
    assert got == want, (name, got, want)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c["params"].items()}, strict=True)
    net.eval()
    DeepTICAModel(cfg, scaler, net, training_history=c["history"]).save(tmp / name)
    model = DeepTICAModel.load(tmp / name)
    final = np.asarray(model.transform(np.asarray(c["X"])), np.float64)
    with torch.no_grad():
        Z = scaler.transform(np.asarray(c["X"], dtype=np.float64))
        raw = model.net(torch.as_tensor(Z, dtype=torch.float32)).detach().cpu().numpy().astype(np.float64)
    dev_raw = float(np.max(np.abs(raw - c["raw"])))
    dev_final = float(np.max(np.abs(final - c["final"])))
    scale_raw, scale_final = float(np.max(np.abs(c["raw"]))), float(np.max(np.abs(c["final"])))
    assert 0.0 < dev_raw <= 1e-4 * scale_raw, (name, "raw", dev_raw, scale_raw)
    assert 0.0 < dev_final <= 1e-4 * scale_final, (name, "final", dev_final, scale_final)
    meta = {"keys": [k for k, _ in got], "ref_dev": {"raw": dev_raw, "final": dev_final},
            "scale": {"raw": scale_raw, "final": scale_final}}
    return raw, final, meta


def main():
    arrays, doc = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in R.CASES:
            raw, final, meta = run_case(name, Path(tmp))
            arrays[f"raw__{name}"], arrays[f"final__{name}"] = raw, final
            doc[name] = meta
            print(name, meta["ref_dev"], meta["scale"])
    (HERE / "deeptica.json").write_text(json.dumps(doc, indent=1) + "\n")
    np.savez_compressed(HERE / "deeptica.npz", **arrays)
    print("wrote", HERE / "deeptica.json", HERE / "deeptica.npz")


if __name__ == "__main__":
    main()
