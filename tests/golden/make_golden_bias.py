"""Generate tests/golden/bias.npz and bias.json by IMPORTING THE REFERENCE's bias potential.

Run in the build container only (the reference tree does not travel):

    PYTHONPATH=/root/reference/src python tests/golden/make_golden_bias.py

The feature specification is the one of tests/golden/pbc.json (23 features on 12 atoms: distances, angles and torsions
with per-entry ``pbc`` flags and weights).  Cases, 16 frames each from tests/_pbc_ref.draw_frames (every frame
well conditioned, asserted here): `ortho` and `tric` (a breathing box per frame), `nobox` (no atom displaced, nothing
wraps: the reference gets the specification with every ``pbc`` off) and `tric15` (15 atoms, three of them referenced by
nothing: their force is exactly zero).  Two networks 23 -> 32 -> 16 -> 3 from the seeded recipes of tests/_bias_ref.py,
built by the reference's build_network and loaded strictly: plain tanh, and input + hidden LayerNorm with gelu.  The
scaler of a case is the mean and standard deviation of its frames' reference features; the strength is 10.

Recorded per case and network: energy, CVs and -dE/dx of the reference's CVBiasPotential with torch autograd, as the
reference runs it (fp32) and in fp64 (modules .double(), the extractor's _feature_dtype float64, the fp32 inputs
widened); and the specification's hash as export.py writes it.  Gaps, per quantity, the largest over all cases:
|ref32 - ref64|, |restatement (tests/_bias_ref.py) - ref64|, and for each of the two adjoints alone |restatement in
float64 - the same restatement in numpy longdouble| over the sum of the absolute terms per output (random upstream
gradient; the network's with its own 2 k y as well; tanh networks only, scipy's erf being fp64).  These recorded
values, not constants chosen in advance, are the yardsticks of tests/test_gpu_bias.py.  No reference source text is stored."""

from __future__ import annotations

import copy
import json
import sys
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(REF / "src"))
sys.path.insert(0, str(OUT.parents[1]))

import torch  # noqa: E402
from pmarlo.features.deeptica._full import DeepTICAConfig  # noqa: E402
from pmarlo.features.deeptica.core.model import build_network  # noqa: E402
from pmarlo.features.deeptica.cv_bias_potential import create_cv_bias_potential  # noqa: E402
from pmarlo.features.deeptica.export import _hash_feature_spec, _json_compatible  # noqa: E402
from pmarlo.features.deeptica.ts_feature_extractor import (  # noqa: E402
    build_feature_extractor_module,
    canonicalize_feature_spec,
)
from sklearn.preprocessing import StandardScaler  # noqa: E402

from tests import _bias_ref as B  # noqa: E402
from tests import _deeptica_ref as R  # noqa: E402
from tests import _pbc_ref as P  # noqa: E402

N_FRAMES, BOND, STRENGTH = 16, 0.15, 10.0
CASES = {"ortho": ((2.0, 2.5, 3.0, 90.0, 90.0, 90.0), 12, True), "tric": ((2.4, 2.6, 2.9, 75.0, 98.0, 62.0), 12, True),
         "nobox": (None, 12, False), "tric15": ((2.4, 2.6, 2.9, 75.0, 98.0, 62.0), 15, True)}
FAR = np.eye(3, dtype=np.float32) * 100.0      # a box nothing wraps in: the reference's forward wants one


def reference_network(name: str):
    config = B.NETWORKS[name]
    cfg = DeepTICAConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in config.items()})
    scaler = StandardScaler()
    scaler.mean_, scaler.scale_ = np.zeros(B.N_FEATURES), np.ones(B.N_FEATURES)
    scaler.n_features_in_ = B.N_FEATURES
    net = build_network(cfg, scaler, seed=0)
    params = B.network_params(name)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == R.key_layout(config, B.N_FEATURES)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    return net.eval()


def run_reference(bias, xyz, box, dtype):
    E, cv, F = [], [], []
    for t in range(xyz.shape[0]):
        pos = torch.tensor(xyz[t], dtype=dtype, requires_grad=True)
        bx = torch.tensor(box[t], dtype=dtype)
        e = bias(pos, bx)
        e.backward()
        with torch.no_grad():
            cv.append(bias.compute_cvs(pos, bx)[0].numpy().astype(np.float64))
        E.append(float(e))
        F.append(-pos.grad.numpy().astype(np.float64))
    return np.asarray(E), np.stack(cv), np.stack(F)


def main() -> None:
    meta_pbc = json.loads((OUT / "pbc.json").read_text())
    raw_spec = meta_pbc["spec"]
    spec = canonicalize_feature_spec(raw_spec)
    off_spec = canonicalize_feature_spec({"use_pbc": False, "features": [{k: v for k, v in e.items() if k != "pbc"}
                                                                         for e in raw_spec["features"]]})
    rec, param, width = B.table_from_spec(spec)
    assert width == B.N_FEATURES
    rng = np.random.default_rng(20261019)
    arrays, gaps = {}, {"ref32_minus_ref64": {}, "restatement_minus_ref64": {}, "featurize_vjp_f64_minus_longdouble": 0.0,
                        "mlp_vjp_f64_minus_longdouble": 0.0}
    per_case = {}
    for case, (cell, n_atoms, wraps) in CASES.items():
        if cell is None:
            xyz = np.stack([(P.random_chain(rng, n_atoms, BOND) + rng.uniform(0.0, 2.0, size=3)).astype(np.float32)
                            for _ in range(N_FRAMES)])
            box = np.tile(FAR, (N_FRAMES, 1, 1))
            assert (P.torsion_lengths(spec, xyz, box) >= 1.0e-3).all()
        else:
            xyz, box, _cells, _ = P.draw_frames(rng, cell, N_FRAMES, spec, n_atoms, BOND)
        assert P.well_conditioned(spec, xyz, box).all()
        ext = build_feature_extractor_module(spec if wraps else off_spec).eval()
        with torch.no_grad():
            feats = np.stack([ext(torch.from_numpy(xyz[t]), torch.from_numpy(box[t])).numpy() for t in range(N_FRAMES)])
        mean = feats.astype(np.float64).mean(axis=0).astype(np.float32)
        scale = (feats.astype(np.float64).std(axis=0) + 0.05).astype(np.float32)
        arrays.update({f"{case}_xyz": xyz, f"{case}_mean": mean, f"{case}_scale": scale})
        if wraps:
            arrays[f"{case}_box"] = box
        dev_box = box if wraps else None
        # the featurizer's adjoint alone: float64 against longdouble
        g = rng.normal(size=(N_FRAMES, width))
        arrays[f"{case}_gfeat"] = g
        v64, s64 = B.featurize_vjp(rec, param, xyz, g, dev_box)
        vld, _ = B.featurize_vjp(rec, param, xyz, g, dev_box, dtype=np.longdouble)
        live = s64 > 0
        gap = float(np.max(np.abs(v64 - vld)[live] / s64[live]))
        gaps["featurize_vjp_f64_minus_longdouble"] = max(gaps["featurize_vjp_f64_minus_longdouble"], gap)
        for net_name in B.NETWORKS:
            net = reference_network(net_name)
            bias32 = create_cv_bias_potential(net, mean, scale, feature_extractor=ext,
                                              feature_spec_hash=_hash_feature_spec(_json_compatible(raw_spec)),
                                              bias_strength=STRENGTH).eval()
            bias64 = copy.deepcopy(bias32).double()
            bias64.feature_extractor._feature_dtype = torch.float64
            E32, cv32, F32 = run_reference(bias32, xyz, box, torch.float32)
            E64, cv64, F64 = run_reference(bias64, xyz, box, torch.float64)
            assert all(np.isfinite(a).all() for a in (E32, cv32, F32, E64, cv64, F64))
            law = B.golden_network(net_name, mean, scale)
            Er, cvr, Fr = B.energy_forces(rec, param, law, xyz, dev_box, "round", STRENGTH)
            key = f"{case}__{net_name}"
            arrays.update({f"{key}__E32": E32, f"{key}__cv32": cv32, f"{key}__F32": F32,
                           f"{key}__E64": E64, f"{key}__cv64": cv64, f"{key}__F64": F64})
            per_case[key] = {}
            for q, a32, a64, ar in (("energy", E32, E64, Er), ("cv", cv32, cv64, cvr), ("force", F32, F64, Fr)):
                d32, dr = float(np.max(np.abs(a32 - a64))), float(np.max(np.abs(ar - a64)))
                per_case[key][q] = {"ref32_minus_ref64": d32, "restatement_minus_ref64": dr,
                                    "largest": float(np.max(np.abs(a64)))}
                gaps["ref32_minus_ref64"][q] = max(gaps["ref32_minus_ref64"].get(q, 0.0), d32)
                gaps["restatement_minus_ref64"][q] = max(gaps["restatement_minus_ref64"].get(q, 0.0), dr)
            if n_atoms == 15:
                assert not F32[:, 12:].any() and not F64[:, 12:].any() and not Fr[:, 12:].any()
        # the network's adjoint alone (tanh networks: the plain one and the one with both LayerNorms)
        x = B.features(rec, param, xyz, dev_box)
        gout = rng.normal(size=(N_FRAMES, 3))
        arrays[f"{case}_gout"] = gout
        for net_name in ("tanh", "ln_tanh"):
            law = B.adjoint_network(net_name, mean, scale)
            for up in (gout, None):
                _e, _y, g64, s64 = B.mlp_vjp(law, x, up, STRENGTH)
                _e, _y, gld, _ = B.mlp_vjp(law, x, up, STRENGTH, dtype=np.longdouble)
                gap = float(np.max(np.abs(g64 - gld) / s64))
                gaps["mlp_vjp_f64_minus_longdouble"] = max(gaps["mlp_vjp_f64_minus_longdouble"], gap)
    np.savez_compressed(OUT / "bias.npz", **arrays)
    meta = {"spec_from": "pbc.json", "feature_spec_sha256": _hash_feature_spec(_json_compatible(raw_spec)),
            "cases": {k: {"n_atoms": v[1], "box": v[2]} for k, v in CASES.items()}, "networks": list(B.NETWORKS),
            "n_frames": N_FRAMES, "strength": STRENGTH, "gaps": gaps, "per_case": per_case}
    (OUT / "bias.json").write_text(json.dumps(meta, indent=1) + "\n")
    print(json.dumps(gaps, indent=1))
    for p in (OUT / "bias.npz", OUT / "bias.json"):
        print(f"{p.name:12s} {p.stat().st_size / 1024:8.1f} KB")


if __name__ == "__main__":
    main()
