"""Generate tests/golden/pbc.npz and pbc.json by IMPORTING THE REFERENCE's feature extractor.

Run in the build container only (the reference tree does not travel):

    PYTHONPATH=/root/reference/src python tests/golden/make_golden_pbc.py

Inputs: for each of three periodic boxes (orthorhombic, triclinic, truncated octahedron; every frame's box breathes
by +-2 %), 64 frames of a 12-atom random-walk chain (bond length 0.15 nm +- 10 %, no bend closer to collinear than
cos = 0.9) whose atoms are then each displaced by a random integer combination (coefficients in {-1, 0, 1}) of the
frame's box vectors, so that essentially every bond vector wraps.  Outputs: the reference extractor
(pmarlo.features.deeptica.ts_feature_extractor) on every frame, for a 23-entry spec interleaving 15 distances, 4 angles and 4 torsions, some
with ``pbc: False``, with weights that are not all 1.  Also stored: the reference's canonicalised metadata, and per
kind the largest |fp32 restatement (tests/_pbc_ref.py) - reference| over all boxes, the yardstick of the tests.

Conditions asserted here, per frame (tests/_pbc_ref.py: well_conditioned), a violating frame being redrawn from the
seeded generator (so no case is ever excluded from a comparison):
  * every flagged fractional component is >= 1e-3 from a half-integer in fp64: the rounding rule is unambiguous;
  * |b1| and both plane normals of every torsion are >= 1e-3 nm on the minimum-image vectors;
  * the gap between the best and the second-best image length of every flagged angle / torsion bond vector is
    >= 1e-3 nm: the true minimum image ("search" mode) is unambiguous too.
No reference source text is stored."""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(REF / "src"))
sys.path.insert(0, str(OUT.parents[1]))

import torch  # noqa: E402
from pmarlo.features.deeptica.ts_feature_extractor import (  # noqa: E402
    build_feature_extractor_module,
    canonicalize_feature_spec,
)

from tests import _pbc_ref as ref  # noqa: E402

N_FRAMES, N_ATOMS, BOND = 64, 12, 0.15
CELLS = {"ortho": (2.0, 2.5, 3.0, 90.0, 90.0, 90.0),
         "tric": (2.4, 2.6, 2.9, 75.0, 98.0, 62.0),
         "octa": (3.0, 3.0, 3.0, 70.53, 109.47, 70.53)}

SPEC = {"use_pbc": True, "features": [
    {"type": "distance", "atoms": [0, 1], "name": "d01"},
    {"type": "angle", "atoms": [0, 1, 2]},
    {"type": "distance", "atom_indices": [0, 11], "weight": 2.0},
    {"type": "torsion", "atoms": [0, 1, 2, 3], "name": "t0123"},
    {"type": "distance", "indices": [3, 9]},
    {"type": "distance", "atoms": [2, 3], "pbc": False},
    {"type": "angle", "atoms": [3, 4, 5], "weight": "0.5"},
    {"type": "distance", "atoms": [5, 6], "weight": -1.5},
    {"type": "dihedral", "atoms": [4, 5, 6, 7], "pbc": False},
    {"type": "distance", "atoms": [1, 10]},
    {"type": "distance", "atoms": [7, 8]},
    {"type": "angle", "atoms": [0, 5, 11]},
    {"type": "distance", "atoms": [4, 11], "weight": 0.25},
    {"type": "distance", "atoms": [6, 2]},
    {"type": "torsion", "atoms": [0, 3, 7, 11], "weight": 3.0},
    {"type": "distance", "atoms": [9, 10], "pbc": False},
    {"type": "distance", "atoms": [8, 0]},
    {"type": "angle", "atoms": [2, 7, 10], "pbc": False},
    {"type": "distance", "atoms": [10, 11]},
    {"type": "distance", "atoms": [5, 1]},
    {"type": "dihedral", "atoms": [8, 9, 10, 11], "name": "tail"},
    {"type": "distance", "atoms": [3, 4]},
    {"type": "distance", "atoms": [11, 6]},
]}


def main() -> None:
    spec = canonicalize_feature_spec(SPEC)
    ext = build_feature_extractor_module(spec).eval()
    rng = np.random.default_rng(20261019)
    arrays, recorded, redrawn = {}, {"distance": 0.0, "angle": 0.0, "dihedral": 0.0}, 0
    for name, cell in CELLS.items():
        xyz, box, cells, again = ref.draw_frames(rng, cell, N_FRAMES, spec, N_ATOMS, BOND)
        redrawn += again
        with torch.no_grad():
            out = np.stack([ext(torch.from_numpy(xyz[t]), torch.from_numpy(box[t])).numpy() for t in range(N_FRAMES)])
        assert out.dtype == np.float32 and np.isfinite(out).all()
        assert ref.well_conditioned(spec, xyz, box).all()
        mine = ref.extract(spec, xyz, box, mic="round", dtype=np.float32)
        wts = np.abs(np.asarray(spec.feature_weights))
        for kind, pos in (("distance", spec.distance_positions), ("angle", spec.angle_positions),
                          ("dihedral", spec.dihedral_positions)):
            pos = np.asarray(pos)
            d = mine[:, pos].astype(np.float64) - out[:, pos].astype(np.float64)
            if kind == "dihedral":       # modulo 2 pi, on the unweighted angle
                d = ref.wrap_to_pi(d / np.asarray(spec.feature_weights)[pos]) * wts[pos]
            recorded[kind] = max(recorded[kind], float(np.abs(d).max()))
        arrays.update({f"{name}_xyz": xyz, f"{name}_box": box, f"{name}_cell": cells, f"{name}_out": out})
    arrays.update(distance_pairs=spec.distance_pairs.numpy(), distance_positions=spec.distance_positions.numpy(),
                  distance_pbc=spec.distance_pbc.numpy(), angle_triplets=spec.angle_triplets.numpy(),
                  angle_positions=spec.angle_positions.numpy(), angle_pbc=spec.angle_pbc.numpy(),
                  dihedral_quads=spec.dihedral_quads.numpy(), dihedral_positions=spec.dihedral_positions.numpy(),
                  dihedral_pbc=spec.dihedral_pbc.numpy(), feature_weights=spec.feature_weights.numpy())
    np.savez_compressed(OUT / "pbc.npz", **arrays)
    meta = {"spec": SPEC, "feature_names": list(spec.feature_names), "use_pbc": bool(spec.use_pbc),
            "atom_count": int(spec.atom_count), "boxes": list(CELLS), "frames_redrawn": redrawn,
            "max_abs_fp32_restatement_minus_reference": recorded}
    (OUT / "pbc.json").write_text(json.dumps(meta, indent=1) + "\n")
    print(json.dumps(meta["max_abs_fp32_restatement_minus_reference"]), "redrawn", redrawn)
    for p in (OUT / "pbc.npz", OUT / "pbc.json"):
        print(f"{p.name:12s} {p.stat().st_size / 1024:8.1f} KB")


if __name__ == "__main__":
    main()
