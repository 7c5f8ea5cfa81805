"""Write tests/golden/conformations.npz and conformations.json: what the reference's own StateDetector (host-only
methods) and result classes return on small recorded inputs.

Usage: python tests/golden/make_golden_conformations.py <reference source root>
(the directory that holds pmarlo/conformations/state_detection.py and results.py; both need numpy, scipy and the
standard library only and are loaded from those files, nothing of them is stored).

conformations.npz: inputs (fes/<name>, pi, committors, cv, dtraj0, dtraj1, labels, and the arrays the result objects
are built from) and outputs, <method>/<case>/source and /sink, or /error holding the exception's class name.
conformations.json: the to_dict() of a TPTResult, a Conformation and a ConformationSet built from those arrays."""

from __future__ import annotations

import importlib.util
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[2]

FES_METHODS = ("watershed", "local_minima", "threshold")
BASINS = (2, 3)


def _load(src: Path, name: str):
    spec = importlib.util.spec_from_file_location(name, src)
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module
    spec.loader.exec_module(module)
    return module


def surfaces() -> dict:
    """Small 2-D free-energy grids: separated wells of different depth, a rugged one, and a flat one (no basins)."""
    y, x = np.mgrid[0:24, 0:30]

    def well(cy, cx, depth, width):
        return -depth * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * width ** 2))

    rng = np.random.default_rng(7)
    return {
        "two_wells": 10.0 + well(6, 7, 8.0, 3.0) + well(17, 22, 6.5, 3.5),
        "three_wells": 10.0 + well(5, 5, 7.0, 2.5) + well(18, 14, 9.0, 3.0) + well(6, 25, 5.0, 2.0),
        "rugged": 10.0 + well(12, 15, 6.0, 6.0) + rng.normal(0.0, 0.6, (24, 30)),
        "flat": np.full((24, 30), 3.0),
    }


def main() -> None:
    src = Path(sys.argv[1]) / "pmarlo" / "conformations"
    sd = _load(src / "state_detection.py", "reference_state_detection")
    rs = _load(src / "results.py", "reference_results")
    det = sd.StateDetector()
    out: dict = {}

    def record(key, call):
        try:
            source, sink = call()
        except Exception as e:       # the class of the error is part of the behaviour
            out[f"{key}/error"] = np.array(type(e).__name__)
            print(f"{key:40s} {type(e).__name__}: {e}")
            return
        out[f"{key}/source"], out[f"{key}/sink"] = np.asarray(source, np.int64), np.asarray(sink, np.int64)
        print(f"{key:40s} source {np.asarray(source).tolist()} sink {np.asarray(sink).tolist()}")

    for name, F in surfaces().items():
        out[f"fes/{name}"] = F
        for method in FES_METHODS:
            for nb in BASINS:
                if name == "flat" and method == "local_minima":
                    continue             # all points tie: the pick would record argsort's order of equal keys
                record(f"{method}/{name}/{nb}",
                       lambda: det.detect_from_fes(SimpleNamespace(F=F), n_basins=nb, method=method))

    rng = np.random.default_rng(11)
    pi = rng.random(17)
    pi /= pi.sum()
    out["pi"] = pi
    for top_n in (2, 3, 5):
        record(f"population/{top_n}", lambda: det.detect_from_populations(pi, top_n=top_n))

    q = np.round(rng.random(40), 2)
    q[:4] = [0.05, 0.95, 0.0, 1.0]
    out["committors"] = q
    a, b, c = det.classify_committor_states(q)
    out["classify/source"], out["classify/sink"], out["classify/transition"] = a, b, c

    cv = rng.normal(0.0, 1.0, 60)
    dtrajs = [rng.integers(0, 9, 25), rng.integers(0, 9, 35)]
    out["cv"], out["dtraj0"], out["dtraj1"] = cv, dtrajs[0], dtrajs[1]
    record("cv_ranges/frames", lambda: det.from_cv_ranges(cv, "x", (-3.0, -0.8), (0.9, 3.0)))
    record("cv_ranges/states", lambda: det.from_cv_ranges(cv, "x", (-3.0, -0.8), (0.9, 3.0), dtrajs=dtrajs))
    record("cv_ranges/empty", lambda: det.from_cv_ranges(cv, "x", (50.0, 60.0), (0.9, 3.0)))
    record("frame_indices", lambda: det.from_frame_indices([0, 3, 3, 30], [59, 12], dtrajs))
    labels = rng.integers(0, 3, 17)
    out["labels"] = labels
    record("macrostate_labels/0_2", lambda: det.from_macrostate_labels(labels, 0, 2))
    record("macrostate_labels/missing", lambda: det.from_macrostate_labels(labels, 0, 7))

    # result classes
    n = 5
    out["res/qp"], out["res/qm"] = rng.random(n), rng.random(n)
    out["res/gross"], out["res/net"] = rng.random((n, n)), rng.random((n, n))
    out["res/path_fluxes"] = rng.random(2)
    out["res/kis"], out["res/evecs"] = rng.random(n), rng.normal(size=(3, n))
    tpt = rs.TPTResult(
        source_states=np.array([0]), sink_states=np.array([3, 4]), forward_committor=out["res/qp"],
        backward_committor=out["res/qm"], flux_matrix=out["res/gross"], net_flux=out["res/net"], total_flux=0.125,
        rate=0.25, mfpt=4.0, pathways=[[0, 2, 4], [0, 1, 3]], pathway_fluxes=out["res/path_fluxes"],
        bottleneck_states=np.array([2, 1, 0, 4, 3]), tpt_converged=False, pathway_iterations=17,
        pathway_max_iterations=10_000)
    kis = rs.KISResult(kis_scores=out["res/kis"], k_slow=2, eigenvectors=out["res/evecs"],
                       eigenvalues=np.array([1.0, 0.9, 0.5]), ranked_states=np.argsort(out["res/kis"])[::-1])
    unc = rs.UncertaintyResult("rate", 0.25, 0.01, 0.23, 0.27, 40, "bootstrap")
    confs = [
        rs.Conformation("metastable", 0, 0.5, 1.75, macrostate_id=0, frame_index=12, trajectory_index=1,
                        local_frame_index=2, committor=0.0, kis_score=0.125, flux=0.0625, structure_path="a/b.pdb",
                        metadata={"role": "source"}),
        rs.Conformation("tse", np.int64(2), np.float64(0.125), np.float64(5.25), committor=np.float64(0.5)),
    ]
    full = rs.ConformationSet(conformations=confs, tpt_result=tpt, kis_result=kis, uncertainty_results=[unc],
                              macrostate_labels=np.array([0, 0, 1, 1, 1]), metadata={"n_conformations": 2})
    doc = {"tpt": tpt.to_dict(), "conformation": confs[0].to_dict(), "conformation_defaults": confs[1].to_dict(),
           "set": full.to_dict(), "set_empty": rs.ConformationSet().to_dict(), "set_json": full.to_json()}
    np.savez_compressed(ROOT / "tests" / "golden" / "conformations.npz", **out)
    (ROOT / "tests" / "golden" / "conformations.json").write_text(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
