"""Write tests/golden/representatives.npz: the picks of the reference's own RepresentativePicker.

Usage: python tests/golden/make_golden_representatives.py <reference source root>
(the directory that holds pmarlo/conformations/representative_picker.py; the module needs numpy only and is
loaded from that file, nothing of it is stored).  For every case of tests/_representatives_ref.GOLDEN_CASES and
every method the fixture holds the picks, int64 [n, 4], and the smallest relative margin that decided one:
between the n_select-th score and the next for the two smallest-n methods, between the best and the second
candidate of every round for `diverse`.  A margin below 1e-9 would make the comparison a coin toss between
summation orders, so such a fixture is refused."""

from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests import _representatives_ref as R  # noqa: E402

MIN_MARGIN = 1e-9


def main() -> None:
    src = Path(sys.argv[1]) / "pmarlo" / "conformations" / "representative_picker.py"
    spec = importlib.util.spec_from_file_location("reference_representative_picker", src)
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module
    spec.loader.exec_module(module)
    picker = module.RepresentativePicker()
    out = {}
    for name, *_ in R.GOLDEN_CASES:
        x, dtrajs, state_ids, weights, n_reps = R.golden_case(name)
        for method in R.METHODS:
            reps = picker.pick_representatives(x, list(dtrajs), state_ids, weights=weights, n_reps=n_reps, method=method)
            margins: list = []
            R.pick(x, dtrajs, state_ids, weights, n_reps, method, margins=margins)
            worst = float(min(margins))
            if worst < MIN_MARGIN:
                raise SystemExit(f"{name}/{method}: margin {worst:.3e} < {MIN_MARGIN}: choose another case")
            out[f"{name}/{method}/picks"] = np.asarray(reps, dtype=np.int64).reshape(-1, 4)
            out[f"{name}/{method}/margin"] = np.float64(worst)
            print(f"{name:22s} {method:20s} picks {len(reps):3d}  worst margin {worst:.2e}")
    np.savez_compressed(ROOT / "tests" / "golden" / "representatives.npz", **out)


if __name__ == "__main__":
    main()
