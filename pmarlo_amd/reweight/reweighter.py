"""Reweighter: MBAR frame weights for a dataset of splits drawn at several temperatures.

The toolkit this engine serves wrote one ``w_frame`` per frame from an MBAR / TRAM reweighter; that package is not
part of the snapshot modelled here, so the interface below is this engine's own.  The consumers are unchanged:
``dataset["frame_weights"][split]`` is what discretize_dataset, prepare_msm_discretization and the free-energy entry
points read.
"""

from __future__ import annotations

from typing import Any, Dict, Mapping, MutableMapping

import numpy as np

from ..device import Engine
from .mbar import temperature_weights

__all__ = ["Reweighter"]


class Reweighter:
    """``Reweighter(temperature_ref_K).apply(dataset)`` writes ``dataset["frame_weights"]``.

    Every split of ``dataset["splits"]`` carries ``"energy"`` [N_s] (kJ / mol) and either a scalar
    ``"temperature_K"`` or a per-frame ``"state_index"`` into the shared ``dataset["temperatures_K"]``.  All splits
    are solved as one MBAR problem and the weights towards ``temperature_ref_K`` are jointly normalised: summed over
    all splits they give 1."""

    def __init__(self, temperature_ref_K: float, *, tol: float = 1e-10, maxiter: int = 100,
                 engine: Engine | None = None) -> None:
        if not np.isfinite(temperature_ref_K) or temperature_ref_K <= 0:
            raise ValueError("temperature_ref_K must be a positive finite number")
        self.temperature_ref_K = float(temperature_ref_K)
        self.tol, self.maxiter, self.engine = float(tol), int(maxiter), engine
        self.result = None          # the MBARResult of the latest apply()

    def apply(self, dataset: MutableMapping[str, Any]) -> Dict[str, np.ndarray]:
        splits = dataset.get("splits") if isinstance(dataset, Mapping) else None
        if not isinstance(splits, Mapping) or not splits:
            raise ValueError('Reweighter.apply needs dataset["splits"]')
        temps = [float(t) for t in np.asarray(dataset.get("temperatures_K", []), np.float64).reshape(-1)]
        n_shared = len(temps)
        energies, index, sizes = [], [], {}
        for name, split in splits.items():
            if not isinstance(split, Mapping) or split.get("energy") is None:
                raise ValueError(f"split '{name}' has no \"energy\"")
            E = np.asarray(split["energy"], np.float64).reshape(-1)
            if split.get("state_index") is not None:
                idx = np.asarray(split["state_index"]).reshape(-1)
                if idx.shape != E.shape:
                    raise ValueError(f"split '{name}': state_index has {idx.size} entries, energy {E.size}")
                if n_shared == 0:
                    raise ValueError(f"split '{name}' has a state_index but the dataset has no \"temperatures_K\"")
                if idx.size and (idx.min() < 0 or idx.max() >= n_shared):
                    raise ValueError(f"split '{name}': state_index outside [0, {n_shared})")
                idx = idx.astype(np.int64)
            elif split.get("temperature_K") is not None:
                t = float(split["temperature_K"])
                if t not in temps:
                    temps.append(t)
                idx = np.full(E.size, temps.index(t), np.int64)
            else:
                raise ValueError(f"split '{name}' needs \"temperature_K\" or \"state_index\"")
            energies.append(E)
            index.append(idx)
            sizes[str(name)] = E.size
        w, self.result = temperature_weights(np.concatenate(energies), np.concatenate(index), temps,
                                             self.temperature_ref_K, tol=self.tol, maxiter=self.maxiter,
                                             engine=self.engine, return_result=True)
        out: Dict[str, np.ndarray] = {}
        at = 0
        for name, n in sizes.items():
            out[name] = w[at:at + n].copy()
            at += n
        fw = dataset.get("frame_weights")
        if not isinstance(fw, MutableMapping):
            fw = {}
            dataset["frame_weights"] = fw
        fw.update(out)
        return out
