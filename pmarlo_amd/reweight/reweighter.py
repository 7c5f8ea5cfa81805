"""Reweighter: MBAR or TRAM frame weights for a dataset of splits drawn at several temperatures.

The toolkit this engine serves wrote one ``w_frame`` per frame from an MBAR / TRAM reweighter; that package is not
part of the snapshot modelled here, so the interface below is this engine's own.  The consumers are unchanged:
``dataset["frame_weights"][split]`` is what discretize_dataset, prepare_msm_discretization and the free-energy entry
points read.
"""

from __future__ import annotations

from typing import Any, Dict, Mapping, MutableMapping

import numpy as np

from ..analysis.fes import BOLTZMANN_CONSTANT_KJ_PER_MOL
from ..device import Engine, get_engine
from .mbar import temperature_weights
from .tram import tram

__all__ = ["Reweighter"]


class Reweighter:
    """``Reweighter(temperature_ref_K).apply(dataset)`` writes ``dataset["frame_weights"]``.

    Every split of ``dataset["splits"]`` carries ``"energy"`` [N_s] (kJ / mol) and either a scalar
    ``"temperature_K"`` or a per-frame ``"state_index"`` into the shared ``dataset["temperatures_K"]``.  All splits
    are solved as one problem and the weights towards ``temperature_ref_K`` are jointly normalised: summed over
    all splits they give 1.

    ``mode="MBAR"`` (the default) treats every frame as an independent draw from its rung.  ``mode="TRAM"`` assumes
    equilibrium only inside a Markov state: it needs ``lag`` and a ``"dtraj"`` [N_s] of Markov state labels in every
    split (a split is one trajectory; negative labels are unassigned frames, which get weight 0), and keeps the
    TRAMResult, with the Markov model of every rung, in ``.result``."""

    def __init__(self, temperature_ref_K: float, mode: str = "MBAR", lag: int | None = None, *, tol: float = 1e-10,
                 maxiter: int | None = None, check_every: int = 16, engine: Engine | None = None) -> None:
        if not np.isfinite(temperature_ref_K) or temperature_ref_K <= 0:
            raise ValueError("temperature_ref_K must be a positive finite number")
        if mode not in ("MBAR", "TRAM"):
            raise ValueError(f'mode must be "MBAR" or "TRAM", got {mode!r}')
        if mode == "TRAM" and (lag is None or int(lag) < 1):
            raise ValueError('mode="TRAM" needs a lag >= 1')
        self.temperature_ref_K = float(temperature_ref_K)
        self.mode, self.lag, self.check_every = mode, None if lag is None else int(lag), int(check_every)
        self.tol, self.engine = float(tol), engine
        self.maxiter = int(maxiter) if maxiter is not None else (100 if mode == "MBAR" else 100_000)
        self.result = None          # the MBARResult / TRAMResult of the latest apply()

    def apply(self, dataset: MutableMapping[str, Any]) -> Dict[str, np.ndarray]:
        splits = dataset.get("splits") if isinstance(dataset, Mapping) else None
        if not isinstance(splits, Mapping) or not splits:
            raise ValueError('Reweighter.apply needs dataset["splits"]')
        temps = [float(t) for t in np.asarray(dataset.get("temperatures_K", []), np.float64).reshape(-1)]
        n_shared = len(temps)
        energies, index, dtrajs, sizes = [], [], [], {}
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
            if self.mode == "TRAM":
                if split.get("dtraj") is None:
                    raise ValueError(f"split '{name}' has no \"dtraj\": mode=\"TRAM\" needs Markov state labels")
                d = np.asarray(split["dtraj"]).reshape(-1)
                if d.shape != E.shape:
                    raise ValueError(f"split '{name}': dtraj has {d.size} entries, energy {E.size}")
                dtrajs.append(d.astype(np.int64))
            energies.append(E)
            index.append(idx)
            sizes[str(name)] = E.size
        if self.mode == "TRAM":
            w = self._tram_weights(energies, index, dtrajs, temps)
        else:
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

    def _tram_weights(self, energies, index, dtrajs, temps) -> np.ndarray:
        """u_kn = E_n / (k_B T_k) over the rungs that drew frames, built on the device as the MBAR path builds it."""
        eng = self.engine if self.engine is not None else get_engine()
        T = np.asarray(temps, np.float64)
        if not (np.isfinite(T).all() and (T > 0).all()):
            raise ValueError("temperatures must be positive and finite")
        idx = np.concatenate(index)
        used = np.nonzero(np.bincount(idx, minlength=T.size))[0]
        rung = np.full(T.size, -1, np.int64)
        rung[used] = np.arange(used.size)
        E_d = eng.to_device(np.concatenate(energies))
        u = eng.mbar_reduced_potentials(E_d, 1.0 / (BOLTZMANN_CONSTANT_KJ_PER_MOL * T[used]))
        ut = eng.mbar_reduced_potentials(E_d, [1.0 / (BOLTZMANN_CONSTANT_KJ_PER_MOL * self.temperature_ref_K)])
        self.result = tram(dtrajs, [rung[i] for i in index], u, self.lag, targets=ut, tol=self.tol,
                           maxiter=self.maxiter, check_every=self.check_every, engine=eng)
        return self.result.weights[0]
