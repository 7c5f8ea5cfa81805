"""Trajectory-bootstrap error bars on the device.

Mirrors pmarlo.conformations.uncertainty.UncertaintyQuantifier (S/conformations/uncertainty.py:15-261, 318-423,
_rebuild_msm :506-530) and UncertaintyResult (S/conformations/results.py:114-152): whole trajectories are resampled
with replacement, the MSM is rebuilt per sample, and mean / std / percentile bounds of the TPT rate, mfpt and total
flux, of the state free energies and of the PCCA+ macrostate populations are reported.

The reference rebuilds one matrix at a time.  Here every trajectory is counted once (msm_count_transitions per
trajectory); transition counts are additive over trajectories, so the counts of sample b are the integer combination
sum_s mult[b, s] * C_s (msm_combine_counts), exact.  The batch is row-normalised (msm_row_normalise_batched), its
stationary vectors come from the batched spectrum (msm_spectrum), and the committor systems of all samples are solved
by one launch with a workgroup per sample (msm_reactive_flux_batched).  The statistics over at most n_boot x k
numbers are numpy on the host.

Resampling: the indices are drawn on the host from np.random.default_rng(random_seed) in the reference's order
(n_traj scalar integers(0, n_traj) draws per sample, sample by sample, one generator per object), so equal seeds give
the reference's resamples.

A sample is dropped (n_samples counts the survivors) when its stationary vector is not unique (second-largest Ritz
modulus above 1 - 1e-9: np.linalg.eig's argmax cannot decide that case either) or not finite; for bootstrap_tpt also
when a row of its count matrix is empty (deeptime's MarkovStateModel refuses a matrix that is not stochastic and the
reference's `except` drops the sample) or a committor system is singular; for bootstrap_macrostate_populations also
when PCCA+ refuses the matrix (not reversible, as in deeptime).

Parity: the reference delegates counting, TPT and PCCA+ to deeptime 0.4.5, which is absent here; as for TPT itself,
parity with the reference's own output is unpinned.  The tests hold this module to a numpy restatement of the rules
above.

Not ported: hyperparameter_ensemble (reclusters with scikit-learn), chapman_kolmogorov_validation (the engine's
markov_state_model.ck covers its numerics) and the helpers only they use (_recluster, _coarse_grain_T).  finder.py,
which drives bootstrap_tpt and bootstrap_free_energies, is ported (finder.py of this package)."""

from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..device import get_engine
from ..markov_state_model.pcca import pcca_memberships
from ..markov_state_model.tpt import _roles

__all__ = ["UncertaintyQuantifier", "UncertaintyResult"]

logger = logging.getLogger("pmarlo.conformations")

# CODATA 2018 (exact since the 2019 SI): what scipy.constants.k and scipy.constants.Avogadro carry
BOLTZMANN_J_PER_K = 1.380649e-23
AVOGADRO_PER_MOL = 6.02214076e23
# a second Ritz value this close to the unit circle: the stationary vector is not unique
_DEGENERATE = 1.0 - 1e-9


@dataclass(frozen=True)
class UncertaintyResult:
    """Mean, standard deviation and confidence bounds of one observable (results.py:114-152).
    method is 'bootstrap' or 'hyperparameter_ensemble'."""

    observable_name: str
    mean: float | np.ndarray
    std: float | np.ndarray
    ci_lower: float | np.ndarray
    ci_upper: float | np.ndarray
    n_samples: int
    method: str

    def to_dict(self) -> Dict[str, Any]:
        def _to_serializable(val: Any) -> Any:
            if isinstance(val, np.ndarray):
                return val.tolist()
            return float(val) if np.isscalar(val) else val

        return {
            "observable_name": self.observable_name,
            "mean": _to_serializable(self.mean),
            "std": _to_serializable(self.std),
            "ci_lower": _to_serializable(self.ci_lower),
            "ci_upper": _to_serializable(self.ci_upper),
            "n_samples": int(self.n_samples),
            "method": str(self.method),
        }


def _array_result(name: str, samples: list, size: int, ci_percentiles, method: str = "bootstrap") -> UncertaintyResult:
    if len(samples) == 0:
        z = [np.zeros(size) for _ in range(4)]
        return UncertaintyResult(name, z[0], z[1], z[2], z[3], 0, method)
    a = np.array(samples)
    return UncertaintyResult(name, np.mean(a, axis=0), np.std(a, axis=0), np.percentile(a, ci_percentiles[0], axis=0),
                             np.percentile(a, ci_percentiles[1], axis=0), len(samples), method)


class UncertaintyQuantifier:
    """Bootstrap error bars of TPT observables, free energies and macrostate populations, and the host-side
    statistics of ensembles and iteration histories."""

    def __init__(self, random_seed: Optional[int] = None) -> None:
        self.random_seed = random_seed
        self.rng = np.random.default_rng(random_seed)
        self.last_kept = np.zeros(0, bool)       # which samples of the latest bootstrap survived, in draw order

    # -- resampling and the batched rebuild ------------------------------------------------------------------
    def _draw_multiplicities(self, n_traj: int, n_boot: int) -> np.ndarray:
        """[n_boot, n_traj] int32: how often trajectory s occurs in sample b (the reference's draw order)."""
        mult = np.zeros((int(n_boot), n_traj), np.int32)
        for b in range(int(n_boot)):
            for _ in range(n_traj):
                mult[b, self.rng.integers(0, n_traj)] += 1
        return mult

    @staticmethod
    def _check_dtrajs(dtrajs: Sequence[np.ndarray]) -> tuple[np.ndarray, np.ndarray, np.ndarray, int]:
        trajs = [np.asarray(d).ravel() for d in dtrajs]
        if len(trajs) == 0:
            raise ValueError("dtrajs is empty")
        labels = np.concatenate(trajs).astype(np.int32) if sum(t.size for t in trajs) else np.zeros(0, np.int32)
        if labels.size == 0 or labels.max() < 0:
            raise ValueError("dtrajs holds no non-negative state label")
        stops = np.cumsum([t.size for t in trajs]).astype(np.int64)
        return labels, stops - np.asarray([t.size for t in trajs], np.int64), stops, int(labels.max()) + 1

    def _rebuild_batch(self, dtrajs, n_boot: int, lag: int):
        """T [n_boot, k, k] and pi [n_boot, k] on the device, rowsum and the keep mask on the host."""
        labels, starts, stops, k = self._check_dtrajs(dtrajs)
        if int(n_boot) <= 0:
            return None, None, np.zeros((0, k), np.int64), np.zeros(0, bool), k
        mult = self._draw_multiplicities(len(starts), n_boot)
        eng = get_engine()
        T, rowsum = eng.bootstrap_transition_matrices(eng.to_device(labels), starts, stops, k, int(lag), mult)
        if k == 1:                               # one state: T = [[1]] or [[0]], pi = 1 either way (np.linalg.eig)
            return T, eng.to_device(np.ones((int(n_boot), 1))), rowsum.to_host(), np.ones(int(n_boot), bool), k
        spec = eng.spectrum(T, n_its=0, n_watch=2, allow_unconverged=True)
        pi = spec["pi"]
        keep = (np.abs(spec["ritz"][:, 1]) <= _DEGENERATE) & np.all(np.isfinite(pi.to_host()), axis=1)
        stuck = keep & ~(spec["residual"] <= 1e-9)
        if np.any(stuck):
            raise RuntimeError(f"stationary vectors of samples {np.flatnonzero(stuck).tolist()} did not converge")
        return T, pi, rowsum.to_host(), keep, k

    # -- bootstraps ----------------------------------------------------------------------------------------------
    def bootstrap_tpt(self, dtrajs: List[np.ndarray], source_states: np.ndarray, sink_states: np.ndarray,
                      n_boot: int = 200, lag: int = 1,
                      ci_percentiles: Tuple[float, float] = (2.5, 97.5)) -> Dict[str, UncertaintyResult]:
        """Mean / std / CI of the A -> B rate, mfpt and total flux over trajectory resamples; {} when every sample
        fails."""
        logger.info(f"Bootstrap TPT uncertainty with {n_boot} samples")
        role, _, _ = _roles(self._check_dtrajs(dtrajs)[3], source_states, sink_states)
        T, pi, rowsum, keep, k = self._rebuild_batch(dtrajs, n_boot, lag)
        totals = np.zeros((0, 4))
        if T is not None:
            out = get_engine().reactive_flux_batched(T, pi, role, want_committors=False)
            keep = keep & np.all(rowsum > 0, axis=1) & np.all(out["info"] == 0, axis=1)
            totals = out["totals"].to_host()[keep]
        self.last_kept = keep
        if len(totals) == 0:
            logger.warning("All bootstrap samples failed")
            return {}
        results = {}
        for name, col in (("rate", 2), ("mfpt", 3), ("total_flux", 0)):
            s = totals[:, col]
            results[name] = UncertaintyResult(name, float(np.mean(s)), float(np.std(s)),
                                              float(np.percentile(s, ci_percentiles[0])),
                                              float(np.percentile(s, ci_percentiles[1])), len(s), "bootstrap")
        logger.info(f"Bootstrap complete: rate = {results['rate'].mean:.3e} ± {results['rate'].std:.3e}")
        return results

    def bootstrap_macrostate_populations(self, dtrajs: List[np.ndarray], n_macrostates: int, n_boot: int = 200,
                                         lag: int = 1,
                                         ci_percentiles: Tuple[float, float] = (2.5, 97.5)) -> UncertaintyResult:
        """Mean / std / CI of the PCCA+ macrostate populations (argmax of the memberships, pi summed per set)."""
        logger.info(f"Bootstrap macrostate populations with {n_boot} samples")
        T, pi, _, keep, _ = self._rebuild_batch(dtrajs, n_boot, lag)
        m = int(n_macrostates)
        pops, kept = [], np.zeros(len(keep), bool)
        if T is not None and np.any(keep):
            T_h, pi_h = T.to_host(), pi.to_host()
            for b in np.flatnonzero(keep):
                try:
                    chi = pcca_memberships(T_h[b], m, pi_h[b])
                except ValueError as e:
                    logger.debug(f"Bootstrap sample {b} failed: {e}")
                    continue
                pops.append(np.bincount(np.argmax(chi, axis=1), weights=pi_h[b], minlength=m)[:m])
                kept[b] = True
        self.last_kept = kept
        return _array_result("macrostate_populations", pops, m, ci_percentiles)

    def bootstrap_free_energies(self, dtrajs: List[np.ndarray], T_K: float = 300.0, n_boot: int = 200,
                                ci_percentiles: Tuple[float, float] = (2.5, 97.5)) -> UncertaintyResult:
        """Mean / std / CI of the state free energies F = -kT ln max(pi, 1e-10) in kJ/mol, at lag 1."""
        logger.info(f"Bootstrap free energies with {n_boot} samples")
        kT = BOLTZMANN_J_PER_K * T_K * AVOGADRO_PER_MOL / 1000.0
        _, pi, _, keep, k = self._rebuild_batch(dtrajs, n_boot, 1)
        fe = []
        if pi is not None and np.any(keep):
            fe = list(-kT * np.log(np.maximum(pi.to_host()[keep], 1e-10)))
        self.last_kept = keep
        return _array_result("free_energies", fe, k, ci_percentiles)

    # -- host-only statistics ------------------------------------------------------------------------------------
    def ensemble_observable_statistics(self, ensemble_results: List[Any], observable_name: str,
                                       ci_percentiles: Tuple[float, float] = (2.5, 97.5)) -> UncertaintyResult:
        """Mean / std / CI of an observable across the members of an ensemble (uncertainty.py:318-355)."""
        if len(ensemble_results) == 0:
            return UncertaintyResult(observable_name, 0.0, 0.0, 0.0, 0.0, 0, "hyperparameter_ensemble")
        a = np.array(ensemble_results)
        return UncertaintyResult(observable_name, np.mean(a, axis=0), np.std(a, axis=0),
                                 np.percentile(a, ci_percentiles[0], axis=0), np.percentile(a, ci_percentiles[1], axis=0),
                                 len(ensemble_results), "hyperparameter_ensemble")

    def convergence_diagnostics(self, iteration_results: List[Dict[str, Any]]) -> Dict[str, Any]:
        """Relative change of the implied timescales ("its") and absolute change of the populations ("pi") between
        consecutive iterations; converged when the last changes are below 1 % and 1e-3 (uncertainty.py:357-423)."""
        if len(iteration_results) < 2:
            return {"converged": False, "reason": "insufficient_iterations"}
        its_list = [np.asarray(it["its"], dtype=float) for it in iteration_results if it.get("its") is not None]
        pi_list = [np.asarray(it["pi"], dtype=float) for it in iteration_results if it.get("pi") is not None]
        diagnostics: Dict[str, Any] = {"n_iterations": len(iteration_results)}
        if len(its_list) >= 2:
            changes = [np.mean(np.abs(b - a) / np.maximum(a, 1e-10)) for a, b in zip(its_list[:-1], its_list[1:])]
            diagnostics["its_convergence"] = {"mean_relative_change": float(np.mean(changes)),
                                              "converged": bool(changes[-1] < 0.01)}
        if len(pi_list) >= 2:
            changes = [np.mean(np.abs(b - a)) for a, b in zip(pi_list[:-1], pi_list[1:])]
            diagnostics["population_convergence"] = {"mean_absolute_change": float(np.mean(changes)),
                                                     "converged": bool(changes[-1] < 0.001)}
        converged = True
        for key in ("its_convergence", "population_convergence"):
            if key in diagnostics:
                converged = converged and diagnostics[key]["converged"]
        diagnostics["converged"] = converged
        return diagnostics
