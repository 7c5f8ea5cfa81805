"""Transition path theory of one source / sink pair, pathways included, on the device.

Mirrors pmarlo.conformations.tpt_analysis.TPTAnalysis (S/conformations/tpt_analysis.py:34-395).  The reference builds
a deeptime MarkovStateModel and asks it for reactive_flux(A, B) and flux.pathways(fraction, maxiter); here analyze is
one Engine.reactive_flux (committors, gross and net flux, totals: msm_reactive_flux) followed by
Engine.reactive_pathways on the net flux where it lies in device memory (msm_reactive_pathways_*: resumable
max-min Dijkstra, bounded launches).  Only the first n_paths node lists come back; the capacities of all paths do.

The other methods are thin calls to markov_state_model/tpt.py, which already holds their numerics.

Parity: deeptime 0.4.5 is absent, so parity with the reference's own output is unpinned, for the pathways in
particular: the widest path is unique only in its bottleneck, and deeptime recurses on both sides of the bottleneck
edge while this engine takes one max-min Dijkstra with ties to the lowest index.  The tests hold analyze to
markov_state_model.tpt.reactive_flux and pathway_decomposition, bit for bit."""

from __future__ import annotations

import logging
from typing import Any, List, Tuple

import numpy as np

from .. import _lib
from ..device import get_engine
from ..markov_state_model import tpt as _tpt
from .results import TPTResult

__all__ = ["TPTAnalysis", "PATHWAY_MAX_ITERATIONS"]

logger = logging.getLogger("pmarlo.conformations")

# ceiling on the number of paths the decomposition may take (the reference raises deeptime's default of 1000)
PATHWAY_MAX_ITERATIONS = 10_000


def _unique_disjoint(source_states, sink_states) -> Tuple[list, list]:
    source = np.unique(source_states).astype(int).tolist()
    sink = np.unique(sink_states).astype(int).tolist()
    if len(set(source) & set(sink)) > 0:
        raise ValueError("Source and sink states must not overlap")
    return source, sink


class TPTAnalysis:
    """Committors, reactive flux, rate and dominant pathways between a source and a sink set of an MSM."""

    def __init__(self, T: np.ndarray, pi: np.ndarray) -> None:
        self.T = np.asarray(T, dtype=float)
        self.pi = np.asarray(pi, dtype=float)
        if self.T.ndim != 2 or self.T.shape[0] != self.T.shape[1]:
            raise ValueError("Transition matrix must be square")
        self.n_states = self.T.shape[0]
        if len(self.pi) != self.n_states:
            raise ValueError("Stationary distribution length must match T dimensions")

    def analyze(self, source_states: np.ndarray, sink_states: np.ndarray, n_paths: int = 5,
                pathway_fraction: float = 0.99) -> TPTResult:
        """The whole analysis; pathways holds the first n_paths paths, pathway_iterations the number found."""
        logger.info(f"Running TPT analysis: {len(source_states)} source states, {len(sink_states)} sink states")
        source, sink = _unique_disjoint(source_states, sink_states)
        T = _tpt._check_T(self.T)
        role, source, sink = _tpt._roles(self.n_states, source, sink)
        eng = get_engine()
        out = eng.reactive_flux(eng.to_device(T), eng.to_device(np.ascontiguousarray(self.pi, np.float64)), role)
        if np.any(out["info"] != 0):
            raise np.linalg.LinAlgError("committor system is singular (disconnected transition matrix?)")
        totals = out["totals"].to_host()
        flux_matrix = out["gross"].to_host()
        total_flux, rate, mfpt = float(totals[0]), float(totals[2]), float(totals[3])

        # the net flux stays where reactive_flux left it: no host round trip before the walk
        pathways, caps, status = eng.reactive_pathways(out["net"], role, fraction=pathway_fraction,
                                                       maxiter=PATHWAY_MAX_ITERATIONS, keep=max(0, int(n_paths)))
        pathway_iterations = int(len(caps))
        tpt_converged = status != _lib.PATHWAYS_MAXITER
        if not tpt_converged:
            logger.warning("TPT pathway extraction failed to converge after %d iterations (max %d)",
                           pathway_iterations, PATHWAY_MAX_ITERATIONS)
        bottleneck_states = self.find_bottleneck_states(flux_matrix, top_n=10)
        logger.info(f"TPT complete: rate={rate:.3e}, MFPT={mfpt:.1f}, total_flux={total_flux:.3e}, "
                    f"n_pathways={len(pathways)}")
        return TPTResult(
            source_states=np.array(source, dtype=int), sink_states=np.array(sink, dtype=int),
            forward_committor=out["qplus"].to_host(), backward_committor=out["qminus"].to_host(),
            flux_matrix=flux_matrix, net_flux=out["net"].to_host(), total_flux=total_flux, rate=rate, mfpt=mfpt,
            pathways=[list(map(int, p)) for p in pathways],
            pathway_fluxes=np.asarray(caps[:len(pathways)], dtype=float), bottleneck_states=bottleneck_states,
            tpt_converged=tpt_converged, pathway_iterations=pathway_iterations,
            pathway_max_iterations=PATHWAY_MAX_ITERATIONS)

    def compute_committor(self, source_states: np.ndarray, sink_states: np.ndarray, forward: bool = True) -> np.ndarray:
        """q+ (forward) or q- of every state."""
        source, sink = _unique_disjoint(source_states, sink_states)
        return _tpt.compute_committor(self.T, source, sink, forward=forward, stationary_distribution=self.pi)

    def compute_reactive_flux_direct(self, source_states: np.ndarray,
                                     sink_states: np.ndarray) -> Tuple[np.ndarray, np.ndarray, float]:
        """(gross flux, net flux, total flux)."""
        source, sink = _unique_disjoint(source_states, sink_states)
        flux = _tpt.reactive_flux(self.T, self.pi, source, sink)
        logger.debug(f"Total reactive flux: {flux.total_flux:.6e}")
        return flux.gross_flux, flux.net_flux, float(flux.total_flux)

    def coarse_grain_flux(self, source_states: np.ndarray, sink_states: np.ndarray,
                          sets: List[List[int]]) -> Tuple[List[set], Any]:
        """(sets split into source / intermediate / sink parts, the reactive flux between them)."""
        source, sink = _unique_disjoint(source_states, sink_states)
        return _tpt.coarse_grain_flux(self.T, self.pi, source, sink, sets)

    def find_bottleneck_states(self, flux_matrix: np.ndarray, top_n: int = 10) -> np.ndarray:
        """The top_n states by flux through them, half of inflow plus outflow, descending."""
        F = np.asarray(flux_matrix)
        through = 0.5 * (np.sum(F, axis=1) + np.sum(F, axis=0))
        return np.argsort(through)[::-1][:top_n]

    def identify_transition_state_ensemble(self, committor: np.ndarray, tolerance: float = 0.1) -> np.ndarray:
        """States whose forward committor lies within `tolerance` of one half (bounds included)."""
        q = np.asarray(committor)
        lower, upper = 0.5 - tolerance, 0.5 + tolerance
        ts_states = np.where((q >= lower) & (q <= upper))[0]
        logger.info(f"Identified {len(ts_states)} transition state(s) with committor in [{lower:.2f}, {upper:.2f}]")
        return ts_states

    def pathway_statistics(self, pathways: List[List[int]], pathway_fluxes: np.ndarray) -> List[dict]:
        """Per pathway: length, flux and its share of the listed fluxes, the states, -ln pi along them (kT = 1) and
        the highest of these above the first state's."""
        if len(pathways) == 0:
            return []
        total = np.sum(pathway_fluxes) if len(pathway_fluxes) > 0 else 1.0
        statistics = []
        for i, (path, flux) in enumerate(zip(pathways, pathway_fluxes)):
            fe = [float(-np.log(self.pi[s])) if self.pi[s] > 0 else np.inf for s in path]
            statistics.append({
                "pathway_id": i,
                "length": len(path),
                "flux": float(flux),
                "flux_fraction": float(flux / total) if total > 0 else 0.0,
                "states": path,
                "free_energies": fe,
                "max_barrier": float(np.max(fe) - fe[0]) if len(fe) > 0 else 0.0,
            })
        return statistics
