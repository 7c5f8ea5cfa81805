"""Source and sink states for transition path theory: detection from a free-energy surface, from the timescale gap
with PCCA+, from populations, and the explicit ways of naming them.

Mirrors pmarlo.conformations.state_detection.StateDetector (S/conformations/state_detection.py:13-555), every public
method.  The free-energy surfaces are small 2-D grids and stay numpy / scipy.ndimage on the host;
detect_from_timescale_gap takes its memberships from markov_state_model.pcca.pcca_memberships (the dominant
eigenvectors come from the device) where the reference calls deeptime's pcca, so parity with the reference's own
sets is unpinned there as for PCCA+ itself."""

from __future__ import annotations

import logging
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from ..markov_state_model.pcca import pcca_memberships

__all__ = ["StateDetector"]

logger = logging.getLogger("pmarlo.conformations")

StatePair = Tuple[np.ndarray, np.ndarray]


class StateDetector:
    """Finds or takes the source and sink microstates of a TPT analysis."""

    def __init__(self, committor_thresholds: Tuple[float, float] = (0.05, 0.95)) -> None:
        lower, upper = committor_thresholds
        if not (0.0 <= lower < upper <= 1.0):
            raise ValueError("committor_thresholds must satisfy 0 ≤ lower < upper ≤ 1")
        self.committor_thresholds: Tuple[float, float] = (float(lower), float(upper))

    def _resolve_metastable_count(self, value: Optional[int]) -> int:
        resolved = 2 if value is None else int(value)
        if resolved < 2:
            raise ValueError("Number of metastable states must be at least 2")
        return resolved

    def _validate_state_indices(self, source_states: np.ndarray, sink_states: np.ndarray, n_msm_states: int) -> StatePair:
        """The indices below n_msm_states; ValueError when either set loses all of its members."""
        valid_source = source_states[source_states < n_msm_states]
        valid_sink = sink_states[sink_states < n_msm_states]
        if len(valid_source) == 0 or len(valid_sink) == 0:
            raise ValueError(f"Detected states are out of bounds for MSM with {n_msm_states} states. "
                             f"source={source_states.tolist()}, sink={sink_states.tolist()}")
        if len(valid_source) < len(source_states) or len(valid_sink) < len(sink_states):
            logger.warning(f"Filtered out-of-bounds states: source {len(source_states)} → {len(valid_source)}, "
                           f"sink {len(sink_states)} → {len(valid_sink)}")
        return valid_source, valid_sink

    # -- detection ---------------------------------------------------------------------------------------------------
    def auto_detect(self, T: np.ndarray, pi: np.ndarray, fes: Optional[Any] = None, its: Optional[np.ndarray] = None,
                    n_states: Optional[int] = None, method: str = "auto") -> StatePair:
        """method 'auto' tries the free-energy surface (when given, and only if its states exist in the MSM), then
        the timescale gap (when `its` is given), then the populations; a method that raises hands over to the next.
        'fes', 'timescale' and 'population' run that method alone."""
        target_states = self._resolve_metastable_count(n_states)
        n_msm_states = T.shape[0]
        if method == "auto":
            if fes is not None:
                try:
                    source, sink = self.detect_from_fes(fes, n_basins=target_states)
                    return self._validate_state_indices(source, sink, n_msm_states)
                except Exception as e:
                    logger.debug(f"FES detection failed: {e}")
            if its is not None:
                try:
                    return self.detect_from_timescale_gap(T, pi, its, n_states=target_states)
                except Exception as e:
                    logger.debug(f"Timescale gap detection failed: {e}")
            return self.detect_from_populations(pi, top_n=target_states)
        if method == "fes":
            if fes is None:
                raise ValueError("FES data required for fes method")
            return self.detect_from_fes(fes, n_basins=target_states)
        if method == "timescale":
            if its is None:
                raise ValueError("Implied timescales required for timescale method")
            return self.detect_from_timescale_gap(T, pi, its, n_states=target_states)
        if method == "population":
            return self.detect_from_populations(pi, top_n=target_states)
        raise ValueError(f"Unknown detection method: {method}. Choose from: auto, fes, timescale, population")

    def detect_from_fes(self, fes: Any, n_basins: Optional[int] = None, method: str = "watershed") -> StatePair:
        """Basins of a free-energy surface (an object with the 2-D array F).  The indices returned are flat GRID
        indices, which need not be MSM states: prefer the timescale or population methods."""
        if not hasattr(fes, "F"):
            raise ValueError("FES object must have 'F' attribute")
        F = np.asarray(fes.F)
        logger.warning("FES-based state detection may produce indices incompatible with MSM. "
                       "Consider using 'timescale' or 'population' methods instead.")
        target_basins = self._resolve_metastable_count(n_basins)
        if method == "watershed":
            return self._watershed_basins(F, target_basins)
        if method == "local_minima":
            return self._local_minima_basins(F, target_basins)
        if method == "threshold":
            return self._threshold_basins(F, target_basins)
        raise ValueError(f"Unknown FES method: {method}")

    def _watershed_basins(self, F: np.ndarray, n_basins: int) -> StatePair:
        """Connected groups of 3 x 3 local minima, the first 2 n_basins - 1 labels at most; of the n_basins deepest,
        the deepest is the source and the shallowest the sink."""
        from scipy.ndimage import label, minimum_filter

        labeled, n_labels = label(minimum_filter(F, size=3) == F)
        positions, values = [], []
        for i in range(1, min(n_labels + 1, n_basins * 2)):
            coords = np.where(labeled == i)
            if len(coords[0]) > 0:
                idx = np.argmin(F[coords])
                pos = (coords[0][idx], coords[1][idx])
                positions.append(pos)
                values.append(F[pos])
        order = np.argsort(values)[: min(n_basins, len(values))]
        if len(order) < 2:
            raise ValueError("Watershed detection found fewer than two basins")
        source_state = np.ravel_multi_index(positions[order[0]], F.shape)
        sink_state = np.ravel_multi_index(positions[order[-1]], F.shape)
        return np.array([source_state]), np.array([sink_state])

    def _local_minima_basins(self, F: np.ndarray, n_basins: int) -> StatePair:
        """The n_basins lowest grid points that lie more than max(2, rows // (2 n_basins)) apart, taken in ascending
        free energy: the first is the source, the last the sink."""
        selected: List[Tuple[int, ...]] = []
        min_distance = max(2, F.shape[0] // (n_basins * 2))
        for idx in np.argsort(F.ravel()):
            if len(selected) >= n_basins:
                break
            pos = np.unravel_index(idx, F.shape)
            if not selected or all(np.linalg.norm(np.array(pos) - np.array(s)) > min_distance for s in selected):
                selected.append(pos)
        if len(selected) < 2:
            raise ValueError("Local-minima detection found fewer than two basins")
        source_state = np.ravel_multi_index(selected[0], F.shape)
        sink_state = np.ravel_multi_index(selected[-1], F.shape)
        return np.array([source_state]), np.array([sink_state])

    def _threshold_basins(self, F: np.ndarray, n_basins: int) -> StatePair:
        """Connected regions under the 20th percentile of F: the first grid point of the largest region is the
        source, that of the second largest the sink (equal sizes keep label order)."""
        from scipy.ndimage import label

        labeled, n_labels = label(F < np.percentile(F, 20))
        if n_labels < 2:
            raise ValueError("Threshold detection found fewer than two basins")
        sizes = sorted(((i, np.sum(labeled == i)) for i in range(1, n_labels + 1)), key=lambda x: x[1], reverse=True)
        source_region, sink_region = sizes[0][0], sizes[min(1, len(sizes) - 1)][0]
        source_state = np.where((labeled == source_region).ravel())[0][0]
        sink_state = np.where((labeled == sink_region).ravel())[0][0]
        return np.array([source_state]), np.array([sink_state])

    def detect_from_timescale_gap(self, T: np.ndarray, pi: np.ndarray, its: np.ndarray, n_states: Optional[int] = None,
                                  gap_threshold: float = 2.0) -> StatePair:
        """PCCA+ sets (argmax of the memberships) of n_states macrostates: the most populated set is the source, the
        second most populated the sink.  The gap in `its` is only reported."""
        target_states = self._resolve_metastable_count(n_states)
        its = np.asarray(its)
        if len(its) < 2:
            raise ValueError("At least two implied timescales are required")
        ratios = its[:-1] / np.maximum(its[1:], 1e-10)
        gap_idx = np.argmax(ratios)
        if ratios[gap_idx] < gap_threshold:
            logger.debug(f"No clear timescale gap found (max ratio: {ratios[gap_idx]:.2f})")
        T = np.asarray(T)
        pi = np.asarray(pi)
        if target_states > T.shape[0]:
            raise ValueError("Requested number of metastable states exceeds the number of microstates")
        labels = np.argmax(pcca_memberships(T, target_states), axis=1)
        macro_states = [np.where(labels == m)[0] for m in range(target_states)]
        macro_pops = [np.sum(pi[s]) for s in macro_states]
        order = np.argsort(macro_pops)[::-1]
        return macro_states[order[0]], macro_states[order[min(1, len(order) - 1)]]

    def detect_from_populations(self, pi: np.ndarray, top_n: Optional[int] = None) -> StatePair:
        """Of the top_n most populated states, the first is the source and the last the sink."""
        n_states = self._resolve_metastable_count(top_n)
        top_states = np.argsort(pi)[::-1][:n_states]
        if len(top_states) < 2:
            raise ValueError("At least two populated states are required")
        return np.array([top_states[0]]), np.array([top_states[-1]])

    # -- explicit specification --------------------------------------------------------------------------------------
    def from_state_indices(self, source_indices: Sequence[int], sink_indices: Sequence[int]) -> StatePair:
        return np.asarray(source_indices, dtype=int), np.asarray(sink_indices, dtype=int)

    def from_cv_ranges(self, cv_data: np.ndarray, cv_name: str, source_range: Tuple[float, float],
                       sink_range: Tuple[float, float], dtrajs: Optional[List[np.ndarray]] = None) -> StatePair:
        """The states visited by the frames whose collective variable lies in the (closed) ranges; without dtrajs
        the frame indices themselves."""
        source_frames = np.where((cv_data >= source_range[0]) & (cv_data <= source_range[1]))[0]
        sink_frames = np.where((cv_data >= sink_range[0]) & (cv_data <= sink_range[1]))[0]
        if len(source_frames) == 0 or len(sink_frames) == 0:
            raise ValueError(f"No frames found in specified CV ranges for {cv_name}. "
                             f"Source: {source_range}, Sink: {sink_range}")
        if dtrajs is None:
            return source_frames, sink_frames
        states = np.concatenate(dtrajs)
        source_states, sink_states = np.unique(states[source_frames]), np.unique(states[sink_frames])
        logger.info(f"CV-based detection for {cv_name}: {len(source_states)} source states, "
                    f"{len(sink_states)} sink states")
        return source_states, sink_states

    def classify_committor_states(self, committors: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(source-like, sink-like, transition) microstates: q <= lower, q >= upper, strictly between."""
        values = np.asarray(committors, dtype=float)
        if values.ndim != 1:
            raise ValueError("committors array must be one-dimensional")
        lower, upper = self.committor_thresholds
        return (np.where(values <= lower)[0], np.where(values >= upper)[0],
                np.where((values > lower) & (values < upper))[0])

    def from_frame_indices(self, source_frames: Sequence[int], sink_frames: Sequence[int],
                           dtrajs: List[np.ndarray]) -> StatePair:
        """The states of the given global frames."""
        states = np.concatenate(dtrajs)
        return np.unique(states[list(source_frames)]), np.unique(states[list(sink_frames)])

    def from_macrostate_labels(self, macrostate_labels: np.ndarray, source_id: int, sink_id: int) -> StatePair:
        """The microstates of two macrostates."""
        source_states = np.where(macrostate_labels == source_id)[0]
        sink_states = np.where(macrostate_labels == sink_id)[0]
        if len(source_states) == 0 or len(sink_states) == 0:
            raise ValueError(f"No states found for macrostate IDs {source_id} or {sink_id}")
        return source_states, sink_states
