"""Per-state representative frames for the state table (S/markov_state_model/_states.py:131-157).

The reference walks every frame of every discrete trajectory once per state in Python; here the frames are
grouped by state on the device and the nearest member to the unweighted mean comes from the kernels that
RepresentativePicker uses (csrc/representatives.hip)."""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from ..conformations.representative_picker import DeviceStateGroups, build_frame_index_lookup

__all__ = ["find_representatives"]


def find_representatives(features: np.ndarray, dtrajs: Sequence[np.ndarray],
                         n_states: int) -> Tuple[List[Tuple[int, int]], List[Optional[np.ndarray]]]:
    """For every state 0 .. n_states - 1: the ``(trajectory, local frame)`` of the member nearest the state's mean
    feature vector (the lowest frame on equal distances) and that mean; ``(-1, -1)`` and ``None`` for an empty state."""
    n_states = int(n_states)
    if n_states <= 0:
        return [], []
    lookup = build_frame_index_lookup(dtrajs)
    features = np.asarray(features)
    if features.shape[0] != lookup.n_frames:
        raise ValueError(
            "Feature matrix row count does not match total number of frames "
            f"({features.shape[0]} != {lookup.n_frames})."
        )
    frames: List[Tuple[int, int]] = [(-1, -1)] * n_states
    centroids: List[Optional[np.ndarray]] = [None] * n_states
    if lookup.n_frames == 0:
        return frames, centroids
    groups = DeviceStateGroups(features, lookup.state_by_global_frame, n_states)
    occupied = [s for s in range(n_states) if groups.count(s) > 0]
    if not occupied:
        return frames, centroids
    picks = groups.select(groups.centroid_scores(), occupied, 1)
    means = groups.centroid.to_host()
    for q, s in enumerate(occupied):
        frames[s] = lookup.to_local_indices(int(picks[q, 0]))
        centroids[s] = means[s].copy()
    return frames, centroids
