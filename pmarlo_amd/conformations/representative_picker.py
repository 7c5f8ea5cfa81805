"""Representative frames of conformational states, picked on the device.

The interface of pmarlo.conformations.representative_picker (S/conformations/representative_picker.py):
``RepresentativePicker.pick_representatives`` returns ``(state, global_frame, trajectory_index,
local_frame)`` tuples for ``closest_to_centroid`` (alias ``centroid``), ``true_medoid`` and ``diverse``, with
the reference's error messages.  The reference loops over states on the host and, for the medoid, over the
members of a state; here features and labels go to the device once, the frames are grouped by state
(np.where order), and centroids, scores and the selection are kernels (csrc/representatives.hip).  Only the
group offsets, the weight flags and the picks come back.

Deviations (representative frames): with ``n_reps > 1`` the two smallest-n methods return a
state's picks in ascending (score, frame) order, where the reference returns whatever np.argpartition leaves
(the same set); equal scores go to the lowest frame; a negative state id has no frames."""

from __future__ import annotations

import logging
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .. import _lib

logger = logging.getLogger("pmarlo_amd.conformations")

__all__ = ["TrajectorySegment", "TrajectoryFrameLocator", "FrameIndexLookup", "build_frame_index_lookup",
           "RepresentativeFrame", "RepresentativePicker", "DeviceStateGroups"]

RepresentativeFrame = Tuple[int, int, int, int]


@dataclass(frozen=True)
class TrajectorySegment:
    """Global frames [start, stop) live in `path`, at local_start + (g - start) * local_stride."""

    path: Path
    start: int
    stop: int
    local_start: int
    local_stride: int = 1

    def __post_init__(self) -> None:
        if self.local_stride <= 0:
            raise ValueError("TrajectorySegment.local_stride must be positive")

    def contains(self, global_frame: int) -> bool:
        return self.start <= global_frame < self.stop

    def to_local(self, global_frame: int) -> int:
        return self.local_start + (global_frame - self.start) * self.local_stride


@dataclass(frozen=True)
class TrajectoryFrameLocator:
    """Global frame index -> (trajectory file, frame index in that file)."""

    segments: Tuple[TrajectorySegment, ...]

    def resolve(self, global_frame: int) -> Tuple[Path, int]:
        for seg in self.segments:
            if seg.contains(global_frame):
                return seg.path, seg.to_local(global_frame)
        raise IndexError(f"Global frame {global_frame} does not map to any known trajectory segment")


@dataclass(frozen=True)
class FrameIndexLookup:
    """Per global frame: its state, its trajectory and its index in that trajectory."""

    state_by_global_frame: np.ndarray
    trajectory_index: np.ndarray
    local_frame_index: np.ndarray

    def frames_for_state(self, state_id: int) -> np.ndarray:
        return np.where(self.state_by_global_frame == state_id)[0]

    def to_local_indices(self, global_frame: int) -> Tuple[int, int]:
        if global_frame < 0 or global_frame >= len(self.trajectory_index):
            raise IndexError(
                f"Global frame index {global_frame} is out of bounds for lookup of length "
                f"{len(self.trajectory_index)}."
            )
        return int(self.trajectory_index[global_frame]), int(self.local_frame_index[global_frame])

    @property
    def n_frames(self) -> int:
        return int(self.state_by_global_frame.size)


def build_frame_index_lookup(dtrajs: Sequence[np.ndarray]) -> FrameIndexLookup:
    """Concatenate the discrete trajectories and remember where every frame came from."""
    if not isinstance(dtrajs, Iterable) or not dtrajs:
        raise ValueError("dtrajs must be a non-empty sequence of arrays")
    arrays = [np.asarray(dt) for dt in dtrajs]
    if any(a.ndim != 1 for a in arrays):
        raise ValueError("Each discrete trajectory must be one-dimensional")
    lengths = [a.size for a in arrays]
    traj = np.repeat(np.arange(len(arrays), dtype=int), lengths)
    starts = np.repeat(np.cumsum([0] + lengths[:-1]), lengths)
    return FrameIndexLookup(np.concatenate(arrays), traj, np.arange(sum(lengths), dtype=int) - starts)


def _labels_int32(states: np.ndarray) -> np.ndarray:
    """int32 labels for the device; values that do not fit (or are not integers) become -1: no state."""
    s = np.asarray(states)
    if s.dtype.kind not in "iu":
        r = np.rint(np.nan_to_num(s.astype(np.float64), nan=-1.0, posinf=-1.0, neginf=-1.0))
        s = np.where(r == s, r, -1.0)
    fits = (s >= 0) & (s <= np.iinfo(np.int32).max)
    return np.where(fits, s, -1).astype(np.int32)


class DeviceStateGroups:
    """Features, labels and weights on the device, grouped by state; centroids, scores and picks from the kernels.

    One upload per instance.  ``offsets`` (host, int64 [k + 1]), ``flags`` and ``wsum`` (host, per state) are the
    only tables read back by the constructor."""

    def __init__(self, features: np.ndarray, labels: np.ndarray, k: int, weights: Optional[np.ndarray] = None,
                 engine=None):
        from ..device import get_engine

        x = np.asarray(features, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("features must be two-dimensional (n_frames x n_features)")
        if x.shape[1] > _lib.REP_MAX_D:
            raise NotImplementedError(f"representative picking supports at most {_lib.REP_MAX_D} features, "
                                      f"got {x.shape[1]}")
        if x.shape[1] < 1:
            raise ValueError("features must have at least one column")
        self.eng = engine or get_engine()
        self.k = int(k)
        self.x = self.eng.to_device(x)
        self.labels = self.eng.to_device(_labels_int32(labels))
        self.w = None if weights is None else self.eng.to_device(np.asarray(weights, dtype=np.float64))
        self.d_offsets, self.members = self.eng.group_by_label(self.labels, self.k)
        self.centroid, self.d_wsum, d_flags = self.eng.state_centroids(self.x, self.d_offsets, self.members, self.w)
        self.offsets = self.d_offsets.to_host()
        self.flags = d_flags.to_host()
        self.wsum = self.d_wsum.to_host()

    def count(self, state: int) -> int:
        return int(self.offsets[state + 1] - self.offsets[state]) if 0 <= state < self.k else 0

    def centroid_scores(self):
        return self.eng.state_scores(self.x, self.labels, self.d_offsets, self.members, self.offsets,
                                     centroid=self.centroid)

    def medoid_scores(self, states):
        return self.eng.state_scores(self.x, self.labels, self.d_offsets, self.members, self.offsets, wsum=self.d_wsum,
                                     weights=self.w, states=states)

    def select(self, scores, states, n_reps: int, diverse: bool = False) -> np.ndarray:
        return self.eng.state_select(self.x, self.d_offsets, self.members, scores, states, n_reps, diverse=diverse)

    def state_scores_host(self, scores, states) -> dict:
        host = scores.to_host()
        return {int(s): host[self.offsets[s]:self.offsets[s + 1]].copy() for s in states}


_METHODS = {"closest_to_centroid": "centroid", "centroid": "centroid", "true_medoid": "medoid", "diverse": "diverse"}


class RepresentativePicker:
    """Select representative frames of conformational states."""

    def __init__(self) -> None:
        pass

    def pick_representatives(
        self,
        features: np.ndarray,
        dtrajs: List[np.ndarray],
        state_ids: Sequence[int],
        weights: Optional[np.ndarray] = None,
        n_reps: int = 1,
        method: str = "closest_to_centroid",
        *,
        return_scores: bool = False,
    ):
        """``(state_id, global_frame_index, trajectory_index, local_frame_index)`` for every pick, state by state
        in the order of ``state_ids`` (a repeated id returns its picks again).

        ``return_scores=True`` (this engine's extension) returns ``(representatives, scores)`` with ``scores[s]`` the
        fp64 score of every member of state ``s`` in frame order: the distance to the weighted centroid
        (``closest_to_centroid``, ``centroid``, ``diverse``) or the weighted mean distance to the members
        (``true_medoid``)."""
        lookup = build_frame_index_lookup(dtrajs)
        features = np.asarray(features)
        if features.shape[0] != lookup.n_frames:
            raise ValueError(
                "Feature matrix row count does not match total number of frames "
                f"({features.shape[0]} != {lookup.n_frames})."
            )
        if weights is not None:
            weights = np.asarray(weights)
            if weights.shape[0] != lookup.n_frames:
                raise ValueError(
                    "Weights vector length does not match total number of frames "
                    f"({weights.shape[0]} != {lookup.n_frames})."
                )
        if method == "medoid":
            raise ValueError(
                "Method 'medoid' has been renamed. Use 'closest_to_centroid' for the "
                "previous behavior or 'true_medoid' for medoid selection."
            )
        if method not in _METHODS:
            raise ValueError(f"Unknown method: {method}")
        kind = _METHODS[method]
        states = [int(s) for s in state_ids]
        n_reps = int(n_reps)
        empty = ([], {}) if return_scores else []
        if not states:
            return empty
        if lookup.n_frames == 0 or max(states) < 0:
            raise ValueError(f"No frames found for state {states[0]}")

        groups = DeviceStateGroups(features, lookup.state_by_global_frame, max(states) + 1, weights)
        # the reference handles state after state: the first state at fault, in the order given, raises
        for s in states:
            if groups.count(s) == 0:
                raise ValueError(f"No frames found for state {s}")
            if kind == "diverse" and n_reps <= 0:
                continue   # the reference leaves the state before it looks at the weights
            fl = int(groups.flags[s])
            if fl & _lib.REP_FLAG_NONFINITE:
                raise ValueError(f"Non-finite weights for state {s}")
            if fl & _lib.REP_FLAG_NEGATIVE:
                raise ValueError(f"Negative weights for state {s}")
            if fl & _lib.REP_FLAG_NONPOSITIVE_SUM:
                raise ValueError(f"Non-positive weight sum for state {s}: {float(groups.wsum[s])}")
        if n_reps <= 0:
            return empty

        unique = sorted(set(states))
        scores = groups.medoid_scores(unique) if kind == "medoid" else groups.centroid_scores()
        picks = groups.select(scores, unique, n_reps, diverse=kind == "diverse")
        row = {s: picks[q] for q, s in enumerate(unique)}
        representatives: List[RepresentativeFrame] = []
        for s in states:
            for g in row[s]:
                if g < 0:
                    break
                traj_idx, local = lookup.to_local_indices(int(g))
                representatives.append((s, int(g), traj_idx, local))
        logger.info("Selected %d representatives", len(representatives))
        if return_scores:
            return representatives, groups.state_scores_host(scores, unique)
        return representatives

    def pick_from_committor_range(
        self,
        committor: np.ndarray,
        features: np.ndarray,
        dtrajs: List[np.ndarray],
        committor_range: Tuple[float, float] = (0.4, 0.6),
        n_reps: int = 5,
        weights: Optional[np.ndarray] = None,
    ) -> List[RepresentativeFrame]:
        """Diverse representatives of the states whose committor lies in ``committor_range`` (closed)."""
        q = np.asarray(committor)
        ts_states = np.where((q >= committor_range[0]) & (q <= committor_range[1]))[0]
        if len(ts_states) == 0:
            raise ValueError(f"No states found in committor range {committor_range}")
        logger.info("Found %d transition states in committor range %s", len(ts_states), committor_range)
        return self.pick_representatives(features, dtrajs, ts_states, weights=weights, n_reps=n_reps, method="diverse")

    def pick_from_flux(
        self,
        flux_matrix: np.ndarray,
        features: np.ndarray,
        dtrajs: List[np.ndarray],
        top_n: int = 10,
        n_reps_per_state: int = 1,
        weights: Optional[np.ndarray] = None,
    ) -> List[RepresentativeFrame]:
        """Representatives of the ``top_n`` states that carry the most flux (half of inflow plus outflow)."""
        F = np.asarray(flux_matrix)
        through = 0.5 * (np.sum(F, axis=1) + np.sum(F, axis=0))
        bottlenecks = np.argsort(through)[::-1][:top_n]
        logger.info("Selecting from top %d bottleneck states", top_n)
        return self.pick_representatives(features, dtrajs, bottlenecks, weights=weights, n_reps=n_reps_per_state,
                                         method="closest_to_centroid")

    def extract_structures(
        self,
        representatives: List[RepresentativeFrame],
        trajectories: Any,
        output_dir: str,
        prefix: str = "state",
        *,
        topology_path: str | Path | None = None,
        trajectory_locator: TrajectoryFrameLocator | None = None,
    ) -> List[str]:
        """Write one PDB file per representative, ``{prefix}_{state:03d}_{global:06d}.pdb``; returns the paths.

        With a ``trajectory_locator`` the frame is read from its DCD file through pmarlo_amd.io (the topology from
        ``topology_path``, a PDB file); otherwise ``trajectories[traj][local]`` must offer ``save_pdb``."""
        out_dir = Path(output_dir)
        out_dir.mkdir(parents=True, exist_ok=True)
        saved: List[str] = []

        if trajectory_locator is not None:
            if topology_path is None:
                raise ValueError("topology_path is required when extracting structures from raw trajectories")
            top_path = Path(topology_path).resolve()
            if not top_path.exists():
                raise FileNotFoundError(
                    f"Topology file {top_path} required for representative extraction does not exist"
                )
            from ..io import DCDFile, Trajectory, load_pdb

            topology = load_pdb(top_path).topology
            for state_id, global_idx, _traj, _local in representatives:
                traj_path, frame_index = trajectory_locator.resolve(global_idx)
                if not Path(traj_path).exists():
                    raise FileNotFoundError(f"Trajectory file {traj_path} does not exist for state {state_id}")
                xyz, _ = DCDFile(traj_path).read(int(frame_index), int(frame_index) + 1)
                if xyz.shape[0] != 1:
                    raise IndexError(f"Frame {frame_index} is out of bounds for trajectory file {traj_path}")
                target = out_dir / f"{prefix}_{state_id:03d}_{global_idx:06d}.pdb"
                Trajectory(xyz, topology).save_pdb(str(target))
                saved.append(str(target))
            logger.info("Saved %d structures to %s", len(saved), output_dir)
            return saved

        if not isinstance(trajectories, list):
            trajectories = [trajectories]
        for state_id, global_idx, traj_idx, local_idx in representatives:
            if traj_idx is None:
                raise ValueError(f"Representative for state {state_id} is missing trajectory index")
            if traj_idx < 0 or traj_idx >= len(trajectories):
                raise IndexError(f"Trajectory index {traj_idx} is out of bounds for state {state_id}")
            traj = trajectories[traj_idx]
            if local_idx is None:
                raise ValueError(f"Representative for state {state_id} is missing local frame index")
            if local_idx < 0 or local_idx >= len(traj):
                raise IndexError(f"Local frame {local_idx} out of bounds for trajectory {traj_idx}")
            target = out_dir / f"{prefix}_{state_id:03d}_{global_idx:06d}.pdb"
            traj[local_idx].save_pdb(str(target))
            saved.append(str(target))
        logger.info("Saved %d structures to %s", len(saved), output_dir)
        return saved
