"""Lagged index pairs of a set of trajectories: mirror of pmarlo.features.deeptica.core.pairs
(S/features/deeptica/core/pairs.py): derived pairs, the validation of given pairs with the reference's messages,
weight broadcasting and the eight diagnostics.  Host code: index arithmetic over a few integers per trajectory."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

__all__ = ["PairInfo", "build_pair_info"]


@dataclass
class PairInfo:
    idx_t: np.ndarray
    idx_tau: np.ndarray
    weights: np.ndarray
    diagnostics: dict


def _lengths(trajectories) -> list[int]:
    return [int(np.asarray(block).shape[0]) for block in trajectories]


def _uniform_pairs(lengths: Sequence[int], lag: int) -> tuple[np.ndarray, np.ndarray]:
    """Every (t, t + lag) inside a trajectory, rows counted over the concatenated trajectories."""
    if lag < 1:
        raise ValueError("Lag must be a positive integer")
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) if lengths else np.zeros(0, np.int64)
    parts = [start + np.arange(n - lag, dtype=np.int64) for start, n in zip(starts, lengths) if n > lag]
    idx_t = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return idx_t, idx_t + lag


def _check_given_pairs(idx_t: np.ndarray, idx_tau: np.ndarray, n_frames: int) -> None:
    if idx_t.shape != idx_tau.shape:
        raise ValueError("Pair index arrays must have the same shape")
    if idx_t.size == 0:
        return
    if min(idx_t.min(), idx_tau.min()) < 0:
        raise ValueError("Pair indices must be non-negative")
    if n_frames <= 0:
        raise ValueError("Pair indices provided but no trajectories are available")
    if max(idx_t.max(), idx_tau.max()) >= n_frames:
        raise ValueError("Pair indices exceed available trajectory length")
    if np.any(idx_tau <= idx_t):
        raise ValueError("Pair indices must represent positive time lags")


def build_pair_info(trajectories: Sequence[np.ndarray], tau_schedule: Sequence[int],
                    pairs: Tuple[np.ndarray, np.ndarray] | None = None, weights: np.ndarray | None = None) -> PairInfo:
    """The pairs training and its diagnostics refer to.  Given `pairs` are flattened to int64 and validated; else
    the pairs of every positive lag of the schedule are derived, lag after lag.  `weights`: one per pair, or a single
    value for all; float32 ones when absent."""
    schedule = tuple(int(t) for t in tau_schedule if int(t) > 0)
    if not schedule:
        raise ValueError("Tau schedule must contain at least one positive lag")
    lengths = _lengths(trajectories)
    if pairs is not None:
        idx_t = np.asarray(pairs[0], np.int64).reshape(-1)
        idx_tau = np.asarray(pairs[1], np.int64).reshape(-1)
        _check_given_pairs(idx_t, idx_tau, sum(lengths))
    else:
        per_lag = [_uniform_pairs(lengths, tau) for tau in schedule]
        idx_t = np.concatenate([p[0] for p in per_lag])
        idx_tau = np.concatenate([p[1] for p in per_lag])

    count = idx_t.size
    if weights is None:
        w = np.ones(count, np.float32)
    else:
        w = np.asarray(weights, np.float32).reshape(-1)
        if count == 0:
            w = w[:0]
        elif w.size == 1 and count > 1:
            w = np.full(count, w[0], np.float32)
        elif w.size != count:
            raise ValueError("weights must match the number of lagged pairs")

    max_tau = max(schedule)
    # a single lag counts its own pairs; a curriculum counts those of every lag
    possible = sum(max(0, n - tau) for tau in (schedule if len(schedule) > 1 else (max_tau,)) for n in lengths)
    bounds = np.cumsum([0, *lengths])
    usable = int(min(idx_t.size, idx_tau.size))
    diagnostics = {
        "usable_pairs": usable,
        "pair_coverage": float(usable / possible) if possible else 0.0,
        "total_possible_pairs": int(possible),
        "short_trajectories": [i for i, n in enumerate(lengths) if n <= max_tau],
        "pairs_by_trajectory": [int(np.count_nonzero((idx_t >= lo) & (idx_t < hi)))
                                for lo, hi in zip(bounds[:-1], bounds[1:])],
        "lag_used": int(max_tau),
        "expected_pairs": int(possible),
        "tau_schedule_used": list(schedule),
    }
    return PairInfo(idx_t=idx_t, idx_tau=idx_tau, weights=w, diagnostics=diagnostics)
