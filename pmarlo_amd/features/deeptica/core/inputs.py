"""Features ready for DeepTICA training: mirror of pmarlo.features.deeptica.core.inputs
(S/features/deeptica/core/inputs.py).  The frames are concatenated as float32 and uploaded once; the scaler is
sklearn's StandardScaler restated on Engine.column_moments (population statistics, a constant column gets scale 1).
No standardised copy Z is kept: the network kernels standardise as they read (msm_mlp_forward)."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Iterable, Sequence

import numpy as np

__all__ = ["FeaturePrep", "prepare_features"]


@dataclass
class FeaturePrep:
    X: np.ndarray                  # [n, F] float32, the concatenated frames (host)
    x_device: Any                  # the same frames on the device
    mean: np.ndarray               # [F] float64, StandardScaler.mean_
    scale: np.ndarray              # [F] float64, StandardScaler.scale_
    tau_schedule: tuple[int, ...]
    input_dim: int
    seed: int


def prepare_features(arrays: Iterable[np.ndarray], *, tau_schedule: Sequence[int], seed: int, engine=None) -> FeaturePrep:
    blocks = [np.asarray(block, np.float32) for block in arrays]
    if not blocks:
        raise ValueError("Expected at least one trajectory array for DeepTICA")
    schedule = tuple(int(t) for t in tau_schedule if int(t) > 0)
    if not schedule:
        raise ValueError("Tau schedule must contain at least one positive lag")
    X = np.ascontiguousarray(np.concatenate(blocks, axis=0))
    if X.ndim != 2:
        raise ValueError(f"trajectory arrays must be 2-D, got concatenated shape {X.shape}")
    if engine is None:
        from ....device import get_engine

        engine = get_engine()
    xd = engine.to_device(X)
    mean_d, std_d, count_d = engine.column_moments(xd, ddof=0)
    if np.any(count_d.to_host() != X.shape[0]):
        raise ValueError("Input X contains NaN.")          # column_moments skips NaN entries; StandardScaler refuses
    mean, std = mean_d.to_host(), std_d.to_host()
    if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std))):
        raise ValueError("Input X contains infinity or a value too large for dtype('float64').")
    # StandardScaler's constant column (_is_constant_feature): a variance within the rounding bound of the two-pass
    # algorithm, zero included, gets scale 1
    n, eps, var = X.shape[0], np.finfo(np.float64).eps, std * std
    scale = np.where(var <= n * eps * var + (n * mean * eps) ** 2, 1.0, std)
    return FeaturePrep(X=X, x_device=xd, mean=mean, scale=scale, tau_schedule=schedule, input_dim=int(X.shape[1]),
                       seed=int(seed))
