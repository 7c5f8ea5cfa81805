"""Collective-variable training: mirror of pmarlo.cv.train_cv_model (S/cv/__init__.py).

"tica" fits the device TICA that tica_reduce fits (standardise, lagged moments, generalised eigenproblem) and
returns it with a `.transform`; "deeptica" builds a DeepTICAConfig and goes through train_deeptica.

Stated divergences from the reference: its "tica" branch returns deeptime's model, here the device's (the same
estimator, tica_reduce's); its "deeptica" branch passes keywords DeepTICAConfig does not have and a call
train_deeptica does not accept, here lag_time and n_components become `lag` and `n_out`, the features are one
trajectory (or a list of them) and the pairs are derived from the lag."""

from __future__ import annotations

import logging
from typing import Any

import numpy as np

__all__ = ["TicaCVModel", "train_cv_model"]

logger = logging.getLogger(__name__)


class TicaCVModel:
    """A fitted device TICA with the estimator-style `.transform(features)` -> [n, dim] float64."""

    def __init__(self, pipeline, model):
        self._pipeline, self.model = pipeline, model
        self.lagtime, self.dim = model.lag, model.dim

    def transform(self, features) -> np.ndarray:
        from ..markov_state_model.reduction import _as_matrix

        eng = self._pipeline.eng
        return np.ascontiguousarray(self._pipeline.tica_transform(self.model, eng.to_device(_as_matrix(features))).to_host())


def train_cv_model(features, lag_time: int = 1, n_components: int = 2, method: str = "tica", **kwargs: Any) -> Any:
    """Train a collective-variable model on features [n_frames, n_features]; the result has `.transform(features)`.
    method "tica": keywords `scale` (default True), `epsilon`, `kinetic_map` of the device TICA; "deeptica":
    keywords are DeepTICAConfig fields, and `frame_weights` / `weights` go to train_deeptica."""
    if method == "tica":
        from ..device import get_engine
        from ..markov_state_model.reduction import _as_matrix
        from ..pipeline import MSMPipeline

        eng = get_engine()
        pipe = MSMPipeline(eng)
        model = pipe.tica_fit(eng.to_device(_as_matrix(features)), int(lag_time), int(n_components), **kwargs)
        rank = int(model.rank.to_host()[0])
        if rank == 0:
            raise ValueError("TICA: covariance matrix has zero rank")
        model.dim = min(int(n_components), rank)
        logger.info("TICA trained: %d components, lag=%d frames", n_components, lag_time)
        return TicaCVModel(pipe, model)

    if method == "deeptica":
        from ..features.deeptica import DeepTICAConfig, train_deeptica

        extra = {key: kwargs.pop(key) for key in ("weights", "frame_weights") if key in kwargs}
        config = DeepTICAConfig(lag=int(lag_time), n_out=int(n_components), **kwargs)
        trajectories = list(features) if isinstance(features, (list, tuple)) else [np.asarray(features)]
        model = train_deeptica(trajectories, None, config, **extra)
        logger.info("DeepTICA trained: %d components, lag=%d frames", n_components, lag_time)
        return model

    raise ValueError(f"Unknown CV method {method!r}. Choose 'tica' or 'deeptica'.")
