"""train_deeptica: the training pipeline users call, mirror of pmarlo.features.deeptica.train_deeptica
(S/features/deeptica/_full.py:601-624) over the orchestration of S/features/deeptica/core/trainer_api.py:94-338.

The steps, in the reference's order: prepare the features (one upload, scaler from device column moments), build the
network, derive and validate the lagged pairs, score the untrained network (vamp2_before), map the configuration onto
the curriculum trainer's, fit, then finalise: whitening block (computed, not applied), vamp2_after, output variance,
top eigenvalues, pair diagnostics and the echo of the pair weights, all added to the history the model carries.

Stated divergences from the reference:
  * every trainer_backend name trains with the device curriculum trainer (DeepTICACurriculumTrainer); the mlcolvar
    and deeptime backends do not exist, and history_source is "curriculum_trainer" whatever the name;
  * the initial weights are DeepTICAModel.initialize's (numpy's stream, not torch's) unless `initial_state` gives
    them; batch order and dropout masks are the device trainer's (trainer.py's docstring);
  * the network is evaluated in fp64 on the fp32-rounded standardised frames (the reference forwards in fp32), so
    vamp2_before / vamp2_after and the whitening block agree with the reference's to about 1e-6, not to the bit;
  * the whitening block's covariance is sklearn's ShrunkCovariance(shrinkage, assume_centered=True) restated in
    numpy on the n_out x n_out matrix: (1 - s) X'X / n + s tr(X'X / n) / n_out I;
  * summary, checkpoint and metrics files are not written, so the history has no metrics_csv, best_checkpoint or
    summary_dir;
  * `frame_weights` (below) is this engine's addition."""

from __future__ import annotations

import dataclasses
import logging
import time
from typing import Any, Mapping, Optional, Sequence, Tuple

import numpy as np

from .config import TRAINING_BACKENDS
from .core.history import vamp2_proxy
from .core.inputs import prepare_features
from .core.pairs import build_pair_info
from .core.trainer_api import estimate_top_eigenvalues
from .model import DeepTICAModel
from .trainer import CurriculumConfig, DeepTICACurriculumTrainer

__all__ = ["curriculum_config", "output_whitening_info", "shrunk_covariance", "train_deeptica"]

logger = logging.getLogger(__name__)

_TINY, _EIGEN_CLIP, _RIDGE_SCALE, _EIGEN_FLOOR, _SHRINKAGE = 1e-12, 1e-8, 1e-5, 1e-4, 0.02   # S/constants.py, core/model.py:33


def _config_dict(cfg: Any) -> dict:
    if dataclasses.is_dataclass(cfg) and not isinstance(cfg, type):
        return dataclasses.asdict(cfg)
    if isinstance(cfg, Mapping):
        return dict(cfg)
    return dict(vars(cfg))


def curriculum_config(cfg: Any, tau_schedule: Sequence[int]) -> CurriculumConfig:
    """The curriculum trainer's configuration for a DeepTICAConfig (or any object with its attributes), by the
    mapping of _build_curriculum_config (trainer_api.py:543-608): sorted distinct positive lags, val_frac outside
    (0, 1) becomes 0.1, a clip or a batch cap that is not positive becomes None, shuffling on."""
    get = lambda name, default: getattr(cfg, name, default)        # noqa: E731
    schedule = tuple(sorted({int(t) for t in tau_schedule if int(t) > 0})) or (int(tau_schedule[-1]),)
    val_frac = float(get("val_frac", 0.1))
    clip = get("gradient_clip_val", None)
    clip = float(clip) if clip is not None and float(clip) > 0 else None
    cap = get("batches_per_epoch", None)
    cap = int(cap) if cap is not None and int(cap) > 0 else None
    return CurriculumConfig(
        tau_schedule=schedule,
        val_tau=int(get("val_tau", 0) or schedule[-1]),
        epochs_per_tau=max(1, int(get("epochs_per_tau", 15))),
        warmup_epochs=max(0, int(get("warmup_epochs", 5))),
        batch_size=max(1, int(get("batch_size", 256))),
        learning_rate=float(get("learning_rate", 3e-4)),
        weight_decay=max(0.0, float(get("weight_decay", 1e-4))),
        val_fraction=val_frac if 0.0 < val_frac < 1.0 else 0.1,
        shuffle=True,
        grad_clip_norm=clip,
        log_every=max(1, int(get("log_every", 1))),
        vamp_eps=float(get("vamp_eps", 1e-3)),
        vamp_eps_abs=float(get("vamp_eps_abs", 1e-6)),
        vamp_alpha=float(get("vamp_alpha", 0.15)),
        vamp_cond_reg=max(0.0, float(get("vamp_cond_reg", 1e-4))),
        seed=int(get("seed", 0)),
        max_batches_per_epoch=cap)


def shrunk_covariance(centred: np.ndarray, shrinkage: float = _SHRINKAGE) -> np.ndarray:
    """_estimate_covariance (core/model.py:294-320): the shrunk covariance of centred samples [n, d], symmetrised,
    plus a ridge of 1e-5 of its mean diagonal; the identity for a single sample."""
    x = np.asarray(centred, np.float64)
    if x.size == 0:
        return np.eye(0)
    n, d = x.shape
    if n <= 1:
        return np.eye(d)
    emp = x.T @ x / n
    cov = (1.0 - shrinkage) * emp + shrinkage * (np.trace(emp) / d) * np.eye(d)
    cov = 0.5 * (cov + cov.T)
    return cov + np.eye(d) * (max(float(np.trace(cov)), _TINY) / d * _RIDGE_SCALE)


def output_whitening_info(outputs: np.ndarray, idx_tau: np.ndarray | None = None, *, eig_floor: float = _EIGEN_FLOOR) -> dict:
    """The whitening block of apply_output_whitening with apply=False (core/model.py:152-212) from the network's
    outputs [n, n_out] on all frames: their mean, the inverse square root of their shrunk covariance (eigenvalues
    clipped at max(eig_floor, 1e-8)) as `transform`, its condition number, the sample variances, and the same two
    figures for the outputs at the tau frames, centred with the mean of all frames.  Nothing is applied."""
    outputs = np.asarray(outputs, np.float64)
    if outputs.size == 0:
        return {"output_variance": [], "var_zt": [], "cond_c00": None, "cond_ctt": None, "mean": [], "transform": [],
                "transform_applied": False}
    floor = max(float(eig_floor), _EIGEN_CLIP)
    mean = outputs.mean(axis=0)
    centred = outputs - mean
    lam, vec = np.linalg.eigh(shrunk_covariance(centred))
    lam = np.clip(lam, floor, None)
    transform = (vec / np.sqrt(lam)) @ vec.T
    variance = centred.var(axis=0, ddof=1).tolist()
    var_zt, cond_ctt = variance, None
    if idx_tau is not None and np.size(idx_tau):
        tau_centred = outputs[np.asarray(idx_tau, np.int64)] - mean
        var_zt = tau_centred.var(axis=0, ddof=1).tolist()
        lam_t = np.clip(np.linalg.eigvalsh(shrunk_covariance(tau_centred)), floor, None)
        cond_ctt = float(lam_t.max() / lam_t.min())
    return {"output_variance": variance, "var_zt": var_zt, "cond_c00": float(lam.max() / lam.min()), "cond_ctt": cond_ctt,
            "mean": mean.tolist(), "transform": transform.tolist(), "transform_applied": False}


def _tau_schedule_of(cfg: Any) -> tuple[int, ...]:
    schedule = tuple(int(t) for t in (getattr(cfg, "tau_schedule", ()) or ()) if int(t) > 0)
    if schedule:
        return schedule
    lag = int(getattr(cfg, "lag", 0) or 0)
    if lag <= 0:
        raise ValueError("DeepTICA configuration must define a positive lag")
    return (lag,)


def _log_pairs(diag: Mapping[str, Any], n_trajectories: int) -> None:
    usable, total, lag = int(diag["usable_pairs"]), int(diag["total_possible_pairs"]), int(diag["lag_used"])
    short = list(diag["short_trajectories"])
    if short:
        logger.warning("%d/%d trajectories too short for lag %d", len(short), n_trajectories, lag)
    if usable == 0:
        logger.warning("No usable lagged pairs remain after constructing curriculum with lag %d", lag)
    elif diag["pair_coverage"] < 0.5:
        logger.warning("Lagged pair coverage low: %.1f%% (%d/%d possible pairs)", 100.0 * diag["pair_coverage"], usable,
                       total)
    else:
        logger.info("Lagged pair diagnostics: usable=%d coverage=%.1f%% short_trajectories=%s", usable,
                    100.0 * diag["pair_coverage"], short)


def train_deeptica(X_list: Sequence[np.ndarray], pairs: Optional[Tuple[np.ndarray, np.ndarray]], cfg: Any,
                   weights: Optional[np.ndarray] = None, *, frame_weights: Optional[Sequence[np.ndarray]] = None,
                   initial_state: Optional[Mapping[str, np.ndarray]] = None, engine=None) -> DeepTICAModel:
    """Train a DeepTICA network on the trajectories X_list (one [n_i, F] array each) and return the DeepTICAModel,
    its training_history completed as the reference's train_deeptica completes it.

    pairs: (idx_t, idx_tau) into the concatenated frames, or None to derive the pairs of cfg's lags.  As in the
        reference they feed vamp2_before / vamp2_after, top_eigenvalues and the diagnostics; the curriculum draws
        its own (t, t + tau) pairs inside each trajectory.
    cfg: a DeepTICAConfig (or any object with its attributes).
    weights: per pair (or one value for all), the reference's argument, and treated as the reference's curriculum
        backend treats it: recorded as weights_mean / weights_count, NOT part of the loss.
    frame_weights: this engine's addition, and the one that changes what is learnt: one 1-D array of per-frame
        weights per trajectory (for frames of a biased run, exp(beta E_bias)).  It turns on the weighted VAMP-2 loss
        (DeepTICACurriculumTrainer.fit: the weight of a pair is that of its t frame).
    initial_state: the network's initial parameters under the reference's state_dict keys (a warm start, or a
        common start for a comparison); default: DeepTICAModel.initialize(cfg, seed=cfg.seed)."""
    if not len(X_list):
        raise ValueError("Expected at least one trajectory array for DeepTICA")
    backend = str(getattr(cfg, "trainer_backend", "lightning")).strip().lower()
    if backend not in TRAINING_BACKENDS:
        raise ValueError(f"Unsupported DeepTICA trainer backend '{backend}'. Valid backends: {', '.join(TRAINING_BACKENDS)}")
    if engine is None:
        from ...device import get_engine

        engine = get_engine()
    start = time.time()
    seed = int(getattr(cfg, "seed", 2024))
    arrays = [np.asarray(block, np.float32) for block in X_list]
    prep = prepare_features(arrays, tau_schedule=_tau_schedule_of(cfg), seed=seed, engine=engine)
    config = _config_dict(cfg)
    if initial_state is None:
        model = DeepTICAModel.initialize(config, prep.mean, prep.scale, seed)
    else:
        model = DeepTICAModel.from_arrays(config, initial_state, prep.mean, prep.scale)

    info = build_pair_info(arrays, prep.tau_schedule, pairs=pairs, weights=weights)
    idx_t, idx_tau, diag = info.idx_t, info.idx_tau, dict(info.diagnostics)
    _log_pairs(diag, len(arrays))
    before = vamp2_proxy(engine.mlp_forward(prep.x_device, model.spec).to_host(), idx_t, idx_tau)

    trainer = DeepTICACurriculumTrainer(model, curriculum_config(cfg, prep.tau_schedule), engine=engine)
    history = dict(trainer.fit(arrays, frame_weights=frame_weights))

    # the reference finalises with the network as trained (whitening computed, not applied): raw outputs
    outputs = engine.mlp_forward(prep.x_device, model.spec).to_host()
    whitening = output_whitening_info(outputs, idx_tau)
    top = estimate_top_eigenvalues(outputs, idx_t, idx_tau, int(getattr(cfg, "n_out", 2)), engine=engine)
    n_frames, usable, possible = outputs.shape[0], int(diag["usable_pairs"]), int(diag["total_possible_pairs"])
    usable_capped = min(usable, n_frames)

    history.setdefault("history_source", "curriculum_trainer")
    history["wall_time_s"] = float(history.get("wall_time_s", time.time() - start))
    history["vamp2_before"] = float(before)
    history["vamp2_after"] = float(vamp2_proxy(outputs, idx_t, idx_tau))
    history["output_variance"] = outputs.var(axis=0, ddof=1 if n_frames > 1 else 0).tolist()
    if top is not None:
        history["top_eigenvalues"] = [float(x) for x in top]
    history["pair_diagnostics_overall"] = diag
    history["usable_pairs"] = usable_capped
    history["pair_coverage"] = min(float(diag["pair_coverage"]), usable_capped / float(possible)) if possible > 0 else 0.0
    history["pairs_by_trajectory"] = diag["pairs_by_trajectory"]
    history["short_trajectories"] = list(diag["short_trajectories"])
    history["total_possible_pairs"] = possible
    history["lag_used"] = int(diag["lag_used"])
    history["weights_mean"] = float(np.mean(info.weights)) if info.weights.size else 0.0
    history["weights_count"] = int(info.weights.size)
    history["pair_diagnostics"].setdefault("overall", diag)
    history["output_mean"] = whitening["mean"]
    history["output_transform"] = whitening["transform"]
    history["output_transform_applied"] = whitening["transform_applied"]
    history["whitening"] = whitening
    model.training_history = history
    return model
