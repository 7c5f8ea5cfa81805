"""Train a DeepTICA network on the device: mirror of pmarlo.ml.deeptica.trainer's CurriculumConfig and
DeepTICACurriculumTrainer (S/ml/deeptica/trainer.py) over Engine.mlp_loss_grad and Engine.adamw_step.

A step is the reference's (trainer.py:1020-1070): forward pass in training mode on the t and the tau frames of the
batch, VAMP-2 loss with uniform weights, backward pass, gradient norm, clip, AdamW; all of it device kernels (the
law: include/msmhip.h).  Around it this module mirrors the time split (trainer.py:1103-1134), the lagged-pair sets
per tau (:536-564), the warmup / cosine schedule (:952-979), the epoch aggregates (_EpochAccumulator), best-state
restoring (:1136-1142), _build_history's keys and the history attached to the model.  The sequences are uploaded
once; a batch is a pair of index arrays into them.

Stated divergences from the reference:
  * shuffled batches are index arrays drawn from numpy's generator (default_rng(seed)), dropout masks come from
    Philox keyed by the seed and counted by the optimiser step: neither stream is torch's, so curves differ from the
    reference's for the same seed while following the same law;
  * a gradient whose norm is not finite does not touch the parameters: the update is skipped on the device and
    FloatingPointError is raised here (the reference would step and poison the parameters);
  * a batch of a single pair (the tail of a pair set of 1 modulo batch_size) is dropped: the kernels need two pairs,
    and the reference's loss of one pair is the constant 0 with a zero gradient;
  * a dropout probability of 1 or more raises ValueError;
  * device selection, checkpoint / CSV / progress files and the data-loader workers are left out (the fields
    device, checkpoint_dir and num_workers do not exist).

Weights (this engine's addition; the reference's curriculum trainer has none).  train_step, evaluate and fit take
per-pair / per-frame weights and run the weighted loss of VAMP2Loss.forward(z0, zt, weights) on the device
(msm_mlp_loss_grad_weighted).  The weight of a pair is the weight of its t frame; every batch normalises its own
weights, as VAMP2Loss.forward does; epoch aggregates and evaluate then weight a batch by its total (clamped) weight
instead of its size.  A batch whose weights are all zero carries no information and is dropped; one whose effective
number of pairs (Kish) is below n_out + 2 is trained on with a warning.  Without weights nothing changes."""

from __future__ import annotations

import logging
import math
import time
from dataclasses import dataclass
from typing import Any, Optional, Sequence

import numpy as np

from .model import DeepTICAModel, dropout_sites

__all__ = ["CurriculumConfig", "DeepTICACurriculumTrainer", "lagged_pairs", "lr_schedule", "split_train_val"]

logger = logging.getLogger(__name__)

# pmarlo.constants: DEEPTICA_DEFAULT_*, DEEPTICA_MIN_VAMP_EPS, DEEPTICA_{MIN,MAX}_BATCH_FRACTION, the warning threshold
_LEARNING_RATE, _WEIGHT_DECAY, _VAMP_EPS, _VAMP_EPS_ABS, _VAMP_COND_REG = 3e-4, 1e-4, 1e-3, 1e-6, 1e-4
_MIN_VAMP_EPS, _MIN_FRACTION, _MAX_FRACTION, _COND_WARN = 1e-9, 1e-3, 0.9, 1e6
_ADAM_BETAS, _ADAM_EPS = (0.9, 0.999), 1e-8      # torch.optim.AdamW's defaults, which the reference keeps


@dataclass(frozen=True)
class CurriculumConfig:
    """Hyperparameters of the tau curriculum (the reference's fields, validation and defaults)."""

    tau_schedule: Sequence[int] = (2,)
    val_tau: int = 0
    epochs_per_tau: int = 15
    warmup_epochs: int = 5
    batch_size: int = 256
    learning_rate: float = _LEARNING_RATE
    weight_decay: float = _WEIGHT_DECAY
    val_fraction: float = 0.2
    shuffle: bool = True
    grad_clip_norm: Optional[float] = 1.0
    log_every: int = 1
    vamp_eps: float = _VAMP_EPS
    vamp_eps_abs: float = _VAMP_EPS_ABS
    vamp_alpha: float = 0.15
    vamp_cond_reg: float = _VAMP_COND_REG
    seed: Optional[int] = None
    max_batches_per_epoch: Optional[int] = None

    def __post_init__(self) -> None:
        schedule = [int(t) for t in self.tau_schedule if int(t) > 0]
        if not schedule:
            schedule = [max(1, int(self.val_tau) or 2)]
        schedule.sort()
        object.__setattr__(self, "tau_schedule", tuple(schedule))
        object.__setattr__(self, "val_tau", int(self.val_tau) if int(self.val_tau) > 0 else schedule[-1])
        if int(self.epochs_per_tau) <= 0:
            raise ValueError("epochs_per_tau must be positive")
        if int(self.batch_size) <= 0:
            raise ValueError("batch_size must be positive")
        object.__setattr__(self, "warmup_epochs", max(0, int(self.warmup_epochs)))
        frac = float(self.val_fraction)
        if not 0.0 < frac < 1.0:
            object.__setattr__(self, "val_fraction", min(max(frac, _MIN_FRACTION), _MAX_FRACTION))
        if float(self.learning_rate) <= 0:
            raise ValueError("learning_rate must be positive")


def lr_schedule(base_lr: float, warmup_epochs: int, total_epochs: int) -> list[float]:
    """The learning rate of every planned epoch (_initialize_scheduler / _step_scheduler, trainer.py:952-979):
    linear warmup over min(warmup, total) epochs, then half a cosine down to 0 at the last epoch."""
    total = max(0, int(total_epochs))
    warmup = min(max(0, int(warmup_epochs)), total)
    out = []
    for epoch in range(total):
        if warmup > 0 and epoch < warmup:
            factor = float(epoch + 1) / float(max(1, warmup))
        elif total <= warmup:
            factor = 1.0
        else:
            progress = float(epoch + 1 - warmup) / float(max(1, total - warmup))
            factor = 0.5 * (1.0 + math.cos(math.pi * max(0.0, min(1.0, progress))))
        out.append(float(base_lr) * max(0.0, factor))
    return out


def split_train_val(lengths: Sequence[int], max_tau: int, val_fraction: float) -> list[Optional[int]]:
    """Where each sequence is cut in time (_split_train_val, trainer.py:1103-1134): frames [0, split) train,
    [split, n) validate; None for a sequence too short to be used."""
    out: list[Optional[int]] = []
    for n_frames in (int(n) for n in lengths):
        if n_frames <= max_tau + 1:
            out.append(None)
            continue
        val_len = max(int(np.ceil(n_frames * float(val_fraction))), max_tau + 1)
        if val_len >= n_frames:
            val_len = max_tau + 1
        split = n_frames - val_len
        if split <= max_tau:
            split = max_tau + 1
        out.append(None if split >= n_frames else split)
    return out


def lagged_pairs(lengths: Sequence[int], tau: int, offsets: Sequence[int] | None = None):
    """(idx_t, idx_tau, diagnostics) of the pairs (t, t + tau) inside every sequence, in sequence order
    (_LaggedPairDataset.set_tau / diagnostics, trainer.py:536-577); indices count rows of the concatenated
    sequences, sequence i starting at offsets[i] (default: back to back)."""
    tau = int(tau)
    if tau <= 0:
        raise ValueError("tau must be positive")
    lengths = [int(n) for n in lengths]
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]) if lengths else []
    first, counts, short = [], [], []
    for i, (n_frames, off) in enumerate(zip(lengths, offsets)):
        possible = max(0, n_frames - tau)
        counts.append(possible)
        if possible <= 0:
            short.append(i)
            continue
        first.append(int(off) + np.arange(possible, dtype=np.int64))
    idx_t = np.concatenate(first) if first else np.zeros(0, np.int64)
    total = int(sum(counts))
    diag = {"tau": tau, "usable_pairs": int(idx_t.size), "total_possible_pairs": total,
            "pair_coverage": float(idx_t.size / float(total)) if total else 0.0,
            "pairs_per_sequence": counts, "short_sequences": short}
    return idx_t, idx_t + tau, diag


class _EpochSums:
    """The running sums of _EpochAccumulator (trainer.py:281-437)."""

    def __init__(self):
        self.loss = self.score = self.cond0 = self.condt = 0.0
        self.weight = 0
        self.effective: list[float] = []
        self.norms: list[float] = []
        self.norms_preclip: list[float] = []
        self.vectors: dict[str, np.ndarray] = {}
        self.eig = {"eig_c00_min": math.inf, "eig_c00_max": 0.0, "eig_ctt_min": math.inf, "eig_ctt_max": 0.0}

    def update(self, out: dict, batch: int) -> None:
        self.loss += out["loss"] * batch
        self.score += out["score"] * batch
        self.weight += batch
        self.norms.append(out["grad_norm"])
        self.norms_preclip.append(out["grad_norm_preclip"])
        if "effective_pairs" in out:
            self.effective.append(out["effective_pairs"])
        met = out["metrics"]
        self.cond0 += met["cond_C00"] * batch
        self.condt += met["cond_Ctt"] * batch
        for key in ("var_z0", "var_zt", "mean_z0", "mean_zt"):
            arr = np.asarray(met[key], np.float64) * float(batch)
            self.vectors[key] = arr if key not in self.vectors else self.vectors[key] + arr
        self.eig["eig_c00_min"] = min(self.eig["eig_c00_min"], met["eig_C00_min"])
        self.eig["eig_c00_max"] = max(self.eig["eig_c00_max"], met["eig_C00_max"])
        self.eig["eig_ctt_min"] = min(self.eig["eig_ctt_min"], met["eig_Ctt_min"])
        self.eig["eig_ctt_max"] = max(self.eig["eig_ctt_max"], met["eig_Ctt_max"])

    def finalize(self) -> dict:
        if self.weight == 0:
            return {"loss": 0.0, "score": 0.0, "grad_norm_mean": 0.0, "grad_norm_max": 0.0}
        w = float(self.weight)
        agg: dict[str, Any] = {
            "loss": self.loss / w, "score": self.score / w,
            "grad_norm_mean": float(np.mean(self.norms)), "grad_norm_max": float(np.max(self.norms)),
            "grad_norm_preclip_mean": float(np.mean(self.norms_preclip)),
            "grad_norm_preclip_max": float(np.max(self.norms_preclip)),
            "cond_c00": self.cond0 / w, "cond_ctt": self.condt / w}
        for key, arr in self.vectors.items():
            agg[key] = (arr / w).tolist()
        for key, value in self.eig.items():
            if value not in (math.inf, 0.0):
                agg[key] = value
        return agg


class DeepTICACurriculumTrainer:
    """Train a DeepTICAModel with a short-to-long tau curriculum and a fixed validation lag, on the device."""

    def __init__(self, model: DeepTICAModel, cfg: CurriculumConfig, engine=None):
        if not isinstance(model, DeepTICAModel):
            raise TypeError("model must be a pmarlo_amd DeepTICAModel")
        from ...device import get_engine

        self.model, self.cfg = model, cfg
        self.engine = engine if engine is not None else get_engine()
        spec = model.spec
        spec.check_envelope()
        self.dropout = dropout_sites(model.config, len(spec.widths) - 1)
        self.seed = int(cfg.seed) if cfg.seed is not None else 0
        self._rng = np.random.default_rng(self.seed)
        self._loss = {"eps": float(max(cfg.vamp_eps, _MIN_VAMP_EPS)), "eps_abs": float(max(cfg.vamp_eps_abs, 0.0)),
                      "alpha": float(min(max(cfg.vamp_alpha, 0.0), 1.0)), "cond_reg": float(max(cfg.vamp_cond_reg, 0.0))}
        self._params = self.engine._mlp_on_device(spec)[0]          # trained in place; the spec evaluates with them
        self._m = self.engine.zeros((self._params.size,), np.float64)
        self._v = self.engine.zeros((self._params.size,), np.float64)
        self._work = None
        self._x = None
        self.step = 0                                               # optimiser steps taken
        self._base_lr = self._current_lr = float(cfg.learning_rate)
        self._schedule: list[float] = []
        self._epoch = 0
        self.history: dict[str, Any] = {}
        self._best_state: Optional[np.ndarray] = None
        self._best_epoch = self._best_tau = -1
        self._best_score = -math.inf
        self._curves: dict[str, list] = {k: [] for k in (
            "cond_c00_curve", "cond_ctt_curve", "var_z0_curve", "var_zt_curve", "mean_z0_curve", "mean_zt_curve",
            "c0_eig_min_curve", "c0_eig_max_curve", "ctt_eig_min_curve", "ctt_eig_max_curve")}

    # -- data -----------------------------------------------------------------
    def set_frames(self, x) -> None:
        """The resident frame array [n, F] the index arrays of train_step / evaluate refer to: a device array, or
        host frames that are uploaded (float32 as they are, anything else as float64)."""
        from ...device import DeviceArray

        if not isinstance(x, DeviceArray):
            x = np.asarray(x)
            x = self.engine.to_device(np.ascontiguousarray(x if x.dtype == np.float32 else x.astype(np.float64)))
        if len(x.shape) != 2 or x.shape[1] != self.model.spec.widths[0]:
            raise ValueError(f"frames of shape {x.shape} for a network of {self.model.spec.widths[0]} features")
        self._x = x

    def _call(self, idx_t, idx_tau, train: bool, weights=None) -> dict:
        if self._x is None:
            raise RuntimeError("no frames are resident: call set_frames or fit first")
        res = self.engine.mlp_loss_grad(
            self._x, self.model.spec, idx_t, idx_tau, dropout=self.dropout if train else None, seed=self.seed,
            step=self.step, want_grad=train, work=self._work, weights=weights, **self._loss)
        self._work = res.pop("work")
        n_out = int(self.model.spec.widths[-1])
        if weights is not None and res["effective_pairs"] < n_out + 2:
            logger.warning("A batch has %.3g effective pairs for %d outputs (fewer than n_out + 2): its weights "
                           "leave the loss ill-determined", res["effective_pairs"], n_out)
        return res

    def state(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Host copies of the packed fp32 parameters and of AdamW's fp64 first and second moments."""
        return self._params.to_host(), self._m.to_host(), self._v.to_host()

    # -- one optimisation step ------------------------------------------------
    def train_step(self, idx_t, idx_tau, weights=None) -> dict:
        """One step on the pairs (idx_t[i], idx_tau[i]) of the resident frames: loss, score, metrics,
        grad_norm_preclip, grad_norm (after the clip) and batch_size.  Raises FloatingPointError when the gradient
        norm is not finite; the parameters and the optimiser state are then untouched.  ``weights``: one weight per
        pair (host array or f64 device array), normalised within the batch; the result then also has total_weight
        and effective_pairs."""
        res = self._call(idx_t, idx_tau, True) if weights is None else self._call(idx_t, idx_tau, True, weights)
        upd = self.engine.adamw_step(
            self._params, res.pop("grad"), self._m, self._v, self.step + 1, lr=self._current_lr, betas=_ADAM_BETAS,
            eps=_ADAM_EPS, weight_decay=float(max(self.cfg.weight_decay, 0.0)), clip=self.cfg.grad_clip_norm)
        if upd["skipped"]:
            raise FloatingPointError(f"gradient norm {upd['grad_norm_preclip']} at step {self.step + 1}: update skipped")
        self.step += 1
        res.update(grad_norm=upd["grad_norm"], grad_norm_preclip=upd["grad_norm_preclip"],
                   batch_size=int(np.size(idx_t) if not hasattr(idx_t, "size") else idx_t.size))
        return res

    def _batches(self, idx_t, idx_tau, shuffle: bool, weights=None):
        """(idx_t, idx_tau, weights or None, the batch's share in an aggregate) of every batch: the share is the
        batch size without weights and the batch's total clamped weight with them."""
        order = self._rng.permutation(idx_t.size) if shuffle else np.arange(idx_t.size)
        b = int(self.cfg.batch_size)
        for start in range(0, idx_t.size, b):
            sel = order[start:start + b]
            if sel.size < 2:
                continue
            if weights is None:
                yield idx_t[sel], idx_tau[sel], None, sel.size
                continue
            bw = weights[sel]
            total = float(np.clip(bw, 0.0, None).sum())
            if total > 0.0:
                yield idx_t[sel], idx_tau[sel], bw, total

    @staticmethod
    def _pair_weight_array(weights, m: int):
        if weights is None:
            return None
        w = np.asarray(weights, np.float64).reshape(-1)
        if w.size != m:
            raise ValueError(f"{w.size} weights for {m} frame pairs")
        if not np.all(np.isfinite(w)):
            raise ValueError("pair weights must be finite")
        return w

    def evaluate(self, idx_t, idx_tau, weights=None) -> dict:
        """Loss and score in evaluation mode over the pairs, in batches of batch_size, weighted by batch size
        (_evaluate, trainer.py:1072-1101); with per-pair ``weights`` every batch's loss is the weighted one and the
        batches are weighted by their total weight."""
        idx_t, idx_tau = np.asarray(idx_t, np.int64), np.asarray(idx_tau, np.int64)
        weights = self._pair_weight_array(weights, idx_t.size)
        loss = score = 0.0
        weight = 0
        for bt, btau, bw, share in self._batches(idx_t, idx_tau, False, weights):
            res = self._call(bt, btau, False) if bw is None else self._call(bt, btau, False, bw)
            loss += res["loss"] * share
            score += res["score"] * share
            weight += share
        if weight == 0:
            return {"loss": 0.0, "score": 0.0}
        return {"loss": loss / float(weight), "score": score / float(weight)}

    # -- the curriculum -------------------------------------------------------
    @staticmethod
    def _frame_weight_arrays(weights, sequences, what: str):
        if weights is None:
            return None
        out = [np.asarray(w, np.float64).reshape(-1) for w in weights]
        if len(out) != len(sequences) or any(w.size != a.shape[0] for w, a in zip(out, sequences)):
            raise ValueError(f"{what} must hold one 1-D array per sequence, one weight per frame")
        if any(not np.all(np.isfinite(w)) for w in out):
            raise ValueError(f"{what} must be finite")
        return out

    def fit(self, sequences: Sequence[np.ndarray], val_sequences: Optional[Sequence[np.ndarray]] = None,
            frame_weights: Optional[Sequence[np.ndarray]] = None,
            val_frame_weights: Optional[Sequence[np.ndarray]] = None) -> dict:
        """Train the model in place and return the history (also attached to model.training_history).
        ``frame_weights``: one 1-D array of per-frame weights per training sequence; the weight of a pair is that
        of its t frame, and the loss of every batch is the weighted one.  With the time split the validation part
        takes the tail of each sequence's weights; with ``val_sequences`` the validation pairs are weighted by
        ``val_frame_weights`` (uniformly when it is None).  The history then also has weighted_loss and
        effective_pairs_curve (per epoch, the mean over its batches of Kish's effective number of pairs)."""
        cfg = self.cfg
        train = [np.asarray(s, np.float32) for s in sequences]
        if not train:
            raise ValueError("at least one training sequence is required")
        if any(a.ndim != 2 for a in train):
            raise ValueError("training sequences must all be 2-D arrays")
        w_train = self._frame_weight_arrays(frame_weights, train, "frame_weights")
        if val_sequences is None:
            if val_frame_weights is not None:
                raise ValueError("val_frame_weights needs val_sequences: the time split takes the tail of frame_weights")
            max_tau = max([*cfg.tau_schedule, int(cfg.val_tau)])
            cuts = split_train_val([a.shape[0] for a in train], max_tau, cfg.val_fraction)
            val = [a[c:] for a, c in zip(train, cuts) if c is not None]
            w_val = None
            if w_train is not None:
                w_val = [w[c:] for w, c in zip(w_train, cuts) if c is not None]
                w_train = [w[:c] for w, c in zip(w_train, cuts) if c is not None]
            train = [a[:c] for a, c in zip(train, cuts) if c is not None]
            if not train:
                raise ValueError("no training data remained after splitting by time")
        else:
            val = [np.asarray(s, np.float32) for s in val_sequences]
            if any(a.ndim != 2 for a in val):
                raise ValueError("validation sequences must all be 2-D arrays")
            w_val = self._frame_weight_arrays(val_frame_weights, val, "val_frame_weights")
        if not val:
            raise ValueError("validation sequences are empty after splitting")
        weighted = w_train is not None or w_val is not None
        for name, parts in (("frame_weights", w_train), ("the validation part's frame weights", w_val)):
            if parts is not None and not any(np.any(w > 0.0) for w in parts):
                raise ValueError(f"{name} carry no positive weight")
        # one upload: the training sequences back to back, then the validation sequences
        n_train = sum(a.shape[0] for a in train)
        self.set_frames(np.concatenate(train + val, axis=0))
        val_lengths = [a.shape[0] for a in val]
        val_offsets = n_train + np.concatenate([[0], np.cumsum(val_lengths)[:-1]])
        self.val_pairs = lagged_pairs(val_lengths, cfg.val_tau, val_offsets)[:2]
        if self.val_pairs[0].size == 0:
            raise ValueError("validation dataset is empty - ensure val_tau is compatible with sequence lengths")
        # the weight of a pair is the weight of its t frame, looked up by row of the resident array
        wt_rows = np.concatenate(w_train) if w_train is not None else None
        self.val_pair_weights = np.concatenate(w_val)[self.val_pairs[0] - n_train] if w_val is not None else None
        effective_curve: list[float] = []
        blocks = [(int(tau), *lagged_pairs([a.shape[0] for a in train], tau)) for tau in cfg.tau_schedule]
        planned = sum(int(cfg.epochs_per_tau) for _, it, _, _ in blocks if it.size)
        self._schedule = lr_schedule(self._base_lr, cfg.warmup_epochs, planned)
        self._epoch = 0
        self._current_lr = self._base_lr
        start = time.time()

        per_tau: list[dict] = []
        overall: dict[str, list] = {k: [] for k in ("epochs", "train_loss", "train_score", "val_loss", "val_score",
                                                     "learning_rate", "grad_norm_mean", "grad_norm_max")}
        for tau, idx_t, idx_tau, diag in blocks:
            block = {"tau": tau, "epochs": [], "train_loss_curve": [], "train_score_curve": [], "val_loss_curve": [],
                     "val_score_curve": [], "learning_rate_curve": [], "grad_norm_mean_curve": [],
                     "grad_norm_max_curve": [], "diagnostics": diag}
            per_tau.append(block)
            if idx_t.size == 0:
                logger.warning("No lagged pairs available at tau=%d; skipping curriculum stage", tau)
                continue
            for epoch_idx in range(int(cfg.epochs_per_tau)):
                lr = self._current_lr = self._schedule[self._epoch] if self._schedule else self._base_lr
                self._epoch += 1
                sums = _EpochSums()
                pair_w = wt_rows[idx_t] if wt_rows is not None else None
                for b, (bt, btau, bw, share) in enumerate(self._batches(idx_t, idx_tau, bool(cfg.shuffle), pair_w)):
                    if cfg.max_batches_per_epoch is not None and b >= int(cfg.max_batches_per_epoch):
                        break
                    sums.update(self.train_step(bt, btau, bw), share)
                tm = sums.finalize()
                vm = self.evaluate(*self.val_pairs, self.val_pair_weights)
                if weighted:
                    effective_curve.append(float(np.mean(sums.effective)) if sums.effective else math.nan)
                overall_epoch = len(overall["epochs"]) + 1
                row = {"epochs": overall_epoch, "train_loss": tm["loss"], "train_score": tm["score"],
                       "val_loss": vm["loss"], "val_score": vm["score"], "learning_rate": float(lr),
                       "grad_norm_mean": tm["grad_norm_mean"], "grad_norm_max": tm["grad_norm_max"]}
                for key, value in row.items():
                    overall[key].append(value)
                    block["epochs" if key == "epochs" else key + "_curve"].append(value)
                self._record_condition_metrics(tm)
                if vm["score"] > self._best_score:
                    self._best_score, self._best_epoch, self._best_tau = float(vm["score"]), overall_epoch, tau
                    self._best_state = self._params.to_host()
                if int(cfg.log_every) > 0 and ((epoch_idx + 1) % int(cfg.log_every) == 0
                                               or epoch_idx + 1 == int(cfg.epochs_per_tau)):
                    logger.info("tau=%d val_tau=%d epoch=%d/%d lr=%.6e train_loss=%.6f val_score=%.6f", tau,
                                cfg.val_tau, epoch_idx + 1, int(cfg.epochs_per_tau), lr, tm["loss"], vm["score"])
        if self._best_state is not None:
            self._params.copy_from_host(self._best_state)
        self.model.spec.params = self._params.to_host()
        history = self._build_history(per_tau, overall, start)
        if weighted:
            history["weighted_loss"] = True
            history["effective_pairs_curve"] = effective_curve
        self.grad_norm_curve = list(overall["grad_norm_mean"])
        self.history = history
        if isinstance(self.model.training_history, dict):
            self.model.training_history.update(history)
        else:
            self.model.training_history = history
        return history

    def _record_condition_metrics(self, tm: dict) -> None:
        c = self._curves
        c["cond_c00_curve"].append(float(tm.get("cond_c00", 0.0)))
        c["cond_ctt_curve"].append(float(tm.get("cond_ctt", 0.0)))
        c["c0_eig_min_curve"].append(float(tm.get("eig_c00_min", math.nan)))
        c["c0_eig_max_curve"].append(float(tm.get("eig_c00_max", math.nan)))
        c["ctt_eig_min_curve"].append(float(tm.get("eig_ctt_min", math.nan)))
        c["ctt_eig_max_curve"].append(float(tm.get("eig_ctt_max", math.nan)))
        for key in ("var_z0", "var_zt", "mean_z0", "mean_zt"):
            if key not in tm:
                raise KeyError(f"Metric '{key}' is missing from the metrics collection.")
            c[key + "_curve"].append(list(tm[key]))
        for name in ("cond_c00", "cond_ctt"):
            if float(tm.get(name, 0.0)) > _COND_WARN:
                logger.warning("Condition number %s=%.3e exceeds stability threshold", name, tm[name])

    def _build_history(self, per_tau: list[dict], overall: dict[str, list], start: float) -> dict:
        """_build_history's keys (trainer.py:893-947)."""
        cfg, c = self.cfg, self._curves
        by_tau = lambda key: {int(b["tau"]): b[key] for b in per_tau}       # noqa: E731
        return {
            "tau_schedule": [int(t) for t in cfg.tau_schedule],
            "val_tau": int(cfg.val_tau),
            "epochs_per_tau": int(cfg.epochs_per_tau),
            "loss_curve": list(overall["train_loss"]),
            "objective_curve": list(overall["train_score"]),
            "val_loss_curve": list(overall["val_loss"]),
            "val_score_curve": list(overall["val_score"]),
            "learning_rate_curve": list(overall["learning_rate"]),
            "grad_norm_mean_curve": list(overall["grad_norm_mean"]),
            "grad_norm_max_curve": list(overall["grad_norm_max"]),
            "epochs": list(overall["epochs"]),
            "per_tau": per_tau,
            "per_tau_objective_curve": by_tau("val_score_curve"),
            "per_tau_learning_rate_curve": by_tau("learning_rate_curve"),
            "per_tau_grad_norm_mean_curve": by_tau("grad_norm_mean_curve"),
            "per_tau_grad_norm_max_curve": by_tau("grad_norm_max_curve"),
            "pair_diagnostics": by_tau("diagnostics"),
            "cond_c00_curve": [float(x) for x in c["cond_c00_curve"]],
            "cond_ctt_curve": [float(x) for x in c["cond_ctt_curve"]],
            "var_z0_curve": [list(r) for r in c["var_z0_curve"]],
            "var_zt_curve": [list(r) for r in c["var_zt_curve"]],
            "mean_z0_curve": [list(r) for r in c["mean_z0_curve"]],
            "mean_zt_curve": [list(r) for r in c["mean_zt_curve"]],
            "c0_eig_min_curve": [float(x) for x in c["c0_eig_min_curve"]],
            "c0_eig_max_curve": [float(x) for x in c["c0_eig_max_curve"]],
            "ctt_eig_min_curve": [float(x) for x in c["ctt_eig_min_curve"]],
            "ctt_eig_max_curve": [float(x) for x in c["ctt_eig_max_curve"]],
            "grad_norm_curve": list(overall["grad_norm_mean"]),
            "best_val_score": float(self._best_score) if self._best_score > -math.inf else 0.0,
            "best_epoch": int(self._best_epoch) if self._best_epoch >= 0 else None,
            "best_tau": int(self._best_tau) if self._best_tau >= 0 else None,
            "wall_time_s": float(max(0.0, time.time() - start)),
        }
