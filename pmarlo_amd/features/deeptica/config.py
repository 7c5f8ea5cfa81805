"""DeepTICAConfig: mirror of pmarlo.features.deeptica.DeepTICAConfig (S/features/deeptica/_full.py:165-262): the
reference's fields, defaults, backend validation and `small_data` preset.

Every backend name is accepted and every one trains with the device curriculum trainer (train_deeptica); `device`
and `num_workers` are accepted and ignored."""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Iterable, Optional, Tuple

__all__ = ["DeepTICAConfig", "TRAINING_BACKENDS"]

TRAINING_BACKENDS = ("curriculum", "deeptime", "lightning", "mlcolvar")      # sorted: the messages list them so


@dataclass(frozen=True)
class DeepTICAConfig:
    lag: int
    n_out: int = 2
    hidden: Tuple[int, ...] = (32, 16)
    activation: str = "gelu"
    learning_rate: float = 3e-4
    batch_size: int = 1024
    max_epochs: int = 200
    early_stopping: int = 25
    weight_decay: float = 1e-4
    log_every: int = 1
    seed: int = 0
    device: str = "cpu"                         # ignored: training runs on the engine's device
    trainer_backend: str = "lightning"
    val_frac: float = 0.1
    num_workers: int = 2                        # ignored: batches are index arrays into resident frames
    lr_schedule: str = "cosine"
    warmup_epochs: int = 5
    dropout: float = 0.0
    dropout_input: Optional[float] = None
    hidden_dropout: Tuple[float, ...] = field(default_factory=tuple)
    layer_norm_in: bool = False
    layer_norm_hidden: bool = False
    linear_head: bool = False
    batches_per_epoch: int = 200
    gradient_clip_val: float = 1.0
    gradient_clip_algorithm: str = "norm"
    tau_schedule: Tuple[int, ...] = field(default_factory=tuple)
    val_tau: Optional[int] = None
    epochs_per_tau: int = 15
    vamp_eps: float = 1e-3
    vamp_eps_abs: float = 1e-6
    vamp_alpha: float = 0.15
    vamp_cond_reg: float = 1e-4
    grad_norm_warn: Optional[float] = None
    variance_warn_threshold: float = 1e-6
    mean_warn_threshold: float = 5.0

    def __post_init__(self) -> None:
        backend = str(self.trainer_backend).strip().lower()
        if backend not in TRAINING_BACKENDS:
            raise ValueError(f"trainer_backend must be one of: {', '.join(TRAINING_BACKENDS)}")
        object.__setattr__(self, "trainer_backend", backend)

    @classmethod
    def small_data(cls, *, lag: int, n_out: int = 2, hidden: Tuple[int, ...] | None = None,
                   dropout_input: Optional[float] = None, hidden_dropout: Iterable[float] | None = None,
                   **overrides: Any) -> "DeepTICAConfig":
        """The preset for scarce data: one hidden layer of 32 unless `hidden` is given, dropout 0.15 on the inputs
        and on every hidden layer unless overridden (each clamped to [0, 1]), both LayerNorms on; `overrides` win
        over all of it."""
        layers = tuple(int(h) for h in (hidden if hidden is not None else (32,)))
        p_in = 0.15 if dropout_input is None else float(dropout_input)
        p_hidden = [0.15] * len(layers) if hidden_dropout is None else [float(p) for p in hidden_dropout]
        clamp = lambda p: float(min(1.0, max(0.0, p)))      # noqa: E731
        fields = {"lag": int(lag), "n_out": int(n_out), "hidden": layers, "dropout_input": clamp(p_in),
                  "hidden_dropout": tuple(clamp(p) for p in p_hidden), "layer_norm_in": True,
                  "layer_norm_hidden": True}
        fields.update(overrides)
        return cls(**fields)
