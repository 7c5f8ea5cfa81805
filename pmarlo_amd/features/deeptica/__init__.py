"""DeepTICA on the device (mirror of pmarlo.features.deeptica and pmarlo.ml.deeptica.trainer): inference with a
trained network -- load / save the reference's bundle, forward pass and output whitening without the frames leaving
the device (model.py) --, training -- the curriculum trainer over the device's VAMP-2 loss, backward pass and AdamW
(trainer.py) -- and the numpy-level eigenvalue estimator of the trainer (core/)."""

from .model import DeepTICAModel, MLPSpec
from .trainer import CurriculumConfig, DeepTICACurriculumTrainer

__all__ = ["CurriculumConfig", "DeepTICACurriculumTrainer", "DeepTICAModel", "MLPSpec"]
