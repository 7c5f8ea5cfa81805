"""DeepTICA on the device (mirror of pmarlo.features.deeptica and pmarlo.ml.deeptica.trainer): inference with a
trained network -- load / save the reference's bundle, forward pass and output whitening without the frames leaving
the device (model.py) --, training -- the curriculum trainer over the device's VAMP-2 loss, backward pass and AdamW
(trainer.py) --, use -- the bias potential on a trained network's collective variables, energy and forces in one call
(cv_bias_potential.py) -- and the numpy-level eigenvalue estimator of the trainer (core/)."""

from .cv_bias_potential import CVBiasPotential, HarmonicExpansionBias, create_cv_bias_potential, feature_spec_sha256
from .model import DeepTICAModel, MLPSpec
from .trainer import CurriculumConfig, DeepTICACurriculumTrainer

__all__ = ["CVBiasPotential", "CurriculumConfig", "DeepTICACurriculumTrainer", "DeepTICAModel", "HarmonicExpansionBias",
           "MLPSpec", "create_cv_bias_potential", "feature_spec_sha256"]
