"""DeepTICA on the device (mirror of pmarlo.features.deeptica and pmarlo.ml.deeptica.trainer): inference with a
trained network -- load / save the reference's bundle, forward pass and output whitening without the frames leaving
the device (model.py) --, training -- the curriculum trainer over the device's VAMP-2 loss, backward pass and AdamW
(trainer.py) --, use -- the bias potential on a trained network's collective variables, energy and forces in one call
(cv_bias_potential.py), or a metadynamics bias on them with on-line deposition (metadynamics_bias.py), or an OPES
bias with on-line deposition (opes_bias.py) --, the pipeline users call -- DeepTICAConfig and train_deeptica, from
raw trajectories to a trained model with its completed history (config.py, training.py) -- and its pieces: feature
preparation, lagged pairs, the vamp2 proxy and the eigenvalue estimator (core/)."""

from .config import DeepTICAConfig
from .core import FeaturePrep, PairInfo, build_pair_info, prepare_features, vamp2_proxy
from .cv_bias_potential import CVBiasPotential, HarmonicExpansionBias, create_cv_bias_potential, feature_spec_sha256
from .metadynamics_bias import MetadynamicsCVBias
from .model import DeepTICAModel, MLPSpec
from .opes_bias import OPESCVBias
from .trainer import CurriculumConfig, DeepTICACurriculumTrainer
from .training import train_deeptica

__all__ = ["CVBiasPotential", "CurriculumConfig", "DeepTICAConfig", "DeepTICACurriculumTrainer", "DeepTICAModel",
           "FeaturePrep", "HarmonicExpansionBias", "MLPSpec", "MetadynamicsCVBias", "OPESCVBias", "PairInfo",
           "build_pair_info", "create_cv_bias_potential", "feature_spec_sha256", "prepare_features", "train_deeptica",
           "vamp2_proxy"]
