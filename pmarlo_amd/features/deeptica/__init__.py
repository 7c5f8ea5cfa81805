"""DeepTICA on the device (mirror of pmarlo.features.deeptica): inference with a trained network -- load the
reference's bundle, forward pass and output whitening without the frames leaving the device (model.py) -- and the
numpy-level eigenvalue estimator of the trainer (core/).  Training stays PyTorch in the reference and is out of
scope."""

from .model import DeepTICAModel, MLPSpec

__all__ = ["DeepTICAModel", "MLPSpec"]
