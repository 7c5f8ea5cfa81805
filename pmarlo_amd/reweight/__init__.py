"""Frame weights for multi-ensemble runs: MBAR on the device (csrc/mbar.hip).

``mbar`` solves the MBAR equations for K sampled states and evaluates unsampled target states,
``temperature_weights`` is the replica-ladder case built from one energy per frame, and ``Reweighter`` writes
``dataset["frame_weights"]``, where discretize_dataset, prepare_msm_discretization and the free-energy entry points
pick them up.
"""

from .mbar import MBARResult, mbar, temperature_weights
from .reweighter import Reweighter

__all__ = ["MBARResult", "Reweighter", "mbar", "temperature_weights"]
