"""Frame weights for multi-ensemble runs: MBAR (csrc/mbar.hip) and TRAM (csrc/tram.hip) on the device.

``mbar`` solves the MBAR equations for K sampled states and evaluates unsampled target states,
``temperature_weights`` is the replica-ladder case built from one energy per frame, ``tram`` and ``tram_from_counts``
couple the ensembles through one reversible Markov model each and return that model beside the weights, and
``Reweighter`` writes ``dataset["frame_weights"]``, where discretize_dataset, prepare_msm_discretization and the
free-energy entry points pick them up.  Metadynamics (csrc/metad.hip) is the bias that changes with time:
``HillsLedger`` holds the hills on the device, ``metadynamics_weights`` and ``MetadynamicsReweighter`` undo them, and
``read_hills`` / ``read_colvar`` read PLUMED's files.  OPES (csrc/opes.hip) is the bias built from compressed kernels:
``OPESLedger`` replays a KERNELS file (``read_kernels``) into a journal of kernel versions on the device and deposits on
line, ``opes_weights`` and ``OPESReweighter`` undo the bias each frame saw.
"""

from .mbar import MBARResult, mbar, temperature_weights
from .metadynamics import (HillsLedger, MetadWeights, MetadynamicsReweighter, metadynamics_weights, read_colvar,
                           read_hills)
from .opes import OPESLedger, OPESReweighter, OPESWeights, opes_weights, read_kernels
from .reweighter import Reweighter
from .tram import TRAMResult, tram, tram_from_counts

__all__ = ["HillsLedger", "MBARResult", "MetadWeights", "MetadynamicsReweighter", "OPESLedger", "OPESReweighter",
           "OPESWeights", "Reweighter", "TRAMResult", "mbar", "metadynamics_weights", "opes_weights", "read_colvar",
           "read_hills", "read_kernels", "temperature_weights", "tram", "tram_from_counts"]
