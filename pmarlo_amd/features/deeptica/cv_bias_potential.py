"""Bias potential on a DeepTICA collective variable, on the device: mirror of pmarlo.features.deeptica.cv_bias_potential
(CVBiasPotential, HarmonicExpansionBias, create_cv_bias_potential) and of the hash export.py gives a feature
specification (S/features/deeptica/export.py:40-61).

The chain is the reference's: positions + box -> features (the device feature extractor) -> (features - mean) / scale
-> network -> E = k sum cv^2.  The reference hands that energy to OpenMM's TorchForce, which differentiates it with
torch autograd at every MD step; here one call (Engine.bias_energy_forces: three launches) gives the energy, the CVs
and the force -dE/dx on every atom for a batch of frames, and a single frame per MD step is the n = 1 case.  The CVs
are the raw network outputs: the reference wraps the bare network (export.py:133-141), not the whitened transform.

Stated divergences.  The forces are float64, from closed-form Jacobians in float64 on the float32 bond vectors of the
forward (include/msmhip.h: msm_featurize_spec_vjp); at degenerate geometry (a zero-length bond, collinear angle
atoms, a dihedral without a plane) the feature contributes exactly zero where torch's autograd returns 0, inf or NaN
depending on the branch.  The scaler is kept as the reference keeps it, rounded to float32, but applied in float64
before Z is rounded to float32 (msm_mlp_forward's rule).  torch is not needed."""

from __future__ import annotations

import hashlib
import json
import logging
from typing import Any, Mapping, Optional

import numpy as np

from .model import DeepTICAModel, MLPSpec
from .ts_feature_extractor import DeviceFeatureExtractor

logger = logging.getLogger(__name__)

__all__ = ["CVBiasPotential", "HarmonicExpansionBias", "create_cv_bias_potential", "feature_spec_sha256"]


def _json_compatible(obj: Any) -> Any:
    if isinstance(obj, Mapping):
        return {str(k): _json_compatible(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_json_compatible(v) for v in obj]
    if isinstance(obj, np.ndarray):
        return _json_compatible(obj.tolist())
    if isinstance(obj, np.generic):
        return obj.item()
    if isinstance(obj, (int, float, str, bool)) or obj is None:
        return obj
    return str(obj)


def feature_spec_sha256(spec) -> str:
    """The hash export_cv_bias_potential writes for a feature specification given as a mapping or a list of entries:
    SHA-256 of its JSON with sorted keys, numpy values turned into plain ones and anything else into its str()."""
    return hashlib.sha256(json.dumps(_json_compatible(spec), sort_keys=True).encode("utf-8")).hexdigest()


class HarmonicExpansionBias:
    """Harmonic restraint in collective-variable space: E = k sum_i cv_i^2, k in kJ/mol (kept as the float32 the
    reference's buffer holds)."""

    def __init__(self, strength: float = 10.0) -> None:
        self.strength = float(np.float32(float(strength)))

    def forward(self, cvs) -> np.ndarray:
        cvs = np.asarray(cvs, np.float64)
        return self.strength * np.sum(cvs * cvs, axis=-1)

    __call__ = forward


class CVBiasPotential:
    """A DeepTICA network with its feature extractor, scaler and harmonic bias.  `cv_model`: a DeepTICAModel or an
    MLPSpec (its own scaler, if any, is replaced by scaler_mean / scaler_scale); `feature_extractor`: the
    DeviceFeatureExtractor of the specification the network was trained on."""

    def __init__(self, cv_model, scaler_mean, scaler_scale, *, feature_extractor, feature_spec_hash: str,
                 bias_type: str = "harmonic_expansion", bias_strength: float = 10.0,
                 feature_names: Optional[list[str]] = None) -> None:
        if not isinstance(cv_model, (DeepTICAModel, MLPSpec)):
            raise TypeError("cv_model must be a DeepTICAModel or an MLPSpec")
        if not isinstance(feature_extractor, DeviceFeatureExtractor):
            raise TypeError("feature_extractor must be a DeviceFeatureExtractor instance")
        self.cv_model = cv_model
        self.feature_extractor = feature_extractor
        self.feature_spec_sha256 = str(feature_spec_hash)
        self.bias_type = str(bias_type)
        self.bias_strength = float(bias_strength)
        self.feature_names = list(feature_names or [])
        self.scaler_mean = np.asarray(scaler_mean, dtype=np.float32).reshape(-1)
        self.scaler_scale = np.asarray(scaler_scale, dtype=np.float32).reshape(-1)
        self._feature_spec_hash_bytes = np.frombuffer(str(feature_spec_hash).encode("ascii"), dtype=np.uint8).copy()
        if np.any(self.scaler_scale == 0):
            raise ValueError("scaler_scale contains zero; cannot normalise features")
        if self.bias_type != "harmonic_expansion":
            raise ValueError(f"unsupported bias type '{bias_type}'")
        if self.scaler_mean.shape != self.scaler_scale.shape:
            raise ValueError(f"scaler mean {self.scaler_mean.shape} and scale {self.scaler_scale.shape} differ in length")
        self.bias_potential = HarmonicExpansionBias(strength=self.bias_strength)
        self.feature_count = int(self.scaler_mean.size)
        self.atom_count = int(getattr(feature_extractor, "atom_count", self.feature_count))
        self.uses_periodic_boundary_conditions = bool(getattr(feature_extractor, "use_pbc", True))
        net = cv_model.spec if isinstance(cv_model, DeepTICAModel) else cv_model
        if net.widths[0] != self.feature_count:
            raise ValueError(f"the network takes {net.widths[0]} features but the scaler has {self.feature_count}")
        net.check_envelope()
        # the network with this potential's scaler: float32 values as the reference's buffers, widened exactly
        self.spec = MLPSpec(net.widths, net.activation, net.ln_in, net.ln_hidden, net.head_activation, net.params,
                            self.scaler_mean.astype(np.float64), self.scaler_scale.astype(np.float64))
        logger.info("Created CVBiasPotential (%s) with %d features and bias strength %.2f kJ/mol", self.bias_type,
                    self.feature_count, self.bias_strength)

    # -- shapes ---------------------------------------------------------------
    def _frames(self, positions, box):
        """positions (A, 3) or (n, A, 3) -> (float32 [n, A, 3], box or None, single); the reference's errors.  A
        batch takes one box or one per frame; box None (not in the reference): nothing wraps."""
        pos = np.asarray(positions, dtype=np.float32)
        single = pos.ndim == 2
        if pos.ndim not in (2, 3) or pos.shape[-1] != 3:
            raise RuntimeError("positions tensor must have shape (N, 3)")
        if pos.shape[-2] < self.atom_count:
            raise RuntimeError(f"expected at least {self.atom_count} atoms, received {pos.shape[-2]}")
        bx = None
        if box is not None:
            bx = np.asarray(box, dtype=np.float32)
            if bx.shape != (3, 3) and (single or bx.shape != (pos.shape[0], 3, 3)):
                raise RuntimeError("box tensor must have shape (3, 3)")
        if self.feature_extractor.feature_count != self.feature_count:
            raise RuntimeError(f"feature extractor returned {self.feature_extractor.feature_count} features "
                               f"but scaler expects {self.feature_count}")
        return np.ascontiguousarray(pos[None] if single else pos), bx, single

    # -- evaluation -------------------------------------------------------------
    def energy_and_forces_device(self, xyz_d, box_d=None, mic: str = "round", **buffers):
        """(energy float64 [n], force float64 [n, A, 3]) on the device for xyz_d float32 [n, A, 3] and box_d float32
        [1 or n, 9] (or None without flagged entries), both DeviceArrays.  Nothing leaves the device; this is what
        stands where the reference puts TorchForce.  `buffers`: preallocated energy / cv / force / work (see
        Engine.bias_energy_forces), with which a call allocates nothing and can be captured in a graph."""
        res = self._run_device(xyz_d, box_d, mic, want_cv=buffers.get("cv") is not None, **buffers)
        return res["energy"], res["force"]

    def _run_device(self, xyz_d, box_d, mic, **kw):
        eng, table = self.feature_extractor._engine_table()
        if xyz_d.shape[1] < self.atom_count:
            raise RuntimeError(f"expected at least {self.atom_count} atoms, received {xyz_d.shape[1]}")
        return eng.bias_energy_forces(xyz_d, table, self.spec, self.bias_potential.strength,
                                      box=box_d if self.uses_periodic_boundary_conditions else None, mic=mic, **kw)

    def _run(self, positions, box, mic):
        pos, bx, single = self._frames(positions, box)
        eng, _ = self.feature_extractor._engine_table()
        res = self._run_device(eng.to_device(pos), bx, mic)
        return res, single

    def energy_and_forces(self, positions, box=None, mic: str = "round"):
        """(E, F) as host arrays: a scalar and (A, 3) for positions (A, 3), [n] and (n, A, 3) for (n, A, 3).
        E in kJ/mol, F = -dE/dx in kJ/mol/nm for positions in nm."""
        res, single = self._run(positions, box, mic)
        E, F = res["energy"].to_host(), res["force"].to_host()
        return (E[0], F[0]) if single else (E, F)

    def forward(self, positions, box=None) -> np.ndarray:
        """The bias energy: a scalar for positions (A, 3), [n] for (n, A, 3)."""
        return self.energy_and_forces(positions, box)[0]

    __call__ = forward

    def compute_cvs(self, positions, box=None) -> np.ndarray:
        """The collective variables (raw network outputs): float64 [1, n_out] for one frame, [n, n_out] for a batch."""
        res, _single = self._run(positions, box, "round")
        return res["cv"].to_host()

    # -- metadata -----------------------------------------------------------------
    def get_metadata(self) -> dict[str, Any]:
        return {
            "bias_type": self.bias_type,
            "bias_strength": self.bias_strength,
            "feature_names": list(self.feature_names),
            "n_features": int(self.feature_count),
            "cv_model_type": self.cv_model.__class__.__name__,
            "feature_spec_sha256": self.feature_spec_sha256,
            "uses_pbc": self.uses_periodic_boundary_conditions,
            "atom_count": int(self.atom_count),
        }

    def feature_spec_hash_bytes(self) -> np.ndarray:
        return self._feature_spec_hash_bytes


def create_cv_bias_potential(cv_model, scaler_mean, scaler_scale, *, feature_extractor, feature_spec_hash: str,
                             bias_strength: float = 10.0, feature_names: Optional[list[str]] = None) -> CVBiasPotential:
    return CVBiasPotential(cv_model=cv_model, scaler_mean=scaler_mean, scaler_scale=scaler_scale,
                           feature_extractor=feature_extractor, feature_spec_hash=feature_spec_hash,
                           bias_type="harmonic_expansion", bias_strength=bias_strength, feature_names=feature_names)
