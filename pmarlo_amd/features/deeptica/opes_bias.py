"""OPES on a DeepTICA collective variable, on the device: the chain of MetadynamicsCVBias with the OPES bias in the
middle.

    positions + box -> features (featurize_spec) -> CVs (mlp_forward) -> V and dV/dCV (msm_opes_bias, live form)
                    -> dV/dfeatures (mlp_vjp with that upstream gradient) -> forces (featurize_spec_vjp, sign -1)

five launches, nothing read back, n = 1 being one MD step: the live form evaluates a frame against the compressed
kernels with one wave and reads K, W and Z from the device state, so a step neither uploads nor waits.  `deposit`
makes one OPES deposit at the current CVs without the CVs leaving the device: the height exp(V(s) / kT), the width,
the compression and the new Z are all formed by msm_opes_deposit.  Moving the kernels to a retrained network
(`reproject_to` of MetadynamicsCVBias) is not offered: a compressed kernel is a merge of many deposits and has no
single frame whose features could be re-evaluated."""

from __future__ import annotations

from typing import Any

import numpy as np

from ...device import DeviceArray
from ...reweight.opes import OPESLedger
from .metadynamics_bias import MetadynamicsCVBias
from .ts_feature_extractor import DeviceFeatureExtractor

__all__ = ["OPESCVBias"]


class OPESCVBias(MetadynamicsCVBias):
    """A DeepTICA network with its feature extractor and scaler, biased by the OPES kernels of `ledger` (an OPESLedger
    whose CVs are the network's raw outputs).  The other arguments are CVBiasPotential's, with its checks."""

    def __init__(self, cv_model, scaler_mean, scaler_scale, ledger: OPESLedger, *, feature_extractor,
                 feature_spec_hash: str, feature_names: list[str] | None = None) -> None:
        if not isinstance(feature_extractor, DeviceFeatureExtractor):
            raise TypeError("feature_extractor must be a DeviceFeatureExtractor instance")
        if not isinstance(ledger, OPESLedger):
            raise TypeError("ledger must be an OPESLedger")
        self.feature_extractor = feature_extractor
        self.feature_spec_sha256 = str(feature_spec_hash)
        self.feature_names = list(feature_names or [])
        self.scaler_mean = np.asarray(scaler_mean, dtype=np.float32).reshape(-1)
        self.scaler_scale = np.asarray(scaler_scale, dtype=np.float32).reshape(-1)
        if np.any(self.scaler_scale == 0):
            raise ValueError("scaler_scale contains zero; cannot normalise features")
        if self.scaler_mean.shape != self.scaler_scale.shape:
            raise ValueError(f"scaler mean {self.scaler_mean.shape} and scale {self.scaler_scale.shape} "
                             "differ in length")
        self.feature_count = int(self.scaler_mean.size)
        self.atom_count = int(getattr(feature_extractor, "atom_count", self.feature_count))
        self.uses_periodic_boundary_conditions = bool(getattr(feature_extractor, "use_pbc", True))
        self.ledger = ledger
        self._set_model(cv_model)
        eng, _table = feature_extractor._engine_table()
        if ledger.engine is None:
            ledger.engine = eng
        elif ledger.engine is not eng:
            raise ValueError("the ledger and the feature extractor live on different engines")

    def energy_and_forces_device(self, xyz_d: DeviceArray, box_d=None, mic: str = "round") -> dict:
        """{"energy" f64 [n], "cv" f64 [n, d], "force" f64 [n, A, 3] = -dV/dx, "cv_grad" f64 [n, d], "features"} on the
        device for xyz_d float32 [n, A, 3] and box_d float32 [1 or n, 9] (or None), against the live kernels.  With
        device inputs nothing is uploaded or waited for."""
        eng, table = self.feature_extractor._engine_table()
        feats, cv = self.cvs_device(xyz_d, box_d, mic)
        led = self.ledger
        energy, grad = eng.opes_bias(cv, led.device_ledger(), led.params(), live=True, grad=True)
        gx = eng.mlp_vjp(feats, self.spec, gout=grad, want_energy=False, want_outputs=False)["gx"]
        force = eng.featurize_spec_vjp(xyz_d, table, gx, box=self._box(box_d), mic=mic, sign=-1.0)
        return {"energy": energy, "cv": cv, "force": force, "features": feats, "cv_grad": grad}

    def deposit_device(self, xyz_d: DeviceArray, box_d=None, mic: str = "round", *, time: float | None = None) -> int:
        """One OPES deposit at the CVs of the single frame xyz_d float32 [1, A, 3]; returns its index.  The CVs stay on
        the device and nothing waits."""
        if xyz_d.shape[0] != 1:
            raise ValueError("deposit takes one frame")
        _feats, cv = self.cvs_device(xyz_d, box_d, mic)
        k = len(self.ledger)
        self.ledger.deposit(cv, time)
        return k

    def deposit(self, positions, box=None, *, time: float | None = None) -> int:
        """One OPES deposit at the CVs of `positions` (A, 3); returns its index."""
        pos, bx, single = self._frames(positions, box)
        if not single and pos.shape[0] != 1:
            raise ValueError("deposit takes one frame")
        eng, _ = self.feature_extractor._engine_table()
        return self.deposit_device(eng.to_device(pos), bx, time=time)

    def reproject_to(self, new_model):
        raise NotImplementedError("OPES kernels are merges of many deposits: they cannot be moved to another network")

    def get_metadata(self) -> dict[str, Any]:
        return {
            "bias_type": "opes",
            "n_deposits": len(self.ledger),
            "biasfactor": self.ledger.biasfactor,
            "barrier": self.ledger.barrier,
            "feature_names": list(self.feature_names),
            "n_features": int(self.feature_count),
            "cv_model_type": self.cv_model.__class__.__name__,
            "feature_spec_sha256": self.feature_spec_sha256,
            "uses_pbc": self.uses_periodic_boundary_conditions,
            "atom_count": int(self.atom_count),
        }
