"""Metadynamics on a DeepTICA collective variable, on the device: the time-dependent counterpart of CVBiasPotential.

The reference's active-bias example (example_programs/14_muller_brown_active_bias.py) keeps an ActiveBiasLedger of
Gaussian hills in CV space, pushes the walker with force_on_xy, deposits with add_hill and, after the CV model has
been retrained, moves the hills with reproject_to, which re-evaluates the deposit-time positions it kept
(centers_xy).  Here the walker is a molecule: per call the chain is

    positions + box -> features (featurize_spec) -> CVs (mlp_forward) -> hills sum and dV/dCV (msm_metad_bias)
                    -> dV/dfeatures (mlp_vjp with that upstream gradient) -> forces (featurize_spec_vjp, sign -1)

five launches, nothing read back, n = 1 being one MD step.  `deposit` appends a hill at the current CVs without the
CVs leaving the device and keeps the frame's features, which stand where the reference keeps centers_xy: the network
sees a frame only through them, so `reproject_to` runs the new network on the kept features."""

from __future__ import annotations

from typing import Any

import numpy as np

from ...device import DeviceArray
from ...reweight.metadynamics import HillsLedger
from .model import DeepTICAModel, MLPSpec
from .ts_feature_extractor import DeviceFeatureExtractor

__all__ = ["MetadynamicsCVBias"]


class MetadynamicsCVBias:
    """A DeepTICA network with its feature extractor and scaler, biased by the hills of `ledger` (a HillsLedger whose
    CVs are the network's raw outputs).  `cv_model`, `scaler_mean`, `scaler_scale`, `feature_extractor` and
    `feature_spec_hash` are CVBiasPotential's, with its checks."""

    def __init__(self, cv_model, scaler_mean, scaler_scale, ledger: HillsLedger, *, feature_extractor,
                 feature_spec_hash: str, feature_names: list[str] | None = None) -> None:
        if not isinstance(feature_extractor, DeviceFeatureExtractor):
            raise TypeError("feature_extractor must be a DeviceFeatureExtractor instance")
        if not isinstance(ledger, HillsLedger):
            raise TypeError("ledger must be a HillsLedger")
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
        # the features of every deposit, float32 [capacity, F]: what reproject_to re-evaluates
        self._features: DeviceArray | None = None
        self._n_features_kept = 0

    def _set_model(self, cv_model) -> None:
        if not isinstance(cv_model, (DeepTICAModel, MLPSpec)):
            raise TypeError("cv_model must be a DeepTICAModel or an MLPSpec")
        net = cv_model.spec if isinstance(cv_model, DeepTICAModel) else cv_model
        if net.widths[0] != self.feature_count:
            raise ValueError(f"the network takes {net.widths[0]} features but the scaler has {self.feature_count}")
        if net.widths[-1] != self.ledger.n_cv:
            raise ValueError(f"the network gives {net.widths[-1]} CVs but the ledger's hills have {self.ledger.n_cv}")
        net.check_envelope()
        self.cv_model = cv_model
        self.spec = MLPSpec(net.widths, net.activation, net.ln_in, net.ln_hidden, net.head_activation, net.params,
                            self.scaler_mean.astype(np.float64), self.scaler_scale.astype(np.float64))

    # -- shapes ---------------------------------------------------------------
    def _frames(self, positions, box):
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
        self._check_extractor()
        return np.ascontiguousarray(pos[None] if single else pos), bx, single

    def _check_extractor(self) -> None:
        if self.feature_extractor.feature_count != self.feature_count:
            raise RuntimeError(f"feature extractor returned {self.feature_extractor.feature_count} features "
                               f"but scaler expects {self.feature_count}")

    def _box(self, box):
        return box if self.uses_periodic_boundary_conditions else None

    # -- evaluation -------------------------------------------------------------
    def cvs_device(self, xyz_d: DeviceArray, box_d=None, mic: str = "round"):
        """(features float32 [n, F], CVs float64 [n, d]) on the device."""
        eng, table = self.feature_extractor._engine_table()
        if xyz_d.shape[1] < self.atom_count:
            raise RuntimeError(f"expected at least {self.atom_count} atoms, received {xyz_d.shape[1]}")
        self._check_extractor()
        feats = eng.featurize_spec(xyz_d, table, box=self._box(box_d), mic=mic)
        return feats, eng.mlp_forward(feats, self.spec)

    def energy_and_forces_device(self, xyz_d: DeviceArray, box_d=None, mic: str = "round") -> dict:
        """{"energy" f64 [n], "cv" f64 [n, d], "force" f64 [n, A, 3] = -dV/dx} on the device for xyz_d float32
        [n, A, 3] and box_d float32 [1 or n, 9] (or None).  With device inputs nothing is uploaded or waited for."""
        eng, table = self.feature_extractor._engine_table()
        feats, cv = self.cvs_device(xyz_d, box_d, mic)
        led = self.ledger
        energy, grad = eng.metad_bias(cv, led.device_hills(), len(led), periods=led.periods, kernel=led.kernel,
                                      cut=led.cut, grad=True)
        gx = eng.mlp_vjp(feats, self.spec, gout=grad, want_energy=False, want_outputs=False)["gx"]
        force = eng.featurize_spec_vjp(xyz_d, table, gx, box=self._box(box_d), mic=mic, sign=-1.0)
        return {"energy": energy, "cv": cv, "force": force, "features": feats}

    def _run(self, positions, box, mic):
        pos, bx, single = self._frames(positions, box)
        eng, _ = self.feature_extractor._engine_table()
        return self.energy_and_forces_device(eng.to_device(pos), bx, mic), single

    def energy_and_forces(self, positions, box=None, mic: str = "round"):
        """(V, F) as host arrays: a scalar and (A, 3) for positions (A, 3), [n] and (n, A, 3) for (n, A, 3).  V is the
        bias of all hills in the ledger's energy unit, F = -dV/dx."""
        res, single = self._run(positions, box, mic)
        E, F = res["energy"].to_host(), res["force"].to_host()
        return (E[0], F[0]) if single else (E, F)

    def forward(self, positions, box=None) -> np.ndarray:
        return self.energy_and_forces(positions, box)[0]

    __call__ = forward

    def compute_cvs(self, positions, box=None) -> np.ndarray:
        """The collective variables (raw network outputs): float64 [1, d] for one frame, [n, d] for a batch."""
        pos, bx, _single = self._frames(positions, box)
        eng, _ = self.feature_extractor._engine_table()
        return self.cvs_device(eng.to_device(pos), bx)[1].to_host()

    # -- deposition ---------------------------------------------------------------
    def deposit_device(self, xyz_d: DeviceArray, box_d=None, mic: str = "round", *, sigma=None,
                       height: float | None = None, time: float | None = None) -> int:
        """Deposits one hill at the CVs of the single frame xyz_d float32 [1, A, 3]; the CVs stay on the device."""
        if xyz_d.shape[0] != 1:
            raise ValueError("deposit takes one frame")
        eng, _table = self.feature_extractor._engine_table()
        if len(self.ledger) != self._n_features_kept:           # before anything is appended
            raise RuntimeError("the ledger holds hills this potential did not deposit: their features are unknown")
        feats, cv = self.cvs_device(xyz_d, box_d, mic)
        k = self.ledger.add_hill(cv, sigma, height, time=time)
        F = self.feature_count
        if self._features is None or k >= self._features.shape[0]:
            bigger = eng.empty((max(self.ledger.capacity, k + 1), F), np.float32)
            if self._features is not None and self._n_features_kept:
                bigger.view((self._n_features_kept, F)).copy_from(self._features.view((self._n_features_kept, F)))
            self._features = bigger
        self._features.view((1, F), offset_elems=k * F).copy_from(feats)
        self._n_features_kept = k + 1
        return k

    def deposit(self, positions, box=None, *, sigma=None, height: float | None = None,
                time: float | None = None) -> int:
        """Deposits one hill at the CVs of `positions` (A, 3) and returns its index."""
        pos, bx, single = self._frames(positions, box)
        if not single and pos.shape[0] != 1:
            raise ValueError("deposit takes one frame")
        eng, _ = self.feature_extractor._engine_table()
        return self.deposit_device(eng.to_device(pos), bx, sigma=sigma, height=height, time=time)

    def reproject_to(self, new_model) -> "MetadynamicsCVBias":
        """The same hills seen through `new_model` (same features and scaler, same number of CVs): every centre becomes
        the new network's output at the features of its deposit; heights, sigmas and times stay.  Every hill of the
        ledger must have been deposited through this potential."""
        H = len(self.ledger)
        if H != self._n_features_kept:
            raise RuntimeError(f"the ledger holds {H} hills, {self._n_features_kept} of them deposited here: "
                               "the features of the others are unknown")
        self._set_model(new_model)
        if H:
            eng, _ = self.feature_extractor._engine_table()
            cv = eng.mlp_forward(self._features.view((H, self.feature_count)), self.spec)
            self.ledger.set_centers(cv.to_host())
        return self

    def get_metadata(self) -> dict[str, Any]:
        return {
            "bias_type": "metadynamics",
            "n_hills": len(self.ledger),
            "kernel": self.ledger.kernel,
            "bias_factor": self.ledger.bias_factor,
            "feature_names": list(self.feature_names),
            "n_features": int(self.feature_count),
            "cv_model_type": self.cv_model.__class__.__name__,
            "feature_spec_sha256": self.feature_spec_sha256,
            "uses_pbc": self.uses_periodic_boundary_conditions,
            "atom_count": int(self.atom_count),
        }
