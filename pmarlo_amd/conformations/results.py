"""Result containers of the conformation finder.

Mirrors pmarlo.conformations.results (S/conformations/results.py): TPTResult (:13-70), Conformation (:155-217) and
ConformationSet (:220-395) with the reference's field names, defaults and JSON layout, so a file written by either
side loads on the other.  KISResult and UncertaintyResult live with the classes that fill them
(kinetic_importance.py, uncertainty.py) and are re-exported here.

Stated divergence: the finder stores a numpy row (the PCCA+ memberships of a state) in Conformation.metadata, which
json.dumps refuses; to_dict writes arrays and numpy scalars found in a metadata dict as lists and Python numbers."""

from __future__ import annotations

import json
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional

import numpy as np

from .kinetic_importance import KISResult
from .uncertainty import UncertaintyResult

__all__ = ["TPTResult", "KISResult", "UncertaintyResult", "Conformation", "ConformationSet"]


def _plain(value: Any) -> Any:
    """`value` with arrays as lists and numpy scalars as Python numbers, containers walked."""
    if isinstance(value, np.ndarray):
        return value.tolist()
    if isinstance(value, np.generic):
        return value.item()
    if isinstance(value, dict):
        return {k: _plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    return value


def _opt(cast, value):
    return cast(value) if value is not None else None


@dataclass(frozen=True)
class TPTResult:
    """Committors, gross (flux_matrix) and net flux, total flux, rate and mean first-passage time A -> B, the first
    pathways with their fluxes, the states carrying the most flux, and how the pathway decomposition ended:
    pathway_iterations paths were found, tpt_converged is False when that hit pathway_max_iterations."""

    source_states: np.ndarray
    sink_states: np.ndarray
    forward_committor: np.ndarray
    backward_committor: np.ndarray
    flux_matrix: np.ndarray
    net_flux: np.ndarray
    total_flux: float
    rate: float
    mfpt: float
    pathways: List[List[int]] = field(default_factory=list)
    pathway_fluxes: np.ndarray = field(default_factory=lambda: np.array([]))
    bottleneck_states: np.ndarray = field(default_factory=lambda: np.array([]))
    tpt_converged: bool = True
    pathway_iterations: int = 0
    pathway_max_iterations: int = 0

    def to_dict(self) -> Dict[str, Any]:
        return {
            "source_states": self.source_states.tolist(),
            "sink_states": self.sink_states.tolist(),
            "forward_committor": self.forward_committor.tolist(),
            "backward_committor": self.backward_committor.tolist(),
            "flux_matrix": self.flux_matrix.tolist(),
            "net_flux": self.net_flux.tolist(),
            "total_flux": float(self.total_flux),
            "rate": float(self.rate),
            "mfpt": float(self.mfpt),
            "pathways": self.pathways,
            "pathway_fluxes": self.pathway_fluxes.tolist(),
            "bottleneck_states": self.bottleneck_states.tolist(),
            "tpt_converged": bool(self.tpt_converged),
            "pathway_iterations": int(self.pathway_iterations),
            "pathway_max_iterations": int(self.pathway_max_iterations),
        }


@dataclass
class Conformation:
    """One microstate of the analysis: its type ('metastable', 'transition' or 'tse'), population, free energy in
    kJ/mol, forward committor, kinetic importance score, reactive flux through it, macrostate, and the
    representative frame (global, trajectory, local index) and structure file once picked."""

    conformation_type: str
    state_id: int
    population: float
    free_energy: float
    macrostate_id: Optional[int] = None
    frame_index: Optional[int] = None
    trajectory_index: Optional[int] = None
    local_frame_index: Optional[int] = None
    committor: Optional[float] = None
    kis_score: Optional[float] = None
    flux: Optional[float] = None
    structure_path: Optional[str] = None
    metadata: Dict[str, Any] = field(default_factory=dict)

    def to_dict(self) -> Dict[str, Any]:
        return {
            "conformation_type": self.conformation_type,
            "state_id": int(self.state_id),
            "macrostate_id": _opt(int, self.macrostate_id),
            "frame_index": _opt(int, self.frame_index),
            "trajectory_index": _opt(int, self.trajectory_index),
            "local_frame_index": _opt(int, self.local_frame_index),
            "population": float(self.population),
            "free_energy": float(self.free_energy),
            "committor": _opt(float, self.committor),
            "kis_score": _opt(float, self.kis_score),
            "flux": _opt(float, self.flux),
            "structure_path": str(self.structure_path) if self.structure_path else None,
            "metadata": _plain(self.metadata),
        }


def _array_or_scalar(value):
    return np.array(value) if isinstance(value, list) else value


@dataclass
class ConformationSet:
    """Everything one find_conformations call returns."""

    conformations: List[Conformation] = field(default_factory=list)
    tpt_result: Optional[TPTResult] = None
    kis_result: Optional[KISResult] = None
    uncertainty_results: List[UncertaintyResult] = field(default_factory=list)
    macrostate_labels: Optional[np.ndarray] = None
    metadata: Dict[str, Any] = field(default_factory=dict)

    def get_by_type(self, conformation_type: str) -> List[Conformation]:
        return [c for c in self.conformations if c.conformation_type == conformation_type]

    def get_transition_states(self) -> List[Conformation]:
        return self.get_by_type("transition")

    def get_transition_state_ensemble(self) -> List[Conformation]:
        """The reactive states whose committor is close to one half."""
        return self.get_by_type("tse")

    def get_metastable_states(self) -> List[Conformation]:
        return self.get_by_type("metastable")

    def to_dict(self) -> Dict[str, Any]:
        return {
            "conformations": [c.to_dict() for c in self.conformations],
            "tpt_result": self.tpt_result.to_dict() if self.tpt_result else None,
            "kis_result": self.kis_result.to_dict() if self.kis_result else None,
            "uncertainty_results": [u.to_dict() for u in self.uncertainty_results],
            "macrostate_labels": self.macrostate_labels.tolist() if self.macrostate_labels is not None else None,
            "metadata": _plain(self.metadata),
        }

    def to_json(self, indent: int = 2) -> str:
        return json.dumps(self.to_dict(), indent=indent)

    def save(self, filepath: str | Path) -> None:
        path = Path(filepath)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(self.to_json())

    @classmethod
    def load(cls, filepath: str | Path) -> "ConformationSet":
        data = json.loads(Path(filepath).read_text())
        tpt_result = kis_result = macrostate_labels = None
        t = data.get("tpt_result")
        if t:
            tpt_result = TPTResult(
                source_states=np.array(t["source_states"]), sink_states=np.array(t["sink_states"]),
                forward_committor=np.array(t["forward_committor"]), backward_committor=np.array(t["backward_committor"]),
                flux_matrix=np.array(t["flux_matrix"]), net_flux=np.array(t["net_flux"]), total_flux=t["total_flux"],
                rate=t["rate"], mfpt=t["mfpt"], pathways=t.get("pathways", []),
                pathway_fluxes=np.array(t.get("pathway_fluxes", [])),
                bottleneck_states=np.array(t.get("bottleneck_states", [])),
                tpt_converged=bool(t.get("tpt_converged", True)), pathway_iterations=int(t.get("pathway_iterations", 0)),
                pathway_max_iterations=int(t.get("pathway_max_iterations", 0)))
        k = data.get("kis_result")
        if k:
            kis_result = KISResult(
                kis_scores=np.array(k["kis_scores"]), k_slow=k["k_slow"], eigenvectors=np.array(k["eigenvectors"]),
                eigenvalues=np.array(k["eigenvalues"]), ranked_states=np.array(k["ranked_states"]),
                stability_metric=k.get("stability_metric"),
                bootstrap_std=np.array(k["bootstrap_std"]) if k.get("bootstrap_std") else None)
        uncertainty_results = [
            UncertaintyResult(observable_name=u["observable_name"], mean=_array_or_scalar(u["mean"]),
                              std=_array_or_scalar(u["std"]), ci_lower=_array_or_scalar(u["ci_lower"]),
                              ci_upper=_array_or_scalar(u["ci_upper"]), n_samples=u["n_samples"], method=u["method"])
            for u in data.get("uncertainty_results", [])]
        if data.get("macrostate_labels") is not None:
            macrostate_labels = np.array(data["macrostate_labels"])
        return cls(conformations=[Conformation(**c) for c in data.get("conformations", [])], tpt_result=tpt_result,
                   kis_result=kis_result, uncertainty_results=uncertainty_results, macrostate_labels=macrostate_labels,
                   metadata=data.get("metadata", {}))
