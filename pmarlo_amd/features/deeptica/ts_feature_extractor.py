"""Position -> feature extraction for DeepTICA models, on the device: the public names of
pmarlo.features.deeptica.ts_feature_extractor (S/features/deeptica/ts_feature_extractor.py).

A feature specification is a list of entries, or a mapping with ``features`` and an optional ``use_pbc``.  Each entry
names a ``type`` (``distance``, ``angle``, ``dihedral``; ``torsion`` is a dihedral), its atoms (``atom_indices``,
``atoms`` or ``indices``), and optionally a ``name`` (default ``feature_<position>``), a ``weight`` (a number or a
numeric string, default 1) and a ``pbc`` flag (default: the spec's ``use_pbc``, which defaults to True).  The feature
vector keeps the order of the entries.  A flagged entry measures minimum-image bond vectors: ``f = v . inv(box)``,
``v' = (f - round(f)) . box``, the reference's rule, which ``Engine.featurize_spec(mic="round")`` restates.

Where the reference holds torch tensors, ``NormalizedFeatureSpec`` holds numpy arrays under the same field names; where
it builds a TorchScript module, ``build_feature_extractor_module`` returns an object whose ``forward`` takes one frame
as the reference's does and whose ``transform`` takes a batch that may already live on the device."""

from __future__ import annotations

from collections.abc import Mapping, Sequence
from dataclasses import dataclass
from numbers import Real

import numpy as np

__all__ = ["FeatureSpecError", "NormalizedFeatureSpec", "build_feature_extractor_module", "canonicalize_feature_spec"]

_ARITY = {"distance": 2, "angle": 3, "dihedral": 4}


class FeatureSpecError(ValueError):
    """The feature specification cannot be used."""


@dataclass(frozen=True)
class NormalizedFeatureSpec:
    feature_names: tuple[str, ...]
    use_pbc: bool                       # any entry flagged
    atom_count: int                     # largest atom index + 1
    distance_pairs: np.ndarray          # int64 (n, 2)
    distance_positions: np.ndarray      # int64 (n,): position of each distance in the feature vector
    distance_pbc: np.ndarray            # bool (n,)
    angle_triplets: np.ndarray
    angle_positions: np.ndarray
    angle_pbc: np.ndarray
    dihedral_quads: np.ndarray
    dihedral_positions: np.ndarray
    dihedral_pbc: np.ndarray
    feature_weights: np.ndarray         # float32 (n_features,)

    @property
    def n_features(self) -> int:
        return len(self.feature_names)


def _weight(raw, name: str) -> float:
    if isinstance(raw, Real):
        return float(raw)
    if isinstance(raw, str):
        try:
            return float(raw)
        except ValueError:
            pass
    raise FeatureSpecError(f"weight for feature '{name}' must be numeric")


def canonicalize_feature_spec(spec) -> NormalizedFeatureSpec:
    """Group the entries of `spec` by type, remembering where each belongs in the feature vector."""
    default_pbc = True
    entries = spec
    if isinstance(spec, Mapping):
        entries = spec.get("features")
        if entries is None:
            raise FeatureSpecError("feature spec mapping is missing 'features'")
        default_pbc = bool(spec.get("use_pbc", True))
    if not isinstance(entries, Sequence):
        raise FeatureSpecError("feature list must be a sequence")

    names: list[str] = []
    weights: list[float] = []
    atoms_of: dict[str, list[list[int]]] = {k: [] for k in _ARITY}
    pos_of: dict[str, list[int]] = {k: [] for k in _ARITY}
    pbc_of: dict[str, list[bool]] = {k: [] for k in _ARITY}
    max_index = -1
    for position, entry in enumerate(entries):
        if not isinstance(entry, Mapping):
            raise FeatureSpecError("each feature entry must be a mapping")
        if entry.get("type") is None:
            raise FeatureSpecError("feature entry missing 'type'")
        kind = str(entry["type"]).strip().lower()
        kind = "dihedral" if kind == "torsion" else kind
        raw_atoms = entry.get("atom_indices") or entry.get("atoms") or entry.get("indices")
        if raw_atoms is None:
            raise FeatureSpecError("feature entry missing 'atom_indices' / 'atoms' / 'indices'")
        if not isinstance(raw_atoms, Sequence):
            raise FeatureSpecError("feature atoms must be a sequence of integers")
        atoms = [int(a) for a in raw_atoms]
        name = str(entry["name"]) if entry.get("name") is not None else f"feature_{position}"
        weight = _weight(entry.get("weight", 1.0), name)
        if kind not in _ARITY:
            raise FeatureSpecError(f"unsupported feature type '{kind}'")
        if len(atoms) != _ARITY[kind]:
            raise FeatureSpecError(f"{kind} requires exactly {_ARITY[kind]} atom indices")
        if min(atoms) < 0:
            raise FeatureSpecError(f"{kind} indices must be non-negative")
        names.append(name)
        weights.append(weight)
        atoms_of[kind].append(atoms)
        pos_of[kind].append(position)
        pbc_of[kind].append(bool(entry.get("pbc", default_pbc)))
        max_index = max(max_index, max(atoms))
    if not names:
        raise FeatureSpecError("feature specification must contain at least one entry")

    def _arrays(kind):
        return (np.asarray(atoms_of[kind], dtype=np.int64).reshape(-1, _ARITY[kind]),
                np.asarray(pos_of[kind], dtype=np.int64), np.asarray(pbc_of[kind], dtype=bool))

    return NormalizedFeatureSpec(tuple(names), any(any(v) for v in pbc_of.values()), max_index + 1,
                                 *_arrays("distance"), *_arrays("angle"), *_arrays("dihedral"),
                                 np.asarray(weights, dtype=np.float32))


class DeviceFeatureExtractor:
    """The extractor of one specification.  Its feature table is uploaded once per engine and stays on the device."""

    def __init__(self, spec: NormalizedFeatureSpec, engine=None) -> None:
        self.spec = spec
        self.engine = engine                # None: the process-wide engine
        self.feature_count = int(spec.n_features)
        self.atom_count = int(spec.atom_count)
        self.use_pbc = bool(spec.use_pbc)
        self._table = None

    def _engine_table(self):
        from ...device import get_engine

        eng = self.engine if self.engine is not None else get_engine()
        if self._table is None or self._table.rec.engine is not eng or not eng.handle:
            self._table = eng.feature_table(self.spec)
        return eng, self._table

    def transform(self, xyz, box=None, mic: str = "round", out=None, col0: int = 0):
        """xyz float32 (n, A, 3), a host array or a DeviceArray; box None, (3, 3) or (n, 3, 3), host or device
        (device: float32 [n_box, 9]).  Returns the DeviceArray float32 [n, F] (or `out`)."""
        eng, table = self._engine_table()
        if isinstance(xyz, np.ndarray):
            xyz = eng.to_device(np.ascontiguousarray(xyz, np.float32))
        if xyz.shape[1] < self.atom_count:
            raise RuntimeError(f"positions have {xyz.shape[1]} atoms, but specification references {self.atom_count}")
        return eng.featurize_spec(xyz, table, box=box, mic=mic, out=out, col0=col0)

    def forward(self, positions, box) -> np.ndarray:
        """One frame: positions (N, 3) and box (3, 3) in nm -> float32 (F,).  As in the reference the box is only
        looked at when an entry is flagged."""
        pos = np.asarray(positions, dtype=np.float32)
        if pos.ndim != 2 or pos.shape[-1] != 3:
            raise RuntimeError("positions must have shape (N, 3)")
        bx = np.asarray(box, dtype=np.float32)
        if bx.shape != (3, 3):
            raise RuntimeError("box tensor must have shape (3, 3)")
        out = self.transform(pos[None], bx if self.use_pbc else None)
        return out.to_host()[0]

    __call__ = forward


def build_feature_extractor_module(spec: NormalizedFeatureSpec, engine=None) -> DeviceFeatureExtractor:
    return DeviceFeatureExtractor(spec, engine)
