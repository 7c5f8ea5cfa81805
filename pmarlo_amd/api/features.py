"""compute_features with the on-disk feature cache, trajectory alignment and the universal metric: mirror of
pmarlo.api.features (S/api/features.py:27-107 cache file, :110-135 align_trajectory, :192-208 compute_features,
:319-342 block assembly, :345-465 compute_universal_metric / compute_universal_embedding).

The cache is the only on-disk format on the path.  File name and
payload follow the reference, so caches written by either implementation are picked up by the
other: ``<cache_path>/features_<sha1>.npz`` holding ``X``, ``columns`` (str) and ``periodic``;
the key is the sha1 of the compact, key-sorted JSON of

    n_frames, n_atoms, specs,
    top_hash = sha1(json [n_atoms, n_residues, n_chains, first 50 atom names, first 50 residue names]),
    pos_hash = sha1 of round(1000 * xyz[::max(1, n_frames // min(n_frames, 10)), :50]) as int32.
"""

from __future__ import annotations

import hashlib
import json
import logging
from pathlib import Path
from typing import Any, Dict, List, Literal, Optional, Sequence, Tuple

import numpy as np

from ..features import get_feature, parse_feature_spec
from ..features.featurize import trig_expand_periodic
from ..markov_state_model.reduction import pca_reduce, tica_reduce, vamp_reduce

__all__ = ["compute_features", "feature_cache_file", "trig_expand_periodic", "align_trajectory",
           "compute_universal_metric", "compute_universal_embedding"]

_DEFAULT_UNIVERSAL_SPECS = ["phi_psi", "chi1", "Rg", "sasa", "hbonds_count", "ssfrac"]

logger = logging.getLogger("pmarlo")


def _compact(obj, **kw) -> bytes:
    return json.dumps(obj, separators=(",", ":"), **kw).encode()


def _residue_names(top) -> list[str]:
    """One name per residue, in file order (what iterating mdtraj's ``top.residues`` gives)."""
    if hasattr(top, "residues") and not hasattr(top, "res_index"):
        return [r.name for r in top.residues]
    names: list[str] = []
    last = None
    for i, r in enumerate(np.asarray(top.res_index)):
        if r != last:
            names.append(top.res_names[i])
            last = r
    return names


def _atom_names(top) -> list[str]:
    return list(top.atom_names) if hasattr(top, "atom_names") else [a.name for a in top.atoms]


def _n_chains(top) -> int:
    if hasattr(top, "chains") and not hasattr(top, "chain_ids"):
        return len(list(top.chains))
    ids = list(getattr(top, "chain_ids", []) or [])
    if not ids:
        return 1
    n, last = 0, None
    for c in ids:
        if c != last:
            n += 1
            last = c
    return n


def feature_cache_file(traj, feature_specs: Sequence[str], cache_path: Optional[str]) -> Optional[Path]:
    """Path of the cache entry for (trajectory, specs), or None when caching is off.  Creates the
    cache directory.  Same key as the reference's _resolve_cache_file (S/api/features.py:27-77)."""
    if not cache_path:
        return None
    folder = Path(cache_path)
    folder.mkdir(parents=True, exist_ok=True)
    top = traj.topology
    atoms, residues = _atom_names(top), _residue_names(top)
    top_hash = hashlib.sha1(_compact([len(atoms), len(residues), _n_chains(top), atoms[:50], residues[:50]])).hexdigest()
    pos_hash = None
    xyz = traj.xyz
    if xyz is not None and np.size(xyz):
        n_frames = int(traj.n_frames)
        nf = min(n_frames, 10)
        na = min(int(traj.n_atoms), 50)
        sample = np.asarray(xyz[::max(1, n_frames // nf), :na, :], dtype=np.float32)
        pos_hash = hashlib.sha1((sample * 1000.0).round().astype(np.int32).tobytes()).hexdigest()
    meta = {"n_frames": int(traj.n_frames), "n_atoms": int(traj.n_atoms), "specs": list(feature_specs),
            "top_hash": top_hash, "pos_hash": pos_hash}
    cell = getattr(traj, "unitcell", None)
    if cell is not None:   # periodic features depend on the cell; the key of a cell-less trajectory stays as it was
        meta["cell_hash"] = hashlib.sha1(np.ascontiguousarray(cell, dtype=np.float64).tobytes()).hexdigest()
    return folder / f"features_{hashlib.sha1(_compact(meta, sort_keys=True)).hexdigest()}.npz"


def _column_labels(fc, name: str, n_cols: int, kwargs: dict) -> List[str]:
    labels = getattr(fc, "labels", None)
    if isinstance(labels, list) and len(labels) == n_cols:
        return list(labels)
    if name == "phi_psi" and n_cols > 0:
        half = n_cols // 2
        return [f"phi_{i}" for i in range(half)] + [f"psi_{i}" for i in range(n_cols - half)]
    base = name
    if name == "distance_pair" and "i" in kwargs and "j" in kwargs:
        base = f"dist:atoms:{kwargs['i']}-{kwargs['j']}"
    return [base] if n_cols == 1 else [f"{base}_{i}" for i in range(n_cols)]


def _compute_blocks(traj, feature_specs: Sequence[str]) -> Tuple[np.ndarray, List[str], np.ndarray]:
    blocks: list[np.ndarray] = []
    flags: list[np.ndarray] = []
    columns: List[str] = []
    for spec in feature_specs:
        name, kwargs = parse_feature_spec(spec)
        fc = get_feature(name)
        X = fc.compute(traj, **kwargs)
        logger.info("[features] %-14s -> shape=%s", name, tuple(X.shape))
        if X.size == 0:
            continue
        periodic = np.asarray(fc.is_periodic())
        if name in {"distance", "distance_pair"} and bool(periodic.any()):
            raise ValueError(f"Distance features must not be flagged as periodic; feature '{name}' returned "
                             f"periodicity {periodic}")
        blocks.append(X)
        flags.append(periodic)
        columns.extend(_column_labels(fc, name, X.shape[1], kwargs))
    if not blocks:
        return np.empty((traj.n_frames, 0), dtype=float), columns, np.empty((0,), dtype=bool)
    lengths = [int(b.shape[0]) for b in blocks]
    n_min = min(lengths)
    if any(n != n_min for n in lengths):
        logger.warning("[features] Frame count mismatch across features: %s -> truncating to %d", lengths, n_min)
    X_all = np.hstack([b[:n_min] for b in blocks])
    return X_all, columns, np.concatenate(flags) if flags else np.zeros((X_all.shape[1],), dtype=bool)


def compute_features(traj, feature_specs: Sequence[str], cache_path: Optional[str] = None
                     ) -> Tuple[np.ndarray, List[str], np.ndarray]:
    """(X, columns, periodic) for the feature specs, e.g. ``["phi_psi", "distance([0, 5])"]``.
    With ``cache_path`` the result is loaded from / saved to ``features_<sha1>.npz`` there."""
    cache_file = feature_cache_file(traj, feature_specs, cache_path)
    if cache_file is not None and cache_file.exists():
        with np.load(cache_file) as data:
            X, cols, periodic = data["X"], [str(c) for c in data["columns"].tolist()], data["periodic"]
        logger.info("[features] Loaded from cache %s: shape=%s, columns=%d", cache_file, tuple(X.shape), len(cols))
        return X, cols, periodic
    X, columns, periodic = _compute_blocks(traj, feature_specs)
    if cache_file is not None:
        np.savez_compressed(cache_file, X=X, columns=np.array(columns, dtype=np.str_), periodic=periodic)
    return X, columns, periodic


def align_trajectory(traj, atom_selection: str | Sequence[int] | None = "name CA"):
    """Superpose all frames onto the first frame on the selected atoms (C-alpha by default; a selection string, None
    for "name CA", or a sequence of atom indices) and return the trajectory.  As in the reference
    (S/api/features.py:110-135) the alignment is ``traj.superpose(traj[0], atom_indices=...)``: it acts on ``traj``
    itself, and an empty selection raises instead of returning the unaligned trajectory."""
    top = traj.topology
    if isinstance(atom_selection, str):
        atom_indices = top.select(atom_selection)
    elif atom_selection is None:
        atom_indices = top.select("name CA")
    else:
        atom_indices = list(atom_selection)

    if atom_indices is None or len(atom_indices) == 0:
        raise ValueError("No atoms were selected for trajectory alignment; check the atom selection.")

    ref = traj[0]          # frame 0 before the alignment: superpose replaces traj.xyz, it does not write into it
    return traj.superpose(ref, atom_indices=atom_indices)


def _reduce(Xe: np.ndarray, method: str, lag: int, k: int) -> np.ndarray:
    if method == "pca":
        return pca_reduce(Xe, n_components=k)
    if method == "tica":
        return tica_reduce(Xe, lag=int(max(1, lag)), n_components=k)
    return vamp_reduce(Xe, lag=int(max(1, lag)), n_components=k)     # VAMP default


def compute_universal_metric(
    traj,
    feature_specs: Optional[Sequence[str]] = None,
    align: bool = True,
    atom_selection: str | Sequence[int] | None = "name CA",
    method: Literal["vamp", "tica", "pca"] = "vamp",
    lag: int = 10,
    *,
    cache_path: Optional[str] = None,
) -> Tuple[np.ndarray, Dict[str, Any]]:
    """A universal 1D metric from many CVs (S/api/features.py:345-420): optional superposition (C-alpha by default),
    the default feature set phi/psi, chi1, Rg, SASA, H-bond count, secondary-structure fractions unless specs are
    given, cos/sin expansion of the periodic columns, then one VAMP / TICA / PCA component.  Returns the metric
    (n_frames,) and metadata.

    Every default feature is invariant under rigid motion, so the alignment changes the metric only through the
    fp32 rounding of the moved coordinates; its use is the aligned coordinates themselves and ``RMSD_ref``."""
    logger.info("[universal] Starting computation (align=%s, method=%s, lag=%s)", bool(align), method, int(lag))
    traj_in = align_trajectory(traj, atom_selection=atom_selection) if align else traj
    if align:
        logger.info("[universal] Alignment complete: %d frames", traj_in.n_frames)
    specs = list(feature_specs) if feature_specs is not None else list(_DEFAULT_UNIVERSAL_SPECS)
    logger.info("[universal] Computing features: %s", ", ".join(specs))
    X, cols, periodic = compute_features(traj_in, feature_specs=specs, cache_path=cache_path)
    logger.info("[universal] Features computed: shape=%s, columns=%d", tuple(X.shape), len(cols))
    if X.size == 0:
        return np.zeros((traj.n_frames,), dtype=float), {
            "columns": cols,
            "periodic": periodic,
            "reduction": method,
            "lag": int(lag),
            "aligned": bool(align),
            "specs": specs,
        }
    Xe, index_map = trig_expand_periodic(X, periodic)
    logger.info("[universal] Expanded shape=%s; reducing with %s -> 1D", tuple(Xe.shape), method)
    metric = _reduce(Xe, method, lag, 1).reshape(-1)
    meta: Dict[str, Any] = {
        "columns": cols,
        "periodic": periodic,
        "reduction": method,
        "lag": int(lag),
        "aligned": bool(align),
        "specs": specs,
        "index_map": index_map,
    }
    return metric, meta


def compute_universal_embedding(
    traj,
    feature_specs: Optional[Sequence[str]] = None,
    align: bool = True,
    atom_selection: str | Sequence[int] | None = "name CA",
    method: Literal["vamp", "tica", "pca"] = "vamp",
    lag: int = 10,
    n_components: int = 2,
    *,
    cache_path: Optional[str] = None,
) -> Tuple[np.ndarray, Dict[str, Any]]:
    """A universal low-dimensional embedding (>= 1D) from many CVs (S/api/features.py:423-465): array of shape
    (n_frames, n_components) and metadata."""
    specs = list(feature_specs) if feature_specs is not None else list(_DEFAULT_UNIVERSAL_SPECS)
    traj_in = align_trajectory(traj, atom_selection=atom_selection) if align else traj
    X, cols, periodic = compute_features(traj_in, feature_specs=specs, cache_path=cache_path)
    Xe, index_map = trig_expand_periodic(X, periodic)
    k = int(max(1, n_components))
    Y = _reduce(Xe, method, lag, k)
    meta: Dict[str, Any] = {
        "columns": cols,
        "periodic": periodic,
        "reduction": method,
        "lag": int(lag),
        "aligned": bool(align),
        "specs": specs,
        "n_components": k,
        "index_map": index_map,
    }
    return Y, meta
