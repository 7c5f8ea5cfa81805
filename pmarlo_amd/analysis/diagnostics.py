"""Triviality / stability diagnostics of learned CVs: mirror of pmarlo.analysis.diagnostics
(S/analysis/diagnostics.py:33-112 segments, tau grid, integrated time, CK lags; :126-221 canonical correlations;
:247-351 autocorrelation curve; :357-579 tau derivation; :585-712 compute_diagnostics).

The passes over the frames run on the device: the per-segment autocorrelations of every lag come from one
``msm_autocorr_lagscan`` call per split, the joint second moments behind the canonical correlations from one
``msm_lagged_moments(lag = 0)`` pass over [inputs | CVs].  Each split is uploaded once and both share the copy.
The tau grid, the weighting of the segments, the integrated autocorrelation time and the (p + q)-sized algebra
of the canonical correlations are host arithmetic.  Pinned by tests/golden/diagnostics.*, made by importing
the reference.

Not replicated: the reference asks scikit-learn's iterative NIPALS ``CCA`` for scores and correlates them, which
approximates the classical canonical correlations to about its 1e-6 stopping rule and returns them in the order
NIPALS found them.  Here they are the exact singular values of the whitened cross-covariance, in descending
order (only ``min(correlations) > 0.95`` is ever read from the list)."""

from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Any, Dict, Mapping, MutableMapping, Sequence

import numpy as np

from ..device import get_engine
from .discretize import _coerce_array, _normalise_splits, _segments_from_split_metadata, _truncate_segments
from .project_cv import apply_whitening_from_metadata

logger = logging.getLogger("pmarlo")

__all__ = ["compute_diagnostics", "derive_taus", "CanonicalCorrelationError", "InsufficientSamplesError"]

DatasetLike = Mapping[str, Any] | MutableMapping[str, Any]
_VAR_FLOOR = 1e-8                 # pmarlo.constants.NUMERIC_RELATIVE_TOLERANCE, used as an absolute variance floor
_MAX_TAU_FRACTION = 1.0 / 3.0
_MIN_CK_MULTIPLIER = 2.0
_MAX_CK_MULTIPLIER = 5.0
_MAX_JOINT_WIDTH = 256            # widest [inputs | CVs] block of the moment pass
_RANK_CUTOFF = 1e-12              # eigenvalues of a correlation block below this fraction of the largest are dropped
_INPUT_KEYS = ("inputs", "raw", "raw_inputs", "raw_features", "features", "input_features")


@dataclass(frozen=True)
class _SegmentDescriptor:
    length: int
    stride: int


def _resolve_segments_for_split(split: Any, total_frames: int) -> tuple[list[int], list[int]]:
    lengths, strides = _segments_from_split_metadata(split) if isinstance(split, Mapping) else ([], [])
    return _truncate_segments(lengths, strides, total_frames)


def _segment_descriptors_for_split(split_name: str, split: Any, total_frames: int) -> list[_SegmentDescriptor]:
    lengths, strides = _resolve_segments_for_split(split, total_frames)
    out = [_SegmentDescriptor(length=int(L), stride=max(1, int(s))) for L, s in zip(lengths, strides)]
    consumed = sum(d.length for d in out)
    if consumed != int(total_frames):
        raise ValueError(f"Segment metadata for split '{split_name}' spans {consumed} frames "
                         f"but split contains {total_frames} frames")
    if not out:
        raise ValueError(f"No segment descriptors available for split '{split_name}'")
    return out


def _prepare_tau_grid(taus: Sequence[int]) -> list[int]:
    """0 followed by the distinct lags >= 1 in ascending order."""
    return [0] + sorted({int(t) for t in taus if int(t) >= 1})


def _integrated_autocorrelation_time(taus: Sequence[int], values: Sequence[float]) -> float:
    """1 + 2 x trapezoid of the curve from lag 0 up to the first non-positive or non-finite value; at least 1."""
    if len(taus) != len(values) or not taus:
        return float("nan")
    tau_int, last_tau, last_val = 1.0, 0.0, 1.0
    for tau, rho in zip(np.asarray(taus, np.float64)[1:], np.asarray(values, np.float64)[1:]):
        if not np.isfinite(rho) or rho <= 0.0:
            break
        delta = tau - last_tau
        if delta <= 0.0:
            continue
        tau_int += 2.0 * (0.5 * (last_val + rho)) * delta
        last_tau, last_val = tau, rho
    return float(max(1.0, tau_int))


def _recommend_ck_lags(tau_int: float, tau_limit: int) -> tuple[list[int], tuple[int, int] | None]:
    """Up to five geometrically spaced lags in [ceil(2 tau_int), ceil(min(5 tau_int, tau_limit))]."""
    if not np.isfinite(tau_int) or tau_int <= 0.0:
        return [], None
    lower = max(1, int(np.ceil(_MIN_CK_MULTIPLIER * tau_int)))
    upper = max(lower, int(np.ceil(min(_MAX_CK_MULTIPLIER * tau_int, tau_limit))))
    if upper == lower:
        return [lower], (lower, upper)
    raw = np.geomspace(lower, upper, num=min(5, upper - lower + 1))
    lags = sorted({max(lower, min(upper, int(round(v)))) for v in raw})
    if lags[0] > lower:
        lags.insert(0, lower)
    if lags[-1] < upper:
        lags.append(upper)
    return lags, (lower, upper)


class CanonicalCorrelationError(ValueError):
    """Base error raised when canonical correlation computation fails."""


class InsufficientSamplesError(CanonicalCorrelationError):
    """Raised when there are not enough paired samples (need at least 2)."""


# -- canonical correlations ---------------------------------------------------------------------------------

def _extract_optional_inputs(split: Mapping[str, Any]) -> np.ndarray | None:
    """The first 2-D, non-empty, finite array under the candidate keys."""
    for key in _INPUT_KEYS:
        value = split.get(key)
        if value is None:
            continue
        arr = np.asarray(value, dtype=np.float64)
        if arr.ndim != 2 or arr.shape[0] == 0 or not np.isfinite(arr).all():
            continue
        return arr
    return None


def _validate_canonical_inputs(X: np.ndarray, Y: np.ndarray) -> int:
    if X.ndim != 2 or Y.ndim != 2:
        raise CanonicalCorrelationError("X and Y must be 2D arrays")
    if not np.isfinite(X).all() or not np.isfinite(Y).all():
        raise CanonicalCorrelationError("X and Y must contain only finite values")
    n = min(int(X.shape[0]), int(Y.shape[0]))
    if n < 2:
        logger.error("Canonical correlation: insufficient paired samples (n=%d < 2)", n)
        raise InsufficientSamplesError(f"Need at least 2 paired samples, got {n}")
    return n


def _whitener(C: np.ndarray) -> np.ndarray:
    """W [p, r] with W' C W = I on the numerical range of the covariance block C (r = its rank)."""
    d = np.sqrt(np.clip(np.diag(C), 0.0, None))
    keep = d > 0.0
    if not keep.any():
        return np.zeros((C.shape[0], 0))
    inv_d = np.where(keep, 1.0 / np.where(keep, d, 1.0), 0.0)
    R = C * inv_d[:, None] * inv_d[None, :]          # correlation matrix: the cut-off does not see column scales
    lam, V = np.linalg.eigh(0.5 * (R + R.T))
    sel = lam > _RANK_CUTOFF * max(float(lam[-1]), 0.0)
    return (inv_d[:, None] * V[:, sel]) / np.sqrt(lam[sel])[None, :]


def _correlations_from_moments(mom: np.ndarray, n: int, p: int, q: int) -> list[float]:
    """Singular values of the whitened cross block of the joint covariance, descending, padded with zeros."""
    w = p + q
    s1 = mom[2 * w * w:2 * w * w + w] / float(n)               # residual mean about the shift
    C = 0.5 * mom[:w * w].reshape(w, w) / float(n) - np.outer(s1, s1)
    C = 0.5 * (C + C.T)
    Wx, Wy = _whitener(C[:p, :p]), _whitener(C[p:, p:])
    k = min(p, q, n)
    out = np.zeros(k)
    if Wx.shape[1] and Wy.shape[1]:
        sv = np.linalg.svd(Wx.T @ C[:p, p:] @ Wy, compute_uv=False)
        m = min(k, sv.shape[0])
        out[:m] = np.clip(sv[:m], 0.0, 1.0)
    return [float(v) for v in out]


def _canonical_correlations(X: np.ndarray, Y: np.ndarray, *, x_device=None, y_device=None) -> list[float]:
    """Canonical correlations of the paired samples X [n, p], Y [n, q]: min(p, q, n) values in descending order,
    0.0 beyond the rank of either block.  ``x_device`` / ``y_device``: the same arrays already on the device
    (any row count >= the common length)."""
    X, Y = np.asarray(X), np.asarray(Y)
    n = _validate_canonical_inputs(X, Y)
    p, q = int(X.shape[1]), int(Y.shape[1])
    if min(p, q, n) <= 0:
        return []
    if p + q > _MAX_JOINT_WIDTH:
        raise NotImplementedError(f"canonical correlations support up to {_MAX_JOINT_WIDTH} columns in all, "
                                  f"got {p} + {q}")
    eng = get_engine()
    xd = x_device if x_device is not None else eng.to_device(np.ascontiguousarray(X, np.float64))
    yd = y_device if y_device is not None else eng.to_device(np.ascontiguousarray(Y, np.float64))
    # the leading n rows of a row-major array are a prefix of its memory
    joint = eng.hstack(xd.view((n, p)), yd.view((n, q)))
    mean, _, _ = eng.column_moments(joint, ddof=0)
    mom = eng.lagged_moments(joint, 0, mean, assume_finite=True).to_host()
    return _correlations_from_moments(mom, n, p, q)


# -- autocorrelation ------------------------------------------------------------------------------------------

def _nan_curve(tau_grid: Sequence[int]) -> Dict[str, Any]:
    return {"taus": [int(t) for t in tau_grid], "values": [float("nan") for _ in tau_grid], "tau_int": float("nan"),
            "lag_window": None, "recommended_ck_lags": []}


def _combine_segments(tau_grid: Sequence[int], lengths: Sequence[int], seg_values: np.ndarray) -> Dict[str, Any]:
    """The curve from the per-segment values [n_seg, len(tau_grid) - 1] of the lags tau_grid[1:]: segments weigh
    L - tau; a segment with L <= 1, tau >= L or a non-finite value is left out; clipped to [-1, 1]; 1 at lag 0."""
    lengths = [int(v) for v in lengths]
    num, den = np.zeros(len(tau_grid)), np.zeros(len(tau_grid))
    for s, L in enumerate(lengths):
        if L <= 1:
            continue
        for idx, tau in enumerate(tau_grid[1:], start=1):
            v = float(seg_values[s, idx - 1])
            if tau >= L or not np.isfinite(v):
                continue
            num[idx] += (L - tau) * v
            den[idx] += L - tau
    averaged = np.full(len(tau_grid), np.nan)
    mask = den > 0.0
    averaged[mask] = num[mask] / den[mask]
    averaged = np.clip(averaged, -1.0, 1.0)
    averaged[0] = 1.0
    values = [float(v) if np.isfinite(v) else float("nan") for v in averaged]
    bad = [i for i, v in enumerate(values) if not np.isfinite(v)]
    if bad:
        logger.warning("Autocorrelation: %d/%d NaN values in curve (first indices: %s)", len(bad), len(values), bad[:10])
    usable = [L for L in lengths if L > 1]
    shortest = min(usable) if usable else min(lengths)
    tau_limit = max(1, int(np.floor(shortest * _MAX_TAU_FRACTION)))
    taus = [int(t) for t in tau_grid]
    tau_int = _integrated_autocorrelation_time(taus, values)
    lags, window = _recommend_ck_lags(tau_int, tau_limit)
    return {"taus": taus, "values": values, "tau_int": float(tau_int), "lag_window": window,
            "recommended_ck_lags": lags}


def _autocorrelation_curve(X, taus: Sequence[int], segments: Sequence[_SegmentDescriptor], *,
                           device_array=None) -> Dict[str, Any]:
    """Segment-wise autocorrelation of the standardised columns and its summary statistics.
    ``device_array``: X already on the device."""
    tau_grid = _prepare_tau_grid(taus)
    shape = device_array.shape if device_array is not None else np.shape(X)
    if len(shape) != 2 or shape[0] < 2:
        logger.warning("Autocorrelation: invalid input; returning NaNs for %d taus", len(tau_grid))
        return _nan_curve(tau_grid)
    n = int(shape[0])
    lengths = [int(d.length) for d in segments]
    stops = np.cumsum(np.asarray(lengths, np.int64))
    if len(stops) and stops[-1] > n and any(L > 1 for L in lengths):
        raise ValueError(f"Segment descriptors exceed split length ({int(stops[-1])} > {n})")
    if not len(stops) or stops[-1] != n:
        raise ValueError(f"Segment metadata consumed {int(stops[-1]) if len(stops) else 0} frames "
                         f"but split contains {n}")
    starts = stops - np.asarray(lengths, np.int64)
    if len(tau_grid) == 1:
        return _combine_segments(tau_grid, lengths, np.zeros((len(lengths), 0)))
    eng = get_engine()
    if device_array is None:
        arr = np.asarray(X)
        if arr.dtype not in (np.float32, np.float64):
            arr = arr.astype(np.float64)
        device_array = eng.to_device(np.ascontiguousarray(arr))
    value, _ = eng.autocorr_lagscan(device_array, tau_grid[1:], starts=starts, stops=stops, var_floor=_VAR_FLOOR)
    return _combine_segments(tau_grid, lengths, value.to_host())


# -- tau derivation --------------------------------------------------------------------------------------------

def _validate_user_taus(user_taus: Sequence[int], min_length: int) -> list[int]:
    """Integers >= 1, strictly increasing (repeats dropped), at least one below the shortest split."""
    if user_taus is None or len(user_taus) == 0:
        raise ValueError("Provided taus sequence is empty")
    cleaned: list[int] = []
    last = 0
    for raw in user_taus:
        if not isinstance(raw, (int, np.integer)):
            raise ValueError(f"Tau '{raw}' is not an integer")
        t = int(raw)
        if t < 1:
            raise ValueError(f"Tau must be >=1, got {t}")
        if t in cleaned:
            continue
        if t <= last:
            raise ValueError("Taus must be strictly increasing")
        cleaned.append(t)
        last = t
    if all(t >= min_length for t in cleaned):
        raise ValueError(f"All taus ({cleaned}) are >= minimum split length {min_length}; would yield all NaNs")
    return cleaned


def derive_taus(dataset: DatasetLike | Sequence[int], *, max_lags: int = 10, min_lag: int = 1,
                fraction_max: float = _MAX_TAU_FRACTION, geometric: bool = True,
                base: Sequence[int] | None = None) -> list[int]:
    """A validated list of autocorrelation lags for a dataset (or a list of segment lengths): geometrically
    spaced between min_lag and fraction_max of the shortest segment, or the usable entries of ``base``."""
    if max_lags < 1:
        raise ValueError(f"max_lags must be >=1, got {max_lags}")
    if min_lag < 1:
        raise ValueError(f"min_lag must be >=1, got {min_lag}")
    if not 0 < fraction_max <= 1:
        raise ValueError(f"fraction_max must be in (0,1], got {fraction_max}")
    lengths, strides = _collect_tau_lengths(dataset)
    min_length = min(lengths)
    if min_length <= min_lag:
        raise ValueError(f"Minimum split length {min_length} is not greater than min_lag {min_lag}; cannot derive taus.")
    lag_floor = max(min_lag, min(strides) if strides else 1)
    if geometric:
        taus = _derive_geometric_taus(min_length, lag_floor, fraction_max, max_lags, base)
    else:
        taus = _derive_base_taus(base, min_length, lag_floor)
    logger.info("Derived taus %s (strategy=%s, min_length=%d, n_splits=%d)", taus,
                "geometric" if geometric else "base-filter", min_length, len(lengths))
    return taus


def _collect_tau_lengths(dataset: DatasetLike | Sequence[int]) -> tuple[list[int], list[int]]:
    if isinstance(dataset, Mapping):
        lengths: list[int] = []
        strides: list[int] = []
        for value in _normalise_splits(dataset).values():
            try:
                arr = _coerce_array(value)
            except Exception as exc:  # pragma: no cover - defensive
                logger.debug("Skipping split during tau derivation: %s", exc)
                continue
            seg_l, seg_s = _resolve_segments_for_split(value, arr.shape[0])
            lengths.extend(int(v) for v in seg_l)
            strides.extend(max(1, int(v)) for v in seg_s)
    else:
        lengths = [int(v) for v in dataset]
        strides = [1] * len(lengths)
    if not lengths:
        raise ValueError("No split lengths available for tau derivation")
    if any(v <= 0 for v in lengths):
        raise ValueError(f"Non-positive split length encountered: {lengths}")
    return lengths, strides


def _derive_geometric_taus(min_length: int, min_lag: int, fraction_max: float, max_lags: int, base) -> list[int]:
    if base is not None:
        logger.warning("derive_taus: 'base' provided but ignored because geometric=True")
    upper = min(int(max(min_lag + 1, np.floor(min_length * fraction_max))), min_length - 1)
    if upper <= min_lag:
        raise ValueError(f"Upper bound {upper} not greater than min_lag {min_lag}; cannot derive taus.")
    raw = np.exp(np.linspace(np.log(min_lag), np.log(upper), num=max_lags))
    taus: list[int] = []
    for cand in (int(round(v)) for v in raw):
        if min_lag <= cand < min_length and cand > (taus[-1] if taus else 0):
            taus.append(cand)
    if not taus:
        raise ValueError("Geometric tau derivation yielded empty set "
                         f"(min_length={min_length}, min_lag={min_lag}, upper={upper}).")
    return taus


def _derive_base_taus(base, min_length: int, min_lag: int) -> list[int]:
    if base is None:
        raise ValueError("Non-geometric tau derivation requires a 'base' sequence")
    if len(base) == 0:
        raise ValueError("Base tau candidate sequence is empty")
    invalid = [c for c in base if not isinstance(c, (int, np.integer)) or int(c) <= 0]
    if invalid:
        raise ValueError(f"Base tau sequence must contain only positive integers, got invalid entries {invalid}")
    taus: list[int] = []
    for cand in (int(c) for c in base):
        if min_lag <= cand < min_length and cand not in taus:
            taus.append(cand)
    if not taus:
        raise ValueError("Base tau filtering produced empty set "
                         f"(base={list(base)}, min_length={min_length}, min_lag={min_lag})")
    return taus


# -- public entry ----------------------------------------------------------------------------------------------

def compute_diagnostics(dataset: DatasetLike, *, diag_mass: float | None = None,
                        taus: Sequence[int] | None = None) -> Dict[str, Any]:
    """Canonical correlations between inputs and CVs, the autocorrelation curve of the CVs and the warnings drawn
    from them, per split.  ``taus`` None: lags derived geometrically from the split lengths; given lags are
    validated strictly."""
    splits = _normalise_splits(dataset)
    lengths: list[int] = []
    for value in splits.values():
        try:
            lengths.append(int(_coerce_array(value).shape[0]))
        except Exception as exc:  # pragma: no cover - defensive
            logger.debug("Skipping length collection for a split: %s", exc)
    if not lengths:
        raise ValueError("Could not determine split lengths for tau derivation")
    min_length = min(lengths)
    if taus is None:
        taus_used = derive_taus(lengths)
    else:
        taus_used = _validate_user_taus(taus, min_length)
        logger.info("Validated user taus %s (min split length %d)", taus_used, min_length)

    canonical: Dict[str, list[float]] = {}
    autocorr: Dict[str, Dict[str, Any]] = {}
    warnings: list[str] = []
    for name, split in splits.items():
        processed = _compute_split_diagnostics(name, split, taus_used)
        if processed is None:
            continue
        split_canonical, split_autocorr, split_warnings = processed
        if split_canonical:
            canonical[name] = split_canonical
        autocorr[name] = split_autocorr
        warnings.extend(split_warnings)

    if diag_mass is not None and np.isfinite(diag_mass) and diag_mass > 0.95:
        msg = f"MSM diagonal mass high ({diag_mass:.3f})"
        warnings.append(msg)
        logger.warning(msg)
    return {"canonical_correlation": canonical, "autocorrelation": autocorr,
            "diag_mass": float(diag_mass) if diag_mass is not None else None, "taus": list(taus_used),
            "warnings": warnings}


def _compute_split_diagnostics(name: str, split: Any, taus: Sequence[int]):
    """(canonical correlations or None, autocorrelation summary, warnings) of one split; None when the split
    cannot be read as an array."""
    try:
        X = _coerce_array(split)
    except Exception as exc:  # pragma: no cover - defensive
        logger.debug("Skipping diagnostic split %s: %s", name, exc)
        return None
    metadata = split.get("meta") if isinstance(split, Mapping) else None
    whitened = apply_whitening_from_metadata(X, metadata)[0] if metadata is not None else X
    n = int(whitened.shape[0])
    xd = get_engine().to_device(np.ascontiguousarray(whitened, np.float64))   # the one upload of this split

    canonical: list[float] | None = None
    warnings: list[str] = []
    inputs = _extract_optional_inputs(split) if isinstance(split, Mapping) else None
    if inputs is not None:
        length = min(int(inputs.shape[0]), n)
        try:
            correlations = _canonical_correlations(inputs[:length], whitened[:length], y_device=xd)
        except InsufficientSamplesError:
            logger.error("%s: insufficient samples for canonical correlation (need >=2)", name)
            raise
        except CanonicalCorrelationError as exc:
            msg = f"{name}: canonical correlation failed ({exc})"
            warnings.append(msg)
            logger.warning(msg)
        else:
            if correlations:
                canonical = correlations
                if min(correlations) > 0.95:
                    msg = f"{name}: CVs reparametrize inputs"
                    warnings.append(msg)
                    logger.warning(msg)

    descriptors = _segment_descriptors_for_split(name, split, n)
    autocorr = _autocorrelation_curve(whitened, taus, descriptors, device_array=xd)
    values = autocorr.get("values", [])
    if len(values) >= 4 and np.isfinite(values[1]) and np.isfinite(values[3]):
        if abs(values[1] - values[3]) < 0.05:
            msg = f"{name}: CV autocorrelation flat across early lags"
            warnings.append(msg)
            logger.warning(msg)
    return canonical, autocorr, warnings
