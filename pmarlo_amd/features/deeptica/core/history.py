"""vamp2_proxy: mirror of pmarlo.features.deeptica.core.history.vamp2_proxy (S/features/deeptica/core/history.py:57-73),
the quick score recorded as vamp2_before / vamp2_after.  Host code on the [n, n_out] outputs the device hands back."""

from __future__ import annotations

from typing import Iterable

import numpy as np

__all__ = ["vamp2_proxy"]

_TINY = 1e-12      # S/constants.py: NUMERIC_MIN_POSITIVE


def vamp2_proxy(Y: np.ndarray, idx_t: Iterable[int], idx_tau: Iterable[int]) -> float:
    """Mean over the output columns of the squared Pearson correlation between the column at the t frames and at
    the tau frames (sample statistics; each standard deviation padded by 1e-12).  0.0 without outputs or pairs, and
    for a single pair."""
    Y = np.asarray(Y)
    it = np.asarray(list(idx_t), dtype=int)
    itau = np.asarray(list(idx_tau), dtype=int)
    if Y.size == 0 or it.size == 0 or itau.size == 0 or it.size <= 1:
        return 0.0
    a = np.asarray(Y[it], np.float64)
    b = np.asarray(Y[itau], np.float64)
    a = a - a.mean(axis=0, keepdims=True)
    b = b - b.mean(axis=0, keepdims=True)
    a = a / (a.std(axis=0, ddof=1) + _TINY)
    b = b / (b.std(axis=0, ddof=1) + _TINY)
    r = (a * b).sum(axis=0) / float(a.shape[0] - 1)
    return float(np.mean(r * r))
