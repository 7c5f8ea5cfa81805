"""numpy restatement of the silhouette coefficient in the difference form, for the tests of msm_silhouette_samples.

d(i, j) = sqrt(sum_f (x_if - x_jf)^2) is taken feature by feature from the differences themselves, never from
x.x - 2 x.y + y.y (what sklearn's pairwise distances expand to), so two near points far from the origin keep their
distance.  The queries go by in chunks; a chunk costs chunk * n doubles."""

from __future__ import annotations

import numpy as np


def silhouette_samples_ref(X: np.ndarray, labels: np.ndarray, k: int | None = None, chunk: int = 512) -> np.ndarray:
    """s_i for dense ids 0 .. k-1 (an id may have no member): a_i = mean distance to the other members of i's
    cluster, b_i = smallest mean distance to the members of another non-empty cluster, s_i = (b_i - a_i) / max(a_i,
    b_i); 0 for the member of a singleton cluster and where max(a_i, b_i) = 0.
    NaN rule (include/msmhip.h): the sums are ordinary IEEE sums, the minimum in b_i and the maximum in the denominator
    keep NaN, "another cluster exists" is decided by the counts; finite input gives the bits it always gave."""
    X = np.ascontiguousarray(X, np.float64)
    labels = np.asarray(labels).astype(np.int64)
    n, d = X.shape
    k = int(labels.max()) + 1 if k is None else int(k)
    assert labels.shape == (n,) and labels.min() >= 0 and labels.max() < k
    counts = np.bincount(labels, minlength=k)
    order = np.argsort(labels, kind="stable")
    occupied = np.flatnonzero(counts > 0)
    starts = (np.cumsum(counts) - counts)[occupied]
    col_of = np.full(k, -1, np.int64)
    col_of[occupied] = np.arange(occupied.size)
    Xs = X[order]
    out = np.zeros(n)
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        d2 = np.zeros((i1 - i0, n))
        with np.errstate(invalid="ignore", over="ignore"):
            for f in range(d):
                diff = X[i0:i1, f, None] - Xs[None, :, f]
                d2 += diff * diff
        sums = np.add.reduceat(np.sqrt(d2), starts, axis=1)          # [m, occupied clusters]
        rows = np.arange(i1 - i0)
        own = col_of[labels[i0:i1]]
        n_own = counts[labels[i0:i1]]
        a = sums[rows, own] / np.maximum(n_own - 1, 1)
        mean = sums / counts[occupied][None, :]
        mean[rows, own] = np.inf
        b = mean.min(axis=1)                      # np.min and np.maximum keep NaN
        den = np.maximum(a, b)
        ok = (n_own > 1) & (occupied.size > 1) & ~(den == 0)
        with np.errstate(invalid="ignore"):
            out[i0:i1] = np.where(ok, (b - a) / np.where(ok, den, 1.0), 0.0)
    return out


def recipe_labels(n: int, k: int) -> np.ndarray:
    """The labels of test_silhouette_score_vs_sklearn (random ids, id k-1 a singleton at frame 0), plus a cluster of
    exactly two members (id k-3, frames 1 and 2) and an id without any member (k-5)."""
    rng = np.random.default_rng(n + k)
    labels = rng.integers(0, k, n)
    labels[:k] = np.arange(k)
    labels[labels == k - 1] = k - 2
    labels[0] = k - 1
    labels[labels == k - 3] = k - 4
    labels[1:3] = k - 3
    labels[labels == k - 5] = k - 6
    return labels
