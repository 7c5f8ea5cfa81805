"""Plain numpy restatements of the counting operations (pmarlo_amd/csrc/counts.hip), and the label and segment
generators the counting tests share.  tests/test_counts_reference.py checks them against oracle/cport and
oracle/npport on a machine without a GPU; tests/test_gpu_counts_paths.py compares the kernels with them.

Everything here is exact: integers, or (weighted) one correctly rounded `math.fsum` per bin, which does not depend
on the order of the terms."""

from __future__ import annotations

import math

import numpy as np

from tests import _gen

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


# ---- the operations -----------------------------------------------------------------------------------------------
def pair_starts(n: int, lag: int, segments=None, stride: int = 1) -> np.ndarray:
    """Start frame t of every pair (t, t + lag), in segment order.  Segments are clipped to [0, n]; a segment of
    at most `lag` frames has no pair.  segments=None: one segment over everything."""
    segments = [(0, n)] if segments is None else segments
    parts = []
    for a, b in segments:
        a, b = max(int(a), 0), min(int(b), n)
        if b - a <= lag:
            continue
        parts.append(np.arange(a, b - lag, stride, dtype=np.int64))
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def total_pairs(n: int, lag: int, segments=None, stride: int = 1) -> int:
    """Pair positions (valid labels or not): what the dispatch of the count kernels sees."""
    return int(pair_starts(n, lag, segments, stride).size)


def _valid_pairs(labels, k, lag, segments, stride):
    lab = np.asarray(labels, np.int64)
    t = pair_starts(lab.size, lag, segments, stride)
    a, b = lab[t], lab[t + lag]
    ok = (a >= 0) & (a < k) & (b >= 0) & (b < k)
    return t[ok], a[ok], b[ok]


def count_transitions(labels, k: int, lag: int, *, segments=None, stride: int = 1):
    """-> (counts int64 [k, k], pairs counted).  A pair counts only if both labels are in [0, k)."""
    _, a, b = _valid_pairs(labels, k, lag, segments, stride)
    c = np.bincount(a * k + b, minlength=k * k).astype(np.int64).reshape(k, k)
    return c, int(a.size)


def count_transitions_weighted(labels, weights, k: int, lag: int, *, segments=None, stride: int = 1):
    """-> (sums f64 [k, k], pairs counted, terms per bin int64 [k, k], sum |w| per bin f64 [k, k]).
    counts[a][b] = fsum of the weights of the STARTING frames of the pairs (a, b): correctly rounded."""
    w = np.asarray(weights, np.float64)
    t, a, b = _valid_pairs(labels, k, lag, segments, stride)
    key = a * k + b
    order = np.argsort(key, kind="stable")
    key, wt = key[order], w[t[order]]
    terms = np.bincount(key, minlength=k * k).astype(np.int64)
    cuts = np.concatenate([[0], np.cumsum(terms)])
    out, mass = np.zeros(k * k), np.zeros(k * k)
    for i in np.flatnonzero(terms):
        seg = wt[cuts[i]:cuts[i + 1]].tolist()
        out[i] = math.fsum(seg)
        mass[i] = math.fsum(abs(x) for x in seg)
    return out.reshape(k, k), int(a.size), terms.reshape(k, k), mass.reshape(k, k)


def state_counts(labels, k: int) -> np.ndarray:
    lab = np.asarray(labels, np.int64)
    return np.bincount(lab[(lab >= 0) & (lab < k)], minlength=k).astype(np.int64)


def runs(labels, k: int):
    """Dwell runs: maximal stretches of one label in [0, k); any other label separates runs and belongs to none.
    -> (state of every run, its length, its first frame), in frame order."""
    lab = np.asarray(labels, np.int64)
    n = lab.size
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z, z
    edges = np.concatenate([[0], np.flatnonzero(lab[1:] != lab[:-1]) + 1, [n]])
    first, length = edges[:-1], np.diff(edges)
    state = lab[first]
    keep = (state >= 0) & (state < k)
    return state[keep], length[keep], first[keep]


def run_stats(labels, k: int) -> np.ndarray:
    """int64 [4, k]: min (-1 for a state without runs), max, sum and number of the run lengths per state."""
    state, length, _ = runs(labels, k)
    out = np.zeros((4, k), np.int64)
    out[0] = -1
    for s in np.unique(state):
        m = length[state == s]
        out[:, s] = m.min(), m.max(), m.sum(), m.size
    return out


def row_normalise(counts):
    """-> (T f64 [k, k] = C / row sum with zero rows left zero, rowsum f64 [k], trace(T) / k).  The diagonal is
    added up in ascending order with math.fsum's correctly rounded sum for reference only: compare the device's
    diagonal mass with the device's own two-call form bit for bit, and with this one to a few ulp."""
    c = np.asarray(counts, np.float64)
    rs = c.sum(axis=1)
    T = np.divide(c, rs[:, None], out=np.zeros_like(c), where=rs[:, None] > 0)
    return T, rs, math.fsum(np.diag(T).tolist()) / c.shape[0]


# ---- inputs --------------------------------------------------------------------------------------------------------
KINDS = ("markov", "random", "constant", "runs")


def labels_of_kind(kind: str, n: int, k: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "markov":
        return _gen.markov_labels(n, k, seed)
    if kind == "random":
        return rng.integers(0, k, n).astype(np.int32)
    if kind == "constant":
        return np.full(n, k - 1, np.int32)
    if kind == "runs":
        return np.repeat(rng.integers(0, k, n // 37 + 1), 37)[:n].astype(np.int32)
    if kind == "two_states":
        return (rng.integers(0, 2, n) * (k - 1)).astype(np.int32)
    raise ValueError(kind)


def sprinkle_invalid(labels: np.ndarray, k: int) -> np.ndarray:
    """-1, k, k + 5, INT32_MIN and INT32_MAX at co-prime strides: none may be counted, none may be written to."""
    lab = np.array(labels, np.int32)
    if lab.size > 100:
        lab[11::4099] = -1
        lab[3::7001] = k
        lab[7::9001] = k + 5
        lab[5::10007] = INT32_MIN
        lab[2::12011] = INT32_MAX
    return lab


def ragged_segments(n: int):
    """Empty, one-frame, clipped at both ends, and ordinary segments."""
    a, b = n // 3, (2 * n) // 3
    return [(-10, a), (a, a), (a + 1, a + 2), (a + 7, b), (b + 5, n + 50)]


def integer_weights(n: int, seed: int) -> np.ndarray:
    """Integer-valued weights in [1, 8): their fp64 sums are exact in any order."""
    return np.random.default_rng(seed).integers(1, 8, n).astype(np.float64)


# ---- the shapes of tests/test_gpu_counts_paths.py (for a device of 256 compute units) --------------------------------
# name -> (k, n, lag, label kinds).  What each shape is there for is asserted through Engine.count_plan by the GPU test.
UNWEIGHTED_SHAPES = {
    "privatised_8_row_blocks": (500, 249_000, 3, KINDS),
    "privatised_16_row_blocks": (700, 480_000, 1, KINDS),
    # 131072 // (4 k) rows of LDS bins a workgroup: 45 at k = 720 .. 728, and 16 x 45 = 720
    "privatised_last_k": (720, 480_000, 1, ("markov", "random")),
    "global_first_k": (721, 300_000, 1, ("markov", "random")),
    "global_k725": (725, 300_000, 1, KINDS),
    "bucket_key_space_limit": (2048, 4_200_000, 3, KINDS + ("two_states",)),
    "past_the_bucket_limit": (2049, 4_210_000, 3, KINDS),
}
# name -> (k, n, lag, stride, path): ragged_segments(n), kinds "markov" and "random"
RAGGED_SHAPES = {
    "bucket": (300, 300_000, 2, 3, "bucket"),
    "privatised": (700, 480_000, 1, 3, "privatised"),
    "global": (725, 300_000, 1, 3, "global"),
}
WEIGHTED_LAG = 2
# name -> (k, n for n_cu compute units)
WEIGHTED_SHAPES = {
    "budget_switch_small_side": (90, lambda n_cu: 300_000),
    "budget_switch_large_side": (91, lambda n_cu: 300_000),
    # more than 4096 pairs for each of n_cu chunks
    "single_block_unrolled": (128, lambda n_cu: max(1_100_000, 4096 * n_cu + 51_424)),
    "several_row_blocks": (300, lambda n_cu: 300_000),
    "sixteen_row_blocks": (512, lambda n_cu: 200_000),
    "global": (513, lambda n_cu: 200_000),
}
LAGSCAN = dict(k=200, n=60_000, lags=(1, 7, 20_000, 30_000, 59_990, 59_999, 60_000),
               segments=[(0, 25_000), (25_000, 60_000)])
CAPTURE = dict(k=500, n=1_000_000, lag=10)
STATE_COUNTS_N = 300_000
RUN_LENGTHS_N = 300_000
