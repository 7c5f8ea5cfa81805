"""The numpy restatements of tests/_counts_ref.py against oracle/cport and oracle/npport (no GPU), at every shape
tests/test_gpu_counts_paths.py feeds the kernels -- segments, stride and the sprinkled invalid labels included.

  test_unweighted_shapes     count_transitions / state_counts vs cport (the C restatement) at the unweighted shapes
  test_ragged_shapes         the same with ragged_segments and stride 3; total_pairs vs npport.expected_pairs
  test_weighted_shapes       the per-bin fsum vs cport's running fp64 sum: equal, since integer weights add exactly
  test_weighted_fsum_bound   non-integer weights: cport's running sum lies within the bound the GPU test uses
  test_lagscan_shapes        every lag of the scan, one and two segments; the shape of the capture test
  test_state_counts_shapes   state visits at k = 1, 16384 and 16385 vs cport
  test_row_normalise         vs npport.normalise_counts
  test_runs                  vs the edges-based code of test_gpu_debug_export.py, and a frame-by-frame walk when
                             labels >= k separate runs
  test_constants_mirror_the_header  the thresholds pmarlo_amd._lib restates (LDS limit of the state visits, k-means++
                             block, count paths) against include/msmhip.h
  test_numpy_port_agrees     npport.weighted_counts (the reference's own numpy form) where no label is >= k
"""

from __future__ import annotations

import numpy as np
import pytest

from oracle import cport, npport
from tests import _counts_ref as ref

N_CU = 256


def _labels(kind, n, k, seed=1):
    return ref.sprinkle_invalid(ref.labels_of_kind(kind, n, k, seed), k)


@pytest.mark.parametrize("name", list(ref.UNWEIGHTED_SHAPES))
def test_unweighted_shapes(name):
    k, n, lag, kinds = ref.UNWEIGHTED_SHAPES[name]
    for kind in kinds:
        lab = _labels(kind, n, k)
        want, pw = cport.count_transitions(lab, k, lag)
        got, pg = ref.count_transitions(lab, k, lag)
        np.testing.assert_array_equal(got, want)
        assert pg == pw and ref.total_pairs(n, lag) == n - lag
    np.testing.assert_array_equal(ref.state_counts(lab, k), cport.state_counts(lab, k))


@pytest.mark.parametrize("name", list(ref.RAGGED_SHAPES))
def test_ragged_shapes(name):
    k, n, lag, stride, _ = ref.RAGGED_SHAPES[name]
    segs = ref.ragged_segments(n)
    for kind in ("markov", "random"):
        lab = _labels(kind, n, k)
        want, pw = cport.count_transitions(lab, k, lag, segments=segs, stride=stride)
        got, pg = ref.count_transitions(lab, k, lag, segments=segs, stride=stride)
        np.testing.assert_array_equal(got, want)
        assert pg == pw
    lengths = [min(b, n) - max(a, 0) for a, b in segs]
    assert ref.total_pairs(n, lag, segs, stride) == npport.expected_pairs(lengths, lag, stride)


@pytest.mark.parametrize("name", list(ref.WEIGHTED_SHAPES))
def test_weighted_shapes(name):
    k, n_of = ref.WEIGHTED_SHAPES[name]
    n = n_of(N_CU)
    w = ref.integer_weights(n, k)
    for kind in ref.KINDS:
        lab = _labels(kind, n, k)
        want, pw = cport.count_transitions(lab, k, ref.WEIGHTED_LAG, weights=w)
        got, pg, terms, mass = ref.count_transitions_weighted(lab, w, k, ref.WEIGHTED_LAG)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(terms, ref.count_transitions(lab, k, ref.WEIGHTED_LAG)[0])
        np.testing.assert_array_equal(mass, got)
        assert pg == pw
    segs = ref.ragged_segments(n)
    want, pw = cport.count_transitions(lab, k, ref.WEIGHTED_LAG, segments=segs, stride=3, weights=w)
    got, pg, _, _ = ref.count_transitions_weighted(lab, w, k, ref.WEIGHTED_LAG, segments=segs, stride=3)
    np.testing.assert_array_equal(got, want)
    assert pg == pw


def test_weighted_fsum_bound():
    k, n = 300, 300_000
    w = np.random.default_rng(5).lognormal(size=n)
    lab = _labels("markov", n, k)
    run, _ = cport.count_transitions(lab, k, ref.WEIGHTED_LAG, weights=w)
    exact, _, terms, mass = ref.count_transitions_weighted(lab, w, k, ref.WEIGHTED_LAG)
    assert terms.max() > 100                                    # bins with many terms: the bound is not vacuous
    assert np.all(np.abs(run - exact) <= terms * 2.0**-52 * mass)
    assert np.any(run != exact)                                 # and fsum is not the running sum restated


def test_lagscan_shapes():
    k, n = ref.LAGSCAN["k"], ref.LAGSCAN["n"]
    lab = _labels("markov", n, k)
    for segs in (None, ref.LAGSCAN["segments"]):
        for lag in ref.LAGSCAN["lags"]:
            want, pw = cport.count_transitions(lab, k, lag, segments=segs)
            got, pg = ref.count_transitions(lab, k, lag, segments=segs)
            np.testing.assert_array_equal(got, want)
            assert pg == pw
    assert ref.total_pairs(n, 20_000) == k * k and ref.total_pairs(n, n) == 0
    c = ref.CAPTURE
    lab = _labels("markov", c["n"], c["k"])
    np.testing.assert_array_equal(ref.count_transitions(lab, c["k"], c["lag"])[0],
                                  cport.count_transitions(lab, c["k"], c["lag"])[0])


def test_state_counts_shapes():
    for k in (1, 16384, 16385):
        n = 1 if k == 1 else ref.STATE_COUNTS_N
        lab = _labels("random", n, k)
        np.testing.assert_array_equal(ref.state_counts(lab, k), cport.state_counts(lab, k))


def test_row_normalise():
    lab = _labels("markov", 100_000, 300)
    c, _ = ref.count_transitions(lab, 300, 3)
    c[17] = 0                                                   # a state never left: its row stays zero
    T, rs, dm = ref.row_normalise(c)
    np.testing.assert_array_equal(T, npport.normalise_counts(c))
    np.testing.assert_array_equal(rs, c.sum(axis=1).astype(np.float64))
    assert T[17].sum() == 0.0 and abs(dm - np.trace(T) / 300) <= 1e-15


def _runs_by_walking(seq, k):
    out, t, n = [], 0, len(seq)
    while t < n:
        s = int(seq[t])
        u = t + 1
        while u < n and seq[u] == s:
            u += 1
        if 0 <= s < k:
            out.append((s, u - t, t))
        t = u
    return out


def test_runs():
    rng = np.random.default_rng(4)
    seq = np.repeat(rng.integers(0, 5, size=3000), rng.integers(1, 400, size=3000)).astype(np.int32)
    seq[100_000:100_050] = -1
    edges = np.flatnonzero(np.diff(np.concatenate([[-7], seq, [-7]])) != 0)
    want = [(int(seq[a]), int(b - a)) for a, b in zip(edges[:-1], edges[1:]) if seq[a] >= 0]
    st, ln, _ = ref.runs(seq, 5)
    assert list(zip(st.tolist(), ln.tolist())) == want
    # labels >= k, INT32_MIN / INT32_MAX and -1 all separate runs and own none
    seq = np.repeat(rng.integers(-1, 9, size=4000), rng.integers(1, 6, size=4000)).astype(np.int32)
    seq[::97] = ref.INT32_MAX
    seq[5::101] = ref.INT32_MIN
    st, ln, first = ref.runs(seq, 6)
    assert list(zip(st.tolist(), ln.tolist(), first.tolist())) == _runs_by_walking(seq, 6)
    stats = ref.run_stats(seq, 6)
    for s in range(6):
        m = ln[st == s]
        assert stats[:, s].tolist() == [m.min(), m.max(), m.sum(), m.size]
    assert ref.run_stats(np.full(10, 7, np.int32), 3).tolist() == [[-1] * 3, [0] * 3, [0] * 3, [0] * 3]
    for seq in (np.zeros(0, np.int32), np.asarray([2], np.int32), np.tile([0, 1], 50).astype(np.int32)):
        st, ln, first = ref.runs(seq, 3)
        assert list(zip(st.tolist(), ln.tolist(), first.tolist())) == _runs_by_walking(seq, 3)


def test_constants_mirror_the_header():
    """The thresholds the GPU tests place their shapes at are read from pmarlo_amd._lib: they must be the header's."""
    import re
    from pathlib import Path

    from pmarlo_amd import _lib

    text = (Path(__file__).resolve().parents[1] / "include" / "msmhip.h").read_text()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (MSM_[A-Z0-9_]+) (\d+)\s*$", text, flags=re.M)}
    assert defs["MSM_STATE_COUNTS_LDS_MAX_K"] == _lib.STATE_COUNTS_LDS_MAX_K
    assert defs["MSM_KPP_BLOCK"] == _lib.KPP_BLOCK
    assert [defs[f"MSM_COUNT_PATH_{p}"] for p in ("BUCKET", "PRIVATISED", "GLOBAL", "NONE")] == [
        _lib.COUNT_PATH_BUCKET, _lib.COUNT_PATH_PRIVATISED, _lib.COUNT_PATH_GLOBAL, _lib.COUNT_PATH_NONE]


def test_numpy_port_agrees():
    n, k = 50_000, 40
    lab = ref.labels_of_kind("markov", n, k, 2)
    lab[::501] = -1
    w = ref.integer_weights(n, 1)
    segs = ref.ragged_segments(n)
    want, pw = npport.weighted_counts(lab, k, 4, weights=w, segments=segs, stride=3)
    got, pg, _, _ = ref.count_transitions_weighted(lab, w, k, 4, segments=segs, stride=3)
    np.testing.assert_array_equal(got, want)
    assert pg == pw
    want, pw = npport.weighted_counts(lab, k, 4)
    got, pg = ref.count_transitions(lab, k, 4)
    np.testing.assert_array_equal(got, want.astype(np.int64))
    assert pg == pw
