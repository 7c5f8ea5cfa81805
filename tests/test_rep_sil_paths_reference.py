"""CPU checks of tests/_rep_sil_paths_ref.py: the longdouble laws against the fp64 restatements and sklearn, the
yardstick of the GPU bounds (what a plain fp64 numpy evaluation loses against the laws on the test inputs), and the
margins that make the exact comparison of picks in tests/test_gpu_rep_sil_paths.py meaningful."""

from __future__ import annotations

import numpy as np
import pytest

from tests import _gen
from tests import _rep_sil_paths_ref as P
from tests import _representatives_ref as R
from tests._silhouette_ref import recipe_labels, silhouette_samples_ref

U = P.U


# ---- the laws against what the suite already trusts -----------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.GOLDEN_CASES])
def test_laws_agree_with_the_fp64_restatements_on_the_golden_cases(name):
    x, dtrajs, state_ids, weights, n_reps = R.golden_case(name)
    labels = np.concatenate(dtrajs)
    offsets, members = P.group_ref(labels, int(labels.max()) + 1)
    for s in state_ids:
        frames = np.where(labels == s)[0]
        assert np.array_equal(members[offsets[s]:offsets[s + 1]], frames)
        cen = R.centroid(x[frames], weights, frames)
        np.testing.assert_allclose(np.asarray(P.centroid_law(x, frames, weights)[0], np.float64), cen, rtol=1e-13, atol=1e-14)
        sc = R.centroid_scores(x, frames, weights)
        np.testing.assert_allclose(np.asarray(P.centroid_scores_law(x, frames, weights), np.float64), sc, rtol=1e-12)
        sm = R.medoid_scores(x, frames, weights)
        np.testing.assert_allclose(np.asarray(P.medoid_scores_law(x, frames, weights), np.float64), sm, rtol=1e-12)
        # the selection rules on the same fp64 scores: the same picks
        assert P.smallest_law(sm, frames, n_reps)[:min(n_reps, frames.size)] == R.smallest(sm, frames, n_reps)
        assert P.diverse_law(x, frames, sc, n_reps)[:min(n_reps, frames.size)] == R.diverse_walk(x, frames, weights, n_reps)


def test_silhouette_law_agrees_with_sklearn_and_the_fp64_restatement():
    from sklearn.metrics import silhouette_samples

    n, d, k = 500, 2, 4
    X, _ = _gen.gaussian_clusters(k, n // k + 1, d, seed=k)
    X = X[:n]
    labels = recipe_labels(n, 6)          # a singleton, a pair, an unused id
    law = np.asarray(P.silhouette_law(X, labels, 6), np.float64)
    np.testing.assert_allclose(law, silhouette_samples(X, labels), rtol=0, atol=1e-12)
    np.testing.assert_allclose(law, silhouette_samples_ref(X, labels, 6), rtol=0, atol=1e-13)


def test_extended_restatement_keeps_its_bits_on_finite_input(golden):
    """silhouette_samples_ref gained the NaN rule; on finite input it returns what it returned: the formula it had,
    restated here, gives the same bytes on the recipe cases."""
    for n, d, k in ((1500, 3, 33), (700, 256, 40)):
        X, labels = P.recipe_points(n, d, k)
        got = silhouette_samples_ref(X, labels, k)
        counts = np.bincount(labels, minlength=k)
        order = np.argsort(labels, kind="stable")
        occ = np.flatnonzero(counts > 0)
        starts = (np.cumsum(counts) - counts)[occ]
        col = np.full(k, -1)
        col[occ] = np.arange(occ.size)
        d2 = np.zeros((n, n))
        for f in range(d):
            diff = X[:, f, None] - X[order][None, :, f]
            d2 += diff * diff
        sums = np.add.reduceat(np.sqrt(d2), starts, axis=1)
        rows = np.arange(n)
        a = sums[rows, col[labels]] / np.maximum(counts[labels] - 1, 1)
        mean = sums / counts[occ][None, :]
        mean[rows, col[labels]] = np.inf
        b = mean.min(axis=1)
        den = np.maximum(a, b)
        ok = (counts[labels] > 1) & np.isfinite(b) & (den > 0)
        old = np.where(ok, (b - a) / np.where(ok, den, 1.0), 0.0)
        assert got.tobytes() == old.tobytes()
        # and the device, before it had the rule, was within the tolerance of it
        np.testing.assert_allclose(golden(P.BEFORE_NAN_RULE)[f"samples/{n}_{d}_{k}"], got, rtol=0, atol=P.SIL_ATOL)


def test_nan_rules_of_the_silhouette_law():
    X = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 2.0], [5.0, 5.0], [6.0, 5.0], [9.0, 9.0], [20.0, 0.0], [21.0, 0.0]])
    labels = np.array([0, 0, 0, 2, 2, 4, 5, 5])   # ids 1 and 3 unused, id 4 a singleton
    for fn in (lambda X: np.asarray(P.silhouette_law(X, labels, 6), np.float64), lambda X: silhouette_samples_ref(X, labels, 6)):
        base = fn(X)
        assert np.isfinite(base).all() and base[5] == 0.0
        Y = X.copy()
        Y[3, 0] = np.nan                      # a frame of cluster 2
        s = fn(Y)
        # every frame's b_i has to look at cluster 2 (or it is the frame's own cluster): NaN everywhere but the singleton
        assert s[5] == 0.0 and np.isnan(np.delete(s, 5)).all()
        Y = X.copy()
        Y[5, 1] = np.nan                      # the singleton
        s = fn(Y)
        assert s[5] == 0.0 and np.isnan(np.delete(s, 5)).all()
        Y = X.copy()
        Y[6, 0] = np.inf
        s = fn(Y)
        assert np.isnan(s[6]) and np.isnan(s[7])          # (inf - inf) / inf
        # the others see cluster 5 at mean distance inf: it never is the minimum, nothing changes
        np.testing.assert_array_equal(s[:6], base[:6])
    # one occupied cluster: 0, whatever the coordinates
    one = np.array([3, 3, 3, 3, 3, 3, 3, 3])
    assert not silhouette_samples_ref(X, one, 5).any() and not P.silhouette_law(X, one, 5).any()


def test_selection_laws_on_non_finite_scores():
    frames = np.array([3, 5, 8, 13, 21])
    assert P.smallest_law([np.nan] * 5, frames, 3) == [-1, -1, -1]
    assert P.smallest_law([2.0, np.nan, np.inf, 1.0, np.inf], frames, 5) == [13, 3, 8, 21, -1]
    assert P.smallest_law([0.0, -0.0, 1.0, -0.0, 0.0], frames, 4) == [3, 5, 13, 21]
    x = np.zeros((22, 1))
    x[frames, 0] = [0.0, 1.0, 5.0, 2.0, 9.0]
    assert P.diverse_law(x, frames, [np.nan] * 5, 3) == [3, 21, 8]          # starts at the first member
    x[8, 0] = np.nan
    assert P.diverse_law(x, frames, [1.0, 0.5, 2.0, 3.0, 4.0], 5) == [5, 21, 3, 13, -1]   # frame 8 is never picked
    assert P.diverse_law(x, frames, [1.0, 0.5, 0.1, 3.0, 4.0], 4) == [8, -1, -1, -1]      # the walk starts on it


# ---- the yardstick --------------------------------------------------------------------------------------------------
def _print(name, err, bound):
    print(f"yardstick {name}: plain fp64 numpy is off by {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{name}: the bound, not a kernel, is wrong ({err:.3e} > {bound:.3e})"


@pytest.mark.parametrize("d", P.CENTROID_D)
def test_yardstick_centroid_distance(d):
    x, labels, k, w = P.state_case(d, P.score_sizes(d), seed=100 + d)
    xmax = np.abs(x).max()
    for weights in (None, w):
        for s in range(k):
            frames = np.where(labels == s)[0]
            if frames.size == 0:
                continue
            err = float(np.abs(R.centroid_scores(x, frames, weights) - P.centroid_scores_law(x, frames, weights)).max())
            ns = frames.size
            bound = 4 * ns * U * np.sqrt(d) * xmax
            _print(f"centroid distance d={d} n_s={ns} weighted={weights is not None}", err, bound)


@pytest.mark.parametrize("d", P.MEDOID_D)
def test_yardstick_medoid_score(d):
    x, labels, k, w = P.state_case(d, P.MEDOID_SIZES, seed=200 + d)
    for weights in (None, w):
        worst = 0.0
        for s in range(k):
            frames = np.where(labels == s)[0]
            law = P.medoid_scores_law(x, frames, weights)
            got = R.medoid_scores(x, frames, weights)
            if frames.size == 1:
                assert got[0] == 0.0 and law[0] == 0.0
                continue
            err = float((np.abs(got - law) / law).max())
            _print(f"medoid score d={d} n_s={frames.size} weighted={weights is not None}", err, 4 * (frames.size + d) * U)
            worst = max(worst, err)


@pytest.mark.parametrize("name", list(P.SAMPLES_SHAPES))
def test_yardstick_silhouette_samples(name):
    X, labels, k, law = P.samples_case(name)
    err = float(np.abs(silhouette_samples_ref(X, labels, k) - law).max())
    _print(f"silhouette samples {name}", err, P.SIL_ATOL)


@pytest.mark.parametrize("k,d,n", P.SORTED_SHAPES)
def test_yardstick_silhouette_sorted(k, d, n):
    X, labels, offsets, law = P.sorted_case(k, d, n)
    assert offsets[-1] == n and np.array_equal(np.diff(offsets), np.bincount(labels, minlength=k))
    got = silhouette_samples_ref(X, labels, k)
    _print(f"silhouette sorted ({k}, {d}, {n})", float(np.abs(got - law).max()), P.SIL_ATOL)
    mean = float(law.mean())
    if mean != 0.0:
        _print(f"silhouette score ({k}, {d}, {n})", abs(got.mean() - mean) / abs(mean), P.SCORE_RTOL)


@pytest.mark.parametrize("name", list(P.NONFINITE))
def test_non_finite_cases_mark_what_they_should(name):
    X, labels, offsets, law, frame = P.nonfinite_case(name)
    ref = silhouette_samples_ref(X, labels, len(P.NONFINITE_SIZES))
    nan = np.isnan(law)
    assert np.array_equal(nan, np.isnan(ref)) and nan.any() and np.isnan(law.mean())
    np.testing.assert_allclose(ref[~nan], np.asarray(law[~nan], np.float64), rtol=0, atol=P.SIL_ATOL)
    if name == "nan_in_singleton":
        assert law[frame] == 0.0 and nan.sum() == labels.size - 1
    elif name == "nan_in_middle_cluster":
        assert nan.sum() == labels.size - 1      # all but the singleton
    else:
        # +inf: the frame and its cluster are NaN; the other frames see a mean of inf, never their minimum
        assert nan.sum() == P.NONFINITE_SIZES[2] and nan[labels == 2].all()


# ---- the condition for exact picks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in P.PICK_CASES])
def test_margins_of_the_full_path_pick_cases(name):
    x, labels, k, w, n_reps = P.pick_case(name)
    for weights in (None, w):
        for s in range(k):
            frames = np.where(labels == s)[0]
            cs = P.centroid_scores_law(x, frames, weights)
            ms = P.medoid_scores_law(x, frames, weights)
            margins = []
            P.diverse_law(x, frames, cs, n_reps, margins)
            got = min([P.smallest_margin(cs, n_reps), P.smallest_margin(ms, n_reps)] + margins)
            print(f"pick case {name} state {s} n_s={frames.size} weighted={weights is not None}: margin {got:.3e}")
            assert got >= P.MIN_MARGIN


@pytest.mark.parametrize("n_states", [1, 300])
@pytest.mark.parametrize("n_reps", P.SELECT_REPS)
@pytest.mark.parametrize("mode", ["smallest", "diverse"])
def test_margins_of_the_select_case(mode, n_reps, n_states):
    rows, margin = P.select_rows(mode, n_reps, n_states)
    print(f"select case {mode} n_reps={n_reps} n_states={n_states}: smallest margin {margin:.3e}")
    assert margin >= P.MIN_MARGIN
    sizes = P.select_case()[3]
    for row, s in zip(rows, P.select_states(n_states)):
        taken = min(n_reps, sizes[s])
        assert (row[:taken] >= 0).all() and (row[taken:] == -1).all() and len(set(row[:taken])) == taken


def test_margins_of_the_other_exact_pick_inputs():
    """The diverse walks of the pre-set score patterns, of the NaN-feature case and of the picker's NaN case."""
    margins = []
    x, _, k, offsets, members, scores = P.preset_case()
    for s in range(k):
        P.diverse_law(x, members[offsets[s]:offsets[s + 1]], scores[offsets[s]:offsets[s + 1]], P.PRESET_SIZE + 1, margins,
                      score_margin=False)
    print(f"preset scores: smallest margin of the diverse walks {min(margins):.3e}")
    assert min(margins) >= P.MIN_MARGIN
    margins = []
    x, _, k, offsets, members, scores = P.nan_feature_case()
    for s in range(k):
        P.diverse_law(x, members[offsets[s]:offsets[s + 1]], scores[offsets[s]:offsets[s + 1]], 40, margins, score_margin=False)
    print(f"NaN features: smallest margin of the diverse walks {min(margins):.3e}")
    assert min(margins) >= P.MIN_MARGIN
    margins = []
    x, _, _, frames1, _ = P.picker_nan_case()
    P.diverse_law(x, frames1, np.full(frames1.size, np.nan), frames1.size, margins, score_margin=False)
    print(f"picker NaN case: smallest margin of the diverse walk {min(margins):.3e}")
    assert min(margins) >= P.MIN_MARGIN


def test_group_labels_have_the_states_the_grouping_test_names():
    for n in (1023, 1024, 1025, 64 * 1024, 64 * 1024 + 1, 130 * 1024 + 7):
        for k in (1, 3, 4, 5, 257):
            lab = P.group_labels(n, k, seed=n + k)
            chunks = -(-n // 1024)
            assert {-1, k, P.INT32_MAX} <= set(lab.tolist())
            zero = np.flatnonzero(lab == 0) // 1024
            assert np.unique(zero).size >= chunks - 1        # state 0 in every chunk (a one-frame last chunk aside)
            if k >= 3:
                last = np.flatnonzero(lab == k - 1)
                assert last.size >= 1 and (last // 1024 == chunks - 1).all()
            if k >= 4:
                assert not (lab == 1).any()
