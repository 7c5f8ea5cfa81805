"""The numpy restatement the GPU silhouette tests compare against (tests/_silhouette_ref.py), checked on the CPU."""

from __future__ import annotations

import numpy as np
import pytest

from tests import _gen
from tests._silhouette_ref import recipe_labels, silhouette_samples_ref


def test_restatement_matches_sklearn():
    from sklearn.metrics import silhouette_samples, silhouette_score

    n, d, k = 500, 2, 4
    rng = np.random.default_rng(n + k)
    X, _ = _gen.gaussian_clusters(k, n // k + 1, d, seed=k)
    X = X[:n]
    labels = rng.integers(0, k, n)
    labels[:k] = np.arange(k)
    labels[labels == k - 1] = k - 2
    labels[0] = k - 1
    got = silhouette_samples_ref(X, labels, k)
    # sklearn expands |x - y|^2; on this well-conditioned input that costs a few ulp of the distances
    np.testing.assert_allclose(got, silhouette_samples(X, labels), rtol=0, atol=1e-12)
    np.testing.assert_allclose(got.mean(), silhouette_score(X, labels), rtol=1e-10, atol=1e-12)
    # the chunking changes nothing
    np.testing.assert_array_equal(got, silhouette_samples_ref(X, labels, k, chunk=77))


def test_recipe_has_a_singleton_a_pair_and_an_unused_id():
    for n, k in ((1500, 33), (2000, 200), (700, 40)):
        counts = np.bincount(recipe_labels(n, k), minlength=k)
        assert counts[k - 1] == 1 and counts[k - 3] == 2 and counts[k - 5] == 0
        assert np.count_nonzero(counts == 0) == 1


def test_singleton_and_unused_id_rules():
    X = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 2.0], [5.0, 5.0], [6.0, 5.0], [9.0, 9.0]])
    labels = np.array([0, 0, 0, 2, 2, 4])           # ids 1 and 3 have no member, id 4 is a singleton
    s = silhouette_samples_ref(X, labels, 5)
    assert s[5] == 0.0
    # frame 3 by hand: a = |x3 - x4| = 1, b = min(mean distance to cluster 0, distance to frame 5)
    a = 1.0
    b = min(np.mean([np.hypot(5, 5), np.hypot(4, 5), np.hypot(5, 3)]), np.hypot(4, 4))
    assert s[3] == pytest.approx((b - a) / max(a, b), rel=1e-15)
    # the unused ids change nothing: the same values under dense ids
    np.testing.assert_array_equal(s, silhouette_samples_ref(X, np.array([0, 0, 0, 1, 1, 2]), 3))


def test_all_coincident_points_score_zero():
    X = np.full((6, 3), 2.5)
    s = silhouette_samples_ref(X, np.array([0, 0, 1, 1, 1, 2]), 3)
    np.testing.assert_array_equal(s, np.zeros(6))


def test_restatement_keeps_nan():
    """One NaN coordinate: its cluster does not vanish from the other frames' b_i, and the frame itself is not 0."""
    rng = np.random.default_rng(1)
    labels = np.repeat([0, 1, 2], [30, 30, 30])
    X = rng.normal(size=(90, 2)) + 4.0 * labels[:, None]
    X[40, 0] = np.nan
    s = silhouette_samples_ref(X, labels, 3)
    assert np.isnan(s).all() and np.isnan(s.mean())


def test_auto_n_states_refuses_a_non_finite_score(monkeypatch):
    """_auto_select_n_states raises where the reference raises through sklearn's input check: a candidate whose
    silhouette score is not finite names the non-finite features.  The device is stood in for by a stub engine."""
    from pmarlo_amd.markov_state_model import clustering

    class _Arr:
        dtype = np.dtype(np.float64)

        def __init__(self, a):
            self.a = a

        def to_host(self):
            return self.a

    class _Engine:
        def to_device(self, a):
            return _Arr(np.asarray(a))

        def state_counts(self, lab, k):
            return _Arr(np.full(k, 5))

        def silhouette_samples(self, y, lab, k):
            return (0.5 if k < 6 else float("nan")), None

    monkeypatch.setattr(clustering, "get_engine", lambda: _Engine())
    monkeypatch.setattr(clustering, "MSMPipeline", lambda eng: None)
    monkeypatch.setattr(clustering, "_fit_once", lambda *a, **kw: (None, None, 1.0))
    Y = np.zeros((100, 2))
    Y[3, 1] = np.nan
    with pytest.raises(ValueError, match=r"k = 6 candidate is nan.*non-finite"):
        clustering._auto_select_n_states(Y, 0, sample_size=None, override_n_states=None, kwargs={})
