"""msm_silhouette_samples: any cluster count, frame order, the same bytes for every launch cut.

The reference is the numpy restatement in the difference form (tests/_silhouette_ref.py); tolerance of the per-sample
values: atol 1e-10.  A cluster sum has at most n fp64 terms that each carry a few ulp of a distance, so a_i and b_i
are good to about n * 2e-16 relative (2e-12 at n = 5000, 4e-12 at n = 16500) and s_i, a ratio of them in [-1, 1], to
the same absolute size; 1e-10 leaves a factor of 25 and more."""

from __future__ import annotations

import functools
import time

import numpy as np
import pytest

from pmarlo_amd import _lib
from tests import _gen
from tests._silhouette_ref import recipe_labels, silhouette_samples_ref

pytestmark = pytest.mark.gpu

L = _lib.SIL_SEG_LEN
ATOL = 1e-10


@functools.lru_cache(maxsize=None)
def _recipe_case(n, d, k):
    X, _ = _gen.gaussian_clusters(k, n // k + 1, d, seed=k)
    X = np.ascontiguousarray(X[:n], np.float64)
    labels = recipe_labels(n, k)
    ref = silhouette_samples_ref(X, labels, k)
    for a in (X, labels, ref):
        a.setflags(write=False)
    return X, labels, ref


def _run(engine, X, labels, k, **kw):
    score, samples = engine.silhouette_samples(engine.to_device(X), engine.to_device(labels.astype(np.int32)), k, **kw)
    return score, samples.to_host()


def _report(name, got, ref):
    print(f"{name}: max |s - ref| = {np.abs(got - ref).max():.3e}, mean {got.mean():.15f} vs {ref.mean():.15f}")


@pytest.mark.parametrize("n,d,k", [(1500, 3, 33), (2000, 10, 200), (700, 256, 40)])
def test_many_clusters(engine, n, d, k):
    """More than 32 clusters, a singleton, a pair, an id without members, d up to 256; values in frame order."""
    from sklearn.metrics import silhouette_score as sk_score

    from pmarlo_amd.markov_state_model.clustering import silhouette_samples, silhouette_score

    X, labels, ref = _recipe_case(n, d, k)
    score, got = _run(engine, X, labels, k)            # ids as they are: k - 5 has no member
    _report(f"engine ({n}, {d}, {k})", got, ref)
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)
    assert got[0] == 0.0                                # the singleton
    want = sk_score(X, labels)
    np.testing.assert_allclose(score, want, rtol=1e-10, atol=1e-12)
    # the public functions take any integer labels and densify them
    shifted = labels * 7 - 11
    pub = silhouette_samples(X, shifted)
    np.testing.assert_allclose(pub, ref, rtol=0, atol=ATOL)
    np.testing.assert_allclose(silhouette_score(X, shifted), want, rtol=1e-10, atol=1e-12)


def test_near_points_far_from_the_origin(engine):
    """Clusters 3e-3 apart at 1e3 from the origin: x.x - 2 x.y + y.y under the root loses the distances (sklearn is off
    by 4e-5 per sample here), the difference form does not.  Frames 0 and 1 are the same point."""
    n, k = 600, 5
    rng = np.random.default_rng(5)
    labels = np.arange(n) % k
    X = 1e3 + labels[:, None] * np.array([3e-3, 0.0, 0.0]) + rng.normal(scale=1e-3, size=(n, 3))
    X[1] = X[0]
    ref = silhouette_samples_ref(X, labels, k)
    _, got = _run(engine, X, labels, k)
    _report("ill-conditioned", got, ref)
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)


@functools.lru_cache(maxsize=None)
def _boundary_case(case):
    if case == 0:
        X, labels, ref = _recipe_case(4097, 45, 7)
        return "recipe", X, labels, 7, ref
    # clusters of exactly L, L + 1 and 2 L - 1 members (one segment; a segment and one row; two segments, the second
    # one row short) and one of five, the frames shuffled
    sizes = [L, L + 1, 2 * L - 1, 5]
    rng = np.random.default_rng(11)
    labels = rng.permutation(np.repeat(np.arange(4), sizes))
    X = rng.normal(size=(labels.size, 3)) + 4.0 * labels[:, None]
    return "segment lengths", X, labels, 4, silhouette_samples_ref(X, labels, 4)


@pytest.mark.parametrize("case", [0, 1])
def test_launch_cut_changes_no_byte(engine, case):
    name, X, labels, k, ref = _boundary_case(case)
    n, d = X.shape
    tiles = -(-n // _lib.SIL_TILE_I)
    score0, base = _run(engine, X, labels, k)
    _report(name, base, ref)
    np.testing.assert_allclose(base, ref, rtol=0, atol=ATOL)
    score1, again = _run(engine, X, labels, k)
    assert base.tobytes() == again.tobytes() and score0 == score1
    # a full segment against a fifth of the query tiles per launch (5 launches a segment), and one workgroup per
    # launch (one launch per tile: `tiles` >= 33 launches for every cluster, however small)
    for max_products in (_lib.SIL_TILE_I * L * d * (tiles // 5), 1):
        score, got = _run(engine, X, labels, k, max_products=max_products)
        assert got.tobytes() == base.tobytes(), f"{name}: max_products = {max_products} changed the samples"
        assert score == score0


def test_segment_and_query_chunks(engine):
    """2100 clusters make more segments than one slab of partial sums holds (2048), and 16500 frames more queries
    than it holds then (16384): the fold carries its state across slabs, the queries go by in two chunks."""
    n, k = 16500, 2100
    rng = np.random.default_rng(2)
    labels = rng.permutation(np.arange(n) % k)
    X = rng.normal(size=(n, 1)) + 0.01 * labels[:, None]
    ref = silhouette_samples_ref(X, labels, k)
    score, got = _run(engine, X, labels, k)
    _report("chunks", got, ref)
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)
    np.testing.assert_allclose(score, ref.mean(), rtol=1e-10, atol=1e-12)


def test_sample_size_scores_that_subset(engine):
    from pmarlo_amd.markov_state_model.clustering import silhouette_score

    X, labels, _ = _recipe_case(1500, 3, 33)
    idx = np.random.default_rng(7).choice(X.shape[0], 300, replace=False)
    assert silhouette_score(X, labels, sample_size=300, random_state=7) == silhouette_score(X[idx], labels[idx])


def test_auto_n_states_on_every_point(engine):
    """The default call above the old 200 000 point cap: 17 candidates x 4e10 pair distances and 51 small fits.
    Time on one MI355X: not measured yet (the test prints it; DESIGN.md, n_states="auto", has the table)."""
    from pmarlo_amd.markov_state_model import cluster_microstates

    n = 200_001
    rng = np.random.default_rng(0)
    centres = np.array([[0.0, 0.0], [12.0, 0.0], [0.0, 12.0], [12.0, 12.0], [6.0, 24.0]])
    planted = np.arange(n) % 5
    X = centres[planted] + rng.normal(scale=0.4, size=(n, 2))
    t0 = time.perf_counter()
    res = cluster_microstates(X, n_states="auto")
    print(f"cluster_microstates(200001 x 2, n_states='auto'): {time.perf_counter() - t0:.2f} s, {res.rationale}")
    assert res.n_states == 5 and res.rationale.startswith("silhouette=") and "sample" not in res.rationale
    # the five states are the planted ones
    assert np.unique(res.labels * 5 + planted).size == 5


def test_errors(engine):
    X, labels, _ = _recipe_case(1500, 3, 33)
    xd, ld = engine.to_device(X), engine.to_device(labels.astype(np.int32))
    with pytest.raises(ValueError, match="msm_silhouette_samples: need 2 <= k <= n - 1"):
        engine.silhouette_samples(xd, ld, 1)
    few = engine.to_device(X[:33])
    with pytest.raises(ValueError, match="msm_silhouette_samples: need 2 <= k <= n - 1"):
        engine.silhouette_samples(few, engine.to_device(np.arange(33, dtype=np.int32)), 33)
    wide = engine.zeros((40, 257), np.float64)
    with pytest.raises(ValueError, match="msm_silhouette_samples: need 1 <= d <= 256"):
        engine.silhouette_samples(wide, engine.to_device((np.arange(40) % 3).astype(np.int32)), 3)
    with pytest.raises(ValueError, match=r"msm_silhouette_samples: \d+ of the 1500 labels lie outside \[0, 20\)"):
        engine.silhouette_samples(xd, ld, 20)
