"""Host side of pmarlo_amd.conformations.KineticImportanceScore: the k_slow selection rules, KISResult, the argument
errors and the resampling order.  Nothing here touches the device."""
import numpy as np
import pytest

from pmarlo_amd.conformations import KineticImportanceScore, KISResult
from pmarlo_amd.conformations.kinetic_importance import _draw_multiplicities


def _kis(n):
    return KineticImportanceScore(np.eye(n), np.full(n, 1.0 / n))


@pytest.mark.parametrize("n,want", [(3, 2), (19, 2), (20, 2), (30, 3), (49, 4), (50, 5), (500, 5)])
def test_default_rule(n, want):
    kis = _kis(n)
    assert kis.select_k_slow() == want == min(5, max(2, n // 10))
    assert kis.select_k_slow(None, method="timescale_gap") == want
    assert isinstance(kis.select_k_slow(), int)


def test_timescale_gap_rule():
    kis = _kis(50)
    # the largest ratio its[i] / its[i + 1] is at i = 2 and reaches the threshold: k_slow = i + 1
    assert kis.select_k_slow(np.array([900.0, 700.0, 500.0, 40.0, 30.0, 20.0])) == 3
    assert kis.select_k_slow(np.array([900.0, 700.0, 500.0, 300.0, 30.0, 20.0])) == 4
    # a gap at index 0 gives 1, lifted to the floor of 2
    assert kis.select_k_slow(np.array([900.0, 9.0, 8.0, 7.0])) == 2
    # no ratio reaches the threshold: min(5, len)
    assert kis.select_k_slow(np.array([90.0, 80.0, 70.0, 60.0, 50.0, 45.0, 40.0])) == 5
    assert kis.select_k_slow(np.array([90.0, 80.0, 70.0])) == 3
    assert kis.select_k_slow(np.array([90.0, 80.0])) == 2
    # the threshold is a parameter; exactly at it counts as a gap
    assert kis.select_k_slow(np.array([90.0, 80.0, 60.0, 55.0]), gap_threshold=4.0 / 3.0) == 2
    assert kis.select_k_slow(np.array([90.0, 80.0, 70.0, 35.0, 30.0]), gap_threshold=2.0) == 3
    # fewer than two timescales: 2; a zero timescale is floored at 1e-10 in the ratio
    assert kis.select_k_slow(np.array([5.0])) == 2
    assert kis.select_k_slow(np.array([9.0, 8.0, 7.0, 0.0])) == 3


def test_variance_rule_on_the_host():
    # eigenvalues 1, 0.9, 0.8 (squares 1, 0.81, 0.64: cumulative 0.408, 0.739, 1): the threshold 0.9 needs all three,
    # capped at n_states - 1
    T = np.array([[0.9, 0.1, 0.0], [0.05, 0.9, 0.05], [0.0, 0.1, 0.9]])
    kis = KineticImportanceScore(T, np.array([0.25, 0.5, 0.25]))
    assert kis.select_k_slow(method="variance") == 2
    # one dominant eigenvalue: one mode reaches the threshold, lifted to the floor of 2
    kis = KineticImportanceScore(np.full((6, 6), 1.0 / 6.0), np.full(6, 1.0 / 6.0))
    assert kis.select_k_slow(method="variance") == 2
    T = np.diag([1.0, 0.99, 0.98, 0.97, 0.1, 0.1, 0.1, 0.1])
    assert KineticImportanceScore(T, np.full(8, 0.125)).select_k_slow(method="variance") == 4


def test_result_to_dict():
    r = KISResult(kis_scores=np.array([0.25, 0.5]), k_slow=np.int64(1), eigenvectors=np.array([[0.6, 0.8], [0.8, -0.6]]),
                  eigenvalues=np.array([1.0, 0.5]), ranked_states=np.array([1, 0]))
    d = r.to_dict()
    assert list(d) == ["kis_scores", "k_slow", "eigenvectors", "eigenvalues", "ranked_states", "stability_metric",
                       "bootstrap_std"]
    assert d["kis_scores"] == [0.25, 0.5] and d["eigenvectors"] == [[0.6, 0.8], [0.8, -0.6]]
    assert d["k_slow"] == 1 and type(d["k_slow"]) is int
    assert d["ranked_states"] == [1, 0] and d["eigenvalues"] == [1.0, 0.5]
    assert d["stability_metric"] is None and d["bootstrap_std"] is None
    full = KISResult(r.kis_scores, 1, r.eigenvectors, r.eigenvalues, r.ranked_states, stability_metric=np.float32(0.5),
                     bootstrap_std=np.array([0.125, 0.25])).to_dict()
    assert full["stability_metric"] == 0.5 and type(full["stability_metric"]) is float
    assert full["bootstrap_std"] == [0.125, 0.25]


def test_constructor_errors():
    with pytest.raises(ValueError, match="square"):
        KineticImportanceScore(np.zeros((3, 4)), np.zeros(3))
    with pytest.raises(ValueError, match="length must match"):
        KineticImportanceScore(np.eye(3), np.zeros(4))
    kis = KineticImportanceScore([[0.5, 0.5], [0.5, 0.5]], [0.5, 0.5])       # lists are taken
    assert kis.n_states == 2 and kis.T.dtype == np.float64 and kis.pi.dtype == np.float64


@pytest.mark.parametrize("n,k_slow", [(5, 0), (5, -1), (5, 5), (5, 6), (2, 2)])
def test_k_slow_range(n, k_slow):
    with pytest.raises(ValueError, match=f"between 1 and n_states-1 \\({n - 1}\\)"):
        _kis(n).compute(k_slow=k_slow)


def test_k_slow_beyond_the_solver_subspace():
    with pytest.raises(ValueError, match="at most 31"):
        _kis(40).compute(k_slow=32)
    with pytest.raises(ValueError, match="at most 32 eigenvectors"):
        KineticImportanceScore._compute_eigenvectors_for(np.eye(40), 33)


def test_draw_order():
    """n_traj scalar integers(0, n_traj) draws per sample, sample by sample, from default_rng(seed)."""
    n_traj, n_boot, seed = 5, 3, 17
    got = _draw_multiplicities(np.random.default_rng(seed), n_traj, n_boot)
    rng = np.random.default_rng(seed)
    want = np.zeros((n_boot, n_traj), np.int32)
    i00, i01, i02, i03, i04 = (rng.integers(0, 5) for _ in range(5))
    i10, i11, i12, i13, i14 = (rng.integers(0, 5) for _ in range(5))
    i20, i21, i22, i23, i24 = (rng.integers(0, 5) for _ in range(5))
    for b, row in enumerate(((i00, i01, i02, i03, i04), (i10, i11, i12, i13, i14), (i20, i21, i22, i23, i24))):
        for i in row:
            want[b, i] += 1
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.all(got.sum(axis=1) == n_traj)
    assert _draw_multiplicities(np.random.default_rng(seed), n_traj, 0).shape == (0, n_traj)
