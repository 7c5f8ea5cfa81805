"""The numpy / Python-int restatement of the effective-count contract (tests/_effective_ref.py) checked against itself
and against first principles, without a GPU: it is the yardstick tests/test_gpu_effective_counts.py holds the kernels
to."""

from fractions import Fraction

import numpy as np
import pytest

from tests._effective_ref import (average_counts, dense_inefficiencies, effective_reference, position_inefficiencies,
                                  regime_chain, rows_of, sliding_counts, split_valid, sticky_chain)


@pytest.mark.parametrize("seed, k, lag, lens", [(1, 3, 1, (300,)), (2, 4, 2, (150, 40, 3, 90)), (3, 5, 3, (200, 7, 120)),
                                                (4, 4, 1, (400, 250)), (5, 4, 2, (300, 2, 180))])
def test_dense_and_position_forms_agree(seed, k, lag, lens):
    rng = np.random.default_rng(seed)
    if seed >= 4:      # long autocorrelations: truncation lags well above 1
        trajs = [regime_chain(rng, n, 1.0 / 25) for n in lens]
    else:
        trajs = [sticky_chain(rng, n, k, 0.8) for n in lens]
    dense = dense_inefficiencies(trajs, k, lag)
    si, trunc, C = position_inefficiencies(trajs, k, lag)
    assert np.array_equal(C, sliding_counts(trajs, k, lag))
    assert np.array_equal(si > 0, C > 0)
    # the float loop carries the rounding of a mean-removed series of up to 300 terms per lag; away from a sign
    # flip of the autocovariance (none on these chains) the two agree far below this
    np.testing.assert_allclose(si, dense, rtol=1e-10, atol=0)
    assert trunc[C > 0].min() >= 0 and (trunc[C == 0] == 0).all()
    if seed == 4:
        assert trunc.max() >= 10


def exact_inefficiency(subseqs, j, mact=1):
    """si and truncation lag of target j over the sub-sequences, from the definition in rational arithmetic."""
    X = [[Fraction(int(v == j)) for v in s] for s in subseqs]
    flat = [v for x in X for v in x]
    N, c = len(flat), sum(flat)
    mean = c / N
    M = max(len(x) for x in X)
    corrsum, l_star = Fraction(0), M
    for l in range(M):
        acf = sum((x[p] - mean) * (x[p + l] - mean) for x in X for p in range(len(x) - l))
        n = sum(max(len(x) - l, 0) for x in X)
        acf /= n
        if acf <= 0:
            l_star = l
            break
        if l > 0:
            corrsum += acf * (1 - Fraction(l, M))
    return 1 / (1 + 2 * mact * corrsum * N / c), l_star


def test_hand_worked_sequence_in_rationals():
    # two trajectories; at lag 1 row 0 has the sub-sequences (0 0 0 1 0 0 1) and (0 1)
    trajs = [np.array([0, 0, 0, 0, 1, 0, 0, 0, 1, 1]), np.array([0, 0, 1, 1, 0])]
    k, lag = 2, 1
    rows = rows_of(trajs, k, lag)
    assert [r.tolist() for r in rows[0]] == [[0, 0, 0, 1, 0, 0, 1], [0, 1]]
    assert [r.tolist() for r in rows[1]] == [[0, 1], [1, 0]]
    si, trunc, C = position_inefficiencies(trajs, k, lag)
    assert C.tolist() == [[6, 3], [2, 2]]
    for i in range(k):
        for j in range(k):
            want, l_star = exact_inefficiency(rows[i], j)
            assert trunc[i, j] == l_star
            assert si[i, j] == pytest.approx(float(want), rel=4 * 2.0 ** -52, abs=0)
    # by hand, cell (1, 1): x = (0 1), (1 0); N = 4, c = 2, Q_0 = c N (N - c) = 16; lag 1: n = 2, S = 0, A = 0 + 1,
    # B = 1 + 0, Q_1 = 0 - 2 * 4 * 2 + 4 * 2 = -8: truncated at 1 with an empty sum
    assert trunc[1, 1] == 1 and si[1, 1] == 1.0
    # cell (0, 1): x = (0 0 0 1 0 0 1), (0 1); N = 9, c = 3; lag 1: n = 7, S = 0, A = 1 + 0, B = 2 + 1,
    # Q_1 = 0 - 3 * 9 * 4 + 9 * 7 = -45
    assert trunc[0, 1] == 1 and si[0, 1] == 1.0
    # cell (0, 0) is the complement of (0, 1) in its row: the same series up to sign, the same inefficiency
    assert trunc[0, 0] == 1 and si[0, 0] == 1.0
    # a sequence with a non-empty sum: state 0 leaves to 1 for a stretch, then to 2 for a stretch, so the targets
    # of row 0 come in runs; every cell against the rational form
    def stretch(target, times):
        return np.tile([0, target], times)

    trajs = [np.concatenate([stretch(1, 6), stretch(2, 5), stretch(1, 7), stretch(2, 4)]),
             np.concatenate([stretch(2, 5), stretch(1, 3), [0]])]
    rows = rows_of(trajs, 3, 1)
    si, trunc, C = position_inefficiencies(trajs, 3, 1)
    for i in range(3):
        for j in np.flatnonzero(C[i]):
            want, l_star = exact_inefficiency(rows[i], j)
            assert trunc[i, j] == l_star
            assert si[i, j] == pytest.approx(float(want), rel=4 * 2.0 ** -52, abs=0)
    assert trunc[0].max() > 1 and si[0, 1] < 1.0       # the sum is not empty


def test_single_target_row_has_unit_inefficiency():
    trajs = [np.array([2, 1, 1, 1, 1, 0]), np.array([1, 1, 1])]
    si, trunc, C = position_inefficiencies(trajs, 3, 1)
    assert C[2].tolist() == [0, 1, 0] and si[2, 1] == 1.0 and trunc[2, 1] == 0      # Q_0 = c N (N - c) = 0
    assert si[0].tolist() == [0.0, 0.0, 0.0]                                       # state 0 never starts a pair
    np.testing.assert_array_equal(dense_inefficiencies(trajs, 3, 1)[2], si[2])


def test_averages_satisfy_their_defining_sums():
    rng = np.random.default_rng(7)
    trajs = [sticky_chain(rng, n, 4, 0.7) for n in (120, 60)]
    si, _, C = position_inefficiencies(trajs, 4, 2)
    Cf = C.astype(float)
    none = average_counts(C, si, "none")
    row = average_counts(C, si, "row")
    whole = average_counts(C, si, "all")
    np.testing.assert_array_equal(none, Cf * si)
    np.testing.assert_allclose(row.sum(axis=1), none.sum(axis=1), rtol=1e-14)       # a row keeps its effective mass
    np.testing.assert_allclose(whole.sum(), none.sum(), rtol=1e-14)                 # and so does the whole matrix
    assert np.ptp((whole / Cf)[C > 0]) < 1e-15                                      # "all": one weight
    for i in range(4):
        assert np.ptp((row[i] / Cf[i])[C[i] > 0]) < 1e-15                           # "row": one weight per row
    assert (si[C > 0] > 0).all() and (si <= 1.0).all()


def test_invalid_labels_cut_trajectories():
    d = [np.array([0, 1, -1, 1, 0, 5, 0, 0, 1])]
    parts = split_valid(d, 2)
    assert [p.tolist() for p in parts] == [[0, 1], [1, 0], [0, 0, 1]]
    ceff, si, C, _ = effective_reference(d, 2, 1)
    assert C.tolist() == [[1, 2], [1, 0]]
    assert ceff.shape == (2, 2) and (ceff <= C).all()
