"""The numpy restatement of the HMM contract (tests/_hmm_ref.py) against brute-force enumeration, its chunked order
against its sequential order, the exact case, and lag_observations against a plain loop.  No GPU."""
import numpy as np
import pytest

from tests import _hmm_ref as ref

LD = np.longdouble


@pytest.mark.parametrize("n,T,seed", [(1, 3, 0), (2, 1, 1), (2, 6, 2), (3, 5, 3), (3, 6, 4)])
def test_restatement_matches_enumeration(n, T, seed):
    A, B, p0 = ref.random_model(n, 3, seed, zeros=seed == 4)
    obs = ref.sample_labels(A, B, p0, T, seed)
    bf = ref.brute_force(A, B, p0, obs)
    for fb in (ref.forward_backward, ref.forward_backward_chunked):
        r = fb(A, B, p0, obs, LD)
        assert abs(r["logL"] - np.log(bf["likelihood"])) < 1e-17 * T * 10
        np.testing.assert_allclose(r["gamma"].astype(float), bf["gamma"].astype(float), rtol=1e-15, atol=1e-300)
        np.testing.assert_allclose(r["C"].astype(float), bf["C"].astype(float), rtol=1e-15, atol=1e-300)
    path, lp = ref.viterbi(A, B, p0, obs, LD)
    assert abs(lp - np.log(bf["best"])) < 1e-17 * T * 10
    assert tuple(path) == min(bf["best_paths"])               # ties to the lowest index
    assert abs(ref.path_log_probability(A, B, p0, obs, path) - lp) < 1e-17 * T * 10


def test_zero_probability_sequence_is_reported_not_nan():
    A, B, p0 = ref.random_model(2, 3, 0)
    B[:, 2] = 0.0
    for fb in (ref.forward_backward, ref.forward_backward_chunked):
        r = fb(A, B, p0, np.array([0, 1, 2, 1]), np.float64)
        assert r["dead"] and r["logL"] == -np.inf and not np.isnan(r["gamma"]).any() and not r["C"].any()
    assert ref.viterbi(A, B, p0, np.array([0, 1, 2, 1]))[0] is None


@pytest.mark.parametrize("chunk", [1, 4, ref.L])
@pytest.mark.parametrize("T", [1, 2, 5, 23, 3 * ref.L + 5])
def test_chunked_order_matches_sequential_order(T, chunk):
    n, k = 3, 5
    A, B, p0 = ref.random_model(n, k, 7, zeros=True)
    obs = ref.sample_labels(A, B, p0, T, T)
    want = ref.forward_backward(A, B, p0, obs, LD)
    got = ref.forward_backward_chunked(A, B, p0, obs, LD, chunk)
    np.testing.assert_allclose(got["gamma"].astype(float), want["gamma"].astype(float), rtol=1e-14, atol=1e-300)
    assert float(np.max(np.abs(got["gamma"] - want["gamma"]))) < 1e-15
    assert float(np.max(np.abs(got["C"] - want["C"]))) < 1e-15 * T
    assert abs(got["logL"] - want["logL"]) < 1e-15
    # the fp64 run of the chunked order sits inside the derived bounds
    f64 = ref.forward_backward_chunked(A, B, p0, obs, np.float64, chunk)
    ref.check_close(f64["gamma"], want["gamma"], ref.depth_gamma(T, n, chunk), "gamma")
    ref.check_close(f64["C"], want["C"], ref.depth_C([T], n, chunk), "C")
    assert abs(f64["logL"] - want["logL"]) <= ref.bound_logL(T, n, want["S"], chunk)


def test_rescaling_keeps_tiny_emissions_finite():
    n, k, T = 2, 3, 3 * ref.L
    A, B, p0 = ref.random_model(n, k, 1)
    B = B * 1e-3                                  # every emission <= 1e-3: the plain product underflows to 0 by T = 110
    obs = ref.sample_labels(A, B, p0, T, 3)
    r = ref.forward_backward_chunked(A, B, p0, obs, np.float64)
    want = ref.forward_backward(A, B, p0, obs, LD)
    assert np.isfinite(r["logL"]) and r["logL"] < -3 * T
    ref.check_close(r["gamma"], want["gamma"], ref.depth_gamma(T, n), "gamma")


def exact_case(T=200, n=3, k=7, seed=0):
    """Every symbol is emitted by exactly one hidden state: B has one non-zero per column."""
    rng = np.random.default_rng(seed)
    owner = np.arange(k) % n
    A, _, p0 = ref.random_model(n, k, seed)
    B = np.zeros((n, k))
    B[owner, np.arange(k)] = rng.random(k) + 0.1
    B /= B.sum(axis=1, keepdims=True)
    labels = ref.sample_labels(A, B, p0, T, seed)
    return A, B, p0, labels, owner


@pytest.mark.parametrize("lag", [1, 3])
def test_exact_case_counts_transitions(lag):
    A, B, p0, labels, owner = exact_case()
    labels = labels.copy()
    labels[77] = -1                               # a split
    k, n = B.shape[1], A.shape[0]
    lab, table = ref.lag_observations_loop([labels], lag, k)
    lumped = np.where(lab >= 0, owner[np.clip(lab, 0, k - 1)], -1)
    counts = np.zeros((n, n))
    for t in range(len(lab) - lag):
        if (lab[t:t + lag + 1] >= 0).all():
            counts[lumped[t], lumped[t + lag]] += 1
    for chunked in (False, True):
        e = ref.estep(A, B, p0, lab, table, k, np.float64, chunked=chunked)
        hot = np.zeros((len(lab), n))
        hot[np.flatnonzero(lab >= 0), lumped[lab >= 0]] = 1.0
        if chunked:                               # the device's order: exact, bit for bit
            assert np.array_equal(e["gamma"], hot)
            assert np.array_equal(e["C"], counts)
            (A1, _, _, _), _, _ = ref.em_step(A, B, p0, lab, table, k, np.float64)
        else:
            np.testing.assert_allclose(e["gamma"], hot, atol=1e-13)
            np.testing.assert_allclose(e["C"], counts, rtol=1e-13)
    e = ref.estep(A, B, p0, lab, table, k, np.float64, chunked=True)
    A1 = ref.mstep(e["C"], e["E"], e["gamma0"], len(table), np.float64, reversible=False)[0]
    assert np.array_equal(A1, counts / counts.sum(axis=1, keepdims=True))


def test_lag_observations_against_a_plain_loop():
    from pmarlo_amd.markov_state_model.hmm import lag_observations

    rng = np.random.default_rng(0)
    k = 4
    dtrajs = [rng.integers(0, k, 37), rng.integers(0, k, 2), rng.integers(0, k, 11), np.array([], np.int64)]
    dtrajs[0][[5, 6, 20]] = -1                    # split by -1 (twice in a row, and once)
    dtrajs[2][0] = k                              # an out-of-range label at the very start
    for lag in (1, 3, 5, 50):
        labels, table = lag_observations(dtrajs, lag, k)
        want_labels, want_table = ref.lag_observations_loop(dtrajs, lag, k)
        assert np.array_equal(labels, want_labels) and np.array_equal(table, want_table)
        covered = np.concatenate([r[0] + r[1] * np.arange(r[2]) for r in table])
        assert np.array_equal(np.sort(covered), np.flatnonzero((labels >= 0) & (labels < k)))   # each valid frame once
