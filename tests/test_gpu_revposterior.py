"""Reversible posterior samples of the transition matrix (msm_sample_reversible_transition_matrices) and the
reversible=True path of compute_implied_timescales.

deeptime's BayesianMSM is absent, so parity with its stream is unpinned.  What is pinned is the law
(csrc/revposterior.hip): the invariants every sample must obey, the closed forms the law has where the reversibility
constraint is vacuous (n = 2 and tree-patterned counts: independent rows T_i. ~ Dirichlet(C_i.), no "+1"), agreement
with an independent numpy chain (tests/_revposterior_ref.py) elsewhere, burn-in adequacy, determinism, and consistency
with the reversible maximum-likelihood estimate as the counts grow."""
import functools

import numpy as np
import pytest
from scipy import stats

from tests import _revposterior_ref as ref

gpu = pytest.mark.gpu

U = 2.0 ** -53                                                # unit roundoff of f64
C2 = np.array([[12.0, 5.0], [3.0, 7.0]])
C3_TREE = np.array([[12.0, 5.0, 0.0], [3.0, 7.0, 4.0], [0.0, 6.0, 9.0]])
C3_CYCLIC = np.array([[12.0, 9.0, 1.0], [1.0, 7.0, 9.0], [9.0, 1.0, 9.0]])
C5 = np.array([[20.0, 5.0, 0.0, 2.0, 1.0], [4.0, 15.0, 3.0, 1.0, 2.0], [0.0, 2.0, 12.0, 6.0, 1.0],
               [3.0, 1.0, 5.0, 18.0, 2.0], [1.0, 3.0, 2.0, 1.0, 10.0]])      # one zero pair: (0, 2)
S_DEV, S_REF, REF_SWEEPS = 4000, 4000, 300


def _draw(engine, C, **kw):
    cd = engine.to_device(np.ascontiguousarray(C, dtype=np.float64))
    T, pi = engine.sample_reversible_transition_matrices(cd, want_pi=True, **kw)
    return T.to_host(), pi.to_host()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(T, slowest timescale) of the numpy chain: computed once, shared, read only."""
    T, _ = ref.sample({"cyclic": C3_CYCLIC, "five": C5}[name], S_REF, REF_SWEEPS, seed=17)
    ts = ref.slowest_timescale(T)
    T.setflags(write=False)
    ts.setflags(write=False)
    return T, ts


def _means_agree(Ta, tsa, Tb, tsb):
    """per-cell mean of T and mean slowest timescale of two independent sets of independent chains: 5 standard errors,
    both standard errors from the chains' own sample variances"""
    se = np.sqrt(Ta.var(0, ddof=1) / Ta.shape[0] + Tb.var(0, ddof=1) / Tb.shape[0])
    z = np.abs(Ta.mean(0) - Tb.mean(0))
    print("mean T a\n", Ta.mean(0), "\nmean T b\n", Tb.mean(0), "\n|diff| / se\n", z / np.where(se > 0, se, 1.0))
    assert np.all(z <= 5.0 * se), (z, se)
    se_t = np.sqrt(tsa.var(ddof=1) / tsa.size + tsb.var(ddof=1) / tsb.size)
    print("mean slowest timescale", tsa.mean(), tsb.mean(), "se", se_t)
    assert np.isfinite(tsa).all() and np.isfinite(tsb).all()
    assert abs(tsa.mean() - tsb.mean()) <= 5.0 * se_t


def test_numpy_reference_reproduces_the_beta_marginals():
    """The oracle itself, on the CPU: for n = 2 and tridiagonal counts T_ij ~ Beta(C_ij, c_i - C_ij), rows independent."""
    S = 4000
    for C, cells in ((C2, ((0, 1), (1, 0))), (C3_TREE, ((0, 1), (1, 0), (1, 2), (2, 1)))):
        T, pi = ref.sample(C, S, 400, seed=5)
        np.testing.assert_allclose(T.sum(-1), 1.0, rtol=1e-13)
        np.testing.assert_allclose(pi[:, :, None] * T, np.swapaxes(pi[:, :, None] * T, 1, 2), rtol=1e-12, atol=1e-300)
        for i, j in cells:
            a, b = C[i, j], C[i].sum() - C[i, j]
            p = stats.kstest(T[:, i, j], stats.beta(a, b).cdf).pvalue
            print(C.shape[0], (i, j), "KS p", p)
            assert p > 1e-4, (i, j, p)
        assert abs(np.corrcoef(T[:, 0, 1], T[:, 1, 0])[0, 1]) < 5.0 / np.sqrt(S)
    assert np.all(T[:, 0, 2] == 0.0) and np.all(T[:, 2, 0] == 0.0)


def _random_counts(n, seed):
    """dense counts with a quarter of the pairs exactly zero (both directions) and a ring that keeps them connected"""
    rng = np.random.default_rng(seed)
    C = rng.integers(0, 20, size=(n, n)).astype(np.float64)
    dead = np.triu(rng.random((n, n)) < 0.25, 1)
    C[dead | dead.T] = 0.0
    idx = np.arange(n)
    C[idx, (idx + 1) % n] += 1.0
    return C


def _nine_state():
    """the matrix of test_gpu_posterior.test_samples_match_the_numpy_restatement on its active set: a state that is only
    entered (prior-only row), alpha = 1e-3 on every cell -- and then three pairs exactly zero"""
    rng = np.random.default_rng(4)
    k = 9
    C = rng.integers(0, 60, size=(k, k))
    C[rng.random((k, k)) < 0.4] = 0
    C[3, :] = 0
    C[:, 3] = 0
    C[5, :] = 0
    active = np.array([s for s in range(k) if s != 3])
    raw = C[np.ix_(active, active)].astype(np.float64)
    A = raw + 1e-3
    for i, j in ((0, 6), (2, 7), (1, 4)):
        A[i, j] = A[j, i] = 0.0
        raw[i, j] = raw[j, i] = 0.0
    prior_only = (raw + raw.T == 0.0) & (A + A.T > 0.0)
    assert prior_only.any() and np.all(raw[4] == 0.0)               # packed index 4 = state 5
    return A, prior_only


_SHAPES = [("n1", lambda: np.array([[5.0]]), {"n_samples": 8}),
           ("n2", lambda: C2, {"n_samples": 8}),
           ("n3", lambda: C3_CYCLIC, {"n_samples": 8}),
           ("n7", lambda: _random_counts(7, 1), {"n_samples": 8}),
           ("n130", lambda: _random_counts(130, 2), {"n_samples": 4}),
           ("n600", lambda: _random_counts(600, 3), {"n_samples": 4, "n_sweeps": 3}),
           ("nine_state", lambda: _nine_state()[0], {"n_samples": 24})]


@gpu
@pytest.mark.parametrize("name,make,kw", _SHAPES, ids=[s[0] for s in _SHAPES])
def test_every_sample_obeys_the_invariants(engine, name, make, kw):
    C = make()
    n = C.shape[0]
    T, pi = _draw(engine, C, seed=21, **kw)
    assert T.shape == (kw["n_samples"], n, n) and pi.shape == (kw["n_samples"], n)
    assert np.isfinite(T).all() and np.all(T >= 0.0) and np.isfinite(pi).all() and np.all(pi > 0.0)
    np.testing.assert_allclose(T.sum(-1), 1.0, rtol=1e-14)
    pinned = (C + C.T) == 0.0
    assert np.all(T[:, pinned] == 0.0)
    assert np.all(T[:, ~pinned] > 0.0)
    # Detailed balance.  The kernel stores T_ij = fl(x_ij / x_i) and pi_i = fl(x_i / sum) from ONE symmetric x_ij and ONE
    # x_i; the flux formed here, fl(pi_i T_ij), carries three roundings: x_ij / sum * (1 + d1)(1 + d2)(1 + d3), |d| <= u.
    # Two such fluxes of the same x_ij differ by at most ((1 + u)^3 - (1 - u)^3) x_ij / sum ~ 6 u x_ij / sum, and
    # 6 u / (1 - 3 u) = 6.7e-16 < 1e-15 relative to the larger of the two.
    F = pi[:, :, None] * T
    bound = 1e-15 * np.maximum(np.maximum(F, np.swapaxes(F, 1, 2)), np.finfo(np.float64).tiny)
    assert np.all(np.abs(F - np.swapaxes(F, 1, 2)) <= bound)
    # pi T = pi: column j of F sums x_ij / sum over i to x_j / sum; x_j is itself an n-term sum (<= n u), every flux
    # carries 3 u and numpy's column sum at most another n u
    np.testing.assert_allclose(F.sum(1), pi, rtol=(2 * n + 6) * U)
    np.testing.assert_allclose(pi.sum(-1), 1.0, rtol=(n + 2) * U)
    if name == "nine_state":
        prior_only = _nine_state()[1]
        for i, j in zip(*np.nonzero(prior_only)):                   # a prior-only cell moves: it is not stuck
            assert np.unique(T[:, i, j]).size > 1, (i, j)


@gpu
def test_closed_forms_where_reversibility_is_vacuous(engine):
    S = 6000
    for C, cells in ((C2, ((0, 1), (1, 0))), (C3_TREE, ((0, 1), (1, 0), (1, 2), (2, 1)))):
        T, _ = _draw(engine, C, seed=31, n_samples=S)
        for i, j in cells:
            a, b = C[i, j], C[i].sum() - C[i, j]                    # Dirichlet(C_i.) marginal: Beta(C_ij, c_i - C_ij)
            p = stats.kstest(T[:, i, j], stats.beta(a, b).cdf).pvalue
            mean, var = a / (a + b), a * b / ((a + b) ** 2 * (a + b + 1.0))
            print(C.shape[0], (i, j), "KS p", p, "mean", T[:, i, j].mean(), "want", mean, "5 se", 5.0 * np.sqrt(var / S))
            assert p > 1e-4, (i, j, p)
            assert abs(T[:, i, j].mean() - mean) < 5.0 * np.sqrt(var / S)
        r = np.corrcoef(T[:, 0, 1], T[:, 1, 0])[0, 1]
        print("cross-row correlation", r)
        assert abs(r) < 5.0 / np.sqrt(S)


@gpu
@pytest.mark.parametrize("name", ["cyclic", "five"])
def test_general_case_matches_the_numpy_chain(engine, name):
    C = {"cyclic": C3_CYCLIC, "five": C5}[name]
    Td, _ = _draw(engine, C, seed=41, n_samples=S_DEV)
    Tr, tsr = _reference(name)
    _means_agree(Td, ref.slowest_timescale(Td), Tr, tsr)
    if name == "cyclic":
        # not the old sampler: independent Dirichlet rows put T_02 at C_02 / c_0 = 1 / 22
        se = np.sqrt(Td[:, 0, 2].var(ddof=1) / S_DEV)
        print("mean T_02", Td[:, 0, 2].mean(), "Dirichlet rows", 1.0 / 22.0, "se", se)
        assert abs(Td[:, 0, 2].mean() - 1.0 / 22.0) > 10.0 * se


@gpu
@pytest.mark.parametrize("name", ["cyclic", "five"])
def test_default_burn_in_is_enough(engine, name):
    C = {"cyclic": C3_CYCLIC, "five": C5}[name]
    default = 2 * int(np.ceil(np.sqrt(C.shape[0]))) + 10
    Ta, _ = _draw(engine, C, seed=51, n_samples=S_DEV)                        # n_sweeps=None: the default
    Tb, _ = _draw(engine, C, seed=52, n_samples=S_DEV, n_sweeps=4 * default)
    Tc, _ = _draw(engine, C, seed=51, n_samples=8, n_sweeps=default)
    np.testing.assert_array_equal(Ta[:8], Tc)                                 # None means 2 ceil(sqrt n) + 10
    _means_agree(Ta, ref.slowest_timescale(Ta), Tb, ref.slowest_timescale(Tb))


@gpu
@pytest.mark.parametrize("n", [7, 130])
def test_samples_are_deterministic_and_do_not_depend_on_the_batch(engine, n):
    C = _random_counts(n, 6)
    whole, pw = _draw(engine, C, seed=3, n_samples=6)
    again, pa = _draw(engine, C, seed=3, n_samples=6)
    np.testing.assert_array_equal(whole, again)
    np.testing.assert_array_equal(pw, pa)
    tail, pt = _draw(engine, C, seed=3, n_samples=2, first_sample=4)
    np.testing.assert_array_equal(whole[4:], tail)
    np.testing.assert_array_equal(pw[4:], pt)
    other, _ = _draw(engine, C, seed=4, n_samples=1)
    assert np.abs(other[0] - whole[0]).max() > 1e-3
    assert np.abs(whole[0] - whole[1]).max() > 1e-3


@gpu
def test_posterior_mean_approaches_the_reversible_mle(engine):
    dist, last = [], None
    for scale in (1.0, 10.0, 100.0):
        C = scale * C3_CYCLIC
        T, _ = _draw(engine, C, seed=61, n_samples=S_DEV)
        mle = engine.reversible_mle(engine.to_device(np.ascontiguousarray(C)))["T"].to_host()
        dist.append(np.abs(T.mean(0) - mle).max())
        last = (T, mle, C)
    print("max |mean T - MLE| at x1, x10, x100:", dist)
    assert dist[0] > dist[1] > dist[2]
    T, mle, C = last
    se = np.sqrt(T.var(0, ddof=1) / S_DEV)
    # O(1/c) term: a cell of row i behaves like a Beta(a, b) with a + b = c_i, whose mean a / (a + b) and mode
    # (a - 1) / (a + b - 2) differ by |b - a| / ((a + b)(a + b - 2)) <= 1 / (c_i - 2); the point estimate is a mode, the
    # posterior mean is a mean
    bias = 1.0 / (C.sum(1) - 2.0)
    print("|mean T - MLE|\n", np.abs(T.mean(0) - mle), "\n5 se\n", 5.0 * se, "\nbias term", bias)
    assert np.all(np.abs(T.mean(0) - mle) <= 5.0 * se + bias[:, None])


def _chain(P, n, seed):
    rng = np.random.default_rng(seed)
    cdf = np.cumsum(P, axis=1)
    u = rng.random(n)
    x = np.zeros(n, dtype=np.int64)
    for t in range(1, n):
        x[t] = min(P.shape[0] - 1, int(np.searchsorted(cdf[x[t - 1]], u[t])))
    return x


@gpu
def test_reversible_its_end_to_end(engine):
    from pmarlo_amd.markov_state_model import compute_implied_timescales
    from pmarlo_amd.markov_state_model.estimation import ensure_connected_counts

    two = _chain(np.array([[0.9, 0.1], [0.2, 0.8]]), 30_000, 0)
    lags = [1, 2, 3]
    res = compute_implied_timescales([two], 2, lag_times=lags, n_timescales=1, n_samples=1000, ci=0.99, random_state=7,
                                     reversible=True, return_samples=True)
    t_true = -1.0 / np.log(0.7)
    lo, hi = res.timescales_ci[:, 0, 0], res.timescales_ci[:, 0, 1]
    print("two-state band", lo, hi, "median", res.timescales[:, 0], "analytic", t_true)
    assert np.isfinite(res.timescales).all() and np.isfinite(res.timescales_ci).all()
    assert np.all(lo < res.timescales[:, 0]) and np.all(res.timescales[:, 0] < hi)
    # The band contains the analytic timescale at lag 1.  Whether it does is a property of the trajectory as much as of
    # the sampler: this realisation's estimate lies two posterior standard deviations below the truth (the closed form
    # below says so without the device), hence the 99 % band; at lags 2 and 3 sliding-window counts overstate the
    # sample size, the nominal band is too narrow by construction, and only the law is checked.
    assert lo[0] < t_true < hi[0]
    # n = 2: the law is closed-form, lambda_2 = 1 - T_01 - T_10 with independent Beta rows on the regularised counts.
    # A 0.5 % quantile from 1000 draws has a standard error of sqrt(p (1 - p) / S) / density ~ 0.15 posterior standard
    # deviations ~ 0.3 % of the timescale: 2 % is more than five of them.
    for q, lag in enumerate(lags):
        C = np.zeros((2, 2))
        np.add.at(C, (two[:-lag], two[lag:]), 1.0)
        a = C + 1e-3
        draws = 1.0 - stats.beta(a[0, 1], a[0, 0]).rvs(200_000, random_state=1) - stats.beta(a[1, 0], a[1, 1]).rvs(
            200_000, random_state=2)
        want = np.percentile(-lag / np.log(draws), [0.5, 50.0, 99.5])
        print("lag", lag, "closed form", want, "device", lo[q], res.timescales[q, 0], hi[q])
        np.testing.assert_allclose([lo[q], res.timescales[q, 0], hi[q]], want, rtol=0.02)
    det = compute_implied_timescales([two], 2, lag_times=lags, n_timescales=1, n_samples=0, reversible=True)
    assert np.all(np.abs(res.timescales - det.timescales) / det.timescales < 0.03)

    cyc = _chain(np.array([[0.5, 0.4, 0.1], [0.1, 0.5, 0.4], [0.4, 0.1, 0.5]]), 30_000, 1)
    kw = dict(lag_times=[1], n_timescales=2, n_samples=200, random_state=9, return_samples=True)
    rev = compute_implied_timescales([cyc], 3, reversible=True, **kw)
    ev = rev.samples["eigenvalues"][0]                                          # [S, 2]
    assert np.isfinite(ev).all() and np.all(ev > 0.0) and np.all(ev < 1.0) and np.all(ev[:, 0] >= ev[:, 1])
    # the very matrices behind those spectra: real eigenvalues, the same numbers
    C = np.zeros((3, 3))
    np.add.at(C, (cyc[:-1], cyc[1:]), 1.0)
    T, _ = _draw(engine, ensure_connected_counts(C, alpha=1e-3).counts, seed=9, n_samples=200, first_sample=0)
    lam = np.linalg.eigvals(T)
    assert np.abs(lam.imag).max() < 1e-12
    np.testing.assert_allclose(np.sort(lam.real, axis=1)[:, ::-1][:, 1:], ev, rtol=1e-6)
    off = compute_implied_timescales([cyc], 3, reversible=False, **kw)
    omitted = compute_implied_timescales([cyc], 3, **kw)
    for name in ("eigenvalues", "eigenvalues_ci", "timescales", "timescales_ci", "rates", "rates_ci"):
        np.testing.assert_array_equal(getattr(off, name), getattr(omitted, name))
    np.testing.assert_array_equal(off.samples["timescales"], omitted.samples["timescales"])
    print("cyclic medians: reversible", rev.timescales, "non-reversible", off.timescales)
    assert np.isfinite(rev.timescales).all() and not np.allclose(rev.timescales, off.timescales, rtol=1e-6)
