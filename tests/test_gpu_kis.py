"""Kinetic importance scores on the GPU (msm_kis_scores and pmarlo_amd.conformations.KineticImportanceScore) against
the numpy restatement in tests/_kis_ref.py.

Tolerances are computed from the reference's own quantities (R.score_bound): both sides solve the same matrix, the
device's Ritz pairs have residuals of at most 1e-9, so an eigenvector is off by at most 1e-9 / gap in the pi-weighted
norm, sqrt(max pi / min pi) times that in the 2-norm, and a score by pi_max * k_slow * 2 * that; a factor 10 covers the
constants.  Every test first asserts on the reference that the gap it divides by is there.

Realised on the MI355X (every test prints its figures): compute within 5.2e-15 on the scores and 2.8e-14 on the
eigenvectors (bounds 1.4e-7 .. 5.2e-7 and 1.4e-7 .. 1.6e-6); bootstrap scores within 1.3e-13 and bootstrap_std within
9.2e-15 (bounds 7e-7 .. 1.1e-5); subspace overlaps within 4.4e-16 (bounds 1.6e-6 and 3.2e-6)."""
import functools

import numpy as np
import pytest

from oracle import npport
from pmarlo_amd.conformations import KineticImportanceScore
from tests import _kis_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-9                      # the spectrum solver's residual bound


def _up_to_sign(got, want):
    return got * np.sign(np.sum(got * want, axis=1))[:, None]


def _check_compute(T, pi, k_slow, label):
    gap = R.modulus_gap(T, k_slow + 2)
    assert gap >= 0.01, gap                                    # otherwise the sum of squares is not well defined
    want, w_ref, v_ref = R.kis_scores(T, pi, k_slow)
    bound, dv = R.score_bound(TOL, gap, pi, k_slow)
    res = KineticImportanceScore(T, pi).compute(k_slow=k_slow)
    err = float(np.max(np.abs(res.kis_scores - want)))
    v_err = float(np.max(np.abs(_up_to_sign(res.eigenvectors, v_ref) - v_ref)))
    print(f"{label} k_slow={k_slow}: score error {err:.3e} (bound {bound:.3e}), vector error {v_err:.3e} (bound {dv:.3e})")
    assert res.k_slow == k_slow and res.eigenvectors.shape == (k_slow + 1, len(pi))
    assert err <= bound and v_err <= dv
    np.testing.assert_allclose(res.eigenvalues, w_ref, rtol=0, atol=dv)
    assert np.all(np.diff(np.abs(res.eigenvalues)) <= 0)
    np.testing.assert_allclose(np.linalg.norm(res.eigenvectors, axis=1), 1.0, rtol=1e-12)
    assert np.array_equal(res.ranked_states, np.argsort(res.kis_scores)[::-1])
    s = np.sort(want)
    if np.min(np.diff(s)) > 2 * bound:                         # the ranking is decided beyond the error
        assert np.array_equal(res.ranked_states, np.argsort(want)[::-1])
    return res


# ---- compute -------------------------------------------------------------------------------------------------------
BIRTH_DEATH = np.array([[0.9, 0.1, 0.0], [0.05, 0.9, 0.05], [0.0, 0.1, 0.9]])
BIRTH_DEATH_PI = np.array([0.25, 0.5, 0.25])


@pytest.mark.parametrize("k_slow", [1, 2])
def test_compute_birth_death(k_slow):
    """Eigenvalues 1, 0.9, 0.8 with left eigenvectors pi, (1, 0, -1) / sqrt 2 and (1, -2, 1) / sqrt 6."""
    res = _check_compute(BIRTH_DEATH, BIRTH_DEATH_PI, k_slow, "birth-death")
    exact_vecs = np.array([[1.0, 2.0, 1.0] / np.sqrt(6.0), [1.0, 0.0, -1.0] / np.sqrt(2.0), [1.0, -2.0, 1.0] / np.sqrt(6.0)])
    exact = BIRTH_DEATH_PI * np.sum(exact_vecs[1:k_slow + 1] ** 2, axis=0)
    bound, dv = R.score_bound(TOL, 0.1, BIRTH_DEATH_PI, k_slow)
    np.testing.assert_allclose(res.kis_scores, exact, rtol=0, atol=bound)
    np.testing.assert_allclose(res.eigenvalues, [1.0, 0.9, 0.8][:k_slow + 1], rtol=0, atol=dv)
    np.testing.assert_allclose(_up_to_sign(res.eigenvectors, exact_vecs[:k_slow + 1]), exact_vecs[:k_slow + 1], rtol=0, atol=dv)


@pytest.mark.parametrize("k_slow", [1, 2, 3])
def test_compute_three_blocks(k_slow):
    T, pi = R.reversible_block_chain(9, 3, seed=4)
    np.testing.assert_allclose(pi[:, None] * T, (pi[:, None] * T).T, rtol=1e-13)
    _check_compute(T, pi, k_slow, "three blocks")


def test_compute_auto_and_a_larger_chain():
    """40 states: the spectrum iterates (subspace smaller than the matrix) and k_slow comes from the default rule."""
    T, pi = R.reversible_block_chain(40, 4, seed=2)
    res = KineticImportanceScore(T, pi).compute()
    assert res.k_slow == 4
    _check_compute(T, pi, 3, "four blocks")
    its = -1.0 / np.log(np.sort(np.abs(np.linalg.eigvals(T)))[::-1][1:8])
    assert KineticImportanceScore(T, pi).compute(k_slow="auto", its=its).k_slow == 3


def test_complex_leading_pair_is_refused():
    T = np.array([[0.1, 0.8, 0.1], [0.1, 0.1, 0.8], [0.8, 0.1, 0.1]])
    assert np.abs(np.linalg.eigvals(T).imag).max() > 0.5
    for k_slow in (1, 2):
        with pytest.raises(ValueError, match="complex"):
            KineticImportanceScore(T, np.full(3, 1.0 / 3.0)).compute(k_slow=k_slow)
    with pytest.raises(ValueError, match="complex"):
        KineticImportanceScore(BIRTH_DEATH, BIRTH_DEATH_PI).eigenvector_subspace_overlap(T, k=1)


# ---- the score kernel ----------------------------------------------------------------------------------------------
def test_score_kernel_scatter_and_info(engine):
    """Packed inputs of different orders in one batch: scores land at active[a], inactive states score 0, info tells
    a short active set (1) and a NaN vector row (2) apart."""
    k, n_vecs, k_slow = 70, 4, 2
    rng = np.random.default_rng(0)
    n_active = np.array([70, 33, 2, 1, 64, 0], np.int32)
    batch = len(n_active)
    vecs = rng.standard_normal((batch, n_vecs, k))
    pi = rng.random((batch, k))
    active = np.full((batch, k), -1, np.int32)
    for b, n in enumerate(n_active):
        active[b, :n] = np.sort(rng.choice(k, size=n, replace=False))
    vecs[4, 2, 5] = np.nan                                       # a needed row; row 3 is not needed
    vecs[1, 3, :] = np.nan
    scores, info = engine.kis_scores(engine.to_device(vecs), engine.to_device(pi), engine.to_device(active),
                                     engine.to_device(n_active), k_slow)
    scores = scores.to_host()
    assert info.tolist() == [0, 0, 1, 1, 2, 1]
    for b in (0, 1):
        n = n_active[b]
        want = np.zeros(k)
        want[active[b, :n]] = pi[b, :n] * (vecs[b, 1, :n] ** 2 + vecs[b, 2, :n] ** 2)
        np.testing.assert_allclose(scores[b], want, rtol=1e-15)
        assert np.all(scores[b][np.setdiff1d(np.arange(k), active[b, :n])] == 0.0)
    assert not np.any(scores[[2, 3, 5]])
    assert scores[4, active[4, 5]] == 0.0 and np.all(np.isfinite(scores[4]))


# ---- bootstrap -----------------------------------------------------------------------------------------------------
N_BOOT = 40
# name: (states, blocks, leak per block, trajectories, frames, k_slow, top_n, chain seed, bootstrap seed); the seeds are
# ones for which the reference meets the preconditions asserted below
CASES = {
    "9 states": (9, 3, (0.01, 0.03, 0.05), 6, 3000, 2, 3, 1, 3),
    "40 states": (40, 4, (0.01, 0.02, 0.035, 0.05), 8, 4000, 3, 10, 2, 4),
}


@functools.lru_cache(maxsize=None)
def _dataset(k, blocks, leaks, n_traj, frames, seed):
    d = R.trajectories(R.leaky_block_chain(k, blocks, seed, leaks), n_traj, frames, seed + 1)
    est = R.reversible_mle_packed(npport._pair_counts(d, k, 1))
    assert est["n_active"] == k
    return d, est["T"], est["pi"]


@functools.lru_cache(maxsize=None)
def _bootstrap_ref(name):
    k, blocks, leaks, n_traj, frames, k_slow, top_n, seed, boot_seed = CASES[name]
    d, T0, pi0 = _dataset(k, blocks, leaks, n_traj, frames, seed)
    return R.bootstrap_stability(T0, pi0, d, N_BOOT, k_slow, top_n, boot_seed)


def _check_bootstrap(kis, dtrajs, ref, k_slow, top_n, boot_seed, label):
    stab, std = kis.bootstrap_stability(dtrajs, n_boot=len(ref["kept"]), k_slow=k_slow, top_n=top_n,
                                        random_seed=boot_seed, lag=1)
    assert np.array_equal(kis.last_kept, ref["kept"])
    bound = float(np.nanmax(ref["bound"][ref["kept"]]))
    score_err = float(np.max(np.abs(kis.last_scores[ref["kept"]] - ref["scores"][ref["kept"]])))
    std_err = float(np.max(np.abs(std - ref["bootstrap_std"])))
    print(f"{label}: stability {stab} (reference {ref['stability_metric']}), std error {std_err:.3e}, "
          f"score error {score_err:.3e} (bound {bound:.3e})")
    assert isinstance(stab, float) and std.shape == ref["bootstrap_std"].shape
    assert stab == ref["stability_metric"]
    assert score_err <= bound and std_err <= bound            # a standard deviation moves by at most the largest shift
    return stab, std


@pytest.mark.parametrize("name", list(CASES))
def test_bootstrap_stability(name):
    k, blocks, leaks, n_traj, frames, k_slow, top_n, seed, boot_seed = CASES[name]
    d, T0, pi0 = _dataset(k, blocks, leaks, n_traj, frames, seed)
    ref = _bootstrap_ref(name)
    # preconditions, on the reference: nothing dropped, every state active, the top_n cut and the spectrum decided
    assert np.all(ref["kept"]) and np.all(ref["n_active"] == k)
    assert np.min(ref["cut_gap"]) >= 1e-7 and np.min(ref["modulus_gap"]) >= 1e-3
    assert ref["iterations"].min() >= 100
    stab, _ = _check_bootstrap(KineticImportanceScore(T0, pi0), d, ref, k_slow, top_n, boot_seed, name)
    assert 0.5 < stab < 1.0                                     # neither trivial nor noise


def test_bootstrap_is_reproducible_and_seeded():
    k, blocks, leaks, n_traj, frames, k_slow, top_n, seed, boot_seed = CASES["9 states"]
    d, T0, pi0 = _dataset(k, blocks, leaks, n_traj, frames, seed)
    kis = KineticImportanceScore(T0, pi0)
    a = kis.bootstrap_stability(d, n_boot=12, k_slow=k_slow, top_n=top_n, random_seed=5)
    b = kis.bootstrap_stability(d, n_boot=12, k_slow=k_slow, top_n=top_n, random_seed=5)
    c = kis.bootstrap_stability(d, n_boot=12, k_slow=k_slow, top_n=top_n, random_seed=6)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[1], c[1])


@functools.lru_cache(maxsize=None)
def _unvisited_case():
    """The 9-state data plus a tenth state that only one short trajectory visits."""
    k, blocks, leaks, n_traj, frames, k_slow, top_n, seed, boot_seed = CASES["9 states"]
    d, _, _ = _dataset(k, blocks, leaks, n_traj, frames, seed)
    d = list(d) + [np.array([6, 9, 7, 8, 9, 6, 7, 9, 8, 6, 9, 7, 8, 9, 7, 6, 9, 8] * 2, np.int32)]
    est = R.reversible_mle_packed(npport._pair_counts(d, 10, 1))
    return d, est["T"], est["pi"], R.bootstrap_stability(est["T"], est["pi"], d, N_BOOT, k_slow, top_n, 11)


def test_unvisited_states_score_zero():
    d, T0, pi0, ref = _unvisited_case()
    k_slow, top_n = CASES["9 states"][5:7]
    lacking = ref["n_active"] == 9
    assert 0 < lacking.sum() < N_BOOT and np.all((ref["n_active"] == 10) | lacking)
    assert np.all(ref["kept"])                                   # nothing is dropped for that reason
    assert np.nanmin(ref["cut_gap"]) >= 1e-7 and np.nanmin(ref["modulus_gap"]) >= 1e-3
    kis = KineticImportanceScore(T0, pi0)
    _check_bootstrap(kis, d, ref, k_slow, top_n, 11, "unvisited")
    assert np.all(kis.last_scores[lacking, 9] == 0.0)
    assert np.all(kis.last_scores[~lacking, 9] > 0.0)


@functools.lru_cache(maxsize=None)
def _short_active_set_case():
    """Five states, of which all trajectories but one see only two: a resample without that one has two active
    states, not more than k_slow = 2."""
    T = R.leaky_block_chain(5, 2, 3, (0.05, 0.08))
    rng = np.random.default_rng(8)
    rich = R.simulate(T, 3000, rng)
    assert np.unique(rich).size == 5
    poor = [R.simulate(np.array([[0.8, 0.2], [0.3, 0.7]]), 300, rng) for _ in range(3)]
    d = [rich] + poor
    est = R.reversible_mle_packed(npport._pair_counts(d, 5, 1))
    return d, est["T"], est["pi"], R.bootstrap_stability(est["T"], est["pi"], d, 24, 2, 2, 21)


def test_short_active_sets_are_dropped():
    d, T0, pi0, ref = _short_active_set_case()
    short = ref["n_active"] <= 2
    assert 0 < short.sum() < len(short) and np.array_equal(ref["kept"], ~short)      # only those are dropped
    assert np.nanmin(ref["cut_gap"][ref["kept"]]) >= 1e-7 and np.nanmin(ref["modulus_gap"][ref["kept"]]) >= 1e-3
    kis = KineticImportanceScore(T0, pi0)
    _check_bootstrap(kis, d, ref, 2, 2, 21, "short active sets")
    assert not np.any(kis.last_scores[short])
    with pytest.raises(RuntimeError, match="All bootstrap samples failed"):
        kis.bootstrap_stability(d[1:], n_boot=6, k_slow=2, top_n=2, random_seed=1)
    assert kis.last_kept.shape == (6,) and not np.any(kis.last_kept)


# ---- two models ----------------------------------------------------------------------------------------------------
def _symmetric_chain(k, seed):
    """Symmetric and doubly stochastic (uniform pi): its left eigenvectors are orthogonal in the 2-norm."""
    T, _ = R.reversible_block_chain(k, 3, seed)
    W = 0.5 * (T + T.T)
    np.fill_diagonal(W, 0.0)
    W *= 0.9 / W.sum(axis=1).max()
    return W + np.diag(1.0 - W.sum(axis=1))


@pytest.mark.parametrize("k", [1, 2])
def test_subspace_overlap(k):
    T = _symmetric_chain(9, 6)
    pi = np.full(9, 1.0 / 9.0)
    rng = np.random.default_rng(3)
    P = T * (1.0 + 0.2 * rng.random((9, 9)))
    P /= P.sum(axis=1, keepdims=True)
    gap = min(R.modulus_gap(T, k + 2), R.modulus_gap(P, k + 2))
    assert gap >= 0.01
    w = np.real(np.linalg.eig(P.T)[1][:, np.argmax(np.real(np.linalg.eigvals(P.T)))])
    dv = max(R.score_bound(TOL, gap, pi, k)[1], R.score_bound(TOL, gap, w / w.sum(), k)[1])
    bound = 4 * k * dv                                           # s^2 of a k x k product of vectors off by dv each
    kis = KineticImportanceScore(T, pi)
    same, other, want = kis.eigenvector_subspace_overlap(T, k=k), kis.eigenvector_subspace_overlap(P, k=k), R.subspace_overlap(T, P, k)
    print(f"k={k}: self overlap error {abs(same - 1.0):.3e}, perturbed {other} (reference {want}, error "
          f"{abs(other - want):.3e}), bound {bound:.3e}")
    assert abs(same - 1.0) <= bound
    assert abs(other - want) <= bound and want < 1.0 - 1e-6
