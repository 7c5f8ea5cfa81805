"""Kinetic importance scores and their bootstrap stability on the device.

Mirrors pmarlo.conformations.kinetic_importance.KineticImportanceScore (S/conformations/kinetic_importance.py:17-315,
431-456) and KISResult (S/conformations/results.py:74-111): KIS(i) = pi_i * sum_{k=2..K_slow+1} phi_k(i)^2 over the
slow left eigenvectors phi_k of T (unit 2-norm), which ranks microstates that are both populated and involved in the
slow dynamics, and the stability of that ranking when whole trajectories are resampled with replacement.

compute: the leading k_slow + 1 left eigenvectors come from the engine's spectrum solver (msm_spectrum, subspace of
at most 32 vectors, hence k_slow <= 31), the scores from msm_kis_scores; the ranking is an argsort on the host.

bootstrap_stability: every trajectory is counted once and the counts of a resample are the exact integer combination
(Engine.bootstrap_counts, as for UncertaintyQuantifier); all resamples are then re-estimated by ONE launch of the
batched reversible maximum-likelihood estimator (msm_reversible_mle_batched: active set, prior 1e-3 on the active
block as ensure_connected_counts adds it, deeptime's stopping rule maxerr = 1e-8), their spectra by the batched
spectrum solver and their scores by msm_kis_scores.  The overlap of the top_n rankings and the standard deviation
over at most n_boot x n_states numbers are numpy on the host.

Resampling: the indices are drawn on the host from np.random.default_rng(random_seed) in the reference's order
(n_traj scalar integers(0, n_traj) draws per sample, sample by sample), so equal seeds give the reference's resamples.

Stated divergences from the reference:
  * Complex Ritz values.  The reference takes the real part of a complex eigenvector with a warning; here compute and
    eigenvector_subspace_overlap raise ValueError when one of the needed eigenvalues is complex (a sum of squares of
    real parts is not a property of the matrix).
  * Unvisited states.  The reference embeds T = I on the states a resample never visits, which gives the eigenvalue 1
    a multiplicity and makes its "slow" vectors arbitrary.  Here the slow modes of a resample are those of its active
    block, and its inactive states score exactly 0.
  * A resample is dropped, and counted in a warning as the reference's `except` does, when its active set has at most
    k_slow states, its estimate did not reach maxerr, its spectrum did not converge, or a needed eigenvector belongs
    to a complex pair.  RuntimeError when none is left.  last_kept holds the mask of the latest bootstrap and
    last_scores the scores of all its samples.

Parity: the reference delegates counting and the reversible estimate to deeptime 0.4.5 and the partial spectrum to
scipy's eigs; neither is present, so parity with the reference's own output is unpinned.  The tests hold this module to
a numpy restatement of the rules above.

Not ported: hyperparameter_ensemble_stability and _recluster (they re-cluster with scikit-learn's
MiniBatchKMeans(random_state=42), whose stream cannot be reproduced).  finder.py and state_detection.py are ported
(finder.py, state_detection.py of this package)."""

from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from ..device import get_engine
from .uncertainty import UncertaintyQuantifier

__all__ = ["KineticImportanceScore", "KISResult"]

logger = logging.getLogger("pmarlo.conformations")

# the prior ensure_connected_counts adds to every active cell, deeptime's stopping rule, the spectrum's residual bound
_ALPHA, _MAXERR, _SPECTRUM_TOL = 1e-3, 1e-8, 1e-9
_MAX_K_SLOW = 31                             # the spectrum solver's subspace holds 32 vectors, one is stationary


@dataclass(frozen=True)
class KISResult:
    """Scores per microstate, the number of slow modes, the eigenvectors used ((k_slow + 1) x n_states, row 0 the
    stationary one) with their eigenvalues, the states by descending score, and the bootstrap figures when computed
    (results.py:74-111)."""

    kis_scores: np.ndarray
    k_slow: int
    eigenvectors: np.ndarray
    eigenvalues: np.ndarray
    ranked_states: np.ndarray
    stability_metric: Optional[float] = None
    bootstrap_std: Optional[np.ndarray] = None

    def to_dict(self) -> Dict[str, Any]:
        return {
            "kis_scores": self.kis_scores.tolist(),
            "k_slow": int(self.k_slow),
            "eigenvectors": self.eigenvectors.tolist(),
            "eigenvalues": self.eigenvalues.tolist(),
            "ranked_states": self.ranked_states.tolist(),
            "stability_metric": float(self.stability_metric) if self.stability_metric is not None else None,
            "bootstrap_std": self.bootstrap_std.tolist() if self.bootstrap_std is not None else None,
        }


def _draw_multiplicities(rng: np.random.Generator, n_traj: int, n_boot: int) -> np.ndarray:
    """[n_boot, n_traj] int32: how often trajectory s occurs in sample b, drawn in the reference's order."""
    mult = np.zeros((int(n_boot), int(n_traj)), np.int32)
    for b in range(int(n_boot)):
        for _ in range(int(n_traj)):
            mult[b, rng.integers(0, n_traj)] += 1
    return mult


def _left_eigenvectors(T: np.ndarray, n_vecs: int) -> Tuple[np.ndarray, np.ndarray]:
    """The n_vecs eigenvalues of largest modulus (descending) and their unit-norm left eigenvectors as rows."""
    eng = get_engine()
    spec = eng.spectrum(eng.to_device(np.ascontiguousarray(T, np.float64)), n_vecs=int(n_vecs), want_pi=False)
    values = spec["ritz"][0, :n_vecs]
    vectors = spec["vecs"].to_host()[0]
    if np.any(values.imag != 0.0) or not np.all(np.isfinite(vectors)):
        raise ValueError("a needed eigenvalue of the transition matrix is complex: its eigenvector has no real form "
                         f"(leading values {values.tolist()})")
    return values.real.copy(), vectors


class KineticImportanceScore:
    """KIS(i) = pi_i * sum of phi_k(i)^2 over the k_slow slow left eigenvectors of T."""

    def __init__(self, T: np.ndarray, pi: np.ndarray) -> None:
        self.T = np.asarray(T, dtype=float)
        self.pi = np.asarray(pi, dtype=float)
        self.n_states = self.T.shape[0]
        if self.T.ndim != 2 or self.T.shape[0] != self.T.shape[1]:
            raise ValueError("Transition matrix must be square")
        if len(self.pi) != self.n_states:
            raise ValueError("Stationary distribution length must match T dimensions")
        self.last_kept = np.zeros(0, bool)       # which samples of the latest bootstrap survived, in draw order
        self.last_scores = np.zeros((0, self.n_states))      # the scores of all its samples [n_boot, n_states]

    # -- scores ------------------------------------------------------------------------------------------------------
    def _check_k_slow(self, k_slow: int) -> int:
        k_slow = int(k_slow)
        if k_slow < 1 or k_slow >= self.n_states:
            raise ValueError(f"k_slow must be between 1 and n_states-1 ({self.n_states - 1}), got {k_slow}")
        if k_slow > _MAX_K_SLOW:
            raise ValueError(f"k_slow must be at most {_MAX_K_SLOW} (the spectrum solver's subspace), got {k_slow}")
        return k_slow

    def compute(self, k_slow: int | str = "auto", its: Optional[np.ndarray] = None) -> KISResult:
        """Scores of all states; k_slow 'auto' asks select_k_slow(its)."""
        k_slow_val = self._check_k_slow(self.select_k_slow(its) if isinstance(k_slow, str) and k_slow == "auto" else k_slow)
        logger.info("Computing KIS with k_slow=%d", k_slow_val)
        eigenvalues, eigenvectors = self._compute_eigenvectors(k_slow_val + 1)
        eng = get_engine()
        n = self.n_states
        scores, info = eng.kis_scores(eng.to_device(eigenvectors.reshape(1, k_slow_val + 1, n)),
                                      eng.to_device(self.pi.reshape(1, n)),
                                      eng.to_device(np.arange(n, dtype=np.int32).reshape(1, n)),
                                      eng.to_device(np.array([n], np.int32)), k_slow_val)
        if info[0] != 0:
            raise ValueError(f"the kinetic importance scores are undefined (msm_kis_scores info {int(info[0])})")
        kis_scores = scores.to_host()[0]
        ranked_states = np.argsort(kis_scores)[::-1]
        logger.info("KIS computed. Top state: %d (score: %.6f)", ranked_states[0], kis_scores[ranked_states[0]])
        return KISResult(kis_scores=kis_scores, k_slow=k_slow_val, eigenvectors=eigenvectors, eigenvalues=eigenvalues,
                         ranked_states=ranked_states)

    # -- the number of slow modes (host arithmetic) ------------------------------------------------------------------
    def select_k_slow(self, its: Optional[np.ndarray] = None, method: str = "timescale_gap",
                      gap_threshold: float = 2.0) -> int:
        """The largest ratio of consecutive implied timescales when `its` is given, the eigenvalue variance rule for
        method 'variance', otherwise min(5, max(2, n_states // 10))."""
        if method == "timescale_gap" and its is not None:
            return self._select_by_timescale_gap(its, gap_threshold)
        if method == "variance":
            return self._select_by_variance_explained()
        default_k = min(5, max(2, self.n_states // 10))
        logger.debug("Using default k_slow=%d", default_k)
        return int(default_k)

    def _select_by_timescale_gap(self, its: np.ndarray, gap_threshold: float) -> int:
        its = np.asarray(its)
        if len(its) < 2:
            return 2
        ratios = its[:-1] / np.maximum(its[1:], 1e-10)
        gap_idx = int(np.argmax(ratios))
        if ratios[gap_idx] >= gap_threshold:
            k_slow = gap_idx + 1
            logger.debug("Timescale gap detected at index %d (ratio: %.2f), k_slow=%d", gap_idx, ratios[gap_idx], k_slow)
        else:
            k_slow = int(min(5, len(its)))
            logger.debug("No clear gap (max ratio: %.2f), k_slow=%d", ratios[gap_idx], k_slow)
        return int(max(2, k_slow))

    def _select_by_variance_explained(self, variance_threshold: float = 0.9) -> int:
        """Smallest number of squared eigenvalues (descending) that reaches the threshold of their sum.  Needs all
        eigenvalues: numpy on the host (a selection helper, not a hot path)."""
        squared = np.sort(np.real(np.linalg.eigvals(self.T.T)) ** 2)[::-1]
        total = np.sum(squared)
        k_slow = int(np.searchsorted(np.cumsum(squared) / total, variance_threshold) + 1) if total > 0 else 2
        k_slow = int(max(2, min(k_slow, self.n_states - 1)))
        logger.debug("Variance-based selection: k_slow=%d", k_slow)
        return k_slow

    # -- eigenvectors ------------------------------------------------------------------------------------------------
    @staticmethod
    def _compute_eigenvectors_for(T: np.ndarray, n_vecs: int) -> Tuple[np.ndarray, np.ndarray]:
        """(eigenvalues, eigenvectors): the min(n_vecs, n) eigenvalues of largest modulus, descending, and their
        unit-norm left eigenvectors as rows.  ValueError when one of them is complex or n_vecs exceeds 32."""
        T = np.asarray(T, dtype=float)
        n_vecs = min(int(n_vecs), T.shape[0])
        if n_vecs > _MAX_K_SLOW + 1:
            raise ValueError(f"at most {_MAX_K_SLOW + 1} eigenvectors (the spectrum solver's subspace), got {n_vecs}")
        return _left_eigenvectors(T, n_vecs)

    def _compute_eigenvectors(self, n_vecs: int) -> Tuple[np.ndarray, np.ndarray]:
        return self._compute_eigenvectors_for(self.T, n_vecs)

    # -- bootstrap ---------------------------------------------------------------------------------------------------
    def bootstrap_stability(self, dtrajs: List[np.ndarray], n_boot: int = 200, k_slow: Optional[int] = None,
                            top_n: int = 10, random_seed: Optional[int] = None, lag: int = 1) -> Tuple[float, np.ndarray]:
        """(stability_metric, bootstrap_std): the mean share of the original top_n states found in a resample's
        top_n, and the standard deviation of every state's score over the resamples that were kept."""
        if k_slow is None:
            k_slow = self.select_k_slow()
        logger.info("Bootstrap KIS stability with %d samples", n_boot)
        original_top = self.compute(k_slow=k_slow).ranked_states[:top_n]
        k_slow = int(k_slow)
        labels, starts, stops, k = UncertaintyQuantifier._check_dtrajs(dtrajs)
        k = max(k, self.n_states)
        mult = _draw_multiplicities(np.random.default_rng(random_seed), len(starts), n_boot)
        kept = np.zeros(int(n_boot), bool)
        valid = np.zeros((int(n_boot), k))
        eng = get_engine()
        chunks = eng.bootstrap_counts(eng.to_device(labels), starts, stops, k, int(lag), mult) if int(n_boot) > 0 else ()
        for b, nb, counts in chunks:
            mle = eng.reversible_mle_batched(counts, alpha=_ALPHA, maxerr=_MAXERR)
            ok = (mle["n_active"].to_host() > k_slow) & (mle["err"] <= _MAXERR)
            # a sample that is already out leaves the spectrum as an empty matrix
            n_spec = eng.to_device(np.where(ok, mle["n_active"].to_host(), 0).astype(np.int32))
            spec = eng.spectrum(mle["T"], n=n_spec, n_vecs=k_slow + 1, want_pi=False, tol=_SPECTRUM_TOL,
                                allow_unconverged=True)
            scores, info = eng.kis_scores(spec["vecs"], mle["pi"], mle["active"], n_spec, k_slow)
            ok &= (spec["residual"] <= _SPECTRUM_TOL) & (info == 0)
            kept[b:b + nb] = ok
            valid[b:b + nb] = scores.to_host()
        self.last_kept, self.last_scores = kept, valid
        failed = int(np.sum(~kept))
        if failed > 0:
            logger.warning("%d/%d bootstrap samples failed and were excluded", failed, n_boot)
        if not np.any(kept):
            raise RuntimeError("All bootstrap samples failed; cannot compute stability")
        valid = valid[kept]
        overlap = np.array([len(np.intersect1d(original_top, np.argsort(row)[::-1][:top_n])) for row in valid], dtype=float)
        stability_metric = float(np.mean(overlap) / top_n)
        bootstrap_std = np.std(valid, axis=0)
        logger.info("KIS stability metric: %.3f", stability_metric)
        return stability_metric, bootstrap_std

    # -- two models --------------------------------------------------------------------------------------------------
    def eigenvector_subspace_overlap(self, T_other: np.ndarray, k: Optional[int] = None) -> float:
        """mean(s^2) of the singular values of V1'V2, V the k slow left eigenvectors (rows 1 .. k) of either matrix:
        1 for equal subspaces when the vectors within one are orthogonal, 0 for orthogonal subspaces."""
        if k is None:
            k = self.select_k_slow()
        k = int(k)
        _, evecs1 = self._compute_eigenvectors(k + 1)
        _, evecs2 = self._compute_eigenvectors_for(np.asarray(T_other, dtype=float), k + 1)
        s = np.linalg.svd(evecs1[1:k + 1] @ evecs2[1:k + 1].T, compute_uv=False)
        return float(np.mean(s ** 2))
