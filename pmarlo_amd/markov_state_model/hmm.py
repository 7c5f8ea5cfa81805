"""Discrete-output hidden Markov models: coarse-graining a microstate MSM into a few hidden states by Baum-Welch on
the device (Engine.hmm_*, csrc/hmm.hip; the contract is in include/msmhip.h, "HMM").

The workflow is that of PyEMMA's `coarse_grain` / deeptime's MaximumLikelihoodHMM seeded from an MSM: the reversible
MSM at the lag gives PCCA+ memberships, those give a start (init_hmm_from_msm), and EM runs on the lagged observation
sequences (lag_observations).  Everything here is written from the published method (Rabiner 1989; Noe, Wu, Prinz,
Plattner, J. Chem. Phys. 139, 184114, 2013); neither deeptime nor PyEMMA is available, so parity with their output
is NOT pinned.  The tests hold the kernels to a numpy restatement run in 80-bit floats (tests/_hmm_ref.py)."""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

from ..device import get_engine
from .estimation import _concat_dtrajs, _infer_states, count_transitions, fit_reversible_msm
from .its import safe_timescales
from .pcca import pcca_memberships

__all__ = ["lag_observations", "init_hmm_from_msm", "estimate_hmm", "coarse_grain_hmm", "HMMResult"]


def _sequence_table(segments, lag: int) -> np.ndarray:
    """(start, stride, length) of piece[s::lag], s = 0 .. min(lag, len) - 1, for every piece [a, b)."""
    rows = []
    for a, b in segments:
        ell = int(b) - int(a)
        for s in range(min(lag, ell)):
            rows.append((int(a) + s, lag, (ell - s + lag - 1) // lag))
    return np.asarray(rows, np.int64).reshape(-1, 3)


def lag_observations(dtrajs: Sequence[np.ndarray], lag: int, n_states: int | None = None):
    """The observation sequences of an HMM at lag time `lag`, without a copy: (labels int32 [N], table int64 [Q, 3]).
    The trajectories are concatenated and split at labels outside [0, n_states); every piece of length l gives the
    sequences piece[s::lag], s = 0 .. min(lag, l) - 1, as rows (start, stride, length) into `labels` (deeptime's
    lag_observations with stride 1).  Every valid frame belongs to exactly one sequence."""
    lag = int(lag)
    if lag < 1:
        raise ValueError("lag must be >= 1")
    n_states = _infer_states(dtrajs, n_states)
    labels, segs = _concat_dtrajs(dtrajs, n_states)
    return labels, _sequence_table(segs, lag)


def init_hmm_from_msm(T: np.ndarray, pi: np.ndarray, n_hidden: int):
    """A start (A [n, n], B [n, k], p0 [n]) for Baum-Welch from a reversible MSM (T, pi) on k microstates: with the
    PCCA+ memberships M [k, n], B ~ M' diag(pi) with rows normalised, A = (M' D M)^-1 M' D T M with negatives clipped
    and rows renormalised (Kube and Weber 2007), p0 = pi M.  A and B are mixed with 0.01 of the uniform distribution
    (0.01 / n and 0.01 / k per entry), so that no entry the fit may need starts at 0.  Written from the published
    method; parity with deeptime's metastable_from_msm is not pinned."""
    T = np.asarray(T, np.float64)
    pi = np.asarray(pi, np.float64)
    n, k = int(n_hidden), T.shape[0]
    if not 1 <= n <= k:
        raise ValueError(f"n_hidden must be in [1, {k}]")
    active = np.flatnonzero(pi > 0)
    M = np.zeros((k, n))
    M[active] = pcca_memberships(T[np.ix_(active, active)], n, pi[active] / pi[active].sum())
    B = M.T * pi[None, :]
    B /= B.sum(axis=1, keepdims=True)
    W = M.T @ (pi[:, None] * M)
    A = np.linalg.solve(W, M.T @ (pi[:, None] * (T @ M)))
    A = np.clip(A, 0.0, None)
    A /= A.sum(axis=1, keepdims=True)
    eps = 0.01
    A = (1.0 - eps) * A + eps / n
    B = (1.0 - eps) * B + eps / k
    p0 = pi @ M
    return A, B, p0 / p0.sum()


@dataclass
class HMMResult:
    transition_matrix: np.ndarray
    output_probabilities: np.ndarray
    initial_distribution: np.ndarray
    stationary_distribution: np.ndarray
    count_matrix: np.ndarray
    likelihoods: np.ndarray
    likelihood: float
    n_iterations: int
    converged: bool
    lag: int
    timescales: np.ndarray
    metastable_memberships: np.ndarray
    metastable_assignments: np.ndarray
    _gamma: np.ndarray = field(repr=False, default=None)
    _path: np.ndarray = field(repr=False, default=None)
    _lengths: list = field(repr=False, default_factory=list)

    def hidden_state_probabilities(self) -> list[np.ndarray]:
        """gamma [len, n] of every input trajectory, in frame order (zero rows for frames outside every sequence)."""
        cuts = np.cumsum([0] + self._lengths)
        return [self._gamma[a:b] for a, b in zip(cuts[:-1], cuts[1:])]

    def viterbi(self) -> list[np.ndarray]:
        """The most probable hidden path of every input trajectory, int32 in frame order.  At lag > 1 the interleaved
        lagged sequences of a trajectory are decoded independently; -1 marks frames outside every sequence."""
        cuts = np.cumsum([0] + self._lengths)
        return [self._path[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def _result(eng, tables, A, B, p0, fit, lag, lengths) -> HMMResult:
    # the state's arrays are those of the last iteration's E-step: one more E-step describes the final parameters
    last = eng.hmm_estep(tables, A, B, p0, want_emissions=False)
    Ah, Bh, pih = A.to_host(), B.to_host(), fit["pi"].to_host()
    ev = np.linalg.eigvals(Ah)
    ev = ev[np.argsort(-np.abs(ev))][1:]
    memb = pih[:, None] * Bh
    col = memb.sum(axis=0, keepdims=True)
    memb = np.divide(memb, col, out=np.full_like(memb, 1.0 / Ah.shape[0]), where=col > 0).T
    likes = np.append(fit["likelihoods"], last["total"])
    return HMMResult(transition_matrix=Ah, output_probabilities=Bh, initial_distribution=p0.to_host(),
                     stationary_distribution=pih, count_matrix=last["C"].to_host(), likelihoods=likes,
                     likelihood=float(last["total"]), n_iterations=int(fit["n_iterations"]),
                     converged=bool(fit["converged"]), lag=int(lag), timescales=safe_timescales(lag, ev),
                     metastable_memberships=memb, metastable_assignments=np.argmax(memb, axis=1),
                     _gamma=last["gamma"].to_host(), _path=eng.hmm_viterbi(tables, A, B, p0)["path"].to_host(),
                     _lengths=lengths)


def estimate_hmm(dtrajs: Sequence[np.ndarray], n_hidden: int, lag: int, n_states: int | None = None, *,
                 reversible: bool = True, stationary: bool = False, accuracy: float = 1e-3, maxit: int = 1000,
                 init=None) -> HMMResult:
    """Maximum-likelihood HMM with `n_hidden` states of the discrete trajectories at lag time `lag`.  `init` is
    (A, B, p0); None builds the reversible MSM at that lag and starts from init_hmm_from_msm.  EM stops when the
    log-likelihood moves by less than `accuracy`, or after `maxit` iterations."""
    n_states = _infer_states(dtrajs, n_states)
    labels, table = lag_observations(dtrajs, lag, n_states)
    if table.shape[0] == 0:
        raise ValueError("no valid frames")
    if init is None:
        T, pi, _ = fit_reversible_msm(count_transitions(dtrajs, n_states, lag=int(lag)))
        init = init_hmm_from_msm(T, pi, n_hidden)
    A0, B0, p00 = (np.ascontiguousarray(x, np.float64) for x in init)
    if A0.shape != (n_hidden, n_hidden) or B0.shape != (n_hidden, n_states) or p00.shape != (n_hidden,):
        raise ValueError("init must be (A [n, n], B [n, k], p0 [n])")
    eng = get_engine()
    tables = eng.hmm_tables(eng.to_device(labels), n_states, table)
    A, B, p0 = eng.to_device(A0), eng.to_device(B0), eng.to_device(p00)
    fit = eng.hmm_fit(tables, A, B, p0, reversible=reversible, stationary=stationary, accuracy=accuracy, maxit=maxit)
    return _result(eng, tables, A, B, p0, fit, lag, [len(d) for d in dtrajs if len(d)])


def coarse_grain_hmm(dtrajs: Sequence[np.ndarray], n_states: int, n_macrostates: int, lag: int) -> HMMResult:
    """The microstate trajectories coarse-grained into an HMM of `n_macrostates` hidden states at `lag` (PyEMMA's
    `coarse_grain`): estimate_hmm with its defaults."""
    return estimate_hmm(dtrajs, int(n_macrostates), int(lag), int(n_states))
