"""Plain numpy sampler of the reversible posterior (a distribution oracle for msm_sample_reversible_transition_matrices,
not a stream oracle: its scan, its updates and its random numbers are its own).

Target (Trendelkamp-Schroer, Wu, Paul and Noe, J. Chem. Phys. 143, 174101 (2015), improper "-1" prior), for a symmetric
non-negative X with x_i = sum_k x_ik, T_ij = x_ij / x_i, pi_i = x_i / sum x and c_i = sum_j C_ij:

    p(X | C)  ~  prod_i x_ii^(C_ii - 1)  prod_{i<j} x_ij^(C_ij + C_ji - 1)  prod_i x_i^(-c_i)

Vectorised over chains, sequential over cells.  Per sweep: every diagonal by its exact conditional
x_ii / x_i ~ Beta(C_ii, c_i - C_ii), every live off-diagonal by two plain random-walk Metropolis steps on log x_ij
(a wide and a narrow one) against the conditional v^(a-1) (v + v1)^(-c_i) (v + v2)^(-c_j), then sum x = 1.
Cells with C_ij + C_ji == 0 stay exactly 0."""
from __future__ import annotations

import numpy as np


def _log_cond(w, a, ci, cj, v1, v2):
    """log density of w = log x_ij (the Jacobian included)"""
    v = np.exp(w)
    return a * w - ci * np.log(v + v1) - cj * np.log(v + v2)


def sample(C, n_chains: int, n_sweeps: int, seed: int = 0):
    """(T [S, n, n], pi [S, n]) after n_sweeps sweeps of S = n_chains independent chains started at C + C'."""
    C = np.asarray(C, dtype=np.float64)
    n = C.shape[0]
    rng = np.random.default_rng(seed)
    c = C.sum(1)
    A = C + C.T
    X = np.repeat((A / A.sum())[None], n_chains, axis=0)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if A[i, j] > 0]
    for _ in range(int(n_sweeps)):
        for i in range(n):
            a, b = C[i, i], c[i] - C[i, i]
            if a > 0 and b > 0:
                s = X[:, i, :].sum(1) - X[:, i, i]
                u = rng.beta(a, b, size=n_chains)
                X[:, i, i] = np.where(s > 0, s * u / (1.0 - u), X[:, i, i])
        for i, j in pairs:
            a = A[i, j]
            for width in (2.0, 0.6):
                v = X[:, i, j]
                v1 = X[:, i, :].sum(1) - v
                v2 = X[:, j, :].sum(1) - v
                w = np.log(v)
                wp = w + width / np.sqrt(max(a, 0.25)) * rng.standard_normal(n_chains)
                with np.errstate(all="ignore"):
                    delta = _log_cond(wp, a, c[i], c[j], v1, v2) - _log_cond(w, a, c[i], c[j], v1, v2)
                    take = np.log(rng.random(n_chains)) < delta
                vn = np.where(take, np.exp(wp), v)
                X[:, i, j] = vn
                X[:, j, i] = vn
        X /= X.sum((1, 2), keepdims=True)
    x = X.sum(2)
    return X / x[:, :, None], x / x.sum(1, keepdims=True)


def slowest_timescale(T, lag: float = 1.0):
    """-lag / log |lambda_2|, lambda_2 the second largest eigenvalue by magnitude, of every matrix of a batch."""
    ev = np.sort(np.abs(np.linalg.eigvals(T)), axis=-1)[:, -2]
    with np.errstate(all="ignore"):
        return -float(lag) / np.log(ev)
