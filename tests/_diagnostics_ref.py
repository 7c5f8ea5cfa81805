"""Numpy restatement of msm_autocorr_lagscan's definition (include/msmhip.h), classical canonical correlations,
and the seeded input recipes that tests/golden/make_golden_diagnostics.py and the diagnostics tests share
(test infrastructure only: the goldens hold the reference's outputs, the inputs are regenerated from here)."""

from __future__ import annotations

import numpy as np

VAR_FLOOR = 1e-8


# ---------------------------------------------------------------------------------------------------------------
# the kernel's definition
# ---------------------------------------------------------------------------------------------------------------
def autocorr_lagscan_ref(x, starts, stops, lags, var_floor: float = VAR_FLOOR, acc=np.longdouble):
    """(values f64 [n_seg, n_lag], nvalid int32 [n_seg]); sums are carried in ``acc`` (long double by default, so the
    result is the definition's value to well below the 1e-11 the kernel is held to)."""
    x = np.asarray(x)
    values = np.full((len(starts), len(lags)), np.nan)
    nvalid = np.zeros(len(starts), np.int32)
    for s, (a, b) in enumerate(zip(starts, stops)):
        L = int(b) - int(a)
        if L <= 0:
            continue
        with np.errstate(all="ignore"):
            blk = x[int(a):int(b)].astype(acc)
            c = blk - blk.mean(axis=0)
            var = (c * c).mean(axis=0)
            valid = np.asarray(var > acc(var_floor))
            m = int(valid.sum())
            nvalid[s] = m
            if m == 0 or L <= 1:
                continue
            z = c[:, valid] / np.sqrt(var[valid])
            for l, tau in enumerate(lags):
                tau = int(tau)
                if tau >= L:
                    continue
                values[s, l] = float((z[:L - tau] * z[tau:]).sum() / (acc(L - tau) * m))
    return values, nvalid


def cca_classical(X, Y) -> np.ndarray:
    """Canonical correlations by QR of both centred blocks and the singular values of Qx' Qy, descending."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    n = min(len(X), len(Y))
    X, Y = X[:n] - X[:n].mean(axis=0), Y[:n] - Y[:n].mean(axis=0)
    qx, _ = np.linalg.qr(X)
    qy, _ = np.linalg.qr(Y)
    return np.clip(np.linalg.svd(qx.T @ qy, compute_uv=False), 0.0, 1.0)


def cov_condition(X) -> float:
    X = np.asarray(X, np.float64)
    return float(np.linalg.cond(np.cov(X - X.mean(axis=0), rowvar=False, ddof=0)))


# ---------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------
def ar1(rng, n: int, coefs) -> np.ndarray:
    """Stationary AR(1) columns with unit innovations."""
    coefs = np.asarray(coefs, np.float64)
    e = rng.standard_normal((n, len(coefs)))
    out = np.empty_like(e)
    out[0] = e[0] / np.sqrt(1.0 - coefs ** 2)
    for t in range(1, n):
        out[t] = coefs * out[t - 1] + e[t]
    return out


CURVE_SEGMENTS = (40_000, 1, 25_000, 35_000)
CURVE_LAGS = (1, 2, 5, 10, 30, 100, 300, 1000, 3000, 10_000, 24_999, 25_000, 30_000)
CURVE_SEED = 20240917


def curve_input(offset: float = 0.0, dtype=np.float64) -> np.ndarray:
    """AR(1) columns 0.999 / 0.99 / 0.9 / 0.5 (the 0.9 one scaled by 1e-3) and a fifth column that is constant inside
    the third segment only; ``offset`` is added to everything before the cast."""
    rng = np.random.default_rng(CURVE_SEED)
    n = sum(CURVE_SEGMENTS)
    x = ar1(rng, n, [0.999, 0.99, 0.9, 0.5, 0.95])
    x[:, 2] *= 1e-3
    a = CURVE_SEGMENTS[0] + CURVE_SEGMENTS[1]
    x[a:a + CURVE_SEGMENTS[2], 4] = 0.75
    return (x + offset).astype(dtype)


CURVE_CASES = {"f64_offset0": (0.0, np.float64), "f64_offset1000": (1000.0, np.float64),
               "f32_offset0": (0.0, np.float32), "f32_offset1000": (1000.0, np.float32)}

NONFINITE_SEGMENTS = (3000, 2000, 4000)
NONFINITE_LAGS = (1, 3, 10, 100, 1500, 2500)


def nonfinite_input() -> np.ndarray:
    """Two AR(1) columns; the middle segment holds a NaN in one column and an Inf in the other."""
    rng = np.random.default_rng(77)
    x = ar1(rng, sum(NONFINITE_SEGMENTS), [0.9, 0.6])
    x[3500, 0] = np.nan
    x[4100, 1] = np.inf
    return x


def _mixing(rng, p: int, log10_cond_half: float) -> np.ndarray:
    u, _ = np.linalg.qr(rng.standard_normal((p, p)))
    v, _ = np.linalg.qr(rng.standard_normal((p, p)))
    return u @ np.diag(np.logspace(0.0, log10_cond_half, p)) @ v.T


CCA_CASES = {
    # name: (seed, n, p, q, population correlations, log10 of the mixing's singular-value spread, duplicate a column)
    "n5000_p8_q3": (11, 5000, 8, 3, (0.9, 0.6, 0.3), 1.0, False),
    "n20000_p6_q6": (12, 20000, 6, 6, (0.95, 0.8, 0.65, 0.5, 0.35, 0.2), 1.5, False),
    "n3000_p4_q2": (13, 3000, 4, 2, (0.99, 0.7), 2.0, False),
    "duplicated_column": (14, 4000, 3, 3, (0.85, 0.5), 0.5, True),
}


def cca_input(name: str):
    """(X, Y): Y's latent columns correlate with X's at the given population values; both blocks are then mixed.
    With the duplicate flag X's last column repeats its first (rank p - 1) and carries no correlation of its own."""
    seed, n, p, q, rho, spread, dup = CCA_CASES[name]
    rng = np.random.default_rng(seed)
    zx = rng.standard_normal((n, p))
    zy = rng.standard_normal((n, q))
    for j, r in enumerate(rho):
        zy[:, j] = r * zx[:, j] + np.sqrt(1.0 - r * r) * zy[:, j]
    if dup:
        X = zx.copy()
        X[:, :p - 1] = zx[:, :p - 1] @ _mixing(rng, p - 1, spread)
        X[:, p - 1] = X[:, 0]
    else:
        X = zx @ _mixing(rng, p, spread)
    Y = zy @ _mixing(rng, q, spread)
    return X + rng.standard_normal(p), Y + rng.standard_normal(q)


def cca_expected(name: str) -> np.ndarray:
    """Classical values; for the rank-deficient case those of the reduced problem, then zeros."""
    X, Y = cca_input(name)
    _, n, p, q, _, _, dup = CCA_CASES[name]
    if not dup:
        return cca_classical(X, Y)
    out = np.zeros(min(p, q, n))
    sv = cca_classical(X[:, :p - 1], Y)
    out[:len(sv)] = sv[:len(out)]
    return out


E2E_CASES = {
    # name: (CVs follow the inputs, slow CVs, diag_mass, user taus or None)
    "auto_taus_reparam_high_mass": (True, False, 0.97, None),
    "user_taus_flat_low_mass": (False, True, 0.5, [1, 2, 5, 20, 100, 1000]),
}


def e2e_dataset(name: str) -> dict:
    """Two splits: "train" with whitening metadata, inputs and segment lengths, "val" a bare array.  Built afresh
    on every call: the whitening marks its metadata as applied."""
    follow, slow, _, _ = E2E_CASES[name]
    rng = np.random.default_rng(500 + sorted(E2E_CASES).index(name))
    n_train, n_val, d = 6000, 4000, 3
    coefs = [0.999, 0.998, 0.997] if slow else [0.9, 0.6, 0.3]
    inputs = ar1(rng, n_train, coefs + [0.5, 0.2])
    if follow:
        cvs = inputs[:, :d] @ _mixing(rng, d, 0.5) + 0.02 * rng.standard_normal((n_train, d))
    else:
        cvs = 0.3 * inputs[:, :d] + ar1(rng, n_train, coefs)
    meta = {"output_mean": cvs.mean(axis=0) + 0.1, "output_transform": _mixing(rng, d, 0.3),
            "output_transform_applied": False}
    train = {"X": cvs, "meta": meta, "inputs": inputs, "segment_lengths": [2500, 3500]}
    return {"splits": {"train": train, "val": ar1(rng, n_val, coefs)}}
