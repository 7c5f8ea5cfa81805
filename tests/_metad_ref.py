"""The metadynamics law in numpy: host-only companion of tests/test_metad_reference.py, tests/test_gpu_metad.py and
tests/test_gpu_metad_paths.py.  No product code, no device code.

Restated here as include/msmhip.h states it for msm_metad_bias and msm_metad_grid_scan, on PACKED hills
[H, 2 d + 1] = (centre, 1 / sigma, height), fp64 inputs; `dtype` is the arithmetic (float64: what the device is held
to; longdouble: the yardstick of its rounding):

    dp_i = s_i - c_i;  periodic: dp_i -= P_i rint(dp_i / P_i);  z_i = dp_i (1 / sigma_i)
    dp2 = 0.5 sum_i z_i^2 (ascending i);  nothing where dp2 >= cut
    term = h (A exp(-dp2) + B),  d term / d s_i = -(h (A exp(-dp2))) (z_i (1 / sigma_i))
    A = 1, B = 0 (gaussian);  A = 1 / (1 - exp(-cut)), B = -exp(-cut) A (stretched-gaussian), both formed in fp64:
    they are constants of the law, handed to either arithmetic as the fp64 numbers they are.

A frame adds its first count[n] terms in ascending hill index (np.cumsum is sequential).

The rounding bound (`bound`).  exp(-dp2) carries the rounding of its argument, at most 6.25 relative roundings of dp2,
which itself is built from 2 d + 3 rounded operations on z (subtract, wrap, scale, square, add, halve): a relative
error of 6.25 (2 d + 3) eps on exp.  Four more roundings shape the term (A e, + B, h *, and exp's own), and a sum of
H_n terms adds H_n eps of the sum of their magnitudes.  The magnitude of a term is h (A exp(-dp2) + |B|), NOT |term|:
near the cutoff the stretched term is a small difference of A exp(-dp2) and |B|, and each of the two carries its own
rounding.  Hence, per frame,
    |fp64 - exact| <= (6.25 (2 d + 3) + 4 + H_n) eps  sum_k h_k (A exp(-dp2_k) + |B|).
The gradient's terms are the value's times z_i / sigma_i, one more rounding each; its bound is the same factor on the
sum of the absolute gradient terms (which is at most the value's bound times max |dp / sigma^2|)."""

from __future__ import annotations

import numpy as np

CUT = 6.25
EPS = float(np.finfo(np.float64).eps)
KERNELS = ("gaussian", "stretched-gaussian")


def pack(centers, sigmas, heights) -> np.ndarray:
    """[H, 2 d + 1] fp64: centre, 1 / sigma (the fp64 quotient), height."""
    c = np.asarray(centers, np.float64)
    c = c.reshape(c.shape[0], -1) if c.ndim else c.reshape(0, 1)
    s = np.broadcast_to(np.asarray(sigmas, np.float64), c.shape) if np.ndim(sigmas) < 2 else np.asarray(sigmas, np.float64)
    h = np.broadcast_to(np.asarray(heights, np.float64), (c.shape[0],))
    return np.ascontiguousarray(np.concatenate([c, 1.0 / s, h[:, None]], axis=1))


def constants(kernel: str, cut: float = CUT) -> tuple[float, float]:
    assert kernel in KERNELS
    if kernel == "gaussian":
        return 1.0, 0.0
    A = 1.0 / (1.0 - np.exp(-np.float64(cut)))
    return float(A), float(-np.exp(-np.float64(cut)) * A)


def hill_terms(cv, packed, periods=None, kernel="gaussian", cut=CUT, dtype=np.float64, strict=True):
    """(term [n, H], dterm [n, H, d], magnitude [n, H], |dterm| [n, H, d]) in `dtype`.  strict=False is the WRONG
    reading `dp2 <= cut` (kept only to show that a golden file tells the two apart)."""
    t = np.dtype(dtype).type
    packed = np.asarray(packed, np.float64)
    d = (packed.shape[1] - 1) // 2
    s = np.asarray(cv, np.float64)[:, None, :d].astype(t)
    c, isg, h = packed[None, :, :d].astype(t), packed[None, :, d:2 * d].astype(t), packed[None, :, 2 * d].astype(t)
    dp = s - c
    if periods is not None:
        for i, P in enumerate(np.asarray(periods, np.float64)):
            if P > 0:
                dp[..., i] = dp[..., i] - t(P) * np.rint(dp[..., i] / t(P))
    z = dp * isg
    q = z[..., 0] * z[..., 0]
    for i in range(1, d):
        q = q + z[..., i] * z[..., i]
    q = t(0.5) * q
    A, B = (t(v) for v in constants(kernel, cut))
    with np.errstate(over="ignore", invalid="ignore"):
        live = (q < t(cut)) if strict else (q <= t(cut))
        e = np.exp(-np.where(live, q, t(0)))
        term = np.where(live, h * (A * e + B), t(0))
        mag = np.where(live, np.abs(h) * (A * e + np.abs(B)), t(0))
        w = -(h * (A * e))
        dterm = np.where(live[..., None], w[..., None] * (z * isg), t(0))
    return term, dterm, mag, np.abs(dterm)


def _take(prefix, counts):
    """prefix [n, H (, d)] of sequential sums -> the entry count - 1 of every row, 0 where count == 0."""
    n, H = prefix.shape[:2]
    out = np.zeros((n,) + prefix.shape[2:], prefix.dtype)
    rows = np.nonzero(counts > 0)[0]
    out[rows] = prefix[rows, counts[rows] - 1]
    return out


def bias(cv, packed, counts=None, periods=None, kernel="gaussian", cut=CUT, dtype=np.float64, strict=True):
    """{"bias" [n], "grad" [n, d], "mag" [n] (sum of the terms' magnitudes), "gmag" [n, d], "count" [n]} in `dtype`.
    A frame with a non-finite CV is NaN in bias and grad."""
    cv = np.asarray(cv, np.float64)
    cv = cv.reshape(cv.shape[0], -1)
    packed = np.asarray(packed, np.float64)
    n, H = cv.shape[0], packed.shape[0]
    d = (packed.shape[1] - 1) // 2
    counts = np.full(n, H, np.int64) if counts is None else np.clip(np.asarray(counts, np.int64), 0, H)
    t = np.dtype(dtype).type
    bad = ~np.isfinite(cv[:, :d]).all(axis=1)
    safe = np.where(bad[:, None], 0.0, cv[:, :d])
    if H == 0:
        z1, zd = np.zeros(n, t), np.zeros((n, d), t)
        out = {"bias": z1, "grad": zd, "mag": z1.copy(), "gmag": zd.copy()}
    else:
        term, dterm, mag, dmag = hill_terms(safe, packed, periods, kernel, cut, dtype, strict)
        out = {"bias": _take(np.cumsum(term, axis=1), counts), "grad": _take(np.cumsum(dterm, axis=1), counts),
               "mag": _take(np.cumsum(mag, axis=1), counts), "gmag": _take(np.cumsum(dmag, axis=1), counts)}
    out["bias"][bad] = np.nan
    out["grad"][bad] = np.nan
    out["count"] = counts
    return out


def bound_factor(d: int, counts) -> np.ndarray:
    """(6.25 (2 d + 3) + 4 + H_n) eps: times the sum of the terms' magnitudes it bounds |fp64 - exact| of a frame."""
    return (CUT * (2 * d + 3) + 4 + np.asarray(counts, np.float64)) * EPS


def counts_from_times(hill_times, frame_times) -> np.ndarray:
    """A frame sees the hills deposited strictly before its time."""
    return np.searchsorted(np.asarray(hill_times, np.float64), np.asarray(frame_times, np.float64), side="left").astype(np.int32)


# ---- the grid and c(t) ---------------------------------------------------------------------------------------------
def grid_spec(lo, hi, bins, periods=None):
    """(lo, step, bins): `bins` points per axis from lo to hi inclusive; a periodic axis has no duplicate end point."""
    lo, hi = np.atleast_1d(np.asarray(lo, np.float64)), np.atleast_1d(np.asarray(hi, np.float64))
    bins = np.atleast_1d(np.asarray(bins, np.int32))
    per = np.zeros(lo.size) if periods is None else np.asarray(periods, np.float64)
    step = np.where(per > 0, (hi - lo) / bins, (hi - lo) / np.maximum(bins - 1, 1))
    return lo, step, bins


def grid_points(lo, step, bins) -> np.ndarray:
    """[G, d], the last axis fastest: point i_a at lo_a + i_a * step_a."""
    axes = [np.asarray(l + np.arange(b, dtype=np.float64) * s) for l, s, b in zip(lo, step, bins)]
    mesh = np.meshgrid(*axes, indexing="ij")
    return np.stack([m.reshape(-1) for m in mesh], axis=1)


def grid_prefix(packed, lo, step, bins, periods=None, kernel="gaussian", cut=CUT, dtype=np.float64):
    """(V [G, H + 1] with V[:, k] the sum of the first k hills, magnitudes [G, H + 1]) in `dtype`."""
    pts = grid_points(lo, step, bins)
    t = np.dtype(dtype).type
    H = np.asarray(packed).shape[0]
    V, Mg = np.zeros((pts.shape[0], H + 1), t), np.zeros((pts.shape[0], H + 1), t)
    if H:
        term, _d, mag, _g = hill_terms(pts, packed, periods, kernel, cut, dtype)
        V[:, 1:], Mg[:, 1:] = np.cumsum(term, axis=1), np.cumsum(mag, axis=1)
    return V, Mg


def lse(x, axis=0):
    """log sum exp along `axis` in x's own arithmetic, the maximum taken out first."""
    m = x.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def scan(packed, lo, step, bins, checkpoints, a1, a2, periods=None, kernel="gaussian", cut=CUT, dtype=np.float64):
    """(lse [M, 2], V_H [G], bound_V [M]: the largest rounding bound of V_{k_j} over the grid) in `dtype`."""
    t = np.dtype(dtype).type
    V, Mg = grid_prefix(packed, lo, step, bins, periods, kernel, cut, dtype)
    ck = np.asarray(checkpoints, np.int64)
    d = len(bins)
    out = np.stack([lse(t(a1) * V[:, ck], axis=0), lse(t(a2) * V[:, ck], axis=0)], axis=1)
    bound_v = (bound_factor(d, ck)[None, :] * Mg[:, ck].astype(np.float64)).max(axis=0)
    return out, V[:, -1], bound_v


def lse_brute(packed, lo, step, bins, k, a, periods=None, kernel="gaussian", cut=CUT):
    """log sum_g exp(a V_k(g)) with nothing clever: longdouble, the bare sum (the caller keeps a V_k small)."""
    V, _ = grid_prefix(packed, lo, step, bins, periods, kernel, cut, np.longdouble)
    return np.log(np.exp(np.longdouble(a) * V[:, k]).sum())


def exponents(kT: float, bias_factor=None) -> tuple[float, float]:
    """(a1, a2): gamma / ((gamma - 1) kT), 1 / ((gamma - 1) kT); without tempering 1 / kT, 0."""
    if bias_factor is None or not bias_factor > 1:
        return 1.0 / kT, 0.0
    g = float(bias_factor)
    return g / ((g - 1.0) * kT), 1.0 / ((g - 1.0) * kT)


def checkpoints(H: int, stride: int = 1) -> np.ndarray:
    return np.arange(0, H + 1, stride, dtype=np.int32)


def tiwary_log_weights(cv, frame_counts, packed, lo, step, bins, kT, bias_factor=None, stride=1, periods=None,
                       kernel="gaussian", cut=CUT, dtype=np.float64):
    """(log w [n] unnormalised, c [M], V [n]): log w_n = (V(s_n, t_n) - c(t_n)) / kT with c evaluated every `stride`
    hills and held between evaluations: a frame that sees k hills uses c at checkpoint (k // stride) * stride."""
    t = np.dtype(dtype).type
    a1, a2 = exponents(kT, bias_factor)
    ck = checkpoints(np.asarray(packed).shape[0], stride)
    L, _vh, _b = scan(packed, lo, step, bins, ck, a1, a2, periods, kernel, cut, dtype)
    c = t(kT) * (L[:, 0] - L[:, 1])
    V = bias(cv, packed, frame_counts, periods, kernel, cut, dtype)["bias"]
    k = np.asarray(frame_counts, np.int64) // stride
    return (V - c[k]) / t(kT), c, V


def normalise(logw):
    """(weights summing to 1, normalised log-weights, Kish effective sample size)."""
    lw = logw - lse(logw)
    w = np.exp(lw)
    return w, lw, float(1.0 / np.sum(w * w))
