"""The centre side of the k-means filter (filter_stage_build, pmarlo_amd/csrc/kmeans_filter.h) restated in numpy:
what a launch puts into its LDS tables for a centre table c [k, d] and the frames' scale exponent e_x, and which
branch of the fp16 split every coordinate takes.  The tests use it to make sure that the centres they hand the kernel
reach every branch, and that the table's scale sits where they mean it to."""

from __future__ import annotations

import numpy as np

KAPPA = 52.0 * 2.0 ** -24
F16_MIN = 2.0 ** -14
SCALED_HI = 2.0 ** 14
HI = 1e18
SCALE_TOP = 13
UP20 = 1.0 + 2.0 ** -20

# branches of f16_split2 for one scaled coordinate
EXACT, NEEDS_LO, LO_LEFT_OUT, WHOLE_LEFT_OUT, ZERO = range(5)


def scale_exp(amax: float) -> int:
    """filter_scale_exp: e with amax 2^e in [2^12, 2^13); 0 for a zero or non-finite bound; clamped to +-60."""
    if not (amax > 0.0) or not np.isfinite(amax):
        return 0
    q = int(np.floor(np.log2(amax))) + 1
    while np.ldexp(1.0, q) <= amax:          # log2 rounds: settle q exactly (amax = m 2^q, m in [0.5, 1))
        q += 1
    while np.ldexp(1.0, q - 1) > amax:
        q -= 1
    return int(np.clip(SCALE_TOP - q, -60, 60))


def f16_round(v: np.ndarray) -> np.ndarray:
    """Nearest fp16 number (normal range), ties to even: numpy's float16 conversion of a value that is first made
    exactly representable in fp32 would round twice, so round at 11 significant bits directly."""
    v = np.asarray(v, np.float64)
    m, q = np.frexp(v)
    return np.ldexp(np.rint(np.ldexp(m, 11)), q - 11)


def split_branches(w: np.ndarray) -> np.ndarray:
    """Branch of f16_split2 per scaled coordinate w (finite, |w| <= 2^14)."""
    w = np.asarray(w, np.float64)
    a = np.abs(w)
    hi = np.where(a >= F16_MIN, f16_round(np.where(a >= F16_MIN, w, 1.0)), 0.0)
    r = np.abs(w - hi)
    out = np.full(w.shape, NEEDS_LO, np.int64)
    out[(a >= F16_MIN) & (r == 0.0)] = EXACT
    out[(a >= F16_MIN) & (r > 0.0) & (r < F16_MIN)] = LO_LEFT_OUT
    out[(a < F16_MIN) & (a > 0.0)] = WHOLE_LEFT_OUT
    out[a == 0.0] = ZERO
    return out


def centre_tables(c: np.ndarray, e_x: int = 0) -> dict:
    """e_c, any_bad, and per centre: h_j (the ascending-feature fma chain cannot be restated in numpy without an fma:
    here the plain sum of squares, for magnitudes only), the left-out sum `tiny`, |c'_j|, the kappa slot's lower limit
    kappa |c'_j| + 2 tiny (the kernel rounds it up by at most 2^-20 and to the next fp16 number) and the split branches."""
    c = np.asarray(c, np.float64)
    finite = np.abs(c) <= HI                                  # False for NaN
    amax = float(np.max(np.abs(c[np.isfinite(c)]), initial=0.0))
    e_c = scale_exp(amax)
    w = np.ldexp(np.where(np.isfinite(c), c, 0.0), e_c)
    ok_rows = np.all(finite & (np.abs(w) <= SCALED_HI), axis=1)
    br = split_branches(np.where(ok_rows[:, None], w, 0.0))
    a = np.abs(w)
    hi = np.where(a >= F16_MIN, f16_round(np.where(a >= F16_MIN, w, 1.0)), 0.0)
    r = np.abs(w - hi)
    left = np.where(a < F16_MIN, a, np.where(r < F16_MIN, r, 0.0))
    tiny = left.sum(axis=1)
    cnorm = np.sqrt((w * w).sum(axis=1))
    with np.errstate(over="ignore", invalid="ignore"):
        h = 0.5 * (c * c).sum(axis=1)
        cval = np.ldexp(-(h - KAPPA * h), e_x + e_c)
    ok_rows &= np.abs(cval) <= 2.0 ** 100
    return {"e_c": e_c, "any_bad": bool(not ok_rows.all()), "ok_rows": ok_rows, "h": h, "tiny": tiny, "cnorm": cnorm,
            "kappa_slot_min": np.maximum(KAPPA * cnorm + 2.0 * tiny, F16_MIN), "branches": br, "scaled": w}
