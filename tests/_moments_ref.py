"""Host-only companions of tests/test_gpu_moments_paths.py (numpy, no GPU).

exact_project / exact_column_sums /    the operations of csrc/moments.hip as plain slicing: the fused standardise +
finalize / standardise / minmax        project, the raw column sums, the two kernels that turn the sums into mean / std
                                       and mean / scale (rational arithmetic, rounded once), the finite minima / maxima
project_data / moments_data            data for which every product and every partial sum is an exact fp64 number, so a
                                       correct kernel is BIT-equal to the reference in any summation order; each
                                       generator asserts that condition itself
project_path / moments_path            the launch rule of moments.hip restated (project_impl and the structure inside
                                       project_mfma_kernel / project_kernel; pick_tf and the block split)
CASES                                  the table the GPU test runs; each row names the branch it is there to reach, and
                                       tests/test_moments_reference.py proves with the rule that it does

The constants below restate moments.hip; a change there has to be made here too (the CPU test compares the table with
the rule, the GPU test compares the results that depend on it)."""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

K_THREADS = 256          # kThreads
PROJ_FRAMES = 64         # kProjFrames: frames per tile of the generic kernel
PROJ_FT = 64             # kProjFT: its feature chunk
P_CHUNK = 64             # kPChunk: features per pipelined chunk of the vector matrix-core kernel
MFMA_FRAMES = 16         # frames per wave group of the matrix-core kernels
MFMA_MAX_D = 16
LDS_DEFAULT = 48 * 1024  # the W' image has to fit it; the generic kernel opts in beyond it
GENERIC_WG_PER_CU = 8
MOMENTS_WG_PER_CU = 4
MOMENTS_ROWS_PER_THREAD = 16
MINMAX_WG_PER_CU = 8
MINMAX_MAX_F = 4096
SENTINEL = 2.0 ** 100    # finite, exact in fp32 and fp64: pad columns of X, W and Y, rows of Y past n, stale absmax
BIG = 2 ** 25 + 1        # not an fp32 number
ITEMSIZE = {"f32": 4, "f64": 8}
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
N_CU_CHECKED = (256, 304, 64)
PER_CU_CHECKED = tuple(range(1, 9))     # at most 8 workgroups of 256 threads fit a compute unit


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def exact_project(X, mu, inv_sigma, m2, W, d: int) -> np.ndarray:
    """Y [n, d] = ((X - mu) * inv_sigma, NaN -> 0, - m2) @ W[:, :d] in fp64.  Exact on project_data; otherwise numpy's
    rounding (the rounding test has its own long-double evaluation)."""
    X = np.asarray(X, np.float64)
    with np.errstate(invalid="ignore"):
        Z = (X - np.asarray(mu, np.float64)[None, :]) * np.asarray(inv_sigma, np.float64)[None, :]
    Z = np.where(np.isnan(X), 0.0, Z)
    if m2 is not None:
        Z = Z - np.asarray(m2, np.float64)[None, :]
    W = np.asarray(W, np.float64)[:, :d]
    Y = np.zeros((X.shape[0], d))
    with np.errstate(invalid="ignore"):
        for f in range(X.shape[1]):          # no BLAS: a matrix product may not keep an inf or a NaN in its own row
            Y += Z[:, f:f + 1] * W[f:f + 1, :]
    return Y


def implicit_shift(X) -> np.ndarray:
    """Row 0 of X with NaN -> 0: the shift the kernel takes when none is given."""
    r0 = np.asarray(X, np.float64)[0]
    return np.where(np.isnan(r0), 0.0, r0)


def exact_column_sums(X, shift=None):
    """([count | S1 | S2] (3F float64), shift) over the non-NaN entries of every column, about `shift` (None: row 0,
    NaN -> 0).  Integers are summed as int64."""
    X = np.asarray(X, np.float64)
    shift = implicit_shift(X) if shift is None else np.asarray(shift, np.float64)
    ok = ~np.isnan(X)
    with np.errstate(invalid="ignore"):
        Z = np.where(ok, X - shift[None, :], 0.0)
    fin = np.isfinite(Z)
    if np.all(fin) and np.all(Z == np.rint(Z)) and np.abs(Z).max(initial=0.0) < 2.0 ** 31:
        Z = Z.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        s1, s2 = Z.sum(axis=0), (Z * Z).sum(axis=0)
    return np.concatenate([ok.sum(axis=0).astype(np.float64), s1.astype(np.float64), s2.astype(np.float64)]), shift


def sqrt_rounded(q: Fraction) -> float:
    """The fp64 number nearest to sqrt(q), q >= 0 rational."""
    if q <= 0:
        return 0.0
    c = math.sqrt(float(q))
    for _ in range(4):
        up, dn = math.nextafter(c, math.inf), math.nextafter(c, -math.inf)
        if ((Fraction(c) + Fraction(up)) / 2) ** 2 < q:
            c = up
        elif ((Fraction(c) + Fraction(dn)) / 2) ** 2 > q:
            c = dn
        else:
            return c
    raise AssertionError("sqrt_rounded did not settle")


def _fr(v) -> Fraction:
    return Fraction(float(v))


def variance(sums, f: int, F: int, denom) -> Fraction:
    """(S2 - S1^2 / cnt) / denom of column f as a rational number."""
    cnt, s1, s2 = _fr(sums[f]), _fr(sums[F + f]), _fr(sums[2 * F + f])
    return (s2 - s1 * s1 / cnt) / Fraction(denom)


def finalize(sums, shift, ddof: int):
    """moments_finalize_kernel -> (mean, std, count), each value the rational result rounded once:
    mean = shift + S1 / cnt, std = sqrt(max((S2 - S1^2 / cnt) / (cnt - ddof), 0)); cnt = 0 -> 0, 0; cnt <= ddof -> NaN."""
    F = len(shift)
    mean, std = np.zeros(F), np.zeros(F)
    for f in range(F):
        cnt = sums[f]
        if not cnt > 0:
            continue
        mean[f] = float(_fr(shift[f]) + _fr(sums[F + f]) / _fr(cnt))
        std[f] = sqrt_rounded(variance(sums, f, F, int(cnt) - ddof)) if cnt - ddof > 0 else np.nan
    return mean, std, np.array(sums[:F], np.float64)


def standardise(sums, shift, n_rows, with_std: bool):
    """standardise_params_kernel -> (mean, scale, inv_scale): scale = sqrt(max((S2 - S1^2 / cnt) / n_rows, 0)), below
    10 eps -> 1, and 1 without with_std or without a single entry."""
    F = len(shift)
    mean, scale = np.zeros(F), np.ones(F)
    for f in range(F):
        if not sums[f] > 0:
            continue
        mean[f] = float(_fr(shift[f]) + _fr(sums[F + f]) / _fr(sums[f]))
        if with_std:
            sd = sqrt_rounded(variance(sums, f, F, int(n_rows)))
            scale[f] = 1.0 if sd < 10.0 * np.finfo(np.float64).eps else sd
    return mean, scale, 1.0 / scale


def std_interval(sums, f: int, F: int, denom):
    """[lo, hi] that holds the device's sqrt of the variance of column f: the three roundings of S1*S1, / cnt and the
    subtraction and the one of the division move the variance by at most 4 * 2^-53 * (S2 + S1^2 / cnt) / denom; the
    square root is monotonic and rounds once more (one ulp on either side)."""
    cnt, s1, s2 = _fr(sums[f]), _fr(sums[F + f]), _fr(sums[2 * F + f])
    var = (s2 - s1 * s1 / cnt) / Fraction(denom)
    err = Fraction(4, 2 ** 53) * (s2 + s1 * s1 / cnt) / Fraction(denom)
    lo, hi = sqrt_rounded(max(var - err, Fraction(0))), sqrt_rounded(var + err)
    return (math.nextafter(lo, -math.inf) if lo > 0 else 0.0), math.nextafter(hi, math.inf)


def minmax(X):
    """(min [F], max [F] over the finite entries, NaN where a column has none; [non-finite entries, finite rows])."""
    X = np.asarray(X, np.float64)
    fin = np.isfinite(X)
    F = X.shape[1]
    mn, mx = np.full(F, np.nan), np.full(F, np.nan)
    for f in range(F):
        col = X[fin[:, f], f]
        if col.size:
            mn[f], mx[f] = col.min(), col.max()
    return mn, mx, np.array([int((~fin).sum()), int(fin.all(axis=1).sum())], np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def dyadic_bits(a) -> int:
    """The smallest g with a * 2^g all integers."""
    a = np.asarray(a, np.float64)
    for g in range(0, 64):
        s = a * 2.0 ** g
        if np.all(s == np.rint(s)):
            return g
    raise AssertionError("not dyadic within 2^-63")


def project_exactness(X, mu, inv_sigma, m2, W, d: int):
    """(g, peak): every intermediate of either kernel -- x - mu, (x - mu) * inv_sigma - m2, inv_sigma * W, m2 * W, each
    product and each partial sum in any order -- is a multiple of 2^-g and at most `peak` in magnitude.  Exact in fp64
    when peak < 2^(53 - g).  NaN entries count as the imputed 0, inf is not allowed."""
    X = np.asarray(X, np.float64)
    assert np.all(np.isfinite(X) | np.isnan(X))
    Xz = np.where(np.isnan(X), np.asarray(mu, np.float64)[None, :], X)
    assert np.all(Xz == np.rint(Xz)) and np.all(mu == np.rint(mu))
    a = np.log2(np.asarray(inv_sigma, np.float64))
    assert np.all(a == np.rint(a)), "inv_sigma has to be a power of two"
    m2 = np.zeros(len(mu)) if m2 is None else np.asarray(m2, np.float64)
    Wd = np.asarray(W, np.float64)[:, :d]
    g = max(dyadic_bits(inv_sigma), dyadic_bits(m2)) + dyadic_bits(Wd)
    assert dyadic_bits(np.asarray(inv_sigma)[:, None] * Wd) <= g and dyadic_bits(m2[:, None] * Wd) <= g
    absz = np.abs(Xz - mu[None, :]) * np.abs(inv_sigma)[None, :]
    peak = ((absz + np.abs(m2)[None, :]) @ np.abs(Wd)).max(initial=0.0)
    peak = max(peak, np.abs(Xz).max(initial=0.0), (absz + np.abs(m2)[None, :]).max(initial=0.0))
    return g, float(peak)


def project_data(row: dict):
    """(X [n, F] float64 holding numbers of the row's dtype, mu, inv_sigma, m2 or None, W [F, ldw]) of a project row:
    integer x and mu, inv_sigma a power of two, W multiples of 1/16, m2 multiples of 1/4.  The pad columns of W hold
    SENTINEL.  Family fp64_only puts +-(2^25 + 1) into a few entries."""
    n, F, d, ldw = row["n"], row["F"], row["d"], row["ldw"]
    rng = np.random.default_rng(row["seed"])
    X = rng.integers(-40, 41, size=(n, F)).astype(np.float64)
    if row["family"] == "fp64_only":
        if row["dtype"] != "f64":
            raise ValueError("the fp64-only family needs fp64 input")
        k = min(max(n, 1) * F, 9)
        idx = rng.choice(n * F, size=min(k, n * F), replace=False)
        X.reshape(-1)[idx] = np.where(np.arange(len(idx)) % 2 == 0, BIG, -BIG)
    mu = rng.integers(-8, 9, size=F).astype(np.float64)
    inv_sigma = 2.0 ** -rng.integers(0, 4, size=F).astype(np.float64)
    if F > 1:
        inv_sigma[F - 1] = 0.125       # never all ones: inv_sigma * W differs from W
    else:
        inv_sigma[0] = 0.5
    m2 = rng.integers(-8, 9, size=F).astype(np.float64) / 4.0 if row["mean2"] else None
    if m2 is not None:
        m2[0] = 1.75
    W = np.full((F, ldw), SENTINEL)
    W[:, :d] = rng.integers(-16, 17, size=(F, d)).astype(np.float64) / 16.0
    W[0, :d] = (np.arange(d) % 7 + 1) / 16.0      # no zero row where m2 is pinned
    g, peak = project_exactness(X, mu, inv_sigma, m2, W, d)
    assert peak < 2.0 ** (53 - g), (row["name"], g, peak)
    assert np.array_equal(X.astype(NP_DTYPE[row["dtype"]]).astype(np.float64), X), row["name"]
    return X, mu, inv_sigma, m2, W


def moments_exactness(X, shift) -> float:
    """The largest column sum of (x - shift)^2 over the non-NaN entries: below 2^53 every partial sum of S1 and S2 is an
    fp64 integer in any order (integers: |z| <= z^2)."""
    X = np.asarray(X, np.float64)
    Z = np.where(np.isnan(X), 0.0, X - np.asarray(shift, np.float64)[None, :])
    assert np.all(Z == np.rint(Z)) and np.abs(Z).max(initial=0.0) < 2.0 ** 31
    Zi = Z.astype(np.int64)
    return float((Zi * Zi).sum(axis=0).max(initial=0))


def moments_data(row: dict):
    """(X [n, F] float64 holding integers of the row's dtype, explicit integer shift or None) of a moments row.
    small: 13 + [-3, 3]; wide: 20000 + [-4095, 4095] (sums pass 2^24 at once); fp64_only: small plus +-(2^25 + 1) in at
    most two rows >= 1 of a column (row 0 may be the shift).  The columns sit away from zero so that the sum S1 / cnt
    the kernels add to the shift is no larger than twice the mean: then the two roundings of shift + S1 / cnt stay
    within 2 ulp of the mean (asserted here; a mean that cancels against its shift has no such bound)."""
    n, F = row["n"], row["F"]
    rng = np.random.default_rng(row["seed"])
    wide = row["family"] == "wide"
    lim, centre = (4095, 20000.0) if wide else (3, 13.0)
    X = centre + rng.integers(-lim, lim + 1, size=(n, F)).astype(np.float64)
    X[:, F // 2] = centre + (np.arange(n) % 5) * (1000.0 if wide else 1.0) - 1.0
    if row["family"] == "fp64_only":
        if row["dtype"] != "f64":
            raise ValueError("the fp64-only family needs fp64 input")
        for q, t in enumerate(rng.choice(np.arange(1, n), size=min(2, n - 1), replace=False)):
            cols = rng.choice(F, size=min(3, F), replace=False)
            X[t, cols] = BIG if q == 0 else -BIG
    shift = centre + rng.integers(-2, 3, size=F).astype(np.float64) * (50.0 if wide else 1.0) if row["shift"] else None
    used = implicit_shift(X) if shift is None else shift
    peak = moments_exactness(X, used)
    assert peak < 2.0 ** 53, (row["name"], peak)
    if row["family"] != "fp64_only":
        assert n * float(np.abs(X - used[None, :]).max()) ** 2 < 2.0 ** 53, row["name"]
    assert np.array_equal(X.astype(NP_DTYPE[row["dtype"]]).astype(np.float64), X), row["name"]
    q = (X - used[None, :]).sum(axis=0) / n
    assert np.all(np.abs(q) <= 2.0 * np.abs(used + q)), row["name"]
    return X, shift


# ---------------------------------------------------------------------------------------------------------------------
# the launch rule
# ---------------------------------------------------------------------------------------------------------------------
def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def project_path(n: int, F: int, d: int, dtype: str, ld: int, base_misalign: int, finite: bool, n_cu: int,
                 per_cu: int) -> dict:
    """What msm_project (finite: msm_project_finite) launches.  base_misalign: elements between an allocation and
    frame 0; per_cu: resident workgroups per compute unit the occupancy query reports for the matrix-core kernel."""
    assert n >= 0 and F >= 1 and 1 <= d <= 64 and ld >= F
    if n == 0:
        return {"kernel": "none"}
    F16 = _ceil_div(F, 16) * 16
    if d <= MFMA_MAX_D and (F16 * 17 + 16) * 8 <= LDS_DEFAULT:
        vec = F % 16 == 0 and ld % 4 == 0 and base_misalign % 4 == 0     # 16 bytes in f32, 32 in f64: 4 elements
        n_groups = _ceil_div(n, MFMA_FRAMES)
        grid = min(_ceil_div(n_groups, 4), n_cu * max(per_cu, 1))
        n_waves = 4 * grid
        return {"kernel": "mfma_vec" if vec else "mfma_scalar", "dtype": dtype, "vec": vec, "finite": vec and finite,
                "lds_opt_in": False, "n_chunks": _ceil_div(F16, P_CHUNK) if vec else 1,
                "dead_q": vec and F16 % P_CHUNK != 0, "pad_features": F16 != F, "tail": n % MFMA_FRAMES != 0,
                "loops": n_groups > n_waves, "grid": grid, "idle_waves": n_waves > n_groups,
                "vec_off_by": None if vec else tuple(k for k, bad in (("F", F % 16 != 0), ("ld", ld % 4 != 0),
                                                                      ("base", base_misalign % 4 != 0)) if bad)}
    lds = (PROJ_FRAMES * (PROJ_FT + 1) + PROJ_FT * d) * 8
    n_tiles = _ceil_div(n, PROJ_FRAMES)
    grid = min(n_tiles, n_cu * GENERIC_WG_PER_CU)
    return {"kernel": "generic", "dtype": dtype, "vec": False, "finite": False, "lds_opt_in": lds > LDS_DEFAULT,
            "n_chunks": _ceil_div(F, PROJ_FT), "dead_q": False, "pad_features": F % PROJ_FT != 0,
            "tail": n % PROJ_FRAMES != 0, "loops": n_tiles > grid, "grid": grid, "idle_waves": False,
            "vec_off_by": None, "wide_F": d <= MFMA_MAX_D}


def pick_tf(F: int) -> int:
    tf = 1
    while tf < F and tf < K_THREADS:
        tf <<= 1
    return tf


def moments_path(n: int, F: int, n_cu: int) -> dict:
    """What msm_column_moments_partial launches: tf lanes across the features, rp = 256 / tf rows per pass, the rows cut
    into blocks of equal length with about 16 rows per thread, at most 4 workgroups per compute unit."""
    assert n >= 1 and F >= 1
    tf = pick_tf(F)
    rp = K_THREADS // tf
    blocks = min(n_cu * MOMENTS_WG_PER_CU, max(1, n // (rp * MOMENTS_ROWS_PER_THREAD)))
    rows_per_block = _ceil_div(n, blocks)
    blocks = _ceil_div(n, rows_per_block)
    last = n - (blocks - 1) * rows_per_block
    return {"tf": tf, "rp": rp, "blocks": blocks, "rows_per_block": rows_per_block,
            "f_passes": _ceil_div(F, tf), "idle_lanes": F % tf != 0, "n_lt_rp": n < rp,
            "unrolled": rows_per_block > 3 * rp,                 # the four-deep loop runs for row slot 0 at least
            "remainder": any(0 < (rows - ry + rp - 1) // rp % 4 for rows in {rows_per_block, last}
                             for ry in range(min(rp, rows))),   # the one-row loop runs after it somewhere
            "ragged": last != rows_per_block,
            "capped": n // (rp * MOMENTS_ROWS_PER_THREAD) >= n_cu * MOMENTS_WG_PER_CU,
            "multi_block": blocks > 1}


def minmax_path(n: int, F: int, n_cu: int) -> dict:
    """What msm_column_minmax launches: one thread per row, at most 8 workgroups per compute unit."""
    if F > MINMAX_MAX_F:
        return {"status": "invalid"}
    if n == 0:
        return {"status": "ok", "grid": 0, "second_row": False, "init_loops": False}
    grid = min(_ceil_div(n, 256), n_cu * MINMAX_WG_PER_CU)
    return {"status": "ok", "grid": grid, "second_row": n > 256 * grid, "init_loops": F > 256}


def covers(got: dict, want: dict) -> list:
    """The entries of a row's `reach` that a path does not deliver (empty: all reached)."""
    return [(k, v, got.get(k)) for k, v in want.items() if got.get(k) != v]


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
CASES: list = []


def _project(name, n, F, d, reach, *, dtype="f32", ld=None, off=0, ldw=None, ldy=None, mean2=True, family="small"):
    assert name not in {r["name"] for r in CASES}, name
    CASES.append({"kind": "project", "name": name, "n": n, "F": F, "d": d, "dtype": dtype, "ld": F if ld is None else ld,
                  "off": off, "ldw": d if ldw is None else ldw, "ldy": d if ldy is None else ldy, "mean2": mean2,
                  "family": family, "reach": reach, "seed": 2000 + len(CASES)})


def _moments(name, n, F, reach, *, dtype="f32", ld=None, shift=False, family="small"):
    assert name not in {r["name"] for r in CASES}, name
    CASES.append({"kind": "moments", "name": name, "n": n, "F": F, "dtype": dtype, "ld": F if ld is None else ld,
                  "shift": shift, "family": family, "reach": reach, "seed": 2000 + len(CASES)})


_N_EDGES = (1, 15, 16, 17, 63, 64, 65)

# -- the vector matrix-core kernel: every frame-count edge, F = 16 .. 352, the tail group, dead q slots ---------------
_q = 0
for _F, _chunks, _dead in ((16, 1, True), (48, 1, True), (64, 1, False), (80, 2, True), (128, 2, False),
                           (352, 6, True)):
    for _n in _N_EDGES if _F in (16, 48, 80) else (17, 64):
        for _dtype in ("f32", "f64"):
            if (_q + _n) % 2 and _F not in (16, 80):        # half of the (n, dtype) pairs of the larger shapes
                _q += 1
                continue
            _h = _q // 2
            _d = (1, 3, 16, 5, 2)[_q % 5]
            _wide = _h % 3 == 1
            _project(f"vec-F{_F}-n{_n}-d{_d}-{_dtype}", _n, _F, _d,
                     {"kernel": "mfma_vec", "n_chunks": _chunks, "dead_q": _dead, "tail": _n % 16 != 0, "loops": False,
                      "lds_opt_in": False}, dtype=_dtype, ld=_F + (4 if _wide else 0),
                     off=(0, 4, 8)[_h % 3] if _wide else 0, ldw=_d + (_h % 2) * 3, ldy=_d + (_h % 4 == 3) * 2,
                     mean2=_h % 4 != 2, family="fp64_only" if _dtype == "f64" and _h % 2 == 0 else "small")
            _q += 1
# several groups per wave slot and several workgroups, with a tail group
for _F, _n, _d, _dtype in ((16, 273, 3, "f32"), (48, 1001, 16, "f64"), (80, 529, 2, "f32"), (128, 333, 7, "f64")):
    _project(f"vec-F{_F}-n{_n}-d{_d}-{_dtype}", _n, _F, _d,
             {"kernel": "mfma_vec", "tail": True, "loops": False}, dtype=_dtype, ld=_F + 8, ldy=_d + 1, ldw=_d + 2,
             family="fp64_only" if _dtype == "f64" else "small")

# -- the scalar matrix-core kernel: vector loads switched off by each condition alone, and F off the tile -------------
_SCALAR = [   # (F, ld, off, what switches the vector loads off)
    (16, 16, 1, ("base",)), (64, 64, 3, ("base",)), (16, 18, 0, ("ld",)), (48, 49, 0, ("ld",)), (128, 130, 0, ("ld",)),
    (1, 4, 0, ("F",)), (1, 1, 0, ("F", "ld")), (15, 16, 0, ("F",)), (17, 20, 0, ("F",)), (100, 100, 4, ("F",)), (351, 352, 0, ("F",)),
    (17, 17, 1, ("F", "ld", "base")),
]
for _i, (_F, _ld, _off, _why) in enumerate(_SCALAR):
    for _j, _dtype in enumerate(("f32", "f64")):
        _n = _N_EDGES[(_i + 3 * _j) % len(_N_EDGES)]
        _d = (3, 1, 16, 4)[(_i + _j) % 4]
        _project(f"scalar-F{_F}-ld{_ld}-off{_off}-n{_n}-d{_d}-{_dtype}", _n, _F, _d,
                 {"kernel": "mfma_scalar", "vec_off_by": _why, "tail": _n % 16 != 0, "loops": False}, dtype=_dtype,
                 ld=_ld, off=_off, ldw=_d + _i % 2, ldy=_d + (_i % 3 == 0), mean2=(_i + _j) % 3 != 0,
                 family="fp64_only" if _dtype == "f64" and _i % 2 else "small")
for _n in _N_EDGES:        # every frame-count edge on one scalar shape, with pad features
    _project(f"scalar-F15-n{_n}-edge", _n, 15, 3, {"kernel": "mfma_scalar", "vec_off_by": ("F",),
                                                  "tail": _n % 16 != 0, "pad_features": True}, dtype="f32", ld=16)
_project("scalar-F50-n309-d9-f64", 309, 50, 9, {"kernel": "mfma_scalar", "tail": True, "loops": False}, dtype="f64",
         ld=53, ldy=12, family="fp64_only")

# -- the generic kernel: d > 16 (default LDS up to d = 31, opt-in from 32), and d <= 16 when W' does not fit 48 KiB ---
_GENERIC = [   # (F, d, opt-in)
    (16, 17, False), (1, 17, False), (64, 30, False), (65, 31, False), (128, 31, False), (70, 32, True), (64, 64, True),
    (17, 64, True), (200, 40, True), (129, 20, False),
]
for _i, (_F, _d, _opt) in enumerate(_GENERIC):
    for _j, _dtype in enumerate(("f32", "f64")):
        _n = _N_EDGES[(2 * _i + 5 * _j) % len(_N_EDGES)]
        _project(f"generic-F{_F}-d{_d}-n{_n}-{_dtype}", _n, _F, _d,
                 {"kernel": "generic", "lds_opt_in": _opt, "tail": _n % 64 != 0, "pad_features": _F % 64 != 0,
                  "n_chunks": -(-_F // 64), "loops": False}, dtype=_dtype, ld=_F + (_i % 3), off=_i % 2,
                 ldw=_d + (_i % 2) * 5, ldy=_d + (_i % 3 == 1) * 3, mean2=(_i + _j) % 3 != 1,
                 family="fp64_only" if _dtype == "f64" and _i % 2 == 0 else "small")
for _n in _N_EDGES:        # every frame-count edge on one generic shape, with a feature tail chunk
    _project(f"generic-F70-d17-n{_n}-edge", _n, 70, 17, {"kernel": "generic", "tail": _n % 64 != 0, "n_chunks": 2,
                                                        "pad_features": True}, dtype="f64" if _n % 2 else "f32")
for _F, _d, _dtype in ((368, 3, "f32"), (368, 16, "f64"), (353, 1, "f64"), (400, 8, "f32")):
    _project(f"generic-wideF-F{_F}-d{_d}-{_dtype}", 131, _F, _d,
             {"kernel": "generic", "wide_F": True, "lds_opt_in": False, "tail": True}, dtype=_dtype, ldy=_d + 1,
             family="fp64_only" if _dtype == "f64" else "small")
_project("vec-F352-n131-d16-f32-largest-image", 131, 352, 16, {"kernel": "mfma_vec", "n_chunks": 6, "dead_q": True},
         dtype="f32")
_project("generic-F70-d20-n1000-f32", 1000, 70, 20, {"kernel": "generic", "tail": True, "loops": False}, dtype="f32",
         ld=72, ldy=21)

# -- a wave (a workgroup of the generic kernel) takes a second group ---------------------------------------------------
# A round of the matrix-core kernels is 16 frames * 4 waves * n_cu * per_cu workgroups, at most 64 * 8 * 304 = 155 648
# frames on the devices checked (8 workgroups of 256 threads are all a compute unit holds); a round of the generic kernel
# is 64 * 8 * n_cu frames.  300 001 frames force a second round (and a tail group) up to 585 compute units, 160 001 up to
# 312.  F = 80: two chunks, so the hand-over to the next group comes after the second chunk of a group, and the last
# chunk has dead q slots.  Should a device be larger than that, loop_is_forced says so and the rows only claim the rest.
_project("vec-second-round-F16", 300_001, 16, 3, {"kernel": "mfma_vec", "loops": True, "tail": True, "n_chunks": 1},
         dtype="f32")
_project("vec-second-round-F80-two-chunks", 160_001, 80, 2,
         {"kernel": "mfma_vec", "loops": True, "tail": True, "n_chunks": 2, "dead_q": True}, dtype="f32")
_project("scalar-second-round-F15", 160_001, 15, 3, {"kernel": "mfma_scalar", "loops": True, "tail": True},
         dtype="f32", ld=16)
_project("generic-second-round-d17", 160_001, 16, 17, {"kernel": "generic", "loops": True, "tail": True}, dtype="f32")

# -- column moments ---------------------------------------------------------------------------------------------------
_MOMENTS = [   # (F, n, what the row is there for)
    (1, 1, {"tf": 1, "rp": 256, "blocks": 1, "n_lt_rp": True}),
    (1, 100, {"tf": 1, "n_lt_rp": True, "unrolled": False}),
    (1, 1030, {"tf": 1, "blocks": 1, "unrolled": True, "remainder": True}),
    (1, 9001, {"tf": 1, "blocks": 2, "ragged": True}),
    (2, 1, {"tf": 2, "rp": 128, "n_lt_rp": True}),
    (2, 127, {"tf": 2, "n_lt_rp": True}),
    (2, 4100, {"tf": 2, "blocks": 2, "unrolled": True}),
    (3, 63, {"tf": 4, "rp": 64, "n_lt_rp": True, "idle_lanes": True}),
    (3, 65, {"tf": 4, "n_lt_rp": False, "blocks": 1}),
    (3, 3077, {"tf": 4, "blocks": 3, "ragged": True}),
    (10, 1000, {"tf": 16, "rp": 16, "blocks": 3, "unrolled": True}),
    (16, 257, {"tf": 16, "blocks": 1, "unrolled": True, "remainder": True}),
    (64, 64, {"tf": 64, "rp": 4, "blocks": 1, "unrolled": True}),
    (255, 1, {"tf": 256, "rp": 1, "idle_lanes": True, "f_passes": 1}),
    (255, 17, {"tf": 256, "blocks": 1, "unrolled": True, "remainder": True}),
    (256, 1, {"tf": 256, "idle_lanes": False, "f_passes": 1}),
    (256, 3, {"tf": 256, "unrolled": False, "remainder": True}),
    (256, 16, {"tf": 256, "blocks": 1, "unrolled": True, "remainder": False}),
    (256, 33, {"tf": 256, "blocks": 2, "ragged": True}),
    (257, 1, {"tf": 256, "f_passes": 2, "idle_lanes": True}),
    (257, 70, {"tf": 256, "f_passes": 2, "blocks": 4, "ragged": True}),
    (513, 1, {"tf": 256, "f_passes": 3}),
    (513, 50, {"tf": 256, "f_passes": 3, "blocks": 3, "ragged": True}),
    (256, 20_001, {"tf": 256, "capped": True, "multi_block": True}),       # 16 * 4 * 304 = 19 456 rows fill every slot
]
for _i, (_F, _n, _reach) in enumerate(_MOMENTS):
    for _j, _dtype in enumerate(("f32", "f64")):
        if _n > 10_000 and _dtype == "f64":
            continue
        _fam = ("small", "wide", "fp64_only")[(_i + _j) % 3] if _dtype == "f64" and _n > 1 else ("small", "wide")[_i % 2]
        _moments(f"moments-F{_F}-n{_n}-{_dtype}", _n, _F, _reach, dtype=_dtype, ld=_F + ((_i + _j) % 2) * 3,
                 shift=(_i + _j) % 3 == 0, family=_fam)


def row_path(row: dict, n_cu: int, per_cu: int = 8, finite: bool = False) -> dict:
    if row["kind"] == "moments":
        return moments_path(row["n"], row["F"], n_cu)
    return project_path(row["n"], row["F"], row["d"], row["dtype"], row["ld"], row["off"], finite, n_cu, per_cu)


def loop_is_forced(row: dict, n_cu: int, per_cu: int) -> bool:
    """Whether a second-round project row makes a wave loop on a device of n_cu units with per_cu resident workgroups
    each; rows that do not name `loops` = True in their reach do not depend on either."""
    if row["kind"] != "project" or row["reach"].get("loops") is not True:
        return True
    if row["reach"]["kernel"] == "generic":
        return row["n"] > PROJ_FRAMES * GENERIC_WG_PER_CU * n_cu
    return row["n"] > MFMA_FRAMES * 4 * n_cu * per_cu


def project_rows():
    return [r for r in CASES if r["kind"] == "project"]


def moments_rows():
    return [r for r in CASES if r["kind"] == "moments"]


def ids(rows):
    return [r["name"] for r in rows]
