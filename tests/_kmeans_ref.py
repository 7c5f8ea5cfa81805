"""The dispatch rule of the k-means passes restated, a shape table built from it, and adversarial inputs (test
infrastructure only).

`dispatch` restates which kernel `dispatch_mfma` / `launch_mfma` (pmarlo_amd/csrc/kmeans.hip) run for a shape: the
fp16 filter, or the instantiation <T, KS, NF, kMT, ACCUM, FOLD, MULTI> of `kmeans_mfma_kernel` with its tile size,
accumulator placement and grid.  The GPU tests compare it with the library's MSM_KMEANS_DEBUG lines, so that the table
provably launches what it names.  The generators build inputs on which a subtly wrong arg-min shows: exact ties placed
where the two winner-recovery routines treat indices differently, near ties, non-finite values, heavy cancellation and
whitening over twelve orders of magnitude."""

from __future__ import annotations

import functools

import numpy as np

# ---------------------------------------------------------------------------------------------------------------
# the dispatch rule (dispatch_mfma, launch_mfma, filter_fits, filter_lds_bytes)
# ---------------------------------------------------------------------------------------------------------------
KS_LADDER = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)     # k-steps of 4 features: the first KS with d <= 4 KS
D_MAX = 4 * KS_LADDER[-1]
LDS_BUDGET = 150 * 1024                                    # centre tile + half-norms (+ LDS accumulators)
LDS_ACC_LIMIT = 64 * 1024                                  # member sums in LDS while k (d + 1) * 8 <= this
FILTER_MAX_D = 10
FILTER_LDS_CAP = 160 * 1024 - 64
N_CU = 256
DTYPES = {"f32": np.float32, "f64": np.float64}


def filter_lds_bytes(k: int, d: int, accum: bool) -> int:
    """LDS of the fp16 filter kernel, 0 when the shape does not fit it."""
    if d > FILTER_MAX_D:
        return 0
    k16 = (k + 15) & ~15
    n_tiles = ((k16 // 16) + 1) & ~1
    row_floats = 8 if d <= 4 else 12
    tile_bytes = 1024 + 16 * row_floats * 4 + 16 * 4 + 16 * 8
    total = n_tiles * tile_bytes + (k * (d + 1) * 8 if accum else 0)
    return total if total <= FILTER_LDS_CAP else 0


def ks_for(d: int) -> int | None:
    return next((ks for ks in KS_LADDER if d <= 4 * ks), None)


def tile_bytes(ks: int) -> int:
    return (64 * ks + 1 + 16) * 8                          # 16 centres: coordinates, one padding double, half-norms


def single_tile_capacity(ks: int, acc_bytes: int = 0) -> int:
    return (LDS_BUDGET - acc_bytes) // tile_bytes(ks) * 16


def dispatch(dtype: str, n: int, d: int, k: int, accumulate: bool, filter_on: bool = True, n_cu: int = N_CU) -> dict:
    """What one assign (accumulate=False) or accumulate launch runs.  dtype: 'f32' / 'f64'."""
    assert dtype in DTYPES and n >= 1 and d >= 1 and k >= 1
    if filter_on and d <= FILTER_MAX_D and filter_lds_bytes(k, d, accumulate):
        return {"kernel": "filter", "T": dtype, "n": n, "d": d, "k": k, "ACCUM": int(accumulate)}
    ks = ks_for(d)
    if ks is None:
        return {"kernel": "unsupported"}
    nf = 2 if ks <= 16 else 1
    mt = 1024 if ks <= 4 else 512
    acc_bytes = k * (d + 1) * 8 if accumulate else 0
    lds_acc = int(accumulate and acc_bytes <= LDS_ACC_LIMIT)
    budget = LDS_BUDGET - (acc_bytes if lds_acc else 0)
    tile_k = budget // tile_bytes(ks) * 16
    k16 = (k + 15) & ~15
    tile_k = max(min(tile_k, k16), 16)
    if tile_k < k16 and tile_k >= 32:
        tile_k &= ~31                                      # chunked: an even number of tiles per chunk
    multi = k > tile_k
    lds = tile_k // 16 * tile_bytes(ks) + (acc_bytes if lds_acc else 0)
    n_units = -(-n // (16 * nf))
    waves = mt // 64
    grid = min(-(-n_units // waves), n_cu)
    chunks = -(-k // tile_k)
    last = k - (chunks - 1) * tile_k
    return {"kernel": "fp64", "T": dtype, "n": n, "d": d, "k": k, "KS": ks, "NF": nf, "MT": mt, "ACCUM": int(accumulate),
            "FOLD": int(d % 4 != 0), "MULTI": int(multi), "tile_k": tile_k, "lds_acc": lds_acc, "grid": grid, "lds": lds,
            "chunks": chunks, "last_tiles": (last + 15) // 16, "tiles": (min(k, tile_k) + 15) // 16,
            "recovery": "global" if multi or ks > 8 else "lds", "prefetch": 4 < ks <= 16, "loop": "narrow" if ks <= 4 else "wide",
            "n_units": n_units, "waves": waves, "units_per_block": -(-n_units // grid)}


def debug_line(path: dict) -> str:
    """The MSM_KMEANS_DEBUG line of a launch that takes `path`."""
    if path["kernel"] == "filter":
        return "msm_kmeans: filter T={T} n={n} d={d} k={k} ACCUM={ACCUM}".format(**path)
    return ("msm_kmeans: fp64 T={T} n={n} d={d} k={k} KS={KS} NF={NF} MT={MT} ACCUM={ACCUM} FOLD={FOLD} MULTI={MULTI} "
            "tile_k={tile_k} lds_acc={lds_acc} grid={grid} lds={lds}").format(**path)


def debug_lines(text: str) -> list[str]:
    return [ln.strip() for ln in text.splitlines() if ln.startswith("msm_kmeans: ")]


def instantiation(path: dict) -> tuple:
    return (path["T"], path["KS"], path["ACCUM"], path["FOLD"], path["MULTI"])


def grid_n(kind: tuple, ks: int, n_cu: int) -> int:
    """n of the rows whose frame count depends on the CU count:
    ('round_up', m): n_units = n_cu * waves * m + 1, so units_per_block rounds up and trailing workgroups are idle;
    ('strides', m):  n_units = n_cu * waves * m + 5 and a ragged last group (static stride of the chunked kernel)."""
    nf = 2 if ks <= 16 else 1
    waves = (1024 if ks <= 4 else 512) // 64
    what, m = kind
    if what == "round_up":
        return 16 * nf * (n_cu * waves * m) + 1
    return 16 * nf * (n_cu * waves * m + 4) + 3


@functools.lru_cache(maxsize=None)
def reachable_accumulate(ks: int, fold: int, multi: int, lds_acc: int):
    """(d, k, filter_on) of the cheapest accumulate shape with this (KS, FOLD, MULTI, lds_acc), or None: a scan of
    every d of the KS step and every k up to twice the single-tile capacity, with the filter on and off (the first
    k >= 37 where there is one)."""
    lo = 4 * KS_LADDER[KS_LADDER.index(ks) - 1] + 1 if ks > 1 else 1
    best = None
    for filter_on in (True, False):
        for d in range(lo, 4 * ks + 1):
            if int(d % 4 != 0) != fold:
                continue
            k_hi = 2 * single_tile_capacity(ks) + 64
            first = None
            for k in range(1, k_hi):
                p = dispatch("f64", 1000, d, k, True, filter_on)
                if p["kernel"] == "fp64" and (p["MULTI"], p["lds_acc"]) == (multi, lds_acc):
                    first = k if first is None or k >= 37 else first
                    if k >= 37:                                         # a few tiles rather than k = 1, where there is a choice
                        break
            if first is not None and (best is None or d * first < best[0] * best[1]):
                best = (d, first, filter_on)
        if best is not None:
            return best
    return None


UNREACHABLE_REASON = ("member sums in LDS need k (d + 1) * 8 <= 64 KiB; for every d of this KS step with this FOLD the "
                      ">= 86 KiB left of the tile budget hold all of those k centres in one chunk")


# ---------------------------------------------------------------------------------------------------------------
# the shape table
# ---------------------------------------------------------------------------------------------------------------
def _row(name, dtype, n, d, k, accum=False, filter_on=True, gens=("smooth", "white", "ties", "near"), **kw):
    r = {"name": name, "dtype": dtype, "n": n, "d": d, "k": k, "accum": accum, "filter_on": filter_on, "gens": gens}
    r.update(kw)
    return r


def row_n(row: dict, n_cu: int = N_CU) -> int:
    return grid_n(row["n"], ks_for(row["d"]), n_cu) if isinstance(row["n"], tuple) else row["n"]


def row_path(row: dict, n_cu: int = N_CU, accumulate: bool | None = None) -> dict:
    acc = row["accum"] if accumulate is None else accumulate
    return dispatch(row["dtype"], row_n(row, n_cu), row["d"], row["k"], acc, row["filter_on"], n_cu)


_SMALL_K = {4: 43, 6: 81, 8: 7, 12: 100, 16: 1, 24: 29, 32: 15, 48: 61, 64: 13}


def _assign_rows() -> list[dict]:
    rows = []
    for i, ks in enumerate(KS_LADDER):
        prev = KS_LADDER[i - 1] if i else 0
        cap = single_tile_capacity(ks)
        tkm = cap & ~31 if cap >= 32 else cap                       # tile_k of a chunked launch
        d0, d1, d1m = 4 * ks, 4 * prev + 1, 4 * ks - 1
        # FOLD single: small k where the filter does not take the shape, else just above the filter's capacity
        k1 = _SMALL_K.get(ks, cap - 16 - 3)
        last_tiles = (1, 3, 2)[i % 3]
        km = (2 if ks >= 16 else 1) * tkm + 16 * last_tiles - 5      # FOLD chunked: a ragged last chunk of 1 / 3 / 2 tiles
        if km <= cap:
            km += tkm
        for j, dt in enumerate(("f32", "f64")):
            n = 600 + 97 * i + 41 * j
            rows.append(_row(f"a_ks{ks}_d{d0}_k{cap}_{dt}", dt, n, d0, cap))            # k = tile_k: the last single tile
            rows.append(_row(f"a_ks{ks}_d{d0}_k{cap + 1}_{dt}", dt, n + 5, d0, cap + 1))  # tile_k + 1: the first chunked
            rows.append(_row(f"a_ks{ks}_d{d1}_k{k1}_{dt}", dt, n + 11, d1, k1))
            rows.append(_row(f"a_ks{ks}_d{d1m}_k{km}_{dt}", dt, n + 18, d1m, km))
    # n at the edges of the frame-group hand-out: a prefetch KS (6, NF = 2) and one without (24, NF = 1)
    for d, k in ((21, 20), (96, 37)):
        for n in (1, 15, 16, 17, 31, 32, 33):
            rows.append(_row(f"a_edge_d{d}_n{n}", "f64" if n % 2 else "f32", n, d, k, gens=("smooth", "white")))
    rows.append(_row("a_ks12_k1", "f64", 77, 45, 1, gens=("smooth", "white")))
    rows.append(_row("a_ks16_odd3tiles", "f32", 500, 64, 48 - 7))       # an odd number of tiles, global recovery
    rows.append(_row("a_ks4_odd5tiles", "f64", 500, 16, 80 - 2))        # ... and LDS recovery
    # frame-group hand-out against the grid: n depends on the CU count of the device
    rows.append(_row("a_grid_narrow", "f32", ("round_up", 1), 16, 20, gens=("smooth",)))
    rows.append(_row("a_grid_wide", "f64", ("round_up", 1), 24, 20, gens=("smooth",)))
    rows.append(_row("a_grid_chunked", "f32", ("strides", 2), 256, single_tile_capacity(64) + 1, gens=("smooth",)))
    return rows


def _accumulate_rows() -> tuple[list[dict], list[tuple]]:
    rows, unreachable = [], []
    for i, ks in enumerate(KS_LADDER):
        for fold in (0, 1):
            for multi in (0, 1):
                for lds_acc in (0, 1):
                    hit = reachable_accumulate(ks, fold, multi, lds_acc)
                    if hit is None:
                        unreachable.append((ks, fold, multi, lds_acc))
                        continue
                    d, k, filter_on = hit
                    if not filter_on:
                        continue                                        # d <= 10 at small k: rows of the filter-off child
                    n = max(k + 200 + 13 * i, 700)
                    first = ("f32", "f64")[(i + fold + multi + lds_acc) % 2]
                    rows.append(_row(f"f_ks{ks}_d{d}_k{k}_m{multi}_l{lds_acc}", first, n, d, k, accum=True))
    # k (d + 1) = 8192 and the next k
    for d, k in ((15, 512), (15, 513), (127, 64), (127, 65), (255, 32), (255, 33)):
        rows.append(_row(f"f_edge_d{d}_k{k}", "f64", k + 300, d, k, accum=True))
    return rows, unreachable


def _child_rows() -> list[dict]:
    """d <= 10 with the filter switched off (one child process): KS = 1, 2, 3 in the single-tile form at small k."""
    rows = []
    for d, k in ((1, 1), (2, 7), (3, 20), (4, 43), (4, 100), (5, 33), (7, 250), (8, 16), (9, 81), (10, 500), (10, 1457)):
        for j, dt in enumerate(("f32", "f64")):
            rows.append(_row(f"c_d{d}_k{k}_{dt}", dt, 700 + 31 * d + j, d, k, filter_on=False,
                             gens=("smooth", "white", "ties", "near") + (("nonfinite",) if d in (4, 10) and k >= 43 else ())))
    for d, k in ((3, 30), (4, 300), (6, 100), (10, 500)):
        rows.append(_row(f"cf_d{d}_k{k}", "f64" if d % 2 else "f32", k + 900, d, k, accum=True, filter_on=False))
    return rows


ASSIGN_ROWS = _assign_rows()
ACCUM_ROWS, UNREACHABLE_ACCUM = _accumulate_rows()
CHILD_ROWS = _child_rows()
# adversarial assign shapes: LDS recovery (KS <= 8, one tile), global recovery in one tile (KS > 8), chunked
ADVERSARIAL_SHAPES = {"lds": (4000, 29, 200), "global": (3000, 100, 120), "multi": (3000, 45, 500)}
CANCELLATION_SHAPES = ((6000, 45, 200), (3000, 100, 150), (1500, 256, 100))


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def smooth(n: int, d: int, k: int, dtype, seed: int):
    """The suite's usual input: a correlated series, centres drawn from it plus noise, and a whitening."""
    from tests import _gen

    rng = np.random.default_rng(seed)
    X = _gen.correlated_series(n, d, seed=seed).astype(dtype)
    centers = X[rng.choice(n, size=k, replace=k > n)].astype(np.float64) + 1e-3 * rng.normal(size=(k, d))
    return X, centers, X.mean(axis=0, dtype=np.float64), X.std(axis=0, dtype=np.float64) + 0.5


def placements(k: int, tile_k: int) -> list[tuple[str, int, int]]:
    """(name, lo, hi) index pairs, lo < hi, at the places where the tile loop and the recoveries order candidates
    differently.  A wave's result register r of lane (g, j) holds centre row g + 4 r of the tile."""
    tile_k = min(tile_k, (k + 15) & ~15)
    chunks = -(-k // tile_k)
    n_tiles = (min(k, tile_k) + 15) // 16                 # tiles of the first chunk
    want = [("same_lane", 1, 5), ("other_lane", 2, 3), ("pair_ab", 6, 16 + 6), ("pair_ab_rows", 7, 16 + 9),
            ("two_pairs", 8, 32 + 8)]
    if chunks == 1 and n_tiles % 2 == 1 and n_tiles >= 3:
        last = 16 * (n_tiles - 1)
        want += [("odd_last_tile", last, last + 1), ("into_odd_last_tile", 10, last + 2)]
    if chunks > 1:
        start = (chunks - 1) * tile_k
        want += [("two_chunks", 13, tile_k + 13), ("first_last_chunk", 14, start), ("in_last_chunk", start + 1, k - 2)]
        lt = (k - start + 15) // 16
        if lt % 2 == 1 and lt >= 3:
            want.append(("odd_last_tile", start + 16 * (lt - 1), start + 16 * (lt - 1) + 1))
    want.append(("k_minus_1", 11 if k > 12 else 0, k - 1))
    used, out = set(), []
    for name, lo, hi in want:
        if 0 <= lo < hi < k and lo not in used and hi not in used:
            used |= {lo, hi}
            out.append((name, lo, hi))
    return out


def ties(n: int, d: int, k: int, tile_k: int, dtype, seed: int):
    """Generator 1: duplicated centres at `placements`, frames on the duplicated centres (exact ties) and around them."""
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(k, d)).astype(dtype).astype(np.float64)      # representable in the frames' type
    pl = placements(k, tile_k)
    for _, lo, hi in pl:
        centers[hi] = centers[lo]
    X = rng.normal(size=(n, d))
    if pl:
        m = max(n // 2, min(n, len(pl)))
        idx = np.asarray([lo for _, lo, _ in pl])[np.arange(m) % len(pl)]
        X[:m] = centers[idx]
        far = np.arange(m) >= 2 * len(pl)                                  # beyond two exact copies: a little off the centre
        X[:m][far] += 1e-3 * rng.normal(size=(int(far.sum()), d))
    X = X[rng.permutation(n)] if n > 1 else X
    return X.astype(dtype), centers, pl


def near(n: int, d: int, k: int, tile_k: int, dtype, seed: int):
    """Generator 2: centre pairs one ulp to 2^-20 apart in one coordinate, frames on their midpoints and on them."""
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(k, d)) + 3.0 * rng.choice([-1.0, 1.0], size=(k, d))      # no coordinate near zero
    pl = placements(k, tile_k)
    for q, (_, lo, hi) in enumerate(pl):
        f = int(rng.integers(0, d))
        eps = np.ldexp(1.0, -(52, 45, 36, 28, 20)[q % 5]) * (1.0 if q % 2 else -1.0)
        centers[hi] = centers[lo]
        centers[hi, f] = centers[lo, f] * (1.0 + eps)
        assert centers[hi, f] != centers[lo, f]
    X = rng.normal(size=(n, d)) * 3.0
    if pl:
        m = max(n // 2, min(n, len(pl)))
        j = np.arange(m)
        lo = np.asarray([p[1] for p in pl])[j % len(pl)]
        hi = np.asarray([p[2] for p in pl])[j % len(pl)]
        kind = (j // len(pl)) % 3
        X[:m] = np.where((kind == 0)[:, None], 0.5 * (centers[lo] + centers[hi]),
                         np.where((kind == 1)[:, None], centers[lo], centers[hi]))
    X = X[rng.permutation(n)] if n > 1 else X
    return X.astype(dtype), centers, pl


def nonfinite(n: int, d: int, k: int, dtype, seed: int) -> list[tuple[np.ndarray, np.ndarray]]:
    """Generator 3: (X, centres) pairs with NaN / inf / huge / tiny / zero frames and centres.  Assign only."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    f = lambda i: i % d                                                   # noqa: E731
    X[10, f(2)] = np.nan
    X[11] = np.nan
    X[12, f(0)] = np.inf
    X[13, f(5)] = -np.inf
    X[14] = 1e200 if dtype == np.float64 else 3e38
    X[15, f(1)] = 1e19
    X[16] = 1e-300 if dtype == np.float64 else 1e-45
    X[17, f(3)] = 3e-15
    X[18] = 0.0
    X[19, f(4)] = 0.0
    X[20] = -1e200 if dtype == np.float64 else -3e38
    X[21, f(7)] = 1e200 if dtype == np.float64 else 3e38
    X = X.astype(dtype)
    base = rng.normal(size=(k, d))
    out = [(X, base)]
    c = base.copy()
    c[k // 3, f(1)] = np.nan                                              # a NaN centre
    out.append((X, c))
    c = base.copy()
    c[0, f(0)] = np.inf                                                   # an inf centre at index 0 and one further on
    c[k // 2] = -np.inf
    out.append((X, c))
    c = base.copy()
    c[k // 4] = 0.0                                                       # a zero centre, tiny centres
    c[k // 5, f(1)] = 1e-300
    out.append((X, c))
    c = base.copy()
    big = np.arange(k) % 7 == 3
    c[big] *= 1e160                                                       # |c|^2 = inf; with the 1e200 frame the dot overflows too
    c[(np.arange(k) % 7 == 5)] *= 1e120                                   # dot with 1e200 overflows, |c|^2 does not: ties at -inf
    out.append((X, c))
    return out


def cancellation(n: int, d: int, k: int, dtype, seed: int):
    """Generator 4: data at 1000 +- 0.01: x.c and |c|^2 / 2 cancel to 1e-7 of their size."""
    rng = np.random.default_rng(seed)
    X = (1000.0 + rng.normal(size=(n, d)) * 0.01).astype(dtype)
    centers = X[rng.choice(n, size=k, replace=False)].astype(np.float64) + 1e-5 * rng.normal(size=(k, d))
    return X, centers


def whitening(n: int, d: int, k: int, dtype, seed: int):
    """Generator 5: a large mean and per-feature std over 1e-6 .. 1e6; centres live in the whitened space."""
    rng = np.random.default_rng(seed)
    std = np.logspace(-6, 6, d)[rng.permutation(d)]
    mean = 1e3 * (1.0 + rng.random(d)) * rng.choice([-1.0, 1.0], size=d)
    X = (mean + std * rng.normal(size=(n, d))).astype(dtype)
    Z = (X.astype(np.float64) - mean) / std
    centers = Z[rng.choice(n, size=k, replace=False)] * (1.0 + 1e-6 * rng.normal(size=(k, d)))
    return X, centers, mean, std


# ---------------------------------------------------------------------------------------------------------------
# conditions on the generators (oracle only)
# ---------------------------------------------------------------------------------------------------------------
def tied_frames(X, centers):
    """Frames with an exact tie at the minimum: the oracle's label under the centres and under the reversed centres
    do not map to each other.  -> (mask, labels, labels under the reversed order mapped back)."""
    from oracle import cport

    X64 = np.asarray(X, np.float64)
    k = centers.shape[0]
    fwd = cport.kmeans_assign(X64, centers)
    rev = k - 1 - cport.kmeans_assign(X64, centers[::-1])
    return fwd != rev, fwd, rev


def placement_tie_counts(X, centers, pl) -> dict:
    tied, fwd, rev = tied_frames(X, centers)
    out = {name: int(np.sum(tied & (fwd == lo) & (rev == hi))) for name, lo, hi in pl}
    out["_tied"] = int(tied.sum())
    out["_n"] = int(tied.size)
    return out


def near_tie_fraction(X, centers, limit: float = 1e-12, sample: int = 400) -> float:
    """Share of (a subsample of) the frames whose two smallest oracle distances |c|^2 - 2 z.c differ by less than
    `limit` relative."""
    X64 = np.asarray(X, np.float64)[:: max(1, X.shape[0] // sample)]
    if centers.shape[0] < 2:
        return 0.0
    D = (centers ** 2).sum(1)[None, :] - 2.0 * X64 @ centers.T
    two = np.partition(D, 1, axis=1)[:, :2]
    rel = (two[:, 1] - two[:, 0]) / np.maximum(np.abs(two[:, 0]), 1e-300)
    return float(np.mean(rel < limit))


# ---------------------------------------------------------------------------------------------------------------
# the engine's Lloyd pass restated with the oracle's assignment (integer member sums: exact)
# ---------------------------------------------------------------------------------------------------------------
def stratified_frames(n: int, k: int, seed: int) -> np.ndarray:
    """The frames msm_kmeans_fit draws its initial centres from: floor((j + u_j) n / k), u_j = splitmix64(seed, j)."""
    m = (1 << 64) - 1
    out = np.empty(k, np.int64)
    for j in range(k):
        h = (seed + 0x9E3779B97F4A7C15 * (j + 1)) & m
        h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & m
        h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & m
        h ^= h >> 31
        u = float(h >> 11) * (1.0 / 9007199254740992.0)
        out[j] = min(int((float(j) + u) * (float(n) / float(k))), n - 1)
    return out


def member_sums(X64: np.ndarray, centers: np.ndarray, scale: float):
    """labels, fixed-point member sums [k, d] and counts [k] of one pass, and the centres after the update."""
    from oracle import cport

    k, d = centers.shape
    lab = cport.kmeans_assign(X64, centers)
    fx = np.rint(X64 * scale).astype(np.int64)
    sums = np.zeros((k, d), np.int64)
    np.add.at(sums, lab, fx)
    counts = np.bincount(lab, minlength=k).astype(np.int64)
    new = centers.copy()
    nz = counts > 0
    new[nz] = sums[nz].astype(np.float64) * (1.0 / scale) / counts[nz, None].astype(np.float64)
    return lab, sums, counts, new
