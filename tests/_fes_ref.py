"""Host-only companions of tests/test_gpu_fes_paths.py (numpy and fractions, no GPU).

hist2d_path / kde_path / wstats_path /   the launch rules of csrc/fes.hip restated, constants named after the source
flat_path
hist_data / hist_reference               edges, samples with the special values, weights; np.histogram2d for counts and
                                         the exact integer restatement of the 2^e fixed point for weights (a correct
                                         kernel is BIT-equal), plus the true sums with their derived bound
kde_indicator / kde_smooth               frames exactly on centres that are >= 39 bandwidths apart (every Gaussian factor
                                         is exactly 1 or 0, the density an integer times the normaliser), and smooth data
                                         with a long-double reference and a per-cell bound
wstats_exact / wstats_reference          integer samples, dyadic weights, integer mean: all six outputs exact
smooth_reference / finalize_reference /  numpy restatements of the small kernels
clip_reference / wrap_reference / gather_reference
CASES                                    the table the GPU test runs; each row names the branch it is there to reach and
                                         tests/test_fes_reference.py proves with the rules that it does

The constants restate fes.hip; a change there has to be made here too."""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

K_T = 256                        # kT: threads of hist2d_kernel
HIST_LDS_BYTES = 64 * 1024       # kHistLdsBytes: dynamic LDS of hist2d_kernel (edges, then bins)
HIST_FRAMES_PER_THREAD = 8
HIST_WG_PER_CU = 4
HIST_MAX_CELLS = 1 << 24
KDE_BLOCK = 64                   # a workgroup of kde2d_kernel owns 64 x 64 centres
KDE_WAVES = 4
KDE_GROUP = 4                    # frames per matrix instruction
KDE_WG_PER_CU = 2
KDE_MAX_AXIS = 4096
WSTATS_FRAMES_PER_BLOCK = 4096
WSTATS_WG_PER_CU = 2
FLAT_FRAMES_PER_BLOCK = 1024     # clip_or_wrap_kernel / gather_kernel: 256 threads, 4 frames each
FLAT_WG_PER_CU = 8
SINGLE_WG_THREADS = 1024         # scale_to_total, fes_finalize_kernel: one workgroup
N_CU_CHECKED = (256, 304, 64)
LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288")
SENTINEL = -1234.5625


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def resolve(v, n_cu: int) -> int:
    """A frame count of the table: an int, or ("cu", a, b) = a * n_cu + b for the rows sized from the device."""
    if isinstance(v, tuple):
        assert v[0] == "cu"
        return v[1] * n_cu + v[2]
    return int(v)


# ---------------------------------------------------------------------------------------------------------------------
# launch rules
# ---------------------------------------------------------------------------------------------------------------------
def hist2d_path(n: int, nx: int, ny: int, weighted: bool, n_cu: int) -> dict:
    """What msm_hist2d launches."""
    if not (n >= 0 and nx >= 1 and ny >= 1 and nx * ny <= HIST_MAX_CELLS):
        return {"status": "invalid"}
    if n == 0:
        return {"status": "ok", "kernel": "none"}
    cells, edge_bytes = nx * ny, (nx + ny + 2) * 8
    lds_edges = edge_bytes <= HIST_LDS_BYTES
    lds_bins = cells * 8 + edge_bytes <= HIST_LDS_BYTES
    lds = (edge_bytes + (cells * 8 if lds_bins else 0)) if lds_edges else 0
    blocks_wanted = _ceil_div(n, K_T * HIST_FRAMES_PER_THREAD)
    grid = min(blocks_wanted, n_cu * HIST_WG_PER_CU)
    return {"status": "ok", "kernel": "hist2d", "weighted": bool(weighted), "lds_bins": lds_bins, "lds_edges": lds_edges,
            "lds_bytes": lds, "grid": grid, "capped": blocks_wanted > n_cu * HIST_WG_PER_CU,
            "second_round": n > grid * K_T, "rounds": _ceil_div(n, grid * K_T), "idle_lanes": n < grid * K_T,
            "multi_block": grid > 1}


def kde_path(n: int, nx: int, ny: int, n_cu: int) -> dict:
    """What msm_kde2d launches.  c_sum: the longest chain of additions behind one cell (4 frames per instruction and
    iteration, the 4 waves one after the other, then the slabs)."""
    if not (n >= 1 and 1 <= nx <= KDE_MAX_AXIS and 1 <= ny <= KDE_MAX_AXIS):
        return {"status": "invalid"}
    nby, nbz = _ceil_div(nx, KDE_BLOCK), _ceil_div(ny, KDE_BLOCK)
    n_groups = _ceil_div(n, KDE_GROUP)
    gx = max(1, min(_ceil_div(n_groups, KDE_WAVES), max(1, n_cu * KDE_WG_PER_CU // (nby * nbz))))
    iters = _ceil_div(n_groups, gx * KDE_WAVES)
    return {"status": "ok", "nby": nby, "nbz": nbz, "gx": gx, "n_groups": n_groups, "iters": iters,
            "tail_lanes": n - KDE_GROUP * (n_groups - 1), "idle_waves": n_groups < gx * KDE_WAVES,
            "loops": iters > 1, "multi_slab": gx > 1, "blocks": nby * nbz, "clamped": nx % KDE_BLOCK != 0 or ny % KDE_BLOCK != 0,
            "c_sum": KDE_GROUP * iters + (KDE_WAVES - 1) + gx, "slab_bytes": gx * nby * nbz * 4096 * 8}


def wstats_path(n: int, n_cu: int) -> dict:
    """What msm_weighted_stats launches: nb blocks of `per` consecutive frames."""
    assert n >= 1
    nb = min(_ceil_div(n, WSTATS_FRAMES_PER_BLOCK), n_cu * WSTATS_WG_PER_CU)
    per = _ceil_div(n, nb)
    return {"nb": nb, "per": per, "empty_block": (nb - 1) * per >= n, "capped": nb == n_cu * WSTATS_WG_PER_CU,
            "ragged": n % per != 0, "strided_loop": per > SINGLE_WG_THREADS}


def flat_path(n: int, n_cu: int) -> dict:
    """clip_or_wrap_kernel and gather_kernel."""
    if n == 0:
        return {"kernel": "none"}
    blocks = min(max(1, _ceil_div(n, FLAT_FRAMES_PER_BLOCK)), n_cu * FLAT_WG_PER_CU)
    return {"kernel": "flat", "blocks": blocks, "capped": _ceil_div(n, FLAT_FRAMES_PER_BLOCK) > n_cu * FLAT_WG_PER_CU,
            "rounds": _ceil_div(n, blocks * K_T)}


def single_wg_path(n: int) -> dict:
    """scale_to_total and fes_finalize_kernel: 1024 threads stride over n cells."""
    return {"loops": n > SINGLE_WG_THREADS, "idle_threads": n < SINGLE_WG_THREADS}


def covers(got: dict, want: dict) -> list:
    return [(k, v, got.get(k)) for k, v in want.items() if got.get(k) != v]


# ---------------------------------------------------------------------------------------------------------------------
# 2-D histogram
# ---------------------------------------------------------------------------------------------------------------------
def hist_edges(kind: str, nb: int) -> np.ndarray:
    if kind == "uniform":
        return np.linspace(-1.5, 2.5, nb + 1)
    if kind == "unit":
        return np.linspace(0.0, 1.0, nb + 1)
    if kind == "geom":                       # six decades: the uniform first guess is far too low, the walk goes up
        return np.geomspace(1e-3, 1e3, nb + 1)
    if kind == "geom_down":                  # mirrored: the first guess is far too high, the walk goes down
        return -np.geomspace(1e-3, 1e3, nb + 1)[::-1].copy()
    if kind in ("repeat", "repeat_last"):    # a zero-width bin in the middle / at the end
        e = np.linspace(-1.5, 2.5, nb + 1)
        assert nb >= 3
        k = nb // 2 if kind == "repeat" else nb - 1
        e[k + 1] = e[k]
        if kind == "repeat_last":
            e[nb] = e[nb - 1]
        return e
    raise ValueError(kind)


def _axis_samples(e: np.ndarray, n: int, rng) -> np.ndarray:
    """n samples: a random bin (or just outside either end) and a random place inside it."""
    nb = len(e) - 1
    b = rng.integers(-1, nb + 1, size=n) if nb > 1 else rng.integers(-1, 2, size=n)
    t = rng.random(n)
    lo = np.where(b < 0, e[0] - 0.3 * (e[-1] - e[0]), e[np.clip(b, 0, nb)])
    hi = np.where(b < 0, e[0], np.where(b >= nb, e[-1] + 0.3 * (e[-1] - e[0]), e[np.clip(b + 1, 0, nb)]))
    return lo + t * (hi - lo)


def axis_specials(e: np.ndarray) -> np.ndarray:
    """Every edge (a subset of 64 and both ends of a long table), one ulp on either side, +-inf and NaN."""
    pick = e if len(e) <= 200 else e[np.unique(np.concatenate([[0, 1, len(e) - 2, len(e) - 1],
                                                                 np.linspace(0, len(e) - 1, 64).astype(int)]))]
    return np.concatenate([pick, np.nextafter(pick, np.inf), np.nextafter(pick, -np.inf), [np.inf, -np.inf, np.nan]])


def pick_w_absmax(n: int, bound: float) -> float:
    """A bound of |w| for which n * w_absmax is well away from a power of two, so that ceil(log2(.)) is the same number
    in any libm; asserts it with rational arithmetic."""
    a = float(bound)
    for _ in range(8):
        v = Fraction(max(1, n)) * Fraction(a)
        c = math.ceil(math.log2(float(v)))
        if Fraction(2) ** (c - 1) * Fraction(102, 100) < v < Fraction(2) ** c * Fraction(98, 100):
            return a
        a *= 1.25
    raise AssertionError("no w_absmax away from a power of two")


def hist_exponent(n: int, w_absmax: float) -> int:
    """e of msm_hist2d: 2^e with n * w_absmax * 2^e < 2^62."""
    v = Fraction(max(1, n)) * Fraction(w_absmax)
    c = math.ceil(math.log2(max(1.0, float(n)) * w_absmax))
    assert Fraction(2) ** (c - 1) * Fraction(101, 100) < v < Fraction(2) ** c * Fraction(99, 100), (n, w_absmax)
    return min(61 - c, 1000)


def hist_data(row: dict, n_cu: int) -> dict:
    """{x, y [n], xe, ye, w or None, w_absmax} of a hist row.  The special values of x sit in the first frames, those
    of y right behind them (each beside an ordinary value of the other axis)."""
    n, nx, ny = resolve(row["n"], n_cu), row["nx"], row["ny"]
    rng = np.random.default_rng(row["seed"])
    xe, ye = hist_edges(row["xedges"], nx), hist_edges(row["yedges"], ny)
    x, y = _axis_samples(xe, n, rng), _axis_samples(ye, n, rng)
    if row["weights"] == "cancel":            # frames 2k and 2k + 1 share a place
        x[1::2], y[1::2] = x[0:n - 1:2], y[0:n - 1:2]
    else:
        sx, sy = axis_specials(xe), axis_specials(ye)
        if n >= len(sx) + len(sy):
            x[:len(sx)] = sx
            y[len(sx):len(sx) + len(sy)] = sy
        elif n >= 8:
            x[:3], y[3:6] = [np.nan, np.inf, xe[-1]], [np.nan, -np.inf, ye[0]]
    out = {"x": x, "y": y, "xe": xe, "ye": ye, "w": None, "w_absmax": 0.0, "n": n}
    kind = row["weights"]
    if kind is None:
        return out
    w = rng.uniform(0.05, 1.0, n) * 3.7
    if kind == "signed":
        w *= rng.choice([-1.0, 1.0], n)
    elif kind == "cancel":
        w[1::2] = -w[0:n - 1:2]
    elif kind == "tiny":                      # every other weight 2^-40 of the largest
        w[0::2] *= 2.0 ** -40
    bound = float(np.abs(w).max(initial=1.0))
    if kind == "over":
        bound *= 2.0 ** 10
    out["w"], out["w_absmax"] = w, pick_w_absmax(n, bound)
    if kind == "over":
        assert out["w_absmax"] >= 2.0 ** 10 * np.abs(w).max()
    return out


def edge_bin(e: np.ndarray, v: np.ndarray) -> np.ndarray:
    """searchsorted(e, v, 'right') - 1, the last edge inclusive, -1 outside or NaN: edge_bin of fes.hip."""
    v = np.asarray(v, np.float64)
    i = np.searchsorted(e, v, side="right") - 1
    i = np.where(v == e[-1], len(e) - 2, i)
    with np.errstate(invalid="ignore"):
        ok = (v >= e[0]) & (v <= e[-1])
    return np.where(ok, i, -1)


def hist_counts(d: dict) -> np.ndarray:
    """np.histogram2d on the same edge arrays, non-finite samples removed first."""
    ok = np.isfinite(d["x"]) & np.isfinite(d["y"])
    H, _, _ = np.histogram2d(d["x"][ok], d["y"][ok], bins=[d["xe"], d["ye"]])
    return H


def hist_weighted(d: dict):
    """(exact, true, bound): the integer restatement sum(rint(w 2^e)) per bin, converted to fp64 once and scaled by
    2^-e; the true sums of w per bin (math.fsum); |exact - true| <= count 2^-(e+1) plus the roundings of the
    conversion and of fsum."""
    nx, ny = len(d["xe"]) - 1, len(d["ye"]) - 1
    e = hist_exponent(d["n"], d["w_absmax"])
    ix, iy = edge_bin(d["xe"], d["x"]), edge_bin(d["ye"], d["y"])
    ok = (ix >= 0) & (iy >= 0)
    cell = (ix * ny + iy)[ok]
    scaled = np.rint(d["w"][ok] * 2.0 ** e)                      # w * 2^e is exact: a power of two, no overflow
    assert np.all(np.abs(scaled) < 2.0 ** 62) and d["n"] * float(np.abs(scaled).max(initial=0.0)) < 2.0 ** 63
    acc = np.zeros(nx * ny, np.int64)
    np.add.at(acc, cell, scaled.astype(np.int64))                # exact: every partial sum is below 2^63
    exact = np.array([float(int(a)) for a in acc]) * 2.0 ** -e   # int -> fp64 rounds once (to nearest even)
    cnt = np.bincount(cell, minlength=nx * ny)
    true = np.zeros(nx * ny)
    order = np.argsort(cell, kind="stable")
    ws, cs = d["w"][ok][order], cell[order]
    starts = np.searchsorted(cs, np.arange(nx * ny), side="left")
    stops = np.searchsorted(cs, np.arange(nx * ny), side="right")
    for c in np.nonzero(cnt)[0]:
        true[c] = math.fsum(ws[starts[c]:stops[c]])
    half = cnt * 2.0 ** -(e + 1)
    bound = half + 2.0 ** -53 * (np.abs(true) + half) + 2.0 ** -53 * np.abs(true)
    return exact.reshape(nx, ny), true.reshape(nx, ny), bound.reshape(nx, ny), cnt.reshape(nx, ny), e


# ---------------------------------------------------------------------------------------------------------------------
# kernel density
# ---------------------------------------------------------------------------------------------------------------------
TWO_PI_F64, PI_F64 = 6.283185307179586, 3.141592653589793      # the constants of wrap_angle


def kde_normaliser(bw_x: float, bw_y: float) -> float:
    """The fp64 expression of msm_kde2d."""
    return 1.0 / (2.0 * 3.14159265358979323846 * bw_x * bw_y)


def device_differences(c: np.ndarray, v: np.ndarray, wrap: bool) -> np.ndarray:
    """centre - sample [len(c), len(v)] with the kernel's own fp64 operations (wrap_angle when the axis is periodic)."""
    d = c[:, None] - v[None, :]
    if wrap:
        m = np.fmod(d + PI_F64, TWO_PI_F64)
        m = np.where(m < 0.0, m + TWO_PI_F64, m)
        d = m - PI_F64
    return d


def kde_indicator(row: dict, n_cu: int) -> dict:
    """Frames exactly on centres (on a periodic axis moved by whole turns), integer weights, dyadic w_scale.  Asserts
    that every Gaussian factor the kernel evaluates is exactly 1 (0.5 u^2 < 2^-60, checked in long double) or exactly 0
    (|u| >= 39: exp(-760) is below the smallest subnormal)."""
    n, nx, ny, per = resolve(row["n"], n_cu), row["nx"], row["ny"], row["periodic"]
    rng = np.random.default_rng(row["seed"])
    if per == 0:
        bwx, bwy = 1.0, 2.0
        xc, yc = 64.0 * np.arange(nx) - 640.0, 128.0 * np.arange(ny) + 77.0
    else:
        bwx, bwy = 2.0 ** -11, 2.0 ** -12
        xc, yc = -3.0 + 2.0 ** -5 * np.arange(nx), -2.5 + 2.0 ** -5 * np.arange(ny)
        assert xc[-1] < 3.0 and yc[-1] < 3.0
    a, b = rng.integers(0, nx, n), rng.integers(0, ny, n)
    a[-1], b[-1] = nx - 1, ny - 1                     # the last frame (alone in its group when n % 4 == 1) on the corner
    a[0], b[0] = 0, ny - 1
    x, y = xc[a].copy(), yc[b].copy()
    if per & 1:
        x = x + TWO_PI_F64 * rng.integers(-3, 4, n)
    if per & 2:
        y = y + TWO_PI_F64 * rng.integers(-2, 3, n)
    w = rng.integers(1, 8, n).astype(np.float64) if row["weights"] else None
    w_scale = row["w_scale"]
    assert math.frexp(w_scale)[0] in (0.5, 0.75, 0.625)           # dyadic with a few bits: w * w_scale is exact
    for c, v, idx, bw, wrap in ((xc, x, a, bwx, bool(per & 1)), (yc, y, b, bwy, bool(per & 2))):
        u = (device_differences(c, v, wrap) * (1.0 / bw)).astype(LD)
        hit = np.arange(len(c))[:, None] == idx[None, :]
        assert np.all(LD(0.5) * u[hit] * u[hit] < LD(2.0) ** -60), row["name"]
        assert np.all(np.abs(u[~hit]) >= 39.0), row["name"]
    mass = np.zeros((nx, ny))
    np.add.at(mass, (a, b), (w if w is not None else np.ones(n)) * w_scale)
    assert np.all(mass * 64 == np.rint(mass * 64)) and mass.max() < 2.0 ** 40
    return {"x": x, "y": y, "xc": xc, "yc": yc, "bw": (bwx, bwy), "w": w, "w_scale": w_scale, "n": n,
            "density": mass * kde_normaliser(bwx, bwy)}


def kde_smooth(row: dict, n_cu: int) -> dict:
    n, nx, ny, per = resolve(row["n"], n_cu), row["nx"], row["ny"], row["periodic"]
    assert n <= 4096
    rng = np.random.default_rng(row["seed"])
    if per & 1:
        x, xc, bwx = rng.uniform(-np.pi, np.pi, n), np.linspace(-np.pi, np.pi, nx, endpoint=False), 0.35
    else:
        x, xc, bwx = rng.normal(0.0, 1.0, n), np.linspace(-2.5, 2.5, nx) if nx > 1 else np.array([0.1]), 0.31
    if per & 2:
        y, yc, bwy = rng.uniform(-np.pi, np.pi, n), np.linspace(-np.pi, np.pi, ny, endpoint=False), 0.5
    else:
        y, yc, bwy = rng.normal(0.5, 0.7, n), np.linspace(-2.0, 3.0, ny) if ny > 1 else np.array([0.4]), 0.47
    w = rng.gamma(1.5, 1.0, n) if row["weights"] else None
    return {"x": x, "y": y, "xc": xc, "yc": yc, "bw": (bwx, bwy), "w": w, "w_scale": row["w_scale"], "n": n}


def kde_reference(d: dict, periodic: int, c_sum: int, K: float):
    """(density, bound) in long double: sum_k t_k with t_k = |w_k| ex ey / (2 pi bw_x bw_y), and per cell
    sum_k t_k (c_sum + K + 2 (u_k^2 + v_k^2)) 2^-52."""
    def axis(c, v, bw, wrap):
        diff = c.astype(LD)[:, None] - v.astype(LD)[None, :]
        if wrap:
            diff = np.remainder(diff + PI_LD, 2 * PI_LD) - PI_LD
        u = diff / LD(bw)
        return np.exp(LD(-0.5) * u * u), u * u
    ex, u2 = axis(d["xc"], d["x"], d["bw"][0], bool(periodic & 1))
    ey, v2 = axis(d["yc"], d["y"], d["bw"][1], bool(periodic & 2))
    w = (np.ones(d["n"]) if d["w"] is None else d["w"]).astype(LD) * LD(d["w_scale"])
    norm = 1 / (2 * PI_LD * LD(d["bw"][0]) * LD(d["bw"][1]))
    dens = (ex @ (ey * w[None, :]).T) * norm
    eyw = ey * np.abs(w)[None, :]
    bound = (ex * (c_sum + K + 2 * u2)) @ eyw.T + 2 * (ex @ (eyw * v2).T)
    return dens, bound * norm * LD(2.0) ** -52


# ---------------------------------------------------------------------------------------------------------------------
# weighted statistics
# ---------------------------------------------------------------------------------------------------------------------
def wstats_exact(n: int, weighted: bool, seed: int):
    """(x, w or None, out6): integer x mirrored about an integer centre, weights in {1/4, 1/2, 1, 2} shared by each
    mirrored pair, so the weighted mean is the centre itself; every term and every partial sum is a multiple of 1/16
    far below 2^53 / 16, and the two quotients are single correctly rounded divisions."""
    rng = np.random.default_rng(seed)
    c = int(rng.integers(-9, 10))
    half = n // 2
    dlt = rng.integers(0, 41, half)
    wh = 2.0 ** rng.integers(-2, 2, half) if weighted else np.ones(half)
    x = np.concatenate([c + dlt, c - dlt, [c] * (n - 2 * half)]).astype(np.float64)
    w = np.concatenate([wh, wh, [0.5 if weighted else 1.0] * (n - 2 * half)])
    order = rng.permutation(n)
    x, w = x[order], w[order]
    wi, xi = np.rint(w * 4).astype(np.int64), x.astype(np.int64)
    assert np.array_equal(wi / 4.0, w) and int((wi * wi).sum()) * 50 * 50 < 2 ** 53
    sw, sw2, swx = Fraction(int(wi.sum()), 4), Fraction(int((wi * wi).sum()), 16), Fraction(int((wi * xi).sum()), 4)
    assert swx == c * sw
    s = Fraction(int((wi * (xi - c) ** 2).sum()), 4)
    out = np.array([float(sw), float(sw2), float(c), float(s / sw), float(xi.min()), float(xi.max())])
    assert Fraction(out[0]) == sw and Fraction(out[1]) == sw2
    return x, (w if weighted else None), out


def wstats_reference(x, w):
    """(values, bounds) for inexact data, rational arithmetic rounded once; bounds: n u sum|terms| for the three sums,
    carried through the two divisions, u = 2^-53."""
    n = len(x)
    w = np.ones(n) if w is None else w
    fx, fw = [Fraction(float(v)) for v in x], [Fraction(float(v)) for v in w]
    sw, sw2, swx = sum(fw), sum(a * a for a in fw), sum(a * b for a, b in zip(fw, fx))
    mean = swx / sw
    s = sum(a * (b - mean) ** 2 for a, b in zip(fw, fx))
    var = s / sw
    u = 2.0 ** -53
    a_w, a_wx = float(sum(abs(a) for a in fw)), float(sum(abs(a * b) for a, b in zip(fw, fx)))
    b_sw, b_sw2 = (n + 1) * u * a_w, (n + 2) * u * float(sw2)
    b_mean = ((n + 3) * u * a_wx + abs(float(mean)) * b_sw) / float(sw) * (1 + 1e-9)
    mad = float(sum(a * abs(b - mean) for a, b in zip(fw, fx)) / sw)
    b_var = (n + 8) * u * float(var) * 2 + b_mean * (b_mean + 8 * u * mad) + float(var) * b_sw / float(sw)
    vals = np.array([float(sw), float(sw2), float(mean), float(var), float(np.min(x)), float(np.max(x))])
    return vals, np.array([b_sw, b_sw2, b_mean, b_var, 0.0, 0.0])


# ---------------------------------------------------------------------------------------------------------------------
# the small kernels
# ---------------------------------------------------------------------------------------------------------------------
def smooth_reference(h: np.ndarray, min_count: float):
    """(out, n_smoothed): bins below min_count take max(mean of the 8 neighbours with replicated edges, min_count)
    when that mean is positive and the value larger.  Exact on integer histograms ((tot - c) / 8 is a dyadic number)."""
    h = np.asarray(h, np.float64)
    p = np.pad(h, 1, mode="edge")
    tot = np.zeros_like(h)
    for di in range(3):
        for dj in range(3):
            tot = tot + p[di:di + h.shape[0], dj:dj + h.shape[1]]
    nm = (tot - h) / 8.0
    target = np.maximum(nm, min_count)
    take = (h < min_count) & (nm > 0.0) & (target > h)
    return np.where(take, target, h), int(take.sum())


def finalize_status(h: np.ndarray) -> int:
    """bit 0: an entry is NaN or beyond +-1e300, bit 1: not 0 < total < 1e300, bit 2: an entry <= 0.  Only for inputs
    whose total is far from 0 and from 1e300 (the device adds in another order)."""
    h = np.asarray(h, np.float64).ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        total = float(np.sum(h))
        st = 1 * bool(np.any(np.isnan(h) | (h > 1e300) | (h < -1e300))) | 4 * bool(np.any(h <= 0.0))
    return st | 2 * (not (total > 0.0 and total < 1e300))


def finalize_reference(h: np.ndarray, kT: float):
    """(F, bound) in long double: F = -kT ln(h / total) - min.  One division, one log and the product with kT bring
    kT (u + 2 u |ln p|), the subtraction of the minimum u |F - min| <= u kT (|ln p| + |ln p_max|), and the minimum
    carries its own share: with eps = 2^-52 = 2 u, |error| <= kT 2 eps ((1 + |ln p|) + (1 + |ln p_max|)).  The error of
    the total moves every cell alike and cancels."""
    hl = np.asarray(h, np.float64).astype(LD)
    lnp = np.log(hl / hl.sum())
    F = -LD(kT) * lnp
    F = F - F.min()
    bound = LD(kT) * 2 * LD(2.0) ** -52 * ((1 + np.abs(lnp)) + (1 + np.abs(lnp).min()))
    return F, bound


def clip_reference(x, lo: float, hi: float) -> np.ndarray:
    return np.clip(np.asarray(x, np.float64), lo, hi)


def wrap_reference(x, lo: float, hi: float) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, np.float64) - lo) % (hi - lo) + lo


def gather_reference(table, idx) -> np.ndarray:
    table, idx = np.asarray(table, np.float64), np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < len(table))
    return np.where(ok, table[np.where(ok, idx, 0)], 0.0)


def flat_specials(lo: float, hi: float) -> np.ndarray:
    span = hi - lo
    return np.array([lo, hi, np.nextafter(hi, np.inf), np.nextafter(hi, -np.inf), np.nextafter(lo, np.inf),
                     np.nextafter(lo, -np.inf), lo - 1e-20, -0.0, 0.0, np.inf, -np.inf, np.nan, lo + 1e6 * span + 0.25 * span,
                     lo - 1e6 * span - 0.25 * span, lo + 12345.0 * span, lo - 777.0 * span, 1e300, -1e300, 5e-324, -5e-324])


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
CASES: list = []


def _add(kind, name, reach, **kw):
    assert name not in {r["name"] for r in CASES}, name
    CASES.append({"kind": kind, "name": name, "reach": reach, "seed": 4000 + len(CASES), **kw})


def _hist(name, n, nx, ny, reach, *, weights=None, xedges="uniform", yedges="uniform", xy=False):
    _add("hist", name, reach, n=n, nx=nx, ny=ny, weights=weights, xedges=xedges, yedges=yedges, xy=xy)


_LDS = {"lds_bins": True, "lds_edges": True}
_GLOBAL = {"lds_bins": False, "lds_edges": True}
# -- shapes: either side of (nx + 1)(ny + 1) <= 8191, the degenerate grids ----------------------------------------------
_hist("hist-89x90-last-lds", 5000, 89, 90, dict(_LDS, lds_bytes=65528))
_hist("hist-90x90-first-global", 5000, 90, 90, dict(_GLOBAL, lds_bytes=182 * 8))
_hist("hist-91x91-global", 5000, 91, 91, _GLOBAL)
_hist("hist-1x7", 900, 1, 7, _LDS)
_hist("hist-7x1", 900, 7, 1, _LDS)
_hist("hist-1x1", 900, 1, 1, dict(_LDS, lds_bytes=40))
# -- frame counts ------------------------------------------------------------------------------------------------------
_hist("hist-n0", 0, 5, 3, {"kernel": "none"})
_hist("hist-n1", 1, 5, 3, {"grid": 1, "idle_lanes": True})
_hist("hist-n2047", 2047, 5, 3, {"grid": 1, "rounds": 8})
_hist("hist-n2049", 2049, 5, 3, {"grid": 2, "rounds": 5, "multi_block": True})
_hist("hist-n2049-global", 2049, 95, 93, dict(_GLOBAL, grid=2))
_hist("hist-past-one-round-of-the-largest-grid", ("cu", 4 * 256, 1), 6, 5, {"second_round": True, "capped": False})
_hist("hist-grid-capped", ("cu", 4 * 2048, 1), 6, 5, {"capped": True, "rounds": 9})
# -- inputs ------------------------------------------------------------------------------------------------------------
_hist("hist-two-arrays-two-strides", 3000, 9, 11, _LDS, xy=True)
_hist("hist-two-arrays-global", 3000, 96, 92, _GLOBAL, xy=True)
_hist("hist-geometric-edges", 4000, 37, 41, _LDS, xedges="geom", yedges="geom_down")
_hist("hist-geometric-edges-global", 4000, 97, 91, _GLOBAL, xedges="geom_down", yedges="geom")
_hist("hist-zero-width-bin", 3000, 8, 5, _LDS, xedges="repeat", yedges="repeat_last")
_hist("hist-zero-width-bin-global", 3000, 120, 80, _GLOBAL, xedges="repeat_last", yedges="repeat")
# -- weights: every kind on both paths -----------------------------------------------------------------------------------
for _kind in ("plain", "signed", "cancel", "tiny", "over"):
    _hist(f"hist-w-{_kind}-lds", 5001, 8, 6, dict(_LDS, weighted=True), weights=_kind)
    _hist(f"hist-w-{_kind}-global", 5001, 91, 93, dict(_GLOBAL, weighted=True), weights=_kind)
_hist("hist-w-n0", 0, 4, 4, {"kernel": "none"}, weights="plain")
_hist("hist-w-n1", 1, 4, 4, {"grid": 1}, weights="plain")
_hist("hist-w-past-one-round", ("cu", 4 * 256, 1), 7, 9, {"second_round": True, "weighted": True}, weights="signed")
# -- edge tables longer than the LDS -------------------------------------------------------------------------------------
_EDGES_GLOBAL = {"lds_bins": False, "lds_edges": False, "lds_bytes": 0}
_hist("hist-8189x1-longest-lds-edges", 30000, 8189, 1, dict(_GLOBAL, lds_bytes=65536), xedges="unit", yedges="unit")
_hist("hist-8190x1-first-global-edges", 30000, 8190, 1, _EDGES_GLOBAL, xedges="unit", yedges="unit")
_hist("hist-9000x1", 30000, 9000, 1, _EDGES_GLOBAL, xedges="unit", yedges="unit")
_hist("hist-1x9000", 30000, 1, 9000, _EDGES_GLOBAL, xedges="unit", yedges="geom")
_hist("hist-w-9000x1", 30000, 9000, 1, dict(_EDGES_GLOBAL, weighted=True), weights="signed", xedges="geom", yedges="unit")


def _kde(name, n, nx, ny, reach, *, periodic=0, weights=True, w_scale=1.0, cols=(0, 1), d=2, families=("indicator", "smooth")):
    _add("kde", name, reach, n=n, nx=nx, ny=ny, periodic=periodic, weights=weights, w_scale=w_scale, cols=cols, d=d,
         families=families)


# -- frame counts on one block: the tail group, fewer frames than a group, idle waves -----------------------------------
for _n, _tail in ((1, 1), (3, 3), (4, 4), (5, 1), (4095, 3)):
    _kde(f"kde-n{_n}-16x17", _n, 16, 17, {"tail_lanes": _tail, "blocks": 1, "clamped": True, "multi_slab": _n > 16},
         periodic=(0, 3, 1, 2, 0)[_n % 5], weights=_n % 2 == 1, w_scale=(1.0, 0.375)[_n % 2 == 0])
_kde("kde-second-iteration-64x64", ("cu", 32, 1), 64, 64, {"iters": 2, "blocks": 1, "clamped": False, "tail_lanes": 1},
     families=("indicator",))
# -- grids ---------------------------------------------------------------------------------------------------------------
_kde("kde-1x1", 1001, 1, 1, {"blocks": 1, "clamped": True}, w_scale=0.5)
_kde("kde-64x64", 517, 64, 64, {"blocks": 1, "clamped": False, "tail_lanes": 1}, periodic=3)
_kde("kde-65x64", 518, 65, 64, {"nby": 2, "nbz": 1, "clamped": True}, periodic=1, weights=False, w_scale=0.25)
_kde("kde-130x70", 4095, 130, 70, {"nby": 3, "nbz": 2, "loops": True, "multi_slab": True, "tail_lanes": 3}, periodic=2)
_kde("kde-130x70-plain", 1023, 130, 70, {"nby": 3, "nbz": 2, "multi_slab": True}, periodic=0)
# -- strided columns in reversed order, no weights with a scale, every periodic mask -------------------------------------
for _per in (0, 1, 2, 3):
    _kde(f"kde-cols-3-1-periodic{_per}", 203, 33, 20, {"blocks": 1, "tail_lanes": 3}, periodic=_per, cols=(3, 1), d=4,
         weights=_per % 2 == 0, w_scale=(0.75, 0.375)[_per % 2])


def _wstats(name, n, reach, *, layout="column", weighted=True):
    _add("wstats", name, reach, n=n, layout=layout, weighted=weighted)


_wstats("wstats-n1", 1, {"nb": 1, "per": 1}, layout="1d", weighted=False)
_wstats("wstats-n1-weighted", 1, {"nb": 1}, layout="column")
_wstats("wstats-n4096", 4096, {"nb": 1, "per": 4096, "strided_loop": True}, layout="column", weighted=False)
_wstats("wstats-n4097", 4097, {"nb": 2, "per": 2049, "ragged": True}, layout="column")
_wstats("wstats-n4097-1d", 4097, {"nb": 2, "ragged": True}, layout="1d")
_wstats("wstats-n777", 777, {"nb": 1, "strided_loop": False}, layout="column", weighted=False)
_wstats("wstats-every-block", ("cu", 2 * 4096, -4095), {"capped": True, "empty_block": False}, layout="1d")
_wstats("wstats-every-block-strided", ("cu", 2 * 4096, -4095), {"capped": True}, layout="column", weighted=False)

for _shape in ((1, 1), (1, 9), (9, 1), (17, 33), (5, 40)):
    _add("smooth", f"smooth-{_shape[0]}x{_shape[1]}", {"multi_block": _shape[0] * _shape[1] > 256}, shape=_shape)
for _n in (1, 1024, 1025, 70_000):
    _add("finalize", f"finalize-n{_n}", {"loops": _n > 1024, "idle_threads": _n < 1024}, n=_n)
for _n in (1, 1025):
    _add("scale", f"scale-n{_n}", {"loops": _n > 1024}, n=_n)
_add("flat", "flat-n0", {"kernel": "none"}, n=0)
_add("flat", "flat-n1", {"blocks": 1, "rounds": 1}, n=1)
_add("flat", "flat-n1500", {"blocks": 2, "rounds": 3}, n=1500)
_add("flat", "flat-past-the-grid-stride-limit", {"capped": False, "rounds": 4}, n=("cu", 8 * 256, 1))
_add("flat", "flat-grid-capped", {"capped": True, "rounds": 5}, n=("cu", 8 * 1024, 1))


def rows(kind: str) -> list:
    return [r for r in CASES if r["kind"] == kind]


def ids(rs) -> list:
    return [r["name"] for r in rs]


def row_path(row: dict, n_cu: int) -> dict:
    kind = row["kind"]
    if kind == "hist":
        return hist2d_path(resolve(row["n"], n_cu), row["nx"], row["ny"], row["weights"] is not None, n_cu)
    if kind == "kde":
        return kde_path(resolve(row["n"], n_cu), row["nx"], row["ny"], n_cu)
    if kind == "wstats":
        return wstats_path(resolve(row["n"], n_cu), n_cu)
    if kind == "smooth":
        return {"multi_block": row["shape"][0] * row["shape"][1] > 256}
    if kind in ("finalize", "scale"):
        return single_wg_path(row["n"])
    if kind == "flat":
        return flat_path(resolve(row["n"], n_cu), n_cu)
    raise ValueError(kind)
