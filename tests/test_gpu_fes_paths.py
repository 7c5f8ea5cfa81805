"""The free-energy-surface kernels of csrc/fes.hip on every launch path, against exact references.

Each row of tests/_fes_ref.CASES names the branch it is there to reach; tests/test_fes_reference.py proves on the CPU
that it does, and the tests here check it again with the device's own number of compute units.  Outputs are written
into blocks whose guard regions hold a sentinel, inputs that a kernel indexes with a clamp sit between guards as well.

Exact rows (np.testing.assert_array_equal, no tolerance): unweighted histograms against np.histogram2d; weighted
histograms against the integer restatement of the 2^e fixed point; the KDE on "indicator" data, whose Gaussian factors
are all exactly 1 or 0; weighted statistics of integer data with dyadic weights and an integer mean; the sparse-bin
smoothing of integer histograms; clip and wrap against numpy; gather; scale_to_total by a power of two.

Bounded rows compare with a long-double or rational reference, never with the kernel's own output, and print the
worst error / bound they see.  K of the KDE bound (the device exp, the three-factor product and the wrap of a periodic
axis) cannot be derived from the repository: it starts at 8 and is the smallest power of two that leaves a factor 4 over
the worst ratio observed.

Observed on an MI355X (the tests print it): every exact row is bit-equal.  KDE smooth data, worst error / bound over
all rows: 0.59 with K = 8, 0.47 with K = 16, 0.41 with K = 32, 0.33 with K = 64; the worst cell is a single frame on a
torus (n = 1, periodic mask 3), where the error of the wrapped difference, divided by the bandwidth, outweighs the
summation.  Its bound is linear in K, which puts the ratio at 0.235 for K = 128: the first power of two with a factor 4
to spare, and the value kept (measured with K up to 64; 128 is that extrapolation, the run with it has yet to print its
own figure).  Away from that row the worst ratio at K = 32 is 0.34 (n = 3) and 0.16 on grids with hundreds of frames.
fes_finalize: 0.39 of its bound (70 000 cells).  weighted_stats on inexact data: 0.07 (n = 2), below 0.01 from 1000
frames on (the bounds assume a sequential sum, the kernel adds in a tree).

Not covered: a degenerate axis with edges[0] == edges[-1] (the first guess divides by zero); nx or ny near 4096 in
kde2d, where the slabs take gigabytes; frame counts past 2^31; graph capture of these entry points."""

from __future__ import annotations

import math

import numpy as np
import pytest

from pmarlo_amd import _lib
from tests import _fes_ref as fr

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = fr.SENTINEL
LD = np.longdouble
KDE_K = 128


@pytest.fixture(scope="module")
def n_cu(engine) -> int:
    return engine.info()["n_cu"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class _Guarded:
    """A device block [GUARD | size | GUARD] filled with the sentinel (or holding `data` in the middle)."""

    def __init__(self, engine, shape, dtype=np.float64, data=None, fill=FILL):
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        self.size = int(np.prod(self.shape))
        self.fill = np.dtype(dtype).type(fill)
        host = np.full(2 * GUARD + self.size, self.fill, dtype)
        if data is not None:
            host[GUARD:GUARD + self.size] = np.asarray(data, dtype).ravel()
        self.block = engine.to_device(host)
        self.view = self.block.view(self.shape, offset_elems=GUARD)

    def host(self, what=""):
        h = self.block.to_host()
        np.testing.assert_array_equal(h[:GUARD], self.fill, err_msg=f"{what}: written before the output")
        np.testing.assert_array_equal(h[GUARD + self.size:], self.fill, err_msg=f"{what}: written past the output")
        return h[GUARD:GUARD + self.size].reshape(self.shape)


def _column(engine, v, d: int, col: int, pad=np.nan):
    """v as column `col` of an [n, d] device array whose other columns hold `pad` -> (array, pointer, stride)."""
    host = np.full((len(v), d), pad)
    host[:, col] = v
    arr = engine.to_device(host)
    return arr, arr.ptr + 8 * col, d


def _hist_call(engine, lib, d, px, sx, py, sy, tag):
    nx, ny = len(d["xe"]) - 1, len(d["ye"]) - 1
    xe, ye = engine.to_device(d["xe"]), engine.to_device(d["ye"])
    w = engine.to_device(d["w"]) if d["w"] is not None else None
    out = _Guarded(engine, (nx, ny))
    _lib.check(lib.msm_hist2d(engine.handle, px, sx, py, sy, d["n"], w.ptr if w is not None else None,
                              float(d["w_absmax"]), xe.ptr, nx, ye.ptr, ny, out.view.ptr), engine.handle)
    return out.host(tag)


# ---------------------------------------------------------------------------------------------------------------------
# 2-D histogram
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", fr.rows("hist"), ids=fr.ids(fr.rows("hist")))
def test_hist2d_row_is_exact(engine, lib, n_cu, row):
    miss = fr.covers(fr.row_path(row, n_cu), row["reach"])
    assert not miss, (n_cu, row["name"], miss)                      # on THIS device too
    d = fr.hist_data(row, n_cu)
    n = d["n"]
    if row["xy"]:                            # two arrays, two strides, through the wrapper as well
        ax, px, sx = _column(engine, d["x"], 3, 2)
        ay, py, sy = _column(engine, d["y"], 5, 1)
    else:                                    # the columns of one array, in reversed order
        xy = engine.to_device(np.stack([d["y"], np.full(n, np.nan), d["x"]], axis=1) if n else np.zeros((0, 3)))
        px, sx, py, sy = xy.ptr + 16, 3, xy.ptr, 3
    got = _hist_call(engine, lib, d, px, sx, py, sy, row["name"])
    if d["w"] is None:
        ref = fr.hist_counts(d)
        np.testing.assert_array_equal(got, ref, err_msg=row["name"])
        if row["xy"]:
            np.testing.assert_array_equal(engine.hist2d_xy((ax, 2), (ay, 1), d["xe"], d["ye"]).to_host(), ref)
        elif n:
            np.testing.assert_array_equal(engine.hist2d(xy, (2, 0), d["xe"], d["ye"]).to_host(), ref)
        return
    exact, true, bound, cnt, e = fr.hist_weighted(d)
    np.testing.assert_array_equal(got, exact, err_msg=f"{row['name']} (e = {e})")
    assert np.all(np.abs(got - true) <= bound), row["name"]
    if n:
        np.testing.assert_array_equal(engine.hist2d(xy, (2, 0), d["xe"], d["ye"], weights=engine.to_device(d["w"]),
                                                    w_absmax=d["w_absmax"]).to_host(), exact)
    if row["weights"] == "cancel":
        assert np.count_nonzero(got) <= 1 and cnt.sum() > 1000


def test_hist2d_refuses_by_argument_check_not_by_a_failed_launch(engine):
    """Every shape msm_hist2d accepts launches (long edge tables are read from global memory); what it refuses, it
    refuses with a message that names the limit."""
    x = engine.to_device(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="at most 2\\^24"):
        engine.hist2d(x, (0, 1), np.linspace(0, 1, 4098), np.linspace(0, 1, 4098))        # 4097^2 > 2^24 cells
    with pytest.raises(ValueError, match="w_absmax"):
        engine.hist2d(x, (0, 1), np.linspace(0, 1, 4), np.linspace(0, 1, 4), weights=engine.to_device(np.ones(4)), w_absmax=0.0)
    h = engine.hist2d(x, (0, 1), np.linspace(0, 1, 20001), np.array([0.0, 1.0])).to_host()
    assert h.shape == (20000, 1) and h[0, 0] == 4 and h.sum() == 4


def test_generate_1d_pmf_with_thousands_of_bins():
    from pmarlo_amd.markov_state_model.free_energy import generate_1d_pmf

    rng = np.random.default_rng(5)
    cv = np.concatenate([rng.normal(0.0, 1.0, 150_000), rng.uniform(-6, 6, 50_000)])
    r = generate_1d_pmf(cv, bins=9000)
    dens, edges = np.histogram(cv, bins=9000, density=True)
    np.testing.assert_array_equal(r.edges, edges)
    np.testing.assert_allclose(r.counts, dens, rtol=2.0 ** -50, atol=0)        # a / s / d against a / d / s
    counts, _ = np.histogram(cv, bins=9000)
    np.testing.assert_array_equal(np.rint(r.counts * np.diff(edges) * cv.size), counts)


def test_clip_keeps_nan_and_the_histogram_drops_it(engine):
    """The crop path of generate_2d_fes: np.clip keeps a NaN sample, np.histogram2d (NaN removed) never sees it."""
    rng = np.random.default_rng(6)
    xy = rng.normal(size=(5000, 2))
    xy[::97, 0] = np.nan
    xy[5::101, 1] = np.nan
    dev = engine.to_device(xy)
    lo, hi = -1.0, 1.25
    cx, cy = engine.clip_or_wrap(dev, lo, hi, wrap=False, col=0), engine.clip_or_wrap(dev, lo, hi, wrap=False, col=1)
    np.testing.assert_array_equal(cx.to_host(), np.clip(xy[:, 0], lo, hi))
    np.testing.assert_array_equal(cy.to_host(), np.clip(xy[:, 1], lo, hi))
    xe, ye = np.linspace(lo, hi, 13), np.linspace(lo, hi, 8)
    ok = np.isfinite(xy).all(axis=1)
    want, _, _ = np.histogram2d(np.clip(xy[ok, 0], lo, hi), np.clip(xy[ok, 1], lo, hi), bins=[xe, ye])
    got = engine.hist2d_xy(cx, cy, xe, ye).to_host()
    np.testing.assert_array_equal(got, want)
    assert got.sum() == ok.sum() < 5000


# ---------------------------------------------------------------------------------------------------------------------
# kernel density
# ---------------------------------------------------------------------------------------------------------------------
def _kde_call(engine, lib, d, row, tag):
    n, nx, ny = d["n"], row["nx"], row["ny"]
    host = np.full((n, row["d"]), np.nan)
    host[:, row["cols"][0]], host[:, row["cols"][1]] = d["x"], d["y"]
    xy = engine.to_device(host)
    # the centres sit between guards of NaN: a centre index past the grid that is not clamped poisons the block
    xc, yc = _Guarded(engine, nx, data=d["xc"], fill=np.nan), _Guarded(engine, ny, data=d["yc"], fill=np.nan)
    w = engine.to_device(d["w"]) if d["w"] is not None else None
    out = _Guarded(engine, (nx, ny))
    _lib.check(lib.msm_kde2d(engine.handle, xy.ptr + 8 * row["cols"][0], row["d"], xy.ptr + 8 * row["cols"][1], row["d"], n,
                             w.ptr if w is not None else None, float(d["w_scale"]), xc.view.ptr, nx, yc.view.ptr, ny,
                             float(d["bw"][0]), float(d["bw"][1]), int(row["periodic"]), out.view.ptr), engine.handle)
    got = out.host(tag)
    if row["d"] == 2 and row["cols"] == (0, 1):
        np.testing.assert_array_equal(engine.kde2d(xy, (0, 1), d["xc"], d["yc"], d["bw"][0], d["bw"][1], w, d["w_scale"],
                                                   periodic=row["periodic"]).to_host(), got)
    return got


@pytest.mark.parametrize("row", fr.rows("kde"), ids=fr.ids(fr.rows("kde")))
def test_kde2d_indicator_row_is_exact(engine, lib, n_cu, row):
    miss = fr.covers(fr.row_path(row, n_cu), row["reach"])
    assert not miss, (n_cu, row["name"], miss)
    d = fr.kde_indicator(row, n_cu)
    got = _kde_call(engine, lib, d, row, row["name"])
    np.testing.assert_array_equal(got, d["density"], err_msg=row["name"])


_SMOOTH = [r for r in fr.rows("kde") if "smooth" in r["families"]]


@pytest.mark.parametrize("row", _SMOOTH, ids=fr.ids(_SMOOTH))
def test_kde2d_smooth_row_is_within_its_bound(engine, lib, n_cu, row):
    """|density - long double| <= sum_k t_k (c_sum + K + 2 (u_k^2 + v_k^2)) 2^-52 per cell, with c_sum from kde_path."""
    path = fr.row_path(row, n_cu)
    d = fr.kde_smooth(row, n_cu)
    ref, bound = fr.kde_reference(d, row["periodic"], path["c_sum"], KDE_K)
    got = _kde_call(engine, lib, d, row, row["name"])
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    err = np.abs(got.astype(LD) - ref)
    ratio = float((err / bound).max())
    other = {K: float((err / fr.kde_reference(d, row["periodic"], path["c_sum"], K)[1]).max()) for K in (8, 32, 64)}
    print(f"{row['name']}: periodic {row['periodic']}, c_sum {path['c_sum']}, worst error / bound = {ratio:.3f} "
          f"(K = {KDE_K}); with other K: {other}")
    assert np.all(err <= bound), (row["name"], ratio, np.unravel_index(int(np.argmax(err / bound)), got.shape))


# ---------------------------------------------------------------------------------------------------------------------
# weighted statistics
# ---------------------------------------------------------------------------------------------------------------------
def _wstats(engine, x, w, layout):
    wd = engine.to_device(w) if w is not None else None
    if layout == "1d":
        return engine.weighted_stats(engine.to_device(x), 0, wd)
    arr, _, _ = _column(engine, x, 3, 1)
    return engine.weighted_stats(arr, 1, wd)


@pytest.mark.parametrize("row", fr.rows("wstats"), ids=fr.ids(fr.rows("wstats")))
def test_weighted_stats_row_is_exact(engine, n_cu, row):
    miss = fr.covers(fr.row_path(row, n_cu), row["reach"])
    assert not miss, (n_cu, row["name"], miss)
    x, w, want = fr.wstats_exact(fr.resolve(row["n"], n_cu), row["weighted"], row["seed"])
    np.testing.assert_array_equal(_wstats(engine, x, w, row["layout"]), want, err_msg=row["name"])


@pytest.mark.parametrize("n", [2, 1000, 4097, 9001])
def test_weighted_stats_inexact_data_within_the_summation_bounds(engine, n):
    rng = np.random.default_rng(n)
    x, w = rng.normal(1e3, 2.0, n), rng.gamma(2.0, 1.0, n)
    for weights, layout in ((w, "column"), (None, "1d")):
        vals, bounds = fr.wstats_reference(x, weights)
        got = _wstats(engine, x, weights, layout)
        err = np.abs(got - vals)
        ratio = float((err[:4] / bounds[:4]).max())
        print(f"weighted_stats n={n} {'weighted' if weights is not None else 'plain'}: worst error / bound = {ratio:.3f}")
        assert np.all(err <= bounds), (n, err, bounds)


def test_weighted_stats_with_a_nan_and_an_inf_sample(engine):
    """What the kernel does today, pinned down: min and max skip a NaN sample (fmin / fmax), the sums turn NaN; an inf
    sample is the maximum, makes the mean inf and the variance NaN; sum w and sum w^2 never see the samples."""
    rng = np.random.default_rng(3)
    x, w = rng.integers(-20, 21, 5000).astype(np.float64), 2.0 ** rng.integers(-2, 2, 5000)
    for where in (0, 4999, 1234):
        xn = x.copy()
        xn[where] = np.nan
        got = _wstats(engine, xn, w, "column")
        keep = np.arange(5000) != where
        assert got[0] == w.sum() and got[1] == (w * w).sum() and np.isnan(got[2]) and np.isnan(got[3])
        assert got[4] == x[keep].min() and got[5] == x[keep].max()
        xi = x.copy()
        xi[where] = np.inf
        got = _wstats(engine, xi, w, "1d")
        assert got[0] == w.sum() and got[2] == np.inf and np.isnan(got[3]) and got[4] == x[keep].min() and got[5] == np.inf
    with pytest.raises(ValueError):
        engine.weighted_stats(engine.to_device(np.zeros((0, 1))))


# ---------------------------------------------------------------------------------------------------------------------
# the small kernels
# ---------------------------------------------------------------------------------------------------------------------
def _smooth_call(engine, lib, h, min_count, tag):
    nx, ny = h.shape
    src = _Guarded(engine, (nx, ny), data=h, fill=1e9)       # a neighbour index that leaves the grid reads 1e9
    out = _Guarded(engine, (nx, ny))
    cnt = _Guarded(engine, 1, np.int32, fill=-77)
    _lib.check(lib.msm_smooth_sparse_bins(engine.handle, src.view.ptr, nx, ny, float(min_count), out.view.ptr, cnt.view.ptr),
               engine.handle)
    return out.host(tag), int(cnt.host(tag)[0])


@pytest.mark.parametrize("row", fr.rows("smooth"), ids=fr.ids(fr.rows("smooth")))
def test_smooth_sparse_bins_row_is_exact(engine, lib, row):
    nx, ny = row["shape"]
    rng = np.random.default_rng(row["seed"])
    h = rng.integers(0, 40, size=(nx, ny)).astype(np.float64) * (rng.random((nx, ny)) < 0.6)
    h[0, 0], h[nx - 1, ny - 1] = 0.0, 1.0                     # corners below the threshold: every clamp is used
    for min_count in (0.0, 1.0, 5.0, 1000.0):
        want, n_want = fr.smooth_reference(h, min_count)
        got, n_got = _smooth_call(engine, lib, h, min_count, row["name"])
        np.testing.assert_array_equal(got, want, err_msg=f"{row['name']} min_count={min_count}")
        assert n_got == n_want, (row["name"], min_count)
        if min_count == 0.0:
            assert n_got == 0
    got, n_got = _smooth_call(engine, lib, np.zeros((nx, ny)), 3.0, row["name"])     # nothing to take from
    assert n_got == 0 and not got.any()
    out, cnt = engine.smooth_sparse_bins(engine.to_device(h), 5.0)
    np.testing.assert_array_equal(out.to_host(), fr.smooth_reference(h, 5.0)[0])
    assert cnt == fr.smooth_reference(h, 5.0)[1]


def _finalize_call(engine, lib, h, kT, tag):
    src = engine.to_device(np.asarray(h, np.float64))
    F = _Guarded(engine, src.size)
    st = _Guarded(engine, 1, np.int32, fill=-77)
    _lib.check(lib.msm_fes_finalize(engine.handle, src.ptr, src.size, float(kT), F.view.ptr, st.view.ptr), engine.handle)
    return F.host(tag), int(st.host(tag)[0])


@pytest.mark.parametrize("row", fr.rows("finalize"), ids=fr.ids(fr.rows("finalize")))
def test_fes_finalize_row(engine, lib, row):
    """F within kT 2 eps ((1 + |ln p|) + (1 + |ln p_max|)) of the long-double value, its minimum exactly 0; each status
    bit alone and combined, with F left untouched."""
    n, kT = row["n"], 2.4943387
    rng = np.random.default_rng(row["seed"])
    h = rng.gamma(1.2, 50.0, n) + 1e-6
    h[rng.integers(0, n, max(1, n // 50))] *= 1e-9
    ref, bound = fr.finalize_reference(h, kT)
    F, st = _finalize_call(engine, lib, h, kT, row["name"])
    assert st == 0 and F.min() == 0.0 and np.all(F >= 0.0)
    err = np.abs(F.astype(LD) - ref)
    print(f"{row['name']}: worst error / bound = {float((err / bound).max()):.3f}")
    assert np.all(err <= bound), (row["name"], float((err / bound).max()))
    Fw, stw = engine.fes_finalize(engine.to_device(h.reshape(1, n)), kT)
    np.testing.assert_array_equal(Fw.to_host().ravel(), F)
    for where in sorted({0, n - 1, n // 2}):
        cases = [("NaN", {where: np.nan}, 3), ("+inf", {where: np.inf}, 3), ("-inf", {where: -np.inf}, 7),
                 ("zero", {where: 0.0}, 4 if n > 1 else 6), ("negative", {where: -1e-3}, 4 if n > 1 else 6)]
        if n > 1:
            cases.append(("total beyond 1e300", {where: 6e299, (where + 1) % n: 6e299}, 2))
        if where + 1 < n:         # neighbours, so that the pair meets before either has swallowed the rest of the sum
            cases.append(("+-2e300 cancel", {where: 2e300, where + 1: -2e300}, 5))
        for tag, put, want in cases:
            hb = h.copy()
            for k, v in put.items():
                hb[k] = v
            assert fr.finalize_status(hb) == want, (tag, n)
            F, st = _finalize_call(engine, lib, hb, kT, f"{row['name']} {tag}")
            assert st == want, (row["name"], tag, where, st)
            np.testing.assert_array_equal(F, FILL, err_msg=f"{row['name']} {tag}: F written although the status is {st}")
    F, st = _finalize_call(engine, lib, -h, kT, row["name"])                  # every entry negative: total <= 0 as well
    assert st == 6 and np.all(F == FILL)


@pytest.mark.parametrize("row", fr.rows("scale"), ids=fr.ids(fr.rows("scale")))
def test_scale_to_total_row(engine, row):
    n = row["n"]
    rng = np.random.default_rng(row["seed"])
    v = rng.integers(1, 100, n).astype(np.float64)
    total = v.sum()
    for want_total in (total * 2.0 ** -7, total * 8.0, total):               # power-of-two ratios: exact
        g = _Guarded(engine, n, data=v)
        engine.scale_to_total(g.view, want_total)
        np.testing.assert_array_equal(g.host(row["name"]), v * (want_total / total))
    for zero_sum in (np.zeros(n), np.where(np.arange(n) % 2 == 0, 3.0, -3.0) if n % 2 == 0 else -v):
        g = _Guarded(engine, n, data=zero_sum)                                # a total of zero (or below): unchanged
        engine.scale_to_total(g.view, 5.0)
        np.testing.assert_array_equal(g.host(row["name"]), zero_sum)
    g = _Guarded(engine, n, data=v)
    engine.scale_to_total(g.view, 1.0)                                        # inexact ratio: one division, one product
    got = g.host(row["name"])
    np.testing.assert_allclose(got, v / total, rtol=2.0 ** -51)
    assert abs(got.sum() - 1.0) <= n * 2.0 ** -52
    with pytest.raises(ValueError):
        engine.scale_to_total(g.view, 0.0)


@pytest.mark.parametrize("row", fr.rows("flat"), ids=fr.ids(fr.rows("flat")))
def test_clip_wrap_and_gather_row(engine, lib, n_cu, row):
    miss = fr.covers(fr.row_path(row, n_cu), row["reach"])
    assert not miss, (n_cu, row["name"], miss)
    n = fr.resolve(row["n"], n_cu)
    rng = np.random.default_rng(row["seed"])
    for lo, hi in ((-1.5, 2.0), (0.0, 1.0), (-math.pi, math.pi)):
        x = rng.normal(0.0, 3.0, n) * (hi - lo)
        sp = fr.flat_specials(lo, hi)
        if n >= 2 * len(sp):
            x[:len(sp)], x[n - len(sp):] = sp, sp[::-1]                       # in the first round and in the last
        elif n:
            x[:] = sp[(np.arange(n) + int(lo * 4)) % len(sp)]
        arr, ptr, stride = _column(engine, x, 3, 2) if n else (engine.to_device(np.zeros((0, 3))), 0, 3)
        for mode, ref in ((1, fr.clip_reference(x, lo, hi)), (2, fr.wrap_reference(x, lo, hi))):
            out = _Guarded(engine, n)
            _lib.check(lib.msm_clip_or_wrap(engine.handle, ptr or arr.ptr, stride, n, lo, hi, mode, out.view.ptr), engine.handle)
            got = out.host(f"{row['name']} mode {mode}")
            np.testing.assert_array_equal(got, ref, err_msg=f"{row['name']} mode {mode} [{lo}, {hi}]")
            nz = (ref != 0) & ~np.isnan(ref)                                  # bit for bit but for the sign of 0 and of NaN
            np.testing.assert_array_equal(got[nz].view(np.int64), ref[nz].view(np.int64))
            if n:
                np.testing.assert_array_equal(engine.clip_or_wrap(arr, lo, hi, wrap=mode == 2, col=2).to_host(), ref)
    m = 37
    table = rng.normal(size=m)
    idx = rng.integers(-5, m + 5, n).astype(np.int32)
    bad = np.array([-1, m, -2 ** 31, 2 ** 31 - 1, 0, m - 1], np.int32)
    if n >= 2 * len(bad):
        idx[:len(bad)], idx[n - len(bad):] = bad, bad[::-1]
    elif n:
        idx[:] = bad[np.arange(n) % len(bad)]
    tab = _Guarded(engine, m, data=table, fill=9e9)                           # an index that slips through reads 9e9
    out = _Guarded(engine, n)
    _lib.check(lib.msm_gather_f64(engine.handle, tab.view.ptr, m, engine.to_device(idx).ptr, n, out.view.ptr), engine.handle)
    np.testing.assert_array_equal(out.host(row["name"]), fr.gather_reference(table, idx))
    np.testing.assert_array_equal(engine.gather(engine.to_device(table), engine.to_device(idx)).to_host(),
                                  fr.gather_reference(table, idx))


# ---------------------------------------------------------------------------------------------------------------------
# the scratch the entry points share
# ---------------------------------------------------------------------------------------------------------------------
def test_hist2d_kde2d_hist2d_on_one_engine(engine, lib, n_cu):
    """hist2d's integer bins, kde2d's slabs and weighted_stats' partial sums all live in ctx->scratch: interleaved, each
    call gives the bits it gave the first time, and those are the reference's."""
    by = {r["name"]: r for r in fr.CASES}
    hrow, wrow, krow = by["hist-91x91-global"], by["hist-w-signed-lds"], by["kde-130x70-plain"]
    hd, wd, kd = fr.hist_data(hrow, n_cu), fr.hist_data(wrow, n_cu), fr.kde_indicator(krow, n_cu)
    sx, sw, _ = fr.wstats_exact(9001, True, 1)

    def hist(d):
        xy = engine.to_device(np.stack([d["x"], d["y"]], axis=1))
        return _hist_call(engine, lib, d, xy.ptr, 2, xy.ptr + 8, 2, "interleaved")

    ops = {"hist": lambda: hist(hd), "kde": lambda: _kde_call(engine, lib, kd, krow, "interleaved"),
           "whist": lambda: hist(wd), "wstats": lambda: _wstats(engine, sx, sw, "1d")}
    first = {}
    for name in ("hist", "kde", "hist", "whist", "kde", "wstats", "whist", "hist", "wstats", "kde"):
        out = ops[name]()
        if name in first:
            np.testing.assert_array_equal(out, first[name], err_msg=name)
        first.setdefault(name, out)
    np.testing.assert_array_equal(first["hist"], fr.hist_counts(hd))
    np.testing.assert_array_equal(first["whist"], fr.hist_weighted(wd)[0])
    np.testing.assert_array_equal(first["kde"], kd["density"])
