"""The launch rules of csrc/fes.hip restated, the exact references and the case table behind
tests/test_gpu_fes_paths.py (CPU only): every row of the table reaches the branch it names on devices of 256, 304 and
64 compute units, the rows together cover every branch the rules can report, every "exact" generator keeps its own
exactness condition (so the GPU comparison needs no tolerance), and the references agree with straightforward
evaluations."""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import pytest

from tests import _fes_ref as fr

LD = np.longdouble


def test_rules_on_the_shapes_worked_out_by_hand():
    H = fr.hist2d_path
    # bins + edges within 64 KiB of dynamic LDS: (nx + 1)(ny + 1) <= 8191
    assert H(100, 89, 90, False, 256)["lds_bins"] and not H(100, 90, 90, False, 256)["lds_bins"]
    assert H(100, 89, 90, False, 256)["lds_bytes"] == 65528 and H(100, 90, 90, True, 256)["lds_bytes"] == 1456
    assert H(100, 69, 69, False, 256)["lds_bytes"] == (69 * 69 + 140) * 8
    # edge tables: (nx + ny + 2) doubles within 64 KiB, else no dynamic LDS at all
    assert H(100, 8189, 1, False, 256)["lds_edges"] and H(100, 8189, 1, False, 256)["lds_bytes"] == 65536
    assert not H(100, 8190, 1, False, 256)["lds_edges"] and H(100, 8190, 1, False, 256)["lds_bytes"] == 0
    assert all(H(100, nx, ny, w, 256)["lds_bytes"] <= fr.HIST_LDS_BYTES
               for nx, ny in ((1, 1), (89, 90), (90, 90), (4096, 4096), (1 << 24, 1), (1, 1 << 24), (8189, 1), (4095, 4095))
               for w in (False, True))
    assert H(100, 4097, 4096, False, 256) == {"status": "invalid"} and H(0, 5, 5, True, 256)["kernel"] == "none"
    # 2048 frames per workgroup, at most 4 per compute unit
    assert [H(n, 5, 5, False, 256)["grid"] for n in (1, 2048, 2049, 2048 * 1024, 2048 * 1024 + 1, 10 ** 7)] == \
        [1, 1, 2, 1024, 1024, 1024]
    assert not H(2048 * 1024, 5, 5, False, 256)["capped"] and H(2048 * 1024 + 1, 5, 5, False, 256)["capped"]
    assert not H(256, 5, 5, False, 256)["second_round"] and H(257, 5, 5, False, 256)["second_round"]
    K = fr.kde_path
    assert (K(1, 1, 1, 256)["gx"], K(1, 1, 1, 256)["tail_lanes"], K(1, 1, 1, 256)["idle_waves"]) == (1, 1, True)
    assert [K(n, 16, 17, 256)["tail_lanes"] for n in (1, 3, 4, 5, 4095)] == [1, 3, 4, 1, 3]
    assert (K(8192, 64, 64, 256)["gx"], K(8192, 64, 64, 256)["iters"]) == (512, 1) and K(8193, 64, 64, 256)["iters"] == 2
    p = K(4095, 130, 70, 256)
    assert (p["nby"], p["nbz"], p["gx"], p["iters"], p["c_sum"]) == (3, 2, 85, 4, 16 + 3 + 85)
    assert K(10, 4097, 5, 256) == {"status": "invalid"} and K(10 ** 6, 4096, 4096, 256)["gx"] == 1
    W = fr.wstats_path
    assert (W(4096, 256)["nb"], W(4097, 256)["nb"], W(4097, 256)["per"]) == (1, 2, 2049)
    assert W(4096 * 511 + 1, 256)["nb"] == 512 and W(10 ** 8, 256)["nb"] == 512 and W(4096 * 511, 256)["nb"] == 511
    # no block of msm_weighted_stats is ever empty: nb per - n < nb <= per whenever nb > 1
    for n_cu in fr.N_CU_CHECKED:
        for n in list(range(1, 20000, 37)) + [4096 * k + j for k in (1, 2, 127, 2 * n_cu - 1, 2 * n_cu, 5 * n_cu) for j in (-1, 0, 1)]:
            assert not W(n, n_cu)["empty_block"], (n, n_cu)
    F = fr.flat_path
    assert F(0, 256) == {"kernel": "none"} and F(1024, 256)["blocks"] == 1 and F(1025, 256)["blocks"] == 2
    assert not F(2048 * 1024, 256)["capped"] and F(2048 * 1024 + 1, 256)["capped"]


@pytest.mark.parametrize("n_cu", fr.N_CU_CHECKED)
def test_every_row_reaches_the_branch_it_names(n_cu):
    for row in fr.CASES:
        assert row["reach"], row["name"]
        miss = fr.covers(fr.row_path(row, n_cu), row["reach"])
        assert not miss, (n_cu, row["name"], miss)
    by = {r["name"]: r for r in fr.CASES}
    # an edited row is noticed
    for name, change in (("hist-89x90-last-lds", {"nx": 90}), ("hist-90x90-first-global", {"ny": 89}),
                         ("hist-8190x1-first-global-edges", {"nx": 8189}), ("hist-grid-capped", {"n": ("cu", 4 * 2048, 0)}),
                         ("hist-past-one-round-of-the-largest-grid", {"n": 200}),
                         ("kde-second-iteration-64x64", {"n": ("cu", 32, 0)}), ("kde-130x70", {"nx": 128}),
                         ("kde-n5-16x17", {"n": 8}), ("wstats-n4097", {"n": 4096}),
                         ("wstats-every-block", {"n": ("cu", 2 * 4096, -4096)}), ("flat-grid-capped", {"n": ("cu", 8 * 1024, 0)}),
                         ("finalize-n1025", {"n": 1024})):
        row = dict(by[name], **change)
        assert fr.covers(fr.row_path(row, n_cu), row["reach"]), (name, change)


@pytest.mark.parametrize("n_cu", fr.N_CU_CHECKED)
def test_the_table_covers_every_branch_of_the_rules(n_cu):
    hist = [(r, fr.row_path(r, n_cu)) for r in fr.rows("hist")]
    live = [(r, p) for r, p in hist if p["kernel"] == "hist2d"]
    for weighted in (False, True):
        mine = [(r, p) for r, p in live if p["weighted"] == weighted]
        assert {(p["lds_bins"], p["lds_edges"]) for _, p in mine} == {(True, True), (False, True), (False, False)}
        assert any(p["second_round"] and p["multi_block"] for _, p in mine) and any(not p["second_round"] for _, p in mine)
        assert any(p["kernel"] == "none" for r, p in hist if (r["weights"] is not None) == weighted)
    assert any(p["capped"] for _, p in live)
    assert {fr.resolve(r["n"], n_cu) for r, _ in hist} >= {0, 1, 2047, 2049, 4 * n_cu * 256 + 1}
    assert {(r["nx"], r["ny"]) for r, _ in hist} >= {(1, 1), (1, 7), (7, 1), (9000, 1), (1, 9000)}
    for kind in ("plain", "signed", "cancel", "tiny", "over"):        # every weight family on both bin placements
        assert {p["lds_bins"] for r, p in live if r["weights"] == kind} == {False, True}, kind
    for edges in ("geom", "geom_down", "repeat", "repeat_last"):
        assert {p["lds_bins"] for r, p in live if edges in (r["xedges"], r["yedges"])} == {False, True}, edges
    assert {p["lds_bins"] for r, p in live if r["xy"]} == {False, True}
    kde = [(r, fr.row_path(r, n_cu)) for r in fr.rows("kde")]
    assert {fr.resolve(r["n"], n_cu) for r, _ in kde} >= {1, 3, 4, 5, 4095}
    assert {(r["nx"], r["ny"]) for r, _ in kde} >= {(1, 1), (16, 17), (64, 64), (65, 64), (130, 70)}
    assert {p["tail_lanes"] for _, p in kde} == {1, 2, 3, 4} and {r["periodic"] for r, _ in kde} == {0, 1, 2, 3}
    assert any(p["loops"] and p["blocks"] == 1 for _, p in kde) and any(p["multi_slab"] and p["blocks"] > 1 for _, p in kde)
    assert any(p["loops"] and "smooth" in r["families"] for r, p in kde) or n_cu > 256
    assert any(p["idle_waves"] for _, p in kde) and {p["clamped"] for _, p in kde} == {False, True}
    assert any(not r["weights"] and r["w_scale"] != 1.0 for r, _ in kde)
    assert {(r["cols"], r["d"], r["periodic"]) for r, _ in kde} >= {((3, 1), 4, m) for m in range(4)}
    ws = [(r, fr.row_path(r, n_cu)) for r in fr.rows("wstats")]
    assert {p["nb"] for _, p in ws} >= {1, 2, 2 * n_cu} and {r["layout"] for r, _ in ws} == {"1d", "column"}
    assert {fr.resolve(r["n"], n_cu) for r, _ in ws} >= {1, 4096, 4097} and {r["weighted"] for r, _ in ws} == {False, True}
    assert {tuple(r["shape"]) for r in fr.rows("smooth")} == {(1, 1), (1, 9), (9, 1), (17, 33), (5, 40)}
    assert {r["n"] for r in fr.rows("finalize")} == {1, 1024, 1025, 70_000} and {r["n"] for r in fr.rows("scale")} == {1, 1025}
    flat = [fr.row_path(r, n_cu) for r in fr.rows("flat")]
    assert any(p["kernel"] == "none" for p in flat) and {p.get("capped") for p in flat} >= {False, True}
    assert any(fr.resolve(r["n"], n_cu) == 8 * n_cu * 256 + 1 for r in fr.rows("flat"))


def test_histogram_generators_and_references():
    n_cu = 64
    for row in fr.rows("hist"):
        if fr.resolve(row["n"], n_cu) > 100_000:
            continue                                       # the same generator, only longer; the GPU test runs it
        d = fr.hist_data(row, n_cu)
        nx, ny = row["nx"], row["ny"]
        assert len(d["x"]) == len(d["y"]) == d["n"] and len(d["xe"]) == nx + 1 and np.all(np.diff(d["xe"]) >= 0)
        ix, iy = fr.edge_bin(d["xe"], d["x"]), fr.edge_bin(d["ye"], d["y"])
        ok = (ix >= 0) & (iy >= 0)
        mine = np.zeros((nx, ny))
        np.add.at(mine, (ix[ok], iy[ok]), 1.0)
        np.testing.assert_array_equal(mine, fr.hist_counts(d), err_msg=row["name"])     # edge_bin is np.histogram2d's rule
        if d["n"] >= 400:
            assert ok.sum() > d["n"] // 16 and (~ok).sum() > 0, row["name"]
        if d["n"] >= 2000 and row["weights"] != "cancel":      # the special values are all there
            for e, v in ((d["xe"], d["x"]), (d["ye"], d["y"])):
                assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
                for edge in (e[0], e[-1]) + ((e[len(e) // 2],) if len(e) <= 200 else ()):
                    assert (v == edge).any() and (v == np.nextafter(edge, np.inf)).any() and (v == np.nextafter(edge, -np.inf)).any()
        if "geom" in (row["xedges"], row["yedges"]) and nx > 1 and ny > 1 and nx < 200:   # both corrections walk far
            for e, v, i in ((d["xe"], d["x"], ix), (d["ye"], d["y"], iy)):
                nb = len(e) - 1
                with np.errstate(invalid="ignore"):
                    guess = np.clip(((v - e[0]) * (nb / (e[-1] - e[0]))), 0, nb - 1).astype(int)
                step = (i - guess)[i >= 0]
                assert (step.max() > nb // 3 and step.min() >= 0) or (step.min() < -nb // 3 and step.max() <= 0), row["name"]
        if row["weights"] is None:
            continue
        exact, true, bound, cnt, e = fr.hist_weighted(d)
        w = d["w"]
        assert d["w_absmax"] >= np.abs(w).max(initial=0.0) and max(1, d["n"]) * d["w_absmax"] * 2.0 ** e < 2.0 ** 62
        assert max(1, d["n"]) * d["w_absmax"] * 2.0 ** e >= 2.0 ** 60            # e is the largest such exponent
        np.testing.assert_array_equal(cnt, mine)
        assert np.all(np.abs(exact - true) <= bound), row["name"]
        # Python integers give the same sums
        py = [[0] * ny for _ in range(nx)]
        for k in np.nonzero(ok)[0][:3000]:
            py[ix[k]][iy[k]] += int(np.rint(w[k] * 2.0 ** e))
        if ok.sum() <= 3000:
            np.testing.assert_array_equal(exact, np.array([[float(v) for v in r] for r in py]) * 2.0 ** -e)
        if row["weights"] == "cancel":
            assert np.count_nonzero(exact) <= 1 and np.abs(w).sum() > 100 and cnt.sum() > 1000
        if row["weights"] == "tiny":
            small = np.abs(w) < 2.0 ** -30
            assert small.sum() > d["n"] // 3 and np.all(np.rint(w[small] * 2.0 ** e) != 0)
            assert np.any(np.rint(w * 2.0 ** e) != w * 2.0 ** e)                  # the rounding is a real one
        if row["weights"] == "over":
            assert d["w_absmax"] >= 1024 * np.abs(w).max()
        if row["weights"] == "signed":
            assert (w < 0).any() and (w > 0).any()
    # the exponent refuses a product next to a power of two, and pick_w_absmax moves away from one
    with pytest.raises(AssertionError):
        fr.hist_exponent(1024, 1.0)
    a = fr.pick_w_absmax(1024, 1.0)
    assert a > 1.0 and fr.hist_exponent(1024, a) == 61 - 11


def test_kde_generators_keep_their_exactness_condition():
    n_cu = 64
    for row in fr.rows("kde"):
        d = fr.kde_indicator(row, n_cu)              # asserts factor == 1 or 0 itself, in long double
        n = d["n"]
        assert d["density"].shape == (row["nx"], row["ny"]) and (d["w"] is None) == (not row["weights"])
        total = (n if d["w"] is None else d["w"].sum()) * d["w_scale"]
        assert abs(d["density"].sum() / fr.kde_normaliser(*d["bw"]) - total) <= 1e-9 * total
        assert d["density"][row["nx"] - 1, row["ny"] - 1] > 0 or n == 1
        if n >= 100:
            assert not np.array_equal(d["x"], d["y"])
            if row["nx"] == row["ny"] > 1:
                assert not np.array_equal(d["density"], d["density"].T)
        if row["periodic"] & 1 and n >= 100:
            assert np.abs(d["x"]).max() > 2 * np.pi and (np.abs(d["y"]).max() > 2 * np.pi) == bool(row["periodic"] & 2)
        # the indicator density is the plain formula: the long-double evaluation rounds to the same numbers
        if n <= 1100:
            ref, _ = fr.kde_reference(d, row["periodic"], 1, 8)
            np.testing.assert_allclose(d["density"], ref.astype(np.float64), rtol=1e-14, atol=0)
    # a swapped periodic bit, a frame off its centre and centres that are too close are all refused or seen
    row = dict(next(r for r in fr.rows("kde") if r["name"] == "kde-cols-3-1-periodic1"))
    d = fr.kde_indicator(row, n_cu)
    swapped, _ = fr.kde_reference(d, 2, 1, 8)
    assert not np.allclose(swapped.astype(np.float64), d["density"], rtol=1e-6)
    u = fr.device_differences(d["xc"], d["x"] + 1e-6, True) / d["bw"][0]
    assert not np.all((np.abs(u) >= 39.0) | (0.5 * u * u < 2.0 ** -60))


def test_kde_smooth_reference_is_the_formula():
    row = {"name": "t", "n": 57, "nx": 7, "ny": 5, "periodic": 3, "weights": True, "w_scale": 0.3, "seed": 1}
    d = fr.kde_smooth(row, 64)
    for per in (0, 1, 2, 3):
        dens, bound = fr.kde_reference(d, per, 9, 8)
        want = np.zeros((7, 5))
        for i in range(7):
            for j in range(5):
                for k in range(57):
                    dx, dy = d["xc"][i] - d["x"][k], d["yc"][j] - d["y"][k]
                    if per & 1:
                        dx = (dx + math.pi) % (2 * math.pi) - math.pi
                    if per & 2:
                        dy = (dy + math.pi) % (2 * math.pi) - math.pi
                    want[i, j] += d["w"][k] * 0.3 * math.exp(-0.5 * (dx / d["bw"][0]) ** 2 - 0.5 * (dy / d["bw"][1]) ** 2)
        want /= 2 * math.pi * d["bw"][0] * d["bw"][1]
        np.testing.assert_allclose(dens.astype(np.float64), want, rtol=1e-12, atol=1e-300)
        assert np.all(bound > 0) and np.all(bound >= dens * 17 * 2.0 ** -52) and np.all(bound < dens * 1e-11 + 1e-300)


def test_weighted_stats_generators_and_references():
    for row in fr.rows("wstats"):
        n = fr.resolve(row["n"], 64)
        x, w, out = fr.wstats_exact(n, row["weighted"], row["seed"])      # asserts its condition itself
        assert len(x) == n and (w is None) == (not row["weighted"]) and np.all(x == np.rint(x))
        wl = (np.ones(n) if w is None else w).astype(LD)
        mean = (wl * x).sum() / wl.sum()
        assert out[2] == float(mean) == np.rint(out[2]) and out[0] == float(wl.sum()) and out[1] == float((wl * wl).sum())
        assert abs(LD(out[3]) - (wl * (x - mean) ** 2).sum() / wl.sum()) <= 1e-15 * out[3]
        assert (out[4], out[5]) == (x.min(), x.max()) and (n < 50 or out[3] > 0)
    rng = np.random.default_rng(2)
    x, w = rng.normal(3.0, 2.0, 500), rng.gamma(2.0, 1.0, 500)
    vals, bounds = fr.wstats_reference(x, w)
    assert abs(vals[2] - np.average(x, weights=w)) <= bounds[2] and abs(vals[3] - np.average((x - vals[2]) ** 2, weights=w)) <= bounds[3]
    assert abs(vals[0] - w.sum()) <= bounds[0] and abs(vals[1] - (w * w).sum()) <= bounds[1]
    assert np.all(bounds[:4] < 1e-12 * np.abs(vals[:4]))


def test_small_kernel_references():
    h = np.array([[0.0, 8.0, 0.0], [16.0, 0.0, 24.0]])
    out, cnt = fr.smooth_reference(h, 1.0)
    # cell (0, 0): its replicated neighbours are (0,0) x3 (itself twice more), (0,1) x2, (1,0) x2, (1,1)
    assert out[0, 0] == (0 * 3 + 8 * 2 + 16 * 2 + 0) / 8.0 and out[0, 1] == 8.0 and cnt == 3
    out, cnt = fr.smooth_reference(np.zeros((4, 4)), 5.0)
    assert cnt == 0 and not out.any()
    out, cnt = fr.smooth_reference(np.array([[3.0]]), 5.0)            # 1 x 1: the mean of 8 copies of itself, then >= 5
    assert cnt == 1 and out[0, 0] == 5.0
    out, cnt = fr.smooth_reference(h, 0.0)
    assert cnt == 0 and np.array_equal(out, h)
    assert [fr.finalize_status(np.array(v)) for v in ([1.0, 2.0], [1.0, np.nan], [1.0, np.inf], [1.0, -np.inf], [1.0, 0.0],
                                                      [3.0, -1.0], [-3.0, -1.0], [0.0, 0.0], [6e299, 6e299],
                                                      [2e300, -2e300, 1.0])] == [0, 3, 3, 7, 4, 4, 6, 6, 2, 5]
    F, bound = fr.finalize_reference(np.array([1.0, 2.0, 5.0]), 2.5)
    np.testing.assert_allclose(F.astype(np.float64), -2.5 * np.log(np.array([0.2, 0.4, 1.0])), rtol=1e-14, atol=1e-15)
    assert F.min() == 0 and np.all(bound < 1e-13)
    x = fr.flat_specials(-1.5, 2.0)
    c = fr.clip_reference(x, -1.5, 2.0)
    assert np.isnan(c[np.isnan(x)]).all() and np.nanmin(c) == -1.5 and np.nanmax(c) == 2.0
    wr = fr.wrap_reference(x, -1.5, 2.0)
    fin = np.isfinite(x)
    assert np.all((wr[fin] >= -1.5) & (wr[fin] <= 2.0)) and np.isnan(wr[~fin]).all()
    x0 = fr.flat_specials(0.0, 1.0)
    assert x0[6] == -1e-20 and fr.wrap_reference(x0, 0.0, 1.0)[6] == 1.0    # the remainder rounds up to the span: numpy's result
    for v, r in zip(x[fin], wr[fin]):                                 # the remainder of the rounded x - lo is exact
        q = Fraction(float(np.float64(v) - -1.5)) % Fraction(7, 2)
        assert float(q) == float(Fraction(float(q))) and r == float(q) + -1.5, (v, r)
    np.testing.assert_array_equal(fr.gather_reference([1.5, 2.5], [0, 1, -1, 2, -2 ** 31, 2 ** 31 - 1]), [1.5, 2.5, 0, 0, 0, 0])
