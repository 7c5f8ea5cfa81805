"""The exact references, the restated launch rule of csrc/moments.hip and the case table behind
tests/test_gpu_moments_paths.py (CPU only): every row of the table reaches the branch it names on devices of 256, 304
and 64 compute units with 1 to 8 resident workgroups each, the rows together cover every branch the rule can report,
every generator keeps its own exactness condition (so the GPU comparison needs no tolerance), and the references agree
with straightforward long-double evaluations on random data."""

from __future__ import annotations

import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import _moments_ref as mr

LD = np.longdouble


def test_rule_on_the_shapes_worked_out_by_hand():
    P = mr.project_path
    # the W' image: (17 F16 + 16) doubles within 48 KiB, so F16 = 352 is the last matrix-core shape
    assert P(100, 352, 16, "f32", 352, 0, False, 256, 6)["kernel"] == "mfma_vec"
    assert P(100, 353, 16, "f32", 353, 0, False, 256, 6)["kernel"] == "generic"
    assert P(100, 337, 3, "f64", 337, 0, False, 256, 6)["kernel"] == "mfma_scalar"
    assert P(100, 16, 17, "f32", 16, 0, False, 256, 6)["kernel"] == "generic"
    # the generic kernel's LDS is (64 * 65 + 64 d) doubles: exactly 48 KiB at d = 31, so the opt-in starts at d = 32
    assert [P(100, 16, d, "f32", 16, 0, False, 256, 6)["lds_opt_in"] for d in (17, 30, 31, 32, 64)] == \
        [False, False, False, True, True]
    # vector loads: F a multiple of 16, ld and the base a multiple of 4 elements; FINITE only exists with them
    assert P(100, 32, 3, "f32", 32, 0, True, 256, 6)["finite"] and P(100, 32, 3, "f64", 36, 4, False, 256, 6)["vec"]
    for ld, off, why in ((33, 0, ("ld",)), (34, 0, ("ld",)), (32, 1, ("base",)), (32, 2, ("base",)), (35, 3, ("ld", "base"))):
        p = P(100, 32, 3, "f32", ld, off, True, 256, 6)
        assert (p["kernel"], p["vec_off_by"], p["finite"]) == ("mfma_scalar", why, False)
    # chunks of 64 features; dead q slots when F16 is no multiple of 64
    assert [(P(16, F, 1, "f32", F, 0, False, 256, 6)["n_chunks"], P(16, F, 1, "f32", F, 0, False, 256, 6)["dead_q"])
            for F in (16, 48, 64, 80, 128, 352)] == [(1, True), (1, True), (1, False), (2, True), (2, False), (6, True)]
    # one group of 16 frames per wave, 4 waves per workgroup, n_cu * per_cu workgroups at most
    assert P(65, 16, 3, "f32", 16, 0, False, 256, 6)["grid"] == 2 and P(65, 16, 3, "f32", 16, 0, False, 256, 6)["tail"]
    assert not P(16 * 4 * 256 * 6, 16, 3, "f32", 16, 0, False, 256, 6)["loops"]
    assert P(16 * 4 * 256 * 6 + 1, 16, 3, "f32", 16, 0, False, 256, 6)["loops"]
    assert P(300_001, 16, 3, "f32", 16, 0, False, 304, 8)["loops"] and P(300_001, 16, 3, "f32", 16, 0, False, 585, 8)["loops"]
    assert not P(300_001, 16, 3, "f32", 16, 0, False, 586, 8)["loops"]
    assert not P(64 * 8 * 256, 16, 17, "f32", 16, 0, False, 256, 1)["loops"]
    assert P(64 * 8 * 256 + 1, 16, 17, "f32", 16, 0, False, 256, 1)["loops"]
    assert P(0, 16, 3, "f32", 16, 0, False, 256, 6) == {"kernel": "none"}
    # moments
    assert [mr.pick_tf(F) for F in (1, 2, 3, 4, 5, 255, 256, 257, 513)] == [1, 2, 4, 4, 8, 256, 256, 256, 256]
    M = mr.moments_path
    assert (M(100_000, 10, 256)["rp"], M(100_000, 10, 256)["blocks"]) == (16, 390)
    assert M(10 ** 6, 256, 256)["blocks"] == 1024 and M(10 ** 6, 256, 64)["blocks"] == 256
    assert M(31, 256, 256)["blocks"] == 1 and M(32, 256, 256)["blocks"] == 2
    # minmax
    assert mr.minmax_path(10, 4097, 256) == {"status": "invalid"} and mr.minmax_path(10, 4096, 256)["status"] == "ok"
    assert not mr.minmax_path(256 * 8 * 256, 2, 256)["second_row"] and mr.minmax_path(256 * 8 * 256 + 1, 2, 256)["second_row"]
    assert all(mr.minmax_path(700_000, 2, n_cu)["second_row"] for n_cu in mr.N_CU_CHECKED)


@pytest.mark.parametrize("n_cu", mr.N_CU_CHECKED)
def test_every_row_reaches_the_branch_it_names(n_cu):
    for row in mr.CASES:
        assert row["reach"], row["name"]
        for per_cu, finite in itertools.product(mr.PER_CU_CHECKED, (False, True)):
            p = mr.row_path(row, n_cu, per_cu, finite)
            want = dict(row["reach"])
            if not mr.loop_is_forced(row, n_cu, per_cu):      # a second-round row on a device too large for its n
                assert p["loops"] is False, row["name"]
                del want["loops"]
            elif want.get("loops"):
                assert n_cu > 312 or p["loops"] is True, (row["name"], n_cu, per_cu)
            if want.get("kernel") == "mfma_vec":
                assert p["finite"] == finite, row["name"]
            miss = mr.covers(p, want)
            assert not miss, (n_cu, per_cu, row["name"], miss)
    # an edited row is noticed: the same check on rows that were moved off their branch
    by = {r["name"]: r for r in mr.CASES}
    for name, change in (("vec-F48-n17-d3-f64", {"ld": 50}), ("vec-F48-n17-d3-f64", {"n": 32}),
                         ("vec-F48-n17-d3-f64", {"F": 64, "ld": 64}), ("generic-F70-d32-n17-f32", {"d": 31}),
                         ("vec-second-round-F16", {"n": 16 * 4 * 64}), ("scalar-F16-ld18-off0-n16-d16-f32", {"ld": 20}),
                         ("moments-F257-n70-f32", {"F": 256})):
        row = dict(by[name], **change)
        assert mr.covers(mr.row_path(row, n_cu, 8), row["reach"]), (name, change)


@pytest.mark.parametrize("n_cu", mr.N_CU_CHECKED)
def test_the_table_covers_every_branch_of_the_rule(n_cu):
    proj = [(r, mr.row_path(r, n_cu, 6)) for r in mr.project_rows()]
    kernels = ("mfma_vec", "mfma_scalar", "generic")
    for kernel, dtype in itertools.product(kernels, ("f32", "f64")):
        mine = [(r, p) for r, p in proj if p["kernel"] == kernel and r["dtype"] == dtype]
        assert {r["n"] for r, _ in mine} >= {1, 15, 16, 17, 63, 64, 65}, (kernel, dtype)
        assert {r["mean2"] for r, _ in mine} == {False, True}, (kernel, dtype)
        assert any(r["ldw"] > r["d"] for r, _ in mine) and any(r["ldy"] > r["d"] for r, _ in mine), (kernel, dtype)
        assert any(r["ld"] > r["F"] for r, _ in mine), (kernel, dtype)
        assert {p["tail"] for _, p in mine} == {False, True}, (kernel, dtype)
        assert {p["pad_features"] for _, p in mine} == ({False} if kernel == "mfma_vec" else {False, True}), (kernel, dtype)
        if kernel == "mfma_vec":
            assert {p["dead_q"] for _, p in mine} == {False, True} and {p["n_chunks"] for _, p in mine} >= {1, 2, 6}
            assert any(r["off"] for r, _ in mine), dtype
        if kernel == "mfma_scalar":
            assert {p["vec_off_by"] for _, p in mine} >= {("F",), ("ld",), ("base",)}, dtype
        if kernel == "generic":
            assert {p["lds_opt_in"] for _, p in mine} == {False, True} and any(p["wide_F"] for _, p in mine), dtype
            assert {p["n_chunks"] for _, p in mine} >= {1, 2, 3}, dtype
        if dtype == "f64":
            assert any(r["family"] == "fp64_only" for r, _ in mine), kernel
    for kernel in kernels:                          # a second round on every kernel (f32 keeps the buffers small)
        assert any(p["loops"] for _, p in proj if p["kernel"] == kernel), kernel
    assert any(p["loops"] and p["n_chunks"] >= 2 and p["dead_q"] for _, p in proj)
    assert any(p.get("idle_waves") for _, p in proj)
    assert {r["d"] for r, _ in proj} >= {1, 3, 16, 17, 30, 31, 64}
    assert {r["F"] for r, _ in proj} >= {1, 15, 16, 17, 48, 64, 80, 128, 352, 368}
    assert {r["F"] for r, p in proj if p["kernel"] == "generic" and p["wide_F"]} >= {353, 368}
    # moments: every step of pick_tf, every block structure
    mom = [(r, mr.row_path(r, n_cu)) for r in mr.moments_rows()]
    assert {r["F"] for r, _ in mom} >= {1, 2, 3, 255, 256, 257, 513} and {p["tf"] for _, p in mom} >= {1, 2, 4, 16, 64, 256}
    assert {p["f_passes"] for _, p in mom} == {1, 2, 3}
    for key in ("idle_lanes", "n_lt_rp", "unrolled", "remainder", "ragged", "capped", "multi_block"):
        assert {p[key] for _, p in mom} == {False, True}, key
    assert any(r["n"] == 1 for r, _ in mom)
    for dtype in ("f32", "f64"):
        sub = [r for r, _ in mom if r["dtype"] == dtype]
        assert {r["shift"] for r in sub} == {False, True} and any(r["ld"] > r["F"] for r in sub)
        assert {(r["shift"], r["ld"] > r["F"]) for r in sub} == set(itertools.product((False, True), repeat=2)), dtype
    assert {r["family"] for r, _ in mom} == {"small", "wide", "fp64_only"}


def test_generators_keep_their_exactness_condition():
    peak_proj, peak_mom = 0.0, {}
    for row in mr.project_rows():
        if row["n"] > 100_000 and row["F"] > 16:
            continue                                  # the same generator at 100 MB: the GPU test asserts it when it runs
        X, mu, isg, m2, W = mr.project_data(row)     # asserts peak < 2^(53 - g) itself
        g, peak = mr.project_exactness(X, mu, isg, m2, W, row["d"])
        assert g <= 7 and peak < 2.0 ** (53 - g), (row["name"], g, peak)
        assert X.shape == (row["n"], row["F"]) and W.shape == (row["F"], row["ldw"])
        assert np.all(W[:, row["d"]:] == mr.SENTINEL) and (m2 is None) == (not row["mean2"])
        assert np.any(isg != 1.0) and np.any(W[:, :row["d"]] != 0.0)
        peak_proj = max(peak_proj, peak)
        if row["family"] == "fp64_only":             # narrowing the input is visible in the reference
            Y = mr.exact_project(X, mu, isg, m2, W, row["d"])
            Y32 = mr.exact_project(X.astype(np.float32).astype(np.float64), mu, isg, m2, W, row["d"])
            assert np.abs(X).max() == mr.BIG and not np.array_equal(Y, Y32), row["name"]
    assert peak_proj > 2.0 ** 24                      # an fp32 accumulator cannot hold these
    for row in mr.moments_rows():
        X, shift = mr.moments_data(row)              # asserts the column sums of squares < 2^53 itself
        assert X.shape == (row["n"], row["F"]) and (shift is None) == (not row["shift"])
        used = mr.implicit_shift(X) if shift is None else shift
        peak = mr.moments_exactness(X, used)
        assert peak < 2.0 ** 53, row["name"]
        peak_mom[row["family"]] = max(peak_mom.get(row["family"], 0.0), peak)
        if row["family"] == "fp64_only":
            a, _ = mr.exact_column_sums(X, shift)
            b, _ = mr.exact_column_sums(X.astype(np.float32).astype(np.float64), shift)
            assert not np.array_equal(a, b), row["name"]
    assert peak_mom["wide"] > 2.0 ** 24 and peak_mom["fp64_only"] > 2.0 ** 50, peak_mom
    # the condition is a real one: data outside it are refused
    bad = dict(mr.project_rows()[0], n=4, F=16, d=3, ldw=3, family="small", mean2=True, dtype="f32", seed=1)
    X, mu, isg, m2, W = mr.project_data(bad)
    g, peak = mr.project_exactness(X * 2.0 ** 44, mu, isg, m2, W, 3)
    assert not peak < 2.0 ** (53 - g)
    with pytest.raises(AssertionError):
        mr.project_exactness(X, mu, isg * 3.0, m2, W, 3)
    with pytest.raises(AssertionError):
        mr.moments_exactness(X + 0.5, np.zeros(16))


def test_exact_project_agrees_with_long_double():
    rng = np.random.default_rng(3)
    n, F, d = 23, 37, 5
    X = rng.standard_normal((n, F))
    X[4, 0] = X[7, F - 1] = X[9, :] = np.nan
    mu, isg, m2, W = rng.standard_normal(F), rng.uniform(0.5, 2.0, F), rng.standard_normal(F), rng.standard_normal((F, d + 2))
    for m in (m2, None):
        want = np.zeros((n, d), LD)
        for t, c in itertools.product(range(n), range(d)):
            acc = LD(0)
            for f in range(F):
                z = LD(0) if np.isnan(X[t, f]) else (LD(X[t, f]) - LD(mu[f])) * LD(isg[f])
                if m is not None:
                    z -= LD(m[f])
                acc += z * LD(W[f, c])
            want[t, c] = acc
        got = mr.exact_project(X, mu, isg, m, W, d)
        scale = np.abs(X[~np.isnan(X)]).max() * np.abs(W).max() * F * 4
        assert np.abs(got - want).max() <= 8 * F * 2.0 ** -53 * scale
    # integers: the same bits
    row = dict(mr.project_rows()[0], n=19, F=33, d=4, ldw=6, family="small", mean2=True, dtype="f32", seed=5)
    X, mu, isg, m2, W = mr.project_data(row)
    X[3, 2] = np.nan
    want = [[float(sum(((0 if np.isnan(X[t, f]) else Fraction(X[t, f]) - Fraction(mu[f])) * Fraction(isg[f]) - Fraction(m2[f]))
                       * Fraction(W[f, c]) for f in range(33))) for c in range(4)] for t in range(19)]
    np.testing.assert_array_equal(mr.exact_project(X, mu, isg, m2, W, 4), np.array(want))
    # an inf or a NaN row stays in its row
    Xi = np.where(np.isnan(X), 0.0, X)
    base = mr.exact_project(Xi, mu, isg, m2, W, 4)
    Xi2 = Xi.copy()
    Xi2[5, 7] = np.inf
    other = np.arange(19) != 5
    np.testing.assert_array_equal(mr.exact_project(Xi2, mu, isg, m2, W, 4)[other], base[other])


def test_column_sums_finalize_and_standardise_agree_with_long_double():
    rng = np.random.default_rng(9)
    n, F = 211, 7
    X = rng.standard_normal((n, F)) * rng.uniform(0.1, 30.0, F) + rng.standard_normal(F) * 100.0
    X[0, 1] = X[5, 2] = X[n - 1, 2] = np.nan
    X[:, 4] = np.nan
    X[1:, 5] = np.nan
    X[:, 6] = 2.5
    for shift in (None, rng.standard_normal(F)):
        sums, used = mr.exact_column_sums(X, shift)
        assert used[1] == (0.0 if shift is None else shift[1])
        for f in range(F):
            col = X[~np.isnan(X[:, f]), f].astype(LD) - LD(used[f])
            assert sums[f] == len(col)
            assert abs(LD(sums[F + f]) - col.sum()) <= 1e-13 * max(np.abs(col).sum(), 1) if len(col) else sums[F + f] == 0
            assert abs(LD(sums[2 * F + f]) - (col * col).sum()) <= 1e-13 * max((col * col).sum(), 1) if len(col) else True
        for ddof in (0, 1):
            mean, std, cnt = mr.finalize(sums, used, ddof)
            np.testing.assert_array_equal(cnt, sums[:F])
            for f in range(F):
                col = X[~np.isnan(X[:, f]), f].astype(LD)
                if len(col) == 0:
                    assert mean[f] == 0.0 and std[f] == 0.0
                    continue
                assert abs(LD(mean[f]) - col.mean()) <= 1e-13 * abs(col.mean()) + 1e-13
                if len(col) - ddof <= 0:
                    assert np.isnan(std[f])
                else:
                    ref = np.sqrt(((col - col.mean()) ** 2).sum() / LD(len(col) - ddof))
                    # the sums are rounded: the variance the formula sees is off by some 2^-52 (S2 + S1^2 / cnt) / denom
                    slack = math.sqrt(2.0 ** -48 * (sums[2 * F + f] + sums[F + f] ** 2 / len(col)) / (len(col) - ddof))
                    assert abs(LD(std[f]) - ref) <= 1e-9 * float(ref) + slack, (f, std[f], ref)
        mean, scale, inv = mr.standardise(sums, used, n, True)
        fm, fs, _ = mr.finalize(sums, used, 0)
        np.testing.assert_array_equal(mean, fm)
        np.testing.assert_array_equal(inv, 1.0 / scale)
        assert scale[4] == 1.0 and mean[4] == 0.0                       # no entry at all
        for f in (0, 3):                                                # every entry present: the population std
            assert abs(scale[f] - fs[f]) <= 2.0 ** -50 * fs[f]
        assert abs(scale[2] - fs[2] * math.sqrt((n - 2) / n)) <= 1e-12 * fs[2]     # NaNs count in the divisor
        m0, s0, i0 = mr.standardise(sums, used, n, False)
        np.testing.assert_array_equal(s0, 1.0)
        np.testing.assert_array_equal(m0, mean)
    # a constant column has scale 1 (exactly zero variance about its own first row)
    sums, used = mr.exact_column_sums(X, None)
    assert mr.standardise(sums, used, n, True)[1][6] == 1.0 and mr.finalize(sums, used, 0)[1][6] == 0.0
    # sqrt_rounded is the correctly rounded root
    for q in (Fraction(2), Fraction(1, 3), Fraction(10 ** 30 + 1), Fraction(7, 10 ** 20), Fraction(9, 4)):
        c = mr.sqrt_rounded(q)
        lo, hi = math.nextafter(c, 0.0), math.nextafter(c, math.inf)
        assert ((Fraction(lo) + Fraction(c)) / 2) ** 2 <= q <= ((Fraction(c) + Fraction(hi)) / 2) ** 2
    assert mr.sqrt_rounded(Fraction(9, 4)) == 1.5 and mr.sqrt_rounded(Fraction(0)) == 0.0
    lo, hi = mr.std_interval(np.array([10.0, 3.0, 50.0]), 0, 1, 9)
    assert lo < mr.sqrt_rounded(mr.variance(np.array([10.0, 3.0, 50.0]), 0, 1, 9)) < hi and hi - lo < 1e-14


def test_minmax_reference():
    X = np.array([[1.0, -0.0, np.nan, np.inf, -5e-324], [-2.0, 0.0, np.nan, -np.inf, 5e-324], [np.nan, 0.0, np.nan, 3.0, 0.0]])
    mn, mx, cnt = mr.minmax(X)
    np.testing.assert_array_equal(mn, [-2.0, 0.0, np.nan, 3.0, -5e-324])
    np.testing.assert_array_equal(mx, [1.0, 0.0, np.nan, 3.0, 5e-324])
    assert cnt.tolist() == [6, 0]
    mn, mx, cnt = mr.minmax(np.zeros((0, 3)))
    assert np.all(np.isnan(mn)) and np.all(np.isnan(mx)) and cnt.tolist() == [0, 0]
