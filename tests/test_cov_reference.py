"""The exact covariance reference, the restated launch rule of csrc/cov.hip and the case table behind
tests/test_gpu_cov_paths.py (CPU only): the reference agrees with oracle/npport.py and with a triple loop, every row of
the table reaches the branch it names on devices of 256, 304 and 64 compute units, the rows together cover every launch
path, and every generator keeps all partial sums exact in fp64 (so the GPU comparison needs no tolerance)."""

from __future__ import annotations

import itertools

import numpy as np
import pytest

from oracle import npport
from tests import _cov_ref as cr


def _paths(n_cu):
    rows = [cr.resolve(r, n_cu) for r in cr.CASES]
    return rows, [cr.row_path(r, n_cu) for r in rows]


def _assert_same(a: dict, b: dict, exact: bool, tag):
    assert a["T"] == b["T"], tag
    for k in ("M00", "M0t", "sx", "sy"):
        if exact:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag} {k}")
        else:
            np.testing.assert_allclose(a[k], b[k], rtol=1e-12, atol=1e-12 * np.abs(b["M00"]).max(), err_msg=f"{tag} {k}")


@pytest.mark.parametrize("integers", [False, True])
def test_exact_moments_agree_with_the_oracle_and_a_triple_loop(integers):
    rng = np.random.default_rng(5)
    n, F = 61, 5
    X = rng.integers(-9, 10, size=(n, F)).astype(np.float64) if integers else rng.standard_normal((n, F))
    shift = rng.integers(-3, 4, size=F).astype(np.float64) if integers else rng.standard_normal(F)
    segs = [(-4, 9), (9, 11), (13, 30), (30, 33), (40, 90)]
    for lag, flavour in itertools.product((0, 1, 2, 3, 7, 20), cr.FLAVOURS):
        got = cr.exact_moments(X, segs, lag, shift, flavour)
        _assert_same(got, cr.brute_moments(X, segs, lag, shift, flavour), integers, ("brute", lag, flavour))
        if lag == 0:
            continue                      # npport slices X[:-lag]: empty at lag 0
        m = npport.lagged_moments([X[a:b] - shift for a, b in cr.clip_segments(n, segs)], lag)
        if flavour == "onesided":         # the oracle has the reversible M00 only: take x'x from its parts
            m00 = sum((X[a:b - lag] - shift).T @ (X[a:b - lag] - shift) for a, b in cr.clip_segments(n, segs) if b - a > lag)
        else:
            m00 = m["Mxx"]
        m0t = m["Mxy_half"] if flavour != "symmetric" else (m["Mxy_half"] + m["Mxy_half"].T) / 2.0
        _assert_same(got, {"M00": m00, "M0t": m0t, "sx": m["sx"], "sy": m["sy"], "T": m["T"]}, integers,
                     ("npport", lag, flavour))
    # lag 0 is the instantaneous covariance: x = y = every frame of every segment
    z = np.concatenate([X[a:b] for a, b in cr.clip_segments(n, segs)]) - shift
    got = cr.exact_moments(X, segs, 0, shift, "plain")
    _assert_same(got, {"M00": 2 * z.T @ z, "M0t": z.T @ z, "sx": z.sum(0), "sy": z.sum(0), "T": len(z)}, integers, "lag0")
    np.testing.assert_array_equal(cr.exact_moments(X, segs, 0, shift, "onesided")["M00"], got["M0t"])


def test_nan_imputation_and_column_sums():
    X, shift = cr.small(40, 4, 1)
    segs = [(0, 17), (20, 23), (25, 40)]
    Xn = X.copy()
    Xn[3, 2] = Xn[16, 0] = Xn[39, 3] = np.nan
    with pytest.raises(ValueError):
        cr.exact_moments(Xn, segs, 2, shift)
    Xz = np.where(np.isnan(Xn), shift[None, :], Xn)          # NaN -> 0 after centring == the value of the shift
    for flavour in cr.FLAVOURS:
        _assert_same(cr.exact_moments(Xn, segs, 2, shift, flavour, impute_nan=True),
                     cr.exact_moments(Xz, segs, 2, shift, flavour), True, flavour)
    # the identity msm_moments_from_lagged uses: 2 S1 = sx + sy + edges, 2 S2 = diag(M00) + edges^2 (plain flavour)
    for lag in (1, 2, 3, 5, 20):
        m = cr.exact_moments(X, segs, lag, shift, "plain")
        e1, e2 = np.zeros(4), np.zeros(4)
        for a, b in segs:
            z = np.concatenate([X[a:min(a + lag, b)], X[max(b - lag, a):b]]) - shift
            e1 += z.sum(0)
            e2 += (z * z).sum(0)
        want = np.concatenate([np.full(4, 35.0), (m["sx"] + m["sy"] + e1) / 2, (np.diag(m["M00"]) + e2) / 2])
        np.testing.assert_array_equal(cr.exact_column_sums(X, segs, shift), want)


def test_rule_on_the_shapes_worked_out_by_hand():
    """One segment, lag 1: 97, 113 and 124 frames fill one workgroup and give ring lengths {6, 7}, {7, 8}, {6, 7, 8} on
    any device; from 125 frames on a second workgroup halves the chunks; the long rings are device-dependent."""
    for n_cu in cr.N_CU_CHECKED:
        for n, ring in ((97, {6, 7}), (113, {7, 8}), (124, {6, 7, 8})):
            p = cr.cov_path(n, 64, 64, 4, True, None, 1, "plain", n_cu)
            assert p["blocks"] == 1 and cr.reached(p, 1)["ring"] == ring, (n_cu, n, p["blocks"], cr.reached(p, 1)["ring"])
        for n in (125, 160, 300, 1031):
            p = cr.cov_path(n, 64, 64, 4, True, None, 1, "plain", n_cu)
            assert cr.reached(p, 1)["ring"] == set() and all(q["head"] + q["short"] + q["tail"] in (4, 5, 6)
                                                             for q in p["pieces"][:-1]), (n_cu, n)
    for n, ring in ((36869, {7, 9, 10}), (45059, {8, 11, 12}), (49154, {12, 13})):
        assert cr.reached(cr.cov_path(n, 64, 64, 4, True, None, 1, "plain", 256), 1)["ring"] == ring
    # the guarded kernels have no ring; NT = 3 is never a vector kernel; the symmetric kernel exists for split tiles
    for F, NT in ((16, 1), (32, 2), (48, 3), (64, 4)):
        p = cr.cov_path(124, F, F, 4, True, None, 1, "symmetric", 256)
        assert (p["NT"], p["vec"], p["split"], p["sym_kernel"], p["symmetrise"]) == (NT, NT != 3, NT >= 3, NT >= 3, NT < 3)
        assert not cr.cov_path(124, F - 1, F, 4, True, None, 1, "plain", 256)["vec"]
        assert cr.cov_path(124, F, F, 8, False, None, 1, "plain", 256)["vec"] == (NT == 1)   # one element off
        assert cr.cov_path(124, F, F + 1, 8, True, None, 1, "plain", 256)["vec"] == (NT == 1)
    assert not cr.cov_path(124, 64, 2 ** 27, 4, True, None, 1, "plain", 256)["vec"]           # 32-bit lane offsets
    assert cr.cov_path(124, 64, 2 ** 27 - 4, 4, True, None, 1, "plain", 256)["vec"]
    # the blocked kernel: tasks and chunks
    p = cr.cov_path(100_000, 129, 129, 4, True, None, 1, "plain", 256)
    assert (p["n_fb"], p["n_tasks"], p["chunks"], p["vec"]) == (3, 15, 34, False)
    # segments: 16 are the most a call takes, the short ones do not count
    segs = [(10 * i, 10 * i + 5) for i in range(17)]
    assert cr.cov_path(200, 8, 8, 4, True, segs, 1, "plain", 256)["status"] == "unsupported"
    assert cr.cov_path(200, 8, 8, 4, True, segs[:16] + [(190, 191)], 1, "plain", 256)["n_live"] == 16
    assert cr.cov_path(200, 8, 8, 4, True, segs, 5, "plain", 256) == {"status": "empty", "pairs": 0}


@pytest.mark.parametrize("n_cu", cr.N_CU_CHECKED)
def test_every_row_reaches_the_branch_it_names(n_cu):
    rows, paths = _paths(n_cu)
    for row, p in zip(rows, paths):
        assert p["status"] == "ok", row["name"]
        assert row["reach"], row["name"]
        miss = cr.covers(cr.reached(p, row["lag"]), row["reach"])
        assert not miss, (n_cu, row["name"], miss)
        # the partition covers every padded frame exactly once
        covered = sum(q["o_e"] - q["o_b"] for q in p["pieces"])
        assert covered == p["total"] and all(q["o_b"] % 4 == 0 and q["o_e"] % 4 == 0 for q in p["pieces"]), row["name"]
        assert sum(4 * (q["head"] + q["ring"] + q["short"] + q["tail"]) for q in p["pieces"]) == p["total"], row["name"]


@pytest.mark.parametrize("n_cu", cr.N_CU_CHECKED)
def test_the_table_covers_every_launch_path(n_cu):
    rows, paths = _paths(n_cu)
    got = [(r, p, cr.reached(p, r["lag"])) for r, p in zip(rows, paths)]
    fused = [(r, p, g) for r, p, g in got if not p["blocked"]]
    for NT in (1, 2, 3, 4):
        mine = [(r, p, g) for r, p, g in fused if p["NT"] == NT]
        assert {p["vec"] for _, p, _ in mine} == ({False} if NT == 3 else {False, True}), NT
        for vec in {p["vec"] for _, p, _ in mine}:
            sub = [r for r, p, _ in mine if p["vec"] == vec]
            assert {r["flavour"] for r in sub} == set(cr.FLAVOURS), (NT, vec)
            assert {r["dtype"] for r in sub} == {"f32", "f64"}, (NT, vec)
            assert {(r["flavour"], r["dtype"]) for r in sub} >= {(f, d) for f in cr.FLAVOURS for d in ("f32", "f64")} \
                or not vec, (NT, vec)
            assert any(r["ld"] > r["F"] for r in sub), (NT, vec)
        assert any(not r["aligned"] for r, _, _ in mine), NT
    # the ring: every residue mod 3, at exactly 2 * depth and with two and more trips of the steady loop; each of these
    # in every vector kernel (NT = 1, 2, 4), flavour and dtype
    for NT, flavour, dtype in itertools.product((1, 2, 4), cr.FLAVOURS, ("f32", "f64")):
        rings = set().union(*[g["ring"] for r, p, g in fused
                              if p["NT"] == NT and r["flavour"] == flavour and r["dtype"] == dtype])
        assert 6 in rings and {x % 3 for x in rings} == {0, 1, 2}, (NT, flavour, dtype, rings)
    for NT in (1, 2, 4):
        rings = set().union(*[g["ring"] for _, p, g in fused if p["NT"] == NT])
        assert {x % 3 for x in rings if x >= 9} == {0, 1, 2}, (NT, rings)
    long_sym = set().union(*[g["ring"] for _, p, g in fused if p["sym_kernel"]])
    assert {x % 3 for x in long_sym if x >= 9} == {0, 1, 2}, long_sym
    shorts = set().union(*[g["short"] for _, _, g in fused])
    assert shorts and all(1 <= s < 6 for s in shorts), shorts
    vecs = [(r, p, g) for r, p, g in fused if p["vec"]]
    assert any(g["mid_start"] and g["ring"] for _, _, g in vecs)          # a chunk starting inside the head, then a ring
    assert any(g["mid_start"] and not g["ring"] for _, _, g in vecs)
    assert any(g["span"] >= 3 for _, _, g in vecs) and any(g["span"] >= 3 for r, p, g in fused if not p["vec"])
    assert any(g["tiny_seg"] for _, _, g in vecs)
    assert any(g["lag_gt_fpw"] for _, _, g in vecs)
    assert any(g["n_live"] == cr.SEG_INLINE for _, _, g in vecs)
    # lengths and lags in every residue class mod 4, on the vector kernels and over all rows
    for sub in (vecs, got):
        assert {q["len"] % 4 for _, p, _ in sub for q in p["pieces"]} == {0, 1, 2, 3}
        assert {r["lag"] % 4 for r, _, _ in sub} == {0, 1, 2, 3}
    assert any(r["lag"] == 0 for r, _, _ in vecs) and any(r["lag"] == 0 for r, p, _ in fused if p["vec"] and p["split"])
    live = lambda r: [(a, b) for a, b in cr.clip_segments(r["n"], r["segs"]) if b - a > r["lag"]]   # noqa: E731
    assert any(any(b - a == r["lag"] + 1 for a, b in live(r)) for r, _, _ in vecs)           # one pair
    assert any(len(live(r)) < len([1 for a, b in cr.clip_segments(r["n"], r["segs"]) if b > a]) for r, _, _ in vecs)
    assert any(r["segs"] and any(a < 0 for a, _ in r["segs"]) and any(b > r["n"] for _, b in r["segs"]) for r, _, _ in got)
    assert any(r["segs"] and any(r["segs"][i + 1][0] > r["segs"][i][1] for i in range(len(r["segs"]) - 1))
               for r, _, _ in vecs)                                                          # gaps
    # the blocked kernel
    blocked = [(r, p) for r, p, _ in got if p["blocked"]]
    assert {(p["n_fb"], p["vec"]) for _, p in blocked} == {(2, False), (2, True), (3, False), (3, True)}
    assert {r["F"] for r, _ in blocked} >= {65, 100, 128, 129}
    assert {r["flavour"] for r, _ in blocked} == set(cr.FLAVOURS) and {r["dtype"] for r, _ in blocked} == {"f32", "f64"}
    assert any(r["ld"] > r["F"] and p["vec"] for r, p in blocked) and any(not r["aligned"] for r, _ in blocked)
    # every family in both kernels
    assert {r["family"] for r, p, _ in fused} == set(cr.FAMILIES) == {r["family"] for r, _ in blocked}


def test_generators_keep_every_partial_sum_exact():
    """|partial sum| <= the same moment of |z| < 2^52: integers (and the halves the kernel's half-weighted M00 and the
    symmetric flavour's (S - M00) / 2 make of them) of that size are fp64 numbers, so any summation order is exact."""
    peak = {}
    for row in (cr.resolve(r, max(cr.N_CU_CHECKED)) for r in cr.CASES):      # the largest device: the longest rows
        X, shift = cr.case_data(row)
        assert X.shape == (row["n"], row["F"]) and np.all(X == np.rint(X)) and np.all(shift == np.rint(shift))
        Xt = X.astype(cr.NP_DTYPE[row["dtype"]])
        assert np.array_equal(Xt.astype(np.float64), X), row["name"]           # the row's dtype holds the data exactly
        bound = cr.magnitude_bound(X, row["segs"], row["lag"], shift)
        assert bound < 2.0 ** 52, (row["name"], bound)
        peak[row["family"]] = max(peak.get(row["family"], 0.0), bound)
        if row["family"] == "fp64_only":       # narrowing the input is visible in the reference
            a = cr.exact_moments(X, row["segs"], row["lag"], shift, row["flavour"])
            b = cr.exact_moments(X.astype(np.float32).astype(np.float64), row["segs"], row["lag"], shift, row["flavour"])
            assert not np.array_equal(a["M00"], b["M00"]) and not np.array_equal(a["sx"] + a["sy"], b["sx"] + b["sy"])
    assert peak["wide"] > 2.0 ** 24 and peak["fp64_only"] > 2.0 ** 50, peak   # fp32 accumulation cannot hold these
    X, _ = cr.small(50, 3, 0)
    assert np.array_equal(X[:, 1], np.arange(50) % 5) and np.abs(X).max() <= 4
    m = cr.exact_moments(X, None, 1, np.zeros(3))
    assert not np.array_equal(m["M0t"], m["M0t"].T)
