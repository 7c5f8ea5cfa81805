"""The restated k-means dispatch rule, the shape table and the adversarial generators behind
tests/test_gpu_kmeans_fp64_paths.py (CPU only): the rule agrees with the documented constants, the table reaches every
instantiation of kmeans_mfma_kernel and both sides of each threshold, and the generators make the ties they promise
(checked with the oracle alone, so the GPU tests cannot pass vacuously)."""

from __future__ import annotations

import itertools

import numpy as np
import pytest

from tests import _kmeans_ref as kr

ALL_ROWS = kr.ASSIGN_ROWS + kr.ACCUM_ROWS + kr.CHILD_ROWS


def _paths(rows, accumulate=None):
    return [kr.row_path(r, accumulate=accumulate) for r in rows]


def test_rule_agrees_with_the_documented_constants():
    assert kr.LDS_BUDGET == 150 * 1024 and kr.LDS_ACC_LIMIT == 64 * 1024 and kr.D_MAX == 256
    assert kr.KS_LADDER == (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)
    caps = [kr.single_tile_capacity(ks) for ks in kr.KS_LADDER]
    assert caps == [3792, 2112, 1456, 1120, 752, 576, 384, 288, 192, 144, 96, 64]
    for ks, cap in zip(kr.KS_LADDER, caps):
        p = kr.dispatch("f64", 1000, 4 * ks, cap, False, filter_on=False)
        assert (p["KS"], p["MULTI"], p["tile_k"], p["FOLD"]) == (ks, 0, cap, 0)
        q = kr.dispatch("f64", 1000, 4 * ks, cap + 1, False, filter_on=False)
        assert q["MULTI"] == 1 and q["tile_k"] % 32 == 0 and q["tile_k"] == (cap & ~31) and q["lds"] <= kr.LDS_BUDGET
        assert kr.dispatch("f32", 1000, 4 * ks + 1, 20, False, filter_on=False)["kernel"] == ("fp64" if ks < 64 else "unsupported")
    assert kr.dispatch("f64", 10, 257, 3, True)["kernel"] == "unsupported"
    # NF, workgroup size, prefetch, recovery
    for ks in kr.KS_LADDER:
        p = kr.dispatch("f32", 5000, 4 * ks, 33, False, filter_on=False)
        assert p["NF"] == (2 if ks <= 16 else 1) and p["MT"] == (1024 if ks <= 4 else 512)
        assert p["prefetch"] == (ks in (6, 8, 12, 16)) and p["recovery"] == ("lds" if ks <= 8 else "global")
        assert p["grid"] == min(-(-p["n_units"] // (p["MT"] // 64)), kr.N_CU)
    # LDS accumulators: k (d + 1) * 8 <= 64 KiB, taken out of the tile budget
    a, b = kr.dispatch("f64", 900, 15, 512, True), kr.dispatch("f64", 900, 15, 513, True)
    assert (a["lds_acc"], b["lds_acc"]) == (1, 0) and a["lds"] == 32 * kr.tile_bytes(4) + 65536
    assert kr.dispatch("f64", 900, 97, 83, True)["MULTI"] == 1 and kr.dispatch("f64", 900, 97, 83, False)["MULTI"] == 0
    # the filter: d <= 10 while its tables (and the member sums) fit 160 KiB - 64
    assert kr.dispatch("f32", 900, 10, 1312, False)["kernel"] == "filter"
    assert kr.dispatch("f32", 900, 10, 1313, False)["kernel"] == "fp64"
    assert kr.dispatch("f32", 900, 4, 1504, False)["kernel"] == "filter" and kr.dispatch("f32", 900, 4, 1505, False)["KS"] == 1
    assert kr.dispatch("f32", 900, 11, 20, False)["kernel"] == "fp64"
    assert kr.dispatch("f32", 900, 10, 20, False, filter_on=False)["KS"] == 3
    assert kr.dispatch("f64", 900, 10, 500, True)["kernel"] == "filter"


def test_debug_lines_of_the_rule():
    p = kr.dispatch("f32", 1000, 45, 200, True)
    assert kr.debug_line(p) == ("msm_kmeans: fp64 T=f32 n=1000 d=45 k=200 KS=12 NF=2 MT=512 ACCUM=1 FOLD=1 MULTI=0 tile_k=208 "
                                f"lds_acc=0 grid=4 lds={13 * 785 * 8}")
    assert kr.debug_line(kr.dispatch("f64", 64, 4, 9, False)) == "msm_kmeans: filter T=f64 n=64 d=4 k=9 ACCUM=0"
    assert kr.debug_lines("x\nmsm_kmeans: filter T=f64\nmsm_spectrum: y\n") == ["msm_kmeans: filter T=f64"]


def test_assign_table_reaches_every_instantiation_in_both_dtypes():
    got = {kr.instantiation(p) for p in _paths(kr.ASSIGN_ROWS + kr.CHILD_ROWS) if p["kernel"] == "fp64" and not p["ACCUM"]}
    want = set(itertools.product(("f32", "f64"), kr.KS_LADDER, (0,), (0, 1), (0, 1)))
    assert want <= got, sorted(want - got)
    # in the parent process alone too (filter on): the child only adds the small-k forms of KS = 1, 2, 3
    got_parent = {kr.instantiation(p) for p in _paths(kr.ASSIGN_ROWS) if p["kernel"] == "fp64"}
    assert want <= got_parent, sorted(want - got_parent)
    assert all(p["kernel"] == "fp64" for p in _paths(kr.ASSIGN_ROWS + kr.ACCUM_ROWS + kr.CHILD_ROWS))


def test_accumulate_table_reaches_every_reachable_combination():
    rows = kr.ACCUM_ROWS + [r for r in kr.CHILD_ROWS if r["accum"]]
    paths = _paths(rows)
    got = {(p["KS"], p["FOLD"], p["MULTI"], p["lds_acc"]) for p in paths}
    want = set(itertools.product(kr.KS_LADDER, (0, 1), (0, 1), (0, 1)))
    missing = want - got
    # what is missing is unreachable by the rule, for the reason given: no (d, k) of that KS step, with the filter on or
    # off, gives the combination (exhaustive scan in reachable_accumulate)
    assert missing == set(kr.UNREACHABLE_ACCUM), (sorted(missing), sorted(kr.UNREACHABLE_ACCUM))
    assert all(m == 1 and l == 1 for _, _, m, l in missing), f"{sorted(missing)}: {kr.UNREACHABLE_REASON}"
    print(f"unreachable (KS, FOLD, MULTI, lds_acc): {sorted(missing)} -- {kr.UNREACHABLE_REASON}")
    # every instantiation <T, KS, ACCUM = 1, FOLD, MULTI> is launched: the fit runs every row in both dtypes
    inst = {(p["KS"], p["FOLD"], p["MULTI"]) for p in paths}
    assert inst == set(itertools.product(kr.KS_LADDER, (0, 1), (0, 1)))
    # fit needs n >= k
    assert all(kr.row_n(r) >= r["k"] for r in rows)


def test_table_reaches_both_sides_of_every_threshold():
    rows = kr.ASSIGN_ROWS + kr.CHILD_ROWS
    paths = _paths(rows)
    ds = {r["d"] for r in rows} | {r["d"] for r in kr.ACCUM_ROWS}
    for ks in kr.KS_LADDER:
        assert 4 * ks in ds and (4 * ks + 1 in ds or ks == 64), ks
        cap = kr.single_tile_capacity(ks)
        assert any(p["KS"] == ks and p["k"] == cap and not p["MULTI"] and p["tile_k"] == cap for p in paths), ks
        assert any(p["KS"] == ks and p["k"] == cap + 1 and p["MULTI"] for p in paths), ks
    acc = _paths(kr.ACCUM_ROWS)
    assert any(p["k"] * (p["d"] + 1) == 8192 and p["lds_acc"] for p in acc)
    assert any((p["k"] - 1) * (p["d"] + 1) == 8192 and not p["lds_acc"] for p in acc)
    single = [p for p in paths if not p["MULTI"]]
    multi = [p for p in paths if p["MULTI"]]
    assert any(p["k"] % 16 for p in single) and any(p["k"] % 16 for p in multi)
    assert any(p["tiles"] % 2 == 1 and p["tiles"] >= 3 and p["recovery"] == "lds" for p in single)
    assert any(p["tiles"] % 2 == 1 and p["tiles"] >= 3 and p["recovery"] == "global" for p in single)
    assert any(p["last_tiles"] == 1 for p in multi)
    assert any(p["last_tiles"] % 2 == 1 and p["last_tiles"] >= 3 for p in multi)
    assert any(p["last_tiles"] % 2 == 0 for p in multi) and any(p["chunks"] >= 3 for p in multi)
    assert any(p["k"] == 1 for p in paths) and any(1 < p["k"] < 16 for p in paths)
    for prefetch in (True, False):
        ns = {p["n"] for p in paths if p["prefetch"] == prefetch}
        assert {1, 15, 16, 17, 31, 32, 33} <= ns, (prefetch, sorted(ns)[:12])
        assert any(p["n"] == 16 * p["NF"] - 1 for p in paths if p["prefetch"] == prefetch)
    # frame-group hand-out: units_per_block rounds up and trailing workgroups are idle, on each loop body; a chunked
    # launch with several strides per wave and a ragged tail -- for any CU count
    for n_cu in (256, 304, 64):
        grid = [(r, kr.row_path(r, n_cu)) for r in rows if isinstance(r["n"], tuple)]
        for loop in ("narrow", "wide"):
            assert any(not p["MULTI"] and p["loop"] == loop and p["grid"] == n_cu
                       and p["units_per_block"] * p["grid"] > p["n_units"] + p["units_per_block"]
                       and p["n_units"] == n_cu * p["waves"] + 1 for _, p in grid), (n_cu, loop)
        assert any(p["MULTI"] and p["n_units"] > 2 * p["grid"] * p["waves"] and p["n_units"] % (p["grid"] * p["waves"])
                   and p["n"] % (16 * p["NF"]) for _, p in grid), n_cu
    # the oracle's cost per call stays bounded
    for r in ALL_ROWS:
        assert kr.row_n(r, 304) * r["d"] * r["k"] <= 2e9, r["name"]
    assert len({r["name"] for r in ALL_ROWS}) == len(ALL_ROWS)


def test_adversarial_shapes_take_the_recoveries_they_name():
    for what, (n, d, k) in kr.ADVERSARIAL_SHAPES.items():
        for dt in ("f32", "f64"):
            p = kr.dispatch(dt, n, d, k, False)
            assert p["kernel"] == "fp64" and p["MULTI"] == (what == "multi")
            assert p["recovery"] == ("lds" if what == "lds" else "global")
    assert [kr.dispatch("f64", n, d, k, False)["KS"] for n, d, k in kr.CANCELLATION_SHAPES] == [12, 32, 64]


@pytest.mark.parametrize("rows", [kr.ASSIGN_ROWS, kr.ACCUM_ROWS, kr.CHILD_ROWS], ids=["assign", "accumulate", "child"])
def test_tie_generator_makes_exact_ties_at_every_placement(rows):
    """Generator 1, with the oracle alone: a frame is tied iff its label under the reversed centre order does not map
    back.  Every placement of every row must own tied frames, and at least 10 % of all frames are tied."""
    seen: dict[str, int] = {}
    tied = total = 0
    for i, r in enumerate(rows):
        if "ties" not in r["gens"]:
            continue
        p = kr.row_path(r)
        X, C, pl = kr.ties(min(kr.row_n(r), 400), r["d"], r["k"], p["tile_k"], kr.DTYPES[r["dtype"]], seed=i)
        counts = kr.placement_tie_counts(X, C, pl)
        for name, _, _ in pl:
            assert counts[name] > 0, f"{r['name']}: no tied frame at placement {name}: {counts}"
            seen[name] = seen.get(name, 0) + counts[name]
        if r["k"] >= 2:
            assert counts["_tied"] >= 0.1 * counts["_n"], (r["name"], counts)
        tied += counts["_tied"]
        total += counts["_n"]
    want = {"same_lane", "other_lane", "pair_ab", "pair_ab_rows", "two_pairs", "odd_last_tile", "into_odd_last_tile", "k_minus_1"}
    if any(kr.row_path(r)["MULTI"] for r in rows):
        want |= {"two_chunks", "first_last_chunk", "in_last_chunk"}
    assert want <= set(seen), f"placements without a tied frame: {sorted(want - set(seen))}; tied frames per placement: {seen}"
    assert tied >= 0.1 * total, (tied, total)
    print(f"tied frames per placement: {seen}; {tied} of {total} frames tied")


@pytest.mark.parametrize("rows", [kr.ASSIGN_ROWS, kr.CHILD_ROWS], ids=["assign", "child"])
def test_near_tie_generator_makes_near_ties(rows):
    """Generator 2: for at least 10 % of the frames the two smallest oracle distances differ by < 1e-12 relative (a
    property of the input, computed with numpy in fp64), and they are not exact duplicates."""
    fracs = []
    for i, r in enumerate(rows):
        if "near" not in r["gens"] or r["k"] < 2:
            continue
        p = kr.row_path(r, accumulate=False)
        X, C, pl = kr.near(min(kr.row_n(r), 400), r["d"], r["k"], p["tile_k"], kr.DTYPES[r["dtype"]], seed=i)
        assert pl and all(not np.array_equal(C[lo], C[hi]) for _, lo, hi in pl), r["name"]
        frac = kr.near_tie_fraction(X, C)
        assert frac >= 0.1, f"{r['name']}: only {frac:.3f} of the frames are near ties"
        fracs.append(frac)
    print(f"near-tie share: min {min(fracs):.3f}, mean {np.mean(fracs):.3f} over {len(fracs)} rows")


def test_other_generators_hold_what_they_promise():
    for dt in (np.float32, np.float64):
        sets = kr.nonfinite(300, 29, 50, dt, seed=1)
        X = sets[0][0]
        assert np.isnan(X[11]).all() and np.isnan(X[10]).sum() == 1 and np.isinf(X[12]).sum() == 1 and not X[18].any()
        assert any(np.isnan(c).any() for _, c in sets) and any(np.isinf(c).any() for _, c in sets)
        assert any((~c.any(axis=1)).any() for _, c in sets)
        X, C = kr.cancellation(500, 45, 20, dt, seed=2)
        assert abs(X.mean() - 1000.0) < 0.01 and X.std() < 0.02
        X, C, mean, std = kr.whitening(500, 29, 20, dt, seed=3)
        assert std.max() / std.min() >= 1e11 and np.abs(mean).min() >= 1e3
    # with the 1e200 frame several centres tie at -inf (an overflowing dot product): the oracle names the first
    from oracle import cport

    X, C = kr.nonfinite(300, 29, 50, np.float64, seed=1)[4]
    tied, fwd, rev = kr.tied_frames(X[14:15], C)
    assert tied[0] and fwd[0] < rev[0]


def test_restated_lloyd_pass_equals_the_oracle_fit():
    from oracle import cport

    rng = np.random.default_rng(0)
    n, d, k = 2000, 7, 23
    X = rng.normal(size=(n, d))
    want, _, scale = cport.kmeans_fit(X, k, seed=9, max_iter=3, tol2=0.0)
    C = X[kr.stratified_frames(n, k, 9)].copy()
    for _ in range(3):
        _, _, _, C = kr.member_sums(X, C, scale)
    np.testing.assert_array_equal(C, want)
