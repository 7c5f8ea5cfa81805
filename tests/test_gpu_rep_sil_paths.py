"""Every launch path of pmarlo_amd/csrc/representatives.hip and silhouette.hip through the C ABI, against the longdouble
laws of tests/_rep_sil_paths_ref.py (checked on the CPU by tests/test_rep_sil_paths_reference.py, which also measures
what plain fp64 numpy loses against them and asserts the margins behind every exact comparison of picks).

Bounds (u = 2^-53; derivations in test_gpu_representatives.py and test_gpu_silhouette.py): grouping and picks exact;
centroid coordinate 2 n_s u max|x|, weight sum n_s u relative; centroid distance 4 n_s u sqrt(d) max|x| for every state
size; medoid score 4 (n_s + d) u relative; silhouette samples atol 1e-10, score rtol 1e-10.  Every comparison prints
its measured maximum next to the bound.  Rows are `ld` apart with NaN in the padding columns; every output holds 0x5A
bytes before the call, so a word a kernel does not write shows up.

group_rank / group_scan_chunks / group_offsets / group_place_kernel
  test_group_by_label                       one chunk, a chunk and one frame, 64 chunks and the carry of the scan (65, 131
                                            chunks), k = 1 .. 257 (a partial workgroup of four waves, 65 workgroups),
                                            labels -1, k, INT32_MAX, a state in every chunk, one only in the last, one
                                            without a frame; members past offsets[k] untouched; two runs, same bytes
  test_group_smaller_call_after_a_larger    the scratch still holds the larger histogram
state_centroid_kernel
  test_centroids                            cw = d and d rounded up, R = 256 .. 1, states of 0, 1, R - 1, R, R + 1, 1000
                                            members, ld = d, d + 1, d + 1000, with and without weights
  test_centroid_flags                       every flag alone and combined in a state that is not first; neighbours and
                                            an empty state report 0
centroid_score_kernel
  test_centroid_scores                      the same d and ld, total no multiple of 256 and below n
medoid_score_kernel
  test_medoid_scores                        odd d (the zero-filled slot), partial feature chunks, states of 1 .. 257
                                            members, a list that is unsorted, names a state twice and omits one
  test_medoid_without_work                  n_states = 0 and total = 0: MSM_OK, nothing written
  test_medoid_second_launch                 16 500 members at d = 256: 127 tasks in the first launch, 2 in the second
select_smallest_kernel / select_diverse_kernel
  test_select                               n_states 1 and 300, n_reps 1 .. 600 against states of 0 .. 1000 members: the
                                            -1 tail at every position, the fill loops past index 256
  test_select_ties_go_to_the_lowest_frame   duplicated lattice points, equal scores
  test_select_preset_scores                 all NaN, one NaN, +inf among finite, all +inf, signed zeros
  test_select_nan_features                  the "every value NaN" exit of the diverse walk; all-NaN scores start at 0
  test_picker_nan_rule                      the same rule through RepresentativePicker
  test_select_refuses_bad_state_lists       repeated / out of range: MSM_ERR_INVALID, picks untouched
  test_full_path_exact_picks                centroids, scores and selection chained on strided rows
silhouette_kernel (k <= 32) / mean_kernel
  test_silhouette_sorted                    k x d x n crossed: k = 2 .. 32, d = 1 .. 128 (48 / 64 KiB of LDS), n = 2 .. 1000,
                                            an empty cluster between occupied ones, a singleton, clusters of 64 and 65;
                                            msm_silhouette_samples on the same points
  test_silhouette_refusals                  d = 129, k = 33, k = 1
silhouette_pairs_kernel / silhouette_fold_kernel / mean_partial_kernel / mean_final_kernel
  test_silhouette_samples_paths             ld > d, queries past the last tile (n = 3, 127, 128, 129), d = 1, 7, 8, 9,
                                            16 / 17 singletons in a row (kGroupSegs), groups of 1024 / 1025 rows, a
                                            1024-row group cut into launches of 5, 5 and 1 tiles; the same bytes for
                                            every cut
both silhouette entry points
  test_non_finite_coordinates               a NaN / +inf coordinate in a middle cluster, a NaN in a singleton
  test_finite_input_keeps_its_bits          tests/golden/silhouette_before_nan_rule.npz
  test_public_score_of_nan_features_is_nan  clustering.silhouette_score / silhouette_samples: the value the scan refuses
capture
  test_capture_replays_the_linear_sequence  group, centroids, centroid scores: one stream, same bytes on replay
  test_capture_refusals                     medoid scores, select, silhouette samples, a grouping that must grow the
                                            scratch: MSM_ERR_UNSUPPORTED, and the capture still ends and replays

Not reached by any small shape, so not tested: the `ge - gl < 65535` grid limit of msm_silhouette_samples and the
n > 2^31 - 1 refusals."""

from __future__ import annotations

import time

import numpy as np
import pytest

from pmarlo_amd import _lib
from tests import _rep_sil_paths_ref as P

pytestmark = pytest.mark.gpu

U = P.U
OK, INVALID, UNSUPPORTED = _lib.MSM_OK, _lib.MSM_ERR_INVALID, _lib.MSM_ERR_UNSUPPORTED


def _junk(engine, shape, dtype):
    return engine.empty(shape, dtype).fill_bytes_(0x5A)


def _is_junk(a):
    a = np.ascontiguousarray(a)
    return bool((a.view(np.uint8) == 0x5A).all())


def _report(name, err, bound):
    print(f"{name}: measured {err:.3e}, bound {bound:.3e}")
    assert err <= bound, name


def _upload_groups(engine, labels, k):
    """The law's grouping on the device: (labels, offsets, members padded to n with junk), and the host offsets."""
    offsets, members = P.group_ref(labels, k)
    d_mem = _junk(engine, (labels.size,), np.int32)
    if members.size:
        d_mem.view((members.size,)).copy_from_host(members)
    return engine.to_device(labels), engine.to_device(offsets), d_mem, offsets, members


# ---- grouping ------------------------------------------------------------------------------------------------------
def _group(engine, labels, k):
    n = labels.size
    d_lab = engine.to_device(labels)
    d_off, d_mem = _junk(engine, (k + 1,), np.int64), _junk(engine, (n,), np.int32)
    assert P.c_group(engine, d_lab, n, k, d_off, d_mem) == OK
    return d_off.to_host(), d_mem.to_host()


@pytest.mark.parametrize("k", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("n", [1023, 1024, 1025, 64 * 1024, 64 * 1024 + 1, 130 * 1024 + 7])
def test_group_by_label(engine, n, k):
    labels = P.group_labels(n, k, seed=n + k)
    want_off, want_mem = P.group_ref(labels, k)
    assert want_off[-1] < n                       # some labels belong to no state
    off, mem = _group(engine, labels, k)
    np.testing.assert_array_equal(off, want_off)
    np.testing.assert_array_equal(mem[:want_off[-1]], want_mem)
    assert _is_junk(mem[want_off[-1]:])           # not written past offsets[k]
    off2, mem2 = _group(engine, labels, k)
    assert off2.tobytes() == off.tobytes() and mem2.tobytes() == mem.tobytes()


def test_group_smaller_call_after_a_larger(engine):
    from pmarlo_amd.device import Engine

    big = P.group_labels(130 * 1024 + 7, 257, seed=1)
    small = P.group_labels(1025, 5, seed=2)
    _group(engine, big, 257)
    off, mem = _group(engine, small, 5)            # the scratch holds the larger histogram and ranks
    fresh = Engine(0)
    try:
        off_f, mem_f = _group(fresh, small, 5)
    finally:
        fresh.close()
    want_off, want_mem = P.group_ref(small, 5)
    np.testing.assert_array_equal(off, want_off)
    np.testing.assert_array_equal(mem[:want_off[-1]], want_mem)
    assert off.tobytes() == off_f.tobytes() and mem.tobytes() == mem_f.tobytes()


# ---- centroids -----------------------------------------------------------------------------------------------------
def _centroids(engine, x, ld, w, d_off, d_mem, k):
    n, d = x.shape
    d_x = engine.to_device(P.strided(x, ld))
    d_w = None if w is None else engine.to_device(np.ascontiguousarray(w, np.float64))
    cen, wsum, flags = _junk(engine, (k, d), np.float64), _junk(engine, (k,), np.float64), _junk(engine, (k,), np.int32)
    assert P.c_centroids(engine, d_x, n, d, ld, d_w, d_off, d_mem, k, cen, wsum, flags) == OK
    return d_x, d_w, cen, wsum, flags


@pytest.mark.parametrize("d", P.CENTROID_D)
def test_centroids(engine, d):
    sizes = P.centroid_sizes(d)
    x, labels, k, w = P.state_case(d, sizes, seed=300 + d)
    d_lab, d_off, d_mem, offsets, members = _upload_groups(engine, labels, k)
    xmax = float(np.abs(x).max())
    worst_c, worst_w = (0.0, 0.0, 1.0, 0), (0.0, 0.0, 1.0, 0)     # (error / bound, error, bound, n_s) of the worst state
    for ld in (d, d + 1, d + 1000):
        for weights in (None, w):
            _, _, cen, wsum, flags = _centroids(engine, x, ld, weights, d_off, d_mem, k)
            cen, wsum, flags = cen.to_host(), wsum.to_host(), flags.to_host()
            assert not flags.any()
            for s, ns in enumerate(sizes):
                if ns == 0:
                    assert not cen[s].any() and wsum[s] == 0.0
                    continue
                frames = members[offsets[s]:offsets[s + 1]]
                law_c, law_w = P.centroid_law(x, frames, weights)
                err_c = float(np.abs(cen[s] - law_c).max())
                err_w = float(abs(wsum[s] - law_w) / law_w)
                assert err_c <= 2 * ns * U * xmax, (d, ld, s, ns, err_c)
                assert err_w <= ns * U, (d, ld, s, ns, err_w)
                if weights is None:
                    assert wsum[s] == ns
                worst_c = max(worst_c, (err_c / (2 * ns * U * xmax), err_c, 2 * ns * U * xmax, ns))
                worst_w = max(worst_w, (err_w / (ns * U), err_w, ns * U, ns))
    print(f"centroids d={d}: coordinate, worst state (n_s={worst_c[3]}): measured {worst_c[1]:.3e}, bound {worst_c[2]:.3e}; "
          f"weight sum, worst state (n_s={worst_w[3]}): measured {worst_w[1]:.3e}, bound {worst_w[2]:.3e}")


FLAG_PATTERNS = {
    "nonfinite": ([np.inf], _lib.REP_FLAG_NONFINITE),
    "negative": ([-0.01], _lib.REP_FLAG_NEGATIVE),
    "nonpositive_sum": (None, _lib.REP_FLAG_NONPOSITIVE_SUM),     # every weight 0
    "nan": ([np.nan], _lib.REP_FLAG_NONFINITE | _lib.REP_FLAG_NONPOSITIVE_SUM),
    "negative_sum": ([-1e6], _lib.REP_FLAG_NEGATIVE | _lib.REP_FLAG_NONPOSITIVE_SUM),
    "minus_inf": ([-np.inf], _lib.REP_FLAG_NONFINITE | _lib.REP_FLAG_NEGATIVE | _lib.REP_FLAG_NONPOSITIVE_SUM),
    "inf_and_negative": ([np.inf, -0.5], _lib.REP_FLAG_NONFINITE | _lib.REP_FLAG_NEGATIVE),
}


@pytest.mark.parametrize("pattern", list(FLAG_PATTERNS))
def test_centroid_flags(engine, pattern):
    sizes = (5, 300, 40, 0, 77)
    x, labels, k, w = P.state_case(3, sizes, seed=41)
    d_lab, d_off, d_mem, offsets, members = _upload_groups(engine, labels, k)
    values, want = FLAG_PATTERNS[pattern]
    for target in (1, 2):                          # a state of more than 256 members, and one of fewer
        w2 = np.array(w)
        frames = members[offsets[target]:offsets[target + 1]]
        if values is None:
            w2[frames] = 0.0
        else:
            w2[frames[-1 - np.arange(len(values)) * 7]] = values     # late members: not the first trip of the loop
        _, _, cen, wsum, flags = _centroids(engine, x, 4, w2, d_off, d_mem, k)
        flags = flags.to_host()
        expect = np.zeros(k, np.int32)
        expect[target] = want
        np.testing.assert_array_equal(flags, expect)
        assert not cen.to_host()[3].any()          # the empty state


# ---- centroid-mode scores ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", P.CENTROID_D)
def test_centroid_scores(engine, d):
    sizes = P.score_sizes(d)
    x, labels, k, w = P.state_case(d, sizes, seed=100 + d)
    n = labels.size
    d_lab, d_off, d_mem, offsets, members = _upload_groups(engine, labels, k)
    total = int(offsets[-1])
    assert total % 256 != 0 and total < n
    xmax = float(np.abs(x).max())
    worst = (0.0, 0.0, 1.0, 0)
    for ld in (d, d + 1, d + 1000):
        for weights in (None, w):
            d_x, d_w, cen, wsum, _ = _centroids(engine, x, ld, weights, d_off, d_mem, k)
            d_sc = _junk(engine, (n,), np.float64)
            st = P.c_scores(engine, d_x, n, d, ld, d_w, d_lab, d_off, d_mem, k, cen, wsum, _lib.REP_SCORE_CENTROID, offsets,
                            None, d_sc)
            assert st == OK
            sc = d_sc.to_host()
            assert _is_junk(sc[total:])
            for s, ns in enumerate(sizes):
                if ns == 0:
                    continue
                frames = members[offsets[s]:offsets[s + 1]]
                law = P.centroid_scores_law(x, frames, weights)
                err = float(np.abs(sc[offsets[s]:offsets[s + 1]] - law).max())
                bound = 4 * ns * U * np.sqrt(d) * xmax
                assert err <= bound, (d, ld, s, ns, err, bound)
                worst = max(worst, (err / bound, err, bound, ns))
    print(f"centroid distance d={d}: worst state (n_s={worst[3]}): measured {worst[1]:.3e}, bound {worst[2]:.3e}")


# ---- medoid-mode scores --------------------------------------------------------------------------------------------
MEDOID_LIST = (8, 3, 0, 3, 7, 1, 2, 6, 5)       # unsorted, state 3 twice, state 4 (65 members) left out


@pytest.mark.parametrize("d", P.MEDOID_D)
def test_medoid_scores(engine, d):
    x, labels, k, w = P.state_case(d, P.MEDOID_SIZES, seed=200 + d)
    n = labels.size
    d_lab, d_off, d_mem, offsets, members = _upload_groups(engine, labels, k)
    ld = d + 3
    worst = (0.0, 0.0, 1.0, 0)
    for weights in (None, w):
        d_x, d_w, cen, wsum, _ = _centroids(engine, x, ld, weights, d_off, d_mem, k)
        runs = []
        for _ in range(2):
            d_sc = _junk(engine, (n,), np.float64)
            st = P.c_scores(engine, d_x, n, d, ld, d_w, None, d_off, d_mem, k, None, wsum, _lib.REP_SCORE_MEDOID, offsets,
                            MEDOID_LIST, d_sc)
            assert st == OK
            runs.append(d_sc.to_host())
        sc = runs[0]
        assert runs[1].tobytes() == sc.tobytes()
        assert _is_junk(sc[offsets[4]:offsets[5]]) and _is_junk(sc[offsets[-1]:])
        for s in sorted(set(MEDOID_LIST)):
            frames = members[offsets[s]:offsets[s + 1]]
            law = P.medoid_scores_law(x, frames, weights)
            got = sc[offsets[s]:offsets[s + 1]]
            if frames.size == 1:
                assert got[0] == 0.0
                continue
            err = float((np.abs(got - law) / law).max())
            bound = 4 * (frames.size + d) * U
            assert err <= bound, (d, s, frames.size, err, bound)
            worst = max(worst, (err / bound, err, bound, frames.size))
    print(f"medoid score d={d}: worst state (n_s={worst[3]}): measured {worst[1]:.3e}, bound {worst[2]:.3e}")


def test_medoid_without_work(engine):
    x, labels, k, w = P.state_case(7, P.MEDOID_SIZES, seed=207)
    n, d = x.shape
    d_lab, d_off, d_mem, offsets, members = _upload_groups(engine, labels, k)
    d_x, d_w, cen, wsum, _ = _centroids(engine, x, d, None, d_off, d_mem, k)
    d_sc = _junk(engine, (n,), np.float64)
    args = (engine, d_x, n, d, d, None, None, d_off, d_mem, k, None, wsum, _lib.REP_SCORE_MEDOID)
    assert P.c_scores(*args, offsets, None, d_sc) == OK                     # n_states = 0
    assert P.c_scores(*args, np.zeros(k + 1, np.int64), [0, 3], d_sc) == OK  # total = 0: no state has a member
    assert P.c_scores(engine, d_x, n, d, d, None, d_lab, d_off, d_mem, k, cen, wsum, _lib.REP_SCORE_CENTROID,
                      np.zeros(k + 1, np.int64), None, d_sc) == OK
    engine.sync()
    assert _is_junk(d_sc.to_host())


def test_medoid_second_launch(engine):
    """One state of 16 500 members at d = 256: 129 tasks of 128 x 16 500 x 256 = 540 672 000 products; 127 of them fit
    the 2^36 products of a launch, so the first launch takes the rows [0, 16 256) and the second (d_tasks + 127) the
    rest.  64 rows against the law; all rows the same bytes on a second run."""
    ns, d = 16_500, 256
    cost = _lib.REP_TILE_I * ns * d
    assert (2 ** 36) // cost == 127 and -(-ns // _lib.REP_TILE_I) == 129
    cut = 127 * _lib.REP_TILE_I
    rng = np.random.default_rng(36)
    x = rng.standard_normal((ns, d))
    edges = np.array([0, cut - 1, cut, ns - 1])     # the first and last row of each launch
    rows = np.sort(np.concatenate([edges, rng.choice(np.setdiff1d(np.arange(ns), edges), 60, replace=False)]))
    assert rows.size == 64
    offsets = np.array([0, ns], np.int64)
    d_x = engine.to_device(x)
    d_off = engine.to_device(offsets)
    d_mem = engine.to_device(np.arange(ns, dtype=np.int32))
    wsum = engine.to_device(np.array([float(ns)]))
    runs = []
    for _ in range(2):
        d_sc = _junk(engine, (ns,), np.float64)
        engine.sync()
        t0 = time.perf_counter()
        st = P.c_scores(engine, d_x, ns, d, d, None, None, d_off, d_mem, 1, None, wsum, _lib.REP_SCORE_MEDOID, offsets, [0], d_sc)
        engine.sync()
        print(f"medoid scores of 16 500 members at d = 256 (two launches): {time.perf_counter() - t0:.3f} s")
        assert st == OK
        runs.append(d_sc.to_host())
    assert runs[0].tobytes() == runs[1].tobytes()
    assert not _is_junk(runs[0][cut:]) and np.isfinite(runs[0]).all()
    law = P.medoid_scores_law(x, np.arange(ns), None, rows)
    _report("medoid score across the launch cut", float((np.abs(runs[0][rows] - law) / law).max()), 4 * (ns + d) * U)


# ---- selection -----------------------------------------------------------------------------------------------------
def _select(engine, x, ld, d_off, d_mem, k, scores, mode, states, n_reps, expect=OK):
    n, d = x.shape
    d_x = engine.to_device(P.strided(x, ld))
    d_sc = engine.to_device(np.ascontiguousarray(scores, np.float64))
    if d_sc.size < n:                               # scores are laid out like members: n words
        full = _junk(engine, (n,), np.float64)
        full.view((d_sc.size,)).copy_from(d_sc)
        d_sc = full
    diverse = mode == "diverse"
    d_mind = _junk(engine, (n,), np.float64) if diverse else None
    picks = _junk(engine, (len(states), n_reps), np.int32)
    st = P.c_select(engine, d_x, n, d, ld, d_off, d_mem, k, d_sc, d_mind,
                    _lib.REP_SELECT_DIVERSE if diverse else _lib.REP_SELECT_SMALLEST, states, n_reps, picks)
    assert st == expect
    engine.sync()
    return picks.to_host()


@pytest.mark.parametrize("n_states", [1, 300])
@pytest.mark.parametrize("n_reps", P.SELECT_REPS)
@pytest.mark.parametrize("mode", ["smallest", "diverse"])
def test_select(engine, mode, n_reps, n_states):
    x, labels, k, sizes, offsets, members, scores = P.select_case()
    want, _ = P.select_rows(mode, n_reps, n_states)
    d_lab, d_off, d_mem, _, _ = _upload_groups(engine, labels, k)
    states = P.select_states(n_states)
    got = _select(engine, x, P.SELECT_D + 2, d_off, d_mem, k, scores, mode, states, n_reps)
    np.testing.assert_array_equal(got, want)
    for row, s in zip(got, states):                # the -1 tail at every position
        assert (row[min(n_reps, sizes[s]):] == -1).all()
    again = _select(engine, x, P.SELECT_D, d_off, d_mem, k, scores, mode, states, n_reps)
    assert again.tobytes() == got.tobytes()


def test_select_ties_go_to_the_lowest_frame(engine):
    """300 + 270 points on the 7 x 7 x 7 integer lattice: squared distances are exact integers in fp64 and in
    longdouble, so equal distances are equal in both and the frame rule alone decides them."""
    rng = np.random.default_rng(8)
    labels = rng.permutation(np.repeat([0, 1], [300, 270])).astype(np.int32)
    x = rng.integers(-3, 4, size=(labels.size, 3)).astype(np.float64)
    assert np.unique(x[labels == 0], axis=0).shape[0] < 250      # duplicated rows
    scores_by_frame = np.sqrt((x * x).sum(axis=1))                # equal scores wherever |x| is equal
    d_lab, d_off, d_mem, offsets, members = _upload_groups(engine, labels, 2)
    scores = scores_by_frame[members]
    for mode in ("smallest", "diverse"):
        got = _select(engine, x, 5, d_off, d_mem, 2, scores, mode, [1, 0], 40)
        for row, s in zip(got, (1, 0)):
            frames = members[offsets[s]:offsets[s + 1]]
            sc = scores[offsets[s]:offsets[s + 1]]
            want = P.smallest_law(sc, frames, 40) if mode == "smallest" else P.diverse_law(x, frames, sc, 40)
            assert row.tolist() == want, (mode, s)


@pytest.mark.parametrize("n_reps", [3, P.PRESET_SIZE + 1])
@pytest.mark.parametrize("mode", ["smallest", "diverse"])
def test_select_preset_scores(engine, mode, n_reps):
    x, labels, k, offsets, members, scores = P.preset_case()
    d_lab, d_off, d_mem, _, _ = _upload_groups(engine, labels, k)
    states = list(range(k))[::-1]
    got = _select(engine, x, 4, d_off, d_mem, k, scores, mode, states, n_reps)
    for row, s in zip(got, states):
        name = list(P.PRESET_SCORES)[s]
        frames = members[offsets[s]:offsets[s + 1]]
        sc = scores[offsets[s]:offsets[s + 1]]
        want = P.smallest_law(sc, frames, n_reps) if mode == "smallest" else P.diverse_law(x, frames, sc, n_reps)
        assert row.tolist() == want, (mode, name)
        if mode == "smallest" and name == "all_nan":
            assert (row == -1).all()
        if mode == "smallest" and name == "one_nan" and n_reps > P.PRESET_SIZE:
            assert (row[:P.PRESET_SIZE - 1] >= 0).all() and (row[P.PRESET_SIZE - 1:] == -1).all()
        if mode == "diverse" and name == "all_nan":
            assert row[0] == frames[0]             # starts at member 0, as the kernel's comment says


def test_select_nan_features(engine):
    x, labels, k, offsets, members, scores = P.nan_feature_case()
    d_lab, d_off, d_mem, _, _ = _upload_groups(engine, labels, k)
    ns = 40
    got = _select(engine, x, 6, d_off, d_mem, k, scores, "diverse", [2, 0, 1], ns)
    rows = dict(zip((2, 0, 1), got))
    for s in range(k):
        frames = members[offsets[s]:offsets[s + 1]]
        assert rows[s].tolist() == P.diverse_law(x, frames, scores[offsets[s]:offsets[s + 1]], ns), s
    assert rows[0][0] == members[offsets[0]] and (rows[0] >= 0).all()       # all-NaN scores: member 0, a full walk
    bad1 = int(members[offsets[1]:offsets[2]][np.isnan(x[members[offsets[1]:offsets[2]]]).any(axis=1)][0])
    assert bad1 not in rows[1] and (rows[1][:ns - 1] >= 0).all() and rows[1][ns - 1] == -1
    assert np.isnan(x[rows[2][0]]).any() and (rows[2][1:] == -1).all()      # no index to follow from round 1 on
    # smallest never reads the features
    got = _select(engine, x, 6, d_off, d_mem, k, scores, "smallest", [0, 1], 3)
    assert (got[0] == -1).all()
    assert got[1].tolist() == P.smallest_law(scores[offsets[1]:offsets[2]], members[offsets[1]:offsets[2]], 3)


def test_picker_nan_rule(engine):
    """A NaN coordinate in one frame of state 1.  Its centroid and every centroid distance and medoid score of the
    state are NaN, and a NaN never wins: the two smallest-score methods return nothing for the state (the reference's
    np.argpartition would return frames in an unspecified order), `diverse` starts at the state's first frame and never
    picks the NaN frame.  The other states are untouched."""
    from pmarlo_amd.conformations import RepresentativePicker

    x, clean, labels, frames1, bad = P.picker_nan_case()
    picker = RepresentativePicker()
    for method in ("closest_to_centroid", "true_medoid"):
        got = picker.pick_representatives(x, [labels], [0, 1, 2], n_reps=2, method=method)
        assert got == picker.pick_representatives(clean, [labels], [0, 2], n_reps=2, method=method)
        assert [g[0] for g in got] == [0, 0, 2, 2]
    n1 = frames1.size
    got = picker.pick_representatives(x, [labels], [1, 2], n_reps=n1, method="diverse")
    mine = [g[1] for g in got if g[0] == 1]
    assert mine == [f for f in P.diverse_law(x, frames1, np.full(n1, np.nan), n1) if f >= 0]
    assert mine[0] == frames1[0] and bad not in mine and len(mine) == n1 - 1
    assert [g for g in got if g[0] == 2] == picker.pick_representatives(clean, [labels], [2], n_reps=n1, method="diverse")


def test_select_refuses_bad_state_lists(engine):
    x, labels, k, offsets, members, scores = P.preset_case()
    d_lab, d_off, d_mem, _, _ = _upload_groups(engine, labels, k)
    for mode in ("smallest", "diverse"):
        for states in ([0, 2, 0], [1, k], [-1], [P.INT32_MAX]):
            got = _select(engine, x, 3, d_off, d_mem, k, scores, mode, states, 4, expect=INVALID)
            assert _is_junk(got), (mode, states)


@pytest.mark.parametrize("name", [c[0] for c in P.PICK_CASES])
def test_full_path_exact_picks(engine, name):
    """Centroids, both kinds of scores and both selections chained through the C ABI on strided rows.  The margins of
    the law on these inputs are asserted by test_rep_sil_paths_reference.py (>= 1e-6 in every state)."""
    x, labels, k, w, n_reps = P.pick_case(name)
    n, d = x.shape
    ld = d + 2
    d_lab, d_off, d_mem, offsets, members = _upload_groups(engine, labels, k)
    states = list(range(k))[::-1]
    for weights in (None, w):
        d_x, d_w, cen, wsum, _ = _centroids(engine, x, ld, weights, d_off, d_mem, k)
        cs, ms = _junk(engine, (n,), np.float64), _junk(engine, (n,), np.float64)
        assert P.c_scores(engine, d_x, n, d, ld, d_w, d_lab, d_off, d_mem, k, cen, wsum, _lib.REP_SCORE_CENTROID, offsets,
                          None, cs) == OK
        assert P.c_scores(engine, d_x, n, d, ld, d_w, None, d_off, d_mem, k, None, wsum, _lib.REP_SCORE_MEDOID, offsets,
                          states, ms) == OK
        for method, d_sc, mode in (("centroid", cs, "smallest"), ("medoid", ms, "smallest"), ("diverse", cs, "diverse")):
            picks = _junk(engine, (k, n_reps), np.int32)
            mind = _junk(engine, (n,), np.float64)
            assert P.c_select(engine, d_x, n, d, ld, d_off, d_mem, k, d_sc, mind,
                              _lib.REP_SELECT_DIVERSE if mode == "diverse" else _lib.REP_SELECT_SMALLEST, states, n_reps,
                              picks) == OK
            engine.sync()
            for row, s in zip(picks.to_host(), states):
                frames = members[offsets[s]:offsets[s + 1]]
                law_c = P.centroid_scores_law(x, frames, weights)
                law = P.medoid_scores_law(x, frames, weights) if method == "medoid" else law_c
                want = P.diverse_law(x, frames, law, n_reps) if mode == "diverse" else P.smallest_law(law, frames, n_reps)
                assert row.tolist() == want, (method, s, weights is not None)


# ---- msm_silhouette (k <= 32) --------------------------------------------------------------------------------------
def _sorted_entry(engine, X, ld, offsets, k, expect=OK):
    n, d = X.shape
    d_x = engine.to_device(P.strided(X, ld))
    samples, score = _junk(engine, (n,), np.float64), _junk(engine, (1,), np.float64)
    assert P.c_silhouette(engine, d_x, n, d, ld, offsets, k, samples, score) == expect
    engine.sync()
    return samples.to_host(), float(score.to_host()[0])


def _samples_entry(engine, X, ld, labels, k, max_products=0, expect=OK):
    n, d = X.shape
    d_x = engine.to_device(P.strided(X, ld))
    d_lab = engine.to_device(np.ascontiguousarray(labels, np.int32))
    samples, score = _junk(engine, (n,), np.float64), _junk(engine, (1,), np.float64)
    assert P.c_silhouette_samples(engine, d_x, n, d, ld, d_lab, k, samples, score, max_products) == expect
    return samples.to_host(), float(score.to_host()[0])


def _check_score(name, score, law):
    mean = float(law.mean())
    if mean == 0.0:
        assert score == 0.0, name
    else:
        _report(f"{name}: score", abs(score - mean) / abs(mean), P.SCORE_RTOL)


@pytest.mark.parametrize("k,d,n", P.SORTED_SHAPES)
def test_silhouette_sorted(engine, k, d, n):
    X, labels, offsets, law = P.sorted_case(k, d, n)
    name = f"msm_silhouette ({k}, {d}, {n})"
    got, score = _sorted_entry(engine, X, d + 5, offsets, k)
    _report(f"{name}: samples", float(np.abs(got - law).max()), P.SIL_ATOL)
    _check_score(name, score, law)
    sizes = np.diff(offsets)
    assert (got[np.repeat(sizes == 1, sizes)] == 0.0).all()       # singletons
    again, score2 = _sorted_entry(engine, X, d, offsets, k)
    assert again.tobytes() == got.tobytes() and score2 == score
    if n >= 3 and k <= n - 1:
        other, score_s = _samples_entry(engine, X, d + 5, labels, k)
        _report(f"{name}: msm_silhouette_samples on the same points", float(np.abs(other - law).max()), P.SIL_ATOL)
        _check_score(name + " (samples entry)", score_s, law)


def test_silhouette_refusals(engine):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((80, 129))
    off2 = np.array([0, 40, 80], np.int64)
    for Xc, off, k in ((X, off2, 2),                                             # d = 129
                       (X[:, :4], np.concatenate([np.arange(33), [80]]), 33),    # k = 33
                       (X[:, :4], np.array([0, 80]), 1)):                        # k = 1
        got, _ = _sorted_entry(engine, Xc, Xc.shape[1], off, k, expect=INVALID)
        assert _is_junk(got)
    got, _ = _sorted_entry(engine, X[:, :128], 128, off2, 2)                     # the last d that is taken
    assert np.isfinite(got).all()


# ---- msm_silhouette_samples ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.SAMPLES_SHAPES))
def test_silhouette_samples_paths(engine, name):
    X, labels, k, law = P.samples_case(name)
    n, d = X.shape
    got, score = _samples_entry(engine, X, d + 3, labels, k)
    _report(f"msm_silhouette_samples {name}: samples", float(np.abs(got - law).max()), P.SIL_ATOL)
    _check_score(name, score, law)
    tiles = -(-n // _lib.SIL_TILE_I)
    cuts = [1, _lib.SIL_TILE_I * _lib.SIL_SEG_LEN * d * 5]
    if name == "cut_group_of_1024":
        assert tiles == 11                         # 5 tiles a launch: 5, 5 and a remainder of one tile
    for ld, max_products in [(d, 0)] + [(d + 3, c) for c in cuts]:
        other, score_o = _samples_entry(engine, X, ld, labels, k, max_products)
        assert other.tobytes() == got.tobytes() and score_o == score, (name, ld, max_products)


# ---- non-finite coordinates ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.NONFINITE))
def test_non_finite_coordinates(engine, name):
    X, labels, offsets, law, frame = P.nonfinite_case(name)
    k = len(P.NONFINITE_SIZES)
    nan = np.isnan(law)
    assert nan.any()
    for entry, (got, score) in (("msm_silhouette", _sorted_entry(engine, X, 5, offsets, k)),
                                ("msm_silhouette_samples", _samples_entry(engine, X, 5, labels, k)),
                                ("msm_silhouette_samples, one workgroup a launch", _samples_entry(engine, X, 3, labels, k, 1))):
        assert np.array_equal(np.isnan(got), nan), f"{entry} {name}: NaN in {np.isnan(got).sum()} samples, the law in {nan.sum()}"
        _report(f"{entry} {name}: finite samples", float(np.abs(got[~nan] - law[~nan]).max(initial=0.0)), P.SIL_ATOL)
        assert np.isnan(score) == bool(np.isnan(law.mean())), (entry, score)


def test_finite_input_keeps_its_bits(engine, golden):
    """The outputs recorded before the NaN rule (P.recipe_points says how): the same bytes."""
    gold = golden(P.BEFORE_NAN_RULE)
    for n, d, k in ((1500, 3, 33), (700, 256, 40)):
        X, labels = P.recipe_points(n, d, k)
        got, score = _samples_entry(engine, X, d, labels, k)
        assert got.tobytes() == gold[f"samples/{n}_{d}_{k}"].tobytes()
        assert score == gold[f"score/{n}_{d}_{k}"][0]
    n, d, k = 1000, 3, 7
    X, labels = P.recipe_points(n, d, k)
    order = np.argsort(labels, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=k))]).astype(np.int64)
    got, score = _sorted_entry(engine, X[order], d, offsets, k)
    assert got.tobytes() == gold[f"sorted_samples/{n}_{d}_{k}"].tobytes()
    assert score == gold[f"sorted_score/{n}_{d}_{k}"][0]


def test_public_score_of_nan_features_is_nan(engine):
    """clustering.silhouette_score and silhouette_samples, the functions behind the n_states="auto" scan: labels
    fitted on clean features, one coordinate then set to NaN.  The score is the NaN that _auto_select_n_states refuses
    (tests/test_silhouette_host.py), where it used to be a finite, wrong number."""
    from pmarlo_amd.markov_state_model.clustering import cluster_microstates, silhouette_samples, silhouette_score

    rng = np.random.default_rng(3)
    planted = np.arange(600) % 4
    X = 8.0 * np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])[planted] + rng.normal(scale=0.3, size=(600, 2))
    labels = cluster_microstates(X, n_states=4, random_state=0).labels
    assert np.unique(labels * 4 + planted).size == 4
    clean = silhouette_score(X, labels)
    assert np.isfinite(clean) and clean > 0.8
    X[17, 1] = np.nan
    s = silhouette_samples(X, labels)
    np.testing.assert_array_equal(np.isnan(s), np.isnan(P.silhouette_law(X, labels, 4)))
    assert np.isnan(s).all() and np.isnan(silhouette_score(X, labels))


# ---- capture -------------------------------------------------------------------------------------------------------
def _capture_buffers(eng, x, labels, k):
    n, d = x.shape
    return dict(x=eng.to_device(x), lab=eng.to_device(labels), off=_junk(eng, (k + 1,), np.int64),
                mem=_junk(eng, (n,), np.int32), cen=_junk(eng, (k, d), np.float64), wsum=_junk(eng, (k,), np.float64),
                flags=_junk(eng, (k,), np.int32), sc=_junk(eng, (n,), np.float64))


def _linear_sequence(eng, b, n, d, k, h_offsets):
    assert P.c_group(eng, b["lab"], n, k, b["off"], b["mem"]) == OK
    assert P.c_centroids(eng, b["x"], n, d, d, None, b["off"], b["mem"], k, b["cen"], b["wsum"], b["flags"]) == OK
    assert P.c_scores(eng, b["x"], n, d, d, None, b["lab"], b["off"], b["mem"], k, b["cen"], b["wsum"],
                      _lib.REP_SCORE_CENTROID, h_offsets, None, b["sc"]) == OK


def test_capture_replays_the_linear_sequence():
    from pmarlo_amd.device import Engine

    x, labels, k, _ = P.state_case(5, P.score_sizes(5), seed=105)
    n, d = x.shape
    h_offsets, _ = P.group_ref(labels, k)
    eng = Engine(0)
    try:
        eager, cap = _capture_buffers(eng, x, labels, k), _capture_buffers(eng, x, labels, k)
        _linear_sequence(eng, eager, n, d, k, h_offsets)            # the eager warm-up: the scratch has its size
        eng.sync()
        want = {name: eager[name].to_host() for name in ("off", "mem", "cen", "wsum", "flags", "sc")}
        eng.graph_begin()
        try:
            _linear_sequence(eng, cap, n, d, k, h_offsets)
        finally:
            g = eng.graph_end()
        try:
            eng.sync()
            assert _is_junk(cap["sc"].to_host())                    # captured, not run
            for _ in range(2):
                eng.graph_launch(g)
                eng.sync()
                for name, w in want.items():
                    assert cap[name].to_host().tobytes() == w.tobytes(), name
                for name in ("off", "mem", "cen", "wsum", "flags", "sc"):
                    cap[name].fill_bytes_(0x5A)
                eng.sync()
        finally:
            eng.graph_destroy(g)
    finally:
        eng.close()


def test_capture_refusals():
    from pmarlo_amd.device import Engine

    x, labels, k, _ = P.state_case(5, P.score_sizes(5), seed=105)
    n, d = x.shape
    h_offsets, _ = P.group_ref(labels, k)
    eng = Engine(0)
    try:
        b = _capture_buffers(eng, x, labels, k)
        _linear_sequence(eng, b, n, d, k, h_offsets)
        eng.sync()
        want_cen = b["cen"].to_host()
        big_n = 8 * 1024 * 1024                                     # its ranks alone outgrow the warmed-up scratch
        big_lab = eng.zeros((big_n,), np.int32)
        big_mem = _junk(eng, (big_n,), np.int32)
        picks, mind = _junk(eng, (k, 2), np.int32), _junk(eng, (n,), np.float64)
        samples, score = _junk(eng, (n,), np.float64), _junk(eng, (1,), np.float64)
        work = eng.empty((int(_lib.load().msm_silhouette_workspace_bytes(n, d, k)),), np.uint8)
        med = _junk(eng, (n,), np.float64)
        b["cen"].fill_bytes_(0x5A)
        eng.sync()
        eng.graph_begin()
        try:
            st_cen = P.c_centroids(eng, b["x"], n, d, d, None, b["off"], b["mem"], k, b["cen"], b["wsum"], b["flags"])
            st_med = P.c_scores(eng, b["x"], n, d, d, None, None, b["off"], b["mem"], k, None, b["wsum"],
                                _lib.REP_SCORE_MEDOID, h_offsets, [0, 1], med)
            st_sel = P.c_select(eng, b["x"], n, d, d, b["off"], b["mem"], k, b["sc"], mind, _lib.REP_SELECT_DIVERSE, [0, 1], 2,
                                picks)
            st_sml = P.c_select(eng, None, n, d, d, b["off"], b["mem"], k, b["sc"], None, _lib.REP_SELECT_SMALLEST, [0, 1], 2,
                                picks)
            st_sil = P.c_silhouette_samples(eng, b["x"], n, d, d, b["lab"], k, samples, score, work=work)
            st_grp = P.c_group(eng, big_lab, big_n, k, b["off"], big_mem)
        finally:
            g = eng.graph_end()                                     # the capture ends cleanly
        try:
            assert st_cen == OK
            assert (st_med, st_sel, st_sml, st_sil, st_grp) == (UNSUPPORTED,) * 5
            eng.graph_launch(g)
            eng.sync()
            assert b["cen"].to_host().tobytes() == want_cen.tobytes()
            for buf in (med, picks, mind, samples, score, big_mem):
                assert _is_junk(buf.to_host())
        finally:
            eng.graph_destroy(g)
    finally:
        eng.close()
