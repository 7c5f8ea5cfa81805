"""Every launch path of pmarlo_amd/csrc/counts.hip against the exact restatements of tests/_counts_ref.py (which
tests/test_counts_reference.py checks against oracle/cport on the CPU).

Every counts case first asks Engine.count_plan -- the read-only view of the one dispatch function launch_counts
uses -- for the path it is on and the property it exists for, and only then compares.  Every output (matrix, pair
total, T, rowsum, diagonal mass) holds 0x5A bytes before the call: an entry the kernel does not write shows up.
Labels: Markov chain, uniform random, constant k - 1, runs of 37 (and {0, k - 1} at the key-space limit), each with
-1, k, k + 5, INT32_MIN and INT32_MAX sprinkled in; the kernels compare unsigned and none of these may be counted.

  test_unweighted[privatised_8_row_blocks]    count_lds_kernel<false>: 8 row blocks, > 4096 pairs per chunk, so every
                                              thread takes trips of the 4-way unrolled loop and a tail
  test_unweighted[privatised_16_row_blocks]   count_lds_kernel<false>: kMaxRowBlocks row blocks, the last one short
  test_unweighted[privatised_last_k]          count_lds_kernel<false> at k = 720: 16 full row blocks of 45 rows, the last
                                              k the LDS rows hold
  test_unweighted[global_first_k]             count_global_kernel<false> at k = 721, the first k past the row-block
                                              limit, and [global_k725] a few states further
  test_unweighted[bucket_key_space_limit]     count_bucket_*: R k = 16384 = the whole 14-bit key space in one bin copy;
                                              key 0x3FFF, a count element of a whole 4096-pair chunk (constant labels)
  test_unweighted[past_the_bucket_limit]      k = 2049 with pairs >= k^2 falls through to count_global_kernel
  test_normalised_at_the_key_space_limit      count_bucket_bin_kernel<true> at R = 8, 2048 rows: counts, rowsum, T,
                                              diagonal mass equal the two-call form bit for bit, and the reference
  test_ragged_stride3                         bucket / privatised / global with empty, one-frame and clipped
                                              segments and stride 3 (seg_pair_to_frame on the inline table)
  test_weighted[budget_switch_*]              count_lds_kernel<true> at k = 90 (64 KiB budget, no attribute call) and
                                              k = 91 (128 KiB budget, hipFuncSetAttribute)
  test_weighted[single_block_unrolled]        count_lds_kernel<true>: one row block, unrolled trips
  test_weighted[several_row_blocks]           count_lds_kernel<true>: 6 row blocks
  test_weighted[sixteen_row_blocks]           count_lds_kernel<true>: 16 row blocks, exactly 131072 B of LDS
  test_weighted[global]                       count_global_kernel<true> (k = 513)
  test_weighted_ragged_stride3                count_lds_kernel<true> over ragged segments
  test_weighted_real_weights                  fp64 atomics in any order against one fsum per bin
  test_lagscan_across_paths                   msm_count_transitions_lagscan: lags on the bucket path (pairs == k^2
                                              included), the privatised path and with no pair; d_pairs = NULL
  test_capture_falls_back_to_privatised       a capture that cannot grow the auxiliary scratch: count_lds_kernel<false>
                                              at the bench shape, replayed, equal to the eager bucket result
  test_state_counts_lds_switch                state_counts_kernel at k = 16384 (64 KiB of dynamic LDS), 16385
                                              (global atomics), and k = n = 1
  test_run_lengths_*                          run_lengths_kernel: capacity below the number of runs, capacity 0 with
                                              NULL lists, labels >= k as separators, one run over everything,
                                              alternating labels, n = 1
"""

from __future__ import annotations

import numpy as np
import pytest

from pmarlo_amd import _lib
from tests import _counts_ref as ref

pytestmark = pytest.mark.gpu

JUNK64 = 0x5A5A5A5A5A5A5A5A


def _junk(engine, shape, dtype):
    return engine.empty(shape, dtype).fill_bytes_(0x5A)


def _bounds(segs):
    return np.asarray([a for a, _ in segs], np.int64), np.asarray([b for _, b in segs], np.int64)


def _labels(kind, n, k, seed=1):
    return ref.sprinkle_invalid(ref.labels_of_kind(kind, n, k, seed), k)


def _n_cu(engine):
    return engine.info()["n_cu"]


def _count(engine, lab_h, k, lag, segs=None, stride=1):
    kw = {}
    if segs is not None:
        kw["starts"], kw["stops"] = _bounds(segs)
    c, p = engine.count_transitions(engine.to_device(lab_h), k, lag, stride=stride, out=_junk(engine, (k, k), np.int64),
                                    pairs=_junk(engine, (1,), np.int64), **kw)
    return c.to_host(), int(p.to_host()[0])


# ---- unweighted ----------------------------------------------------------------------------------------------------
def _assert_unweighted_plan(engine, name, k, pairs):
    plan = engine.count_plan(k, pairs)
    if name == "privatised_8_row_blocks":
        assert plan["path"] == "privatised" and plan["row_blocks"] == 8, plan
        # more than one unrolled trip's worth (4 x 1024 pairs) and not a multiple of it: unrolled trips and tail trips
        assert plan["pairs_per_chunk"] > 4096 and plan["pairs_per_chunk"] % 4096, plan
    elif name == "privatised_16_row_blocks":
        assert plan["path"] == "privatised" and plan["row_blocks"] == 16, plan
        assert plan["rows"] * 16 > k and plan["pairs_per_chunk"] > 4096, plan
    elif name == "privatised_last_k":
        assert plan["path"] == "privatised" and plan["row_blocks"] == 16 and plan["rows"] * 16 == k, plan
        assert engine.count_plan(k + 1, pairs)["path"] == "global"
    elif name == "global_first_k":
        assert plan["path"] == "global", plan
        assert engine.count_plan(k - 1, pairs)["path"] == "privatised"          # the first k past the limit
    elif name == "global_k725":
        assert plan["path"] == "global", plan
    elif name == "bucket_key_space_limit":
        assert plan["path"] == "bucket" and plan["R"] * k == 16384 and plan["copies"] == 1, plan
        assert plan["chunk"] == 4096, plan
    elif name == "past_the_bucket_limit":
        assert pairs >= k * k and plan["path"] == "global", plan
    else:
        raise AssertionError(name)


@pytest.mark.parametrize("name,kind", [(nm, kd) for nm, v in ref.UNWEIGHTED_SHAPES.items() for kd in v[3]])
def test_unweighted(engine, name, kind):
    k, n, lag, _ = ref.UNWEIGHTED_SHAPES[name]
    pairs = ref.total_pairs(n, lag)
    _assert_unweighted_plan(engine, name, k, pairs)
    lab = _labels(kind, n, k)
    want, pw = ref.count_transitions(lab, k, lag)
    got, pg = _count(engine, lab, k, lag)
    np.testing.assert_array_equal(got, want)
    assert pg == pw


def test_normalised_at_the_key_space_limit(engine):
    k, n, lag, _ = ref.UNWEIGHTED_SHAPES["bucket_key_space_limit"]
    plan = engine.count_plan(k, ref.total_pairs(n, lag))
    assert plan["path"] == "bucket" and plan["R"] == 8 and plan["fuses_normalisation"], plan
    lab = _labels("markov", n, k)
    lab[(lab == 5) | (lab == k - 1)] = -1                      # two states never visited: zero rows stay zero
    dlab = engine.to_device(lab)
    c0, p0 = engine.count_transitions(dlab, k, lag, out=_junk(engine, (k, k), np.int64), pairs=_junk(engine, (1,), np.int64))
    T0, rs0, dm0 = _junk(engine, (k, k), np.float64), _junk(engine, (k,), np.float64), _junk(engine, (1,), np.float64)
    engine.row_normalise_into(c0, T0, rs0, dm0)
    T1, rs1, dm1 = _junk(engine, (k, k), np.float64), _junk(engine, (k,), np.float64), _junk(engine, (1,), np.float64)
    c1, p1 = engine.count_transitions_normalised(dlab, k, lag, T1, rs1, dm1, out=_junk(engine, (k, k), np.int64),
                                                 pairs=_junk(engine, (1,), np.int64))
    want, pw = ref.count_transitions(lab, k, lag)
    Tw, rsw, dmw = ref.row_normalise(want)
    c1h, T1h, rs1h = c1.to_host(), T1.to_host(), rs1.to_host()
    np.testing.assert_array_equal(c1h, want)
    assert int(p1.to_host()[0]) == int(p0.to_host()[0]) == pw
    np.testing.assert_array_equal(c1h, c0.to_host())
    for a, b in ((T1h, T0.to_host()), (rs1h, rs0.to_host()), (dm1.to_host(), dm0.to_host())):
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    np.testing.assert_array_equal(T1h, Tw)                      # one correctly rounded division per entry
    np.testing.assert_array_equal(rs1h, rsw)
    assert rs1h[5] == 0.0 and not T1h[5].any() and not T1h[k - 1].any()
    # trace(T) / k against the correctly rounded sum: k terms whose sum S is at most k, added in the kernel's order,
    # are within (k - 1) 2^-53 S of S, so S / k within (k - 1) 2^-53; the division rounds once more
    assert abs(float(dm1.to_host()[0]) - dmw) <= k * 2.0**-53


@pytest.mark.parametrize("kind", ["markov", "random"])
@pytest.mark.parametrize("name", list(ref.RAGGED_SHAPES))
def test_ragged_stride3(engine, name, kind):
    k, n, lag, stride, path = ref.RAGGED_SHAPES[name]
    segs = ref.ragged_segments(n)
    plan = engine.count_plan(k, ref.total_pairs(n, lag, segs, stride))
    assert plan["path"] == path, plan
    if path == "privatised":
        assert plan["pairs_per_chunk"] > 4096, plan
    lab = _labels(kind, n, k)
    want, pw = ref.count_transitions(lab, k, lag, segments=segs, stride=stride)
    got, pg = _count(engine, lab, k, lag, segs, stride)
    np.testing.assert_array_equal(got, want)
    assert pg == pw


# ---- weighted ------------------------------------------------------------------------------------------------------
def _assert_weighted_plan(name, plan, k, n_cu):
    if name == "budget_switch_small_side":
        assert plan["path"] == "privatised" and plan["row_blocks"] == 1 and plan["lds_bytes"] == 8 * k * k <= 65536, plan
    elif name == "budget_switch_large_side":
        assert plan["path"] == "privatised" and plan["row_blocks"] == 1 and plan["lds_bytes"] == 8 * k * k > 65536, plan
    elif name == "single_block_unrolled":
        assert plan["path"] == "privatised" and plan["row_blocks"] == 1 and plan["pairs_per_chunk"] > 4096, plan
        assert plan["chunks"] == n_cu, plan
    elif name == "several_row_blocks":
        assert plan["path"] == "privatised" and plan["row_blocks"] == 6, plan
    elif name == "sixteen_row_blocks":
        assert plan["path"] == "privatised" and plan["row_blocks"] == 16 and plan["lds_bytes"] == 131072, plan
    elif name == "global":
        assert plan["path"] == "global", plan
    else:
        raise AssertionError(name)


def _count_weighted(engine, lab_h, w_h, k, lag, segs=None, stride=1):
    kw = {}
    if segs is not None:
        kw["starts"], kw["stops"] = _bounds(segs)
    c, p = engine.count_transitions_weighted(engine.to_device(lab_h), engine.to_device(w_h), k, lag, stride=stride,
                                             out=_junk(engine, (k, k), np.float64), pairs=_junk(engine, (1,), np.int64),
                                             **kw)
    return c.to_host(), int(p.to_host()[0])


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("name", list(ref.WEIGHTED_SHAPES))
def test_weighted(engine, name, kind):
    k, n_of = ref.WEIGHTED_SHAPES[name]
    n_cu = _n_cu(engine)
    n, lag = n_of(n_cu), ref.WEIGHTED_LAG
    _assert_weighted_plan(name, engine.count_plan(k, ref.total_pairs(n, lag), weighted=True), k, n_cu)
    lab, w = _labels(kind, n, k), ref.integer_weights(n, k)
    want, pw, _, _ = ref.count_transitions_weighted(lab, w, k, lag)
    got, pg = _count_weighted(engine, lab, w, k, lag)
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))      # integer weights: exact in any order
    assert pg == pw


def test_weighted_ragged_stride3(engine):
    k, n, lag = 300, 300_000, ref.WEIGHTED_LAG
    segs = ref.ragged_segments(n)
    plan = engine.count_plan(k, ref.total_pairs(n, lag, segs, 3), weighted=True)
    assert plan["path"] == "privatised" and plan["row_blocks"] == 6, plan
    lab, w = _labels("markov", n, k), ref.integer_weights(n, k)
    want, pw, _, _ = ref.count_transitions_weighted(lab, w, k, lag, segments=segs, stride=3)
    got, pg = _count_weighted(engine, lab, w, k, lag, segs, 3)
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    assert pg == pw


def test_weighted_real_weights(engine):
    """Any order of m fp64 additions of the terms of a bin lies within (m - 1) u sum|w| (1 + O(m u)) of their exact
    sum, u = 2^-53 (Higham, Accuracy and Stability, eq. 4.4), and fsum within u |sum| of it: together below
    m 2^-52 sum|w|.  m and sum|w| per bin come from the reference; no fixed rtol."""
    k, n, lag = 300, 300_000, ref.WEIGHTED_LAG
    plan = engine.count_plan(k, ref.total_pairs(n, lag), weighted=True)
    assert plan["path"] == "privatised" and plan["row_blocks"] == 6, plan
    lab = _labels("markov", n, k)
    w = np.random.default_rng(5).lognormal(size=n)
    want, pw, terms, mass = ref.count_transitions_weighted(lab, w, k, lag)
    got, pg = _count_weighted(engine, lab, w, k, lag)
    assert pg == pw
    np.testing.assert_array_equal(got == 0.0, terms == 0)
    assert np.all(np.abs(got - want) <= terms * 2.0**-52 * mass)


# ---- lag scan and capture --------------------------------------------------------------------------------------------
def test_lagscan_across_paths(engine):
    k, n, lags = ref.LAGSCAN["k"], ref.LAGSCAN["n"], list(ref.LAGSCAN["lags"])
    paths = [engine.count_plan(k, ref.total_pairs(n, lag))["path"] for lag in lags]
    # pairs >= k^2 = 40000 up to lag 20000 (where pairs == k^2); 30000 pairs and fewer are privatised; lag n: no pair
    assert paths == ["bucket", "bucket", "bucket", "privatised", "privatised", "privatised", "none"], paths
    lab = _labels("markov", n, k)
    dlab = engine.to_device(lab)
    L = len(lags)
    for segs in (None, ref.LAGSCAN["segments"]):
        kw = {}
        if segs is not None:
            kw["starts"], kw["stops"] = _bounds(segs)
        c, p = engine.count_transitions_lagscan(dlab, k, lags, out=_junk(engine, (L, k, k), np.int64),
                                                pairs=_junk(engine, (L,), np.int64), **kw)
        ch, ph = c.to_host(), p.to_host()
        for i, lag in enumerate(lags):
            want, pw = ref.count_transitions(lab, k, lag, segments=segs)
            single, ps = engine.count_transitions(dlab, k, lag, out=_junk(engine, (k, k), np.int64),
                                                  pairs=_junk(engine, (1,), np.int64), **kw)
            np.testing.assert_array_equal(ch[i], want)
            np.testing.assert_array_equal(ch[i], single.to_host())
            assert int(ph[i]) == int(ps.to_host()[0]) == pw
    # d_pairs = NULL through the C ABI: the same matrices
    c2 = _junk(engine, (L, k, k), np.int64)
    s, e = _bounds(ref.LAGSCAN["segments"])
    la = np.asarray(lags, np.int32)
    st = _lib.load().msm_count_transitions_lagscan(engine.handle, dlab.ptr, n, s.ctypes.data, e.ctypes.data, len(s),
                                                   la.ctypes.data, L, k, c2.ptr, None)
    assert st == _lib.MSM_OK
    np.testing.assert_array_equal(c2.to_host(), ch)


def test_capture_falls_back_to_privatised():
    """A capture cannot grow the auxiliary scratch the bucket path needs, and a fresh context holds none: the call
    under capture runs count_lds_kernel (8 row blocks, 31250 pairs per chunk) where the eager call runs the bucket
    path.  Private engine; every buffer exists before the capture begins, and no eager call precedes it."""
    from pmarlo_amd.device import Engine

    k, n, lag = ref.CAPTURE["k"], ref.CAPTURE["n"], ref.CAPTURE["lag"]
    lab = _labels("markov", n, k)
    want, pw = ref.count_transitions(lab, k, lag)
    eng = Engine(0)
    try:
        dlab = eng.to_device(lab)
        c_cap, p_cap = _junk(eng, (k, k), np.int64), _junk(eng, (1,), np.int64)
        c_eag, p_eag = _junk(eng, (k, k), np.int64), _junk(eng, (1,), np.int64)
        pairs = ref.total_pairs(n, lag)
        assert eng.count_plan(k, pairs)["path"] == "bucket"
        eng.sync()
        eng.graph_begin()
        try:
            plan = eng.count_plan(k, pairs)
            eng.count_transitions(dlab, k, lag, out=c_cap, pairs=p_cap)
        finally:
            g = eng.graph_end()
        try:
            assert plan["path"] == "privatised" and plan["row_blocks"] == 8 and plan["pairs_per_chunk"] > 4096, plan
            eng.sync()
            assert (p_cap.to_host().view(np.uint64) == JUNK64).all()      # captured, not run
            eng.graph_launch(g)
            eng.sync()
            np.testing.assert_array_equal(c_cap.to_host(), want)
            assert int(p_cap.to_host()[0]) == pw
            c_cap.fill_bytes_(0x5A)
            p_cap.fill_bytes_(0x5A)
            eng.graph_launch(g)                                           # a replay clears and counts again
            eng.sync()
            np.testing.assert_array_equal(c_cap.to_host(), want)
            assert int(p_cap.to_host()[0]) == pw
        finally:
            eng.graph_destroy(g)
        assert eng.count_plan(k, pairs)["path"] == "bucket"
        eng.count_transitions(dlab, k, lag, out=c_eag, pairs=p_eag)
        np.testing.assert_array_equal(c_eag.to_host(), c_cap.to_host())
        assert int(p_eag.to_host()[0]) == pw
    finally:
        eng.close()


# ---- state visits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", [(_lib.STATE_COUNTS_LDS_MAX_K, ref.STATE_COUNTS_N),
                                 (_lib.STATE_COUNTS_LDS_MAX_K + 1, ref.STATE_COUNTS_N), (1, 1)])
def test_state_counts_lds_switch(engine, k, n):
    lab = _labels("random", n, k)
    if n > 100:
        lab[:64] = k - 1                                         # the last bin of the LDS table / first past it
    v = engine.state_counts(engine.to_device(lab), k, out=_junk(engine, (k,), np.int64))
    np.testing.assert_array_equal(v.to_host(), ref.state_counts(lab, k))
    assert int(v.to_host().sum()) == int(((lab >= 0) & (lab < k)).sum())


# ---- dwell runs ----------------------------------------------------------------------------------------------------------
def _run_lengths(engine, lab_h, k, capacity, null_lists=False):
    """msm_run_lengths through the C ABI -> (stats [4, k], run states, run lengths (whole junk-filled lists), n_runs)."""
    n = lab_h.size
    dlab = engine.to_device(lab_h)
    stats, cnt = _junk(engine, (4, k), np.int64), _junk(engine, (1,), np.int64)
    room = max(capacity, 1) + 8                                    # 8 guard entries behind the capacity
    rs, rl = _junk(engine, (room,), np.int32), _junk(engine, (room,), np.int64)
    st = _lib.load().msm_run_lengths(engine.handle, dlab.ptr, n, k, stats.ptr, None if null_lists else rs.ptr,
                                     None if null_lists else rl.ptr, capacity, cnt.ptr)
    assert st == _lib.MSM_OK, _lib.load().msm_last_error(engine.handle)
    return stats.to_host(), rs.to_host(), rl.to_host(), int(cnt.to_host()[0])


def _assert_run_lists(rs, rl, capacity, n_runs, lab_h, k):
    """min(capacity, runs) entries, each a real run and none twice; junk behind them."""
    st, ln, _ = ref.runs(lab_h, k)
    real = {}
    for pair in zip(st.tolist(), ln.tolist()):
        real[pair] = real.get(pair, 0) + 1
    m = min(capacity, n_runs)
    for pair in zip(rs[:m].tolist(), rl[:m].tolist()):
        assert real.get(pair, 0) > 0, pair
        real[pair] -= 1
    assert (rs[m:] == 0x5A5A5A5A).all() and (rl[m:].view(np.uint64) == JUNK64).all()
    if capacity >= n_runs:
        assert not any(real.values())


def test_run_lengths_capacity_below_the_number_of_runs(engine):
    k, n = 6, 50_000
    rng = np.random.default_rng(8)
    lab = np.repeat(rng.integers(-1, 9, size=n), rng.integers(1, 6, size=n))[:n].astype(np.int32)   # 6, 7, 8 >= k
    lab[::97] = ref.INT32_MAX
    lab[5::101] = ref.INT32_MIN
    st, ln, _ = ref.runs(lab, k)
    assert (lab >= k).any() and st.size > 5000
    for capacity in (st.size + 10, st.size, 1000, 1):
        stats, rs, rl, n_runs = _run_lengths(engine, lab, k, capacity)
        assert n_runs == st.size                                   # the true number, whatever fits the lists
        np.testing.assert_array_equal(stats, ref.run_stats(lab, k))
        _assert_run_lists(rs, rl, capacity, n_runs, lab, k)
    stats, _, _, n_runs = _run_lengths(engine, lab, k, 0, null_lists=True)
    assert n_runs == st.size
    np.testing.assert_array_equal(stats, ref.run_stats(lab, k))


def test_run_lengths_one_run_alternating_and_single(engine):
    n = ref.RUN_LENGTHS_N
    one = np.full(n, 2, np.int32)                                   # the thread of frame 0 walks all of it
    stats, rs, rl, n_runs = _run_lengths(engine, one, 4, 4)
    assert n_runs == 1 and (int(rs[0]), int(rl[0])) == (2, n)
    np.testing.assert_array_equal(stats, ref.run_stats(one, 4))
    _assert_run_lists(rs, rl, 4, 1, one, 4)
    alt = np.tile(np.asarray([0, 3], np.int32), n // 2)             # n runs of one frame
    stats, rs, rl, n_runs = _run_lengths(engine, alt, 4, n)
    assert n_runs == n
    np.testing.assert_array_equal(stats, ref.run_stats(alt, 4))
    _assert_run_lists(rs, rl, n, n, alt, 4)
    sep = np.tile(np.asarray([1, 1, 4, 1, 9, 9], np.int32), 1000)   # labels >= k end a run; they start none
    stats, rs, rl, n_runs = _run_lengths(engine, sep, 4, sep.size)
    assert n_runs == 2000 and stats[:, 1].tolist() == [1, 2, 3000, 2000]
    np.testing.assert_array_equal(stats, ref.run_stats(sep, 4))
    _assert_run_lists(rs, rl, sep.size, n_runs, sep, 4)
    for lab, want in ((np.asarray([1], np.int32), 1), (np.asarray([7], np.int32), 0), (np.asarray([-1], np.int32), 0)):
        stats, rs, rl, n_runs = _run_lengths(engine, lab, 3, 2)
        assert n_runs == want
        np.testing.assert_array_equal(stats, ref.run_stats(lab, 3))
        _assert_run_lists(rs, rl, 2, n_runs, lab, 3)
