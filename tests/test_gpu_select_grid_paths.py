"""The radix selection (pmarlo_amd/csrc/select.hip) and the grid-microstate kernels (pmarlo_amd/csrc/grid.hip) on the
inputs their other tests (test_gpu_fes.py::test_order_statistics_radix_select, test_gpu_grid.py through
GridDiscretizer: fp64, ld == F, linspace edges) do not reach.  References: np.sort, np.digitize, np.unique.

msm_order_statistics (sortable_key, digit_histogram_kernel, the host's descent):
  test_select_nans_of_both_signs_sort_last   a NaN with the sign bit set (x86's inf - inf) must sort last like every
                                             NaN, not below every number; +-inf, denormals of both signs and +-0.0
                                             keep their ranks
  test_select_equal_column                   100 003 equal values: one bin holds everything at every digit
  test_select_last_digit                     40 consecutive doubles that straddle a multiple of 16 in their low bits:
                                             told apart only by the final, 4-bit digit (positive and negative)
  test_select_ranks_and_strides              ranks unsorted and repeated, n_ranks = 0, n = 1, stride 3 with a column offset
  test_select_refused_under_capture          MSM_ERR_UNSUPPORTED and its message; the capture stays valid

msm_grid_cells (grid_cells_kernel<float|double>, digitize_clip):
  test_grid_cells_irregular_edges            fp32 and fp64 rows, ld = F and F + 2 with NaN padding, quantile edges of a
                                             log-normal sample (bins = 37): the linear guess is wrong in both
                                             directions, so both correction loops walk; a value on every edge of every
                                             feature and nextafter either side of it; +-inf and NaN
  test_grid_cells_flat_index_below_2_31      F = 3, bins = 1290: the top corner is cell 2 146 688 999
  test_grid_cells_refuses_overflow           F = 2, bins = 46341: refused before any launch

msm_first_occurrence / msm_relabel (first_occurrence_kernel, relabel_kernel):
  test_first_occurrence_and_relabel          duplicates in the first and the last block, cells never seen (-1), indices
                                             < 0 and >= n_cells, n = 0, and n = 3 000 000 (every thread strides)
"""

from __future__ import annotations

import numpy as np
import pytest

from pmarlo_amd import _lib

pytestmark = pytest.mark.gpu

NEG_NAN = np.copysign(np.nan, -1.0)


# ---- msm_order_statistics -------------------------------------------------------------------------------------------
def _assert_ranks(got, col, ranks):
    """got[q] == np.sort(col)[ranks[q]]: bit for bit for numbers other than zero, any NaN where np.sort has a NaN."""
    want = np.sort(col)[np.asarray(ranks, np.int64)]
    np.testing.assert_array_equal(got, want)                        # (NaN == NaN and -0.0 == 0.0 here)
    strict = ~np.isnan(want) & (want != 0.0)
    np.testing.assert_array_equal(got[strict].view(np.uint64), want[strict].view(np.uint64))


def test_select_nans_of_both_signs_sort_last(engine):
    rng = np.random.default_rng(0)
    tiny = np.float64(5e-324)
    special = np.concatenate([
        np.full(300, np.nan), np.full(300, NEG_NAN), [np.inf] * 3, [-np.inf] * 4,
        tiny * rng.integers(1, 1000, 50), -tiny * rng.integers(1, 1000, 50), [0.0] * 20, [-0.0] * 30])
    assert np.signbit(special[300:600]).all() and np.isnan(special[:600]).all()
    col = np.concatenate([rng.normal(size=50_000), special])
    rng.shuffle(col)
    n, n_num = col.size, int((~np.isnan(col)).sum())
    srt = np.sort(col)
    z0 = int(np.searchsorted(srt, 0.0, side="left"))                # the 50 zeros sit at ranks z0 .. z0 + 49
    ranks = np.unique(np.concatenate([
        [0, 1, 3, 4, 5, z0 - 51, z0 - 50, z0 - 1, z0, z0 + 29, z0 + 30, z0 + 49, z0 + 50, z0 + 99, z0 + 100,
         n_num - 4, n_num - 3, n_num - 1, n_num, n_num + 299, n_num + 300, n - 1], rng.integers(0, n, 20)]))
    got = engine.order_statistics(engine.to_device(col), ranks)
    _assert_ranks(got, col, ranks)
    assert got[0] == -np.inf and not np.isnan(got[ranks < n_num]).any() and np.isnan(got[ranks >= n_num]).all()
    # np.sort leaves the order of -0.0 and +0.0 open; the radix key is a total order with -0.0 first
    zeros = got[(ranks >= z0) & (ranks < z0 + 50)]
    assert np.signbit(zeros).tolist() == [r < z0 + 30 for r in ranks[(ranks >= z0) & (ranks < z0 + 50)]]
    # every rank of a number is what it is without the NaNs
    clean = engine.order_statistics(engine.to_device(col[~np.isnan(col)]), ranks[ranks < n_num])
    np.testing.assert_array_equal(clean.view(np.uint64), got[ranks < n_num].view(np.uint64))


def test_select_equal_column(engine):
    col = np.full(100_003, -1.2345678901234567)
    got = engine.order_statistics(engine.to_device(col), [0, 50_001, 100_002])
    np.testing.assert_array_equal(got.view(np.uint64), col[:3].view(np.uint64))


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_select_last_digit(engine, sign):
    bits = np.uint64(0x3FF0000000000000) + np.uint64(16 * 1000 - 20) + np.arange(40, dtype=np.uint64)
    vals = bits.view(np.float64)
    assert (np.diff(vals) > 0).all() and vals[1] == np.nextafter(vals[0], 2.0)
    assert len(set((bits >> np.uint64(4)).tolist())) == 4          # three multiples of 16 inside: the 60-bit prefix changes
    col = np.repeat(sign * vals, 7)
    np.random.default_rng(3).shuffle(col)
    ranks = np.arange(col.size)
    got = engine.order_statistics(engine.to_device(col), ranks)
    _assert_ranks(got, col, ranks)


def test_select_ranks_and_strides(engine):
    rng = np.random.default_rng(5)
    X = rng.normal(size=(10_001, 3))
    X[::7, 1] = rng.integers(-3, 4, X[::7, 1].size)                 # ties
    dX = engine.to_device(X)
    ranks = [5, 0, 5, 10_000, 3, 3, 9_999, 0]
    for col in (0, 1, 2):                                           # stride 3, column offset 0 .. 2
        _assert_ranks(engine.order_statistics(dX, ranks, col=col), X[:, col], ranks)
    lib = _lib.load()
    # n_ranks = 0: nothing is written
    r0, out = np.zeros(1, np.int64), np.full(1, 7.5)
    assert lib.msm_order_statistics(engine.handle, dX.ptr, 3, 10_001, r0.ctypes.data, 0, out.ctypes.data) == _lib.MSM_OK
    assert out[0] == 7.5
    # n = 1 (of a strided column: the element at the offset alone)
    got = engine.order_statistics(engine.to_device(X[:1]), [0, 0], col=2)
    np.testing.assert_array_equal(got, [X[0, 2]] * 2)
    # a rank outside [0, n) is refused
    bad = np.asarray([10_001], np.int64)
    assert lib.msm_order_statistics(engine.handle, dX.ptr, 3, 10_001, bad.ctypes.data, 1, out.ctypes.data) == _lib.MSM_ERR_INVALID


def test_select_refused_under_capture():
    from pmarlo_amd.device import Engine

    eng = Engine(0)
    try:
        dX = eng.to_device(np.arange(100.0))
        r, out = np.zeros(1, np.int64), np.full(1, 7.5)
        lib = _lib.load()
        eng.sync()
        eng.graph_begin()
        st = lib.msm_order_statistics(eng.handle, dX.ptr, 1, 100, r.ctypes.data, 1, out.ctypes.data)
        msg = lib.msm_last_error(eng.handle)
        g = eng.graph_end()                                         # the (empty) capture is still valid
        eng.graph_destroy(g)
        assert st == _lib.MSM_ERR_UNSUPPORTED and b"polls the host: not capturable" in msg
        assert out[0] == 7.5
        np.testing.assert_array_equal(eng.order_statistics(dX, [99]), [99.0])     # and works eagerly afterwards
    finally:
        eng.close()


# ---- msm_grid_cells -----------------------------------------------------------------------------------------------------
def _digitize_ref(X, edges):
    """np.digitize(v, e) - 1 clipped to [0, bins - 1] per feature, flattened with int64 arithmetic."""
    bins = edges.shape[1] - 1
    flat = np.zeros(X.shape[0], np.int64)
    idx = []
    for f in range(edges.shape[0]):
        i = np.clip(np.digitize(X[:, f].astype(np.float64), edges[f]) - 1, 0, bins - 1)
        idx.append(i)
        flat = flat * bins + i
    return flat, np.stack(idx, axis=1)


def _grid_cells(engine, P, F, edges):
    """msm_grid_cells through the C ABI on rows of P (ld = P.shape[1] >= F) -> (status, flat int32 on the host)."""
    n, ld = P.shape
    dt = _lib.MSM_F32 if P.dtype == np.float32 else _lib.MSM_F64
    flat = engine.empty((n,), np.int32).fill_bytes_(0x5A)
    st = _lib.load().msm_grid_cells(engine.handle, engine.to_device(P).ptr, dt, n, F, ld, engine.to_device(edges).ptr,
                                    edges.shape[1] - 1, flat.ptr)
    engine.sync()
    return st, flat.to_host()


@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_grid_cells_irregular_edges(engine, dtype, pad):
    F, bins = 3, 37
    rng = np.random.default_rng(7)
    # a log-normal sample (the linear guess falls short: the second loop walks), its mirror image (the guess overshoots:
    # the first loop walks) and a mixture of both; edges a float32 holds exactly, so that a value can sit ON an edge in
    # either input type
    ln = rng.lognormal(sigma=1.2, size=(24_011, F))
    S = np.stack([ln[:, 0], -ln[:, 1], np.where(rng.random(ln.shape[0]) < 0.5, ln[:, 2], 12.0 - ln[:, 2])], axis=1)
    edges = np.quantile(S[:4000], np.linspace(0, 1, bins + 1), axis=0).T.astype(np.float32).astype(np.float64)
    assert edges.shape == (F, bins + 1) and (np.diff(edges, axis=1) > 0).all()
    X = S[4000:].astype(dtype)
    on = np.zeros((3 * (bins + 1), F), dtype)
    for f in range(F):
        e = edges[f].astype(dtype)
        on[:, f] = np.concatenate([e, np.nextafter(e, dtype(-np.inf)), np.nextafter(e, dtype(np.inf))])
    odd = np.asarray([[np.inf, -np.inf, np.nan], [np.nan, np.inf, -np.inf], [-np.inf, np.nan, np.inf],
                      [0.0, -0.0, 1e30], [-1e30, 5e-324 if dtype == np.float64 else 1e-45, -1.0]], dtype)
    X = np.concatenate([on, X, odd])
    want, idx = _digitize_ref(X, edges)
    # the inputs do what they are for: the linear guess misses by more than one bin, every bin and both clips occur
    over, under = [], []
    with np.errstate(invalid="ignore"):
        for f in range(F):
            v = X[:, f].astype(np.float64)
            inside = (v >= edges[f, 0]) & (v < edges[f, -1])
            guess = np.clip(((v[inside] - edges[f, 0]) * (bins / (edges[f, -1] - edges[f, 0]))).astype(np.int64), 0, bins - 1)
            over.append(bool((guess > idx[inside, f] + 1).any()))
            under.append(bool((guess < idx[inside, f] - 1).any()))
            assert set(idx[:, f].tolist()) == set(range(bins)) and (~inside).sum() > 10
    assert under[0] and over[1] and over[2] and under[2], (over, under)
    P = X
    if pad:
        P = np.full((X.shape[0], F + pad), np.nan, dtype)
        P[:, :F] = X
    st, got = _grid_cells(engine, P, F, edges)
    assert st == _lib.MSM_OK
    np.testing.assert_array_equal(got, want)


def test_grid_cells_flat_index_below_2_31(engine):
    F, bins = 3, 1290
    assert bins**F == 2_146_689_000 <= 2**31 - 1 < (bins + 1) ** F
    edges = np.tile(np.linspace(0.0, 1.0, bins + 1), (F, 1))
    rng = np.random.default_rng(2)
    top = np.asarray([[1.0, 1.0, 1.0], [np.nextafter(1.0, 0.0)] * 3, [2.0, np.inf, np.nan], [np.nan] * 3])
    X = np.concatenate([top, rng.random((5000, F)), 1.0 - rng.random((500, F)) * 1e-3])
    want, _ = _digitize_ref(X, edges)
    assert (want[:4] == 2_146_688_999).all() and (want >= 0).all() and (want[5004:] > 2**31 - 2**25).all()
    st, got = _grid_cells(engine, X, F, edges)
    assert st == _lib.MSM_OK
    np.testing.assert_array_equal(got.astype(np.int64), want)


def test_grid_cells_refuses_overflow(engine):
    F, bins = 2, 46341
    assert bins**F > 2**31 - 1 >= (bins - 1) ** F
    edges = np.tile(np.linspace(0.0, 1.0, bins + 1), (F, 1))
    st, got = _grid_cells(engine, np.random.default_rng(0).random((300, F)), F, edges)
    assert st == _lib.MSM_ERR_INVALID
    assert b"46341 bins in 2 dimensions overflow the cell index" in _lib.load().msm_last_error(engine.handle)
    assert (got == 0x5A5A5A5A).all()                                # refused before any launch


# ---- msm_first_occurrence / msm_relabel ----------------------------------------------------------------------------
def _first_and_relabel(engine, flat, n_cells, cell_map):
    lib = _lib.load()
    n = flat.size
    d_flat = engine.to_device(flat) if n else None
    first = engine.empty((n_cells,), np.int64).fill_bytes_(0x5A)
    assert lib.msm_first_occurrence(engine.handle, d_flat.ptr if n else None, n, n_cells, first.ptr) == _lib.MSM_OK
    labels = engine.empty((max(n, 1),), np.int32).fill_bytes_(0x5A)
    d_map = engine.to_device(cell_map)
    assert lib.msm_relabel(engine.handle, d_flat.ptr if n else None, n, d_map.ptr, n_cells, labels.ptr) == _lib.MSM_OK
    engine.sync()
    return first.to_host(), labels.to_host()


def _first_ref(flat, n_cells):
    ok = (flat >= 0) & (flat < n_cells)
    cells, idx = np.unique(flat[ok], return_index=True)
    want = np.full(n_cells, -1, np.int64)
    want[cells] = np.flatnonzero(ok)[idx]
    return want


def _relabel_ref(flat, n_cells, cell_map):
    ok = (flat >= 0) & (flat < n_cells)
    return np.where(ok, cell_map[np.where(ok, flat, 0)], -1).astype(np.int32)


@pytest.mark.parametrize("n", [3_000_000, 70_001])
def test_first_occurrence_and_relabel(engine, n):
    n_cells = 5000
    rng = np.random.default_rng(n)
    flat = rng.integers(0, n_cells - 500, n).astype(np.int32)        # the last 500 cells are never seen
    flat[flat == 77] = 78                                            # nor is cell 77 ...
    flat[[3, n - 2]] = 77                                            # ... but in the first and in the last block
    flat[[n - 1, n - 5]] = 4990                                      # a cell seen only at the very end
    flat[5::1009] = -1
    flat[6::1013] = n_cells
    flat[7::1019] = np.iinfo(np.int32).min
    flat[8::1021] = np.iinfo(np.int32).max
    cell_map = rng.permutation(n_cells).astype(np.int32)
    first, labels = _first_and_relabel(engine, flat, n_cells, cell_map)
    want = _first_ref(flat, n_cells)
    assert want[77] == 3 and want[4990] == n - 5 and (want[4500:4990] == -1).all()
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(labels, _relabel_ref(flat, n_cells, cell_map))


def test_first_occurrence_and_relabel_of_nothing(engine):
    first, labels = _first_and_relabel(engine, np.zeros(0, np.int32), 9, np.arange(9, dtype=np.int32))
    assert (first == -1).all() and (labels == 0x5A5A5A5A).all()
