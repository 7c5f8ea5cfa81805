"""The k-means++ seeding kernels (pmarlo_amd/csrc/kmeanspp.hip) on the paths tests/test_gpu_kmeanspp.py does not
reach.  Reference: oracle/npport.kmeans_plusplus; the frames drawn and the centres must be EQUAL.

  test_more_block_sums_than_threads   kpp_pick_kernel level 1 with per = ceil(n_blocks / MSM_KPP_BLOCK) = 3 (f64, d = 2)
                                      and 2 (f32, d = 1): the chunk walk of the owning thread, its early break, and
                                      several owning threads over the seeds
  test_planted_last_frame             the same n, every frame equal but frame n - 1: the second draw must be n - 1 --
                                      the last block sum of the last non-empty level-1 chunk, in a partial block (the
                                      walk passes the zero sums before it); the third draw has W = 0 (uniform)
  test_row_stride_with_nan_padding    ld = d + 3 through the C ABI, f32 and f64: kpp_coord's row stride in all three
                                      kernels; the padding is NaN and must never be read
  test_nan_rows_have_weight_zero      `if (!(m == m)) m = 0` of kpp_update_kernel: never drawn while W > 0
  test_data_scale                     kpp_scale (frexp / ldexp and its clamps) at data of size 1e-100, 1 and 1e100
  test_smallest_shapes                k = 1; n = k = 64 distinct frames (every frame drawn once); n = 1
  test_n_total_of_the_minibatch_caller  n_total = 5 n: a smaller scale, other integer weights
"""

from __future__ import annotations

import numpy as np
import pytest

from oracle import npport
from pmarlo_amd import _lib

pytestmark = pytest.mark.gpu

B = _lib.KPP_BLOCK


def _plusplus_abi(engine, x_dev, n, d, ld, k, seed, state, n_total=None):
    """msm_kmeans_init_plusplus with a row stride and a given state (slot 2 = max |x|) -> (picked, centres)."""
    dt = _lib.MSM_F32 if x_dev.dtype == np.float32 else _lib.MSM_F64
    cen = engine.empty((k, d), np.float64).fill_bytes_(0x5A)
    picked = engine.empty((k,), np.int64).fill_bytes_(0x5A)
    st = _lib.load().msm_kmeans_init_plusplus(engine.handle, x_dev.ptr, dt, n, d, ld, None, None, k, seed & (2**64 - 1),
                                              float(n if n_total is None else n_total), cen.ptr, state.ptr, picked.ptr)
    assert st == _lib.MSM_OK, _lib.load().msm_last_error(engine.handle)
    return picked.to_host(), cen.to_host()


def _state_of(engine, X, k, n_total=None):
    """The fit state (max |x| in slot 2) of NaN-free data, as msm_kmeans_fit_begin leaves it."""
    n = X.shape[0]
    _, state = engine.kmeans_fit_begin(engine.to_device(X), k, seed=0, n_total=n if n_total is None else n_total, tol2=0.0,
                                       init_centers=False)
    return state


BIG = [(2 * B * B + 77, 2, 5, np.float64, 3), (B * B + 1500, 1, 4, np.float32, 2)]


@pytest.fixture(scope="module")
def big_data():
    return {n: np.random.default_rng(n % 1000).normal(size=(n, d)).astype(dt) for n, d, _, dt, _ in BIG}


@pytest.mark.parametrize("n,d,k,dtype,per", BIG)
def test_more_block_sums_than_threads(engine, big_data, n, d, k, dtype, per):
    n_blocks = -(-n // B)
    assert -(-n_blocks // B) == per and n % B                      # per block sums a thread, a partial last block
    X = big_data[n]
    dX = engine.to_device(X)
    owners = set()
    for seed in (7, 11, 2**40 + 7):
        cen, picked = engine.kmeans_init_plusplus(dX, k, seed=seed, return_picked=True)
        want_idx, want_c = npport.kmeans_plusplus(X, k, seed)
        np.testing.assert_array_equal(picked.to_host(), want_idx)
        np.testing.assert_array_equal(cen.to_host(), want_c)
        owners |= {int(t) // B // per for t in want_idx[1:]}
    assert len(owners) >= 6 and max(owners) - min(owners) > 100, owners     # the draws are spread over the threads


@pytest.mark.parametrize("n,d,k,dtype,per", BIG)
def test_planted_last_frame(engine, n, d, k, dtype, per):
    X = np.ones((n, d), dtype)
    X[n - 1] = 3.0
    seed = next(s for s in range(100) if (npport._kpp_hash(s, 0) * n) >> 64 != n - 1)    # the first draw, on the CPU
    want_idx, want_c = npport.kmeans_plusplus(X, 3, seed)
    assert want_idx[0] != n - 1 and want_idx[1] == n - 1
    cen, picked = engine.kmeans_init_plusplus(engine.to_device(X), 3, seed=seed, return_picked=True)
    got = picked.to_host()
    assert got[1] == n - 1                                          # the last block sum, frame 76 / 475 of its block
    np.testing.assert_array_equal(got, want_idx)
    np.testing.assert_array_equal(cen.to_host(), want_c)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_row_stride_with_nan_padding(engine, dtype):
    n, d, k = 5003, 3, 17
    X = np.random.default_rng(2).normal(size=(n, d)).astype(dtype)
    P = np.full((n, d + 3), np.nan, dtype)
    P[:, :d] = X
    state = _state_of(engine, X, k)
    for seed in (0, 12345):
        want_idx, want_c = npport.kmeans_plusplus(X, k, seed)
        packed_idx, packed_c = _plusplus_abi(engine, engine.to_device(X), n, d, d, k, seed, state)
        got_idx, got_c = _plusplus_abi(engine, engine.to_device(P), n, d, d + 3, k, seed, state)
        np.testing.assert_array_equal(packed_idx, want_idx)
        np.testing.assert_array_equal(got_idx, want_idx)
        np.testing.assert_array_equal(got_c, want_c)
        np.testing.assert_array_equal(packed_c, want_c)


def test_nan_rows_have_weight_zero(engine):
    """The state comes from the data with its NaNs replaced by 0 (the same max |x|): what the kernels of this file do
    with a NaN coordinate is under test, not the max |x| pass of the fit."""
    n, d, k = 20_000, 4, 40
    rng = np.random.default_rng(6)
    X = rng.normal(size=(n, d))
    bad = rng.random(n) < 0.05
    X[bad, rng.integers(0, d, int(bad.sum()))] = np.nan              # one NaN coordinate is enough
    X[bad & (rng.random(n) < 0.5)] = np.nan                          # or the whole row
    state = _state_of(engine, np.nan_to_num(X, nan=0.0), k)
    dX = engine.to_device(X)
    clean = [s for s in range(50) if not bad[(npport._kpp_hash(s, 0) * n) >> 64]][:2]
    dirty = next(s for s in range(2000) if bad[(npport._kpp_hash(s, 0) * n) >> 64])
    for seed in clean + [dirty]:
        want_idx, want_c = npport.kmeans_plusplus(X, k, seed)
        got_idx, got_c = _plusplus_abi(engine, dX, n, d, d, k, seed, state)
        np.testing.assert_array_equal(got_idx, want_idx)
        np.testing.assert_array_equal(got_c, want_c)
    for seed in clean:                                              # a finite first centre: W > 0 at every draw
        assert not bad[npport.kmeans_plusplus(X, k, seed)[0]].any()


@pytest.mark.parametrize("size", [1e-100, 1.0, 1e100])
def test_data_scale(engine, size):
    n, d, k = 30_000, 3, 12
    X = np.random.default_rng(9).normal(size=(n, d)) * size
    want_idx, want_c = npport.kmeans_plusplus(X, k, 5)
    if size >= 1.0:
        assert len(set(want_idx.tolist())) == k                     # (at 1e-100 every weight rounds to 0: uniform draws)
    dX = engine.to_device(X)
    got_idx, got_c = _plusplus_abi(engine, dX, n, d, d, k, 5, _state_of(engine, X, k))
    np.testing.assert_array_equal(got_idx, want_idx)
    np.testing.assert_array_equal(got_c, want_c)


def test_smallest_shapes(engine):
    rng = np.random.default_rng(1)
    X = rng.normal(size=(500, 2))
    cen, picked = engine.kmeans_init_plusplus(engine.to_device(X), 1, seed=3, return_picked=True)
    want_idx, want_c = npport.kmeans_plusplus(X, 1, 3)
    np.testing.assert_array_equal(picked.to_host(), want_idx)
    np.testing.assert_array_equal(cen.to_host(), want_c)
    X = rng.normal(size=(64, 3))
    cen, picked = engine.kmeans_init_plusplus(engine.to_device(X), 64, seed=3, return_picked=True)
    want_idx, want_c = npport.kmeans_plusplus(X, 64, 3)
    np.testing.assert_array_equal(picked.to_host(), want_idx)
    np.testing.assert_array_equal(cen.to_host(), want_c)
    assert sorted(picked.to_host().tolist()) == list(range(64))     # a drawn frame has weight 0 afterwards
    X = rng.normal(size=(1, 5))
    cen, picked = engine.kmeans_init_plusplus(engine.to_device(X), 1, seed=8, return_picked=True)
    assert picked.to_host().tolist() == [0]
    np.testing.assert_array_equal(cen.to_host(), X)


def test_n_total_of_the_minibatch_caller(engine):
    n, d, k = 40_000, 3, 25
    X = np.random.default_rng(12).normal(size=(n, d))
    cen, picked = engine.kmeans_init_plusplus(engine.to_device(X), k, seed=4, n_total=5 * n, return_picked=True)
    want_idx, want_c = npport.kmeans_plusplus(X, k, 4, n_total=5 * n)
    np.testing.assert_array_equal(picked.to_host(), want_idx)
    np.testing.assert_array_equal(cen.to_host(), want_c)
