"""msm_metad_bias and msm_metad_grid_scan on every launch path, through Engine.metad_plan / metad_bias /
metad_grid_scan, against tests/_metad_ref.py run in 80-bit floats.

Bounds, none chosen from what the device gives.
  * A frame's bias and gradient: (6.25 (2 d + 3) + 4 + H_n) eps times the sum of the magnitudes of its terms, derived
    in tests/_metad_ref.py, where tests/test_metad_reference.py holds the fp64 restatement to the same bound.
  * Around the cutoff the law is the fp64 one (whether dp2 < cut is decided on the rounded fp64 dp2, which an 80-bit
    evaluation can decide the other way): those frames are held to the fp64 restatement, exactly 0 outside.
  * lse of the scan: a rounding of V moves a V by at most a bound_V, and log-sum-exp is a contraction in the maximum
    norm; the sum itself is a tree whose depth stays under log2 G + 6 roundings at these sizes (6 shuffle levels, 3
    adds over the waves, the tile merge), each at most eps / 2 relative, which the lse sees absolutely:
        |lse - exact| <= a max_g bound_V(g) + (log2 G + 6) eps max(1, |lse|).
Where two device results must agree exactly (default launch against max_workgroups = 1, a frame alone against the
same frame in a batch, any grid of the scan), assert_array_equal on the bits."""

from __future__ import annotations

import numpy as np
import pytest

from pmarlo_amd import _lib
from tests import _metad_ref as R

pytestmark = pytest.mark.gpu

W, T, TILE = _lib.METAD_THREADS, _lib.METAD_TILE, _lib.METAD_SCAN_TILE
H_LIST = (0, 1, T - 1, T, T + 1, 2 * T + 3)
N_LIST = (1, 63, 64, 65, W + 1)
H_MAX, N_MAX = max(H_LIST), max(N_LIST)


def _case(d: int, seed: int):
    """N_MAX frames and H_MAX hills with per-hill sigmas, half to two thirds of the pairs inside the cutoff."""
    rng = np.random.default_rng(seed)
    cv = rng.normal(size=(N_MAX, d))
    centers = rng.normal(size=(H_MAX, d))
    sigmas = rng.uniform(0.6, 1.4, size=(H_MAX, d)) * np.sqrt(d) * 0.4
    heights = rng.uniform(0.1, 1.5, size=H_MAX)
    counts = rng.integers(0, H_MAX + 1, size=N_MAX)
    return cv, R.pack(centers, sigmas, heights), counts


@pytest.fixture(scope="module")
def cases():
    """Per d: the inputs and, per kernel, the longdouble reference of all N_MAX x H_MAX terms, computed once."""
    out = {}
    for d in (1, 2, 8):
        cv, packed, counts = _case(d, 40 + d)
        terms = {k: R.hill_terms(cv, packed, kernel=k, dtype=np.longdouble) for k in R.KERNELS}
        frac = float((terms["gaussian"][0] != 0).mean())
        assert 0.2 < frac < 0.9, frac
        out[d] = (cv, packed, counts, {k: tuple(np.cumsum(a, axis=1) for a in v) for k, v in terms.items()})
    return out


def _want(prefix, counts):
    """(bias, grad, mag, gmag) at the counts from the sequential prefix sums."""
    return tuple(R._take(p[:counts.size], counts).astype(np.float64) for p in prefix)


def _check(got_b, got_g, want, counts, d, what):
    wb, wg, mag, gmag = want
    f = R.bound_factor(d, counts)
    assert np.isfinite(got_b).all(), what
    assert (np.abs(got_b - wb) <= f * mag).all(), (what, float(np.max(np.abs(got_b - wb) / np.maximum(f * mag, 1e-300))))
    assert not got_b[mag == 0].any(), what
    if got_g is not None:
        assert (np.abs(got_g - wg) <= f[:, None] * gmag).all(), what
        assert not got_g[gmag == 0].any(), what


def test_plan(engine):
    p = engine.metad_plan(N_MAX, H_MAX, 2)
    assert p["frames_per_workgroup"] == W and p["hills_per_tile"] == T and p["grid"] == 2
    assert p["lds_bytes"] == T * 5 * 8 + 4 and engine.metad_plan(N_MAX, H_MAX, 8)["lds_bytes"] == T * 17 * 8 + 4
    assert engine.metad_plan(10 ** 9, 5, 1)["grid"] == engine.info()["n_cu"] * 8
    assert engine.metad_plan(10 ** 9, 5, 1, max_workgroups=3)["grid"] == 3
    for bad in ((0, 1, 1), (1, -1, 1), (1, 1, 0), (1, 1, 9)):
        with pytest.raises(ValueError):
            engine.metad_plan(*bad)


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("d", [1, 2, 8])
def test_every_shape(engine, cases, d, kernel):
    """H x n x gradient on and off, all hills and ragged counts; default grid against one workgroup, bit for bit."""
    cv, packed, counts_all, prefix = cases[d]
    cvd = engine.to_device(cv)
    worst = 0.0
    for H in H_LIST:
        hills = engine.to_device(packed[:max(H, 1)])
        pre = tuple(p[:, :max(H, 1)] for p in prefix[kernel])
        for n in N_LIST:
            view = cvd.view((n, d))
            ragged = np.minimum(counts_all[:n], H).astype(np.int32)
            if n >= 2:
                ragged[0], ragged[1] = 0, H                       # 0 and H inside one wave
            for counts in (None, ragged):
                full = np.full(n, H, np.int32) if counts is None else counts
                want = _want(pre, full) if H else tuple(np.zeros((n,) + s) for s in ((), (d,), (), (d,)))
                cd = None if counts is None else engine.to_device(counts)
                kw = dict(kernel=kernel, counts=cd)
                b, g = engine.metad_bias(view, hills, H, grad=True, **kw)
                b, g = b.to_host(), g.to_host()
                _check(b, g, want, full, d, (d, kernel, H, n, counts is None))
                live = want[2] > 0
                if live.any():
                    worst = max(worst, float((np.abs(b - want[0])[live] / want[2][live]).max() / R.EPS))
                # value only: the same bits as with the gradient; one workgroup: the same bits as the default grid
                np.testing.assert_array_equal(engine.metad_bias(view, hills, H, **kw).to_host(), b)
                b1, g1 = engine.metad_bias(view, hills, H, grad=True, max_workgroups=1, **kw)
                np.testing.assert_array_equal(b1.to_host(), b)
                np.testing.assert_array_equal(g1.to_host(), g)
    print(f"d={d} {kernel}: largest |device - longdouble| = {worst:.1f} eps x sum of magnitudes "
          f"(bound {R.CUT * (2 * d + 3) + 4:.0f} + H_n)")


@pytest.mark.parametrize("d", [1, 2, 8])
def test_a_frame_alone_has_the_bits_it_has_in_a_batch(engine, cases, d):
    cv, packed, counts_all, _prefix = cases[d]
    H = 2 * T + 3
    hills = engine.to_device(packed)
    counts = counts_all.astype(np.int32)
    b, g = engine.metad_bias(engine.to_device(cv), hills, H, kernel="stretched-gaussian",
                             counts=engine.to_device(counts), grad=True)
    b, g = b.to_host(), g.to_host()
    for f in (0, 63, 64, 130, N_MAX - 1):
        b1, g1 = engine.metad_bias(engine.to_device(cv[f:f + 1]), hills, H, kernel="stretched-gaussian",
                                   counts=engine.to_device(counts[f:f + 1]), grad=True)
        assert b1.to_host()[0] == b[f]
        np.testing.assert_array_equal(g1.to_host()[0], g[f])
    # a wider row stride of the CVs and of the gradient changes nothing
    wide = np.full((N_MAX, d + 3), np.nan)
    wide[:, :d] = cv
    gout = engine.to_device(np.full((N_MAX, d + 2), -7.0))
    b2, g2 = engine.metad_bias(engine.to_device(wide), hills, H, kernel="stretched-gaussian",
                               counts=engine.to_device(counts), grad=True, grad_out=gout)
    np.testing.assert_array_equal(b2.to_host(), b)
    np.testing.assert_array_equal(g2.to_host()[:, :d], g)
    np.testing.assert_array_equal(g2.to_host()[:, d:], np.full((N_MAX, 2), -7.0))


def test_grid_stride_second_trip(engine, cases):
    """More trips than workgroups: frames of the second and third trip of a workgroup keep their bits."""
    cv, packed, _counts, _prefix = cases[2]
    rng = np.random.default_rng(9)
    big = np.concatenate([cv, rng.normal(size=(3 * W, 2))])           # 4 trips and one frame
    counts = rng.integers(0, 41, size=big.shape[0]).astype(np.int32)
    hills = engine.to_device(packed[:40])
    args = dict(kernel="gaussian", counts=engine.to_device(counts), grad=True)
    b, g = engine.metad_bias(engine.to_device(big), hills, 40, **args)
    for mw in (1, 2, 3):
        b1, g1 = engine.metad_bias(engine.to_device(big), hills, 40, max_workgroups=mw, **args)
        np.testing.assert_array_equal(b1.to_host(), b.to_host())
        np.testing.assert_array_equal(g1.to_host(), g.to_host())
    ref = R.bias(big, packed[:40], counts, dtype=np.longdouble)
    _check(b.to_host(), g.to_host(), tuple(ref[k].astype(np.float64) for k in ("bias", "grad", "mag", "gmag")),
           counts, 2, "grid stride")


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_periodic_cv(engine, kernel):
    """CV 0 has period 2: dp at exactly +-P/2 (rint keeps it), across the seam, and a non-periodic CV beside it."""
    P = 2.0
    packed = R.pack([[0.5, 0.1], [-0.875, -0.2], [0.9375, 0.0]], [[0.5, 0.6], [0.25, 0.5], [0.125, 0.4]], [1.0, 0.7, 1.3])
    cv = np.array([[-0.5, 0.0],          # hill 0: dp = -1 = -P/2 exactly
                   [1.5, 0.1],           # hill 0: dp = +1 = +P/2 exactly
                   [0.96875, 0.1],       # hill 1 across the seam: dp = 1.84375 -> -0.15625
                   [-0.9375, -0.1],      # hill 2 across the seam: dp = -1.875 -> 0.125
                   [4.5, 0.0],           # two periods out
                   [0.0, 0.0]])
    ref = R.bias(cv, packed, periods=[P, 0.0], kernel=kernel, dtype=np.longdouble)
    assert (ref["mag"] > 0).all()
    hills = engine.to_device(packed)
    b, g = engine.metad_bias(engine.to_device(cv), hills, 3, periods=[P, 0.0], kernel=kernel, grad=True)
    _check(b.to_host(), g.to_host(), tuple(ref[k].astype(np.float64) for k in ("bias", "grad", "mag", "gmag")),
           np.full(6, 3), 2, "periodic")
    # shifting a frame by whole periods (exact in fp64 here) changes nothing
    np.testing.assert_array_equal(b.to_host()[4], engine.metad_bias(engine.to_device(np.array([[0.5, 0.0]])), hills, 3,
                                                                    periods=[P, 0.0], kernel=kernel).to_host()[0])
    # without the period the seam frames lose hills 1 and 2
    plain = engine.metad_bias(engine.to_device(cv), hills, 3, kernel=kernel).to_host()
    assert plain[2] < b.to_host()[2] and plain[3] < b.to_host()[3]


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_one_ulp_around_the_cutoff(engine, kernel):
    x = np.sqrt(2 * R.CUT)
    around = [x]
    for _ in range(4):
        around = [np.nextafter(around[0], 0.0)] + around + [np.nextafter(around[-1], 9.0)]
    around = np.array(around)
    q = 0.5 * (around * around)
    below, above = around[q < R.CUT].max(), around[q >= R.CUT].min()
    assert np.nextafter(below, 9.0) == above
    cv = np.array([[below], [above], [-below], [-above]])
    packed = R.pack([[0.0]], [[1.0]], [0.8])
    b, g = engine.metad_bias(engine.to_device(cv), engine.to_device(packed), 1, kernel=kernel, grad=True)
    b, g = b.to_host(), g.to_host()[:, 0]
    ref = R.bias(cv, packed, kernel=kernel)
    assert b[1] == 0.0 and b[3] == 0.0 and g[1] == 0.0 and g[3] == 0.0
    f = R.bound_factor(1, [1, 1])
    for i in (0, 2):
        assert abs(b[i] - ref["bias"][i]) <= f[0] * ref["mag"][i] and abs(g[i] - ref["grad"][i, 0]) <= f[0] * ref["gmag"][i, 0]
        assert g[i] != 0.0 and np.sign(g[i]) == -np.sign(cv[i, 0])
    if kernel == "gaussian":
        assert b[0] == pytest.approx(0.8 * np.exp(-R.CUT), rel=1e-12)
    else:
        assert abs(b[0]) < 1e-14 and b[0] == b[2]            # the stretched kernel arrives at 0


# ------------------------------------------------------------------------------------------------------ the scan
def _scan_case(d: int, bins, H: int, seed: int):
    rng = np.random.default_rng(seed)
    lo, hi = -np.ones(d), np.ones(d)
    packed = R.pack(rng.uniform(-1, 1, size=(H, d)), rng.uniform(0.2, 0.6, size=(H, d)), rng.uniform(0.1, 1.0, size=H))
    return packed, R.grid_spec(lo, hi, bins)


def _check_scan(got, packed, grid, ck, a1, a2, kernel, what):
    lo, step, bins = grid
    want, _vh, bound_v = R.scan(packed, lo, step, bins, ck, a1, a2, kernel=kernel, dtype=np.longdouble)
    want = want.astype(np.float64)
    G = float(np.prod(bins))
    assert np.isfinite(got).all(), what
    for e, a in enumerate((a1, a2)):
        tol = a * bound_v + (np.log2(G) + 6) * R.EPS * np.maximum(1.0, np.abs(want[:, e]))
        assert (np.abs(got[:, e] - want[:, e]) <= tol).all(), (what, e, np.abs(got[:, e] - want[:, e]).max(), tol.min())


@pytest.mark.parametrize("bins", [(1,), (TILE - 1,), (TILE + 1,), (3 * TILE,), (17, 31), (5, 9, 13)])
def test_scan_shapes(engine, bins):
    """G = 1, tile - 1, tile + 1, 3 tiles, and a 2-d and a 3-d grid; M = 1 and H + 1; checkpoints 0 and H; a2 = 0;
    one hills tile and more (H = T + 5)."""
    d = len(bins)
    for H in (7, T + 5):
        packed, grid = _scan_case(d, bins, H, 70 + H + d)
        hills = engine.to_device(packed)
        lo, step, gb = grid
        for kernel in R.KERNELS:
            for ck, a1, a2 in ((np.arange(H + 1), 2.0, 0.25), ([H], 1.5, 0.0), ([0], 3.0, 1.0), ([0, 0, 3, H, H], 0.7, 0.7)):
                res = {}
                for mw in (0, 1, 2):
                    lse, vg = engine.metad_grid_scan(hills, H, lo, step, gb, ck, a1, a2, kernel=kernel, want_grid=True,
                                                     max_workgroups=mw)
                    res[mw] = (lse.to_host(), vg.to_host())
                for mw in (1, 2):
                    np.testing.assert_array_equal(res[mw][0], res[0][0])
                    np.testing.assert_array_equal(res[mw][1], res[0][1])
                got, vg = res[0]
                _check_scan(got, packed, grid, ck, a1, a2, kernel, (bins, H, kernel, len(ck)))
                ck = np.asarray(ck)
                log_g = np.log(float(np.prod(bins)))                 # V_0 = 0, or a = 0: the sum is G exactly
                assert (np.abs(got[ck == 0] - log_g) <= 2 * R.EPS * max(1.0, log_g)).all()
                assert (got[ck == 0][:, 0] == got[ck == 0][:, 1]).all()
                if a2 == 0.0:
                    assert (np.abs(got[:, 1] - log_g) <= 2 * R.EPS * max(1.0, log_g)).all()
                # V_H on the grid is the bias kernel's sum at the grid points, bit for bit
                pts = R.grid_points(lo, step, gb)
                direct = engine.metad_bias(engine.to_device(pts), hills, H, kernel=kernel).to_host()
                np.testing.assert_array_equal(vg.reshape(-1), direct)


def test_scan_periodic_axis(engine):
    rng = np.random.default_rng(3)
    per = [2 * np.pi, 0.0]
    packed = R.pack(np.stack([rng.uniform(-np.pi, np.pi, 9), rng.uniform(0, 1, 9)], axis=1), [[0.5, 0.2]] * 9,
                    rng.uniform(0.2, 1, 9))
    lo, step, bins = R.grid_spec([-np.pi, 0.0], [np.pi, 1.0], [24, 11], periods=per)
    assert step[0] == 2 * np.pi / 24 and step[1] == 0.1
    hills = engine.to_device(packed)
    lse, vg = engine.metad_grid_scan(hills, 9, lo, step, bins, np.arange(10), 1.2, 0.3, periods=per, want_grid=True)
    want, vh, bound_v = R.scan(packed, lo, step, bins, np.arange(10), 1.2, 0.3, periods=per, dtype=np.longdouble)
    tol = 1.2 * bound_v + (np.log2(264) + 6) * R.EPS * np.abs(want[:, 0].astype(np.float64))
    assert (np.abs(lse.to_host()[:, 0] - want[:, 0].astype(np.float64)) <= tol).all()
    direct = engine.metad_bias(engine.to_device(R.grid_points(lo, step, bins)), hills, 9, periods=per).to_host()
    np.testing.assert_array_equal(vg.to_host().reshape(-1), direct)


def test_scan_exponents_that_would_overflow(engine):
    """a1 V of about 800: exp(800) is not a double, the shifted sum is."""
    packed, grid = _scan_case(1, (TILE + 1,), 40, 11)
    lo, step, bins = grid
    vmax = float(R.scan(packed, lo, step, bins, [40], 0.0, 0.0)[1].max())
    a1 = 800.0 / vmax
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(a1 * vmax * 0.95))
    got = engine.metad_grid_scan(engine.to_device(packed), 40, lo, step, bins, np.arange(41), a1, a1 / 7)[0].to_host()
    _check_scan(got, packed, grid, np.arange(41), a1, a1 / 7, "gaussian", "overflow")
    assert 780.0 < got[-1, 0] < 820.0


def test_scan_refusals(engine):
    packed, grid = _scan_case(1, (10,), 4, 1)
    lo, step, bins = grid
    hills = engine.to_device(packed)
    for ck in ([3, 2], [-1], [5], []):
        with pytest.raises(ValueError):
            engine.metad_grid_scan(hills, 4, lo, step, bins, ck, 1.0, 0.0)
    for a1, a2 in ((1.0, 2.0), (1.0, -0.1), (np.inf, 0.0), (np.nan, 0.0)):
        with pytest.raises(ValueError):
            engine.metad_grid_scan(hills, 4, lo, step, bins, [4], a1, a2)
    with pytest.raises(ValueError):
        engine.metad_grid_scan(hills, 4, lo, step, [0], [4], 1.0, 0.0)
    with pytest.raises(ValueError):
        engine.metad_grid_scan(hills, 4, lo, step, bins, [4], 1.0, 0.0, cut=0.0)
    with pytest.raises(ValueError):
        engine.metad_grid_scan(engine.to_device(np.zeros((4, 9))), 4, [0] * 4, [1] * 4, [2] * 4, [4], 1.0, 0.0)   # d = 4
    neg = packed.copy()
    neg[2, -1] = -0.1
    with pytest.raises(ValueError, match="negative"):
        engine.metad_grid_scan(engine.to_device(neg), 4, lo, step, bins, [4], 1.0, 0.0)
    # only the first n_hills records are hills
    assert np.isfinite(engine.metad_grid_scan(engine.to_device(neg), 2, lo, step, bins, [2], 1.0, 0.0)[0].to_host()).all()
