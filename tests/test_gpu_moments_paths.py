"""The fused standardise + project kernels and the column statistics of csrc/moments.hip on every launch path.

Each project row of tests/_moments_ref.CASES runs through msm_project and msm_project_finite on a wide buffer [n, ld]
whose pad columns hold 2^100 (and, in a further run, NaN), into an output [n + 16, ldy] filled with 2^100, with the
absmax slot preloaded with 2^100; Y is compared with np.testing.assert_array_equal against exact_project.  The data
are integers and dyadic rationals whose partial sums are all exact in fp64, so a correct kernel is bit-equal to the
reference whatever order the matrix cores or the LDS tiles add in, and the exact tests hold no tolerance.  The moments
rows compare the raw sums [cnt | S1 | S2] the same way.  tests/test_moments_reference.py proves on the CPU that the
rows reach the branches they name.  Further tests place NaNs where each kernel reads them, put an inf into one frame
or one column, compare inexact data under a derived per-element bound, check mean / std / scale against rational
arithmetic, run the minima / maxima kernel over special values, and interleave the entry points that share the
engine's scratch.

Observed on an MI355X (the tests print it): every exact row is bit-equal; mean is up to 1 ulp, std and scale up to 2 ulp
from the rational value rounded once, so those are asserted under their derived bounds, not for equality; the worst
rounding error of a projected element is 0.17 of its bound.

Not covered: the number of resident workgroups per compute unit comes from the occupancy query and is not visible from
here (the rows that need a second round are sized for the largest possible value, 8)."""

from __future__ import annotations


import numpy as np
import pytest

from tests import _moments_ref as mr

pytestmark = pytest.mark.gpu

PAD_ROWS = 16          # a store that forgot t < n stays inside the buffer (a group is 16 frames) and is seen
GUARD = 64
OUT_FILL = -1234.5625
LD = np.longdouble


@pytest.fixture(scope="module")
def n_cu(engine) -> int:
    return engine.info()["n_cu"]


# ---------------------------------------------------------------------------------------------------------------------
# project
# ---------------------------------------------------------------------------------------------------------------------
def _adhoc(n, F, d, dtype, *, ld=None, off=0, ldw=None, ldy=None, mean2=True, family="small", seed=1):
    return {"kind": "project", "name": f"adhoc-n{n}-F{F}-d{d}-{dtype}", "n": n, "F": F, "d": d, "dtype": dtype,
            "ld": F if ld is None else ld, "off": off, "ldw": d if ldw is None else ldw, "ldy": d if ldy is None else ldy,
            "mean2": mean2, "family": family, "reach": {}, "seed": seed}


def _upload_x(engine, X, dtype: str, ld: int, off: int, pad):
    """X as the left block of a buffer [n, ld] that starts `off` elements into an allocation; everything else is `pad`."""
    n, F = X.shape
    host = np.full(off + n * ld, pad, mr.NP_DTYPE[dtype])
    host[off:].reshape(n, ld)[:, :F] = X
    buf = engine.to_device(host)
    return buf.view((n, F), offset_elems=off)


class _Params:
    def __init__(self, engine, mu, isg, m2, W):
        self.mu, self.isg, self.W = engine.to_device(mu), engine.to_device(isg), engine.to_device(W)
        self.m2 = engine.to_device(m2) if m2 is not None else None


def _project(engine, row: dict, X, par: _Params, *, pad=mr.SENTINEL, finite=False, absmax=True):
    """One call -> (Y [n, d], absmax or None) after checking that the pad columns and the rows past n still hold 2^100."""
    n, d, ldy = row["n"], row["d"], row["ldy"]
    x = _upload_x(engine, X, row["dtype"], row["ld"], row["off"], pad)
    out = engine.to_device(np.full((n + PAD_ROWS, ldy), mr.SENTINEL))
    slot = engine.to_device(np.array([mr.SENTINEL])) if absmax else None
    engine.project(x, par.mu, par.isg, par.W, d, mean2=par.m2, out=out.view((n, ldy)), absmax=slot,
                   assume_finite=finite, ld=row["ld"])
    host = out.to_host()
    np.testing.assert_array_equal(host[n:], mr.SENTINEL, err_msg=f"{row['name']}: rows past n written")
    np.testing.assert_array_equal(host[:n, d:], mr.SENTINEL, err_msg=f"{row['name']}: pad columns of Y written")
    return host[:n, :d], (float(slot.to_host()[0]) if absmax else None)


def _absmax_of(Y) -> float:
    return float(np.abs(Y).max(initial=0.0))


@pytest.mark.parametrize("row", mr.project_rows(), ids=mr.ids(mr.project_rows()))
def test_project_row_is_exact(engine, n_cu, row):
    want = dict(row["reach"])
    if not mr.loop_is_forced(row, n_cu, 8):
        del want["loops"]
    miss = mr.covers(mr.row_path(row, n_cu, 8), want)
    assert not miss, (n_cu, row["name"], miss)                      # on THIS device too
    X, mu, isg, m2, W = mr.project_data(row)
    ref = mr.exact_project(X, mu, isg, m2, W, row["d"])
    par = _Params(engine, mu, isg, m2, W)
    runs = [("plain", mr.SENTINEL, False), ("finite", mr.SENTINEL, True)]
    if row["ld"] > row["F"] or row["off"]:
        runs.append(("NaN in the pad columns", np.nan, False))
    for tag, pad, finite in runs:
        Y, amax = _project(engine, row, X, par, pad=pad, finite=finite)
        np.testing.assert_array_equal(Y, ref, err_msg=f"{row['name']} [{tag}]")
        assert amax == _absmax_of(ref), (row["name"], tag, amax, _absmax_of(ref))


_KERNEL_SHAPES = [   # (kernel, n, F, d, ld, off): a tail group / tile everywhere, pad columns, several workgroups
    ("mfma_vec", 37, 48, 3, 52, 4), ("mfma_vec", 133, 80, 16, 80, 0), ("mfma_vec", 70, 128, 5, 128, 0),
    ("mfma_scalar", 37, 17, 3, 19, 1), ("mfma_scalar", 133, 64, 16, 66, 0),
    ("generic", 70, 70, 17, 71, 1), ("generic", 133, 16, 40, 16, 0), ("generic", 37, 368, 3, 368, 0),
]
_KERNEL_IDS = [f"{k}-n{n}-F{F}-d{d}" for k, n, F, d, _, _ in _KERNEL_SHAPES]


def _shape_row(n_cu, kernel, n, F, d, ld, off, dtype, **kw):
    row = _adhoc(n, F, d, dtype, ld=ld, off=off, ldy=d + 1, ldw=d + 2, **kw)
    assert mr.row_path(row, n_cu)["kernel"] == kernel, row["name"]
    return row


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kernel,n,F,d,ld,off", _KERNEL_SHAPES, ids=_KERNEL_IDS)
def test_project_imputes_nan_wherever_it_is_read(engine, n_cu, kernel, n, F, d, ld, off, dtype):
    """NaN -> z = 0 before m2 is subtracted: at feature 0, at feature F - 1 (the last live slot of a chunk with dead q
    slots, which the clamped loads of those slots read again), at F16 - 4 (the first feature they read), in frame n - 1
    (n % 16 != 0: the lanes past n load it again), in a whole row and in a whole column."""
    row = _shape_row(n_cu, kernel, n, F, d, ld, off, dtype, seed=F + n)
    assert n % 16 != 0 and n % 64 != 0
    X, mu, isg, m2, W = mr.project_data(row)
    par = _Params(engine, mu, isg, m2, W)
    f_clamp = max(0, ((F + 15) // 16) * 16 - 4) if F % 16 == 0 else F // 2
    places = {"feature 0": [(0, 0), (20, 0)], "feature F - 1": [(5, F - 1), (n - 2, F - 1)],
              "first clamped feature": [(9, f_clamp)], "last frame": [(n - 1, 0), (n - 1, F - 1), (n - 1, F // 3)],
              "whole row": [(7, f) for f in range(F)], "whole last row": [(n - 1, f) for f in range(F)],
              "whole column": [(t, min(2, F - 1)) for t in range(n)]}
    everything = X.copy()
    for tag, where in places.items():
        Xn = X.copy()
        for t, f in where:
            Xn[t, f] = everything[t, f] = np.nan
        Y, amax = _project(engine, row, Xn, par)
        ref = mr.exact_project(Xn, mu, isg, m2, W, d)
        assert np.all(np.isfinite(Y)), (row["name"], tag)
        np.testing.assert_array_equal(Y, ref, err_msg=f"{row['name']} [{tag}]")
        assert amax == _absmax_of(ref), (row["name"], tag)
    Y, _ = _project(engine, row, everything, par, pad=np.nan)
    np.testing.assert_array_equal(Y, mr.exact_project(everything, mu, isg, m2, W, d), err_msg=f"{row['name']} [all]")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kernel,n,F,d,ld,off", _KERNEL_SHAPES, ids=_KERNEL_IDS)
def test_project_keeps_a_bad_frame_to_itself(engine, n_cu, kernel, n, F, d, ld, off, dtype):
    """One frame of +inf (the last one, which the lanes past n load again; then an interior one) leaves every other
    frame's output bit-equal to the run without it; so does a frame of NaN.  The inf frame's own values are free."""
    row = _shape_row(n_cu, kernel, n, F, d, ld, off, dtype, seed=3 * F + n)
    X, mu, isg, m2, W = mr.project_data(row)
    par = _Params(engine, mu, isg, m2, W)
    clean, _ = _project(engine, row, X, par)
    np.testing.assert_array_equal(clean, mr.exact_project(X, mu, isg, m2, W, d))
    for t in (n - 1, 18):
        other = np.arange(n) != t
        for value, cols in ((np.inf, slice(None)), (np.inf, [F - 1]), (-np.inf, [0]), (np.nan, slice(None))):
            Xb = X.copy()
            Xb[t, cols] = value
            Y, _ = _project(engine, row, Xb, par, absmax=False)
            np.testing.assert_array_equal(Y[other], clean[other], err_msg=f"{row['name']}: frame {t} = {value}")
            if np.isnan(value):
                np.testing.assert_array_equal(Y, mr.exact_project(Xb, mu, isg, m2, W, d))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kernel,F,d", [("mfma_vec", 48, 3), ("mfma_scalar", 17, 5), ("generic", 20, 17)])
def test_project_absmax(engine, n_cu, kernel, F, d, dtype):
    """max |Y| is reset by every call (the slot starts at 2^100), is 0 without frames, and arrives when a single
    workgroup raises it: X = mu without m2 gives Y = 0 in every frame but one."""
    n = 1000
    row = _adhoc(n, F, d, dtype, mean2=False, seed=F)
    path = mr.row_path(row, n_cu)
    assert path["kernel"] == kernel and path["grid"] >= 16
    X, mu, isg, m2, W = mr.project_data(row)
    assert m2 is None
    par = _Params(engine, mu, isg, None, W)
    for t in (777, 0, n - 1):
        Xo = np.tile(mu, (n, 1))
        Xo[t] = X[t]
        ref = mr.exact_project(Xo, mu, isg, None, W, d)
        assert np.count_nonzero(np.abs(ref).max(axis=1)) == 1
        for finite in (False, True):
            Y, amax = _project(engine, row, Xo, par, finite=finite)
            np.testing.assert_array_equal(Y, ref)
            assert amax == _absmax_of(ref) > 0.0, (t, finite, amax)
    Y, amax = _project(engine, row, np.tile(mu, (n, 1)), par)          # nobody raises it
    assert amax == 0.0 and not Y.any()
    empty = dict(row, n=0)
    Y, amax = _project(engine, empty, np.zeros((0, F)), par)
    assert Y.shape == (0, d) and amax == 0.0
    with pytest.raises(ValueError):
        engine.project(_upload_x(engine, X, dtype, F, 0, 0.0), par.mu, par.isg, par.W, d, ld=F - 1)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kernel,n,F,d,ld,off", _KERNEL_SHAPES, ids=_KERNEL_IDS)
def test_project_rounding_is_within_the_dot_product_bound(engine, n_cu, kernel, n, F, d, ld, off, dtype):
    """Inexact data with a large common offset.  Per element
        |Y - Y_ref| <= (F + 4) 2^-53 (sum_f |x_f - mu_f| |inv_sigma_f W_fc| + sum_f |m2_f W_fc|):
    the classical bound of a dot product of F terms plus the roundings of x - mu, inv_sigma * W (or (x - mu) * inv_sigma
    and - m2 in the generic kernel) and the accumulator start; the reference is evaluated in long double."""
    row = _shape_row(n_cu, kernel, n, F, d, ld, off, dtype)
    rng = np.random.default_rng(F * d)
    X = (1e6 + rng.standard_normal((n, F))).astype(mr.NP_DTYPE[dtype]).astype(np.float64)
    mu = 1e6 + 0.1 * rng.standard_normal(F)
    isg, m2 = rng.uniform(0.5, 2.0, F), 0.01 * rng.standard_normal(F)
    W = np.full((F, row["ldw"]), mr.SENTINEL)
    W[:, :d] = rng.standard_normal((F, d))
    par = _Params(engine, mu, isg, m2, W)
    Zl = (X.astype(LD) - mu.astype(LD)) * isg.astype(LD) - m2.astype(LD)
    ref = Zl @ W[:, :d].astype(LD)
    weight = np.abs(X.astype(LD) - mu.astype(LD)) @ np.abs(isg[:, None].astype(LD) * W[:, :d].astype(LD)) \
        + (np.abs(m2)[:, None].astype(LD) * np.abs(W[:, :d]).astype(LD)).sum(axis=0)[None, :]
    bound = (F + 4) * LD(2.0) ** -53 * weight
    for finite in (False, True):
        Y, amax = _project(engine, row, X, par, finite=finite)
        err = np.abs(Y.astype(LD) - ref)
        worst = float((err / bound).max())
        print(f"{row['name']} finite={finite}: worst error / bound = {worst:.3f}")
        assert np.all(err <= bound), (row["name"], finite, worst, int(np.argmax(err / bound)))
        assert amax == _absmax_of(Y)


# ---------------------------------------------------------------------------------------------------------------------
# column moments
# ---------------------------------------------------------------------------------------------------------------------
def _partial(engine, X, dtype: str, ld: int, shift, pad=mr.SENTINEL):
    """msm_column_moments_partial into a guarded block -> (sums [3F], shift [F]) on the host and the device arrays."""
    n, F = X.shape
    x = _upload_x(engine, X, dtype, ld, 0, pad)
    blk = engine.to_device(np.full(GUARD + 3 * F + GUARD, OUT_FILL))
    shift_d = engine.to_device(shift) if shift is not None else None
    sums_d, used_d = engine.column_moments_partial(x, shift_d, sums=blk.view((3 * F,), offset_elems=GUARD), ld=ld)
    host = blk.to_host()
    np.testing.assert_array_equal(host[:GUARD], OUT_FILL)
    np.testing.assert_array_equal(host[GUARD + 3 * F:], OUT_FILL)
    return host[GUARD:GUARD + 3 * F], used_d.to_host(), sums_d, used_d, x


def _ulps(got, ref):
    return np.abs(got - ref) / np.spacing(np.abs(ref))


def _check_finalize(engine, sums, used, sums_d, used_d, n_rows: int, tag):
    """mean / std / count and mean / scale / inv_scale of the device against rational arithmetic on the same sums."""
    F = len(used)
    worst = {"mean": 0.0, "std": 0.0}
    for ddof in (0, 1):
        mean, std, cnt = (a.to_host() for a in engine.moments_finalize(sums_d, used_d, F, ddof=ddof))
        rmean, rstd, rcnt = mr.finalize(sums, used, ddof)
        np.testing.assert_array_equal(cnt, rcnt, err_msg=f"{tag} count")
        assert np.all(_ulps(mean, rmean) <= 2.0), (tag, ddof, float(_ulps(mean, rmean).max()))
        np.testing.assert_array_equal(np.isnan(std), np.isnan(rstd), err_msg=f"{tag} ddof={ddof}: NaN std")
        for f in range(F):
            if sums[f] - ddof > 0:
                lo, hi = mr.std_interval(sums, f, F, int(sums[f]) - ddof)
                assert lo <= std[f] <= hi, (tag, ddof, f, lo, std[f], hi)
        ok = ~np.isnan(rstd) & (rstd > 0)
        worst["mean"] = max(worst["mean"], float(_ulps(mean, rmean).max()))
        worst["std"] = max(worst["std"], float(_ulps(std[ok], rstd[ok]).max(initial=0.0)))
    for with_std in (True, False):
        mean, scale, inv = (a.to_host() for a in engine.standardise_params(sums_d, used_d, F, float(n_rows), with_std))
        rmean, rscale, _ = mr.standardise(sums, used, n_rows, with_std)
        assert np.all(_ulps(mean, rmean) <= 2.0), (tag, with_std)
        np.testing.assert_array_equal(inv, 1.0 / scale, err_msg=f"{tag}: inv_scale is the IEEE quotient")
        for f in range(F):
            if not with_std or not sums[f] > 0 or rscale[f] == 1.0 and mr.variance(sums, f, F, n_rows) == 0:
                assert scale[f] == 1.0, (tag, with_std, f, scale[f])
            else:
                lo, hi = mr.std_interval(sums, f, F, n_rows)
                assert lo > 1e-12 and lo <= scale[f] <= hi, (tag, f, lo, scale[f], hi)
        worst["std"] = max(worst["std"], float(_ulps(scale, rscale).max()))
    print(f"{tag}: worst distance from the rational value rounded once: mean {worst['mean']:.2f} ulp, "
          f"std / scale {worst['std']:.2f} ulp")


@pytest.mark.parametrize("row", mr.moments_rows(), ids=mr.ids(mr.moments_rows()))
def test_moments_row_is_exact(engine, n_cu, row):
    miss = mr.covers(mr.row_path(row, n_cu), row["reach"])
    assert not miss, (n_cu, row["name"], miss)
    X, shift = mr.moments_data(row)
    ref, ref_shift = mr.exact_column_sums(X, shift)
    for pad in (mr.SENTINEL, np.nan) if row["ld"] > row["F"] else (mr.SENTINEL,):
        sums, used, sums_d, used_d, x = _partial(engine, X, row["dtype"], row["ld"], shift, pad)
        np.testing.assert_array_equal(sums, ref, err_msg=row["name"])
        np.testing.assert_array_equal(used, ref_shift, err_msg=f"{row['name']} shift")
    _check_finalize(engine, sums, used, sums_d, used_d, row["n"], row["name"])
    if shift is None:                     # the one-call entry: the same sums about row 0, finalised
        mean, std, cnt = (a.to_host() for a in engine.column_moments(x, ddof=1, ld=row["ld"]))
        m2_, s2_, c2_ = (a.to_host() for a in engine.moments_finalize(sums_d, used_d, row["F"], ddof=1))
        np.testing.assert_array_equal(mean, m2_)
        np.testing.assert_array_equal(std, s2_)
        np.testing.assert_array_equal(cnt, c2_)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_moments_special_columns(engine, dtype):
    """All-NaN column (count 0, mean 0, std 0, scale 1), a single entry (std NaN at ddof = 1), a constant column
    (std 0, scale = inv_scale = 1), a NaN in row 0 under the implicit shift (that column's shift is 0)."""
    n, F, ld = 300, 9, 11
    row = {"name": "special", "n": n, "F": F, "dtype": dtype, "family": "small", "shift": False, "seed": 5}
    X, _ = mr.moments_data(row)
    X[:, 1] = np.nan
    X[1:, 2] = np.nan
    X[:, 3] = 7.0
    X[0, 4] = np.nan
    X[17, 5] = X[n - 1, 5] = np.nan
    X[:, 6] = np.nan
    X[n - 1, 6] = 21.0
    for shift in (None, np.arange(F, dtype=np.float64) + 9.0):
        ref, ref_shift = mr.exact_column_sums(X, shift)
        sums, used, sums_d, used_d, _ = _partial(engine, X, dtype, ld, shift)
        np.testing.assert_array_equal(sums, ref)
        np.testing.assert_array_equal(used, ref_shift)
        if shift is None:
            assert used[1] == 0.0 and used[4] == 0.0 and used[6] == 0.0 and used[2] == X[0, 2]
        assert sums[1] == 0 and sums[2] == 1 and sums[6] == 1 and sums[5] == n - 2 and sums[4] == n - 1
        _check_finalize(engine, sums, used, sums_d, used_d, n, f"special-{dtype}-{'implicit' if shift is None else 'given'}")
        mean, std, cnt = (a.to_host() for a in engine.moments_finalize(sums_d, used_d, F, ddof=1))
        assert (cnt[1], mean[1], std[1]) == (0.0, 0.0, 0.0)
        assert np.isnan(std[2]) and mean[2] == X[0, 2] and np.isnan(std[6]) and mean[6] == 21.0
        assert std[3] == 0.0 and mean[3] == 7.0
        mean, std, cnt = (a.to_host() for a in engine.moments_finalize(sums_d, used_d, F, ddof=0))
        assert std[2] == 0.0 and std[6] == 0.0 and std[1] == 0.0
        mean, scale, inv = (a.to_host() for a in engine.standardise_params(sums_d, used_d, F, float(n), True))
        assert scale[1] == inv[1] == 1.0 and scale[3] == inv[3] == 1.0 and scale[2] == 1.0 and mean[1] == 0.0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("F,n", [(5, 700), (256, 90), (300, 40)])
def test_moments_keep_a_bad_column_to_itself(engine, F, n, dtype):
    row = {"name": "isolation", "n": n, "F": F, "dtype": dtype, "family": "wide", "shift": True, "seed": F}
    X, shift = mr.moments_data(row)
    ref, _ = mr.exact_column_sums(X, shift)
    for bad, value, rows in ((0, np.inf, [3]), (F - 1, -np.inf, [n - 1]), (F // 2, np.nan, range(n)), (F // 2, np.inf, [0, 5])):
        Xb = X.copy()
        Xb[list(rows), bad] = value
        for sh in (shift, None):
            sums, used, *_ = _partial(engine, Xb, dtype, F + 1, sh)
            want, want_shift = mr.exact_column_sums(Xb, sh)
            keep = np.tile(np.arange(F) != bad, 3)
            np.testing.assert_array_equal(sums[keep], want[keep])
            if sh is not None:
                np.testing.assert_array_equal(sums[keep], ref[keep])
            np.testing.assert_array_equal(sums[:F], want[:F])              # the count of the bad column as well
            if np.isnan(value):
                np.testing.assert_array_equal(sums, want)
                np.testing.assert_array_equal(used, want_shift)


# ---------------------------------------------------------------------------------------------------------------------
# minima and maxima
# ---------------------------------------------------------------------------------------------------------------------
def _minmax(engine, X, dtype: str, ld: int):
    x = _upload_x(engine, X, dtype, ld, 0, mr.SENTINEL)
    mn, mx, cnt = engine.column_minmax(x, ld=ld)
    return mn.to_host(), mx.to_host(), cnt.to_host()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_minmax_special_values(engine, dtype):
    np_t = mr.NP_DTYPE[dtype]
    big, tiny = float(np.finfo(np_t).max), float(np.finfo(np_t).smallest_subnormal)
    n = 600
    rng = np.random.default_rng(8)
    cols = {
        "mixed": rng.integers(-1000, 1001, n) / 8.0,
        "all negative": -1.0 - rng.integers(0, 1000, n) / 4.0,
        "all positive": 0.5 + rng.integers(0, 1000, n) / 4.0,
        "single value": np.full(n, -7.5),
        "both zeros": np.where(np.arange(n) % 2 == 0, -0.0, 0.0),
        "only -0": np.full(n, -0.0),
        "only +0": np.full(n, 0.0),
        "subnormals": np.where(np.arange(n) % 3 == 0, -tiny, np.where(np.arange(n) % 3 == 1, tiny, 3 * tiny)),
        "zero and subnormals": np.where(np.arange(n) % 2 == 0, 0.0, tiny),
        "largest": np.where(np.arange(n) == 311, big, np.where(np.arange(n) == 597, -big, rng.standard_normal(n).astype(np_t))),
        "FLT_MAX": np.where(np.arange(n) == 5, float(np.finfo(np.float32).max), 1.0),
        "nothing finite": np.where(np.arange(n) % 3 == 0, np.nan, np.where(np.arange(n) % 3 == 1, np.inf, -np.inf)),
        "all NaN": np.full(n, np.nan),
        "one finite": np.where(np.arange(n) == n - 1, -3.25, np.nan),
        "inf beside finite": np.where(np.arange(n) % 7 == 0, np.inf, np.where(np.arange(n) % 7 == 1, -np.inf, rng.integers(-9, 10, n))),
    }
    X = np.stack(list(cols.values()), axis=1).astype(np_t).astype(np.float64)
    names = list(cols)
    for ld in (X.shape[1], X.shape[1] + 2):
        mn, mx, cnt = _minmax(engine, X, dtype, ld)
        rmn, rmx, rcnt = mr.minmax(X)
        np.testing.assert_array_equal(mn, rmn)        # by value: NaN == NaN, -0 == +0
        np.testing.assert_array_equal(mx, rmx)
        np.testing.assert_array_equal(cnt, rcnt)
        # bit for bit where no zero is involved
        nz = (rmn != 0) & ~np.isnan(rmn)
        np.testing.assert_array_equal(mn[nz].view(np.int64), rmn[nz].view(np.int64))
        nz = (rmx != 0) & ~np.isnan(rmx)
        np.testing.assert_array_equal(mx[nz].view(np.int64), rmx[nz].view(np.int64))
        # which zero: the order-preserving image puts -0 below +0
        z = {k: names.index(k) for k in ("both zeros", "only -0", "only +0", "zero and subnormals")}
        assert np.signbit(mn[z["both zeros"]]) and not np.signbit(mx[z["both zeros"]])
        assert np.signbit(mn[z["only -0"]]) and np.signbit(mx[z["only -0"]])
        assert not np.signbit(mn[z["only +0"]]) and not np.signbit(mx[z["only +0"]])
        assert not np.signbit(mn[z["zero and subnormals"]]) and mx[z["zero and subnormals"]] == tiny
        assert mn[names.index("largest")] == -big and mx[names.index("largest")] == big
        assert mn[names.index("subnormals")] == -tiny and mx[names.index("subnormals")] == 3 * tiny


@pytest.mark.parametrize("F", [1, 255, 256, 257, 1000])
def test_minmax_feature_counts_and_counters(engine, F):
    rng = np.random.default_rng(F)
    for dtype, n in (("f32", 300), ("f64", 1)):
        X = rng.integers(-10 ** 6, 10 ** 6, size=(n, F)).astype(np.float64)
        bad = rng.random((n, F)) < 0.02
        X[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
        if n > 1:
            X[:, F - 1] = np.nan
            X[n // 2, :] = np.inf
        for ld in (F, F + 3):
            mn, mx, cnt = _minmax(engine, X, dtype, ld)
            rmn, rmx, rcnt = mr.minmax(X)
            np.testing.assert_array_equal(mn, rmn)
            np.testing.assert_array_equal(mx, rmx)
            np.testing.assert_array_equal(cnt, rcnt)
    # no rows at all: nothing finite anywhere, both counters 0
    mn, mx, cnt = _minmax(engine, np.zeros((0, F)), "f64", F)
    assert np.all(np.isnan(mn)) and np.all(np.isnan(mx)) and cnt.tolist() == [0, 0]


def test_minmax_rows_beyond_the_first_round(engine, n_cu):
    n, F = 700_000, 2
    assert mr.minmax_path(n, F, n_cu)["second_row"]
    X = (np.arange(n * F, dtype=np.float64).reshape(n, F) % 1013) - 500.0
    X[n - 3, 0], X[n - 2, 1] = -70000.0, 90000.0          # the extremes sit in rows only a second round reaches
    X[n - 1, 0], X[n - 5, 1], X[5, 0] = np.nan, np.inf, -np.inf
    mn, mx, cnt = _minmax(engine, X, "f32", F)
    rmn, rmx, rcnt = mr.minmax(X)
    np.testing.assert_array_equal(mn, rmn)
    np.testing.assert_array_equal(mx, rmx)
    assert mn[0] == -70000.0 and mx[1] == 90000.0 and cnt.tolist() == [3, n - 3] == rcnt.tolist()


def test_minmax_refuses_more_columns_than_its_lds_holds(engine):
    """A host-side argument check: 2 * F * 8 bytes of LDS per workgroup, 64 KiB without opting in."""
    x = engine.to_device(np.zeros((2, mr.MINMAX_MAX_F + 1), np.float32))
    with pytest.raises(ValueError, match="at most 4096 columns"):
        engine.column_minmax(x)
    mn, mx, cnt = engine.column_minmax(engine.to_device(np.ones((2, mr.MINMAX_MAX_F), np.float32)))
    assert np.all(mn.to_host() == 1.0) and np.all(mx.to_host() == 1.0) and cnt.to_host().tolist() == [0, 2]


# ---------------------------------------------------------------------------------------------------------------------
# the scratch the entry points share
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_that_share_the_scratch_do_not_read_each_other(engine, n_cu):
    """column_moments, column_minmax, project, lagged_moments and transition_matrix all use ctx->scratch.  Interleaved
    in two orders on one engine, each gives the bits it gave the first time (and those are the reference's)."""
    rng = np.random.default_rng(12)
    mrow = {"name": "scratch", "n": 20_000, "F": 64, "dtype": "f32", "family": "wide", "shift": False, "seed": 3}
    Xm, _ = mr.moments_data(mrow)
    xm = engine.to_device(Xm.astype(np.float32))
    prow = _adhoc(500, 48, 3, "f32", seed=4)
    grow = _adhoc(500, 48, 20, "f64", seed=6)
    pdata, gdata = mr.project_data(prow), mr.project_data(grow)
    ppar, gpar = _Params(engine, *pdata[1:]), _Params(engine, *gdata[1:])
    Xl = rng.integers(-3, 4, size=(501, 16)).astype(np.float64)
    xl, shl = engine.to_device(Xl.astype(np.float32)), engine.to_device(np.ones(16))
    counts = engine.to_device(rng.integers(0, 50, size=(60, 60)).astype(np.int64))
    Xmm = rng.integers(-99, 100, size=(3000, 1000)).astype(np.float64)
    xmm = engine.to_device(Xmm.astype(np.float32))

    def moments():
        return np.concatenate([a.to_host() for a in engine.column_moments(xm, ddof=1)])

    def minmax():
        mn, mx, cnt = engine.column_minmax(xmm)
        return np.concatenate([mn.to_host(), mx.to_host(), cnt.to_host().astype(np.float64)])

    ops = {"column_moments": moments, "column_minmax": minmax,
           "project (matrix cores)": lambda: _project(engine, prow, pdata[0], ppar)[0],
           "project (generic)": lambda: _project(engine, grow, gdata[0], gpar)[0],
           "lagged_moments": lambda: engine.lagged_moments(xl, 2, shl).to_host(),
           "transition_matrix": lambda: engine.transition_matrix(counts)["T"].to_host()}
    names = list(ops)
    first = {}
    for order in (names, names[::-1], [names[i] for i in (2, 0, 5, 1, 4, 3, 0, 2, 1)]):
        for name in order:
            out = ops[name]()
            if name in first:
                np.testing.assert_array_equal(out, first[name], err_msg=name)
            first.setdefault(name, out)
    np.testing.assert_array_equal(first["project (matrix cores)"], mr.exact_project(*pdata, 3))
    np.testing.assert_array_equal(first["project (generic)"], mr.exact_project(*gdata, 20))
    rmn, rmx, rcnt = mr.minmax(Xmm)
    np.testing.assert_array_equal(first["column_minmax"], np.concatenate([rmn, rmx, rcnt.astype(np.float64)]))
    sums, used = mr.exact_column_sums(Xm, None)
    np.testing.assert_array_equal(first["column_moments"][2 * 64:], sums[:64])
    assert np.all(_ulps(first["column_moments"][:64], mr.finalize(sums, used, 1)[0]) <= 2.0)
    c = counts.to_host().astype(np.float64)
    np.testing.assert_array_equal(first["transition_matrix"], c / c.sum(axis=1, keepdims=True))
