"""msm_autocorr_lagscan, the device canonical correlations and compute_diagnostics on the GPU, against
tests/golden/diagnostics.* (made by importing the reference) and the numpy restatement of the kernel's definition
in tests/_diagnostics_ref.py.

Bounds: curve and kernel values 1e-11 absolute (the reference itself is within 1e-14 of a long-double evaluation on
these inputs, a fixed-order fp64 tree sum is in the same class); tau_int 1e-9 relative; lag_window and
recommended_ck_lags exact; canonical correlations 1e-10 absolute against QR-SVD on inputs with
cond(Cxx), cond(Cyy) <= 1e6, and no further from the reference's sorted values than the exact answer is
(the gap g stored with each fixture, plus 1e-9)."""

from __future__ import annotations

import json

import numpy as np
import pytest

from tests import _diagnostics_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

ATOL = 1e-11


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLDEN / "diagnostics.json").read_text())


@pytest.fixture(scope="module")
def D():
    from pmarlo_amd.analysis import diagnostics
    return diagnostics


def _bounds(lengths):
    stops = np.cumsum(np.asarray(lengths, np.int64))
    return stops - np.asarray(lengths, np.int64), stops


def _assert_curve(got, want):
    assert got["taus"] == want["taus"]
    g, w = np.asarray(got["values"]), np.asarray(want["values"], np.float64)
    print("max |values - golden| =", np.nanmax(np.abs(g - w)), " tau_int", got["tau_int"], want["tau_int"])
    np.testing.assert_allclose(g, w, rtol=0, atol=ATOL, equal_nan=True)
    assert got["tau_int"] == pytest.approx(want["tau_int"], rel=1e-9, nan_ok=True)
    assert (list(got["lag_window"]) if got["lag_window"] is not None else None) == want["lag_window"]
    assert got["recommended_ck_lags"] == want["recommended_ck_lags"]


# ---- 1. the curve against the reference's _autocorrelation_curve ---------------------------------------------
@pytest.mark.parametrize("case", sorted(R.CURVE_CASES))
def test_curve_matches_reference(case, gold, golden, D):
    offset, dtype = R.CURVE_CASES[case]
    x = R.curve_input(offset, dtype)
    segs = [D._SegmentDescriptor(length=L, stride=1) for L in R.CURVE_SEGMENTS]
    got = D._autocorrelation_curve(x, R.CURVE_LAGS, segs)
    want = dict(gold["curves"][case])
    want["values"] = golden("diagnostics.npz")[f"curve_values__{case}"]
    _assert_curve(got, want)


def test_curve_kernel_masks_the_constant_column_in_its_segment_only(engine):
    x = R.curve_input(0.0, np.float64)
    starts, stops = _bounds(R.CURVE_SEGMENTS)
    values, nvalid = engine.autocorr_lagscan(engine.to_device(x), R.CURVE_LAGS, starts=starts, stops=stops)
    assert nvalid.to_host().tolist() == [5, 0, 4, 5]
    values = values.to_host()
    assert np.isnan(values[1]).all()                                     # the length-1 segment
    lags = np.asarray(R.CURVE_LAGS)
    for s, L in enumerate(R.CURVE_SEGMENTS):
        assert np.array_equal(np.isnan(values[s]), lags >= L) or L <= 1


# ---- 2. the kernel against the numpy restatement of its definition ---------------------------------------------
def _uneven_segments(rng, n_seg, total):
    cuts = np.sort(rng.choice(np.arange(1, total), size=n_seg - 1 - 4, replace=False))
    lengths = np.diff(np.concatenate([[0], cuts, [total]])).tolist()
    for pos, L in ((3, 0), (9, 1), (17, 2), (30, 1)):                     # empty and tiny segments among them
        lengths.insert(pos, L)
    return lengths


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("F", [1, 2, 3, 7, 10, 16, 33, 64, 100, 256])
def test_kernel_matches_definition(engine, F, dtype):
    """40 uneven segments (more than travel by value), row stride ld > F, 70 lags (more than one launch takes)
    with a lag of L - 1 and lags >= L for several segments.  At F = 256 a chunk is 16 rows, so the 40 000 rows make
    more chunks than the grid has workgroups (a workgroup holds several segments); at small F a segment spans
    several chunks (several workgroups share a segment)."""
    rng = np.random.default_rng(1000 + F)
    n = 40_000 if F == 256 else 12_000
    lengths = _uneven_segments(rng, 40, n - 50)                          # the last 50 rows belong to no segment
    starts, stops = _bounds(lengths)
    starts, stops = starts + 7, stops + 7                                # nor do the first 7
    ld = F + 3
    coefs = rng.uniform(0.0, 0.98, size=F)
    buf = rng.standard_normal((n, ld)) * 1e3                             # the padding columns hold other numbers
    buf[:, :F] = R.ar1(rng, n, coefs) * rng.uniform(0.1, 10.0, size=F) + rng.uniform(-50, 50, size=F)
    buf = buf.astype(dtype)
    big = sorted(lengths)[-3:]
    lags = sorted(set([1, 2, 3, 5, 8, 13, 15, 16, 17, 31, 32, 33] + [L - 1 for L in big] + big
                      + rng.integers(1, max(big) + 50, size=70).tolist()))
    assert len(lags) > 64
    want, want_valid = R.autocorr_lagscan_ref(buf[:, :F], starts, stops, lags)
    xd = engine.to_device(buf)
    values, nvalid = engine.autocorr_lagscan(xd.view((n, F)), lags, starts=starts, stops=stops, ld=ld)
    got = values.to_host()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isfinite(want).sum() > 200
    print(f"F={F} {np.dtype(dtype).name}: max |kernel - definition| =", np.nanmax(np.abs(got - want)))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, equal_nan=True)
    assert np.array_equal(nvalid.to_host(), want_valid)


def test_kernel_chunks_of_several_tiles(engine):
    """More than 8192 tiles of 16 rows: a chunk then holds several tiles and the workgroup carries its sums across
    them.  150 000 x 256 float32; the definition is evaluated in float64 here (long double would need 6 GB)."""
    rng = np.random.default_rng(5)
    n, F = 150_000, 256
    x = (R.ar1(rng, n, rng.uniform(0.0, 0.95, size=F)) + 3.0).astype(np.float32)
    lengths = [70_000, 30_001, 49_999]
    starts, stops = _bounds(lengths)
    lags = [1, 7, 16, 40, 1000, 29_999, 30_000, 30_001, 69_999]
    want, want_valid = R.autocorr_lagscan_ref(x, starts, stops, lags, acc=np.float64)
    values, nvalid = engine.autocorr_lagscan(engine.to_device(x), lags, starts=starts, stops=stops)
    got = values.to_host()
    print("max |kernel - definition| =", np.nanmax(np.abs(got - want)))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, equal_nan=True)
    assert np.array_equal(nvalid.to_host(), want_valid)


def test_valid_columns_either_side_of_the_floor(engine):
    rng = np.random.default_rng(9)
    n = 5000
    u = rng.standard_normal((n, 6))
    u = (u - u.mean(axis=0)) / u.std(axis=0)                              # unit population variance
    var = np.array([1e-7, 1e-9, 1.0, 1e-9, 1e-7, 0.0])                    # a factor 10 above / below 1e-8
    x = u * np.sqrt(var) + 5.0
    starts, stops = _bounds([n])
    values, nvalid = engine.autocorr_lagscan(engine.to_device(x), [1, 2], starts=starts, stops=stops)
    assert nvalid.to_host().tolist() == [3]
    want, _ = R.autocorr_lagscan_ref(x, starts, stops, [1, 2])
    np.testing.assert_allclose(values.to_host(), want, rtol=0, atol=ATOL)
    _, nvalid = engine.autocorr_lagscan(engine.to_device(x), [1], starts=starts, stops=stops, var_floor=1e-10)
    assert nvalid.to_host().tolist() == [5]


def test_kernel_rejects_what_it_does_not_support(engine):
    x = engine.to_device(np.zeros((100, 4)))
    with pytest.raises(NotImplementedError):
        engine.autocorr_lagscan(engine.to_device(np.zeros((10, 257))), [1])
    with pytest.raises(ValueError):
        engine.autocorr_lagscan(x, [0, 1])
    with pytest.raises(ValueError):
        engine.autocorr_lagscan(x, [])
    with pytest.raises(ValueError):
        engine.autocorr_lagscan(x, [1], starts=np.array([0, 50]), stops=np.array([50, 101]))
    with pytest.raises(ValueError):
        engine.autocorr_lagscan(x, [1], starts=np.array([60]), stops=np.array([50]))
    with pytest.raises(TypeError):
        engine.autocorr_lagscan(engine.to_device(np.zeros((10, 2), np.int32)), [1])


# ---- 3. non-finite input ------------------------------------------------------------------------------------------
def test_non_finite_segment_is_nan_and_leaves_the_others(engine, gold, D):
    x = R.nonfinite_input()
    starts, stops = _bounds(R.NONFINITE_SEGMENTS)
    values, nvalid = engine.autocorr_lagscan(engine.to_device(x), R.NONFINITE_LAGS, starts=starts, stops=stops)
    values = values.to_host()
    assert np.isnan(values[1]).all() and nvalid.to_host().tolist() == [2, 0, 2]
    clean = x.copy()
    clean[3500, 0] = clean[4100, 1] = 0.0
    want, _ = engine.autocorr_lagscan(engine.to_device(clean), R.NONFINITE_LAGS, starts=starts, stops=stops)
    want = want.to_host()
    assert np.array_equal(values[[0, 2]], want[[0, 2]], equal_nan=True)   # untouched: the same bits
    assert np.isfinite(values[0, :-1]).all() and np.isfinite(values[2]).all()
    segs = [D._SegmentDescriptor(length=L, stride=1) for L in R.NONFINITE_SEGMENTS]
    _assert_curve(D._autocorrelation_curve(x, R.NONFINITE_LAGS, segs), gold["curves"]["nonfinite"])


# ---- 4. determinism -----------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(engine):
    x = R.curve_input(1000.0, np.float64)
    starts, stops = _bounds(R.CURVE_SEGMENTS)
    xd = engine.to_device(x)
    first = [a.to_host() for a in engine.autocorr_lagscan(xd, R.CURVE_LAGS, starts=starts, stops=stops)]
    engine.autocorr_lagscan(xd, [3, 4], starts=starts[:1], stops=stops[:1])          # other work in between
    second = [a.to_host() for a in engine.autocorr_lagscan(xd, R.CURVE_LAGS, starts=starts, stops=stops)]
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


# ---- 5. canonical correlations ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CCA_CASES))
def test_canonical_correlations(name, gold, D):
    X, Y = R.cca_input(name)
    entry = gold["cca"][name]
    assert max(entry.get("cond_cxx", entry.get("cond_cxx_reduced")), entry["cond_cyy"]) <= 1e6
    got = np.asarray(D._canonical_correlations(X, Y))
    want = R.cca_expected(name)
    print(name, "max |device - classical| =", np.abs(got - want).max())
    assert len(got) == min(entry["p"], entry["q"], entry["n"])
    assert np.all(np.diff(got) <= 0) and got.min() >= 0.0 and got.max() <= 1.0
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)
    if "reference_sorted" in entry:
        gap = np.abs(got - np.asarray(entry["reference_sorted"])).max()
        print(name, "max |device - sorted(reference)| =", gap, " g =", entry["gap_reference_to_classical"])
        assert gap <= entry["gap_reference_to_classical"] + 1e-9
    else:
        assert got[-1] == 0.0                                            # the rank-deficient block: zeros, no raise


def test_canonical_correlations_truncate_to_the_common_length(D):
    X, Y = R.cca_input("n3000_p4_q2")
    got = D._canonical_correlations(X[:2500], Y)
    np.testing.assert_allclose(got, R.cca_classical(X[:2500], Y[:2500]), rtol=0, atol=1e-10)
    got32 = D._canonical_correlations(X.astype(np.float32), Y)
    np.testing.assert_allclose(got32, R.cca_classical(X.astype(np.float32), Y), rtol=0, atol=1e-10)


def test_canonical_correlation_exceptions(D):
    ok = np.random.default_rng(0).standard_normal((10, 2))
    with pytest.raises(D.InsufficientSamplesError):
        D._canonical_correlations(ok[:1], ok)
    with pytest.raises(D.CanonicalCorrelationError):
        D._canonical_correlations(ok[:, 0], ok)
    bad = ok.copy()
    bad[3, 1] = np.nan
    with pytest.raises(D.CanonicalCorrelationError):
        D._canonical_correlations(bad, ok)
    with pytest.raises(NotImplementedError):
        D._canonical_correlations(np.zeros((10, 200)) + ok[:, :1], np.zeros((10, 57)) + ok[:, :1])
    wide = np.random.default_rng(1).standard_normal((400, 256))
    assert len(D._canonical_correlations(wide[:, :250], wide[:, 250:])) == 6         # p + q = 256 is served


# ---- 6. compute_diagnostics end to end ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.E2E_CASES))
def test_compute_diagnostics_matches_reference(name, gold):
    from pmarlo_amd.analysis import compute_diagnostics

    _, _, diag_mass, taus = R.E2E_CASES[name]
    entry = gold["end_to_end"][name]
    want = entry["result"]
    got = compute_diagnostics(R.e2e_dataset(name), diag_mass=diag_mass, taus=taus)
    assert list(got) == list(want)
    assert got["taus"] == want["taus"] and got["diag_mass"] == want["diag_mass"]
    assert got["warnings"] == want["warnings"]
    assert list(got["autocorrelation"]) == list(want["autocorrelation"])
    for split, curve in want["autocorrelation"].items():
        assert list(got["autocorrelation"][split]) == list(curve)
        _assert_curve(got["autocorrelation"][split], curve)
    assert list(got["canonical_correlation"]) == list(want["canonical_correlation"])
    for split, corr in want["canonical_correlation"].items():
        g = np.asarray(got["canonical_correlation"][split])
        gap = np.abs(g - np.sort(corr)[::-1]).max()
        print(name, split, "max |device - sorted(reference)| =", gap, " g =", entry["gap_reference_to_classical"][split])
        assert len(g) == len(corr) and np.all(np.diff(g) <= 0)
        assert gap <= entry["gap_reference_to_classical"][split] + 1e-9


def test_compute_diagnostics_segment_lengths_must_add_up(gold):
    from pmarlo_amd.analysis import compute_diagnostics

    ds = R.e2e_dataset("auto_taus_reparam_high_mass")
    ds["splits"]["train"]["segment_lengths"] = [2500, 3000]
    want = gold["end_to_end"]["segments_do_not_add_up"]
    with pytest.raises(ValueError) as info:
        compute_diagnostics(ds)
    assert str(info.value) == want["message"]
