"""Host logic of pmarlo_amd.analysis.diagnostics against tests/golden/diagnostics.json (made by the reference):
tau derivation and validation, the integrated autocorrelation time, the CK lag recommendation, the weighting of
per-segment values, and the algebra that turns joint moments into canonical correlations.  No GPU needed: nothing
here reaches the engine."""

from __future__ import annotations

import json
import math

import numpy as np
import pytest

from tests import _diagnostics_ref as R
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLDEN / "diagnostics.json").read_text())


@pytest.fixture(scope="module")
def D():
    from pmarlo_amd.analysis import diagnostics
    return diagnostics


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b


def _expect(entry, fn, *args, **kwargs):
    if "error" in entry:
        with pytest.raises(ValueError) as info:
            fn(*args, **kwargs)
        assert str(info.value) == entry["message"]
    else:
        assert fn(*args, **kwargs) == entry["ok"]


def test_compute_diagnostics_is_exported():
    from pmarlo_amd.analysis import compute_diagnostics
    from pmarlo_amd.analysis.diagnostics import compute_diagnostics as direct

    assert compute_diagnostics is direct


def test_derive_taus_table(gold, D):
    table = gold["host"]["derive_taus"]
    assert sum("error" in e for e in table) >= 12 and sum("ok" in e for e in table) >= 10
    for entry in table:
        _expect(entry, D.derive_taus, entry["lengths"], **entry["kwargs"])


def test_derive_taus_reads_segments_and_strides_of_a_dataset(gold, D):
    ds = {"splits": {"a": {"X": np.zeros((300, 2)) + np.arange(300)[:, None], "segments": [
        {"length": 120, "stride": 2}, {"start": 120, "stop": 300, "effective_frame_stride": 3}]},
        "b": np.arange(400.0).reshape(200, 2)}}
    _expect(gold["host"]["derive_taus_dataset"], D.derive_taus, ds)


def test_validate_user_taus(gold, D):
    table = gold["host"]["validate_user_taus"]
    assert sum("error" in e for e in table) >= 5
    for entry in table:
        _expect(entry, D._validate_user_taus, entry["taus"], entry["min_length"])
    assert D._validate_user_taus(np.array([1, 4, 9]), 8) == [1, 4, 9]


def test_prepare_tau_grid(gold, D):
    for entry in gold["host"]["prepare_tau_grid"]:
        assert D._prepare_tau_grid(entry["taus"]) == entry["grid"]


def test_integrated_autocorrelation_time(gold, D):
    table = gold["host"]["integrated_time"]
    assert any(any(v <= 0 for v in e["values"][1:]) for e in table)             # a curve that goes non-positive
    assert any(any(math.isnan(v) for v in e["values"]) for e in table)          # and one with a NaN
    for entry in table:
        got = D._integrated_autocorrelation_time(entry["taus"], entry["values"])
        assert _same(got, entry["tau_int"]), entry


def test_recommend_ck_lags(gold, D):
    for entry in gold["host"]["recommend_ck_lags"]:
        lags, window = D._recommend_ck_lags(entry["tau_int"], entry["tau_limit"])
        assert lags == entry["lags"], entry
        assert (list(window) if window is not None else None) == entry["window"], entry


def test_segment_weighting_reproduces_the_reference_curve(gold, D):
    """_combine_segments on the definition's per-segment values (long double numpy) gives the reference's curve."""
    x = R.curve_input(0.0, np.float64)
    stops = np.cumsum(R.CURVE_SEGMENTS)
    starts = stops - np.asarray(R.CURVE_SEGMENTS)
    grid = D._prepare_tau_grid(R.CURVE_LAGS)
    values, _ = R.autocorr_lagscan_ref(x, starts, stops, grid[1:])
    got = D._combine_segments(grid, R.CURVE_SEGMENTS, values)
    want = gold["curves"]["f64_offset0"]
    assert got["taus"] == want["taus"]
    np.testing.assert_allclose(got["values"], want["values"], rtol=0, atol=1e-11)
    assert got["tau_int"] == pytest.approx(want["tau_int"], rel=1e-9)
    assert list(got["lag_window"]) == want["lag_window"]
    assert got["recommended_ck_lags"] == want["recommended_ck_lags"]


def test_segment_weighting_skips_nan_segments(gold, D):
    x = R.nonfinite_input()
    stops = np.cumsum(R.NONFINITE_SEGMENTS)
    starts = stops - np.asarray(R.NONFINITE_SEGMENTS)
    grid = D._prepare_tau_grid(R.NONFINITE_LAGS)
    values, nvalid = R.autocorr_lagscan_ref(x, starts, stops, grid[1:])
    assert nvalid.tolist() == [2, 0, 2] and np.isnan(values[1]).all()
    got = D._combine_segments(grid, R.NONFINITE_SEGMENTS, values)
    want = gold["curves"]["nonfinite"]
    np.testing.assert_allclose(got["values"], want["values"], rtol=0, atol=1e-11, equal_nan=True)
    assert got["recommended_ck_lags"] == want["recommended_ck_lags"]


@pytest.mark.parametrize("name", sorted(R.CCA_CASES))
def test_correlations_from_joint_moments(name, D):
    """The (p + q)-sized algebra, fed with joint moments formed in numpy in the layout of msm_lagged_moments."""
    X, Y = R.cca_input(name)
    n, p, q = len(X), X.shape[1], Y.shape[1]
    J = np.hstack([X, Y])
    Z = J - (J.mean(axis=0) + 1e-9)                # a shift that is not quite the mean: the residual is corrected
    w = p + q
    mom = np.zeros(2 * w * w + 2 * w + 1)
    mom[:w * w] = (2.0 * Z.T @ Z).ravel()
    mom[2 * w * w:2 * w * w + w] = Z.sum(axis=0)
    got = np.asarray(D._correlations_from_moments(mom, n, p, q))
    assert len(got) == min(p, q, n) and np.all(np.diff(got) <= 0) and got.min() >= 0 and got.max() <= 1
    np.testing.assert_allclose(got, R.cca_expected(name), rtol=0, atol=1e-10)


def test_canonical_input_validation(D):
    ok = np.random.default_rng(0).standard_normal((10, 2))
    with pytest.raises(D.InsufficientSamplesError):
        D._canonical_correlations(ok[:1], ok)
    with pytest.raises(D.CanonicalCorrelationError):
        D._canonical_correlations(ok[:, 0], ok)
    bad = ok.copy()
    bad[3, 1] = np.inf
    with pytest.raises(D.CanonicalCorrelationError):
        D._canonical_correlations(ok, bad)
    with pytest.raises(NotImplementedError):
        D._canonical_correlations(np.zeros((10, 200)) + ok[:, :1], np.zeros((10, 57)) + ok[:, :1])
    assert issubclass(D.InsufficientSamplesError, D.CanonicalCorrelationError)
    assert issubclass(D.CanonicalCorrelationError, ValueError)
