"""Regenerate tests/golden/diagnostics.npz / diagnostics.json from the reference implementation.

Run in the build container only (the reference tree does not travel):

    PYTHONPATH=<reference checkout>/src python tests/golden/make_golden_diagnostics.py

The inputs come from the seeded recipes of tests/_diagnostics_ref.py and are NOT stored; the files hold what
pmarlo.analysis.diagnostics returned for them, plus the facts about the inputs that the tests' bounds rest on
(condition numbers, the gap between the reference's iterative CCA and the classical values, the distance of
every compared quantity from its warning threshold).  The script refuses to write a fixture that would make a
test discontinuous.  No reference source text is stored.
"""

from __future__ import annotations

import json
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from pmarlo.analysis import diagnostics as ref  # noqa: E402

from tests import _diagnostics_ref as R  # noqa: E402

warnings.filterwarnings("ignore")


def _clean(obj):
    if isinstance(obj, dict):
        return {str(k): _clean(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_clean(v) for v in obj]
    if isinstance(obj, (np.integer,)):
        return int(obj)
    if isinstance(obj, (np.floating, float)):
        return float(obj)
    return obj


def _call(fn, *args, **kwargs):
    try:
        return {"ok": _clean(fn(*args, **kwargs))}
    except ValueError as exc:
        return {"error": type(exc).__name__, "message": str(exc)}


def _check_curve(curve, what):
    """Every value up to and including the first non-positive one must be well away from zero: the integrated
    time stops there, and a value within rounding of zero would make it discontinuous."""
    smallest = np.inf
    for v in curve["values"][1:]:
        if not np.isfinite(v):
            break
        smallest = min(smallest, abs(v))
        if v <= 0.0:
            break
    assert smallest > 1e-6, f"{what}: |rho| = {smallest} is too close to zero"
    return float(smallest)


def host_tables():
    out = {}
    derive = [
        ([1000], {}), ([100_000], {}), ([50, 2000, 300], {}), ([12], {}), ([4], {}), ([3], {}), ([2], {}), ([1], {}),
        ([1000], {"max_lags": 3}), ([1000], {"max_lags": 1}), ([1000], {"max_lags": 0}), ([1000], {"min_lag": 0}),
        ([1000], {"min_lag": 5}), ([1000], {"min_lag": 400}), ([1000], {"min_lag": 999}), ([1000], {"min_lag": 1000}),
        ([1000], {"fraction_max": 1.0}), ([1000], {"fraction_max": 0.0}), ([1000], {"fraction_max": 1.5}),
        ([1000], {"fraction_max": 0.01}), ([], {}), ([100, 0], {}), ([100, -3], {}),
        ([1000], {"geometric": False}), ([1000], {"geometric": False, "base": []}),
        ([1000], {"geometric": False, "base": [1, 2, 5, 10, 5, 2000, 999]}),
        ([1000], {"geometric": False, "base": [1, 0, 3]}), ([1000], {"geometric": False, "base": [1, 2.5]}),
        ([1000], {"geometric": False, "base": [1000, 2000]}), ([1000], {"geometric": False, "base": [1, 2, 50], "min_lag": 2}),
        ([1000], {"geometric": True, "base": [1, 2]}),
    ]
    out["derive_taus"] = [{"lengths": a, "kwargs": k, **_call(ref.derive_taus, a, **k)} for a, k in derive]
    ds = {"splits": {"a": {"X": np.zeros((300, 2)) + np.arange(300)[:, None], "segments": [
        {"length": 120, "stride": 2}, {"start": 120, "stop": 300, "effective_frame_stride": 3}]},
        "b": np.arange(400.0).reshape(200, 2)}}
    out["derive_taus_dataset"] = _call(ref.derive_taus, ds)
    user = [([1, 2, 5], 10), ([1, 1, 2, 2, 7], 10), ([], 10), ([1, 2.0], 10), ([0, 1], 10), ([3, 2], 10),
            ([10, 20], 10), ([5, 50], 10), ([2, 5, 2, 9], 100)]
    out["validate_user_taus"] = [{"taus": t, "min_length": m, **_call(ref._validate_user_taus, t, m)} for t, m in user]
    nan = float("nan")
    curves = [([0, 1, 2, 4], [1.0, 0.8, 0.5, 0.2]), ([0, 1, 5, 20, 100], [1.0, 0.9, 0.6, -0.1, 0.3]),
              ([0, 1, 5, 20], [1.0, 0.9, nan, 0.4]), ([0, 3], [1.0, 0.0]), ([0], [1.0]), ([], []),
              ([0, 1, 2], [1.0, 0.5]), ([0, 10, 100, 1000], [1.0, 0.99, 0.95, 0.7]), ([0, 1], [1.0, nan])]
    out["integrated_time"] = [{"taus": t, "values": v, "tau_int": ref._integrated_autocorrelation_time(t, v)}
                              for t, v in curves]
    ck = [(1.0, 100), (3.7, 100), (3.7, 5), (40.0, 60), (40.0, 1000), (0.4, 10), (nan, 10), (0.0, 10), (-1.0, 10),
          (1.2, 3), (2.0, 10), (250.0, 13_333)]
    out["recommend_ck_lags"] = []
    for tau_int, limit in ck:
        lags, window = ref._recommend_ck_lags(tau_int, limit)
        out["recommend_ck_lags"].append({"tau_int": tau_int, "tau_limit": limit, "lags": _clean(lags),
                                         "window": _clean(window)})
    out["prepare_tau_grid"] = [{"taus": t, "grid": ref._prepare_tau_grid(t)}
                               for t in ([5, 1, 5, 0, -2, 3], [], [7], [2, 2, 2])]
    return out


def curves():
    out = {}
    segs = [ref._SegmentDescriptor(length=L, stride=1) for L in R.CURVE_SEGMENTS]
    for name, (offset, dtype) in R.CURVE_CASES.items():
        curve = _clean(ref._autocorrelation_curve(R.curve_input(offset, dtype), list(R.CURVE_LAGS), segs))
        curve["smallest_abs_value_before_stop"] = _check_curve(curve, name)
        out[name] = curve
    segs = [ref._SegmentDescriptor(length=L, stride=1) for L in R.NONFINITE_SEGMENTS]
    out["nonfinite"] = _clean(ref._autocorrelation_curve(R.nonfinite_input(), list(R.NONFINITE_LAGS), segs))
    return out


def cca():
    out = {}
    for name, (_, n, p, q, _, _, dup) in R.CCA_CASES.items():
        X, Y = R.cca_input(name)
        entry = {"n": n, "p": p, "q": q}
        if dup:
            entry["cond_cxx_reduced"] = R.cov_condition(X[:, :p - 1])
        else:
            entry["cond_cxx"] = R.cov_condition(X)
            assert entry["cond_cxx"] <= 1e6
            got = np.sort(np.asarray(ref._canonical_correlations(X, Y)))[::-1]
            entry["reference_sorted"] = got.tolist()
            entry["gap_reference_to_classical"] = float(np.max(np.abs(got - R.cca_classical(X, Y))))
        entry["cond_cyy"] = R.cov_condition(Y)
        assert entry["cond_cyy"] <= 1e6
        out[name] = entry
    return out


def end_to_end():
    out = {}
    for name, (_, _, diag_mass, taus) in R.E2E_CASES.items():
        res = _clean(ref.compute_diagnostics(R.e2e_dataset(name), diag_mass=diag_mass, taus=taus))
        gaps = {}
        ds = R.e2e_dataset(name)
        for split, corr in res["canonical_correlation"].items():
            assert abs(min(corr) - 0.95) > 1e-3, (name, split, corr)
            sp = ds["splits"][split]
            Y = ref.apply_whitening_from_metadata(sp["X"], sp["meta"])[0]
            gaps[split] = float(np.max(np.abs(np.sort(corr)[::-1] - R.cca_classical(sp["inputs"], Y))))
        for split, curve in res["autocorrelation"].items():
            _check_curve(curve, f"{name}/{split}")
            v = curve["values"]
            if len(v) >= 4 and np.isfinite(v[1]) and np.isfinite(v[3]):
                assert abs(abs(v[1] - v[3]) - 0.05) > 1e-3, (name, split, v)
        assert abs(diag_mass - 0.95) > 1e-3
        out[name] = {"result": res, "gap_reference_to_classical": gaps}
    ds = R.e2e_dataset("auto_taus_reparam_high_mass")
    ds["splits"]["train"]["segment_lengths"] = [2500, 3000]
    out["segments_do_not_add_up"] = _call(ref.compute_diagnostics, ds)
    return out


def main():
    doc = {"host": host_tables(), "curves": curves(), "cca": cca(), "end_to_end": end_to_end()}
    (HERE / "diagnostics.json").write_text(json.dumps(doc, indent=1) + "\n")
    # the curve values once more as arrays, bit for bit
    arrays = {f"curve_values__{k}": np.asarray(v["values"], np.float64) for k, v in doc["curves"].items()}
    np.savez_compressed(HERE / "diagnostics.npz", **arrays)
    print("wrote", HERE / "diagnostics.json", HERE / "diagnostics.npz")
    for name, entry in doc["cca"].items():
        print(name, {k: v for k, v in entry.items() if k != "reference_sorted"})
    for name, entry in doc["end_to_end"].items():
        if "result" in entry:
            print(name, entry["result"]["warnings"], entry["gap_reference_to_classical"])


if __name__ == "__main__":
    main()
