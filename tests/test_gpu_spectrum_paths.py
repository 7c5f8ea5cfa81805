"""msm_spectrum on every launch path against exact references.

Each case of tests/_spectrum_ref.CASES is solved on the powered iteration (T^4, called without the public retry on
T) and on T itself; Ritz values, pi, implied timescales and the leading left eigenvectors are compared with the
closed-form / symmetric-eigensolve reference of a reversible chain, and the MSM_SPEC_DEBUG lines of every call are
compared with the restated launch-path rule (spectrum_path), so that the table provably reaches the branch it names."""

from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import npport
from tests import _spectrum_ref as sr

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TOL = 1e-9
LAG = 5.0
_REF_CACHE: dict = {}


def _batch_inputs(case: dict, seed0: int = 0):
    """Padded T [B, k, k] (NaN outside each matrix's order: a read past it shows up as NaN), the counts and orders."""
    orders = sr.case_orders(case)
    k, B = case["k"], len(orders)
    T = np.full((B, k, k), np.nan)
    Cs = []
    for b, n in enumerate(orders):
        C = sr.case_counts(case, n, seed=seed0 + 1000 * (b + 1) + n)
        T[b, :n, :n] = sr.rownorm(C)
        Cs.append(C)
    return T, Cs, orders


def _reference(case: dict, C: np.ndarray, key) -> dict:
    if key not in _REF_CACHE:
        _REF_CACHE[key] = sr.reversible_reference(C, case["n_its"], LAG, n_vecs=case["n_vecs"])
    return _REF_CACHE[key]


def _check_matrix(out: dict, b: int, n: int, p_eff: int, ref: dict, case: dict, what: str):
    """One matrix of a solve against its reference."""
    tag = f"{case['name']} [{what}] matrix {b} (n={n})"
    ritz = out["ritz"][b]
    assert abs(ritz[0] - 1.0) <= 1e-12, (tag, ritz[0])
    m = min(case["watch"], p_eff, n)
    np.testing.assert_allclose(ritz[:m].real, ref["ev"][:m], rtol=0, atol=1e-9, err_msg=tag)
    assert np.all(np.abs(ritz[:m].imag) <= 1e-7), tag           # (an exactly repeated value may split at rounding level)
    assert float(out["residual"][b]) <= TOL, (tag, out["residual"][b])
    pi = out["pi"].to_host()[b, :n]
    np.testing.assert_allclose(pi, ref["pi"], rtol=1e-8, atol=0, err_msg=tag)
    if case["n_its"]:
        eig, ts = out["its_eig"][b], out["its_ts"][b]
        np.testing.assert_array_equal(np.isnan(eig), np.isnan(ref["its_eig"]), err_msg=tag)
        np.testing.assert_array_equal(np.isnan(ts), np.isnan(ref["its_ts"]), err_msg=tag)
        np.testing.assert_allclose(eig, ref["its_eig"], rtol=1e-8, equal_nan=True, err_msg=tag)
        np.testing.assert_allclose(ts, ref["its_ts"], rtol=1e-6, equal_nan=True, err_msg=tag)
        if n - 1 < case["n_its"]:
            assert np.all(np.isnan(eig[n - 1:])), tag
    n_vecs = min(case["n_vecs"], case["k"])
    if n_vecs:
        V = out["vecs"].to_host()[b]
        for q in range(n_vecs):
            x = V[q, :n]
            if q >= p_eff:
                assert np.all(np.isnan(x)), (tag, q)
                continue
            # the sign convention on the kernel's own output, exactly
            lead = int(np.argmax(np.abs(x)))
            assert x[lead] > 0, (tag, q, lead, x[lead])
            assert abs(np.dot(x, x) - 1.0) <= 1e-13, (tag, q)
            if ref["gaps"][q] >= 1e-2:
                xr = ref["vecs"][q]
                assert abs(np.dot(xr, x)) >= 1.0 - 1e-10, (tag, q, np.dot(xr, x))
                srt = np.sort(np.abs(xr))
                if n == 1 or srt[-1] - srt[-2] > 1e-6:       # a unique leading component: the same sign as the reference
                    assert np.dot(xr, x) >= 1.0 - 1e-10, (tag, q, np.dot(xr, x))


def _solve(engine, Td, nd, case: dict, powered: bool, B: int):
    kw = dict(n=nd, n_its=case["n_its"], lags=[LAG] * B, p=case["p"], want_pi=True, tol=TOL, seed=0,
              allow_unconverged=False, n_vecs=case["n_vecs"], n_watch=None)
    if powered:
        # the powered iteration exactly as Engine.spectrum runs it, minus its retry on T when it fails
        return engine._spectrum(Td, engine.matrix_power(Td, 2, n=nd), -24 if B == 1 else max(6, 2 * 24 // 3),
                                max_launches=50, **kw)
    return engine.spectrum(Td, squarings=0, **{k: v for k, v in kw.items() if k != "n_watch"})


def _run_case(engine, monkeypatch, capfd, case: dict, modes=(True, False)):
    T, Cs, orders = _batch_inputs(case)
    B = len(orders)
    ragged = case["orders"] is not None
    Td = engine.to_device(T if B > 1 else T[0])
    nd = engine.to_device(np.asarray(orders, np.int32)) if ragged else None
    monkeypatch.setenv("MSM_SPEC_DEBUG", "1")
    outs = {}
    for powered in modes:
        what = "T^4" if powered else "T"
        capfd.readouterr()
        out = _solve(engine, Td, nd, case, powered, B)
        log = capfd.readouterr().err
        calls = sr.check_debug(log, B, case["watch"])
        want = case["path"]
        if any(n > case["p_eff"] for n in orders):
            assert calls[0]["p"] == case["p_eff"], (case["name"], calls[0])
            assert (calls[0]["persist"] is not None) == want["persistent"], (case["name"], calls[0], want)
        for b, n in enumerate(orders):
            ref = _reference(case, Cs[b], (case["name"], b, n))
            _check_matrix(out, b, n, min(out["p"], n), ref, case, what)
        outs[powered] = out
    monkeypatch.delenv("MSM_SPEC_DEBUG")
    return outs


@pytest.mark.parametrize("case", sr.CASES, ids=[c["name"] for c in sr.CASES])
def test_spectrum_case_against_exact_reference(engine, monkeypatch, capfd, case):
    _run_case(engine, monkeypatch, capfd, case)


def test_persistent_alone_and_loop_in_a_batch_agree(engine, monkeypatch, capfd):
    """The same matrices solved one by one (persistent launch) and inside a batch one past 8 * per_xcd (loop)."""
    for name in ("batch_loop_k200_b81", "batch_loop_k544_b9"):
        case = next(c for c in sr.CASES if c["name"] == name)
        assert not case["path"]["persistent"]
        T, Cs, orders = _batch_inputs(case)
        batch = _solve(engine, engine.to_device(T), None, case, True, len(orders))
        single = dict(case, batch=1, path=sr.spectrum_path(case["k"], case["p_eff"], 1, case["watch"]))
        assert single["path"]["persistent"]
        monkeypatch.setenv("MSM_SPEC_DEBUG", "1")
        for b in range(3):
            capfd.readouterr()
            alone = _solve(engine, engine.to_device(T[b]), None, single, True, 1)
            sr.check_debug(capfd.readouterr().err, 1, case["watch"])
            ref = _reference(case, Cs[b], (name, b, orders[b]))
            _check_matrix(alone, 0, orders[b], alone["p"], ref, single, "alone")
            _check_matrix(batch, b, orders[b], batch["p"], ref, case, "batch")
            np.testing.assert_allclose(alone["its_ts"][0], batch["its_ts"][b], rtol=1e-8)
        monkeypatch.delenv("MSM_SPEC_DEBUG")


_CHILD = r"""
import json, sys
import numpy as np
from pmarlo_amd.device import Engine
src, dst = sys.argv[1], sys.argv[2]
d = np.load(src)
meta = json.loads(str(d["meta"]))
eng = Engine(0)
res = {}
for i, m in enumerate(meta):
    Td = eng.to_device(d[f"T{i}"])
    out = eng.spectrum(Td, n_its=m["n_its"], lags=[m["lag"]], p=m["p"], tol=m["tol"], n_vecs=m["n_vecs"], squarings=0)
    res[f"ritz{i}"] = out["ritz"]
    res[f"its_eig{i}"] = out["its_eig"]
    res[f"its_ts{i}"] = out["its_ts"]
    res[f"pi{i}"] = out["pi"].to_host()
    res[f"vecs{i}"] = out["vecs"].to_host()
    res[f"residual{i}"] = out["residual"]
    res[f"p{i}"] = np.asarray([out["p"]])
eng.close()
np.savez(dst, **res)
"""


def test_loop_path_for_single_matrices_in_a_child(engine, tmp_path):
    """Batch-1 shapes that normally take the persistent launch, solved by the launch-per-iteration loop
    (MSM_SPEC_PERSIST=0 is read once per process: one child process for all of them)."""
    names = ["g1_p8", "persist_k200", "persist_k300_p25", "persist_g32_k544"]
    cases = [next(c for c in sr.CASES if c["name"] == nm) for nm in names]
    arrays, meta, refs = {}, [], []
    for i, case in enumerate(cases):
        assert case["path"]["persistent"] and case["batch"] == 1
        T, Cs, orders = _batch_inputs(case)
        arrays[f"T{i}"] = T[0]
        meta.append({"n_its": case["n_its"], "lag": LAG, "p": case["p"], "tol": TOL, "n_vecs": case["n_vecs"]})
        refs.append(_reference(case, Cs[0], (case["name"], 0, orders[0])))
    src, dst = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(src, meta=np.asarray(json.dumps(meta)), **arrays)
    env = dict(os.environ, MSM_SPEC_PERSIST="0", MSM_SPEC_DEBUG="1")
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(src), str(dst)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "persistent launch" not in r.stderr and "first cols" not in r.stderr, r.stderr[-2000:]
    got = np.load(dst)

    class _Host:                     # the device arrays of a solve, already on the host
        def __init__(self, a):
            self.a = a

        def to_host(self):
            return self.a

    for i, case in enumerate(cases):
        out = {"ritz": got[f"ritz{i}"], "its_eig": got[f"its_eig{i}"], "its_ts": got[f"its_ts{i}"],
               "pi": _Host(got[f"pi{i}"]), "vecs": _Host(got[f"vecs{i}"]), "residual": got[f"residual{i}"]}
        _check_matrix(out, 0, case["k"], int(got[f"p{i}"][0]), refs[i], case, "loop, child")


def test_all_zero_lag_in_a_lag_scan_batch(engine, monkeypatch, capfd):
    """A lag longer than every segment: no counts, n_active = 0.  That entry gets NaN timescales and no error; the
    other lags are right, on the persistent launch (4 lags) and on the loop (the scan tiled past 8 * per_xcd)."""
    from tests import _gen

    k, seg = 100, 400
    lab = _gen.metastable_labels(40 * seg, k, 4, seed=11, p_leave=0.05)
    starts = np.arange(0, lab.size, seg, dtype=np.int64)
    stops = starts + seg
    lags = [1, 3, 10, seg + 5]
    counts, _ = engine.count_transitions_lagscan(engine.to_device(lab), k, lags, starts=starts, stops=stops)
    ch = counts.to_host()
    assert not ch[-1].any()
    Ts, ns = [], []
    for i in range(len(lags)):
        out = engine.transition_matrix(engine.to_device(ch[i]), mode=1)
        Ts.append(out["T"].to_host())
        ns.append(int(out["n_active"].to_host()[0]))
    assert ns[-1] == 0 and min(ns[:-1]) > 0
    refs = [npport.its_from_counts(ch[i], lags[i], 3) for i in range(len(lags) - 1)]
    p, watch = sr.engine_p(k, 3)
    reps = sr.loop_batch(k, p) // len(lags) + 1
    monkeypatch.setenv("MSM_SPEC_DEBUG", "1")
    for tile in (1, reps):
        B = len(lags) * tile
        capfd.readouterr()
        spec = engine.spectrum(engine.to_device(np.stack(Ts * tile)), n=engine.to_device(np.asarray(ns * tile, np.int32)),
                               n_its=3, lags=[float(v) for v in lags] * tile)
        calls = sr.check_debug(capfd.readouterr().err, B, watch)
        assert (calls[0]["persist"] is not None) == (tile == 1)
        for t in range(tile):
            for i in range(len(lags)):
                b = t * len(lags) + i
                if ns[i] == 0:
                    assert np.all(np.isnan(spec["its_eig"][b])) and np.all(np.isnan(spec["its_ts"][b]))
                    assert spec["residual"][b] == 0.0
                    continue
                np.testing.assert_allclose(spec["its_eig"][b], refs[i][0], rtol=1e-8)
                np.testing.assert_allclose(spec["its_ts"][b], refs[i][1], rtol=1e-6)
                pi = spec["pi"].to_host()[b, :ns[i]]
                np.testing.assert_allclose(pi @ Ts[i][:ns[i], :ns[i]], pi, atol=1e-12)
    monkeypatch.delenv("MSM_SPEC_DEBUG")


def test_frozen_members_of_a_batch_stay_right(engine):
    """A batch that mixes fast- and slow-converging chains takes several launches; members that met the tolerance in
    the first are frozen (skipped) from then on and must still hold their converged values at the end."""
    k = 200
    fast = dict(name="fast", k=k, n_its=2, n_vecs=2, watch=3, gen="blocks")
    Cf = [sr.block_counts(k, 3, 0.05, seed=s, chain=True) for s in (1, 2)]
    Cs = [sr.block_counts(k, 30, 0.15, seed=s, chain=True) for s in (3, 4)]
    Cb = [Cf[0], Cs[0], Cf[1], Cs[1]]
    T = np.stack([sr.rownorm(C) for C in Cb])
    Td = engine.to_device(T)
    for sq in (2, 0):
        out = engine.spectrum(Td, n_its=2, lags=[LAG] * 4, n_vecs=2, squarings=sq)
        assert out["launches"] > 1, out["launches"]
        for b, C in enumerate(Cb):
            ref = sr.reversible_reference(C, 2, LAG, n_vecs=2)
            _check_matrix(out, b, k, out["p"], ref, fast, f"squarings={sq}")


@pytest.mark.parametrize("k", [300, 700])
def test_nonreversible_chain_eigenvalues_within_their_condition(engine, monkeypatch, capfd, k):
    """A cyclic drift between metastable blocks: a complex slow pair.  Each leading Ritz value must lie within
    cond * residual of an eigenvalue of scipy's dense solve (cond = 1 / |y^H x|)."""
    T = sr.drift_chain(k, seed=k)
    ref = sr.nonreversible_reference(T, 3)
    assert abs(ref["ev"][1].imag) > 1e-3
    p, watch = sr.engine_p(k, 2)
    monkeypatch.setenv("MSM_SPEC_DEBUG", "1")
    for sq in (2, 0):
        capfd.readouterr()
        out = engine.spectrum(engine.to_device(T), n_its=2, lags=[1.0], squarings=sq, tol=1e-10)
        calls = sr.check_debug(capfd.readouterr().err, 1, watch)
        assert (calls[0]["persist"] is not None) == (k == 300)
        got = out["ritz"][0][:3]
        res = float(out["residual"][0])
        assert res <= 1e-10
        for i in range(3):
            tol_i = 100 * ref["cond"][i] * max(res, 1e-13) + 1e-12
            assert np.min(np.abs(got - ref["ev"][i])) <= tol_i, (i, got, ref["ev"][i], tol_i)
        np.testing.assert_allclose(out["pi"].to_host()[0], ref["pi"], rtol=1e-8, atol=1e-14)
    monkeypatch.delenv("MSM_SPEC_DEBUG")


def test_c5_shaped_estimate_against_reversible_reference(engine, monkeypatch, capfd):
    """C5's MSM size (k = 2000): symmetric counts through MSMPipeline.estimate (connected set, +alpha, the default
    powered solve) against the exact reversible reference; the spectrum runs on the loop with W in global memory."""
    from pmarlo_amd.pipeline import MSMPipeline

    k, n_its = 2000, 5
    C = np.rint(200.0 * sr.block_counts(k, 8, 0.3, seed=5, chain=True)).astype(np.int64)
    assert np.array_equal(C, C.T) and (C.sum(1) > 0).all()
    Ca, active = npport.ensure_connected_counts(C)
    assert active.size == k
    eig_ref, ts_ref = npport.reversible_its_from_counts(Ca, LAG, n_its)
    p, watch = sr.engine_p(k, n_its)
    assert not sr.spectrum_path(k, p, 1, watch)["lds_w"]
    monkeypatch.setenv("MSM_SPEC_DEBUG", "1")
    capfd.readouterr()
    est = MSMPipeline(engine).estimate(engine.to_device(C), n_its=n_its, lag=LAG)
    sr.check_debug(capfd.readouterr().err, 1, watch)
    monkeypatch.delenv("MSM_SPEC_DEBUG")
    spec = est["spectrum"]
    assert int(est["n_active"].to_host()[0]) == k
    np.testing.assert_allclose(spec["its_eig"][0], eig_ref, rtol=1e-8)
    np.testing.assert_allclose(spec["its_ts"][0], ts_ref, rtol=1e-6)
    row = Ca.sum(1)
    np.testing.assert_allclose(spec["pi"].to_host()[0], row / row.sum(), rtol=1e-8)
    assert abs(spec["ritz"][0][0] - 1.0) <= 1e-12 and float(spec["residual"][0]) <= TOL
