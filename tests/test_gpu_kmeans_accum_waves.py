"""The d <= 10 accumulate pass of the k-means filter keeps only the fp32 copy of a frame's coordinates after the
candidate pick and reads the fp64 row again for the frames that move their member sums (kmeans_filter.h, kReloadZ).

Small shapes where that can go wrong, three consecutive passes on one state each, no tolerances: labels, int64 member
sums, counts, centres and the fit state (shift2, n_iter, done) after every pass equal
  * the pass restated on the host (labels from oracle/cport.py, exact fixed-point sums, the update and the addition
    order of shift2 written out),
  * the engine's all-fp64 kernel on the same inputs (MSM_KMEANS_FILTER=0 is read once per process: ONE child process
    runs every case of this file),
and the three ways of driving a pass agree: accumulate_delta + update, lloyd_pass (the in-launch close), and the
non-delta accumulate (prev_labels=None, full re-accumulation) + update(clear=True).
Frames with a NaN or |v| > 1e18 have no fixed-point value the host can restate (the conversion of such a product is the
device's): for those cases the host restates labels and counts, and the sums, centres and state are the all-fp64 kernel's."""

from __future__ import annotations

import os
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:          # (the child process runs this file as a script)
    sys.path.insert(0, str(ROOT))

from oracle import cport  # noqa: E402

pytestmark = pytest.mark.gpu

N_PASS = 3
N_UNITS = 64 * 16 * 3 + 37             # three rounds of a 16-wave workgroup's units and a partial unit


# ---------------------------------------------------------------------------------------------------------------
# cases: name -> (X [n, ld], d, centres0 [k, d], mean, std, host_sums)
# ---------------------------------------------------------------------------------------------------------------
def _smooth(n, d, k, seed, ld=None):
    rng = np.random.default_rng(seed)
    X = np.cumsum(rng.normal(size=(n, d)), axis=0) * 0.05 + rng.normal(size=(n, d))
    centres = X[rng.choice(n, size=k, replace=False)] + 1e-4 * rng.normal(size=(k, d))
    if ld is not None:                 # rows ld apart: the columns beyond d must never be read into a result
        X = np.hstack([X, rng.normal(size=(n, ld - d)) * 1e3])
    return np.ascontiguousarray(X), centres


def _cases() -> dict:
    out = {}
    for d in (10, 7):                  # DP = 10 both; d = 7 masks the features beyond d
        for k in (37, 500):            # padding rows in the last tile; 32 tiles / 3 tiles rounded up to 4
            for n in (N_UNITS, 1000):  # the last unit is partial either way
                X, c0 = _smooth(n, d, k, seed=100 * d + k + n)
                out[f"d{d}-k{k}-n{n}"] = (X, d, c0, None, None, True)
    X, c0 = _smooth(N_UNITS, 10, 37, seed=1)
    mean, std = X.mean(0), X.std(0) + 0.25
    out["whitened"] = (X, 10, (c0 - mean) / std, mean, std, True)
    X, c0 = _smooth(1000, 10, 500, seed=2, ld=11)      # 88-byte rows: no 16-byte row loads
    out["ld11"] = (X, 10, c0, None, None, True)

    # nothing moves in the second pass: five tight clouds far apart, centres started inside them
    rng = np.random.default_rng(3)
    spots = 100.0 * rng.normal(size=(5, 10))
    X = np.repeat(spots, 60, axis=0) + 0.01 * rng.normal(size=(300, 10))
    out["converged"] = (X, 10, X[::60].copy(), None, None, True)

    # step 4: duplicated centres (two rows of different lanes, two rows of one lane, three rows of one lane of the
    # fp32 scan) and frames on centres and on midpoints of centre pairs
    rng = np.random.default_rng(4)
    k, d = 500, 10
    c0 = rng.normal(size=(k, d))
    c0[300] = c0[7]
    c0[67] = c0[3]
    c0[69] = c0[133] = c0[5]
    a, b = rng.integers(0, k, size=(2, 1200))
    X = np.vstack([0.5 * (c0[a] + c0[b]), c0, c0 + 1e-9 * rng.normal(size=(k, d)), rng.normal(size=(N_UNITS - 2200, d))])
    out["ties"] = (X, d, c0, None, None, True)

    Xs = X.copy()
    Xs[5, 3] = np.nan
    Xs[70] = np.nan
    Xs[131, 0] = 3e18
    Xs[1500, 9] = -1e19
    out["nan-huge-frames"] = (Xs, d, c0, None, None, False)

    cb = rng.normal(size=(k, d))
    cb[11, 2] = 1e19                   # outside the range guard: every frame takes the plain scan
    out["centre-out-of-range"] = (X[:1000].copy(), d, cb, None, None, True)
    return out


CASES = _cases()
STEP4 = ("ties", "nan-huge-frames", "centre-out-of-range")


# ---------------------------------------------------------------------------------------------------------------
# the engine, through the C ABI (the row stride ld is not part of the Engine's methods)
# ---------------------------------------------------------------------------------------------------------------
def _run_case(engine, case) -> dict:
    """Three passes, three ways -> {"<way>/<pass>/<what>": array}; ways: delta, fused, full."""
    from pmarlo_amd._lib import MSM_F64, check, lib

    X, d, c0, mean, std, _ = case
    n, ld = X.shape
    k = c0.shape[0]
    h = engine.handle
    xd = engine.to_device(X)
    md = engine.to_device(mean) if mean is not None else None
    sd = engine.to_device(std) if std is not None else None
    mp, sp = (md.ptr, sd.ptr) if mean is not None else (None, None)
    out = {}
    for way in ("delta", "fused", "full"):
        cen = engine.to_device(c0)
        st = engine.zeros((8,), np.float64)
        check(lib.msm_kmeans_fit_begin(h, xd.ptr, MSM_F64, n, d, ld, mp, sp, k, 0, 0, float(n), 0.0, cen.ptr, st.ptr, 0), h)
        sums, counts = engine.zeros((k * d,), np.int64), engine.zeros((k,), np.int64)
        prev = engine.empty((n,), np.int32).fill_bytes_(0xFF)
        for it in range(N_PASS):
            if way == "delta":
                check(lib.msm_kmeans_accumulate_delta(h, xd.ptr, MSM_F64, n, d, ld, cen.ptr, k, mp, sp, None, st.ptr, prev.ptr,
                                                      sums.ptr, counts.ptr), h)
            elif way == "fused":
                check(lib.msm_kmeans_lloyd_pass(h, xd.ptr, MSM_F64, n, d, ld, cen.ptr, k, mp, sp, None, st.ptr, prev.ptr,
                                                sums.ptr, counts.ptr), h)
            else:
                check(lib.msm_kmeans_accumulate_packed(h, xd.ptr, MSM_F64, n, d, ld, cen.ptr, k, mp, sp, None, st.ptr, sums.ptr,
                                                       counts.ptr), h)
            out[f"{way}/{it}/sums"] = sums.to_host().reshape(k, d)
            out[f"{way}/{it}/counts"] = counts.to_host()
            if way != "full":
                out[f"{way}/{it}/labels"] = prev.to_host()
            if way != "fused":
                check(lib.msm_kmeans_update(h, sums.ptr, counts.ptr, k, d, cen.ptr, st.ptr, int(way == "full")), h)
            out[f"{way}/{it}/centres"] = cen.to_host()
            out[f"{way}/{it}/state"] = st.to_host()
    return out


def _child_main(path: str) -> None:
    from pmarlo_amd.device import Engine

    eng = Engine(0)
    flat = {}
    for name, case in CASES.items():
        for key, v in _run_case(eng, case).items():
            flat[f"{name}|{key}"] = v
    eng.close()
    np.savez(path, **flat)


@pytest.fixture(scope="module")
def fp64_results(tmp_path_factory):
    """Every case on the all-fp64 kernel: one child process for the module."""
    path = tmp_path_factory.mktemp("kmeans_accum_waves") / "fp64.npz"
    env = dict(os.environ, MSM_KMEANS_FILTER="0")
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(path)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(path) as z:
        return {key: z[key] for key in z.files}


_results: dict = {}


@pytest.fixture
def filter_results(engine):
    """name -> (results of the filter kernel, frames that took step 4), computed once per case."""
    def get(name):
        if name not in _results:
            engine.kmeans_filter_scanned(reset=True)
            res = _run_case(engine, CASES[name])
            _results[name] = (res, engine.kmeans_filter_scanned())
        return _results[name]

    return get


# ---------------------------------------------------------------------------------------------------------------
# the pass restated on the host
# ---------------------------------------------------------------------------------------------------------------
def _fma(a: float, b: float, c: float) -> float:
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # one rounding, to nearest even


def _shift2(old: np.ndarray, new: np.ndarray, counts: np.ndarray) -> float:
    """kmeans_update_kernel's order: virtual thread v of 1024 takes the elements v, v + 1024, ... (an fma chain), 64
    consecutive threads add up by shuffles (lane l += lane l + off, off = 32 .. 1), the sixteen sums in order."""
    k, d = old.shape
    o, w = old.ravel(), new.ravel()
    acc = np.zeros(1024)
    for i in range(k * d):
        if counts[i // d] > 0:
            dl = w[i] - o[i]
            acc[i % 1024] = _fma(dl, dl, acc[i % 1024])
    t = 0.0
    for wv in range(16):
        a = acc[64 * wv:64 * wv + 64].copy()
        for off in (32, 16, 8, 4, 2, 1):
            a[:off] = a[:off] + a[off:2 * off]
        t += a[0]
    return t


def _host_passes(case, scale: float, inv_scale: float):
    X, d, c0, mean, std, _ = case
    k = c0.shape[0]
    Xd = np.ascontiguousarray(X[:, :d])
    Z = (Xd - mean) / std if mean is not None else Xd
    cen, done, n_iter, shift2 = c0.copy(), 0.0, 0.0, 0.0
    lab = np.full(X.shape[0], -1, np.int32)
    sums, counts = np.zeros((k, d), np.int64), np.zeros(k, np.int64)
    out = []
    for _ in range(N_PASS):
        if done == 0.0:
            lab = cport.kmeans_assign(Xd, cen, mean, std)
            counts = np.bincount(lab, minlength=k).astype(np.int64)
            sums = np.zeros((k, d), np.int64)
            np.add.at(sums, lab, np.rint(Z * scale).astype(np.int64))
            new = cen.copy()
            nz = counts > 0
            new[nz] = sums[nz].astype(np.float64) * inv_scale / counts[nz, None].astype(np.float64)
            shift2 = _shift2(cen, new, counts)
            cen = new
            n_iter += 1.0
            done = float(shift2 <= 0.0)         # tol2 = 0: a pass that moves no centre ends the fit
        out.append(dict(labels=lab, counts=counts, sums=sums, centres=cen, shift2=shift2, n_iter=n_iter, done=done))
    return out


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_three_passes_three_ways(filter_results, fp64_results, name):
    case = CASES[name]
    res, scanned = filter_results(name)
    st0 = res["delta/0/state"]
    host = _host_passes(case, float(st0[0]), float(st0[1])) if case[5] else None
    moved = []
    for it in range(N_PASS):
        t = f"{name}, pass {it}"
        for way in ("delta", "fused", "full"):
            for what in ("sums", "counts", "labels", "centres", "state"):
                key = f"{way}/{it}/{what}"
                if key not in res:
                    continue
                got = res[key]
                if way == "full" and what in ("sums", "counts") and it and res[f"full/{it - 1}/state"][5] == 1.0:
                    assert not got.any(), f"{t}: {key}"     # the fit is done: a no-op after update(clear=True)
                    continue
                # the three ways agree (the full re-accumulation has no label buffer)
                np.testing.assert_array_equal(got, res[f"delta/{it}/{what}"], err_msg=f"{t}: {key} against delta")
                # the all-fp64 kernel
                np.testing.assert_array_equal(got, fp64_results[f"{name}|{key}"], err_msg=f"{t}: {key} against the fp64 kernel")
        lab = res[f"delta/{it}/labels"]
        before = res[f"delta/{it - 1}/labels"] if it else np.full(lab.shape, -1, np.int32)
        moved.append(int((lab != before).sum()))
        if host is not None:
            want = host[it]
            np.testing.assert_array_equal(lab, want["labels"], err_msg=t)
            np.testing.assert_array_equal(res[f"delta/{it}/counts"], want["counts"], err_msg=t)
            np.testing.assert_array_equal(res[f"delta/{it}/sums"], want["sums"], err_msg=t)
            np.testing.assert_array_equal(res[f"delta/{it}/centres"], want["centres"], err_msg=t)
            st = res[f"delta/{it}/state"]
            assert (st[3], st[5], st[6]) == (want["shift2"], want["done"], want["n_iter"]), t
        else:
            # labels and counts given the centres the pass started from
            X, d, c0 = case[0], case[1], case[2]
            start = res[f"delta/{it - 1}/centres"] if it else c0
            want = cport.kmeans_assign(np.ascontiguousarray(X[:, :d]), start)
            np.testing.assert_array_equal(lab, want, err_msg=t)
            np.testing.assert_array_equal(res[f"delta/{it}/counts"], np.bincount(want, minlength=c0.shape[0]), err_msg=t)
    print(name, "frames that moved per pass", moved, "frames through step 4", scanned)
    assert moved[0] == case[0].shape[0]                       # labels start at -1: the reload runs on every lane
    if name == "converged":
        assert moved[1] == 0 and res["delta/1/state"][5] == 1.0
        np.testing.assert_array_equal(res["delta/1/sums"], res["delta/0/sums"])
        np.testing.assert_array_equal(res["delta/1/counts"], res["delta/0/counts"])
    elif name.startswith("d"):
        assert 0 < moved[1] < moved[0]                        # the second pass moves some frames, not all
    if name in STEP4:
        assert scanned > 0                                    # step 4 ran
    if name == "centre-out-of-range":
        assert scanned >= 3 * N_PASS * case[0].shape[0]       # ... for every frame of every launch


if __name__ == "__main__":
    _child_main(sys.argv[1])
