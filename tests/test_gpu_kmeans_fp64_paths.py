"""The all-fp64 k-means kernel (kmeans_mfma_kernel) on every specialisation against the C oracle, bit for bit.

Each row of tests/_kmeans_ref's tables is launched with MSM_KMEANS_DEBUG set and the printed line is compared with the
restated dispatch rule, so a row provably ran the instantiation <T, KS, ACCUM, FOLD, MULTI> (and lds_acc, tile_k, grid)
it names.  Inputs: the usual smooth series (with and without whitening), exact ties placed where the recoveries order
candidates differently, near ties, non-finite values, heavy cancellation, whitening over twelve decades.  There are no
tolerances here: labels, distances, member sums and centres equal oracle/cport.py's."""

from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import cport
from tests import _kmeans_ref as kr

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _ids(rows):
    return [r["name"] for r in rows]


def _dev(engine, a, dtype=None):
    return engine.to_device(np.ascontiguousarray(a, dtype)) if a is not None else None


def _assign(engine, X, centers, mean=None, std=None):
    md = engine.empty((X.shape[0],), np.float64)
    lab = engine.kmeans_assign(_dev(engine, X), _dev(engine, centers, np.float64), mean=_dev(engine, mean, np.float64),
                               std=_dev(engine, std, np.float64), mindist=md)
    return lab.to_host(), md.to_host()


def _check_assign(engine, X, centers, mean=None, std=None, tag=""):
    want, md_want = cport.kmeans_assign(X.astype(np.float64), centers, mean, std, want_mindist=True)
    got, md = _assign(engine, X, centers, mean, std)
    np.testing.assert_array_equal(got, want, err_msg=f"{tag}: labels")
    np.testing.assert_array_equal(md, md_want, err_msg=f"{tag}: mindist")


def _row_inputs(row: dict, n: int, tile_k: int, seed: int):
    """(tag, X, centres, mean, std) of every generator the row asks for."""
    d, k, dt = row["d"], row["k"], kr.DTYPES[row["dtype"]]
    out = []
    for g in row["gens"]:
        if g in ("smooth", "white"):
            X, Cn, mean, std = kr.smooth(n, d, k, dt, seed)
            out.append((g, X, Cn, mean, std) if g == "white" else (g, X, Cn, None, None))
        elif g == "ties":
            X, Cn, _ = kr.ties(n, d, k, tile_k, dt, seed)
            out.append((g, X, Cn, None, None))
        elif g == "near" and k >= 2:
            X, Cn, _ = kr.near(n, d, k, tile_k, dt, seed)
            out.append((g, X, Cn, None, None))
        elif g == "nonfinite":
            for q, (X, Cn) in enumerate(kr.nonfinite(n, d, k, dt, seed)):
                out.append((f"nonfinite{q}", X, Cn, None, None))
    return out


@pytest.fixture
def debug(monkeypatch, capfd):
    """Lines the library printed under MSM_KMEANS_DEBUG since the last call."""
    monkeypatch.setenv("MSM_KMEANS_DEBUG", "1")
    capfd.readouterr()

    def lines():
        return kr.debug_lines(capfd.readouterr().err)

    return lines


@pytest.mark.parametrize("row", kr.ASSIGN_ROWS, ids=_ids(kr.ASSIGN_ROWS))
def test_assign_row(engine, debug, row):
    n_cu = engine.info()["n_cu"]
    path = kr.row_path(row, n_cu)
    n = kr.row_n(row, n_cu)
    assert path["kernel"] == "fp64"
    for tag, X, Cn, mean, std in _row_inputs(row, n, path["tile_k"], seed=len(row["name"]) + row["d"]):
        debug()
        _check_assign(engine, X, Cn, mean, std, tag=f"{row['name']} [{tag}]")
        assert debug() == [kr.debug_line(path)], (row["name"], tag)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("what", list(kr.ADVERSARIAL_SHAPES))
def test_adversarial_assign(engine, debug, what, dtype):
    """Non-finite and out-of-range frames and centres, and whitening with std over 1e-6 .. 1e6, on an LDS-recovery, a
    global-recovery and a chunked shape."""
    n, d, k = kr.ADVERSARIAL_SHAPES[what]
    dt = kr.DTYPES[dtype]
    line = kr.debug_line(kr.dispatch(dtype, n, d, k, False, n_cu=engine.info()["n_cu"]))
    for q, (X, Cn) in enumerate(kr.nonfinite(n, d, k, dt, seed=d)):
        _check_assign(engine, X, Cn, tag=f"{what} nonfinite set {q}")
    X, Cn, mean, std = kr.whitening(n, d, k, dt, seed=d + 1)
    _check_assign(engine, X, Cn, mean, std, tag=f"{what} whitening")
    assert set(debug()) == {line}


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", kr.CANCELLATION_SHAPES, ids=lambda s: f"d{s[1]}")
def test_heavy_cancellation(engine, shape, dtype):
    n, d, k = shape
    X, Cn = kr.cancellation(n, d, k, kr.DTYPES[dtype], seed=d)
    _check_assign(engine, X, Cn, tag=f"cancellation d={d}")
    _check_assign(engine, X, Cn, X.mean(0, dtype=np.float64), X.std(0, dtype=np.float64), tag=f"cancellation d={d}, whitened")


def test_d257_is_refused_cleanly(engine):
    rng = np.random.default_rng(0)
    X, Cn = rng.normal(size=(40, 257)), rng.normal(size=(5, 257))
    with pytest.raises(NotImplementedError, match="256"):
        _assign(engine, X, Cn)
    with pytest.raises(ValueError):                                     # the fit checks its shape up front
        engine.kmeans_fit(_dev(engine, X), 5, max_iter=1)
    _check_assign(engine, X[:, :256], Cn[:, :256], tag="d = 256 after the refusal")


# ---------------------------------------------------------------------------------------------------------------
# accumulate
# ---------------------------------------------------------------------------------------------------------------
def _pass_by_pass(engine, debug, X, centers0, path_acc, path_asg, n_pass, tag):
    """Full sums and delta sums (prev_labels) against the restated pass, the label buffer against kmeans_assign, the
    updated centres against the restated update -- after every pass."""
    n, d = X.shape
    k = centers0.shape[0]
    X64 = X.astype(np.float64)
    xd = _dev(engine, X)
    c_f, st_f = engine.kmeans_fit_begin(xd, k, seed=0, n_total=n, tol2=0.0, centers=_dev(engine, centers0), init_centers=False)
    c_d, st_d = engine.kmeans_fit_begin(xd, k, seed=0, n_total=n, tol2=0.0, centers=_dev(engine, centers0), init_centers=False)
    scale = float(st_f.to_host()[0])
    sums_f, counts_f = engine.zeros((k * d,), np.int64), engine.zeros((k,), np.int64)
    sums_d, counts_d = engine.zeros((k * d,), np.int64), engine.zeros((k,), np.int64)
    prev = engine.empty((n,), np.int32).fill_bytes_(0xFF)
    ref = centers0.copy()
    debug()
    ran = 0
    for it in range(n_pass):
        old = ref
        lab, sums, counts, ref = kr.member_sums(X64, ref, scale)
        ran += 1
        engine.kmeans_accumulate(xd, c_f, st_f, sums_f, counts_f)
        engine.kmeans_accumulate(xd, c_d, st_d, sums_d, counts_d, prev_labels=prev)
        got = engine.kmeans_assign(xd, c_d).to_host()
        t = f"{tag}, pass {it}"
        np.testing.assert_array_equal(got, lab, err_msg=t)
        np.testing.assert_array_equal(prev.to_host(), lab, err_msg=t)
        np.testing.assert_array_equal(counts_f.to_host(), counts, err_msg=t)
        np.testing.assert_array_equal(counts_d.to_host(), counts, err_msg=t)
        np.testing.assert_array_equal(sums_f.to_host().reshape(k, d), sums, err_msg=t)
        np.testing.assert_array_equal(sums_d.to_host().reshape(k, d), sums, err_msg=t)
        engine.kmeans_update(sums_f, counts_f, c_f, st_f, clear=True)
        engine.kmeans_update(sums_d, counts_d, c_d, st_d, clear=False)
        np.testing.assert_array_equal(c_f.to_host(), ref, err_msg=t)
        np.testing.assert_array_equal(c_d.to_host(), ref, err_msg=t)
        # no centre moved (k = 1 after its first pass): shift2 = 0 <= tol2 sets `done`, and later launches are no-ops
        stopped = np.array_equal(ref, old)
        assert st_f.to_host()[5] == st_d.to_host()[5] == float(stopped), t
        if stopped:
            break
    assert debug() == [kr.debug_line(path_acc), kr.debug_line(path_acc), kr.debug_line(path_asg)] * ran, tag
    return lab, counts, ref


def _fit_rows(engine, debug, row, filter_on=True):
    n_cu = engine.info()["n_cu"]
    n, d, k = kr.row_n(row, n_cu), row["d"], row["k"]
    for dtype in (row["dtype"], "f64" if row["dtype"] == "f32" else "f32"):
        path = kr.dispatch(dtype, n, d, k, True, filter_on, n_cu)
        assert path["kernel"] == "fp64"
        X, _, _, _ = kr.smooth(n, d, k, kr.DTYPES[dtype], seed=d + k)
        want, _, scale = cport.kmeans_fit(X.astype(np.float64), k, seed=7, max_iter=3, tol2=0.0)
        debug()
        got, st = engine.kmeans_fit(_dev(engine, X), k, seed=7, max_iter=3, tol2=0.0)
        assert debug() == [kr.debug_line(path)] * 3, row["name"]
        assert float(st.to_host()[0]) == scale
        np.testing.assert_array_equal(got.to_host(), want, err_msg=f"{row['name']} {dtype}: fit")


@pytest.mark.parametrize("row", kr.ACCUM_ROWS, ids=_ids(kr.ACCUM_ROWS))
def test_accumulate_row(engine, debug, row):
    """The Lloyd fit against cport.kmeans_fit in both dtypes, then pass by pass in the row's dtype: smooth data, and
    duplicated centres with frames tied between them plus centres nothing is near (empty clusters)."""
    _fit_rows(engine, debug, row)
    n_cu = engine.info()["n_cu"]
    n, d, k, dt = kr.row_n(row, n_cu), row["d"], row["k"], kr.DTYPES[row["dtype"]]
    path_acc, path_asg = kr.row_path(row, n_cu), kr.row_path(row, n_cu, accumulate=False)
    X, Cn, _, _ = kr.smooth(n, d, k, dt, seed=k)
    _pass_by_pass(engine, debug, X, Cn, path_acc, path_asg, 3, f"{row['name']} [smooth]")
    X, Cn, pl = kr.ties(n, d, k, path_acc["tile_k"], dt, seed=k + 1)
    empty = [j for j in (k // 2, k - 3) if k >= 8 and all(j not in p[1:] for p in pl)]
    Cn[empty] += 1e3                                                    # nothing is near: these clusters stay empty
    lab, counts, ref = _pass_by_pass(engine, debug, X, Cn, path_acc, path_asg, 2, f"{row['name']} [ties]")
    for j in empty:
        assert counts[j] == 0 and np.array_equal(ref[j], Cn[j])


def test_done_state_changes_nothing(engine, debug):
    """done = 1 in the fit state: accumulate (full and delta) and update leave sums, counts, labels and centres alone."""
    for n, d, k in ((900, 29, 60), (900, 100, 150)):                    # LDS and global member sums, one and two chunks
        X, Cn, _, _ = kr.smooth(n, d, k, np.float64, seed=3)
        xd = _dev(engine, X)
        c, st = engine.kmeans_fit_begin(xd, k, seed=0, n_total=n, tol2=0.0, centers=_dev(engine, Cn), init_centers=False)
        state = st.to_host()
        state[5] = 1.0
        st = _dev(engine, state)
        sums = _dev(engine, np.full(k * d, 12345, np.int64))
        counts = _dev(engine, np.full(k, 77, np.int64))
        prev = _dev(engine, np.full(n, 5, np.int32))
        engine.kmeans_accumulate(xd, c, st, sums, counts)
        engine.kmeans_accumulate(xd, c, st, sums, counts, prev_labels=prev)
        engine.kmeans_update(sums, counts, c, st, clear=True)
        assert len(debug()) == 2
        assert (sums.to_host() == 12345).all() and (counts.to_host() == 77).all() and (prev.to_host() == 5).all()
        np.testing.assert_array_equal(c.to_host(), Cn)
        np.testing.assert_array_equal(st.to_host(), state)


# ---------------------------------------------------------------------------------------------------------------
# the row stride of the C ABI
# ---------------------------------------------------------------------------------------------------------------
def _assign_strided(engine, X, ld, centers, mean=None, std=None):
    """msm_kmeans_assign on rows `ld` apart, NaN in the padding columns."""
    from pmarlo_amd import _lib

    n, d = X.shape
    buf = np.full((n, ld), np.nan, X.dtype)
    buf[:, :d] = X
    xd, cd = _dev(engine, buf), _dev(engine, centers, np.float64)
    md, sd = _dev(engine, mean, np.float64), _dev(engine, std, np.float64)
    lab, dist = engine.empty((n,), np.int32), engine.empty((n,), np.float64)
    _lib.check(_lib.lib.msm_kmeans_assign(engine.handle, xd.ptr, _lib.MSM_F32 if X.dtype == np.float32 else _lib.MSM_F64,
                                          n, d, ld, cd.ptr, centers.shape[0], md.ptr if md else None,
                                          sd.ptr if sd else None, lab.ptr, dist.ptr), engine.handle)
    return lab.to_host(), dist.to_host()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n,d,k", [(1500, 29, 200), (1500, 13, 70), (900, 100, 120), (1100, 45, 500)],
                         ids=["prefetch_ks8", "narrow_ks4", "no_prefetch_ks32", "chunked_ks12"])
def test_row_stride(engine, debug, n, d, k, dtype):
    X, Cn, mean, std = kr.smooth(n, d, k, kr.DTYPES[dtype], seed=n + d)
    want, md_want = cport.kmeans_assign(X.astype(np.float64), Cn, want_mindist=True)
    want_w, md_want_w = cport.kmeans_assign(X.astype(np.float64), Cn, mean, std, want_mindist=True)
    line = kr.debug_line(kr.dispatch(dtype, n, d, k, False, n_cu=engine.info()["n_cu"]))
    for ld in (d + 1, d + 3, d + 1000):
        got, md = _assign_strided(engine, X, ld, Cn)
        np.testing.assert_array_equal(got, want, err_msg=f"ld={ld}")
        np.testing.assert_array_equal(md, md_want, err_msg=f"ld={ld}")
        got, md = _assign_strided(engine, X, ld, Cn, mean, std)
        np.testing.assert_array_equal(got, want_w, err_msg=f"ld={ld}, whitened")
        np.testing.assert_array_equal(md, md_want_w, err_msg=f"ld={ld}, whitened")
    assert debug() == [line] * 6


# ---------------------------------------------------------------------------------------------------------------
# MSM_KMEANS_FILTER=0: d <= 10 on the fp64 kernel (read once per process: one child for all rows)
# ---------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, sys
import numpy as np
from pmarlo_amd.device import Engine
src, dst = sys.argv[1], sys.argv[2]
d = np.load(src)
jobs = json.loads(str(d["jobs"]))
eng = Engine(0)
res = {}
for i, job in enumerate(jobs):
    print("job", i, job["kind"], file=sys.stderr, flush=True)
    x = eng.to_device(d[f"X{i}"])
    if job["kind"] == "assign":
        c = eng.to_device(d[f"C{i}"])
        m = eng.to_device(d[f"M{i}"]) if job["white"] else None
        s = eng.to_device(d[f"S{i}"]) if job["white"] else None
        md = eng.empty((x.shape[0],), np.float64)
        res[f"lab{i}"] = eng.kmeans_assign(x, c, mean=m, std=s, mindist=md).to_host()
        res[f"md{i}"] = md.to_host()
    else:
        c, st = eng.kmeans_fit(x, job["k"], seed=7, max_iter=3, tol2=0.0)
        res[f"cen{i}"] = c.to_host()
        res[f"st{i}"] = st.to_host()
eng.close()
np.savez(dst, **res)
"""


def test_filter_off_child(engine, tmp_path):
    n_cu = engine.info()["n_cu"]
    arrays, jobs, wants = {}, [], []
    for row in kr.CHILD_ROWS:
        n, d, k = kr.row_n(row, n_cu), row["d"], row["k"]
        path = kr.row_path(row, n_cu)
        assert path["kernel"] == "fp64" and path["KS"] <= 3
        if row["accum"]:
            for dtype in ("f32", "f64"):
                X, _, _, _ = kr.smooth(n, d, k, kr.DTYPES[dtype], seed=d + k)
                i = len(jobs)
                arrays[f"X{i}"] = X
                jobs.append({"kind": "fit", "k": k, "name": row["name"]})
                wants.append((cport.kmeans_fit(X.astype(np.float64), k, seed=7, max_iter=3, tol2=0.0),
                              [kr.debug_line(kr.dispatch(dtype, n, d, k, True, False, n_cu))] * 3))
            continue
        for tag, X, Cn, mean, std in _row_inputs(row, n, path["tile_k"], seed=d + k):
            i = len(jobs)
            arrays[f"X{i}"], arrays[f"C{i}"] = X, Cn
            if mean is not None:
                arrays[f"M{i}"], arrays[f"S{i}"] = mean, std
            jobs.append({"kind": "assign", "white": mean is not None, "name": f"{row['name']} [{tag}]"})
            wants.append((cport.kmeans_assign(X.astype(np.float64), Cn, mean, std, want_mindist=True), [kr.debug_line(path)]))
    src, dst = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(src, jobs=np.asarray(json.dumps(jobs)), **arrays)
    env = dict(os.environ, MSM_KMEANS_FILTER="0", MSM_KMEANS_DEBUG="1")
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(src), str(dst)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "msm_kmeans: filter" not in r.stderr
    # the debug lines, job by job
    log: list[list[str]] = []
    for ln in r.stderr.splitlines():
        if ln.startswith("job "):
            log.append([])
        elif ln.startswith("msm_kmeans: "):
            log[-1].append(ln.strip())
    assert len(log) == len(jobs)
    got = np.load(dst)
    for i, (job, (want, lines)) in enumerate(zip(jobs, wants)):
        assert log[i] == lines, job["name"]
        if job["kind"] == "assign":
            np.testing.assert_array_equal(got[f"lab{i}"], want[0], err_msg=job["name"])
            np.testing.assert_array_equal(got[f"md{i}"], want[1], err_msg=job["name"])
        else:
            np.testing.assert_array_equal(got[f"cen{i}"], want[0], err_msg=job["name"])
            assert got[f"st{i}"][0] == want[2]
