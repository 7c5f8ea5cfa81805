"""The fp16 filter scales frames and centres by powers of two and leaves subnormal fp16 parts out of its operands
(pmarlo_amd/csrc/kmeans_filter.h, "Scales" and "Range"): labels and distances must stay those of the pinned fp64
arithmetic bit for bit where the scaling makes things delicate, against the C restatement (oracle/msm_oracle.c) and
against the engine's own all-fp64 kernel (MSM_KMEANS_FILTER=0, in a child process)."""

from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import cport

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _assign(engine, X, centers, mean=None, std=None, image=False, bound=None):
    x = engine.to_device(X)
    c = engine.to_device(np.ascontiguousarray(centers, np.float64))
    m = engine.to_device(np.asarray(mean, np.float64)) if mean is not None else None
    s = engine.to_device(np.asarray(std, np.float64)) if std is not None else None
    md = engine.empty((X.shape[0],), np.float64)
    img = None
    if image:
        am = engine.to_device(np.array([bound], np.float64)) if bound is not None else None
        img = engine.kmeans_pack(x, mean=m, std=s, absmax=am)
    lab = engine.kmeans_assign(x, c, mean=m, std=s, mindist=md, image=img)
    return lab.to_host(), md.to_host()


def _check(engine, X, centers, mean=None, std=None, bound=None):
    want, md_want = cport.kmeans_assign(np.asarray(X, np.float64), np.asarray(centers, np.float64), mean, std,
                                        want_mindist=True)
    for image in (False, True):
        got, md = _assign(engine, X, centers, mean, std, image=image, bound=bound)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(md, md_want)
    return want


def test_coordinates_over_twelve_decades(engine):
    """Coordinates from 1e-8 to 1e4 in one shard: at the shard's scale the low fp16 parts of the small ones are
    subnormal and are left out of the operands."""
    rng = np.random.default_rng(31)
    n, d, k = 20_000, 10, 300
    mag = 10.0 ** rng.uniform(-8, 4, size=(n, d))
    X = rng.choice([-1.0, 1.0], size=(n, d)) * mag
    centers = X[rng.choice(n, size=k, replace=False)] * (1.0 + 1e-3 * rng.normal(size=(k, d)))
    engine.kmeans_filter_scanned(reset=True)
    _check(engine, X, centers)
    assert engine.kmeans_filter_scanned() < 0.2 * 2 * n


def test_frames_of_near_zero_norm(engine):
    rng = np.random.default_rng(32)
    n, d, k = 10_000, 6, 100
    X = rng.normal(size=(n, d))
    X[:2000] *= 1e-9
    X[2000:2100] = 0.0
    X[2100:2200, 0] = 1e-30
    centers = rng.normal(size=(k, d)) * 0.5
    centers[0] = 0.0
    centers[1] = 1e-10
    _check(engine, X, centers)


@pytest.mark.parametrize("ratio", [1e-12, 1e-6, 1e6, 1e12])
def test_centres_far_from_the_frames_scale(engine, ratio):
    """Given centres far larger or smaller than the frames: the two scales differ by up to 2^80."""
    rng = np.random.default_rng(33)
    n, d, k = 8_000, 5, 64
    X = rng.normal(size=(n, d))
    centers = rng.normal(size=(k, d)) * ratio
    _check(engine, X, centers)
    _check(engine, X * 1e-7, centers)


def test_whitening_and_a_loose_bound(engine):
    """The whitened frames' scale, from the library's own pass and from a caller's bound far above the maximum."""
    rng = np.random.default_rng(34)
    n, d, k = 20_000, 10, 250
    X = rng.normal(size=(n, d)) * np.linspace(0.01, 300.0, d) + np.linspace(-50.0, 50.0, d)
    mean, std = X.mean(0), X.std(0) + 0.125
    Z = (X - mean) / std
    centers = Z[rng.choice(n, size=k, replace=False)] + 1e-4 * rng.normal(size=(k, d))
    _check(engine, X, centers, mean, std)
    _check(engine, X, centers, mean, std, bound=float(np.abs(Z).max()) * 1e3)
    _check(engine, Z, centers, bound=float(np.abs(Z).max()))


@pytest.mark.parametrize("d", [4, 10])
def test_k_at_the_lds_limit(engine, d):
    """The largest k whose centre tables fit the LDS (kmeans_filter.h, filter_lds_bytes) and one tile pair more."""
    rf = 8 if d == 4 else 12                       # floats per fp32 table row
    tile = 1024 + 16 * rf * 4 + 16 * 4 + 16 * 8
    cap = 160 * 1024 - 64
    n_tiles = cap // tile // 2 * 2
    rng = np.random.default_rng(35 + d)
    n = 12_000
    X = np.cumsum(rng.normal(size=(n, d)), axis=0) * 0.05 + rng.normal(size=(n, d))
    for k in (16 * n_tiles - 1, 16 * n_tiles + 20):
        centers = X[rng.choice(n, size=k, replace=False)] + 1e-5 * rng.normal(size=(k, d))
        _check(engine, X, centers)


def test_same_labels_as_the_fp64_kernel():
    """The engine's all-fp64 kernel (MSM_KMEANS_FILTER=0) against the filter on the same data, in child processes."""
    script = (
        "import sys, numpy as np; sys.path.insert(0, sys.argv[1])\n"
        "from pmarlo_amd.device import Engine\n"
        "rng = np.random.default_rng(36); n, d, k = 30000, 10, 500\n"
        "X = np.sign(rng.normal(size=(n, d))) * 10.0 ** rng.uniform(-8, 4, size=(n, d))\n"
        "X[:15000] = rng.normal(size=(15000, d)) * 3.0\n"
        "C = X[rng.choice(n, size=k, replace=False)] * 1.001\n"
        "e = Engine(0); x = e.to_device(X); md = e.empty((n,), np.float64)\n"
        "lab = e.kmeans_assign(x, e.to_device(C), mindist=md).to_host()\n"
        "np.save(sys.argv[2], np.concatenate([lab.astype(np.float64), md.to_host()])); e.close()\n")
    out = {}
    for flag in ("0", "1"):
        path = Path(os.environ.get("TMPDIR", "/tmp")) / f"kmf_scales_{os.getpid()}_{flag}.npy"
        env = dict(os.environ, MSM_KMEANS_FILTER=flag)
        r = subprocess.run([sys.executable, "-c", script, str(ROOT), str(path)], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out[flag] = np.load(path)
        path.unlink()
    np.testing.assert_array_equal(out["1"], out["0"])
