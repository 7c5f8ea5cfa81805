"""The folds of the single-shard step: the clears and one-workgroup launches that ride in a neighbouring launch.

Every comparison is bit for bit against the separate entry points (which stay as they were); where a CPU oracle exists
(tests/_moments_ref, oracle/cport.count_transitions, oracle/npport.normalise_counts) the result is held against it too.

  moments tail   msm_moments_tail            = msm_moments_from_lagged + msm_standardise_params (+ the clear of one word)
  projection     msm_project_preset          = msm_project / msm_project_finite without the clear of max |Y|
  first pass     msm_kmeans_fit_begin_clear, = fit_begin + zeroed member sums + labels filled with -1
                 msm_kmeans_lloyd_pass_from / msm_kmeans_accumulate_delta_from (first_pass)
  counts and T   msm_count_transitions_normalised = msm_count_transitions + msm_transition_matrix (mode 0)
  whole step     ShardedMSM.step with the folds = the step under MSM_STEP_FOLDS=0, eagerly and from a captured graph
"""
import numpy as np
import pytest

from oracle import cport, npport
from pmarlo_amd.dist import ShardConfig, ShardedMSM
from tests import _gen
from tests import _moments_ref as mr

pytestmark = pytest.mark.gpu

GARBAGE64 = 0x5A5A5A5A5A5A5A5A


def _same(a, b, what):
    """Bit equality of two device (or host) arrays of one dtype."""
    a = a.to_host() if hasattr(a, "to_host") else np.asarray(a)
    b = b.to_host() if hasattr(b, "to_host") else np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), f"{what}: bits differ"


# ---------------------------------------------------------------------------------------------------------------------
# 1. moments tail
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("lag", [1, 10])
@pytest.mark.parametrize("F", [3, 16, 64])
@pytest.mark.parametrize("n", [257, 4099])
def test_moments_tail(engine, n, F, lag, dtype):
    # integers about an integer shift: every raw moment is an exact fp64 number, so the column sums have an oracle
    rng = np.random.default_rng(1000 * n + 10 * F + lag)
    X = 13.0 + rng.integers(-3, 4, size=(n, F)).astype(np.float64)
    X[:, F // 2] = 13.0 + (np.arange(n) % 5) - 1.0
    shift = 13.0 + rng.integers(-2, 3, size=F).astype(np.float64)
    x, sh = engine.to_device(X.astype(dtype)), engine.to_device(shift)
    lagged = engine.lagged_moments(x, lag, sh, assume_finite=True, symmetric=True)
    # the separate launches
    sums0 = engine.moments_from_lagged(x, lag, sh, lagged)
    mean0, scale0, inv0 = engine.standardise_params(sums0, sh, F, float(n), True)
    # one launch, onto buffers full of something else; the max |Y| word starts non-zero
    slot = engine.to_device(np.array([GARBAGE64], np.uint64)).view((1,), np.float64)
    fill = lambda m: engine.to_device(np.full(m, -7.25))    # noqa: E731
    sums1, (mean1, scale1, inv1) = engine.moments_tail(x, lag, sh, lagged, float(n), True, sums=fill(3 * F),
                                                       out=(fill(F), fill(F), fill(F)), zero_slot=slot)
    _same(sums1, sums0, "column sums")
    _same(mean1, mean0, "mean")
    _same(scale1, scale0, "scale")
    _same(inv1, inv0, "1 / scale")
    assert slot.view((1,), np.uint64).to_host()[0] == 0, "the max |Y| slot was not cleared"
    # without a word to clear, and without the scale
    _, (mean2, scale2, inv2) = engine.moments_tail(x, lag, sh, lagged, float(n), False)
    m0, s0, i0 = engine.standardise_params(sums0, sh, F, float(n), False)
    _same(mean2, m0, "mean (no scale)")
    _same(scale2, s0, "scale (no scale)")
    _same(inv2, i0, "1 / scale (no scale)")
    # the oracle: exact sums; mean within 2 ulp and scale inside the interval the roundings allow (the bounds of
    # tests/test_gpu_moments_paths.py for standardise_params_kernel)
    want, _ = mr.exact_column_sums(X, shift)
    sums = sums1.to_host()
    np.testing.assert_array_equal(sums, want)
    rmean, rscale, _ = mr.standardise(sums, shift, n, True)
    mean, scale, inv = mean1.to_host(), scale1.to_host(), inv1.to_host()
    assert np.all(np.abs(mean - rmean) <= 2.0 * np.spacing(np.abs(rmean)))
    np.testing.assert_array_equal(inv, 1.0 / scale)
    for f in range(F):
        lo, hi = mr.std_interval(sums, f, F, n)
        assert lo > 1e-12 and lo <= scale[f] <= hi, (f, lo, scale[f], hi)


# ---------------------------------------------------------------------------------------------------------------------
# 2. projection without its clear
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("finite", [True, False], ids=["finite", "nan-aware"])
@pytest.mark.parametrize("F,d", [(64, 10), (5, 2)], ids=["mfma-F64-d10", "plain-F5-d2"])
def test_project_preset(engine, F, d, finite):
    n = 100
    rng = np.random.default_rng(F)
    X = rng.normal(size=(n, F)).astype(np.float32)
    mu, inv_sigma, m2 = rng.normal(size=F), 1.0 / (0.5 + rng.random(F)), rng.normal(size=F) * 0.1
    W = rng.normal(size=(F, F))
    x, mu_d, is_d, m2_d, W_d = (engine.to_device(a) for a in (X, mu, inv_sigma, m2, W))
    stale = engine.to_device(np.array([GARBAGE64], np.uint64)).view((1,), np.float64)     # a huge stale maximum
    Y0 = engine.project(x, mu_d, is_d, W_d, d, mean2=m2_d, absmax=stale, assume_finite=finite)
    zeroed = engine.zeros((1,), np.float64)
    Y1 = engine.project(x, mu_d, is_d, W_d, d, mean2=m2_d, absmax=zeroed, assume_finite=finite, absmax_preset=True)
    _same(Y1, Y0, "Y")
    _same(zeroed, stale, "max |Y|")
    Y = Y0.to_host()
    assert stale.to_host()[0] == np.abs(Y).max()
    np.testing.assert_allclose(Y, mr.exact_project(X, mu, inv_sigma, m2, W, d), rtol=0, atol=1e-9 * np.abs(Y).max())


# ---------------------------------------------------------------------------------------------------------------------
# 3. k-means start: member sums cleared by fit_begin, first pass without a label fill
# ---------------------------------------------------------------------------------------------------------------------
_FIRST = [(n, d, k) for n in (1, 63, 64, 65, 1000) for d in (1, 4, 10) for k in (1, 17, 500) if n >= k]
_FIRST.append((1000, 11, 17))       # d = 11: outside the filter's range, the all-fp64 kernel runs


def _lloyd_run(engine, Y, k, *, folded, label_fill=None, use_lloyd=True):
    """fit_begin + two passes; -> (labels, sums, counts, centres, state) after each pass, as host arrays."""
    n, d = Y.shape
    centers, state = engine.empty((k, d), np.float64), engine.zeros((8,), np.float64)
    labels = engine.empty((n,), np.int32)
    acc = engine.empty((k * d + k,), np.int64)
    sums, counts = acc.view((k * d,)), acc.view((k,), offset_elems=k * d)
    if folded:
        labels.copy_from_host(label_fill)
        acc.fill_bytes_(0x5A)
        engine.kmeans_fit_begin(Y, k, seed=3, n_total=n, tol2=0.0, centers=centers, state=state, sums=sums, counts=counts)
    else:
        engine.kmeans_fit_begin(Y, k, seed=3, n_total=n, tol2=0.0, centers=centers, state=state)
        acc.zero_()
        labels.fill_bytes_(0xFF)
    nbytes = engine.kmeans_image_bytes(n, d)
    image = engine.kmeans_pack(Y, image=engine.empty((nbytes,), np.uint8),
                               absmax=state.view((1,), offset_elems=2)) if nbytes else None
    out = []
    for it in range(2):
        kw = {"first_pass": True} if folded and it == 0 else {}
        if use_lloyd:
            engine.kmeans_lloyd_pass(Y, centers, state, sums, counts, image=image, prev_labels=labels, **kw)
        else:
            engine.kmeans_accumulate(Y, centers, state, sums, counts, image=image, prev_labels=labels, **kw)
            engine.kmeans_update(sums, counts, centers, state, clear=False)
        out.append(tuple(a.to_host() for a in (labels, sums, counts, centers, state)))
    return out


@pytest.mark.parametrize("n,d,k", _FIRST, ids=[f"n{n}-d{d}-k{k}" for n, d, k in _FIRST])
def test_first_pass(engine, n, d, k):
    nc = max(2, min(k, 12))
    pts, _ = _gen.gaussian_clusters(nc, -(-n // nc), d, seed=n + d + k)
    pts = pts[np.random.default_rng(k).permutation(len(pts))[:n]]          # frames of every blob, in no order
    Y = engine.to_device(np.ascontiguousarray(pts))
    assert Y.shape == (n, d)
    want = _lloyd_run(engine, Y, k, folded=False)
    fills = {"sevens": np.full(n, 7, np.int32),
             "out of range": np.resize(np.array([k, k + 3, 2**31 - 1, -5, -2**31], np.int64), n).astype(np.int32)}
    names = ("labels", "member sums", "member counts", "centres", "fit state")
    for tag, fill in fills.items():
        for use_lloyd in (True, False):
            got = _lloyd_run(engine, Y, k, folded=True, label_fill=fill, use_lloyd=use_lloyd)
            for it in range(2):
                for name, a, b in zip(names, got[it], want[it]):
                    _same(a, b, f"{name} after pass {it + 1} (labels pre-filled with {tag}, lloyd_pass={use_lloyd})")
    # the reference run itself against the oracle: the labels of pass 2 are the assignment to the centres of pass 1
    labels2, _, counts2, _, _ = want[1]
    np.testing.assert_array_equal(labels2, cport.kmeans_assign(Y.to_host(), want[0][3]))
    np.testing.assert_array_equal(counts2, np.bincount(labels2, minlength=k))


# ---------------------------------------------------------------------------------------------------------------------
# 4. counts and the row-normalised matrix from one launch
# ---------------------------------------------------------------------------------------------------------------------
def _label_sets(n, k):
    rng = np.random.default_rng(n + k)
    uniform = rng.integers(0, k, size=n).astype(np.int32)
    missing = uniform.copy()
    if k > 1:
        missing[missing == k // 2] = (k // 2 + 1) % k          # state k // 2 is never visited: a zero row and column
    return {"uniform": uniform, "one state": np.full(n, k - 1, np.int32), "state never visited": missing}


def _counts_both(engine, lab, k, lag):
    labels = engine.to_device(lab)
    junk = lambda shape, dt: engine.empty(shape, dt).fill_bytes_(0x5A)     # noqa: E731
    c0, p0 = engine.count_transitions(labels, k, lag, out=junk((k, k), np.int64), pairs=junk((1,), np.int64))
    T0, rs0, dm0 = junk((k, k), np.float64), junk((k,), np.float64), junk((1,), np.float64)
    engine.row_normalise_into(c0, T0, rs0, dm0)
    T1, rs1, dm1 = junk((k, k), np.float64), junk((k,), np.float64), junk((1,), np.float64)
    c1, p1 = engine.count_transitions_normalised(labels, k, lag, T1, rs1, dm1, out=junk((k, k), np.int64),
                                                 pairs=junk((1,), np.int64))
    for what, a, b in (("counts", c1, c0), ("pair total", p1, p0), ("rowsum", rs1, rs0), ("T", T1, T0),
                       ("diagonal mass", dm1, dm0)):
        _same(a, b, what)
    want, pw = cport.count_transitions(lab, k, lag)
    np.testing.assert_array_equal(c1.to_host(), want)
    assert int(p1.to_host()[0]) == pw
    np.testing.assert_array_equal(T1.to_host(), npport.normalise_counts(want))
    np.testing.assert_array_equal(rs1.to_host(), want.sum(axis=1).astype(np.float64))


@pytest.mark.parametrize("chunk", [None, "64"], ids=["default-chunks", "chunks-of-64"])
@pytest.mark.parametrize("k,n", [(2, 200), (33, 5000), (500, 300_000)])
def test_counts_normalised(engine, monkeypatch, k, n, chunk):
    if chunk:
        monkeypatch.setenv("MSM_COUNTS_CHUNK", chunk)      # many chunks at these sizes (read by every call)
    lag = 3
    assert n - lag >= k * k                                # the dense two-pass counting runs
    for tag, lab in _label_sets(n, k).items():
        _counts_both(engine, lab, k, lag)


def test_counts_normalised_sparse_fallback(engine):
    k, n, lag = 500, 5000, 3
    assert n - lag < k * k                                 # too few pairs: counting and normalising stay two launches
    for tag, lab in _label_sets(n, k).items():
        _counts_both(engine, lab, k, lag)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the whole step
# ---------------------------------------------------------------------------------------------------------------------
def _step_outputs(msm):
    own = ("mean", "scale", "inv_scale", "eig", "W", "m2", "rank_d", "Y", "labels", "T", "rowsum", "diag")
    out = {f"buf.{nm}": a.to_host().copy() for nm, a in msm.buf.items()}
    out.update({nm: getattr(msm, nm).to_host().copy() for nm in own if getattr(msm, nm, None) is not None})
    # the frame images: 48 bytes per frame for whole units of 64 frames, then the frames' scale in the int32 at byte 8
    # of the closing 16 (the other 12 bytes are never written)
    rows = (msm.cfg.n_frames + 63) // 64 * 64 * 48
    img = msm.km_image.to_host()
    out["km_image rows"], out["km_image scale"] = img[:rows].copy(), img[rows + 8:rows + 12].copy()
    return out


def test_whole_step(engine, monkeypatch):
    n, F, d, k, lag = 4096, 8, 3, 16, 2
    cfg = ShardConfig(n_frames=n, n_features=F, tica_dim=d, k=k, lag=lag, kmeans_iters=3, seed=1)
    X = _gen.correlated_series(n, F, seed=11).astype(np.float32)
    monkeypatch.setenv("MSM_STEP_FOLDS", "0")
    plain = ShardedMSM(engine, cfg, engine.to_device(X))
    monkeypatch.delenv("MSM_STEP_FOLDS")
    folded = ShardedMSM(engine, cfg, engine.to_device(X))
    assert folded.folds and not plain.folds
    for _ in range(2):                 # the second step starts from what the first left in every buffer
        plain.step()
        folded.step()
        engine.sync()
        want, got = _step_outputs(plain), _step_outputs(folded)
        assert want.keys() == got.keys()
        for nm in want:
            _same(got[nm], want[nm], nm)
    # against the oracle: labels given the centres, counts and T given the labels
    labels = want["labels"]
    np.testing.assert_array_equal(labels, cport.kmeans_assign(want["Y"], want["buf.centers"]))
    cw, pw = cport.count_transitions(labels, k, lag)
    np.testing.assert_array_equal(got["buf.counts"][:k * k].reshape(k, k), cw)
    assert int(got["buf.counts"][k * k]) == pw
    np.testing.assert_array_equal(got["T"], npport.normalise_counts(cw))
    # the folded step from a captured graph
    engine.graph_begin()
    folded.step()
    g = engine.graph_end()
    try:
        for _ in range(2):
            for a in (folded.buf["counts"], folded.T, folded.labels, folded.Y, folded.buf["km_acc"], folded.rowsum):
                a.fill_bytes_(0x5A)
            engine.graph_launch(g)
            engine.sync()
            got = _step_outputs(folded)
            for nm in want:
                _same(got[nm], want[nm], f"{nm} (graph replay)")
    finally:
        engine.graph_destroy(g)
