"""Metadynamics end to end on the device: HillsLedger, metadynamics_weights, MetadynamicsReweighter and
MetadynamicsCVBias against tests/_metad_ref.py (80-bit floats), PLUMED's recorded run (tests/golden/metad) and, for the
DeepTICA chain, tests/_bias_ref.py.

The golden run needs this much of its input files: 2 CVs, sigma = 0.1, height 0.5, one hill per 500 steps of 0.001,
`biasf -1` (no tempering), the bias served from a grid over [-1.5, 1.5] x [-0.5, 2.5].  kT = 1 in the weights tests is
this file's choice (the unit is arbitrary: only V / kT enters).

Bounds.
  * bias and gradient of a frame: tests/_metad_ref.bound_factor times the sum of the terms' magnitudes; the gradient
    also by the coarser product form, the value's bound times max |dp / sigma^2| over the frame's live hills.
  * against PLUMED: 2e-3, twice the 1.003e-3 the restatement itself is away (tests/test_metad_reference.py).
  * c(t): kT (a1 + a2) max bound_V + 2 kT (log2 G + 6) eps: both log-sum-exps are contractions of V's error, and each
    carries log2 G + 6 roundings.
  * log-weights: (bound_V(n) + bound_c) / kT per frame before normalising; normalising subtracts one log-sum-exp of the
    n values, a contraction again, formed on the host in pairwise sums: (log2 n + 4) eps max(1, |LSE|) more.
  * well-tempered heights: the relative error of h_k is the absolute error of V_k(c_k) / ((gamma - 1) kT) plus 4
    roundings, and V_k's error is its rounding bound plus the earlier heights' relative errors times V_k: the
    recursion is evaluated in the test.
  * the DeepTICA chain, stage by stage on the device's own intermediates: CVs against the reference's recorded fp64
    values with the recorded tolerance of tests/test_gpu_bias.py (4 x |restatement - ref64|), the hills sum by the bound
    above, the network adjoint and the featurizer adjoint with that file's 4 x |float64 - longdouble| gaps.
  * the DeepTICA chain as a whole against the numpy chain (fp32 features -> network -> hills -> both adjoints).
    Energy: V is Lipschitz in the CVs with L_i = sum_k h_k A e^(-1/2) / sigma_ki (z e^(-z^2/2) <= e^(-1/2)), the device's
    CVs are within tol_cv of the recorded fp64 values and the restatement's within tol_cv / 4 (that is how tol_cv was
    recorded), so |E - V(numpy CVs)| <= 1.25 tol_cv sum_i L_i + the hills sum's rounding bound; it must also stay inside
    the recorded energy tolerance of the harmonic chain.  Forces: tests/test_gpu_bias.py holds F of the harmonic chain
    E = K sum cv^2 to its numpy chain within a recorded tolerance.  A force is -J' g with g the upstream gradient; the
    harmonic g reaches 2 K (|cv| < 1 behind a tanh head) and changes with the CVs at the rate 2 K, the hills' g is at
    most max_i L_i and changes at most at the rate max_i sum_j sum_k h_k A / (sigma_ki sigma_kj) (|z_i z_j - delta_ij|
    e^(-z^2/2) <= 1).  The recorded force tolerance is scaled by the larger of the two ratios, and never up."""

from __future__ import annotations

import json

import numpy as np
import pytest

from pmarlo_amd.device import DeviceArray
from pmarlo_amd.features.deeptica import MetadynamicsCVBias, MLPSpec, feature_spec_sha256
from pmarlo_amd.features.deeptica.ts_feature_extractor import build_feature_extractor_module, canonicalize_feature_spec
from pmarlo_amd.reweight import (HillsLedger, MetadynamicsReweighter, Reweighter, metadynamics_weights, read_colvar,
                                 read_hills)
from tests import _bias_ref as B
from tests import _metad_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

PLUMED_TOL = 2.0e-3
LO, HI, BINS = [-1.5, -0.5], [1.5, 2.5], [61, 61]
KT = 1.0


@pytest.fixture(scope="module")
def run(engine):
    led = read_hills(GOLDEN / "metad" / "HILLS", engine=engine)
    col = read_colvar(GOLDEN / "metad" / "COLVAR")
    cv = np.stack([col["cv.x"], col["cv.y"]], axis=1)
    counts = R.counts_from_times(led.times, col["time"])
    ref = R.bias(cv, led.packed(), counts, kernel=led.kernel, dtype=np.longdouble)
    return led, col, cv, counts, {k: np.asarray(v, np.float64) for k, v in ref.items()}


def _grad_bound_product_form(cv, packed, counts, mag, d):
    """value's bound x max |dp / sigma^2| over the hills the frame sees inside the cutoff."""
    dp = cv[:, None, :] - packed[None, :, :d]
    isg = packed[None, :, d:2 * d]
    live = (0.5 * ((dp * isg) ** 2).sum(axis=2) < R.CUT) & (np.arange(packed.shape[0])[None, :] < counts[:, None])
    r = np.where(live[..., None], np.abs(dp) * isg * isg, 0.0).max(axis=1)
    return (R.bound_factor(d, counts) * mag)[:, None] * r


# ------------------------------------------------------------------------------------------------- the golden run
def test_golden_bias_and_gradient(run):
    led, col, cv, counts, ref = run
    V, g = led.bias(cv, times=col["time"], grad=True)
    assert V.shape == (2501,) and g.shape == (2501, 2) and V.dtype == np.float64
    f = R.bound_factor(2, counts)
    err = np.abs(V - ref["bias"])
    live = ref["mag"] > 0
    print(f"bias: largest |device - longdouble| = {(err[live] / ref['mag'][live]).max() / R.EPS:.1f} eps x magnitudes; "
          f"max |device - PLUMED| = {np.max(np.abs(V - col['metad.bias'])):.4e}")
    assert (err <= f * ref["mag"]).all() and not V[~live].any()
    assert np.max(np.abs(V - col["metad.bias"])) <= PLUMED_TOL
    gerr = np.abs(g - ref["grad"])
    assert (gerr <= f[:, None] * ref["gmag"]).all() and not g[ref["gmag"] == 0].any()
    assert (gerr <= _grad_bound_product_form(cv, led.packed(), counts, ref["mag"], 2)).all()
    # counts in place of times, and value only: the same bits
    np.testing.assert_array_equal(led.bias(cv, counts=counts), V)
    # device in, device out
    cvd = led.engine.to_device(cv)
    out = led.bias(cvd, counts=counts)
    assert isinstance(out, DeviceArray)
    np.testing.assert_array_equal(out.to_host(), V)
    # all hills for every frame is another question with another answer
    assert (led.bias(cv)[counts < 50] >= V[counts < 50]).all() and led.bias(cv)[0] > 0 == V[0]


def _c_bound(led, kT, ck, a1, a2):
    lo, step, bins = led.grid(LO, HI, BINS)
    _l, _vh, bound_v = R.scan(led.packed(), lo, step, bins, ck, a1, a2, kernel=led.kernel)
    G = float(np.prod(bins))
    return kT * (a1 + a2) * bound_v.max() + 2 * kT * (np.log2(G) + 6) * R.EPS


@pytest.mark.parametrize("stride", [1, 3])
def test_golden_tiwary_weights(run, stride):
    led, col, cv, counts, ref = run
    res = metadynamics_weights(led, cv, col["time"], KT, method="tiwary", grid=(LO, HI, BINS), rct_stride=stride)
    lo, step, bins = led.grid(LO, HI, BINS)
    logw, c, V = R.tiwary_log_weights(cv, counts, led.packed(), lo, step, bins, KT, None, stride, kernel=led.kernel,
                                      dtype=np.longdouble)
    ck = R.checkpoints(50, stride)
    assert res.c.shape == (ck.size,) and res.c[0] == 0.0 and (np.diff(res.c) > 0).all()
    tol_c = _c_bound(led, KT, ck, 1.0 / KT, 0.0)
    print(f"stride {stride}: max |c - longdouble| = {np.max(np.abs(res.c - c.astype(np.float64))):.3e}, bound {tol_c:.3e}; "
          f"c_H = {res.c[-1]:.6f}, ESS = {res.ess:.1f} of 2501")
    assert np.max(np.abs(res.c - c.astype(np.float64))) <= tol_c
    w, lw, ess = R.normalise(logw)
    per_frame = (R.bound_factor(2, counts) * ref["mag"] + tol_c) / KT
    tol = 2 * per_frame.max() + (np.log2(2501) + 4) * R.EPS * np.maximum(1.0, np.abs(lw.astype(np.float64)))
    assert (np.abs(res.log_weights - lw.astype(np.float64)) <= tol).all()
    assert (np.abs(res.weights - w.astype(np.float64)) <= 2 * tol * w.astype(np.float64)).all()
    assert abs(res.weights.sum() - 1.0) <= 64 * R.EPS and abs(res.ess - ess) <= 1e-9 * ess
    weights, log_weights, kish = res
    assert weights is res.weights and log_weights is res.log_weights and kish == res.ess
    if stride == 3:          # held between evaluations: V - kT log w is one constant per group of 3 counts
        offset = res.bias - KT * res.log_weights
        for k in range(17):
            group = offset[counts // 3 == k]
            assert group.size and np.ptp(group) <= 64 * R.EPS * np.abs(group).max()
        assert offset[counts == 5][0] < offset[counts == 6][0]
        one = metadynamics_weights(led, cv, col["time"], KT, grid=(LO, HI, BINS), rct_stride=1)
        np.testing.assert_array_equal(res.c, one.c[::3])


def test_golden_final_weights_fes_and_grid(run):
    led, col, cv, counts, ref = run
    res = metadynamics_weights(led, cv, None, KT, method="final")
    full = R.bias(cv, led.packed(), kernel=led.kernel, dtype=np.longdouble)
    w, lw, ess = R.normalise(full["bias"] / np.longdouble(KT))
    tol = 2 * (R.bound_factor(2, np.full(2501, 50)) * full["mag"].astype(np.float64)).max() / KT + \
        (np.log2(2501) + 4) * R.EPS * np.maximum(1.0, np.abs(lw.astype(np.float64)))
    assert res.c is None and (np.abs(res.log_weights - lw.astype(np.float64)) <= tol).all()
    # the grid: V_H at every point is the frame kernel's value there; the FES is its mirror image, minimum 0
    lo, step, bins = led.grid(LO, HI, BINS)
    assert step[0] == 3.0 / 60
    pts = R.grid_points(lo, step, bins)
    vg = led.on_grid(LO, HI, BINS)
    assert vg.shape == (61, 61)
    np.testing.assert_array_equal(vg.reshape(-1), led.bias(pts))
    want = R.bias(pts, led.packed(), kernel=led.kernel, dtype=np.longdouble)
    assert (np.abs(vg.reshape(-1) - want["bias"].astype(np.float64))
            <= R.bound_factor(2, np.full(pts.shape[0], 50)) * want["mag"].astype(np.float64)).all()
    fes = led.fes(LO, HI, BINS)
    np.testing.assert_array_equal(fes, -vg - (-vg).min())
    assert fes.min() == 0.0 and fes.max() == vg.max()
    tempered = HillsLedger.from_arrays(led.times, led.centers, led.sigmas, led.heights, kernel=led.kernel,
                                       bias_factor=5.0, engine=led.engine)
    np.testing.assert_array_equal(tempered.fes(LO, HI, BINS), -(5.0 / 4.0) * vg - (-(5.0 / 4.0) * vg).min())


def test_reweighter_layout(run):
    led, col, cv, counts, ref = run
    cut = 1300
    data = {"splits": {"a": {"cv": cv[:cut], "time": col["time"][:cut]},
                       "b": {"cv": cv[cut:], "time": col["time"][cut:], "ledger": GOLDEN / "metad" / "HILLS"}},
            "frame_weights": {"old": np.ones(3)}}
    rw = MetadynamicsReweighter(kT=KT, ledger=led, grid=(LO, HI, BINS))
    out = rw.apply(data)
    whole = metadynamics_weights(led, cv, col["time"], KT, grid=(LO, HI, BINS))
    assert set(out) == {"a", "b"} and set(data["frame_weights"]) == {"old", "a", "b"}
    assert data["frame_weights"]["a"].shape == (cut,) and data["frame_weights"]["a"].dtype == np.float64
    np.testing.assert_allclose(np.concatenate([out["a"], out["b"]]), whole.weights, rtol=1e-13)
    assert abs(out["a"].sum() + out["b"].sum() - 1.0) < 1e-13 and rw.result["ess"] == pytest.approx(whole.ess)
    # splits that share a ledger share its c(t): one grid scan, not one per split
    calls = []
    scan = led.scan
    led.scan = lambda *a, **k: calls.append(1) or scan(*a, **k)
    try:
        shared = rw.apply({"splits": {"a": data["splits"]["a"], "b": {"cv": cv[cut:], "time": col["time"][cut:]}}})
    finally:
        del led.scan
    assert len(calls) == 1
    np.testing.assert_array_equal(np.concatenate([shared["a"], shared["b"]]), np.concatenate([out["a"], out["b"]]))
    # a split's own ledger is used even when it is empty (no hills: no bias, uniform weights)
    none = HillsLedger(2, kernel=led.kernel, engine=led.engine)
    flat = rw.apply({"splits": {"a": {"cv": cv[:10], "time": col["time"][:10], "ledger": none}}})["a"]
    np.testing.assert_allclose(flat, np.full(10, 0.1), rtol=4 * R.EPS, atol=0)
    # Reweighter keeps its contract: metadynamics is not one of its modes
    with pytest.raises(ValueError, match="MBAR"):
        Reweighter(300.0, mode="metadynamics")
    for bad, what in (({}, "splits"), ({"splits": {"a": {"time": [0.0]}}}, "cv"),
                      ({"splits": {"a": {"cv": cv[:4]}}}, "time"),
                      ({"splits": {"a": {"cv": cv[:4], "time": [0.0, 1.0]}}}, "entries")):
        with pytest.raises(ValueError, match=what):
            rw.apply(bad)
    with pytest.raises(ValueError, match="ledger"):
        MetadynamicsReweighter(kT=KT, grid=(LO, HI, BINS)).apply({"splits": {"a": {"cv": cv[:4], "time": col["time"][:4]}}})


# ---------------------------------------------------------------------------------------------- deposition
def test_well_tempered_heights(engine):
    gamma, kT, h0 = 6.0, 0.8, 1.2
    rng = np.random.default_rng(17)
    centers = rng.normal(scale=0.25, size=(9, 2))
    sig = np.array([0.3, 0.2])
    led = HillsLedger(2, sigma=sig, height=h0, bias_factor=gamma, kT=kT, kernel="stretched-gaussian", capacity=4,
                      engine=engine)
    dev = HillsLedger(2, sigma=sig, height=h0, bias_factor=gamma, kT=kT, kernel="stretched-gaussian", capacity=16,
                      engine=engine)
    for c in centers:                      # `led` grows twice on the way; `dev` takes its centres from the device
        led.add_hill(c)
        dev.add_hill(engine.to_device(c.reshape(1, 2)))
    got = led.heights
    np.testing.assert_array_equal(dev.heights, got)
    np.testing.assert_array_equal(dev.centers, centers)
    np.testing.assert_array_equal(led.centers, centers)
    np.testing.assert_array_equal(led.times, np.arange(9.0))
    assert got[0] == h0 and (got[1:] < h0).all()
    # the law, sequentially, in 80-bit floats; the error recursion beside it
    L = np.longdouble
    heights, delta = [], []
    for k, c in enumerate(centers):
        V, Mg = L(0), 0.0
        if k:       # unit heights through the law, the 80-bit heights applied here
            term, _d, mag, _g = R.hill_terms(c.reshape(1, 2), R.pack(centers[:k], np.broadcast_to(sig, (k, 2)), np.ones(k)),
                                             kernel="stretched-gaussian", dtype=L)
            V, Mg = (term[0] * np.asarray(heights, L)).sum(), float((mag[0] * np.asarray(heights, L)).sum())
        heights.append(L(h0) * np.exp(-V / L((gamma - 1.0) * kT)))
        err_v = (R.bound_factor(2, [k])[0] + (max(delta) if delta else 0.0)) * Mg
        delta.append(err_v / ((gamma - 1.0) * kT) + 4 * R.EPS)
    want = np.asarray(heights, np.float64)
    print("well-tempered heights:", got, "relative error", np.abs(got - want) / want, "bound", delta)
    assert (np.abs(got - want) <= np.asarray(delta) * want).all()
    # a given height overrides the rule; the ledger then evaluates like any other
    led.add_hill([0.0, 0.0], height=0.25, time=20.0)
    assert led.heights[-1] == 0.25 and led.times[-1] == 20.0 and len(led) == 10
    ref = R.bias(centers, led.packed(), kernel="stretched-gaussian", dtype=L)
    V = led.bias(centers)
    bound = R.bound_factor(2, np.full(9, 10)) * ref["mag"].astype(np.float64)
    assert (np.abs(V - ref["bias"].astype(np.float64)) <= bound).all()


def test_nan_frames_are_isolated(run):
    led, col, cv, counts, ref = run
    dirty = cv[:300].copy()
    rows = [0, 5, 63, 64, 130, 299]
    dirty[rows[0], 0], dirty[rows[1], 1], dirty[rows[2], 0] = np.nan, np.inf, -np.inf
    dirty[rows[3]], dirty[rows[4], 1], dirty[rows[5], 0] = np.nan, np.nan, np.inf
    V, g = led.bias(dirty, grad=True)
    clean_V, clean_g = led.bias(cv[:300], grad=True)
    assert np.isnan(V[rows]).all() and np.isnan(g[rows]).all()
    keep = np.setdiff1d(np.arange(300), rows)
    np.testing.assert_array_equal(V[keep], clean_V[keep])
    np.testing.assert_array_equal(g[keep], clean_g[keep])
    # with no hills to see, a NaN frame is still NaN
    assert np.isnan(led.bias(dirty[:1], counts=[0])[0]) and led.bias(cv[:1], counts=[0])[0] == 0.0
    with pytest.raises(ValueError, match="non-finite"):
        metadynamics_weights(led, dirty, None, KT, method="final")


def test_every_value_error(run, engine):
    led, col, cv, counts, ref = run
    hills = led.device_hills()
    cvd = engine.to_device(cv[:8])
    with pytest.raises(ValueError, match="columns"):
        led.bias(np.zeros((4, 3)))
    with pytest.raises(ValueError, match="not both"):
        led.bias(cv[:4], times=col["time"][:4], counts=counts[:4])
    with pytest.raises(ValueError, match="for 4 frames"):
        led.bias(cv[:4], counts=counts[:3])
    with pytest.raises(ValueError, match="outside"):
        led.bias(cv[:2], counts=[0, 51])
    with pytest.raises(ValueError, match="outside"):
        led.bias(cv[:2], counts=[-1, 5])
    assert led.bias(np.zeros((0, 2))).shape == (0,)
    for kw in (dict(kernel="box"), dict(cut=0.0), dict(cut=np.inf), dict(periods=[1.0]), dict(periods=[-1.0, 0.0]),
               dict(counts=engine.to_device(np.zeros(7, np.int32))), dict(counts=engine.to_device(np.zeros(8, np.int64))),
               dict(bias=engine.empty((7,), np.float64)), dict(grad_out=engine.empty((8, 1), np.float64)),
               dict(max_workgroups=-1)):
        with pytest.raises(ValueError):
            engine.metad_bias(cvd, hills, 50, **kw)
    with pytest.raises(ValueError):
        engine.metad_bias(cvd, hills, 51)
    with pytest.raises(ValueError):
        engine.metad_bias(engine.to_device(cv[:8, :1]), hills, 50)               # too few CV columns
    with pytest.raises(ValueError):
        engine.metad_bias(engine.to_device(cv[:8].astype(np.float32)), hills, 50)
    with pytest.raises(ValueError):
        engine.metad_bias(cvd, engine.to_device(np.zeros((4, 4))), 4)            # not 2 d + 1 columns
    with pytest.raises(ValueError):
        engine.metad_bias(engine.to_device(np.zeros((2, 9))), engine.to_device(np.ones((4, 19))), 4)     # d = 9
    for args in ((5, [0.0, 0.0, 10.0, 10.0, 1.0]), (0, [0.0, 0.0, 10.0, 10.0]), (0, [0.0, 0.0, 10.0, 0.0, 1.0]),
                 (0, [0.0, 0.0, 10.0, 10.0, -1.0]), (-1, [0.0, 0.0, 10.0, 10.0, 1.0])):
        with pytest.raises(ValueError):
            engine.metad_append(engine.zeros((5, 5), np.float64), *args)
    for kw, what in ((dict(kT=None), "kT"), (dict(method="bonomi"), "method"), (dict(grid=None), "grid"),
                     (dict(rct_stride=0), "rct_stride"), (dict(kT=-1.0), "kT"), (dict(times=None), "times")):
        args = dict(times=col["time"][:8], kT=KT, method="tiwary", grid=(LO, HI, BINS), rct_stride=1)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            metadynamics_weights(led, cv[:8], **args)
    with pytest.raises(ValueError):
        led.on_grid(LO, [1.5, -0.5], BINS)
    with pytest.raises(ValueError, match="at most"):
        HillsLedger.from_arrays([0.0], np.zeros((1, 4)), 0.1, 1.0, engine=engine).on_grid(0, 1, 4)
    with pytest.raises(ValueError, match="negative"):
        HillsLedger.from_arrays([0.0, 1.0], np.zeros((2, 1)), 0.1, [1.0, -1.0], engine=engine).on_grid(0, 1, 4)


# ------------------------------------------------------------------------------------ the DeepTICA chain
CASE, NET = "ortho", "tanh"


@pytest.fixture(scope="module")
def chain(engine):
    g = np.load(GOLDEN / "bias.npz", allow_pickle=False)
    meta = json.loads((GOLDEN / "bias.json").read_text())
    raw = json.loads((GOLDEN / "pbc.json").read_text())["spec"]
    spec = canonicalize_feature_spec(raw)
    rec, param, _width = B.table_from_spec(spec)
    gaps = meta["gaps"]
    tol = ({q: 4.0 * v for q, v in gaps["restatement_minus_ref64"].items()},
           4.0 * gaps["featurize_vjp_f64_minus_longdouble"], 4.0 * gaps["mlp_vjp_f64_minus_longdouble"],
           2.0 * meta["strength"])
    mean, scale = g[f"{CASE}_mean"], g[f"{CASE}_scale"]
    xyz, box = g[f"{CASE}_xyz"], g[f"{CASE}_box"]

    def potential(ledger, net_name=NET):
        net = B.golden_network(net_name, mean, scale)
        ms = MLPSpec(net["widths"], net["activation"], net["ln_in"], net["ln_hidden"], net["head_activation"],
                     net["params"], net["mean"], net["scale"])
        return MetadynamicsCVBias(ms, mean, scale, ledger, feature_extractor=build_feature_extractor_module(spec, engine),
                                  feature_spec_hash=feature_spec_sha256(raw)), net

    return g, rec, param, tol, xyz, box, potential


def _assert_adjoint(got, want, scale, gap, what):
    ratio = np.abs(got - want)[scale > 0] / scale[scale > 0]
    print(f"{what}: largest |device - restatement| / sum|terms| = {ratio.max():.3e}, bound {gap:.3e}")
    assert np.isfinite(got).all() and not got[scale == 0].any() and ratio.max() <= gap, what


def test_cv_bias_three_frames_five_hills(engine, chain):
    g, rec, param, tol, xyz, box, potential = chain
    # CVs of a tanh head lie in (-1, 1): with these widths every hill is inside the cutoff of every frame
    led = HillsLedger(3, sigma=[1.0, 0.9, 1.1], kernel="stretched-gaussian", engine=engine)
    bias, net = potential(led)
    frames, at = xyz[:3], xyz[3:8]
    centers = bias.compute_cvs(at, box[3:8])
    for k, c in enumerate(centers):
        led.add_hill(c, height=0.4 + 0.1 * k)
    E, F = bias.energy_and_forces(frames, box[:3])
    cv = bias.compute_cvs(frames, box[:3])
    assert E.shape == (3,) and cv.shape == (3, 3) and F.shape == frames.shape and F.dtype == np.float64
    # stage 1: the CVs against the reference's recorded fp64 values, as tests/test_gpu_bias.py holds them
    feats_ref = B.features(rec, param, frames, box[:3], "round", np.float32)
    _e, y_ref, _gx, _s = B.mlp_vjp(net, feats_ref, None, 1.0)
    assert np.max(np.abs(cv - g[f"{CASE}__{NET}__cv64"][:3])) <= tol[0]["cv"]
    res = bias.energy_and_forces_device(engine.to_device(frames), box[:3])
    np.testing.assert_array_equal(res["cv"].to_host(), cv)
    np.testing.assert_array_equal(res["energy"].to_host(), E)
    np.testing.assert_array_equal(res["force"].to_host(), F)
    # stage 2: the hills sum at those CVs
    ref = R.bias(cv, led.packed(), kernel=led.kernel, dtype=np.longdouble)
    f = R.bound_factor(3, np.full(3, 5))
    assert (ref["mag"] > 0).all()
    assert (np.abs(E - ref["bias"].astype(np.float64)) <= f * ref["mag"].astype(np.float64)).all()
    Vd, gd = led.bias(res["cv"], grad=True)
    np.testing.assert_array_equal(Vd.to_host(), E)
    grad = gd.to_host()
    assert (np.abs(grad - ref["grad"].astype(np.float64)) <= f[:, None] * ref["gmag"].astype(np.float64)).all()
    # stage 3: the network's adjoint of that gradient, stage 4: the featurizer's, on the device's own intermediates
    feats = res["features"].to_host()
    _e, _y, gx_ref, gx_scale = B.mlp_vjp(net, feats, grad, 1.0)
    gx = engine.mlp_vjp(res["features"], bias.spec, gout=gd, want_energy=False, want_outputs=False)["gx"]
    _assert_adjoint(gx.to_host(), gx_ref, gx_scale, tol[2], "mlp_vjp of the hills gradient")
    F_ref, F_scale = B.featurize_vjp(rec, param, frames, gx.to_host(), box[:3], "round", sign=-1.0, width=feats.shape[1])
    _assert_adjoint(F, F_ref, F_scale, tol[1], "forces")
    assert np.abs(F).max() > 0
    # the chain as a whole against the numpy chain; the tolerances are derived in the module docstring
    packed = led.packed()
    chain_ref = R.bias(y_ref, packed, kernel=led.kernel)
    gx_chain = B.mlp_vjp(net, feats_ref, chain_ref["grad"], 1.0)[2]
    F_chain, _ = B.featurize_vjp(rec, param, frames, gx_chain, box[:3], "round", sign=-1.0, width=feats.shape[1])
    weight = packed[:, 6] * R.constants(led.kernel)[0]                       # h_k A
    lip = (weight[:, None] * np.exp(-0.5) * packed[:, 3:6]).sum(axis=0)      # L_i
    hess = np.einsum("k,ki,kj->ij", weight, packed[:, 3:6], packed[:, 3:6]).sum(axis=1).max()
    tol_E = min(tol[0]["energy"], 1.25 * tol[0]["cv"] * lip.sum() + float((f * ref["mag"].astype(np.float64)).max()))
    tol_F = tol[0]["force"] * min(1.0, max(lip.max() / tol[3], hess / tol[3]))
    err_y, err_E = np.max(np.abs(cv - y_ref)), np.max(np.abs(E - chain_ref["bias"]))
    err_F = np.max(np.abs(F - F_chain))
    print(f"against the numpy chain: cv {err_y:.3e} / {1.25 * tol[0]['cv']:.3e}, energy {err_E:.3e} / {tol_E:.3e}, "
          f"force {err_F:.3e} / {tol_F:.3e} (largest force {np.abs(F).max():.3e})")
    assert err_y <= 1.25 * tol[0]["cv"] and err_E <= tol_E and err_F <= tol_F
    # one frame is one MD step: a scalar, (A, 3), the batch's bits
    e1, f1 = bias.energy_and_forces(frames[1], box[1])
    assert np.ndim(e1) == 0 and e1 == E[1] and bias(frames[1], box[1]) == E[1]
    np.testing.assert_array_equal(f1, F[1])
    # an empty ledger pushes nobody
    empty, _ = potential(HillsLedger(3, sigma=0.3, engine=engine))
    e0, f0 = empty.energy_and_forces(frames, box[:3])
    assert not e0.any() and not f0.any()


def test_cv_bias_deposit_and_reproject(engine, chain):
    g, rec, param, tol, xyz, box, potential = chain
    led = HillsLedger(3, sigma=0.3, height=0.5, kernel="gaussian", capacity=2, engine=engine)
    bias, net = potential(led)
    e_before, _ = bias.energy_and_forces(xyz[0], box[0])
    assert e_before == 0.0
    for k in range(4):                                   # past the capacity of 2: ledger and kept features grow
        assert bias.deposit(xyz[k], box[k], time=0.5 * k) == k
    cvs = bias.compute_cvs(xyz[:4], box[:4])
    np.testing.assert_array_equal(led.centers, cvs)                  # the CVs went to the ledger on the device
    np.testing.assert_array_equal(led.heights, np.full(4, 0.5))
    np.testing.assert_array_equal(led.times, [0.0, 0.5, 1.0, 1.5])
    # the second call sees the hills: at a hill's own centre its term is h exactly (dp = 0), the others add
    e_after, f_after = bias.energy_and_forces(xyz[0], box[0])
    ref = R.bias(cvs[:1], led.packed(), dtype=np.longdouble)
    assert e_after >= 0.5 and abs(e_after - float(ref["bias"][0])) <= R.bound_factor(3, [4])[0] * float(ref["mag"][0])
    assert np.isfinite(f_after).all()
    with pytest.raises(ValueError, match="one frame"):
        bias.deposit(xyz[:2], box[:2])
    # another network (same inputs, same number of CVs): every centre becomes its output at the kept features
    _other, net2 = potential(HillsLedger(3, sigma=0.3, engine=engine), "ln_gelu")
    ms2 = MLPSpec(net2["widths"], net2["activation"], net2["ln_in"], net2["ln_hidden"], net2["head_activation"],
                  net2["params"], net2["mean"], net2["scale"])
    assert bias.reproject_to(ms2) is bias
    cvs2 = bias.compute_cvs(xyz[:4], box[:4])
    assert np.max(np.abs(cvs2 - cvs)) > 1e-3
    np.testing.assert_array_equal(led.centers, cvs2)
    np.testing.assert_array_equal(led.heights, np.full(4, 0.5))
    e2, _ = bias.energy_and_forces(xyz[0], box[0])
    ref2 = R.bias(cvs2[:1], led.packed(), dtype=np.longdouble)
    assert abs(e2 - float(ref2["bias"][0])) <= R.bound_factor(3, [4])[0] * float(ref2["mag"][0])
    # hills this potential did not deposit have no features to re-evaluate; a refused deposit leaves the ledger alone
    led.add_hill([0.0, 0.0, 0.0])
    with pytest.raises(RuntimeError, match="unknown"):
        bias.reproject_to(ms2)
    with pytest.raises(RuntimeError, match="unknown"):
        bias.deposit(xyz[4], box[4])
    assert len(led) == 5
    bias.feature_count += 1                              # an extractor that does not fit the scaler is named at once
    with pytest.raises(RuntimeError, match="feature extractor returned 23 features but scaler expects 24"):
        bias.energy_and_forces(xyz[0], box[0])
    bias.feature_count -= 1
    with pytest.raises(ValueError, match="CVs"):
        potential(HillsLedger(2, sigma=0.3, engine=engine))
    with pytest.raises(TypeError):
        MetadynamicsCVBias(ms2, g[f"{CASE}_mean"], g[f"{CASE}_scale"], "ledger", feature_extractor=bias.feature_extractor,
                           feature_spec_hash="0")
