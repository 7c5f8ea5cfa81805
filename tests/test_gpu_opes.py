"""OPES end to end on the device: OPESLedger, opes_weights, OPESReweighter, read_kernels and OPESCVBias against
tests/_opes_ref.py run in 80-bit floats and, for the DeepTICA chain, tests/_bias_ref.py.

The deposit sequences are the committed ones of tests/_opes_ref.case (T = 300 deposits of a slow random walk, d in
{1, 2, 3, 8}, with and without a periodic axis); tests/test_opes_reference.py asserts that each has a chain of two
merges, a merge across the boundary where periodic, and a relative margin >= 1e-9 on every merge decision and nearest
choice, so the integers of the journal are decided the same way in fp64 and are compared EXACTLY.

Bounds.  The restatement's own error (80-bit against exact) is 2^-11 of fp64's; what remains is the device's rounding,
which accumulates over the merges a kernel has been through and over the T incremental updates of S.  It is measured,
not derived: every test prints the largest error it saw, BOUNDS holds 4 x the largest figure of a run of this file and
tests/test_gpu_opes_paths.py on an MI355X (the factor the metadynamics tests use, to cover another compiler's libm), and
DESIGN.md ("OPES") lists the measured figures.  The measures:
  * centres: |device - restatement| / sigma of the kernel; sigmas, heights, W, Z, neff: relative;
  * V: |device - restatement| / (kT p): V = kT p log(x), so this is the relative error of x = P / Z + epsilon;
  * dV/ds: |device - restatement| / max(|dV/ds|, kT p / sigma0), the scale of a gradient one kernel wide.
  * the DeepTICA chain, stage by stage on the device's own intermediates: CVs against the reference's recorded fp64
    values with the recorded tolerance of tests/test_gpu_bias.py, V and dV/dCV of the live form by the bounds above
    against the restatement evaluated on the device's own journal, the network adjoint and the featurizer adjoint
    with that file's 4 x |float64 - longdouble| gaps.
  * forces against a central difference of the energy at n = 1, in one coordinate at a time with a step h = 2^-9 nm
    (x + h and x - h are formed in float32, the step used is their exact difference).  The difference quotient is off
    by its truncation error, C h^2, and by the noise of the energy.  D(2h) - D(h) = 3 C h^2 + O(h^4), so
    |D(2h) - D(h)| stands in for the truncation error with a factor 3 to spare.  The energy is a function of float32
    features: a feature carries at most 16 float32 roundings (difference, minimum image, squares, sum, root, and the
    trigonometry of an angle), so |dE| <= sum_i |dV/dfeature_i| 16 2^-24 max(1, |feature_i|), and the two energies of
    a quotient contribute 2 |dE| / (2 h) each way: tolerance = |D(2h) - D(h)| + 2 |dE| / h."""

from __future__ import annotations

import json

import numpy as np
import pytest

from pmarlo_amd import _lib
from pmarlo_amd.features.deeptica import MLPSpec, OPESCVBias, feature_spec_sha256
from pmarlo_amd.features.deeptica.ts_feature_extractor import build_feature_extractor_module, canonicalize_feature_spec
from pmarlo_amd.reweight import OPESLedger, OPESReweighter, Reweighter, opes_weights, read_kernels
from tests import _bias_ref as B
from tests import _opes_ref as O
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

# 4 x the largest error observed on an MI355X (see the module docstring; the observed figures are in DESIGN.md)
# observed: center 1.32e-14, sigma 9.94e-16, height 4.36e-16, W 1.52e-15, Z 1.52e-15, neff 2.66e-15, bias 1.53e-14,
# grad 1.76e-14, online 2.04e-14
BOUNDS = {"center": 5.3e-14, "sigma": 4.0e-15, "height": 1.8e-15, "W": 6.1e-15, "Z": 6.1e-15, "neff": 1.1e-14,
          "bias": 6.2e-14, "grad": 7.1e-14, "online": 8.2e-14}

CASES = [(d, periodic) for d in O.DIMS for periodic in (False, True)]
F64 = lambda a: np.asarray(a, np.float64)      # noqa: E731


def device_ledger(engine, par, rec, max_steps: int = 0, **kw) -> OPESLedger:
    d = par.d
    return OPESLedger.from_arrays(np.arange(float(rec.shape[0])), rec[:, :d], rec[:, d:2 * d], rec[:, 2 * d],
                                  rec[:, 2 * d + 1], par.kT, barrier=O.BARRIER, periods=par.periods, sigma0=par.sigma0,
                                  threshold=par.threshold, max_steps=max_steps, engine=engine, **kw)


def relative_v(V, ref, par) -> np.ndarray:
    return np.abs(F64(V) - F64(ref)) / par.kTp


def grad_scale(ref, par) -> np.ndarray:
    return np.maximum(np.abs(F64(ref)), par.kTp / par.sigma0[None, :])


def _rel(got, ref) -> float:
    ref = F64(ref)
    return float((np.abs(F64(got) - ref) / np.abs(ref)).max())


# ------------------------------------------------------------------------------------------------- replay
@pytest.mark.parametrize("d,periodic", CASES)
def test_replay_against_the_restatement(engine, d, periodic):
    x, par, rec, run = O.case(d, periodic)
    led = device_ledger(engine, par, rec)
    T = O.T_DEPOSITS
    J = led.journal()
    assert len(led) == T and led.n_kernels == run.K[-1]
    # the integers, exactly: which version died when, how many kernels lived after every deposit, who lives in which slot
    np.testing.assert_array_equal(J["death"], np.minimum(run.death, T))
    np.testing.assert_array_equal(J["K"], run.K)
    np.testing.assert_array_equal(J["live_version"], run.live_version)
    ref = F64(run.journal)
    err = {"center": float((np.abs(J["kernels"][:, :d] - ref[:, :d]) / ref[:, d:2 * d]).max()),
           "sigma": _rel(J["kernels"][:, d:2 * d], ref[:, d:2 * d]), "height": _rel(J["kernels"][:, 2 * d], ref[:, 2 * d]),
           "W": _rel(J["W"], run.W), "Z": _rel(J["Z"], run.Z), "neff": _rel(J["neff"], run.neff)}
    # the incrementally updated Z against the full double sum over the final live set, and the properties
    zf = float(O.full_z(run, par))
    err["Z"] = max(err["Z"], abs(led.zed - zf) / zf)
    print(f"d={d} periodic={periodic}: K={run.K[-1]} " + " ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for key, value in err.items():
        assert value <= BOUNDS[key], (key, value)
    assert led.zed == J["Z"][-1] and abs(led.neff - float(run.neff[-1])) <= BOUNDS["neff"] * led.neff
    live = led.kernels()
    np.testing.assert_array_equal(live, J["kernels"][J["live_version"]])
    np.testing.assert_array_equal(led.times, np.arange(float(T)))


@pytest.mark.parametrize("n", [1, 257, 1000])
@pytest.mark.parametrize("d,periodic", CASES)
def test_bias_and_gradient_at_the_frames(engine, d, periodic, n):
    x, par, rec, run = O.case(d, periodic)
    led = device_ledger(engine, par, rec)
    cv, times = O.frames(d, periodic, n)
    counts = O.counts_from_times(np.arange(O.T_DEPOSITS), times)
    ref = O.bias(run, par, cv, counts)
    V, g = led.bias(cv, times, gradient=True)
    assert V.shape == (n,) and g.shape == (n, d) and V.dtype == np.float64
    err_v, err_g = relative_v(V, ref["bias"], par).max(), (np.abs(g - F64(ref["grad"])) / grad_scale(ref["grad"], par)).max()
    # the final state, by both forms
    final = O.bias(run, par, cv)
    Vf, gf = led.bias(cv, gradient=True)
    Vw, gw = led.bias(cv, gradient=True, live=True)
    err_f = max(relative_v(Vf, final["bias"], par).max(), relative_v(Vw, final["bias"], par).max())
    err_fg = max((np.abs(a - F64(final["grad"])) / grad_scale(final["grad"], par)).max() for a in (gf, gw))
    print(f"d={d} periodic={periodic} n={n}: V {err_v:.3e} dV {err_g:.3e}; final (journal and wave) V {err_f:.3e} "
          f"dV {err_fg:.3e}; frames outside every kernel: {int((F64(ref['mag']) == 0).sum())}")
    assert max(err_v, err_f) <= BOUNDS["bias"] and max(err_g, err_fg) <= BOUNDS["grad"]
    # a frame exactly at a deposit's time does not see that deposit; one at time 0 sees the empty ledger
    assert counts[0] == 0 and abs(V[0] - par.kTp * np.log(par.eps)) <= 2 * O.EPS * abs(V[0]) and not g[0].any()
    if n > 1:
        assert counts[1] == 17 and counts[2] == O.T_DEPOSITS
        assert V[1] == led.bias(cv[1], counts=[17])[0] != led.bias(cv[1], counts=[18])[0]


def test_online_deposits_against_the_restatement(engine):
    """the on-line rule with shrinking widths (pow, exp, log on the device) against the 80-bit run of the same rule"""
    d = 2
    x, par, online = O.online_case()      # tests/test_opes_reference.py asserts this run's decision margins
    led = OPESLedger(d, par.kT, barrier=O.BARRIER, periods=par.periods, sigma0=par.sigma0, capacity=8, engine=engine)
    made = np.concatenate([led.deposit(x[:150]).to_host(), led.deposit(engine.to_device(x[150:]), max_steps=32).to_host()])
    J = led.journal()
    np.testing.assert_array_equal(J["death"], np.minimum(online.death, O.T_DEPOSITS))
    np.testing.assert_array_equal(J["K"], online.K)
    ref = F64(online.records)
    err = max(_rel(made[:, d:2 * d], ref[:, d:2 * d]), _rel(made[:, 2 * d], ref[:, 2 * d]),
              float(np.abs(made[:, 2 * d + 1] - ref[:, 2 * d + 1]).max()), _rel(J["Z"], online.Z), _rel(J["W"], online.W))
    print(f"on-line deposits: largest error of sigma, height, logweight, Z, W = {err:.3e}")
    assert err <= BOUNDS["online"]
    assert made[-1, d] < 0.6 * made[0, d]           # the widths shrink as neff grows
    assert led.n_kernels == online.K[-1] and len(led) == O.T_DEPOSITS


# ------------------------------------------------------------------------------------------------- edge cases
def test_edges(engine):
    d = 2
    x, par, rec, run = O.case(d, False)
    empty = OPESLedger(d, par.kT, barrier=O.BARRIER, sigma0=par.sigma0, engine=engine)
    v0 = par.kTp * np.log(par.eps)
    for kw in (dict(), dict(live=True), dict(times=[0.0, 1.0, 2.0, 3.0])):
        V, g = empty.bias(x[:4], gradient=True, **kw)
        assert (np.abs(V - v0) <= 2 * O.EPS * abs(v0)).all() and (V == V[0]).all() and not g.any(), kw
    assert empty.n_kernels == 0 and empty.zed == 1.0 and empty.neff == 1.0 and len(empty) == 0
    # a full ledger is a status, not a write past the end: capacity 8, 12 records through the raw engine call
    dev = engine.opes_state(8, d)
    recd = engine.to_device(rec[:12])
    guard = engine.opes_state(8, d)                 # allocated right after: its buffers must stay untouched
    engine.opes_deposit(dev, empty.params(), recd, max_steps=5)
    s = engine.opes_read_state(dev)
    assert s["status"] == _lib.OPES_FULL and s["count"] == 8 and s["cursor"] == 8
    assert not guard["journal"].to_host().any() and not guard["live"].to_host().any()
    eight = device_ledger(engine, par, rec[:8])
    np.testing.assert_array_equal(dev["journal"].to_host(), eight.device_ledger()["journal"].to_host()[:8])
    # an unusable record stops the replay there and says so
    bad = rec[:6].copy()
    bad[3, d] = 0.0                                 # a sigma of 0
    dev2 = engine.opes_state(8, d)
    engine.opes_deposit(dev2, empty.params(), engine.to_device(bad))
    s2 = engine.opes_read_state(dev2)
    assert s2["status"] == _lib.OPES_BAD_RECORD and s2["count"] == 3 and s2["cursor"] == 3
    with pytest.raises(ValueError, match="positive"):
        empty.deposit_records(None, bad[:, :d], bad[:, d:2 * d], bad[:, 2 * d], bad[:, 2 * d + 1])
    # NaN CVs: the frame is NaN in its own outputs and nowhere else, in both forms
    led = device_ledger(engine, par, rec)
    cv, times = O.frames(d, False, 300)
    dirty = cv.copy()
    rows = [0, 5, 63, 64, 130, 299]
    dirty[rows[0], 0], dirty[rows[1], 1], dirty[rows[2], 0] = np.nan, np.inf, -np.inf
    dirty[rows[3]], dirty[rows[4], 1], dirty[rows[5], 0] = np.nan, np.nan, np.inf
    keep = np.setdiff1d(np.arange(300), rows)
    for kw in (dict(times=times), dict(live=True)):
        V, g = led.bias(dirty, gradient=True, **kw)
        cV, cg = led.bias(cv, gradient=True, **kw)
        assert np.isnan(V[rows]).all() and np.isnan(g[rows]).all()
        np.testing.assert_array_equal(V[keep], cV[keep])
        np.testing.assert_array_equal(g[keep], cg[keep])
    assert np.isnan(led.bias(dirty[:1], counts=[0])[0])
    with pytest.raises(ValueError, match="non-finite"):
        opes_weights(led, dirty)
    with pytest.raises(ValueError, match="finite"):
        led.deposit(dirty[0])
    for call in (lambda: led.bias(np.zeros((4, 3))), lambda: led.bias(cv[:4], times=times[:4], counts=[0, 0, 0, 0]),
                 lambda: led.bias(cv[:4], counts=[0, 0, 0]), lambda: led.bias(cv[:2], counts=[0, 301]),
                 lambda: led.bias(cv[:2], live=True, times=times[:2]), lambda: OPESLedger(9, 1.0, barrier=5.0),
                 lambda: OPESLedger(2, 1.0), lambda: OPESLedger(2, 1.0, barrier=0.5),
                 lambda: engine.opes_bias(engine.to_device(cv[:4]), led.device_ledger(), led.params()[:5], 300),
                 lambda: engine.opes_bias(engine.to_device(cv[:4]), led.device_ledger(), led.params(), 301),
                 lambda: engine.opes_bias(engine.to_device(cv[:4]), led.device_ledger(), led.params(), 300,
                                          max_workgroups=-1)):
        with pytest.raises(ValueError):
            call()
    assert led.bias(np.zeros((0, 2))).shape == (0,)


def test_a_refused_online_deposit_leaves_a_usable_ledger(engine):
    """a device CV row that is not finite cannot be seen by the host without waiting: the device refuses it and all after
    it, the bias keeps to the deposits made, the next read of the state says so, and clear_status() recovers"""
    d = 2
    x, par, rec, run = O.case(d, False)
    kw = dict(barrier=O.BARRIER, sigma0=par.sigma0, fixed_sigma=True, capacity=64, engine=engine)
    led, good = OPESLedger(d, par.kT, **kw), OPESLedger(d, par.kT, **kw)
    rows = x[:40].copy()
    rows[25, 1] = np.nan
    led.deposit(engine.to_device(rows))
    led.deposit(engine.to_device(x[40:50]))            # submitted after the refusal: consumed by nobody
    good.deposit(x[:25])
    assert len(led) == 50                              # the host has not looked yet
    cv, _times = O.frames(d, False, 257)
    want = good.bias(cv, gradient=True)
    got = led.bias(engine.to_device(cv), gradient=True)        # T = 50 on the host, 25 on the device
    np.testing.assert_array_equal(got[0].to_host(), want[0])
    np.testing.assert_array_equal(got[1].to_host(), want[1])
    with pytest.raises(ValueError, match="refused a deposit.*holds 25"):
        led.n_kernels
    assert len(led) == 25 and led.state()["status"] == _lib.OPES_BAD_RECORD and led.times.tolist() == list(range(25))
    with pytest.raises(ValueError, match="clear_status"):
        led.journal()
    assert led.clear_status() == 25 and led.state()["status"] == 0
    led.deposit(x[25:50])
    good.deposit(x[25:50])
    assert len(led) == 50 and led.n_kernels == good.n_kernels and led.zed == good.zed
    np.testing.assert_array_equal(led.journal()["kernels"], good.journal()["kernels"])
    np.testing.assert_array_equal(led.times, np.arange(50.0))
    # the raw call: a marked ledger consumes nothing, from record 0 or from the cursor
    dev = engine.opes_state(8, d)
    engine.opes_deposit(dev, led.params(), engine.to_device(rec[:12]))
    assert engine.opes_read_state(dev)["status"] == _lib.OPES_FULL
    before = {k: v.to_host() for k, v in dev.items() if hasattr(v, "to_host")}
    engine.opes_deposit(dev, led.params(), engine.to_device(rec[12:14]))
    for key, value in before.items():
        np.testing.assert_array_equal(dev[key].to_host(), value, err_msg=key)
    assert engine.opes_clear_status(dev)["status"] == 0 and engine.opes_read_state(dev)["count"] == 8


# ------------------------------------------------------------------------------------------------- weights and files
def test_weights_reweighter_and_kernels_file(engine, tmp_path):
    d, periodic = 2, True
    x, par, rec, run = O.case(d, periodic)
    led = device_ledger(engine, par, rec)
    cv, times = O.frames(d, periodic, 257)
    V = led.bias(cv, times)
    res = opes_weights(led, cv, times)
    w, lw, ess = O.normalise(V / par.kT)                        # the host formula on the device's own V
    np.testing.assert_array_equal(res.bias, V)
    np.testing.assert_allclose(res.weights, w, rtol=64 * O.EPS, atol=0)
    np.testing.assert_allclose(res.log_weights, lw, rtol=0, atol=64 * O.EPS * np.abs(lw).max())
    assert abs(res.weights.sum() - 1.0) <= 64 * O.EPS and res.ess == pytest.approx(ess, rel=1e-12)
    weights, log_weights, kish = res
    assert weights is res.weights and log_weights is res.log_weights and kish == res.ess
    static = opes_weights(led, cv, kT=2.0)
    np.testing.assert_allclose(static.weights, O.normalise(led.bias(cv) / 2.0)[0], rtol=64 * O.EPS)
    # the KERNELS file: written as PLUMED writes it, read back into the same ledger
    path = tmp_path / "KERNELS"
    lines = ["#! FIELDS time phi psi sigma_phi sigma_psi height logweight", f"#! SET biasfactor {par.gamma!r}",
             f"#! SET epsilon {par.eps!r}", f"#! SET kernel_cutoff {par.cutoff!r}",
             f"#! SET compression_threshold {par.threshold!r}", "#! SET min_phi -pi", "#! SET max_phi pi"]
    lines += [" ".join(repr(float(v)) for v in [j] + list(rec[j])) for j in range(O.T_DEPOSITS)]
    path.write_text("\n".join(lines) + "\n")
    filed = read_kernels(path, par.kT, engine=engine)
    assert filed.names == ["phi", "psi"] and filed.periods.tolist() == [2 * np.pi, 0.0] and filed.epsilon == par.eps
    assert filed.cutoff == par.cutoff and filed.biasfactor == par.gamma and len(filed) == O.T_DEPOSITS
    np.testing.assert_array_equal(filed.journal()["kernels"], led.journal()["kernels"])
    np.testing.assert_array_equal(filed.bias(cv, times), V)
    with pytest.raises(ValueError, match="FIELDS"):
        read_kernels(GOLDEN / "metad" / "HILLS", 1.0, engine=engine)
    # the reweighter: the layout Reweighter.apply writes
    cut = 130
    data = {"splits": {"a": {"cv": cv[:cut], "time": times[:cut]}, "b": {"cv": cv[cut:], "time": times[cut:], "ledger": path}},
            "frame_weights": {"old": np.ones(3)}}
    rw = OPESReweighter(kT=par.kT, ledger=led)
    out = rw.apply(data)
    assert set(out) == {"a", "b"} and set(data["frame_weights"]) == {"old", "a", "b"}
    assert data["frame_weights"]["a"].shape == (cut,) and data["frame_weights"]["a"].dtype == np.float64
    np.testing.assert_allclose(np.concatenate([out["a"], out["b"]]), res.weights, rtol=1e-13)
    assert abs(out["a"].sum() + out["b"].sum() - 1.0) < 1e-13 and rw.result["ess"] == pytest.approx(res.ess)
    np.testing.assert_array_equal(rw.result["a"]["bias"], V[:cut])
    with pytest.raises(ValueError, match="MBAR"):
        Reweighter(300.0, mode="opes")
    for bad, what in (({}, "splits"), ({"splits": {"a": {"time": [0.0]}}}, "cv"),
                      ({"splits": {"a": {"cv": cv[:4], "time": [0.0, 1.0]}}}, "entries")):
        with pytest.raises(ValueError, match=what):
            rw.apply(bad)
    with pytest.raises(ValueError, match="ledger"):
        OPESReweighter(kT=1.0).apply({"splits": {"a": {"cv": cv[:4]}}})


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
           4.0 * gaps["featurize_vjp_f64_minus_longdouble"], 4.0 * gaps["mlp_vjp_f64_minus_longdouble"])
    mean, scale = g[f"{CASE}_mean"], g[f"{CASE}_scale"]
    net = B.golden_network(NET, mean, scale)
    ms = MLPSpec(net["widths"], net["activation"], net["ln_in"], net["ln_hidden"], net["head_activation"],
                 net["params"], net["mean"], net["scale"])
    # CVs of a tanh head lie in (-1, 1): kernels 0.3 wide, merged where the frames' CVs are close
    led = OPESLedger(3, 1.0, barrier=8.0, sigma0=[0.3, 0.25, 0.35], engine=engine)
    bias = OPESCVBias(ms, mean, scale, led, feature_extractor=build_feature_extractor_module(spec, engine),
                      feature_spec_hash=feature_spec_sha256(raw))
    return g, rec, param, tol, g[f"{CASE}_xyz"], g[f"{CASE}_box"], bias, net


def _assert_adjoint(got, want, scale, gap, what):
    ratio = np.abs(got - want)[scale > 0] / scale[scale > 0]
    print(f"{what}: largest |device - restatement| / sum|terms| = {ratio.max():.3e}, bound {gap:.3e}")
    assert np.isfinite(got).all() and not got[scale == 0].any() and ratio.max() <= gap, what


def test_cv_bias_stage_by_stage(engine, chain):
    g, rec, param, tol, xyz, box, bias, net = chain
    led = bias.ledger
    par = O.Params(3, 1.0, 8.0, sigma0=[0.3, 0.25, 0.35])
    e0, f0 = bias.energy_and_forces(xyz[0], box[0])
    v0 = par.kTp * np.log(par.eps)
    assert abs(e0 - v0) <= 2 * O.EPS * abs(v0) and not f0.any()          # nothing deposited: a constant, no force
    for k in range(3, 8):
        assert bias.deposit(xyz[k], box[k]) == k - 3
    for k in (3, 4):                                                     # twice at the same place: merged at once
        bias.deposit(xyz[k], box[k], time=10.0 + k)
    assert len(led) == 7 and led.n_kernels <= 5 and led.times.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 13.0, 14.0]
    frames = xyz[:3]
    E, F = bias.energy_and_forces(frames, box[:3])
    cv = bias.compute_cvs(frames, box[:3])
    assert E.shape == (3,) and cv.shape == (3, 3) and F.shape == frames.shape and F.dtype == np.float64
    # stage 1: the CVs against the reference's recorded fp64 values, as tests/test_gpu_bias.py holds them
    assert np.max(np.abs(cv - g[f"{CASE}__{NET}__cv64"][:3])) <= tol[0]["cv"]
    res = bias.energy_and_forces_device(engine.to_device(frames), box[:3])
    np.testing.assert_array_equal(res["cv"].to_host(), cv)
    np.testing.assert_array_equal(res["energy"].to_host(), E)
    np.testing.assert_array_equal(res["force"].to_host(), F)
    # the deposits were made at the CVs of their frames, which never left the device
    J = led.journal()
    assert J["K"][-1] == led.n_kernels and J["death"][0] < 7 and J["death"][1] < 7
    # stage 2: V and dV/dCV at those CVs against the restatement on the device's own journal
    ref = O.bias(None, par, cv, journal=J["kernels"], death=np.where(J["death"] >= 7, O.ALIVE, J["death"]), W=J["W"], Z=J["Z"])
    grad = res["cv_grad"].to_host()
    err_v = relative_v(E, ref["bias"], par).max()
    err_g = (np.abs(grad - F64(ref["grad"])) / grad_scale(ref["grad"], par)).max()
    print(f"OPESCVBias: V {err_v:.3e} dV/dCV {err_g:.3e}; P / Z = {F64(ref['mag'])}")
    assert (F64(ref["mag"]) > 0).all() and err_v <= BOUNDS["bias"] and err_g <= BOUNDS["grad"]
    # stage 3: the network's adjoint of that gradient, stage 4: the featurizer's, on the device's own intermediates
    feats = res["features"].to_host()
    _e, _y, gx_ref, gx_scale = B.mlp_vjp(net, feats, grad, 1.0)
    gx = engine.mlp_vjp(res["features"], bias.spec, gout=res["cv_grad"], want_energy=False, want_outputs=False)["gx"]
    _assert_adjoint(gx.to_host(), gx_ref, gx_scale, tol[2], "mlp_vjp of the OPES gradient")
    F_ref, F_scale = B.featurize_vjp(rec, param, frames, gx.to_host(), box[:3], "round", sign=-1.0, width=feats.shape[1])
    _assert_adjoint(F, F_ref, F_scale, tol[1], "forces")
    assert np.abs(F).max() > 0
    # one frame is one MD step: a scalar, (A, 3), the batch's bits
    e1, f1 = bias.energy_and_forces(frames[1], box[1])
    assert np.ndim(e1) == 0 and e1 == E[1] and bias(frames[1], box[1]) == E[1]
    np.testing.assert_array_equal(f1, F[1])
    # forces against a central difference of the energy at n = 1 (the tolerance is derived in the module docstring)
    gxh = gx.to_host()[1]
    dE = float((np.abs(gxh) * 16 * 2.0 ** -24 * np.maximum(1.0, np.abs(feats[1]))).sum())
    atoms = np.argsort(-np.abs(F[1]).sum(axis=1))[:3]
    h = np.float32(2.0 ** -9)

    def quotient(a, c, step):
        plus, minus = frames[1].copy(), frames[1].copy()
        plus[a, c] += step
        minus[a, c] -= step
        width = float(plus[a, c]) - float(minus[a, c])
        return -(float(bias(plus, box[1])) - float(bias(minus, box[1]))) / width

    for a in atoms:
        for c in range(3):
            d1, d2 = quotient(a, c, h), quotient(a, c, np.float32(2) * h)
            tol_fd = abs(d2 - d1) + 2 * dE / float(h)
            print(f"atom {a} axis {c}: force {F[1, a, c]:+.6e}, quotient {d1:+.6e}, off by {abs(d1 - F[1, a, c]):.2e}, "
                  f"tolerance {tol_fd:.2e}")
            assert abs(d1 - F[1, a, c]) <= tol_fd
    with pytest.raises(NotImplementedError):
        bias.reproject_to(bias.cv_model)
    with pytest.raises(ValueError, match="one frame"):
        bias.deposit(xyz[:2], box[:2])
    with pytest.raises(TypeError):
        OPESCVBias(bias.cv_model, g[f"{CASE}_mean"], g[f"{CASE}_scale"], "ledger", feature_extractor=bias.feature_extractor,
                   feature_spec_hash="0")
    assert bias.get_metadata()["bias_type"] == "opes" and bias.get_metadata()["n_deposits"] == 7
