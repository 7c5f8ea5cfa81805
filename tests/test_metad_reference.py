"""The metadynamics law (tests/_metad_ref.py) against what it restates, and the readers of PLUMED's files.  CPU only.

The golden run (tests/golden/metad/HILLS and COLVAR, PLUMED's recorded output, copied unchanged) is a METAD on the
two components of a distance: 2 CVs, SIGMA = 0.1 for both, HEIGHT = 0.5, one hill every 500 steps of 0.001 (50 hills,
PACE = 500), no tempering (`biasf -1`), the bias served from a grid over [-1.5, 1.5] x [-0.5, 2.5], COLVAR printed
every 10 steps with 6 decimals (2501 rows).  That is all the test needs of the run's input files.

Measured here: the numpy hills sum is 1.003e-3 away from PLUMED's metad.bias column at the worst of the 2501 rows --
PLUMED's grid interpolation plus its 6-decimal printing of CVs and bias.  The test allows 2e-3, twice that.  The three
wrong readings miss by far more (plain Gaussian 3.6e-2; a frame at a hill's time seeing that hill 0.50; both 0.53),
asserted as more than ten times the tolerance: the golden file discriminates."""

from __future__ import annotations

import numpy as np
import pytest

from pmarlo_amd.reweight import metadynamics as M
from tests import _metad_ref as R
from tests.conftest import GOLDEN

HILLS, COLVAR = GOLDEN / "metad" / "HILLS", GOLDEN / "metad" / "COLVAR"
PLUMED_TOL = 2.0e-3


@pytest.fixture(scope="module")
def run():
    led = M.read_hills(HILLS)
    col = M.read_colvar(COLVAR)
    return led, col, np.stack([col["cv.x"], col["cv.y"]], axis=1)


# ------------------------------------------------------------------------------------------------------ the readers
def test_read_hills_golden(run):
    led, col, cv = run
    assert len(led) == 50 and led.n_cv == 2 and led.names == ["cv.x", "cv.y"]
    assert led.kernel == "stretched-gaussian" and led.bias_factor is None
    np.testing.assert_array_equal(led.periods, [0.0, 0.0])
    np.testing.assert_array_equal(led.times, 0.5 * np.arange(1, 51))
    np.testing.assert_array_equal(led.sigmas, np.full((50, 2), 0.1))
    np.testing.assert_array_equal(led.heights, np.full(50, 0.5))
    assert led.centers[0, 0] == -0.5350629399960102 and led.centers[-1, 1] == 1.066135669808446
    np.testing.assert_array_equal(led.packed(), R.pack(led.centers, led.sigmas, led.heights))
    assert sorted(col) == ["cv.x", "cv.y", "ff", "metad.bias", "time"] and cv.shape == (2501, 2)
    assert col["time"][-1] == 25.0 and col["metad.bias"][-1] == 1.422105


def _write(tmp_path, text):
    p = tmp_path / "HILLS"
    p.write_text(text)
    return p


def test_round_trip_and_well_tempered_heights(tmp_path):
    rng = np.random.default_rng(5)
    t, c, s = np.arange(1.0, 7.0), rng.normal(size=(6, 2)), rng.uniform(0.05, 0.4, size=(6, 2))
    h, gamma = rng.uniform(0.1, 1.2, size=6), 8.0
    lines = ["#! FIELDS time phi d sigma_phi sigma_d height biasf", "#! SET multivariate false",
             "#! SET kerneltype gaussian", "#! SET min_phi -pi", "#! SET max_phi pi"]
    for i in range(6):
        stored = h[i] * gamma / (gamma - 1.0)       # what PLUMED writes for a tempered run
        lines.append(" ".join(repr(float(v)) for v in (t[i], *c[i], *s[i], stored, gamma)))
    led = M.read_hills(_write(tmp_path, "\n".join(lines) + "\n"))
    assert led.kernel == "gaussian" and led.bias_factor == gamma and led.names == ["phi", "d"]
    np.testing.assert_array_equal(led.periods, [np.pi - -np.pi, 0.0])
    np.testing.assert_array_equal(led.times, t)
    np.testing.assert_array_equal(led.centers, c)
    np.testing.assert_array_equal(led.sigmas, s)
    # heights as applied: the stored value x (gamma - 1) / gamma, one rounding away from h
    np.testing.assert_array_equal(led.heights, (h * gamma / (gamma - 1.0)) * ((gamma - 1.0) / gamma))
    np.testing.assert_allclose(led.heights, h, rtol=4 * R.EPS)
    # biasf <= 1 means no tempering: heights as stored
    plain = M.read_hills(_write(tmp_path, "#! FIELDS time x sigma_x height biasf\n 1 0.5 0.1 0.7 1\n"))
    assert plain.bias_factor is None and plain.heights[0] == 0.7 and plain.kernel == "gaussian" and plain.n_cv == 1


@pytest.mark.parametrize("text, what", [
    ("#! FIELDS time x sigma_x height biasf\n#! SET multivariate true\n 1 0.5 0.1 0.7 1\n", "multivariate"),
    ("#! FIELDS time x y sigma_x height biasf\n 1 0.5 0.1 0.7 1 1\n", "pair per CV"),
    ("#! FIELDS time x sigma_y height biasf\n 1 0.5 0.1 0.7 1\n", "sigma columns"),
    ("#! FIELDS time x sigma_x height biasf\n#! SET kerneltype triangular\n 1 0.5 0.1 0.7 1\n", "kerneltype"),
    ("#! FIELDS time x sigma_x height biasf\n#! SET min_x -pi\n 1 0.5 0.1 0.7 1\n", "only one of"),
    ("#! FIELDS time x sigma_x height biasf\n 1 0.5 0.1 0.7\n", "columns"),
    (" 1 0.5 0.1 0.7 1\n", "FIELDS"),
    ("#! FIELDS time x sigma_x height biasf\n 1 0.5 0.1 0.7 8\n 2 0.5 0.1 0.7 9\n", "biasf changes"),
    ("#! FIELDS time x sigma_x height biasf\n 2 0.5 0.1 0.7 1\n 1 0.5 0.1 0.7 1\n", "must not decrease"),
])
def test_read_hills_refusals(tmp_path, text, what):
    with pytest.raises(ValueError, match=what):
        M.read_hills(_write(tmp_path, text))


def test_ledger_host_side(run):
    led = run[0]
    # a frame at exactly a hill's time does not see that hill
    np.testing.assert_array_equal(led.counts([0.0, 0.5, 0.50001, 24.99, 25.0, 25.01]), [0, 0, 1, 49, 49, 50])
    np.testing.assert_array_equal(led.counts(led.times), np.arange(50))
    new = M.HillsLedger(2, sigma=0.1, height=0.5, capacity=2)
    for k in range(5):                                                  # grows past its capacity on the host
        assert new.add_hill([0.1 * k, -0.2 * k]) == k
    np.testing.assert_array_equal(new.times, np.arange(5.0))
    np.testing.assert_array_equal(new.centers[:, 0], 0.1 * np.arange(5))
    assert new.capacity >= 5 and len(new) == 5
    lo, step, bins = led.grid([-1.5, -0.5], [1.5, 2.5], [31, 16])
    np.testing.assert_array_equal(step, [3.0 / 30, 3.0 / 15])
    per = M.HillsLedger(1, periods=[2 * np.pi])
    np.testing.assert_array_equal(per.grid(-np.pi, np.pi, 8)[1], [2 * np.pi / 8])
    for bad in (dict(n_cv=0), dict(n_cv=9), dict(n_cv=1, kernel="box"), dict(n_cv=1, bias_factor=1.0),
                dict(n_cv=1, kT=0.0), dict(n_cv=2, periods=[1.0]), dict(n_cv=1, cut=0.0)):
        with pytest.raises(ValueError):
            M.HillsLedger(**bad)
    with pytest.raises(ValueError, match="sigma"):
        M.HillsLedger(1, height=1.0).add_hill([0.0])
    with pytest.raises(ValueError, match="height"):
        M.HillsLedger(1, sigma=0.1).add_hill([0.0])
    with pytest.raises(ValueError, match="before the last"):
        new.add_hill([0.0, 0.0], time=1.0)
    with pytest.raises(ValueError, match="exactly one"):
        M.MetadynamicsReweighter()
    with pytest.raises(ValueError, match="grid"):
        M.MetadynamicsReweighter(kT=1.0, ledger=led)
    with pytest.raises(ValueError, match="method"):
        M.MetadynamicsReweighter(kT=1.0, ledger=led, method="bonomi")
    assert M.MetadynamicsReweighter(temperature_K=300.0, ledger=led, method="final").kT == pytest.approx(2.494338785)


# ------------------------------------------------------------------------------------------------- against PLUMED
def test_hills_sum_against_plumed(run):
    led, col, cv = run
    packed = led.packed()
    seen = R.counts_from_times(led.times, col["time"])
    later = np.searchsorted(led.times, col["time"], side="right")          # WRONG: sees the hill of its own time
    dev = {}
    for name, kernel, counts in (("law", "stretched-gaussian", seen), ("plain Gaussian", "gaussian", seen),
                                 ("<= instead of <", "stretched-gaussian", later), ("both", "gaussian", later)):
        dev[name] = float(np.max(np.abs(R.bias(cv, packed, counts, kernel=kernel)["bias"] - col["metad.bias"])))
        print(f"{name}: max |numpy - PLUMED| over {cv.shape[0]} rows = {dev[name]:.4e}")
    assert dev["law"] <= PLUMED_TOL
    for name in ("plain Gaussian", "<= instead of <", "both"):
        assert dev[name] > 10 * PLUMED_TOL, name


# ----------------------------------------------------------------------------------------------- rounding of the law
def test_fp64_against_longdouble(run):
    led, col, cv = run
    packed = led.packed()
    seen = R.counts_from_times(led.times, col["time"])
    for kernel in R.KERNELS:
        f64 = R.bias(cv, packed, seen, kernel=kernel)
        f80 = R.bias(cv, packed, seen, kernel=kernel, dtype=np.longdouble)
        for q, m in (("bias", "mag"), ("grad", "gmag")):
            err = np.abs(f64[q] - f80[q]).astype(np.float64)
            scale = f80[m].astype(np.float64)
            factor = R.bound_factor(2, seen) if q == "bias" else R.bound_factor(2, seen)[:, None]
            assert (err <= factor * scale).all(), (kernel, q)
            assert not err[scale == 0].any()
            ratio = float((err[scale > 0] / scale[scale > 0]).max() / R.EPS)
            print(f"{kernel} {q}: largest |fp64 - longdouble| = {ratio:.1f} eps x sum of magnitudes")


def test_periodic_and_per_hill_sigma_terms():
    """The wrap at the seam and at exactly +-P/2 (rint rounds half to even), per-hill sigmas, cutoff on both sides."""
    P = 2.0
    packed = R.pack([[0.9], [-0.9], [0.0]], [[0.3], [0.2], [0.25]], [1.0, 2.0, 0.5])
    cv = np.array([[-0.95], [0.85], [1.0], [-1.0], [-0.1]])
    term, dterm, _m, _g = R.hill_terms(cv, packed, periods=[P], kernel="gaussian")
    dp = np.array([0.15, 0.05, 0.1, 0.1])                  # hill 0 seen from -0.95 (wrapped), 0.85, 1.0, -1.0 (wrapped)
    np.testing.assert_allclose(term[:4, 0], np.exp(-0.5 * (dp / 0.3) ** 2), rtol=1e-13)
    assert dterm[0, 0, 0] < 0 < dterm[1, 0, 0]             # -0.95 lies to the right of 0.9 through the seam
    # exactly half a period away: rint(+-0.5) = +-0 keeps dp = +-P/2
    z = (-0.1 - 0.9) * (1.0 / 0.3)
    assert term[4, 0] == np.exp(-(0.5 * (z * z))) and dterm[4, 0, 0] > 0
    assert term[2, 2] == 0.0 and term[3, 2] == 0.0         # 1 / 0.25 = 4 sigma away: outside the cutoff
    q = 0.5 * (np.array([0.1]) / 0.25) ** 2
    assert R.hill_terms(np.array([[0.1]]), packed[2:], kernel="stretched-gaussian")[0][0, 0] == \
        0.5 * (R.constants("stretched-gaussian")[0] * np.exp(-q[0]) + R.constants("stretched-gaussian")[1])
    # the stretched kernel reaches 0 at the cutoff, the plain one jumps by h exp(-cut)
    edge = np.array([[np.sqrt(2 * R.CUT) * 0.25 * (1 - 1e-9)]])
    assert 0 <= R.hill_terms(edge, packed[2:], kernel="stretched-gaussian")[0][0, 0] < 1e-10
    assert R.hill_terms(edge, packed[2:], kernel="gaussian")[0][0, 0] == pytest.approx(0.5 * np.exp(-R.CUT), rel=1e-6)


# ------------------------------------------------------------------------------------------------------------- c(t)
@pytest.mark.parametrize("bias_factor", [None, 6.0])
def test_ct_reference_against_brute_force(run, bias_factor):
    led = run[0]
    packed, kT = led.packed()[:20], 2.5
    lo, step, bins = R.grid_spec([-1.5, -0.5], [1.5, 2.5], [41, 37])
    a1, a2 = R.exponents(kT, bias_factor)
    ck = R.checkpoints(20, 3)
    np.testing.assert_array_equal(ck, [0, 3, 6, 9, 12, 15, 18])
    L, VH, bound_v = R.scan(packed, lo, step, bins, ck, a1, a2, kernel=led.kernel)
    G = int(np.prod(bins))
    assert L[0, 0] == L[0, 1] == np.log(G)                               # c_0 = 0 exactly
    for j, k in enumerate(ck):
        for e, a in enumerate((a1, a2)):
            want = R.lse_brute(packed, lo, step, bins, k, a, kernel=led.kernel)
            # a rounding of V moves a V by a bound_V; the LSE of G terms adds log2 G + 6 roundings
            tol = a * bound_v[j] + (np.log2(G) + 6) * R.EPS * max(1.0, abs(float(want)))
            assert abs(float(L[j, e] - want)) <= tol, (j, e)
    np.testing.assert_array_equal(VH, R.bias(R.grid_points(lo, step, bins), packed, kernel=led.kernel)["bias"])
    # the weights' reference: c grows, and a frame uses the latest evaluated c
    logw, c, V = R.tiwary_log_weights(run[2][:400], np.minimum(R.counts_from_times(led.times, run[1]["time"][:400]), 20),
                                      packed, lo, step, bins, kT, bias_factor, stride=3, kernel=led.kernel)
    assert c[0] == 0.0 and (np.diff(c) > 0).all()
    w, lw, ess = R.normalise(logw)
    assert abs(w.sum() - 1) < 1e-12 and 1 <= ess <= 400
