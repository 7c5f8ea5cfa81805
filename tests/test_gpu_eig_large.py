"""Orders 257 .. 2048 of msm_eigh, msm_tica_solve and msm_onesided_tica_eigenvalues (the device-wide block Jacobi of
pmarlo_amd/csrc/eig_large.h), the wide passes around them, and the reductions end to end at F = 300.

Inputs and bounds are those of tests/_eig_ref.py, taken unchanged (tests/_eig_large_ref.py lists the cases;
tests/test_eig_large_reference.py proves numpy meets each with a tenth to spare).  Every solve runs twice and must
repeat bit for bit.  Before the dispatch on the order existed, every test from msm_eigh at 257 down to the end-to-end
calls failed with "need 1 <= F <= 256"."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import npport
from pmarlo_amd import _lib
from tests import _cov_ref as cr
from tests import _eig_large_ref as lr
from tests import _eig_ref as er
from tests import _gen
from tests import _moments_ref as mr

pytestmark = pytest.mark.gpu

LD = np.longdouble


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ---- msm_eigh ---------------------------------------------------------------------------------------------------------
def _eigh(engine, case, want_vectors=True):
    w, v, sweeps = engine.eigh(engine.to_device(case["A_in"]), want_vectors=want_vectors)
    return w.to_host(), (v.to_host() if v is not None else None), int(sweeps.to_host()[0])


def _eigh_checked(engine, case):
    assert lr.dispatch(case["n"]) == "block_jacobi"
    w, v, sweeps = _eigh(engine, case)
    fig = er.check_eigh(w, v, case)
    print(case["name"], lr.layout(case["n"]), "sweeps", sweeps, fig, "tol", case["tol"])
    assert 0 <= sweeps < lr.SWEEP_CAP          # the cap itself says the iteration ran out
    w2, v2, sweeps2 = _eigh(engine, case)
    assert _same((w, v), (w2, v2)) and sweeps2 == sweeps, "two calls on the same input differ"
    return w, v, sweeps


@pytest.mark.parametrize("n", lr.SEPARATED_N)
def test_eigh_separated_around_the_block_multiples(engine, n):
    """First order above the old cap (257: nine blocks, the last one a single row), 258, one below / at / one above
    nine whole blocks (287, 288, 289: odd and even block counts), ten whole blocks (320) and sixteen (512)."""
    w, v, sweeps = _eigh_checked(engine, lr.separated_case(n))
    assert sweeps <= 14                         # what test_eigh_every_path allows a well-separated spectrum


@pytest.mark.parametrize("case", lr.n300_cases(), ids=lambda c: c["name"])
def test_eigh_300_spectra(engine, case):
    """n = 300 (nine whole blocks and twelve rows): a triple eigenvalue, a cluster 1e-10 apart, fourteen decades,
    2^+-200, an input that is not symmetric, the zero matrix, the identity, a diagonal matrix holding an eigenvalue 0
    (padding is dropped by index) and a block-diagonal matrix whose blocks are the solver's (every rotation between
    blocks is skipped)."""
    w, v, sweeps = _eigh_checked(engine, case)
    if case["name"] in ("zero-300", "identity-300", "diagonal-300"):
        assert sweeps == 0 and np.array_equal(w, case["w"])
    if case["name"] == "blockdiag-300":
        assert sweeps == 1
        for j in range(case["n"]):               # no rotation ever mixed two blocks: exact zeros outside one block
            nz = np.nonzero(v[:, j])[0] // lr.B
            assert nz.min() == nz.max(), (j, nz.min(), nz.max())
    w3, v3, sweeps3 = _eigh(engine, case, want_vectors=False)       # d_v = NULL
    assert v3 is None and w3.tobytes() == w.tobytes() and sweeps3 == sweeps


def test_eigh_without_vectors_at_257(engine):
    case = lr.separated_case(257)
    w, _, sweeps = _eigh(engine, case)
    w3, v3, sweeps3 = _eigh(engine, case, want_vectors=False)
    assert v3 is None and w3.tobytes() == w.tobytes() and sweeps3 == sweeps
    er.check_eigh(w3, None, case)


def test_eigh_at_the_cap(engine):
    """n = 2048, three Householder reflectors on a known diagonal; bound n eps |w|_inf + the construction's own
    rounding (tests/_eig_large_ref.cap_case), orthogonality 1e-12 and residual 1e-11 |w|_inf as everywhere."""
    case = lr.cap_case()
    w, v, sweeps = _eigh(engine, case)
    fig = er.check_eigh(w, v, case)
    print(case["name"], "sweeps", sweeps, fig, "tol", case["tol"], "construction", case["construction"])
    assert 0 < sweeps < lr.SWEEP_CAP


def test_eigh_above_the_cap_is_unsupported(engine):
    with pytest.raises(NotImplementedError, match="2049.*2048"):
        engine.eigh(engine.zeros((2049, 2049), np.float64))
    mom = engine.zeros((2 * 2049 * 2049 + 2 * 2049 + 1,), np.float64)
    with pytest.raises(NotImplementedError, match="2049.*2048"):
        engine.tica_solve(mom, 2049)
    with pytest.raises(NotImplementedError, match="2049.*2048"):
        engine.onesided_tica_eigenvalues(mom, 2049)


# ---- msm_tica_solve ---------------------------------------------------------------------------------------------------
def _tica(engine, case, n_lead=0):
    F = case["F"]
    sc = None if case["scale"] is None else engine.to_device(case["scale"])
    eig, W, mean, rank = engine.tica_solve(engine.to_device(case["moments"]), F, scale=sc, epsilon=case["epsilon"],
                                           kinetic_map=case["kinetic_map"], n_lead=n_lead)
    return eig.to_host(), W.to_host(), mean.to_host(), int(rank.to_host()[0])


def _tica_checked(engine, case):
    assert lr.dispatch(case["F"]) == "block_jacobi"
    out = _tica(engine, case)
    fig = er.check_tica(out, case)
    print(case["name"], fig, "tol", case["tol"])
    assert _same(out, _tica(engine, case)), (case["name"], "second solve differs")
    return out


@pytest.mark.parametrize("F", lr.FULL_F)
def test_tica_full_rank(engine, F):
    """Full-rank C00 with a mean of up to three standard deviations and a per-feature scale: 257, 320 (ten whole
    blocks), 384."""
    case = lr.tica_full_case(F)
    assert case["rank"] == F
    _tica_checked(engine, case)


@pytest.mark.parametrize("F,r", lr.DEFICIENT)
def test_tica_rank_deficient(engine, F, r):
    """(320, 200): the second eigensolve works on the leading 200 x 200 part, block pairs past it are skipped and the
    seventh block is cut by the rank; (300, 256): the rank sits on a block boundary."""
    case = lr.tica_deficient_case(F, r)
    assert case["rank"] == r
    _tica_checked(engine, case)


@pytest.mark.parametrize("which", ["cut", "indefinite", "raw", "T-zero"])
def test_tica_300_variants(engine, which):
    """F = 300: the last C00 direction below epsilon (cut), at -1e-3 (epsilon is raised to -s_min + 1e-16), the
    kinetic map off, and T = 0 (rank 0, zeros, zero mean)."""
    case = lr.tica_300_cases()[which]
    out = _tica_checked(engine, case)
    if which == "indefinite":
        ref = er.numpy_tica(case)
        assert out[3] == ref["rank"] == 299
        np.testing.assert_allclose(out[0], ref["eig"], rtol=0, atol=1.1 * case["tol"])
    if which == "T-zero":
        assert out[3] == 0 and not out[0].any() and not out[1].any() and not out[2].any()


def test_tica_n_lead_is_the_full_solve_truncated(engine):
    case = lr.tica_full_case(320)
    full = _tica(engine, case)
    lead = _tica(engine, case, n_lead=10)
    assert lead[0][:10].tobytes() == full[0][:10].tobytes() and lead[1][:, :10].tobytes() == np.ascontiguousarray(full[1][:, :10]).tobytes()
    assert not lead[0][10:].any() and not lead[1][:, 10:].any()
    assert lead[2].tobytes() == full[2].tobytes() and lead[3] == full[3] == 320


# ---- msm_onesided_tica_eigenvalues ------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", lr.ONESIDED_F)
def test_onesided_estimator(engine, F):
    from pmarlo_amd.features.deeptica.core import trainer_api

    case = er.onesided_case(F)
    idx = case["idx"]
    ev = trainer_api.estimate_top_eigenvalues(case["X"], idx, idx + case["lag"], F, engine=engine)
    print(case["name"], er.check_onesided(ev, case))
    ev2 = trainer_api.estimate_top_eigenvalues(case["X"], idx, idx + case["lag"], F, engine=engine)
    assert ev2.tobytes() == ev.tobytes()


# ---- the passes around the solve, as wide as the solve now goes -------------------------------------------------------
GUARD, OUT_FILL = 64, -1234.5625
ENTRY = {"plain": "msm_lagged_moments", "symmetric": "msm_lagged_moments_reversible",
         "onesided": "msm_lagged_moments_onesided"}


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("F", [257, 320, 321])
def test_lagged_moments_five_and_six_feature_blocks(engine, F, dtype, aligned):
    """The 64 x 64 block-task kernel at n_fb = 5 (257, 320) and 6 (321), all three flavours, with and without
    assume_finite, compared exactly (integer data: any summation order gives the same bits) the way
    tests/test_gpu_cov_paths.py compares: wide buffer whose pad columns and out-of-segment frames hold 2^100, guard
    bands around the output."""
    n, lag, segs = 190, 2 if dtype == "f32" else 3, cr._SEGS_BLK
    ld = F if aligned else F + 2
    off = 0 if aligned else 1
    X, shift = (cr.wide if dtype == "f32" else cr.small)(n, F, 5000 + F)
    host = np.full(off + n * ld, cr.SENTINEL, cr.NP_DTYPE[dtype])
    frames = host[off:].reshape(n, ld)
    for a, b in cr.clip_segments(n, segs):
        if b > a:
            frames[a:b, :F] = X[a:b]
    buf = engine.to_device(host)
    shift_d = engine.to_device(shift)
    starts = np.ascontiguousarray([a for a, _ in segs], np.int64)
    stops = np.ascontiguousarray([b for _, b in segs], np.int64)
    size = 2 * F * F + 2 * F + 1
    for flavour in cr.FLAVOURS:
        ref = cr.exact_moments(X, segs, lag, shift, flavour)
        for finite in (0, 1):
            tag = f"F{F}-{dtype}-{flavour}-finite{finite}"
            blk = engine.to_device(np.full(GUARD + size + GUARD, OUT_FILL))
            st = getattr(_lib.lib, ENTRY[flavour])(engine.handle, buf.ptr + off * host.itemsize,
                                                   _lib.MSM_F32 if dtype == "f32" else _lib.MSM_F64, n, F, ld,
                                                   starts.ctypes.data, stops.ctypes.data, len(segs), lag, shift_d.ptr,
                                                   finite, blk.ptr + GUARD * 8)
            assert st == _lib.MSM_OK, (tag, _lib.lib.msm_last_error(engine.handle))
            out = blk.to_host()
            np.testing.assert_array_equal(out[:GUARD], OUT_FILL, err_msg=f"{tag}: written below the output")
            np.testing.assert_array_equal(out[GUARD + size:], OUT_FILL, err_msg=f"{tag}: written past the output")
            out = out[GUARD:GUARD + size]
            assert not np.any(out == OUT_FILL), tag
            np.testing.assert_array_equal(out[:F * F].reshape(F, F), ref["M00"], err_msg=f"{tag} M00")
            np.testing.assert_array_equal(out[F * F:2 * F * F].reshape(F, F), ref["M0t"], err_msg=f"{tag} M0t")
            np.testing.assert_array_equal(out[2 * F * F:2 * F * F + F], ref["sx"], err_msg=f"{tag} sx")
            np.testing.assert_array_equal(out[2 * F * F + F:2 * F * F + 2 * F], ref["sy"], err_msg=f"{tag} sy")
            assert out[-1] == ref["T"], tag


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("F,kernel", [(300, "mfma_scalar"), (400, "generic")])
def test_project_on_both_sides_of_the_lds_switch(engine, F, kernel, dtype):
    """d = 4: at F = 300 the padded W image fits the default 48 KiB of LDS (matrix-core kernel), at F = 400 it does not
    (generic kernel).  Bound of test_project_rounding_is_within_the_dot_product_bound:
        |Y - Y_ref| <= (F + 4) 2^-53 (sum_f |x_f - mu_f| |inv_sigma_f W_fc| + sum_f |m2_f W_fc|)."""
    n, d = 333, 4
    assert mr.project_path(n, F, d, dtype, F, 0, False, engine.info()["n_cu"], 8)["kernel"] == kernel
    rng = np.random.default_rng(F * d)
    X = (1e6 + rng.standard_normal((n, F))).astype(mr.NP_DTYPE[dtype])
    mu = 1e6 + 0.1 * rng.standard_normal(F)
    isg, m2 = rng.uniform(0.5, 2.0, F), 0.01 * rng.standard_normal(F)
    W = rng.standard_normal((F, d))
    Xl = X.astype(np.float64).astype(LD)
    ref = ((Xl - mu.astype(LD)) * isg.astype(LD) - m2.astype(LD)) @ W.astype(LD)
    weight = np.abs(Xl - mu.astype(LD)) @ np.abs(isg[:, None].astype(LD) * W.astype(LD)) \
        + (np.abs(m2)[:, None].astype(LD) * np.abs(W).astype(LD)).sum(axis=0)[None, :]
    bound = (F + 4) * LD(2.0) ** -53 * weight
    for finite in (False, True):
        Y = engine.project(engine.to_device(X), engine.to_device(mu), engine.to_device(isg), engine.to_device(W), d,
                           mean2=engine.to_device(m2), assume_finite=finite).to_host()
        err = np.abs(Y.astype(LD) - ref)
        print(f"project F={F} {dtype} finite={finite}: worst error / bound = {float((err / bound).max()):.3f}")
        assert Y.shape == (n, d) and np.all(err <= bound)


# ---- end to end -------------------------------------------------------------------------------------------------------
N_E2E, F_E2E = 3000, 300


@pytest.fixture(scope="module")
def wide_series():
    X = _gen.correlated_series(N_E2E, F_E2E, seed=N_E2E + F_E2E).astype(np.float64)
    X *= np.linspace(0.5, 3.0, F_E2E)[None, :]
    clean = X.copy()
    X[::97, 1] = np.nan                                         # imputed to the column mean by _preprocess
    X.setflags(write=False)
    clean.setflags(write=False)
    return X, clean


def _allclose_up_to_sign(got, want, rel):
    assert got.shape == want.shape
    for c in range(want.shape[1]):
        s = np.sign(np.dot(got[:, c], want[:, c])) or 1.0
        np.testing.assert_allclose(s * got[:, c], want[:, c], rtol=0, atol=rel * np.abs(want).max(), err_msg=f"column {c}")


def test_tica_reduce_at_300_features(engine, wide_series):
    from pmarlo_amd.markov_state_model import reduce_features, tica_reduce

    X, _ = wide_series
    got = tica_reduce(X, lag=5, n_components=4)
    want = npport.tica_reduce(X, lag=5, n_components=4)
    assert got.shape == (N_E2E, 4) and got.dtype == np.float64
    _allclose_up_to_sign(got, want, 1e-8)
    np.testing.assert_array_equal(reduce_features(X, method="tica", n_components=4, lag=5), got)


def test_pca_reduce_at_300_features(engine, wide_series):
    from sklearn.decomposition import IncrementalPCA

    from pmarlo_amd.markov_state_model import pca_reduce

    X, _ = wide_series
    got = pca_reduce(X, n_components=4)
    want = npport.pca_reduce(X, 4)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * np.abs(want).max())
    # batch_size: the reference switches to IncrementalPCA, which is what test_gpu_api.py compares against (2e-7)
    got = pca_reduce(X, n_components=4, batch_size=500)
    want = IncrementalPCA(n_components=4, batch_size=500).fit_transform(npport.preprocess(X, scale=True).copy())
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-7 * np.abs(want).max())


def test_vamp_reduce_at_300_features(engine, wide_series):
    from pmarlo_amd.markov_state_model import vamp_reduce

    X, _ = wide_series
    got = vamp_reduce(X, lag=5, n_components=4)
    want, _ = npport.vamp_reduce(X, lag=5, n_components=4)
    assert got.shape == want.shape == (N_E2E, 4)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-8 * np.abs(want).max())


def test_tica_on_three_trajectories_at_300_features(engine, wide_series):
    from pmarlo_amd.markov_state_model.reduction import tica_fit_transform_trajectories

    _, X = wide_series
    lens, lag = [1000, 1000, 1000], 5
    Y, model = tica_fit_transform_trajectories(X, lens, n_components_hint=4, lag=lag)
    assert Y.shape == (N_E2E - 3 * lag, 4)
    Xs = [X[1000 * i:1000 * (i + 1)] for i in range(3)]
    ref = npport.tica_fit(Xs, lag, dim=4)
    np.testing.assert_allclose(model.eigenvalues.to_host()[:4], ref["eigenvalues"][:4], rtol=1e-8)
    want = np.vstack([npport.tica_transform(ref, x)[:-lag] for x in Xs])
    _allclose_up_to_sign(Y, want, 1e-8)
