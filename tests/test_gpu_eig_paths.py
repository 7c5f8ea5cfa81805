"""pmarlo_amd/csrc/eig.hip on every launch path, against inputs whose spectrum is prescribed (tests/_eig_ref.py).

msm_tica_solve, msm_eigh and msm_onesided_tica_eigenvalues each pick their code path from the matrix order and the
data alone; the cases below sit on both sides of every switch (`tica_path`, `eigh_path`, `onesided_path` restate the
rule and each test asserts the branch it means to reach).  The truth of every case comes from its construction in
long double, not from another eigensolver; tolerances are those of tests/_eig_ref.py, which
tests/test_eig_reference.py proves numpy meets with a tenth to spare.  Every solve runs twice and must repeat bit for
bit."""

from __future__ import annotations

import numpy as np
import pytest

from tests import _eig_ref as er

pytestmark = pytest.mark.gpu

_FIRST: dict = {}     # name -> outputs of the first solve of a tica case in this session


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _tica(engine, case):
    F = case["F"]
    sc = None if case["scale"] is None else engine.to_device(case["scale"])
    eig, W, mean, rank = engine.tica_solve(engine.to_device(case["moments"]), F, scale=sc, epsilon=case["epsilon"],
                                           kinetic_map=case["kinetic_map"])
    return eig.to_host(), W.to_host(), mean.to_host(), int(rank.to_host()[0])


def _tica_checked(engine, case):
    out = _tica(engine, case)
    fig = er.check_tica(out, case)
    print(case["name"], case["path"]["kernel"], case["path"]["first"], case["path"]["second"], fig, "tol", case["tol"])
    assert _same(out, _tica(engine, case)), (case["name"], "second solve differs")
    _FIRST.setdefault(case["name"], out)
    return out


@pytest.mark.parametrize("F,cond4", [(F, False) for F in er.FULL_RANK_F] + [(F, True) for F in er.COND4_F])
def test_tica_full_rank_every_kernel(engine, F, cond4):
    """Full-rank C00, eigenvalues over [-0.6, 0.97] (negative TICA eigenvalues included), kinetic_map on and off
    (kinetic_map = 0), scale = NULL / a per-feature scale / a mean of up to three standard deviations; cond 1e2 and, at
    F = 64, 69, 97, 256, cond 1e4 with epsilon = 1e-12.  F <= 64: the fused path (ldl_whiten_registers, the
    1 / |W|_F^2 certificate, tridiag_eigh, the tail in LDS), F = 1 included.  65: four matrices in LDS, not fused
    (cholesky_lower_pair, lower_inverse, Jacobi on the whitened matrix, sort_desc_abs and canonical_signs).  66..97:
    tica_solve_kernel<2>, A and V in LDS, B1 and B2 in global memory (66..69 would fit the 150 KiB budget with four
    matrices, but not next to the kernel's own 27 KiB of __shared__ structs: they failed to launch before the
    launcher took those into account).  98..256: tica_solve_kernel<0>, everything in global memory."""
    want = "fused" if F <= 64 else "lds4" if F <= 65 else "lds2" if F <= 97 else "global"
    cases = [c for c in er.tica_full_rank_cases(F) if ("cond1e4" in c["name"]) == cond4]
    assert len(cases) == 6 and all(c["epsilon"] == (1e-12 if cond4 else 1e-6) for c in cases)
    for case in cases:
        p = case["path"]
        assert p["kernel"] == want and p["first"] == ("ldl_registers" if F <= 64 else "cholesky_pair")
        assert p["second"] == ("tridiag" if F <= 64 else "jacobi_" + er.jacobi_variant(F, p["ld"]))
        _tica_checked(engine, case)


@pytest.mark.parametrize("F,r", er.DEFICIENT)
def test_tica_rank_deficient(engine, F, r):
    """C00 = B C00^ B' of rank r: the first eigensolve is jacobi_eigh -- pipelined at (8, 5) and (64, 60), generic at
    the odd and the large orders -- then the r x r problem.  (64, 60) and the small orders go on to tridiag_eigh;
    (65, 64) and (65, 40) are the one non-fused order that reaches it; (66, 64) and (69, 33) have the same sizes but
    run Jacobi (pipelined at rank 64) in tica_solve_kernel<2>; (80, 70), (100, 37) and (256, 200) run mfma_mm with inner
    dimensions that are no multiple of 4 or 16 on matrices in global memory."""
    cases = [c for c in er.tica_deficient_cases() if c["F"] == F and c["rank"] == r]
    assert len(cases) == 2
    p = er.tica_path(F, r)
    assert p["first"] == "jacobi_" + er.jacobi_variant(F, p["ld"])
    assert (p["second"] == "tridiag") == (F <= 65)
    if (F, r) == (64, 60):
        assert p["first"] == "jacobi_pipelined"
    if F in (66, 69):
        assert p["lds_mats"] == 2 and p["second"] == "jacobi_" + er.jacobi_variant(r, p["ld"])
    for case in cases:
        assert case["path"] == p
        _tica_checked(engine, case)


def test_tica_epsilon_cut_off_the_fused_path(engine):
    """The smallest C00 eigenvalue at 1.5e-6 (kept: the Cholesky probe of C00 - epsilon I succeeds, full rank) and at
    0.6e-6 (the probe fails, build_cov runs again and the eigen path cuts the direction), at F = 70
    (tica_solve_kernel<2>) and F = 100 (tica_solve_kernel<0>)."""
    cases = er.tica_cut_cases()
    assert sorted((c["F"], c["F"] - c["rank"]) for c in cases) == [(70, 0), (70, 1), (100, 0), (100, 1)]
    for case in cases:
        _tica_checked(engine, case)


@pytest.mark.parametrize("i", range(len(er.CLUSTERED)))
def test_tica_clustered_whitened_spectrum_takes_the_fallback(engine, i):
    """Three equal whitened eigenvalues and a pair 1e-12 apart: tridiag_eigh rejects its own result (orthogonality
    defect above 1e-11), tica_solve restores the copy saved in wk.A and runs Jacobi.  F = 16 and 64 on the fused
    path, (65, 64) on the non-fused one.  tica_solve shows no path indicator, so the witness is msm_eigh on the same
    whitened matrix (formed on the host): it must report sweeps > 0."""
    case = er.tica_clustered_cases()[i]
    assert case["path"]["second"] == "tridiag" and er.eigh_path(case["rank"])["solver"] == "tridiag"
    _tica_checked(engine, case)
    sweeps = int(engine.eigh(engine.to_device(er.whitened_matrix(case)))[2].to_host()[0])
    assert sweeps > 0, "the tridiagonal solver accepted a spectrum with a triple eigenvalue"


def test_tica_indefinite_c00_raises_the_cut(engine):
    """One C00 eigenvalue at -1e-3 (F = 6 fused, F = 70 tica_solve_kernel<2>): epsilon is raised to -ev_min + 1e-16,
    the negative direction is cut; rank and eigenvalues as npport.tica_from_moments, which implements the same cut."""
    for case in er.tica_indefinite_cases():
        assert case["rank"] == case["F"] - 1
        out = _tica_checked(engine, case)
        ref = er.numpy_tica(case)
        assert out[3] == ref["rank"]
        np.testing.assert_allclose(out[0], ref["eig"], rtol=0, atol=1.1 * case["tol"])


def test_tica_rank_zero_and_no_pairs(engine):
    """All-zero moments with T > 0: rank 0, eig and W all zero (the numpy port raises there; the kernel's contract
    is zeros).  T = 0 and T < 0: rank 0 and eig, W and mean all zero."""
    for case in er.tica_zero_cases():
        assert case["zero"]
        _tica_checked(engine, case)


@pytest.mark.parametrize("descending", [True, False])
def test_tica_results_do_not_depend_on_what_ran_before(engine, descending):
    """The whole case list once in descending and then once in ascending F on the session's engine: the scratch
    buffer grows, the dynamic-LDS attribute of the three kernels goes up and down between launches; every result
    repeats the first solve of its case bit for bit."""
    cases = er.all_tica_cases()
    for case in cases:
        if case["name"] not in _FIRST:
            _FIRST[case["name"]] = _tica(engine, case)
    for case in sorted(cases, key=lambda c: -c["F"] if descending else c["F"]):
        assert _same(_tica(engine, case), _FIRST[case["name"]]), case["name"]


# ---- msm_eigh ---------------------------------------------------------------------------------------------------------
def _eigh(engine, case, want_vectors=True):
    w, v, sweeps = engine.eigh(engine.to_device(case["A_in"]), want_vectors=want_vectors)
    return w.to_host(), (v.to_host() if v is not None else None), int(sweeps.to_host()[0])


@pytest.mark.parametrize("case", er.eigh_cases(), ids=lambda c: c["name"])
def test_eigh_every_path(engine, case):
    """A = Q diag(w) Q' formed in long double.  n <= 64: three LDS matrices and tridiag_eigh (sweeps == 0 on the
    well-separated spectra: accepted); a triple eigenvalue is rejected, A is restored from gA and Jacobi runs
    (sweeps >= 1), pipelined at n = 8 and 64, generic at n = 33.  n = 65..91 (66, 91): Jacobi in LDS; n = 92..256 (92,
    94, 95, 100, 128, 255, 256): Jacobi in global memory (92..94 fit the 140 KiB budget but not next to the kernel's
    own __shared__ structs).  Clusters with relative gaps 1e-6, 1e-8, 1e-10 lie around the
    acceptance threshold (either path must deliver), graded spectra logspace(0, -14), A 2^+-200, the zero matrix, the
    identity, an unsorted diagonal with negatives, 1 x 1, [[a, b], [b, a]], and an input that is not symmetric (the
    truth is that of (A + A') / 2).  want_vectors=False returns the same bytes of w."""
    assert case["path"] == er.eigh_path(case["n"])
    w, v, sweeps = _eigh(engine, case)
    fig = er.check_eigh(w, v, case)
    print(case["name"], case["path"], "sweeps", sweeps, fig, "tol", case["tol"])
    # Sweeps: a count equal to jacobi_eigh's cap is the one value that says the iteration did not converge.  On the
    # well-separated spectra the count also stays within the 14 that test_jacobi_eigh allows for such matrices; the
    # graded and clustered ones (condition up to 1e14) have no such figure to go by, only the cap.
    assert 0 <= sweeps < er.JACOBI_MAX_SWEEPS
    if case["kind"] == "separated":
        assert sweeps <= 14
    if case["expect_sweeps"] == "zero":
        assert case["path"]["solver"] == "tridiag" and sweeps == 0
    if case["expect_sweeps"] == "positive":
        assert case["path"]["solver"] == "tridiag" and sweeps >= 1
    w2, v2, sweeps2 = _eigh(engine, case)
    assert _same((w, v), (w2, v2)) and sweeps2 == sweeps
    w3, v3, sweeps3 = _eigh(engine, case, want_vectors=False)
    assert v3 is None and w3.tobytes() == w.tobytes() and sweeps3 == sweeps


# ---- msm_onesided_tica_eigenvalues -------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,const", [(F, None) for F in er.ONESIDED_F] + [(8, 3), (70, 3)])
def test_onesided_estimator_every_path(engine, F, const):
    """The DeepTICA eigenvalue estimator through trainer_api.estimate_top_eigenvalues against the numpy restatement:
    F <= 64 in LDS with tridiag_eigh (1, 2, 63, 64), F = 65 in LDS with Jacobi, F = 66, 67, 128, 256 in global
    memory (66 fits the 140 KiB budget but not next to the kernel's own __shared__ structs).  A constant column (F = 8: LDS and tridiagonal; F = 70: global memory and Jacobi) gives an exact zero row
    and column of C0, so the `clip` branch runs."""
    from pmarlo_amd.features.deeptica.core import trainer_api

    case = er.onesided_case(F, const)
    p = case["path"]
    assert p["storage"] == ("lds" if F <= 65 else "global") and p["solver"] == ("tridiag" if F <= 64 else "jacobi")
    idx = case["idx"]
    ev = trainer_api.estimate_top_eigenvalues(case["X"], idx, idx + case["lag"], F, engine=engine)
    fig = er.check_onesided(ev, case)
    print(case["name"], p, fig)
    ev2 = trainer_api.estimate_top_eigenvalues(case["X"], idx, idx + case["lag"], F, engine=engine)
    assert ev2.tobytes() == ev.tobytes()
