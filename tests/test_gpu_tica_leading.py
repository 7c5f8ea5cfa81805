"""msm_tica_solve_leading (Engine.tica_solve(n_lead=...)) against msm_tica_solve, byte for byte.

The leading solve returns the first min(n_lead, rank) components of the full solve with the same bits and exact zeros
after them.  On the fused path (F <= 64) the tridiagonal solver then brackets only the n_lead + 1 eigenvalues at
either end of the spectrum (the candidates) plus one guard beyond them, and forms only the candidates' vectors -- for
full-rank and rank-deficient C00 alike, as long as 2 (n_lead + 2) < rank; every other path, F = 65 with rank <= 64
(which reaches the tridiagonal solver too) included, computes all pairs and truncates.  The inputs are those of
tests/_eig_ref.py (prescribed spectra, truth by construction).  Every output buffer is filled with NaN before the
launch, so a zero is a zero the kernel wrote.

One case is NOT byte-equal by design and is tested for what does hold: the acceptance test of the leading solve sees
the candidates' vectors only, so a failed test that involves a vector it does not form (a cluster among eigenvalues
that are neither candidates nor guards) sends the full solve to Jacobi and not the leading one
(test_cluster_outside_the_candidates_agrees_to_solver_accuracy; the near-tie spectrum below n_lead = 9 is left out
of the byte comparison for the same reason)."""

from __future__ import annotations

import numpy as np
import pytest

from tests import _eig_ref as er

pytestmark = pytest.mark.gpu

_FULL: dict = {}     # case name -> outputs of msm_tica_solve (computed once, never modified)


def _outputs(engine, F):
    return (engine.to_device(np.full(F, np.nan)), engine.to_device(np.full((F, F), np.nan)),
            engine.to_device(np.full(F, np.nan)), engine.to_device(np.full(1, -7, np.int32)))


def _host(out):
    eig, W, mean, rank = out
    return eig.to_host(), W.to_host(), mean.to_host(), int(rank.to_host()[0])


def _full(engine, case):
    """msm_tica_solve itself (the C entry, not the engine method, which goes through the new one)."""
    if case["name"] not in _FULL:
        from pmarlo_amd._lib import check, lib

        F = case["F"]
        sc = None if case["scale"] is None else engine.to_device(case["scale"])
        mom = engine.to_device(case["moments"])
        eig, W, mean, rank = out = _outputs(engine, F)
        check(lib.msm_tica_solve(engine.handle, mom.ptr, sc.ptr if sc is not None else None, F, float(case["epsilon"]),
                                 int(case["kinetic_map"]), eig.ptr, W.ptr, mean.ptr, rank.ptr), engine.handle)
        res = _host(out)
        for a in res[:3]:
            a.setflags(write=False)
        _FULL[case["name"]] = res
    return _FULL[case["name"]]


def _lead(engine, case, n_lead):
    F = case["F"]
    sc = None if case["scale"] is None else engine.to_device(case["scale"])
    out = _outputs(engine, F)
    engine.tica_solve(engine.to_device(case["moments"]), F, scale=sc, epsilon=case["epsilon"],
                      kinetic_map=case["kinetic_map"], out=out, n_lead=n_lead)
    return _host(out)


def _assert_leading_bytes(engine, case, n_lead):
    """The whole contract: kept part, mean and rank byte-equal to the full solve, exact zeros after the kept part."""
    F = case["F"]
    feig, fW, fmean, frank = _full(engine, case)
    eig, W, mean, rank = _lead(engine, case, n_lead)
    tag = (case["name"], n_lead)
    assert rank == frank == case["rank"], tag
    m = frank if n_lead <= 0 or n_lead >= F else min(n_lead, frank)
    assert mean.tobytes() == fmean.tobytes(), tag
    assert eig[:m].tobytes() == feig[:m].tobytes(), (tag, "eigenvalues", eig[:m], feig[:m])
    assert np.ascontiguousarray(W[:, :m]).tobytes() == np.ascontiguousarray(fW[:, :m]).tobytes(), (
        tag, "columns", np.nonzero((W[:, :m] != fW[:, :m]).any(axis=0))[0])
    # exact +0.0, not NaN and not -0.0
    assert eig[m:].tobytes() == np.zeros(F - m).tobytes(), (tag, "eigenvalues past the kept ones")
    assert np.ascontiguousarray(W[:, m:]).tobytes() == np.zeros((F, F - m)).tobytes(), (tag, "columns past the kept ones")
    return m


def _takes_candidates(case, n_lead):
    """Whether the solve brackets the two ends only: fused path, tridiagonal solver, 2 (n_lead + 2) < rank."""
    p = case["path"]
    return p["fused"] and p["second"] == "tridiag" and 0 < n_lead and 2 * (n_lead + 2) < case["rank"]


def _n_leads(F):
    return sorted({1, 2, 10, F - 1, F} - {0})


# ---- 1. byte equality on every kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("F", [6, 16, 33, 64, 65, 70, 100])
def test_leading_equals_full_on_every_kernel(engine, F):
    """F = 6, 16, 33, 64: the fused path; candidates only at (16, n_lead 1 / 2), (33, 1 / 2 / 10), (64, 1 / 2 / 10), all
    pairs and a truncated tail elsewhere (6: candidates and guards are all there is).  65: four matrices in LDS,
    Jacobi; 70: tica_solve_kernel<2>; 100: tica_solve_kernel<0> -- all pairs, the generic tail truncates.  n_lead = 10
    exceeds F = 6 and means everything, like n_lead = F.  kinetic_map on and off, with and without a scale (and a
    mean, which the moments carry)."""
    want_kernel = "fused" if F <= 64 else "lds4" if F == 65 else "lds2" if F == 70 else "global"
    took = []
    for km in (True, False):
        for sc in (False, True):
            case = er.tica_case(f"lead-{F}-{'km' if km else 'raw'}-{'scale' if sc else 'plain'}", F, seed=F,
                                kinetic_map=km, scale=sc, mean=sc)
            assert case["path"]["kernel"] == want_kernel and case["rank"] == F
            er.check_tica(_full(engine, case), case)
            for n_lead in _n_leads(F):
                _assert_leading_bytes(engine, case, n_lead)
                if _takes_candidates(case, n_lead):
                    took.append(n_lead)
    assert sorted(set(took)) == {16: [1, 2], 33: [1, 2, 10], 64: [1, 2, 10]}.get(F, [])
    # n_lead <= 0 is the full solve
    case = er.tica_case(f"lead-{F}-km-plain", F, seed=F, kinetic_map=True)
    for n_lead in (0, -3, F + 5):
        assert _assert_leading_bytes(engine, case, n_lead) == F


# ---- 2. |ev| order against algebraic order ---------------------------------------------------------------------
def _spectra(F):
    mag = 0.97 - (0.94 / F) * np.arange(F)          # descending magnitudes, 0.94 / F apart
    alt = np.where(np.arange(F) % 2 == 1, -mag, mag)
    top_negative = np.where(np.arange(F) < 12, -mag, mag)
    near_same = mag.copy()
    near_same[10] = near_same[9] * (1.0 - 1e-13)     # 10th and 11th magnitude 1e-13 apart, same sign: neighbours
    near_opposite = alt.copy()
    near_opposite[10] = -near_opposite[9] * (1.0 - 1e-13)   # ... opposite signs: far apart in the spectrum
    pm = mag.copy()
    pm[10] = -pm[9]                                  # lambda and -lambda straddle a cut at 10
    pm_inside = alt.copy()
    pm_inside[3] = -pm_inside[2]
    return {"top-negative": top_negative, "alternating": alt, "all-positive": mag, "all-negative": -mag,
            "near-tie-same-sign": near_same, "near-tie-opposite-sign": near_opposite, "plus-minus-at-the-cut": pm,
            "plus-minus-inside": pm_inside}


@pytest.mark.parametrize("name", sorted(_spectra(64)))
@pytest.mark.parametrize("F", [33, 64])
def test_order_by_magnitude_is_not_algebraic_order(engine, F, name):
    """Prescribed whitened spectra whose leading magnitudes sit at the negative end, alternate, or all sit at one end;
    magnitudes 1e-13 apart and an exact +- pair on either side of a cut at 10 (the computed values decide the order:
    whatever they are, both solves must cut alike).  n_lead on both sides of each such cut and on both sides of the
    switch 2 (n_lead + 2) < F.  near-tie-same-sign at n_lead = 9 puts the close pair on candidate and guard (all pairs
    are computed then), from n_lead = 10 on two candidates (both solves refuse the vectors and run Jacobi); below 9
    neither of the pair is bracketed, which is the exception of the module docstring (the full solve runs Jacobi, the
    leading one does not), so those n_lead are left to the last test of this file."""
    lam = _spectra(F)[name]
    switch = (F - 1) // 2 - 2          # the largest n_lead that takes the candidates
    for km in (True, False):
        case = er.tica_case(f"order-{F}-{name}-{'km' if km else 'raw'}", F, lam=lam, seed=F + 11, kinetic_map=km,
                            scale=km)
        assert case["path"]["fused"] and case["rank"] == F
        assert _takes_candidates(case, switch) and not _takes_candidates(case, switch + 1)
        for n_lead in (1, 2, 3, 9, 10, 11, 12, switch, switch + 1):
            if name == "near-tie-same-sign" and n_lead < 9:
                continue
            _assert_leading_bytes(engine, case, n_lead)


# ---- 3. rank, cut, fallback, no pairs --------------------------------------------------------------------------
@pytest.mark.parametrize("F,r", [(9, 6), (63, 50), (64, 60), (65, 40), (100, 37)])
def test_rank_deficient_c00(engine, F, r):
    """spd_inv_split by Jacobi, then the r x r problem.  Up to F = 64 the tridiagonal solver, on the candidates when
    2 (n_lead + 2) < r ((63, 50) and (64, 60) at n_lead 1, 2, 10).  (65, 40): the one non-fused order that reaches the
    tridiagonal solver; the generic tail follows it, so all pairs are asked for.  (100, 37): Jacobi.  n_lead below, at
    and above the rank: min(n_lead, rank) columns come back."""
    for case in (c for c in er.tica_deficient_cases() if c["F"] == F and c["rank"] == r):
        for n_lead in (1, 2, 10, r - 1, r, r + 1, F - 1):
            m = _assert_leading_bytes(engine, case, n_lead)
            assert m == min(n_lead, r)
    if F <= 64 and r >= 24:
        assert _takes_candidates(case, 10)


def test_indefinite_c00_raises_the_cut(engine):
    """One C00 eigenvalue at -1e-3 (F = 6: fused, F = 70: tica_solve_kernel<2>): epsilon is raised, the direction cut,
    rank F - 1; both compute all pairs and truncate."""
    for case in er.tica_indefinite_cases():
        for n_lead in (1, 2, case["F"] - 2, case["F"] - 1):
            _assert_leading_bytes(engine, case, n_lead)


@pytest.mark.parametrize("i", range(len(er.CLUSTERED)))
def test_clustered_spectrum_takes_the_fallback_in_both(engine, i):
    """Three equal eigenvalues at magnitude ranks 2-4 (all at the positive end) and a pair 1e-12 apart at 6-7.  n_lead
    = 2: the guard equals the last candidate, all pairs are computed.  n_lead >= 3: two members of the triple are
    candidates, the tridiagonal solver refuses their vectors exactly as in the full solve, the saved copy goes to
    Jacobi and the result is truncated."""
    case = er.tica_clustered_cases()[i]
    assert case["path"]["second"] == "tridiag"
    er.check_tica(_full(engine, case), case)
    for n_lead in (2, 3, 4, 5, 10, case["rank"] - 1):
        _assert_leading_bytes(engine, case, n_lead)


def test_order_65_reaches_the_tridiagonal_solver_and_computes_all_pairs(engine):
    """F = 65 with rank <= 64: four matrices in LDS at the solver's stride, tridiag_eigh runs, the generic tail follows.
    That tail ranks all `rank` eigenvalues, so the solver must be asked for all pairs.  Witness: clustered-65-64 at
    n_lead = 1, 2.  On the candidates the triple at magnitude ranks 2-4 would go unseen and the result would keep the
    tridiagonal vectors (what F = 64 does, last test of this file); computing all pairs, the solver refuses them as in
    the full solve and the bits agree.  (65, 40) and (65, 64) with spread spectra: byte equality at n_lead where
    2 (n_lead + 2) < rank."""
    clustered = next(c for c in er.tica_clustered_cases() if c["F"] == 65)
    cases = [clustered] + [c for c in er.tica_deficient_cases() if c["F"] == 65]
    assert len(cases) == 5
    for case in cases:
        p = case["path"]
        assert p["kernel"] == "lds4" and not p["fused"] and p["second"] == "tridiag" and p["tail"] == "generic"
        assert 2 * (10 + 2) < case["rank"] and not _takes_candidates(case, 10)
        for n_lead in (1, 2, 10):
            _assert_leading_bytes(engine, case, n_lead)


def test_no_pairs_and_rank_zero(engine):
    for case in er.tica_zero_cases():
        for n_lead in (1, 2):
            eig, W, mean, rank = _lead(engine, case, n_lead)
            assert rank == 0 and not eig.any() and not W.any()
            _assert_leading_bytes(engine, case, n_lead)


# ---- 4. against the numpy port ----------------------------------------------------------------------------------
def _check_kept_against_port(out, case, m):
    """The comparisons of er.check_tica with the port, on the kept columns: eigenvalues within 1.1 tol (the bound of
    test_tica_indefinite_c00_raises_the_cut), a column within 1.1 tol / gap of the port's up to sign."""
    eig, W, mean, rank = out
    ref = er.numpy_tica(case)
    tol, rn = case["tol"], case["rnorm"]
    assert rank == ref["rank"]
    np.testing.assert_allclose(eig[:m], ref["eig"][:m], rtol=0, atol=1.1 * tol)
    np.testing.assert_allclose(mean, ref["mean"], rtol=0, atol=8 * er.EPS * max(1.0, float(np.abs(ref["mean"]).max())))
    for a, b in case["groups"]:
        if b - a == 1 and a < m:
            bound = tol / min(case["gap"][a], 1.0)
            s = np.sign(np.dot(W[:, a], ref["W"][:, a])) or 1.0
            dn = float(np.linalg.norm(s * W[:, a] - ref["W"][:, a])) / rn
            print(case["name"], "column", a, "against the port", dn, "bound", 1.1 * bound)
            assert dn <= 1.1 * bound, (case["name"], a, dn, bound)


def test_kept_columns_against_the_numpy_port(engine):
    alt = _spectra(64)["alternating"]
    cases = [er.tica_case("port-64-alternating", 64, lam=alt, seed=75, kinetic_map=True, scale=True),
             next(c for c in er.tica_deficient_cases() if c["F"] == 64 and c["rank"] == 60 and c["kinetic_map"])]
    for case in cases:
        assert _takes_candidates(case, 10)
        _check_kept_against_port(_lead(engine, case, 10), case, 10)


def test_cluster_outside_the_candidates_agrees_to_solver_accuracy(engine):
    """The one documented exception to byte equality.  clustered-64 with n_lead = 1: the candidates are the two
    eigenvalues at either end, the guard (the first of the triple at magnitude ranks 2-4) is 0.015 away, its two
    partners are never bracketed, the two kept candidates' vectors
    pass the acceptance test and come from the tridiagonal solver, while the full solve falls back to Jacobi.  The
    kept pair then meets the bounds that every solve meets against the construction and the numpy port."""
    case = next(c for c in er.tica_clustered_cases() if c["F"] == 64 and c["rank"] == 64)
    assert _takes_candidates(case, 1) and case["groups"][0] == (0, 1)
    out = _lead(engine, case, 1)
    eig, W, mean, rank = out
    feig, fW, fmean, frank = _full(engine, case)
    assert rank == frank and mean.tobytes() == fmean.tobytes()
    assert not eig[1:].any() and not W[:, 1:].any()
    assert abs(eig[0] - case["lam"][0]) <= case["tol"] and abs(eig[0] - feig[0]) <= 2 * case["tol"]
    _check_kept_against_port(out, case, 1)
    bound = case["tol"] / min(case["gap"][0], 1.0)
    assert float(np.linalg.norm(W[:, 0] - fW[:, 0])) / case["rnorm"] <= 2 * bound
