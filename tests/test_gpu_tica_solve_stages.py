"""The two sequential stages of the TICA solve in eig.hip, the tridiagonalisation and the whitening, at every size
where their code changes shape.

Tridiagonal path: orders on both sides of every multiple of sixteen (the register tiles of the matrix-core products,
the row groups of the Householder phase), with inputs whose reflectors drop out (tau = 0) everywhere, from the start,
or in the middle of the reduction.  Whitening: a blocked LDL' with four pivots per barrier and 16 x 16 accumulator
tiles, so orders on both sides of the edges of four and of sixteen, condition numbers up to 1e12, and rank-deficient
C00 whose first failing pivot sits at every position of a block of four.

Inputs, truths and bounds are those of tests/_eig_ref.py (prescribed spectra, margin 1.0); nothing here is looser."""

from __future__ import annotations

import numpy as np
import pytest

from tests import _eig_ref as er
from tests.test_gpu_tica_leading import _assert_leading_bytes, _takes_candidates

pytestmark = pytest.mark.gpu

ORDERS = (2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 63, 64)
WHITEN_F = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64)


# ---- inputs ------------------------------------------------------------------------------------------------------
def _toeplitz(n):
    """Tridiagonal already (every tau = 0): diagonal 0.5, off-diagonal 0.25, eigenvalues 0.5 + 0.5 cos(k pi / (n + 1))."""
    A = 0.5 * np.eye(n) + 0.25 * (np.eye(n, k=1) + np.eye(n, k=-1))
    pi = er.LD(np.pi) + er.LD(1.2246467991473532e-16)    # float64 pi and its rounding error
    w = er.LD(0.5) + er.LD(0.5) * np.cos(np.arange(1, n + 1, dtype=er.LD) * pi / (n + 1))
    return A, np.asarray(w, np.float64)


def _diagonal(n):
    d = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (0.25 + np.arange(n) / n)
    return np.diag(d), d


def _reduced_in_the_middle(n):
    """Block diagonal, blocks of n / 2 + 2 and the rest: columns n / 2 and n / 2 + 1 meet zeros below the subdiagonal
    (tau = 0 inside a panel) while the columns before and after them need their reflectors."""
    n1 = n // 2 + 2
    w = er._separated(n, 40 + n)
    if n1 >= n:
        return er.eigh_case(f"dense-{n}", n, w, seed=40 + n)["A"], w
    a = er.eigh_case(f"blk1-{n}", n1, w[:n1], seed=41 + n)
    b = er.eigh_case(f"blk2-{n}", n - n1, w[n1:], seed=42 + n)
    A = np.zeros((n, n))
    A[:n1, :n1] = a["A"]
    A[n1:, n1:] = b["A"]
    return A, w


def _eigh_inputs(n):
    sep = er._separated(n, n)
    t_a, t_w = _toeplitz(n)
    d_a, d_w = _diagonal(n)
    m_a, m_w = _reduced_in_the_middle(n)
    return [er.eigh_case(f"stage-separated-{n}", n, sep, seed=n),
            er.eigh_case(f"stage-tridiagonal-{n}", n, t_w, A=t_a),
            er.eigh_case(f"stage-diagonal-{n}", n, d_w, A=d_a),
            er.eigh_case(f"stage-reduced-mid-{n}", n, m_w, A=m_a),
            er.eigh_case(f"stage-scaled-up-{n}", n, sep, seed=n, exp2=200),
            er.eigh_case(f"stage-scaled-down-{n}", n, sep, seed=n, exp2=-200)]


def _eigh(engine, case):
    w, v, sweeps = engine.eigh(engine.to_device(case["A_in"]))
    return w.to_host(), v.to_host(), int(sweeps.to_host()[0])


def _tica(engine, case, n_lead=0):
    F = case["F"]
    sc = None if case["scale"] is None else engine.to_device(case["scale"])
    out = (engine.to_device(np.full(F, np.nan)), engine.to_device(np.full((F, F), np.nan)),
           engine.to_device(np.full(F, np.nan)), engine.to_device(np.full(1, -7, np.int32)))
    engine.tica_solve(engine.to_device(case["moments"]), F, scale=sc, epsilon=case["epsilon"],
                      kinetic_map=case["kinetic_map"], out=out, n_lead=n_lead)
    eig, W, mean, rank = out
    return eig.to_host(), W.to_host(), mean.to_host(), int(rank.to_host()[0])


def _check_tica(engine, case):
    out = _tica(engine, case)
    if not case["zero"]:
        assert out[3] == er.numpy_tica(case)["rank"], case["name"]
    fig = er.check_tica(out, case, margin=1.0)
    print(case["name"], case["path"]["first"], case["path"]["second"], fig, "tol", case["tol"])
    return out


# ---- tridiagonal path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ORDERS)
def test_tridiagonal_path_through_eigh(engine, n):
    """Separated, tridiagonal, diagonal, reduced-in-the-middle and 2^+-200-scaled inputs meet the bounds of check_eigh.
    The sweep count says which solver answered (0: the tridiagonal one) and is printed; the solver's own acceptance
    test may hand any matrix to Jacobi, which is no error, so only the cap is asserted."""
    for case in _eigh_inputs(n):
        assert case["path"]["solver"] == "tridiag"
        w, v, sweeps = _eigh(engine, case)
        fig = er.check_eigh(w, v, case, margin=1.0)
        print(case["name"], "sweeps", sweeps, fig, "tol", case["tol"])
        assert 0 <= sweeps < er.JACOBI_MAX_SWEEPS, case["name"]


@pytest.mark.parametrize("F", ORDERS)
def test_tridiagonal_path_through_tica_solve(engine, F):
    for km in (True, False):
        case = er.tica_case(f"stage-tri-{F}-{'km' if km else 'raw'}", F, seed=F, kinetic_map=km, mean=km, scale=not km)
        assert case["path"]["first"] == "ldl_registers" and case["path"]["second"] == "tridiag"
        _check_tica(engine, case)


# ---- clustered spectra still reach Jacobi --------------------------------------------------------------------------
def test_clustered_spectra_fall_back_to_jacobi_within_the_bounds(engine):
    for case in er.eigh_cases():
        if case["n"] <= er.TRI_MAX and case["name"].startswith(("triple", "cluster")):
            w, v, sweeps = _eigh(engine, case)
            er.check_eigh(w, v, case, margin=1.0)
            if case["expect_sweeps"] == "positive":
                assert sweeps >= 1, (case["name"], "the tridiagonal result was accepted")
    for case in er.tica_clustered_cases():
        _check_tica(engine, case)
        if case["rank"] <= er.TRI_MAX and case["path"]["second"] == "tridiag":
            sweeps = int(engine.eigh(engine.to_device(er.whitened_matrix(case)))[2].to_host()[0])
            assert sweeps > 0, (case["name"], "the tridiagonal solver accepted a triple eigenvalue")


# ---- leading solve against full solve ----------------------------------------------------------------------------
@pytest.mark.parametrize("F,rank", [(16, None), (33, None), (64, None), (65, 64)])
def test_leading_solve_carries_the_bits_of_the_full_solve(engine, F, rank):
    """n_lead = 1, 2, 10, F - 1, and on both sides of the n_lead from which 2 (n_lead + 2) >= rank makes the solve
    compute all pairs.  F = 65 with rank 64: four matrices at stride 65, all pairs whatever n_lead."""
    r = rank or F
    edge = (r + 1) // 2 - 2     # the smallest n_lead with 2 (n_lead + 2) >= rank
    case = er.tica_case(f"stage-lead-{F}-{r}", F, rank=rank, seed=F + 5, mean=True)
    assert case["rank"] == r
    took = []
    for n_lead in sorted({1, 2, 10, F - 1, edge - 1, edge} - {0, -1}):
        _assert_leading_bytes(engine, case, n_lead)
        if _takes_candidates(case, n_lead):
            took.append(n_lead)
    want = [m for m in sorted({1, 2, 10, F - 1, edge - 1, edge} - {0, -1}) if F <= 64 and 2 * (m + 2) < r]
    assert took == want, (took, want)
    if F <= 64:
        assert edge - 1 in took and edge not in took


# ---- whitening -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", WHITEN_F)
def test_whitening_full_rank(engine, F):
    """cond(C00) = 1e2 (the certificate decides), 1e6 and 1e12 with epsilon below the smallest eigenvalue."""
    for cond, eps in ((1e2, 1e-6), (1e6, 1e-9), (1e12, 1e-14)):
        if F == 1 and cond > 1e2:
            continue
        case = er.tica_case(f"stage-whiten-{F}-{cond:g}", F, seed=F + 7, cond=cond, epsilon=eps, mean=True)
        assert case["rank"] == F and case["path"]["first"] == "ldl_registers"
        _check_tica(engine, case)


def test_whitening_cut_indefinite_and_zero_cases(engine):
    cases = list(er.tica_cut_cases()) + list(er.tica_indefinite_cases()) + list(er.tica_zero_cases())
    # the same cuts on the fused path: the smallest eigenvalue of C00 just above and just below epsilon, and negative
    for F in (9, 16, 64):
        for small in (1.5e-6, 0.6e-6, -1e-3):
            cases.append(er.tica_case(f"stage-cut-{F}-{small:g}", F, s2=er._cut_s2(F, small), seed=F + 1))
    for case in cases:
        _check_tica(engine, case)   # (the rank-0 cases are not put to the numpy port, which raises on zero moments)


@pytest.mark.parametrize("F,rank", [(9, 4), (9, 5), (9, 6), (9, 7), (64, 60), (64, 61), (64, 62), (64, 63)])
def test_whitening_rank_deficient_at_every_position_of_a_block(engine, F, rank):
    """rank = 4 m + r, r = 0 .. 3: the first pivot that fails sits at each position of a group of four."""
    for km in (True, False):
        case = er.tica_case(f"stage-rank-{F}-{rank}-{'km' if km else 'raw'}", F, rank=rank, seed=F + rank, kinetic_map=km,
                            mean=km, scale=not km)
        assert case["rank"] == rank and case["path"]["first"].startswith("jacobi")
        eig, W, mean, got = _check_tica(engine, case)
        assert got == rank and np.all(eig[rank:] == 0.0) and np.all(W[:, rank:] == 0.0)
