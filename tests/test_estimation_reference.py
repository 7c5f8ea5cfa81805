"""Host-only checks of tests/_estimation_ref.py: the references, closed forms, tolerance helpers and the conditions
the GPU tests of the dense estimation / CK / TPT kernels rely on.  Runs on a machine without a GPU."""
import math

import numpy as np
import pytest

from oracle import cport, npport
from tests import _estimation_ref as R

U, LD = R.U, R.LD


# -- tolerance helpers on hand-made sums --------------------------------------------------------------------
def test_sum_bound_counts_additions():
    assert R.sum_bound(1) == 0.0 and R.sum_bound(0) == 0.0
    assert R.sum_bound(2) == U and R.sum_bound(1025) == 1024 * U
    assert R.product_bound(4) == 4 * U


def test_sum_bound_holds_for_naive_orders_and_is_not_slack():
    rng = np.random.default_rng(0)
    x = rng.random(5000)
    exact = LD(math.fsum(x))
    for order in (np.arange(5000), np.arange(5000)[::-1], rng.permutation(5000)):
        s = 0.0
        for v in x[order]:
            s += v
        R.assert_sum_close(s, exact, 5000)
    # three terms with a worst-case rounding each: 1 + u + u rounds down twice; the helper allows 2u, not 0
    terms = [1.0, U, U]
    got = (terms[0] + terms[1]) + terms[2]
    assert got == 1.0
    R.assert_sum_close(got, LD(1) + 2 * LD(U), 3)
    with pytest.raises(AssertionError):
        R.assert_sum_close(got, LD(1) + 2 * LD(U), 2)
    with pytest.raises(AssertionError):           # a lost term of relative size 0.1 / k is far outside
        R.assert_sum_close(1.0 - 0.1 / 2304, 1.0, 2304)


def test_assert_within_rejects_non_finite_and_rel_dev_pins_zeros():
    with pytest.raises(AssertionError):
        R.assert_within(np.nan, 1.0, 1.0)
    with pytest.raises(AssertionError):
        R.assert_within([1.0, np.inf], [1.0, np.inf], 1.0)
    assert R.rel_dev([1.0, 0.0, 2.0], [1.0, 0.0, 4.0]) == 0.5
    with pytest.raises(AssertionError):
        R.rel_dev([1.0, 1e-300], [1.0, 0.0])
    assert R.rule3_limit(1e-16, 3e-16) == 8e-16 and R.rule3_limit(1e-18, 3e-16) == 3e-16


def test_padding_helpers():
    a = np.arange(6.0).reshape(2, 3)
    p = R.pad2d(a)
    assert p.shape == (2, 3 + R.PAD) and np.array_equal(p[:, :3], a) and np.isnan(p[:, 3:]).all()
    buf = R.pad_batch([a, a[:1, :2]], 2, 3, 5, 13)
    assert buf.size == 26 and np.array_equal(R.batch_view(buf, 0, 2, 5, 13)[:, :3], a)
    v1 = R.batch_view(buf, 1, 2, 5, 13)
    assert np.array_equal(v1[0, :2], a[0, :2]) and np.isnan(v1[1]).all() and np.isnan(v1[0, 2:]).all()
    mask = R.batch_padding_mask(2, 2, 3, 5, 13)
    assert mask.sum() == 26 - 12 and np.isnan(buf[mask]).all()


# -- conditions the GPU tests rely on -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 17, 65, 70, 257, 1025])
def test_generated_stochastic_matrices_have_row_sums_within_4u(n):
    mats = [R.stochastic(n, n), R.reversible_chain(n, n)[0]]
    if n >= 2:
        mats.append(R.birth_death(n, n)[0])
    for T in mats[:1] + mats[2:]:
        assert (T >= 0).all()
        rs = T.astype(LD).sum(axis=1)
        assert np.abs(rs - 1).max() <= 4 * U
    rs = mats[1].astype(LD).sum(axis=1)               # X / rowsum: n roundings of relative u, averaged -> within u
    assert np.abs(rs - 1).max() <= 4 * U


@pytest.mark.parametrize("n,nrhs", R.SOLVE_SHAPES)
def test_solve_inputs_are_well_conditioned_and_lapack_is_accurate(n, nrhs):
    A, B = R.solve_system(n, nrhs)
    assert n == 1 or A[0, 0] == 0.0
    assert R.cond_inf(A) <= 1e6
    limit, ref = R.solve_limit(A, B)
    print(f"n={n} nrhs={nrhs} cond_inf={R.cond_inf(A):.3g} omega(LAPACK)={ref / U:.3g} u limit={limit / U:.3g} u")
    assert ref <= 16 * U and limit >= n * U


def test_ck_perturbations_are_at_least_1e_3():
    for n in (1, 17, 70):
        T1, Tk, E = R.ck_case(n, n)
        for i, f in enumerate(R.CK_FACTORS):
            if f == 1:
                assert np.array_equal(Tk[i], T1) and not E[i].any()
            else:
                assert np.abs(E[i]).min() >= 1e-3
        assert np.array_equal(E[0], E[3]) and np.array_equal(Tk[0], Tk[3])         # the two entries of factor 3
        assert Tk.min() >= 0.0 and Tk.max() <= 1.0                                 # p (1 - p) >= 0 in the noise sum
        ref = R.ck_mse_reference(T1, Tk, R.CK_FACTORS)
        assert ref[1] == 0
        for i, f in enumerate(R.CK_FACTORS):
            if f > 1:                 # the planted E dominates: mse = mean(E^2) up to the rounding of the power
                R.assert_within(ref[i], (E[i].astype(LD) ** 2).mean(), 1e-10, f"factor {f}")
                want = npport.ck_error(T1, Tk[i], f) ** 2
                R.assert_within(want, ref[i], R.ck_mse_rtol(f, n), f"npport factor {f}")


# -- references against the project's float64 oracles ---------------------------------------------------------
def test_multinomial_se_reference_and_bad_row_counts():
    P = R.stochastic(17, 3)
    N = np.random.default_rng(3).integers(1, 500, 17).astype(float)
    N[[0, 4, 9, 16]] = [0.0, -3.0, np.inf, np.nan]
    want = npport.multinomial_rms_se(P, N)
    fixed = N.copy()
    fixed[[0, 4, 9, 16]] = 1.0
    assert want == npport.multinomial_rms_se(P, fixed)
    R.assert_within(want, R.multinomial_se_ld(P, N), (17 * 17 + 3) * U)


def test_diff_norms_reference():
    rng = np.random.default_rng(1)
    for n, m in R.DIFF_SHAPES:
        P, Q = rng.standard_normal((n, m)), rng.standard_normal((n, m))
        ref = R.diff_norms_ld(P, Q)
        d = P - Q
        for got, want in zip((np.abs(d).sum(), np.abs(Q).sum(), (d * d).sum()), ref):
            R.assert_within(got, want, R.sum_bound(n * m) + 2 * U)
        assert not R.diff_norms_ld(P, P)[[0, 2]].any()


@pytest.mark.parametrize("variant", ["planted", "all", "zero"])
@pytest.mark.parametrize("dtype", [np.int64, np.float64])
@pytest.mark.parametrize("k", [1, 40, 1025])
def test_mode1_reference_matches_npport(k, dtype, variant):
    eps = 0.5 if dtype is np.float64 else 1e-12
    C, info = R.mode1_counts(k, dtype, k, variant=variant, epsilon=eps)
    for alpha in (1e-3, 0.5):
        active, inv, T = R.mode1_reference(C, alpha, eps)
        Ca, act_np = npport.ensure_connected_counts(C, alpha=alpha, epsilon=eps)
        assert np.array_equal(active, act_np)
        assert np.array_equal(np.nonzero(inv >= 0)[0], active) and np.array_equal(inv[active], np.arange(active.size))
        if active.size:
            np.testing.assert_allclose(T.astype(float), Ca / Ca.sum(axis=1, keepdims=True), rtol=1e-13)
            assert np.abs(T.sum(axis=1) - 1).max() < 1e-17
    if variant == "zero":
        assert active.size == 0
    elif variant == "all" or k == 1:
        assert active.size == k
    if variant == "planted" and k > 1:
        dead = R.mode1_inactive(k)
        assert {0, k - 1} <= set(dead) and (k <= 1024 or {1023, 1024} <= set(dead))
        s = info["column_only"]
        assert C[s].sum() == 0 and C[:, s].sum() > 0 and inv[s] >= 0
        np.testing.assert_allclose(float(T[inv[s]].sum() * active.size * 0.5), active.size * 0.5, rtol=1e-15)
        if dtype is np.float64:
            assert inv[info["at_epsilon"]] == -1 and inv[info["above_epsilon"]] >= 0
            assert np.array_equal(np.setdiff1d(np.arange(k), active), np.setdiff1d(dead, [info["above_epsilon"]]))
        else:
            assert np.array_equal(np.setdiff1d(np.arange(k), active), dead)


def test_mode1_default_epsilon_matches_ml_msm():
    C, _ = R.mode1_counts(40, np.int64, 5)
    ref = npport.ml_msm(C)
    active, inv, T = R.mode1_reference(C, 1e-3, 1e-12)
    assert np.array_equal(active, ref["active"])
    Tpad = np.zeros((40, 40))
    Tpad[:active.size, :active.size] = T.astype(float)
    full, pi = R.embed_reference(Tpad, inv, np.arange(1.0, 41.0))
    np.testing.assert_allclose(full, ref["transition_matrix"], rtol=1e-13)
    assert np.array_equal(np.nonzero(pi)[0], active)


def test_mode0_counts_carry_what_the_cases_need():
    for k in (1, 2, 257, 1025):
        for dtype in (np.int64, np.float64):
            C = R.mode0_counts(k, dtype, k)
            assert C.dtype == dtype and C.max() <= 2.0 ** 41 and float(C.astype(LD).sum(axis=1).max()) < 2.0 ** 53
            rs = C.astype(np.float64).sum(axis=1)
            if k > 2:
                assert rs[0] == 0 and rs[k - 1] == 0 and (rs == 0).sum() >= 3 and C.max() > 2.0 ** 39
            T = npport.normalise_counts(C)
            assert (np.diag(T) >= 0.1).sum() >= max(1, k // 8)
            T = npport.normalise_counts(R.mode0_counts(k, dtype, k, zero_rows=False))
            assert T[0, 0] >= 0.1 and T[k - 1, k - 1] >= 0.1 and (k <= 2 or (T.sum(axis=1) == 0).sum() >= 1)


def test_power_reference_and_its_bound():
    T = R.stochastic(65, 2)
    for s in (1, 3, 6):
        want = R.power_ld(T, s)
        got = np.linalg.matrix_power(T, 2 ** s)
        assert np.abs(got - want).max() <= (2 ** s - 1) * 65 * U
        assert np.abs(want.sum(axis=1) - 1).max() <= 2 ** s * 4 * U
    R.assert_within(R.matpow_ld(T, 5), np.linalg.matrix_power(T, 5), 1e-12)


@pytest.mark.parametrize("n", [1, 3, 5, 65])
def test_revmle_longdouble_restatement(n):
    C = R.revmle_counts(n, n)
    for it in (1, 33):
        T, pi = R.revmle_ld(C, it)
        T64, pi64, done = npport.reversible_mle(C, maxerr=1e-300, maxiter=it)
        assert done == it or n == 1
        assert R.rel_dev(T64, T) <= 64 * n * U and R.rel_dev(pi64, pi) <= 64 * n * U
        assert np.abs(T.sum(axis=1) - 1).max() < 1e-17


def test_revmle_restatement_keeps_self_loops_and_handles_bands():
    C = R.revmle_counts(9, 1)
    C[[2, 6], :] = 0.0
    C[:, [2, 6]] = 0.0
    T, pi = R.revmle_ld(C, 40)
    keep = np.setdiff1d(np.arange(9), [2, 6])
    Tr, pir = R.revmle_ld(C[np.ix_(keep, keep)], 40)
    assert R.rel_dev(T[np.ix_(keep, keep)], Tr) <= 1e-16 and R.rel_dev(pi[keep], pir) <= 1e-16
    assert T[2, 2] == 1 and T[6, 6] == 1 and T[2].sum() == 1 and pi[2] == 0 and pi[6] == 0
    Cb = R.banded_circulant_counts(50)
    assert np.array_equal(np.count_nonzero(Cb + Cb.T, axis=1), np.full(50, 5))
    Tb, pib = R.revmle_ld(Cb, 3)
    T64, pi64, _ = npport.reversible_mle(Cb, maxerr=1e-300, maxiter=3)
    assert R.rel_dev(T64, Tb) <= 64 * 50 * U and R.rel_dev(pi64, pib) <= 64 * 50 * U


# -- the C restatement of the solve ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,nrhs", R.SOLVE_SHAPES)
def test_lu_solve_fma_against_lapack(n, nrhs):
    A, B = R.solve_system(n, nrhs)
    LU, X, info = cport.lu_solve_fma(A, B)
    assert info == 0
    limit, ref = R.solve_limit(A, B)
    got = R.backward_error(A, X, B)
    print(f"n={n}: omega(restatement)={got / U:.3g} u, omega(LAPACK)={ref / U:.3g} u")
    assert got <= limit
    np.testing.assert_allclose(X, np.linalg.solve(A, B), rtol=1e-7, atol=1e-9)
    # the factors: unit-lower L with |l| <= 1 (partial pivoting) and U reproduce a row permutation of A
    L = np.tril(LU, -1) + np.eye(n)
    assert np.abs(np.tril(LU, -1)).max(initial=0.0) <= 1.0
    PA = L @ np.triu(LU)
    order = np.lexsort(np.round(PA, 6).T[::-1])
    np.testing.assert_allclose(PA[order], A[np.lexsort(np.round(A, 6).T[::-1])], atol=1e-9 * max(1, n))


def test_lu_solve_fma_pivot_rule_and_singular_reports():
    # ties: the FIRST row of maximal |a| is taken, so an all-ones first column swaps nothing
    A = np.array([[1.0, 2.0], [-1.0, 5.0]])
    LU, X, info = cport.lu_solve_fma(A, np.array([3.0, 4.0]))
    assert info == 0 and np.array_equal(LU, [[1.0, 2.0], [-1.0, 7.0]]) and np.array_equal(X, [1.0, 1.0])
    A, B = R.tied_pivot_matrix()
    LU, X, info = cport.lu_solve_fma(A, B)
    assert info == 0 and R.cond_inf(A) <= 1e6
    assert R.backward_error(A, X, B) <= R.solve_limit(A, B)[0]
    for name, A, B in R.singular_cases():
        _, _, info = cport.lu_solve_fma(A, B)
        n = A.shape[0]
        if name.startswith("zero_column"):
            assert info == int(name.rsplit("_", 1)[1]) + 1, name
        else:
            assert info == n, name                 # the copy of the row is eliminated exactly; its zero surfaces last
    assert cport.lu_solve_fma(np.full((5, 5), np.nan), np.ones(5))[2] == 1
    assert cport.lu_solve_fma(np.zeros((1, 1)), np.ones(1))[2] == 1


# -- closed forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 17, 64])
def test_birth_death_closed_forms(n):
    T, pi, a, b, pi_ld = R.birth_death(n, n)
    Tl = T.astype(LD)
    flux = pi_ld[:, None] * Tl
    assert np.abs(flux - flux.T).max() < 1e-18                      # detailed balance of the closed-form pi
    assert np.abs(pi_ld @ Tl - pi_ld).max() < 1e-18
    assert np.array_equal(Tl.sum(axis=1), np.ones(n))               # dyadic rates: the float64 chain IS the ideal one
    role = R.roles(n)
    Wf, rf, Wb, rb = R.committor_systems(T, pi, role)
    q = R.solve_ld(Wf, rf)
    R.assert_within(q, R.birth_death_qplus(a, pi_ld), 0.0, "q+ closed form", atol=1e-16)
    qm = R.solve_ld(Wb, rb)
    R.assert_within(qm, 1 - q, 0.0, "q- = 1 - q+", atol=8 * R.cond_inf(Wb) * n * U)
    np.testing.assert_allclose(npport.committor(T, [0], [n - 1]), q.astype(float), atol=1e-12)
    M = R.birth_death_mfpt(a, b, pi_ld)
    for t, (A, rhs) in enumerate(R.mfpt_systems(T)):
        x = R.solve_ld(A, rhs)
        keep = np.arange(n) != t
        R.assert_within(x, M[keep, t], 1e-13, f"mfpt to {t}")
    np.testing.assert_allclose(npport.macro_mfpt(T), M.astype(float), rtol=1e-9)


def test_closed_class_chains_are_exactly_singular_where_stated():
    for name, T, singular in R.closed_class_chains():
        assert np.array_equal(T.sum(axis=1), np.ones(T.shape[0]))
        got = [t for t, (A, rhs) in enumerate(R.mfpt_systems(T)) if cport.lu_solve_fma(A, rhs)[2] != 0]
        assert got == singular, name
        want = npport.macro_mfpt(T)
        for t in range(T.shape[0]):
            if t not in singular:
                keep = np.arange(T.shape[0]) != t
                A, rhs = R.mfpt_systems(T)[t]
                np.testing.assert_allclose(cport.lu_solve_fma(A, rhs)[1], want[keep, t], rtol=1e-12)


@pytest.mark.parametrize("n,n_macro,empty", [(5, 2, None), (70, 63, 7), (70, 65, None)])
def test_lump_reference_matches_npport(n, n_macro, empty):
    T = R.stochastic(n, n)
    pi = R.stationary_ld(T)
    macro = R.lump_assignment(n, n_macro, n, empty=empty)
    assert set(macro) == set(range(n_macro)) - {empty}
    Tm, pm = R.lump_reference(T, pi, macro, n_macro)
    if empty is None:
        np.testing.assert_allclose(Tm.astype(float), npport.lump_micro_to_macro_T(T, pi, macro), rtol=1e-12)
        np.testing.assert_allclose(pm.astype(float), npport.macro_populations(pi, macro), rtol=1e-12)
    else:
        assert not Tm[empty].any() and pm[empty] == 0
        live = np.abs(Tm.sum(axis=1) - 1) < 1e-17
        assert live.sum() == n_macro - 1


def test_reactive_flux_references_agree_with_npport():
    T = R.stochastic(30, 30)
    pi = R.stationary_ld(T)
    np.testing.assert_allclose(pi @ T, pi, rtol=1e-13)
    role = R.roles(30, seed=1)
    Wf, rf, Wb, rb = R.committor_systems(T, pi, role)
    ref = npport.reactive_flux(T, pi, np.nonzero(role == 1)[0], np.nonzero(role == 2)[0])
    np.testing.assert_allclose(R.solve_ld(Wf, rf).astype(float), ref["qplus"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(R.solve_ld(Wb, rb).astype(float), ref["qminus"], rtol=1e-10, atol=1e-14)
    assert R.cond_inf(Wf) <= 1e6 and R.cond_inf(Wb) <= 1e6
