"""The dense kernels after the spectrum on every launch path: msm_gemm_f64, msm_ck_test, msm_diff_norms,
msm_solve_f64, msm_reactive_flux, msm_lump_macro and msm_macro_mfpt against the exact references of
tests/_estimation_ref.py.

Strided cases go through the C ABI with ld = n + 3 (batch strides larger than n * ld) in NaN-filled buffers: the
results must equal the packed call's bit for bit and the padding of every output must still be NaN."""
import time

import numpy as np
import pytest

from oracle import cport, npport
from pmarlo_amd._lib import check, lib
from tests import _estimation_ref as R

pytestmark = pytest.mark.gpu

U, LD, NAN, PAD = R.U, R.LD, np.nan, R.PAD


def _nan_device(engine, shape):
    return engine.to_device(np.full(shape, NAN))


def _minus_ones(engine, n):
    return engine.empty((n,), np.int32).fill_bytes_(0xFF)


# ---------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------
def _gemm(engine, A, B, pad):
    (m, k), n = A.shape, B.shape[1]
    Ad, Bd = engine.to_device(R.pad2d(A, k + pad)), engine.to_device(R.pad2d(B, n + pad))
    Cd = _nan_device(engine, (m, n + pad))
    check(lib.msm_gemm_f64(engine.handle, m, n, k, Ad.ptr, k + pad, Bd.ptr, n + pad, Cd.ptr, n + pad), engine.handle)
    out = Cd.to_host()
    assert np.isnan(out[:, n:]).all()                      # the padding of C is left alone (k = 0 included)
    return out[:, :n]


@pytest.mark.parametrize("k", [0, 1, 3, 4, 5, 15, 16, 17, 19, 20])
def test_gemm_edges_padded_bit_exact(engine, k):
    rng = np.random.default_rng(k)
    for m in (1, 15, 16, 17, 33):
        for n in (1, 15, 16, 17, 33):
            A, B = rng.standard_normal((m, k)), rng.standard_normal((k, n))
            want = cport.gemm_fma(A, B)                    # the ascending-k fma chain from +0, bit for bit
            np.testing.assert_array_equal(_gemm(engine, A, B, PAD), want, err_msg=f"padded {m}x{n}x{k}")
            np.testing.assert_array_equal(_gemm(engine, A, B, 0), want, err_msg=f"packed {m}x{n}x{k}")
            if k == 0:
                assert not want.any()
                continue
            A[m - 1] = NAN                                 # the clamped edge lanes compute on it and must not store
            got = _gemm(engine, A, B, PAD)
            assert np.isnan(got[m - 1]).all()
            np.testing.assert_array_equal(got[:m - 1], want[:m - 1], err_msg=f"NaN row {m}x{n}x{k}")


# ---------------------------------------------------------------------------------------------------------
# Chapman-Kolmogorov test and the difference norms
# ---------------------------------------------------------------------------------------------------------
def _bad_rowcounts(F, n, seed):
    """[F, n] row counts with 0, -3, inf and NaN planted in every row (n >= 4) or spread over the rows (n = 1)."""
    rng = np.random.default_rng(seed)
    rc = rng.integers(1, 500, size=(F, n)).astype(float)
    bad = [0.0, -3.0, np.inf, NAN]
    for i in range(F):
        if n >= 4:
            rc[i, rng.permutation(n)[:4]] = bad
        else:
            rc[i, 0] = bad[i % 4]
    return rc


def _ck(engine, T1, Tk, factors, rc, pad):
    n, F = T1.shape[0], len(factors)
    ld1, ldk = n + pad, n + pad
    tk_stride = n * ldk + (5 if pad else 0)
    rc_stride = n + (PAD if pad else 0)
    T1d = engine.to_device(R.pad2d(T1, ld1))
    Tkd = engine.to_device(R.pad_batch(list(Tk), n, n, ldk, tk_stride))
    fac = np.ascontiguousarray(factors, np.int32)
    mse = _nan_device(engine, F + 2)
    rcd = noise = None
    if rc is not None:
        rcd, noise = engine.to_device(R.pad2d(rc, rc_stride)), _nan_device(engine, F + 2)
    check(lib.msm_ck_test(engine.handle, T1d.ptr, ld1, Tkd.ptr, tk_stride, ldk, n, fac.ctypes.data, F,
                          rcd.ptr if rcd is not None else None, rc_stride, mse.ptr,
                          noise.ptr if noise is not None else None), engine.handle)
    mse = mse.to_host()
    assert np.isnan(mse[F:]).all()
    if noise is None:
        return mse[:F], None
    noise = noise.to_host()
    assert np.isnan(noise[F:]).all()
    return mse[:F], noise[:F]


@pytest.mark.parametrize("n", [1, 17, 70])
def test_ck_test_unsorted_factors_padded(engine, n):
    factors = R.CK_FACTORS
    T1, Tk, _ = R.ck_case(n, n)
    rc = _bad_rowcounts(len(factors), n, n)
    mse, noise = _ck(engine, T1, Tk, factors, rc, PAD)
    mse_packed, noise_packed = _ck(engine, T1, Tk, factors, rc, 0)
    np.testing.assert_array_equal(mse, mse_packed)
    np.testing.assert_array_equal(noise, noise_packed)
    mse_only, none = _ck(engine, T1, Tk, factors, None, PAD)            # the two-NULL form
    assert none is None
    np.testing.assert_array_equal(mse_only, mse)
    want = R.ck_mse_reference(T1, Tk, factors)
    for i, f in enumerate(factors):
        if f == 1:
            assert mse[i] == 0.0                                         # Tk = T1: exactly zero
        else:
            R.assert_within(mse[i], want[i], R.ck_mse_rtol(f, n), f"mse of factor {f}")
            assert mse[i] >= 1e-6 * 0.99                                 # |E| >= 1e-3 is what is measured
        fixed = np.where(np.isfinite(rc[i]) & (rc[i] > 0), rc[i], 1.0)
        assert (fixed == 1.0).sum() >= 1
        R.assert_within(noise[i], R.multinomial_se_ld(Tk[i], rc[i]), (n * n + 3) * U, f"noise of factor {f}")
        R.assert_within(noise[i], npport.multinomial_rms_se(Tk[i], fixed), (n * n + 3) * U, f"noise vs npport {f}")
    assert mse[0] == mse[3]                                              # factor 3 twice: the same bits
    assert n == 1 or noise[0] != noise[3]                                # ... each with its own row counts
    # against the wrapper, which passes the packed strides
    m_w, n_w = engine.ck_test(engine.to_device(T1), engine.to_device(Tk), factors, engine.to_device(rc))
    np.testing.assert_array_equal(m_w, mse)
    np.testing.assert_array_equal(n_w, noise)


def _diff_norms(engine, P, Q, padp, padq):
    n, m = P.shape
    Pd, Qd = engine.to_device(R.pad2d(P, m + padp)), engine.to_device(R.pad2d(Q, m + padq))
    out = _nan_device(engine, 5)
    check(lib.msm_diff_norms(engine.handle, Pd.ptr, m + padp, Qd.ptr, m + padq, n, m, out.ptr), engine.handle)
    out = out.to_host()
    assert np.isnan(out[3:]).all()
    return out[:3]


@pytest.mark.parametrize("n,m", R.DIFF_SHAPES)
def test_diff_norms_padded(engine, n, m):
    rng = np.random.default_rng(n * 10007 + m)
    P, Q = rng.standard_normal((n, m)), rng.standard_normal((n, m))
    got = _diff_norms(engine, P, Q, PAD, PAD + 2)
    np.testing.assert_array_equal(got, _diff_norms(engine, P, Q, 0, 0))
    np.testing.assert_array_equal(got, engine.diff_norms(engine.to_device(P), engine.to_device(Q)))
    want = R.diff_norms_ld(P, Q)
    R.assert_sum_close(got[0], want[0], n * m, "sum |P - Q|")
    R.assert_sum_close(got[1], want[1], n * m, "sum |Q|")
    # sum (P - Q)^2 is an fma chain: the square is not rounded on its own, but the first fma rounds where a plain
    # sum's first term is exact, so n m terms take n m roundings (sum_bound counts one fewer)
    R.assert_sum_close(got[2], want[2], n * m + 1, "sum (P - Q)^2")
    same = _diff_norms(engine, Q, Q, PAD, 0)
    assert same[0] == 0.0 and same[2] == 0.0 and same[1] == got[1]


# ---------------------------------------------------------------------------------------------------------
# linear solve
# ---------------------------------------------------------------------------------------------------------
def _solve(engine, A, B, pad):
    """msm_solve_f64 with lda = n + pad, ldb = nrhs + pad -> (LU, X, info)."""
    n = A.shape[0]
    B2 = B.reshape(n, -1)
    nrhs = B2.shape[1]
    Ad, Bd = engine.to_device(R.pad2d(A, n + pad)), engine.to_device(R.pad2d(B2, nrhs + pad))
    info = _minus_ones(engine, 2)
    check(lib.msm_solve_f64(engine.handle, n, nrhs, Ad.ptr, n + pad, Bd.ptr, nrhs + pad, info.ptr), engine.handle)
    LU, X, info = Ad.to_host(), Bd.to_host(), info.to_host()
    assert np.isnan(LU[:, n:]).all() and np.isnan(X[:, nrhs:]).all() and info[1] == -1
    return LU[:, :n], X[:, :nrhs].reshape(B.shape), int(info[0])


def _solve_both(engine, A, B):
    LU, X, info = _solve(engine, A, B, 0)
    LUp, Xp, infop = _solve(engine, A, B, PAD)
    np.testing.assert_array_equal(LUp, LU)
    np.testing.assert_array_equal(Xp, X)
    assert infop == info
    return LU, X, info


@pytest.mark.parametrize("n,nrhs", R.SOLVE_SHAPES)
def test_solve_backward_error_and_fixed_arithmetic_order(engine, n, nrhs):
    A, B = R.solve_system(n, nrhs)
    LU, X, info = _solve_both(engine, A, B)
    assert info == 0
    limit, ref = R.solve_limit(A, B)
    omega = R.backward_error(A, X, B)
    print(f"solve n={n} nrhs={nrhs}: omega(device)={omega / U:.3g} u, omega(LAPACK)={ref / U:.3g} u, limit={limit / U:.3g} u")
    assert omega <= limit
    LU_c, X_c, info_c = cport.lu_solve_fma(A, B)          # same pivots, same single fma per update: same bits
    assert info_c == 0
    np.testing.assert_array_equal(LU, LU_c)
    np.testing.assert_array_equal(X, X_c)


def test_solve_tied_pivots_take_the_first_row(engine):
    A, B = R.tied_pivot_matrix()
    LU, X, info = _solve_both(engine, A, B)
    LU_c, X_c, info_c = cport.lu_solve_fma(A, B)
    assert info == info_c == 0
    np.testing.assert_array_equal(LU, LU_c)
    np.testing.assert_array_equal(X, X_c)
    assert R.backward_error(A, X, B) <= R.solve_limit(A, B)[0]
    # ties across the waves and across the 1024 stride: an all-ones first column keeps row 0 where it is
    n = 1100
    A = np.eye(n) * 3.0
    A[:, 0] = 1.0
    A[0, 1:] = 0.5
    LU, X, info = _solve(engine, A, np.ones(n), PAD)
    LU_c, X_c, _ = cport.lu_solve_fma(A, np.ones(n))
    assert info == 0 and np.array_equal(LU[0], A[0])
    np.testing.assert_array_equal(LU, LU_c)
    np.testing.assert_array_equal(X, X_c)


def test_solve_reports_the_singular_column(engine):
    for name, A, B in R.singular_cases():
        n = A.shape[0]
        LU, X, info = _solve_both(engine, A, B)
        LU_c, X_c, info_c = cport.lu_solve_fma(A, B)
        want = int(name.rsplit("_", 1)[1]) + 1 if name.startswith("zero_column") else n
        assert info == info_c == want, name
        np.testing.assert_array_equal(LU, LU_c, err_msg=name)          # the state at the column that has no pivot
        np.testing.assert_array_equal(X, X_c, err_msg=name)
    A = np.full((33, 33), NAN)                  # every `v > best` is false on NaN: column 1 has no pivot; no hang
    LU, X, info = _solve_both(engine, A, np.ones(33))
    assert info == 1 and np.isnan(LU).all() and np.array_equal(X, np.ones(33))


# ---------------------------------------------------------------------------------------------------------
# committors and reactive flux
# ---------------------------------------------------------------------------------------------------------
def _flux(engine, T, pi, role, pad, form="all"):
    """msm_reactive_flux with ldt = n + pad; form: 'q' (committors only), 'flux' (+ gross, net), 'all' (+ totals)."""
    n = T.shape[0]
    Td, pid = engine.to_device(R.pad2d(T, n + pad)), engine.to_device(pi)
    rd = engine.to_device(np.ascontiguousarray(role, np.int32))
    qp, qm = _nan_device(engine, n + 2), _nan_device(engine, n + 2)
    info = _minus_ones(engine, 3)
    gross = net = tot = None
    if form != "q":
        gross, net = _nan_device(engine, n * n + 2), _nan_device(engine, n * n + 2)
        tot = _nan_device(engine, 6) if form == "all" else None
    ptr = lambda a: a.ptr if a is not None else None
    check(lib.msm_reactive_flux(engine.handle, Td.ptr, n + pad, pid.ptr, rd.ptr, n, qp.ptr, qm.ptr, ptr(gross), ptr(net),
                                ptr(tot), info.ptr), engine.handle)
    out = {"qplus": qp.to_host(), "qminus": qm.to_host(), "info": info.to_host()}
    assert np.isnan(out["qplus"][n:]).all() and np.isnan(out["qminus"][n:]).all() and out["info"][2] == -1
    out["qplus"], out["qminus"] = out["qplus"][:n], out["qminus"][:n]
    for name, a, size in (("gross", gross, n * n), ("net", net, n * n), ("totals", tot, 4)):
        if a is not None:
            h = a.to_host()
            assert np.isnan(h[size:]).all(), name
            out[name] = h[:size].reshape((4,) if name == "totals" else (n, n))
    return out


def _check_flux(engine, T, pi, role, reversible, forms=("all",)):
    n = T.shape[0]
    res = _flux(engine, T, pi, role, PAD, "all")
    packed = _flux(engine, T, pi, role, 0, "all")
    for key in ("qplus", "qminus", "gross", "net", "totals", "info"):
        np.testing.assert_array_equal(res[key], packed[key], err_msg=key)
    for form in forms:
        part = _flux(engine, T, pi, role, PAD, form)
        for key in part:
            np.testing.assert_array_equal(part[key], res[key], err_msg=f"{form}: {key}")
    assert not res["info"][:2].any()
    qp, qm = res["qplus"], res["qminus"]
    A, B = role == 1, role == 2
    assert (qp[A] == 0.0).all() and (qp[B] == 1.0).all() and (qm[A] == 1.0).all() and (qm[B] == 0.0).all()
    Wf, rf, Wb, rb = R.committor_systems(T, pi, role)
    for name, W, r, q in (("q+", Wf, rf, qp), ("q-", Wb, rb, qm)):
        limit, ref = R.solve_limit(W, r)
        omega = R.backward_error(W, q, r)
        print(f"flux n={n} {name}: omega(device)={omega / U:.3g} u, omega(LAPACK)={ref / U:.3g} u, limit={limit / U:.3g} u")
        assert omega <= limit
        np.testing.assert_array_equal(q, cport.lu_solve_fma(W, r)[1], err_msg=name)     # the system, bit for bit
    if reversible:
        R.assert_within(qm, 1 - qp.astype(LD), 0.0, "q- = 1 - q+", atol=8 * R.cond_inf(Wb) * n * U)
    # gross: four factors given the device's committors; net: the rounded difference of two such products
    T_, pi_, qp_, qm_ = (np.asarray(v, LD) for v in (T, pi, qp, qm))
    f = (pi_ * qm_)[:, None] * T_ * qp_[None, :]
    np.fill_diagonal(f, 0)
    R.assert_within(res["gross"], f, R.product_bound(4), "gross flux")
    R.assert_within(res["net"], np.maximum(0, f - f.T), 0.0, "net flux", atol=8 * U * np.maximum(f, f.T))
    assert not np.diag(res["gross"]).any() and not np.diag(res["net"]).any()
    tot = res["totals"]
    sel = np.outer(A, ~A)
    R.assert_sum_close(tot[0], res["gross"].astype(LD)[sel].sum(), int(sel.sum()), "total flux")
    # sum_i pi_i q-_i is an fma chain: n terms, n roundings (see the difference norms)
    R.assert_sum_close(tot[1], (pi_ * qm_).sum(), n + 1, "sum pi q-")
    assert tot[2] == tot[0] / tot[1] and tot[3] == tot[1] / tot[0]
    return res


@pytest.mark.parametrize("reversible", [True, False], ids=["reversible", "nonreversible"])
@pytest.mark.parametrize("n", [2, 3, 257, 1025])
def test_reactive_flux_padded(engine, n, reversible):
    if reversible:
        T, pi = R.reversible_chain(n, n)
    else:
        T = R.stochastic(n, n)
        pi = R.stationary_ld(T)
    role = R.roles(n, seed=n if n > 3 else None)
    assert (role == 0).sum() == (n - 2 if n <= 3 else n - 2 - n // 5) and (role == 1).sum() >= 1 <= (role == 2).sum()
    t0 = time.perf_counter()
    _check_flux(engine, T, pi, role, reversible, forms=("q", "flux") if n < 1025 else ())
    print(f"flux n={n}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("n", [3, 17, 64])
def test_reactive_flux_birth_death_closed_form(engine, n):
    T, pi, a, b, pi_ld = R.birth_death(n, n)
    role = R.roles(n)
    res = _check_flux(engine, T, pi, role, True)
    Wf, rf, _, _ = R.committor_systems(T, pi, role)
    limit, _ = R.solve_limit(Wf, rf)
    # forward error of a solve with backward error omega: 2 cond omega / (1 - cond omega) <= 4 cond omega
    R.assert_within(res["qplus"], R.birth_death_qplus(a, pi_ld), 0.0, "q+ (harmonic in the resistances)",
                    atol=4 * R.cond_inf(Wf) * limit)
    assert (np.diff(res["qplus"]) > 0).all()


# ---------------------------------------------------------------------------------------------------------
# lumping
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lump_chain():
    """A dense chain of order 4099 and positive weights (the lumping does not ask for the stationary vector)."""
    rng = np.random.default_rng(4099)
    T = rng.random((4099, 4099))
    return T / T.sum(axis=1, keepdims=True), rng.random(4099) + 0.1


@pytest.mark.parametrize("n,n_macro,empty", [(1, 1, None), (5, 2, None), (70, 63, 7), (70, 65, None), (2051, 2048, None),
                                             (2052, 2049, 1000), (4099, 4096, None)])
def test_lump_macro_padded_every_lds_size(engine, lump_chain, n, n_macro, empty):
    """n_macro > 2048 takes more than 64 KB of dynamic LDS (four waves of n_macro doubles, 128 KB at 4096);
    msm_lump_macro raises the kernel's dynamic-LDS limit before such a launch."""
    T_big, pi_big = lump_chain
    T = np.ascontiguousarray(T_big[:n, :n] / T_big[:n, :n].sum(axis=1, keepdims=True))
    pi = pi_big[:n] / pi_big[:n].sum()
    macro = R.lump_assignment(n, n_macro, n, empty=empty)
    outs = []
    pid, md = engine.to_device(pi), engine.to_device(macro)
    for pad in (PAD, 0):
        Td = engine.to_device(R.pad2d(T, n + pad))
        Tm, pm = _nan_device(engine, n_macro * n_macro + 2), _nan_device(engine, n_macro + 2)
        check(lib.msm_lump_macro(engine.handle, Td.ptr, n + pad, pid.ptr, md.ptr, n, n_macro, Tm.ptr, pm.ptr),
              engine.handle)
        Tm, pm = Tm.to_host(), pm.to_host()
        assert np.isnan(Tm[n_macro * n_macro:]).all() and np.isnan(pm[n_macro:]).all()
        outs.append((Tm[:n_macro * n_macro].reshape(n_macro, n_macro), pm[:n_macro]))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    Tm, pm = outs[0]
    Tm_ref, pm_ref = R.lump_reference(T, pi, macro, n_macro)
    R.assert_within(Tm, Tm_ref, (n + 3) * U, "T_macro")
    R.assert_within(pm, pm_ref, (n + 3) * U, "pi_macro")
    if empty is not None:
        assert not Tm[empty].any() and pm[empty] == 0.0 and not Tm[:, empty].any()


# ---------------------------------------------------------------------------------------------------------
# macrostate mean first-passage times
# ---------------------------------------------------------------------------------------------------------
def _mfpt(engine, T, pad):
    n = T.shape[0]
    Td = engine.to_device(R.pad2d(T, n + pad))
    out, info = _nan_device(engine, n * n + 4), _minus_ones(engine, n + 2)
    check(lib.msm_macro_mfpt(engine.handle, Td.ptr, n + pad, n, out.ptr, info.ptr), engine.handle)
    out, info = out.to_host(), info.to_host()
    assert np.isnan(out[n * n:]).all() and (info[n:] == -1).all()
    return out[:n * n].reshape(n, n), info[:n]


@pytest.mark.parametrize("n", [2, 3, 17, 64])
def test_macro_mfpt_birth_death_closed_form(engine, n):
    T, pi, a, b, pi_ld = R.birth_death(n, n)
    M, info = _mfpt(engine, T, PAD)
    Mp, infop = _mfpt(engine, T, 0)
    np.testing.assert_array_equal(M, Mp)
    np.testing.assert_array_equal(info, infop)
    assert not info.any()
    assert np.isfinite(M).all() and not np.diag(M).any()             # pre-filled with NaN: every entry was written
    assert (M[~np.eye(n, dtype=bool)] > 0).all()
    truth = R.birth_death_mfpt(a, b, pi_ld)
    ref = npport.macro_mfpt(T)
    for t, (A, rhs) in enumerate(R.mfpt_systems(T)):
        keep = np.arange(n) != t
        x = M[keep, t]
        limit, ref_omega = R.solve_limit(A, rhs)
        omega = R.backward_error(A, x, rhs)
        assert omega <= limit, (t, omega / U, ref_omega / U)
        np.testing.assert_array_equal(x, cport.lu_solve_fma(A, rhs)[1], err_msg=f"target {t}")
        # forward error of a solve with backward error omega <= 4 cond omega, against the closed form
        R.assert_within(x, truth[keep, t], 0.0, f"closed form, target {t}",
                        atol=4 * R.cond_inf(A) * limit * float(truth[keep, t].max()))
    dev_err, ref_err = R.rel_dev(M, truth), R.rel_dev(ref, truth)
    print(f"mfpt n={n}: device {dev_err / U:.3g} u, npport {ref_err / U:.3g} u from the closed form")


def test_macro_mfpt_closed_classes_report_singular_targets():
    from pmarlo_amd.device import get_engine
    from pmarlo_amd.markov_state_model.tpt import compute_macro_mfpt

    engine = get_engine()
    for name, T, singular in R.closed_class_chains():
        n = T.shape[0]
        M, info = _mfpt(engine, T, PAD)
        want_info = [cport.lu_solve_fma(A, rhs)[2] for A, rhs in R.mfpt_systems(T)]
        np.testing.assert_array_equal(info, want_info, err_msg=name)        # the column, not just "non-zero"
        assert np.nonzero(info)[0].tolist() == singular, name
        assert not np.diag(M).any()
        got = compute_macro_mfpt(T)
        nan_cols = [t for t in range(n) if np.isnan(got[np.arange(n) != t, t]).all()]
        assert nan_cols == singular and not np.diag(got).any(), name
        fine = [t for t in range(n) if t not in singular]
        assert np.isfinite(got[:, fine]).all()
        want = npport.macro_mfpt(T)
        np.testing.assert_allclose(got[:, fine], want[:, fine], rtol=1e-12)
