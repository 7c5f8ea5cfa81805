"""The count matrix -> transition matrix chain on every launch path: msm_transition_matrix (both modes),
msm_embed_full, msm_matrix_power and msm_reversible_mle against the exact references of tests/_estimation_ref.py.

Strided cases go through the C ABI with ld = n + 3 in NaN-filled buffers: the results must equal the packed call's
bit for bit and the padding of every output must still be NaN (a read past n poisons the result, a write past n
shows in the padding)."""
import ctypes

import numpy as np
import pytest

from oracle import npport
from pmarlo_amd._lib import check, lib
from tests import _estimation_ref as R

pytestmark = pytest.mark.gpu

U, LD, NAN = R.U, R.LD, np.nan


def _nan_device(engine, shape):
    return engine.to_device(np.full(shape, NAN))


# ---------------------------------------------------------------------------------------------------------
# mode 0: one launch, cross-workgroup hand-off of the diagonal
# ---------------------------------------------------------------------------------------------------------
def _poison_next_matrix(engine, k):
    """The engine hands a freed block to the next request of its size: the T the wrapper is about to allocate starts
    as NaN, so an entry the kernels do not write shows."""
    _nan_device(engine, (k, k)).free()


def _check_mode0(engine, C):
    k = C.shape[0]
    Cd = engine.to_device(C)
    _poison_next_matrix(engine, k)
    out = engine.transition_matrix(Cd, mode=0)
    T, rs, dm = out["T"].to_host(), out["rowsum"].to_host(), float(out["diag_mass"].to_host()[0])
    Cf = C.astype(np.float64)
    if C.dtype == np.int64:
        np.testing.assert_array_equal(rs, C.sum(axis=1).astype(np.float64))        # integers below 2^53: exact
    else:
        R.assert_sum_close(rs, C.astype(LD).sum(axis=1), k, "rowsum")
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(rs[:, None] > 0, Cf / rs[:, None], 0.0)                    # correctly rounded division
    np.testing.assert_array_equal(T, want)
    diag = np.diag(T).astype(LD)
    # one lost or stale T_ii >= 0.1 moves the mean by >= 0.1 / k; the bound is (k - 1) u sum|T_ii| / k
    R.assert_sum_close(dm, diag.sum() / k, k, "diag_mass")
    return T, dm


@pytest.mark.parametrize("dtype", [np.int64, np.float64], ids=["i64", "f64"])
@pytest.mark.parametrize("k", [1, 2, 255, 256, 257, 1023, 1025, 2304])
def test_mode0_row_normalise_every_k(engine, k, dtype):
    T, dm = _check_mode0(engine, R.mode0_counts(k, dtype, k))
    assert (np.diag(T) >= 0.1).sum() >= max(1, k // 8)
    if k > 2:
        assert not T[0].any() and not T[k - 1].any()
    # the same with the ends of the diagonal in use: the first and the last entry of the hand-off carry >= 0.1
    T, dm = _check_mode0(engine, R.mode0_counts(k, dtype, k + 1, zero_rows=False))
    assert T[0, 0] >= 0.1 and T[k - 1, k - 1] >= 0.1


def test_mode0_scratch_and_ticket_are_reused(engine):
    """k = 2304 and then k = 257 with another diagonal on the same engine: the second diag_mass is the second
    matrix's (the scratch still holds 2304 entries of the first, the ticket must be back at 0)."""
    _, dm_big = _check_mode0(engine, R.mode0_counts(2304, np.float64, 1))
    C = R.mode0_counts(257, np.int64, 2)
    C[np.arange(257), np.arange(257)] += 2 ** 44               # a diagonal unlike the first matrix's
    C[[0, 256]] = 0
    _, dm_small = _check_mode0(engine, C)
    assert abs(dm_small - dm_big) > 0.1
    _check_mode0(engine, R.mode0_counts(2304, np.int64, 3))  # and back: a ticket left at 257 would end early


# ---------------------------------------------------------------------------------------------------------
# mode 1 (active set, Dirichlet prior) and the embedding
# ---------------------------------------------------------------------------------------------------------
def _check_mode1(engine, C, alpha, eps):
    k = C.shape[0]
    Cd = engine.to_device(C)
    _poison_next_matrix(engine, k)
    out = engine.transition_matrix(Cd, mode=1, alpha=alpha, epsilon=eps)
    T, active, inv = out["T"].to_host(), out["active"].to_host(), out["inv_map"].to_host()
    ka = int(out["n_active"].to_host()[0])
    act_ref, inv_ref, T_ref = R.mode1_reference(C, alpha, eps)
    Ca, act_np = npport.ensure_connected_counts(C, alpha=alpha, epsilon=eps)
    assert ka == act_ref.size == act_np.size
    np.testing.assert_array_equal(active[:ka], act_ref)
    np.testing.assert_array_equal(active[:ka], act_np)
    np.testing.assert_array_equal(inv, inv_ref)
    R.assert_within(T[:ka, :ka], T_ref, 3 * U, "T active block")           # C + alpha, the denominator, the division
    outside = np.ones((k, k), bool)
    outside[:ka, :ka] = False
    assert not T[outside].any()
    # embedding: identity rows on inactive states, exact zeros in inactive columns, the block bit-identical
    pi_act = np.zeros(k)
    pi_act[:ka] = np.arange(1, ka + 1) / max(ka, 1)
    for pa in (pi_act, None):
        T_full, pi_full = engine.embed_full(out["T"], out["inv_map"], engine.to_device(pa) if pa is not None else None)
        T_want, pi_want = R.embed_reference(T, inv_ref, pa)
        np.testing.assert_array_equal(T_full.to_host(), T_want)
        np.testing.assert_array_equal(pi_full.to_host(), pi_want)
    assert not pi_want.any()                                                # the pi_active = None call: all zeros
    return ka, act_ref


@pytest.mark.parametrize("dtype", [np.int64, np.float64], ids=["i64", "f64"])
@pytest.mark.parametrize("k", [1, 40, 1024, 1025, 2049, 3000])
def test_mode1_planted_inactive_states(engine, k, dtype):
    eps = 0.5 if dtype is np.float64 else 1e-12
    C, info = R.mode1_counts(k, dtype, k, epsilon=eps)
    for alpha in (1e-3, 0.5):
        ka, active = _check_mode1(engine, C, alpha, eps)
    if k == 1:
        assert ka == 1
        return
    dead = set(R.mode1_inactive(k).tolist())
    assert {0, k - 1} <= dead and (k <= 1024 or {1023, 1024} <= dead)
    assert info["column_only"] in active
    if dtype is np.float64:
        assert info["at_epsilon"] not in active and info["above_epsilon"] in active
        dead.discard(info["above_epsilon"])
    assert ka == k - len(dead)


@pytest.mark.parametrize("k", [1, 1025, 2049])
def test_mode1_every_state_active_and_none_active(engine, k):
    C, _ = R.mode1_counts(k, np.int64, k, variant="all")
    assert _check_mode1(engine, C, 1e-3, 1e-12)[0] == k
    Z, _ = R.mode1_counts(k, np.float64, k, variant="zero")
    assert _check_mode1(engine, Z, 0.5, 1e-12)[0] == 0


# ---------------------------------------------------------------------------------------------------------
# matrix power: ragged batch, padded ld and stride, both parities of the ping-pong
# ---------------------------------------------------------------------------------------------------------
POWER_ORDERS = [0, 1, 63, 64, 65]
POWER_NMAX = 65


@pytest.fixture(scope="module")
def power_inputs():
    return [R.stochastic(n, 100 + n) if n else np.zeros((0, 0)) for n in POWER_ORDERS]


def _matrix_power(engine, mats, squarings, ld, stride):
    nmax, batch = POWER_NMAX, len(mats)
    src = engine.to_device(R.pad_batch(mats, nmax, nmax, ld, stride))
    dn = engine.to_device(np.asarray(POWER_ORDERS, np.int32))
    scratch, out = _nan_device(engine, batch * stride), _nan_device(engine, batch * stride)
    check(lib.msm_matrix_power(engine.handle, src.ptr, stride, ld, dn.ptr, nmax, batch, squarings, scratch.ptr, out.ptr),
          engine.handle)
    return out.to_host(), scratch.to_host()


@pytest.mark.parametrize("squarings", [1, 2, 3, 4, 5, 6])
def test_matrix_power_ragged_batch_padded(engine, power_inputs, squarings):
    nmax, batch = POWER_NMAX, len(POWER_ORDERS)
    ld, stride = nmax + R.PAD, nmax * (nmax + R.PAD) + 5
    out, scratch = _matrix_power(engine, power_inputs, squarings, ld, stride)
    packed, _ = _matrix_power(engine, power_inputs, squarings, nmax, nmax * nmax)
    pad = R.batch_padding_mask(batch, nmax, nmax, ld, stride)
    assert np.isnan(out[pad]).all() and np.isnan(scratch[pad]).all()
    for b, n in enumerate(POWER_ORDERS):
        got = R.batch_view(out, b, nmax, ld, stride)[:, :nmax]
        np.testing.assert_array_equal(got, R.batch_view(packed, b, nmax, nmax, nmax * nmax))
        outside = np.ones((nmax, nmax), bool)
        outside[:n, :n] = False
        assert not got[outside].any()                              # zeros, not NaN; order 0: the whole matrix
        if n:
            R.assert_within(got[:n, :n], R.power_ld(power_inputs[b], squarings), 0.0, f"order {n}",
                            atol=(2 ** squarings - 1) * n * U)


# ---------------------------------------------------------------------------------------------------------
# reversible maximum-likelihood estimator
# ---------------------------------------------------------------------------------------------------------
def _revmle(engine, Cm, maxerr, maxiter, pad=0):
    """msm_reversible_mle through the C ABI with ld = ldt = n + pad -> (T [n, n + pad], pi, iterations, err)."""
    n = Cm.shape[0]
    Cd = engine.to_device(R.pad2d(Cm, n + pad))
    Td, pid = _nan_device(engine, (n, n + pad)), _nan_device(engine, n)
    it, err = ctypes.c_int(-1), ctypes.c_double(NAN)
    check(lib.msm_reversible_mle(engine.handle, Cd.ptr, n, n + pad, float(maxerr), int(maxiter), Td.ptr, n + pad,
                                 pid.ptr, ctypes.byref(it), ctypes.byref(err)), engine.handle)
    return Td.to_host(), pid.to_host(), it.value, err.value


def _revmle_both_layouts(engine, Cm, maxerr, maxiter):
    n = Cm.shape[0]
    T, pi, it, err = _revmle(engine, Cm, maxerr, maxiter)
    Tp, pip, itp, errp = _revmle(engine, Cm, maxerr, maxiter, pad=R.PAD)
    np.testing.assert_array_equal(Tp[:, :n], T)
    np.testing.assert_array_equal(pip, pi)
    assert np.isnan(Tp[:, n:]).all() and (itp, errp) == (it, err)
    return T, pi, it


@pytest.mark.parametrize("n", [1, 3, 5, 65, 257])
def test_reversible_mle_converged_packed_and_padded(engine, n):
    Cm = R.revmle_counts(n, n)
    T, pi, it = _revmle_both_layouts(engine, Cm, 1e-13, 1_000_000)
    T_ref, pi_ref, _ = npport.reversible_mle(Cm, maxerr=1e-13)
    np.testing.assert_allclose(T, T_ref, rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(pi, pi_ref, rtol=1e-9)
    np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=1e-14)
    if n == 1:
        assert T[0, 0] == 1.0 and pi[0] == 1.0


@pytest.mark.parametrize("maxiter", [1, 33, 97])
@pytest.mark.parametrize("n", [3, 5, 65, 257])
def test_reversible_mle_fixed_iteration_count(engine, n, maxiter):
    """maxerr = 1e-300 never stops the loop: exactly maxiter iterations, also when that ends inside a check interval
    (32, then 64); the iterate then agrees with the longdouble restatement as well as the float64 oracle does.
    (Order 1 is left to the converged test: its iterate is [1] from the start, the error is exactly 0 at the first
    check and the loop rightly ends there.  At these orders the oracle's step is still > 1e-7 after 97 iterations.)"""
    Cm = R.revmle_counts(n, 7 * n)
    T, pi, it = _revmle_both_layouts(engine, Cm, 1e-300, maxiter)
    assert it == maxiter
    T_ld, pi_ld = R.revmle_ld(Cm, maxiter)
    T64, pi64, it64 = npport.reversible_mle(Cm, maxerr=1e-300, maxiter=maxiter)
    for name, got, ref, truth in (("T", T, T64, T_ld), ("pi", pi, pi64, pi_ld)):
        ref_err, dev_err = R.rel_dev(ref, truth), R.rel_dev(got, truth)
        limit = R.rule3_limit(ref_err, 64 * n * U)
        print(f"revmle n={n} it={maxiter} {name}: device {dev_err / U:.3g} u, oracle {ref_err / U:.3g} u, limit {limit / U:.3g} u")
        assert dev_err <= limit


def test_reversible_mle_order_6145_raises_the_lds_limit(engine):
    """n = 6145: 49160 bytes of dynamic LDS (the attribute is raised above 48 KB), 1537 workgroups of which the last
    holds one row.  Three iterations of the banded circulant matrix against the oracle at the same three."""
    n, iters = 6145, 3
    Cm = R.banded_circulant_counts(n)
    T, pi, it, _ = _revmle(engine, Cm, 1e-300, iters)
    assert it == iters
    (r, c, vals), pi_ld = R.revmle_ld(Cm, iters)
    T64, pi64, _ = npport.reversible_mle(Cm, maxerr=1e-300, maxiter=iters)
    assert np.count_nonzero(T) == r.size == 5 * n
    for name, got, ref, truth in (("T", T[r, c], T64[r, c], vals), ("pi", pi, pi64, pi_ld)):
        ref_err, dev_err = R.rel_dev(ref, truth), R.rel_dev(got, truth)
        limit = R.rule3_limit(ref_err, 64 * n * U)
        print(f"revmle n={n} {name}: device {dev_err / U:.3g} u, oracle {ref_err / U:.3g} u, limit {limit / U:.3g} u")
        assert dev_err <= limit


def test_reversible_mle_states_without_counts_keep_a_self_loop(engine):
    n, lone = 23, [4, 17]
    Cm = R.revmle_counts(n, 11)
    Cm[lone, :] = 0.0
    Cm[:, lone] = 0.0
    T, pi, _ = _revmle_both_layouts(engine, Cm, 1e-13, 1_000_000)
    keep = np.setdiff1d(np.arange(n), lone)
    want_rows = np.zeros((2, n))
    want_rows[[0, 1], lone] = 1.0
    np.testing.assert_array_equal(T[lone], want_rows)
    np.testing.assert_array_equal(pi[lone], 0.0)
    assert not T[np.ix_(keep, lone)].any()
    T_ref, pi_ref, _ = npport.reversible_mle(Cm[np.ix_(keep, keep)], maxerr=1e-13)
    np.testing.assert_allclose(T[np.ix_(keep, keep)], T_ref, rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(pi[keep], pi_ref, rtol=1e-9)


def test_reversible_mle_state_with_incoming_counts_only(engine):
    n, s = 19, 6
    Cm = R.revmle_counts(n, 13)
    Cm[s, :] = 0.0                                   # c_s = 0: the state is entered, never left
    T, pi, _ = _revmle_both_layouts(engine, Cm, 1e-13, 1_000_000)
    T_ref, pi_ref, _ = npport.reversible_mle(Cm, maxerr=1e-13)
    assert np.isfinite(T_ref).all() and pi_ref[s] > 0
    np.testing.assert_allclose(T, T_ref, rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(pi, pi_ref, rtol=1e-9)
    np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=1e-14)
    flux = pi[:, None] * T
    np.testing.assert_allclose(flux, flux.T, rtol=1e-9, atol=1e-18)
