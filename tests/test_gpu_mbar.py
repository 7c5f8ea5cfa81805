"""Engine.mbar_pass / mbar_weights (csrc/mbar.hip) and reweight.mbar against the numpy restatement of the contract
(tests/_mbar_ref.py) run in 80-bit floats on the same fp64 (or fp32-rounded) inputs.

Tolerance (derived, not fitted; R.pass_bound, R.check_pass, R.target_bound, R.check_targets):
  bound = n_ops * 2^-52 * A,   n_ops = K + ceil(log2 N) + 32,
  A = max(1, |b_k|, |u_kn - m_n| where that difference is not exact) over the finite entries, with m_n = min_k u_kn the
  per-frame shift and b_k = (f_k - (u_kn - m_n)) + ln N_k the exponent argument after it.  The inner difference is exact
  when u_kn and m_n lie within a factor 2 (Sterbenz: the ladder at |u| = 1.6e4), else it rounds at its own size; the
  outer difference and sum round at the size of the argument.  So an argument carries a few roundings of numbers up to
  A; exp turns that absolute error into the same relative error of W_kn; exp and log of the device math library are good
  to 1 ulp in fp64.  The operations per output are the K terms of the logsumexp, the ceil(log2 N) levels of the sum over
  frames (the device adds four 16-term chains per row and trip, then trips, waves and workgroups: at these shapes every
  chain after the first is shorter than log2 N) and a fixed number around them (the roundings of b, b - M, M + log S,
  the subtraction of m_n, 1 / S, two products, exp and log, the 16-term chain), which 32 covers.  The floor 1 on A is
  there because those last errors are relative to the result whatever the argument.
  d_n: |error| <= bound + 2^-52 |d_n| (absolute; the last term is the subtraction of m_n and the stored number).
  s_k: relative bound.  G_ij: relative, twice the bound (products of two W).
  obj: absolute, sum_n of the d_n bounds + n_ops * 2^-52 * sum_n |d_n| for the summation.
  target weights: the argument c_n - lse, c_n = -u_tn - d_n, adds to the error of the stored d_n one rounding at
  max(|u_tn|, |d_n|) and a logsumexp over N frames, (1 + ceil(log2 N) + 32) operations at max(1, |c_n - lse|).
tests/test_mbar_reference.py holds the restatement's own fp64 pass to the same bounds on the same inputs.

Exact: two calls return the same bits, G is symmetric bit for bit, want_gram = 0 returns the bits of want_gram = 1.

Inputs (R.CASES): the smallest at which each mechanism can fail: K = 1; N on both sides of a wave; K on both sides of
a Gram tile; K = 64; one trip + 1 frame (two workgroups); five trips + 3 frames on two workgroups (grid-stride loop,
ragged tail); rows padded with poison; unequal N_k with a single-frame state; the 8-rung ladder at -4e4 kJ/mol (wrong
without the per-frame shift); +inf entries; fp32 input."""
import functools

import numpy as np
import pytest

from pmarlo_amd import _lib, reweight
from tests import _mbar_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
PASS_CASES = sorted(R.CASES)


@functools.lru_cache(maxsize=None)
def yardstick(name, f32=False):
    """The longdouble pass of a named input at its fixed f, computed once."""
    u, N_k, _ = R.case(name)
    if f32:
        u = u.astype(np.float32).astype(np.float64)
    return R.mbar_pass(u, N_k, R.fixed_f(name, f32), LD)


def device_pass(engine, name, *, f32=False, ld=None, want_gram=True, f=None):
    u, N_k, max_wg = R.case(name)
    K, N = u.shape
    host = u.astype(np.float32) if f32 else u
    if ld is not None:                       # padded rows: what lies past N must never be read
        padded = np.full((K, ld), np.nan, host.dtype)
        padded[:, N + 1::2] = -np.inf
        padded[:, :N] = host
        host = padded
    f = R.fixed_f(name, f32) if f is None else f
    r = engine.mbar_pass(engine.to_device(host), engine.to_device(np.asarray(f, np.float64)),
                         engine.to_device(np.log(N_k.astype(np.float64))), n=N, want_gram=want_gram,
                         max_workgroups=max_wg)
    return {"d": r["logden"].to_host(), "s": r["s"].to_host(), "G": r["G"].to_host() if want_gram else None,
            "obj": float(r["obj"].to_host()[0])}


def check(engine, name, **kw):
    u, N_k, _ = R.case(name)
    f32 = kw.get("f32", False)
    if f32:
        u = u.astype(np.float32).astype(np.float64)
    got = device_pass(engine, name, **kw)
    K, N = u.shape
    assert got["d"].shape == (N,) and got["s"].shape == (K,) and got["G"].shape == (K, K)
    np.testing.assert_array_equal(got["G"], got["G"].T)
    R.check_pass(got, yardstick(name, f32), R.pass_bound(u, N_k, R.fixed_f(name, f32)), K)
    return got


def same_bits(a, b):
    for key in ("d", "s", "obj"):
        assert np.array_equal(np.asarray(a[key]).view(np.uint64), np.asarray(b[key]).view(np.uint64)), key


def test_plan_names_the_launch_shape(engine):
    p = engine.mbar_plan(32, 1_000_000)
    assert p["frames_per_trip"] == R.TRIP == _lib.MBAR_THREADS
    assert p["gram_tiles"] == 3 and 0 < p["lds_bytes"] <= 160 * 1024 and 1 <= p["grid"] <= -(-1_000_000 // R.TRIP)
    assert engine.mbar_plan(64, 1000)["gram_tiles"] == 10 and engine.mbar_plan(64, 1000)["lds_bytes"] <= 160 * 1024
    trip = p["frames_per_trip"]
    assert engine.mbar_plan(3, trip)["grid"] == 1 and engine.mbar_plan(3, trip + 1)["grid"] == 2
    assert engine.mbar_plan(3, 5 * trip + 3, max_workgroups=2)["grid"] == 2
    assert R.CASES["two_wg"][1] == trip + 1 and R.CASES["stride"][1:] == (5 * trip + 3, 2)


@pytest.mark.parametrize("name", PASS_CASES)
def test_pass_matches_the_longdouble_restatement(engine, name):
    got = check(engine, name)
    same_bits(got, device_pass(engine, name))                          # run to run
    again = device_pass(engine, name)
    assert np.array_equal(got["G"].view(np.uint64), again["G"].view(np.uint64))
    same_bits(got, device_pass(engine, name, want_gram=False))         # the line-search pass


def test_padded_rows_are_not_read(engine):
    got = check(engine, "unequal", ld=640)
    same_bits(got, device_pass(engine, "unequal"))


@pytest.mark.parametrize("name", R.F32_CASES)
def test_fp32_input(engine, name):
    check(engine, name, f32=True)
    check(engine, name, f32=True, ld=R.case(name)[0].shape[1] + 3)


def test_ladder_needs_the_shift(engine):
    """The fp64 pass without the per-frame shift leaves the bound on this input (so the device must be shifting)."""
    u, N_k, _ = R.case("ladder")
    f = R.fixed_f("ladder")
    a = (f + np.log(N_k))[:, None] - u
    M = a.max(axis=0)
    d = M + np.log(np.exp(a - M).sum(axis=0))
    s_plain = np.exp(f[:, None] - u - d[None, :]).sum(axis=1)
    want = yardstick("ladder")["s"]
    assert float((np.abs(s_plain.astype(LD) - want) / want).max()) > 2 * R.pass_bound(u, N_k, f)
    check(engine, "ladder")


# ---- errors ------------------------------------------------------------------------------------------------------
def bad_input(engine, poison, where):
    u, N_k, _ = R.case("unequal")
    u = u.copy()
    u[where] = poison
    return engine.to_device(u), engine.to_device(np.zeros(len(N_k))), engine.to_device(np.log(N_k.astype(np.float64)))


@pytest.mark.parametrize("poison", [np.nan, -np.inf])
def test_nan_and_minus_inf_raise(engine, poison):
    u, f, lnN = bad_input(engine, poison, (3, 17))
    with pytest.raises(ValueError, match="NaN or -inf"):
        engine.mbar_pass(u, f, lnN)
    assert engine.mbar_pass(u, f, lnN, check_status=False)["status"] & _lib.MBAR_BAD_INPUT
    with pytest.raises(ValueError, match="NaN or -inf"):
        reweight.mbar(u, R.case("unequal")[1], engine=engine)


def test_frame_forbidden_everywhere_raises(engine):
    u, f, lnN = bad_input(engine, np.inf, (slice(None), 400))
    with pytest.raises(ValueError, match="forbidden"):
        engine.mbar_pass(u, f, lnN)
    assert engine.mbar_pass(u, f, lnN, check_status=False)["status"] == _lib.MBAR_BAD_FRAME
    with pytest.raises(ValueError, match="forbidden"):
        reweight.mbar(u, R.case("unequal")[1], engine=engine)


def test_more_than_64_states_is_unsupported(engine):
    rng = np.random.default_rng(5)
    u, N_k = R.harmonic(rng, np.full(65, 2), spacing=0.1)
    with pytest.raises(NotImplementedError, match="65"):
        engine.mbar_pass(engine.to_device(u), engine.to_device(np.zeros(65)), engine.to_device(np.log(N_k * 1.0)))
    with pytest.raises(NotImplementedError, match="65"):
        reweight.mbar(u, N_k, engine=engine)


def test_counts_are_validated(engine):
    u, N_k, _ = R.case("unequal")
    with pytest.raises(ValueError, match="sums to"):
        reweight.mbar(u, N_k + 1, engine=engine)
    zero = N_k.copy()
    zero[0] += zero[1]
    zero[1] = 0
    with pytest.raises(ValueError, match="needs frames"):
        reweight.mbar(u, zero, engine=engine)


# ---- solver ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solved(engine, name):
    u, N_k, _ = R.case(name)
    return reweight.mbar(u, N_k, targets=R.targets(name), engine=engine)


@pytest.mark.parametrize("name", R.SOLVER_CASES)
def test_solver_takes_the_prescribed_path(engine, name):
    u, N_k, _ = R.case(name)
    res, ref = solved(engine, name), R.solution(name)
    assert res.n_passes == ref["n_passes"] and res.n_iterations == ref["n_iterations"]
    assert res.f_k[0] == 0.0
    want = R.mbar_pass(u, N_k, res.f_k, LD)
    residual = float(np.abs(N_k * (want["s"] - 1)).max() / N_k.sum())
    bound = R.pass_bound(u, N_k, res.f_k)
    print(name, "passes", res.n_passes, "residual", residual, "bound", bound)
    assert residual <= 1e-10 + bound
    err_d = np.abs(res.log_denominator.to_host().astype(LD) - want["d"]).astype(np.float64)
    assert (err_d <= bound + R.ULP * np.abs(want["d"]).astype(np.float64)).all()


@pytest.mark.parametrize("name", R.SOLVER_CASES)
def test_target_weights(engine, name):
    u, N_k, _ = R.case(name)
    res = solved(engine, name)
    ut = R.targets(name)
    d = R.mbar_pass(u, N_k, res.f_k, LD)["d"]
    R.check_targets((res.target_f, res.weights, res.ess), R.target_weights(ut, d, LD),
                    R.target_bound(u, N_k, res.f_k, ut, d))
    N = u.shape[1]
    assert res.weights.shape == (2, N) and (np.abs(res.weights.sum(axis=1) - 1.0) <= N * R.ULP).all()
    assert (res.ess >= 1.0).all() and (res.ess <= N).all()


def test_one_iteration_is_not_enough(engine):
    u, N_k, _ = R.case("unequal")
    with pytest.raises(RuntimeError, match="NOCONV"):
        reweight.mbar(u, N_k, maxiter=1, engine=engine)
