"""The numpy restatement of the MBAR contract (tests/_mbar_ref.py), pinned by identities that hold to rounding, and
the rounding bound the GPU tests use, checked on every input they use: the restatement's own fp64 pass must stay
inside it when compared with its 80-bit pass."""
import numpy as np
import pytest

from tests import _mbar_ref as R

LD = np.longdouble


def solved(u, N_k, **kw):
    r = R.solve(u, N_k, **kw)
    r["pass"] = R.mbar_pass(u, N_k, r["f"])
    return r


def test_longdouble_is_wider_than_double():
    assert np.finfo(LD).eps < 1e-18


def test_single_state():
    rng = np.random.default_rng(0)
    u, N_k = R.harmonic(rng, [40])
    r = solved(u, N_k)
    assert r["f"].tolist() == [0.0] and r["n_passes"] == 1 and r["n_iterations"] == 0
    ut = (1.7 * u[0] + 0.3)[None, :]
    ft, w, ess = R.target_weights(ut, r["pass"]["d"])
    want = np.exp(-(ut[0] - u[0]))
    np.testing.assert_allclose(w[0], want / want.sum(), rtol=64 * R.ULP)
    np.testing.assert_allclose(ft[0], -np.log(want.mean()), rtol=0, atol=64 * R.ULP)
    assert 1.0 <= ess[0] <= 40.0


def test_two_states_satisfy_bar():
    """BAR: with x_n = (u_1n - u_0n) - f_1 - ln(N_1 / N_0) and fermi(x) = 1 / (1 + e^x), the sum of fermi(x_n) over state
    0's frames equals the sum of fermi(-x_n) over state 1's (s_1 = 1 split by the state that drew the frame)."""
    rng = np.random.default_rng(1)
    u, N_k = R.harmonic(rng, [70, 45], spacing=0.8)
    f = solved(u, N_k)["f"]
    du = u[1] - u[0]
    M = np.log(N_k[1] / N_k[0])
    fermi = lambda x: 1.0 / (1.0 + np.exp(x))
    lhs = fermi(du[:70] - f[1] - M).sum()
    rhs = fermi(-(du[70:] - f[1] - M)).sum()
    assert abs(lhs - rhs) <= 1e-10 * N_k.sum() * 2


def test_constant_shift_moves_f_and_nothing_else():
    rng = np.random.default_rng(2)
    u, N_k = R.harmonic(rng, [50, 20, 35])
    c = np.array([0.0, 3.25, -1.5])            # f_0 = 0 is the gauge: row 0 is not shifted
    a, b = solved(u, N_k), solved(u + c[:, None], N_k)
    np.testing.assert_allclose(b["f"], a["f"] + c, rtol=0, atol=1e-9)
    np.testing.assert_allclose(b["pass"]["d"], a["pass"]["d"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(b["pass"]["W"], a["pass"]["W"], rtol=1e-9)


def test_duplicated_state_gets_equal_f():
    rng = np.random.default_rng(3)
    u, N_k = R.harmonic(rng, [30, 40, 40])
    u = u.copy()
    u[2] = u[1]                                # states 1 and 2 are one state under two labels
    f = solved(u, N_k)["f"]
    assert abs(f[1] - f[2]) <= 1e-9


def test_target_equal_to_a_sampled_state():
    rng = np.random.default_rng(4)
    u, N_k = R.harmonic(rng, [25, 60, 33])
    r = solved(u, N_k, tol=1e-13)
    ft, w, _ = R.target_weights(u[1:2], r["pass"]["d"])
    assert abs(ft[0] - r["f"][1]) <= 1e-10
    assert abs(r["pass"]["s"][1] - 1.0) <= 1e-10 and abs(w[0].sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("name", R.SOLVER_CASES)
def test_convergence(name):
    u, N_k, _ = R.case(name)
    r = R.solution(name)
    s = R.mbar_pass(u, N_k, r["f"])["s"]
    tol, N = 1e-10, N_k.sum()
    assert (np.abs(s - 1.0) <= tol * N / N_k).all()
    assert r["residual"] <= tol and r["n_passes"] == r["n_iterations"] + 1 <= 12


def test_not_converged_raises():
    u, N_k, _ = R.case("unequal")
    with pytest.raises(R.NotConverged):
        R.solve(u, N_k, maxiter=1)


def test_per_frame_shift_is_what_keeps_the_ladder_accurate():
    """Without the shift the fp64 pass on the ladder leaves the bound the shifted pass keeps."""
    u, N_k, _ = R.case("ladder")
    f = R.fixed_f("ladder")
    fl = f + np.log(N_k)
    a = fl[:, None] - u                          # the unshifted exponent arguments
    M = a.max(axis=0)
    d = M + np.log(np.exp(a - M).sum(axis=0))
    s_plain = np.exp(f[:, None] - u - d[None, :]).sum(axis=1)
    want = R.mbar_pass(u, N_k, f, LD)
    err = float((np.abs(s_plain.astype(LD) - want["s"]) / want["s"]).max())
    assert err > 2 * R.pass_bound(u, N_k, f)
    assert err > 10 * float((np.abs(R.mbar_pass(u, N_k, f)["s"].astype(LD) - want["s"]) / want["s"]).max())


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_rounding_bound_holds_for_the_fp64_restatement(name):
    u, N_k, _ = R.case(name)
    f = R.fixed_f(name)
    R.check_pass(R.mbar_pass(u, N_k, f), R.mbar_pass(u, N_k, f, LD), R.pass_bound(u, N_k, f), len(N_k))


@pytest.mark.parametrize("name", R.F32_CASES)
def test_rounding_bound_holds_on_fp32_rounded_values(name):
    u, N_k, _ = R.case(name)
    u = u.astype(np.float32).astype(np.float64)
    f = R.fixed_f(name, True)
    R.check_pass(R.mbar_pass(u, N_k, f), R.mbar_pass(u, N_k, f, LD), R.pass_bound(u, N_k, f), len(N_k))


@pytest.mark.parametrize("name", R.SOLVER_CASES)
def test_target_weights_stay_inside_their_bound(name):
    u, N_k, _ = R.case(name)
    f = R.solution(name)["f"]
    ut = R.targets(name)
    d64, dld = R.mbar_pass(u, N_k, f)["d"], R.mbar_pass(u, N_k, f, LD)["d"]
    R.check_targets(R.target_weights(ut, d64), R.target_weights(ut, dld, LD), R.target_bound(u, N_k, f, ut, dld))
