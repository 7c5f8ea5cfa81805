"""Engine.tram_rows / tram_pass / tram_update / tram_solve / tram_transition_matrices (csrc/tram.hip) and
reweight.tram against the numpy restatement of the contract (tests/_tram_ref.py) run in 80-bit floats on the same fp64
(or fp32-rounded) inputs.

Tolerances (derived, not fitted; the derivation is the comment block "the rounding bounds" of tests/_tram_ref.py):
  rows:  relative (chain + 8 + X) 2^-52, X = max |g_j - g_i| over the pairs with S_ij != 0: a term S_ij / (1 + exp(x))
         carries one rounding of x at |x|, which exp turns into a relative error, and one ulp each of exp, 1 + exp, the
         division (and the log behind it); chain = ceil(m / 64) + 7 is the longest run of additions on the device (a lane's
         columns, six shuffle levels, N - col).  ln out + f: that, absolute, plus two roundings at its magnitudes.
  pass:  (K + chain + 16) 2^-52 A, A = max(1, |a_l|, |u_ln - m_n| where that difference is not exact (Sterbenz)),
         a_l = tab_l - (u_ln - m_n) the exponent argument after the per-frame shift; K terms of the sum S, 16 fixed
         roundings, chain = 21 + the units of the fullest state (16-term chains of a wave's row sum, 2 + 3 to join chains
         and waves, then the units in sequence).  s relative; d_n absolute plus one ulp of |d_n|.
  update: f_new = tab - ln s is one log at 1 ulp of |ln s| and one rounding; the gauge subtracts another such entry
         and rounds; g = ln v + f_new adds a log and a rounding: 8 * 2^-52 * max(1, |tab|, |ln s|, |ln v|, |f|).
  one iteration (R.iteration_bound) = 2 (3 rows + pass + 2 * 2^-52 max(1, |tab|, |ln s|, |f|)): the error of v reaches
         ln R through g, twice, on top of ln R's own; the gauge doubles it.
  solve: the device's (f, v) put through one longdouble iteration moves by at most tol + the iteration bound; against
         the longdouble solution f differs by at most (tol + tol + iteration bound) / (1 - rho), rho read off the
         restatement's last error ratios (R.contraction).
  detailed balance: pi_i p_ij is a product of exp(-f_i) / Z and S_ij / (v_i + v_j exp(f_j - f_i)): two exps whose arguments
         round at F = max |f|, a sum, a product, two divisions, the normalisation: (16 + 3 F) 2^-52 of the product.

Exact: two calls return the same bits; max_workgroups = 1, 2 and 0 return the same bits; the pass with and without
d_logden returns the same s; frames passed in a shuffled order give the same weights bit for bit, because
tram_from_counts orders the frames of a state by the ensemble that drew them and their own values before anything
is summed (the grouping is order-free).

Inputs (CASES): the smallest at which each mechanism can fail: K = 1, 2, 64; m = 1; m on both sides of a wave and
beyond one 64-column trip of a row; more rows than one workgroup of the rows launch holds; a state with 1 frame, with
exactly one segment, with one segment + 1 frame, with several segments; inactive pairs; an active state with an
all-zero S row; rows of u padded with poison; +inf entries; fp32 u; the 8-rung ladder at -4e4 kJ/mol (wrong without
the per-frame shift)."""
import functools
import importlib

import numpy as np
import pytest

from pmarlo_amd import _lib, reweight
from tests import _mbar_ref
from tests import _tram_ref as R

pytestmark = pytest.mark.gpu

T = importlib.import_module("pmarlo_amd.reweight.tram")
LD = np.longdouble
SEG = R.SEGMENT

CASES, case, offsets, host_tab = R.CASES, R.case, R.offsets, R.host_tab


def device_pass(engine, name, *, f32=False, ld=None, want_logden=True, max_workgroups=0):
    prob, _, _ = case(name)
    tab, _, _ = host_tab(name, f32)
    K, N = prob["u"].shape
    host = prob["u"].astype(np.float32) if f32 else prob["u"]
    if ld is not None:                       # padded rows: what lies past N must never be read
        padded = np.full((K, ld), np.nan, host.dtype)
        padded[:, N + 1::2] = -np.inf
        padded[:, :N] = host
        host = padded
    tables = engine.tram_tables(offsets(prob))
    r = engine.tram_pass(engine.to_device(np.ascontiguousarray(host)), tables, engine.to_device(tab),
                         want_logden=want_logden, max_workgroups=max_workgroups)
    return {"d": r["logden"].to_host() if want_logden else None, "s": r["s"].to_host()}


def check_pass(engine, name, **kw):
    prob, _, _ = case(name)
    tab, want, u = host_tab(name, kw.get("f32", False))
    got = device_pass(engine, name, **kw)
    assert got["s"].shape == prob["N"].shape and got["d"].shape == (u.shape[1],)
    R.check_pass(got, want, R.pass_bound(u, prob["state"], tab, R.pass_chain_device(prob["state"], tab.shape[1])))
    return got


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_plan_names_the_launch_shape(engine):
    off = [0, 1, 1 + SEG, 2 + 2 * SEG, 2 + 2 * SEG + 3 * SEG]
    p = engine.tram_plan(32, off)
    assert p["segment"] == SEG == _lib.TRAM_SEGMENT and p["units"] == 1 + 1 + 2 + 3 and p["grid"] == 7
    assert 0 < p["lds_bytes"] <= 160 * 1024 and p["rows_grid"] == 32 * 4 // 4
    assert engine.tram_plan(32, off, max_workgroups=2)["grid"] == 2
    big = engine.tram_plan(_lib.MBAR_MAX_K, np.arange(_lib.TRAM_MAX_STATES + 1))
    assert big["lds_bytes"] <= 160 * 1024 and big["units"] == _lib.TRAM_MAX_STATES
    assert engine.tram_tables(off)["units"] == p["units"]
    with pytest.raises(NotImplementedError, match="65"):
        engine.tram_plan(65, off)
    with pytest.raises(NotImplementedError, match=str(_lib.TRAM_MAX_STATES + 1)):
        engine.tram_plan(2, np.arange(_lib.TRAM_MAX_STATES + 2))
    with pytest.raises(ValueError, match="no frames"):
        engine.tram_plan(2, [0, 4, 4, 9])


@pytest.mark.parametrize("name", sorted(CASES))
def test_rows_match_the_longdouble_restatement(engine, name):
    prob, f, v = case(name)
    m = f.shape[1]
    S, N, col, f_d = (engine.to_device(a) for a in (prob["S"], prob["N"], prob["col"], f))
    g = R.log_multipliers(f, v)
    for mode in ("multipliers", "counts"):
        out, lnout = engine.tram_rows(S, engine.to_device(g), f_d, N, col, mode)
        got = (out.to_host(), lnout.to_host())
        R.check_rows(got, R.rows(prob["S"], g, f, prob["N"], prob["col"], mode, LD),
                     R.rows_bound(prob["S"], g, R.rows_chain_device(m)), f)
        again = engine.tram_rows(S, engine.to_device(g), f_d, N, col, mode)
        assert np.array_equal(bits(got[0]), bits(again[0].to_host())) and np.array_equal(bits(got[1]), bits(again[1].to_host()))
        assert (got[0][prob["N"] == 0] == 0).all() and np.isneginf(got[1][prob["N"] == 0]).all()
    if name not in ("k1_m1", "k2_m1", "ladder"):           # the active state with an all-zero S row: v = 0, R = N
        k, i = 0, int(np.nonzero(prob["N"][0] > 0)[0][0])
        assert (prob["S"][k, i] == 0).all() and prob["N"][k, i] > 0
        assert engine.tram_rows(S, engine.to_device(g), f_d, N, col, "multipliers")[0].to_host()[k, i] == 0.0
        assert engine.tram_rows(S, engine.to_device(g), f_d, N, col, "counts")[0].to_host()[k, i] == prob["N"][k, i]


@pytest.mark.parametrize("name", sorted(CASES))
def test_pass_matches_the_longdouble_restatement(engine, name):
    got = check_pass(engine, name)
    again = device_pass(engine, name)
    assert np.array_equal(bits(got["s"]), bits(again["s"])) and np.array_equal(bits(got["d"]), bits(again["d"]))
    assert np.array_equal(bits(got["s"]), bits(device_pass(engine, name, want_logden=False)["s"]))


@pytest.mark.parametrize("name", ["segments", "k3_m130", "k64_m5"])
def test_pass_does_not_depend_on_the_grid(engine, name):
    base = device_pass(engine, name)
    for max_wg in (1, 2):
        got = device_pass(engine, name, max_workgroups=max_wg)
        assert np.array_equal(bits(got["s"]), bits(base["s"])) and np.array_equal(bits(got["d"]), bits(base["d"]))


def test_padded_rows_are_not_read(engine):
    got = check_pass(engine, "segments", ld=case("segments")[0]["u"].shape[1] + 131)
    assert np.array_equal(bits(got["s"]), bits(device_pass(engine, "segments")["s"]))


@pytest.mark.parametrize("name", ["segments", "k2_m65", "ladder"])
def test_fp32_input(engine, name):
    check_pass(engine, name, f32=True)
    check_pass(engine, name, f32=True, ld=case(name)[0]["u"].shape[1] + 3)


def test_ladder_needs_the_shift(engine):
    """The fp64 pass without the per-frame shift leaves the bound on this input (so the device must be shifting)."""
    prob, _, _ = case("ladder")
    tab, want, u = host_tab("ladder")
    a = tab[:, prob["state"]] - u
    M = a.max(axis=0)
    r = np.exp(a - M) / np.exp(a - M).sum(axis=0)
    s_plain = np.stack([np.bincount(prob["state"], weights=r[k], minlength=4) for k in range(8)])
    big = want["s"] > 0
    bound = R.pass_bound(u, prob["state"], tab, R.pass_chain_device(prob["state"], 4))
    assert float((np.abs(s_plain.astype(LD) - want["s"])[big] / want["s"][big]).max()) > 2 * bound
    check_pass(engine, "ladder")


@pytest.mark.parametrize("name", ["segments", "k2_m65", "inf"])
def test_update_matches_the_longdouble_restatement(engine, name):
    prob, f, _ = case(name)
    tab, want, _ = host_tab(name)
    g0 = R.log_multipliers(f, case(name)[2])
    v1, _ = R.rows(prob["S"], g0, f, prob["N"], prob["col"], "multipliers")
    s = want["s"].astype(np.float64)
    f_d = engine.to_device(f)
    g_d, err_d = engine.tram_update(engine.to_device(prob["N"]), engine.to_device(tab), engine.to_device(s),
                                    engine.to_device(v1), f_d)
    fn, gn, err = R.update(prob["N"], tab, s, v1, f, LD)
    act = prob["N"] > 0
    with np.errstate(divide="ignore"):
        mag = max(1.0, np.abs(tab[act]).max(), np.abs(np.log(s[act])).max(), np.abs(f[act]).max(),
                  np.abs(np.log(v1[act & (v1 > 0)])).max())
    tol = 8 * R.ULP * mag
    got_f, got_g = f_d.to_host(), g_d.to_host()
    assert float(np.abs(got_f[act].astype(LD) - fn[act]).max()) <= tol and got_f[act].min() == 0.0
    assert np.array_equal(got_f[~act], f[~act])
    live = act & (v1 > 0)
    assert float(np.abs(got_g[live].astype(LD) - gn[live]).max()) <= 2 * tol and np.isneginf(got_g[~live]).all()
    assert abs(float(err_d.to_host()[0]) - err) <= 2 * tol


# ---- errors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [np.nan, -np.inf])
def test_nan_and_minus_inf_are_flagged(engine, poison):
    prob, _, _ = case("segments")
    tab, _, _ = host_tab("segments")
    u = prob["u"].copy()
    u[1, SEG + 7] = poison
    tables = engine.tram_tables(offsets(prob))
    with pytest.raises(ValueError, match="NaN or -inf"):
        engine.tram_pass(engine.to_device(u), tables, engine.to_device(tab))
    r = engine.tram_pass(engine.to_device(u), tables, engine.to_device(tab), check_status=False)
    assert r["status"] & _lib.MBAR_BAD_INPUT
    with pytest.raises(ValueError, match="NaN"):
        reweight.tram_from_counts(prob["C"], u, prob["state"], prob["thermo"], engine=engine)


def test_frame_forbidden_where_it_was_drawn_is_flagged(engine):
    """State 0 of `segments` has one frame; +inf in every ensemble active there leaves it without a finite term."""
    prob, _, _ = case("segments")
    tab, _, _ = host_tab("segments")
    u = prob["u"].copy()
    u[prob["N"][:, 0] > 0, 0] = np.inf
    tables = engine.tram_tables(offsets(prob))
    r = engine.tram_pass(engine.to_device(u), tables, engine.to_device(tab), check_status=False)
    assert r["status"] == _lib.MBAR_BAD_FRAME and np.isneginf(r["logden"].to_host()[0])
    assert (r["s"].to_host()[:, 0] == 0).all()
    with pytest.raises(ValueError, match="forbidden"):
        engine.tram_pass(engine.to_device(u), tables, engine.to_device(tab))


def test_inputs_are_validated(engine):
    prob, _ = R.state_only_case()
    C, u, state, thermo = prob["C"], prob["u"], prob["state"], prob["thermo"]
    call = functools.partial(reweight.tram_from_counts, engine=engine)
    with pytest.raises(ValueError, match="has no frames"):
        call(np.pad(C, ((0, 0), (0, 1), (0, 1))), u, state, thermo)
    with pytest.raises(ValueError, match="transitions into"):
        call(C * 3.0, u, state, thermo)
    extra = C.copy()
    extra[0, 3, 0] = 0.5                                     # ensemble 0 never drew state 3
    with pytest.raises(ValueError, match="drew no frame"):
        call(extra, u, state, thermo)
    neg = C.copy()
    neg[1, 0, 1] = -1.0
    with pytest.raises(ValueError, match="not negative"):
        call(neg, u, state, thermo)
    with pytest.raises(ValueError, match="shapes do not match"):
        call(C, u[:, :-1], state, thermo)
    with pytest.raises(ValueError, match="shapes do not match"):
        call(C[:2], u, state, thermo)
    with pytest.raises(ValueError, match="shape"):
        call(C[:, :, :4], u, state, thermo)
    with pytest.raises(ValueError, match="targets"):
        call(C, u, state, thermo, targets=np.zeros((1, 3)))
    with pytest.raises(_lib.MsmError, match="NOCONV"):
        call(C, u, state, thermo, maxiter=16)


# ---- solver ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solved(engine, name):
    prob, targets = R.solve_case(name)
    return reweight.tram_from_counts(prob["C"], prob["u"], prob["state"], prob["thermo"], targets=targets, engine=engine)


def device_state(res):
    return res._device["f"].to_host(), res._device["v"].to_host()


@pytest.mark.parametrize("name", R.SOLVE_CASES)
def test_solution_is_a_fixed_point_of_the_restatement(engine, name):
    prob, _ = R.solve_case(name)
    res = solved(engine, name)
    ref = R.solution(name)
    f, v = device_state(res)
    m = f.shape[1]
    bound = R.iteration_bound(prob, f, v, R.rows_chain_device(m), R.pass_chain_device(prob["state"], m))
    _, _, err, _ = R.iteration(prob, f, v, LD)
    rho = R.contraction(ref["history"])
    print(name, "iterations", res.n_iterations, "(restatement", ref["n_iterations"], ") err", res.err, "one more step",
          err, "bound", bound, "rho", rho)
    assert res.n_iterations % 16 == 0 and res.err <= 1e-10
    assert err <= 1e-10 + bound
    act = prob["N"] > 0
    diff = float(np.abs(f[act].astype(LD) - ref["f"][act]).max())
    print(name, "f against the longdouble solution", diff, "allowed", (2e-10 + bound) / (1 - rho))
    assert diff <= (1e-10 + 1e-10 + bound) / (1 - rho)
    assert np.isnan(res.f_ik[~act]).all() and np.array_equal(res.f_ik[act], f[act]) and res.f_ik[act].min() == 0.0
    assert np.array_equal(res.state_counts, prob["N"])
    want_fk = -np.log(np.where(act, np.exp(-np.where(act, f, 0.0)), 0.0).sum(axis=1))
    assert np.abs(res.f_k - want_fk).max() <= 8 * R.ULP * max(1.0, np.abs(want_fk).max())


@pytest.mark.parametrize("name", R.TARGET_CASES)
def test_target_weights(engine, name):
    prob, targets = R.solve_case(name)
    res = solved(engine, name)
    N = prob["u"].shape[1]
    assert res.weights.shape == (targets.shape[0], N)
    assert (np.abs(res.weights.sum(axis=1) - 1.0) <= N * R.ULP).all() and (res.weights >= 0).all()
    assert (res.ess >= 1.0).all() and (res.ess <= N).all()
    d = -res.log_mu.to_host()
    want = _mbar_ref.target_weights(targets, d, LD)
    # the stored d_n is the input on both sides: what is left is the logsumexp over N frames of arguments c_n - lse
    with np.errstate(divide="ignore"):
        arg = max(1.0, float(np.abs(np.log(want[1][want[1] > 0])).max()))
    bound = 2 * R.ULP * max(np.abs(d).max(), np.abs(targets).max()) + _mbar_ref.n_ops(1, N) * R.ULP * arg
    _mbar_ref.check_targets((res.target_f, res.weights, res.ess), want, bound)
    m = prob["N"].shape[1]
    fs = R.target_state_f(targets, d, prob["state"], m, LD)
    assert float(np.abs(res.target_state_f - fs).max()) <= bound + (m + 4) * R.ULP * max(1.0, float(np.abs(fs).max()))
    if name == "state_only":
        pi = R.state_only_case()[1]
        pop = np.array([res.weights[0][prob["state"] == i].sum() for i in range(m)])
        rho = R.contraction(R.solution(name)["history"])
        assert np.abs(np.log(pop) - np.log(pi)).max() <= (1e-10 + 0.0) / (1 - rho) + bound


@pytest.mark.parametrize("name", R.SOLVE_CASES)
def test_markov_models_are_reversible(engine, name):
    prob, _ = R.solve_case(name)
    res = solved(engine, name)
    f, v = device_state(res)
    K, m = f.shape
    all_P = engine.tram_transition_matrices(res._device["S"], res._device["N"], res._device["f"], res._device["v"]).to_host()
    for k in range(K):
        est = res.msm(k)
        P, pi = est.transition_matrix, est.stationary_distribution
        assert P.shape == (m, m) and np.abs(P.sum(axis=1) - 1.0).max() <= 1e-12 and (P >= 0).all()
        act = prob["N"][k] > 0
        assert np.array_equal(est.active, np.nonzero(act)[0]) and np.array_equal(P[np.ix_(act, act)], all_P[k][np.ix_(act, act)])
        assert np.array_equal(P[~act][:, ~act], np.eye(int((~act).sum()))) and (pi[~act] == 0).all()
        assert abs(pi.sum() - 1.0) <= m * R.ULP
        flux = pi[:, None] * P
        F = float(np.abs(f[k][act]).max())
        assert (np.abs(flux - flux.T) <= (16 + 3 * F) * R.ULP * np.maximum(flux, flux.T)).all()
        want = R.transition_matrix(prob["S"], prob["N"], f, v, k, LD)
        # an entry: exp at an argument rounded at F, the sum, the division; the diagonal sums m of them
        assert float(np.abs(P.astype(LD) - want)[np.ix_(act, act)].max()) <= (m + 8 + 2 * F) * R.ULP
        assert (all_P[k][~act] == 0).all() and (all_P[k][:, ~act] == 0).all()


def test_unconverged_matrices_are_scaled_to_stay_stochastic(engine):
    """At the start (f = 0, v = S row sums / 2) short rows can exceed 1: dividing by the largest row sum keeps P >= 0."""
    prob, _ = R.solve_case("umbrella_small")
    f, v = R.start(prob)
    v = v * 0.05
    P = engine.tram_transition_matrices(*(engine.to_device(a) for a in (prob["S"], prob["N"], f, v))).to_host()
    for k in range(P.shape[0]):
        want = R.transition_matrix(prob["S"], prob["N"], f, v, k, LD)
        assert want.sum(axis=1).max() <= 1 + 1e-15 and (np.diag(want) >= -1e-15).all() and (np.diag(want) < 1e-12).any()
        assert float(np.abs(P[k].astype(LD) - want).max()) <= (P.shape[1] + 10) * R.ULP


def test_solver_reads_one_word_per_interval(engine):
    prob, _ = R.solve_case("state_only")
    a = reweight.tram_from_counts(prob["C"], prob["u"], prob["state"], prob["thermo"], engine=engine, check_every=16, tol=1e-8)
    b = reweight.tram_from_counts(prob["C"], prob["u"], prob["state"], prob["thermo"], engine=engine, check_every=1, tol=1e-8)
    ref = R.solve(prob, tol=1e-8, check_every=1)
    assert a.n_iterations % 16 == 0 and a.n_iterations - 16 < b.n_iterations <= a.n_iterations
    assert abs(b.n_iterations - ref["n_iterations"]) <= 1          # err crosses tol within a rounding of the same step
    again = reweight.tram_from_counts(prob["C"], prob["u"], prob["state"], prob["thermo"], engine=engine, tol=1e-8)
    assert np.array_equal(bits(again.f_ik), bits(a.f_ik)) and np.array_equal(bits(again.log_v), bits(a.log_v))


def test_f0_starts_from_mbar(engine):
    prob, N_k = R.mbar_limit_case()
    mb = reweight.mbar(prob["u"], N_k, engine=engine)
    cold = solved(engine, "mbar_limit")
    warm = reweight.tram_from_counts(prob["C"], prob["u"], prob["state"], prob["thermo"], f0=mb.f_k, engine=engine)
    assert warm.n_iterations == 16 < cold.n_iterations
    assert np.abs(warm.f_ik - cold.f_ik).max() <= 4e-10 / (1 - R.contraction(R.solution("mbar_limit")["history"]))
    with pytest.raises(ValueError, match="f0"):
        reweight.tram_from_counts(prob["C"], prob["u"], prob["state"], prob["thermo"], f0=[0.0], engine=engine)


# ---- API ---------------------------------------------------------------------------------------------------------
def hopping_trajectories():
    """The small umbrella run recut so that two replicas swap windows half way, plus a side state visited once."""
    _, dtrajs, ttrajs, ublocks, target = R.umbrella_case()
    h = dtrajs[0].size // 2
    swap = lambda a, b, axis=0: np.concatenate([np.take(a, range(h), axis), np.take(b, range(h, 2 * h), axis)], axis)
    d = [swap(dtrajs[0], dtrajs[1]), swap(dtrajs[1], dtrajs[0]), dtrajs[2].copy()]
    t = [swap(ttrajs[0], ttrajs[1]), swap(ttrajs[1], ttrajs[0]), ttrajs[2].copy()]
    u = [swap(ublocks[0], ublocks[1], 1), swap(ublocks[1], ublocks[0], 1), ublocks[2]]
    n = int(max(x.max() for x in d)) + 1
    d[2][-1] = n                                # entered at the last frame, never left: outside the connected set
    d[2][10] = -1                               # an unassigned frame
    cols = np.concatenate([np.arange(h), 2 * h + np.arange(h, 2 * h), 2 * h + np.arange(h), np.arange(h, 2 * h),
                           4 * h + np.arange(2 * h)])
    return d, t, u, target[:, cols], n + 2       # one more state nobody visits


def test_tram_equals_tram_from_counts_on_numpy_counts(engine):
    d, t, u, target, n_states = hopping_trajectories()
    res = reweight.tram(d, t, u, 1, n_markov_states=n_states, targets=target, engine=engine)
    labels, thermo, U = np.concatenate(d), np.concatenate(t), np.concatenate(u, axis=1)
    C0 = R.counts_from_trajs(d, t, 3, n_states, 1)
    active = T.largest_connected_set(C0.sum(axis=0), np.bincount(labels[labels >= 0], minlength=n_states))
    assert np.array_equal(res.active_set, active) and active.size == n_states - 2
    lab = T.restrict_labels(labels, active, n_states)
    C = R.counts_from_trajs(np.split(lab, [d[0].size, 2 * d[0].size]), t, 3, active.size, 1)
    assert np.array_equal(res.count_matrices, C)
    keep = lab >= 0
    assert (~keep).sum() == 2
    ref = reweight.tram_from_counts(C, U[:, keep], lab[keep], thermo[keep], targets=target[:, keep], engine=engine)
    assert np.array_equal(bits(res.f_ik), bits(ref.f_ik)) and res.n_iterations == ref.n_iterations
    assert np.array_equal(bits(res.weights[:, keep]), bits(ref.weights)) and (res.weights[:, ~keep] == 0).all()
    assert np.isneginf(res.log_mu.to_host()[~keep]).all()
    est = res.msm(0)
    assert est.transition_matrix.shape == (n_states, n_states) and np.array_equal(est.active, active[res.state_counts[0] > 0])
    assert est.transition_matrix[n_states - 1, n_states - 1] == 1.0 and est.stationary_distribution[n_states - 2] == 0.0
    # a list of blocks and one matrix are the same input
    one = reweight.tram(d, t, U, 1, n_markov_states=n_states, targets=target, engine=engine)
    assert np.array_equal(bits(one.weights), bits(res.weights))


def test_frame_order_does_not_change_a_bit(engine):
    prob, target = R.solve_case("umbrella_small")
    base = solved(engine, "umbrella_small")
    perm = np.random.default_rng(41).permutation(prob["state"].size)
    res = reweight.tram_from_counts(prob["C"], prob["u"][:, perm], prob["state"][perm], prob["thermo"][perm],
                                    targets=target[:, perm], engine=engine)
    assert np.array_equal(bits(res.f_ik), bits(base.f_ik))
    assert np.array_equal(bits(res.weights), bits(base.weights[:, perm]))
    assert np.array_equal(bits(res.log_mu.to_host()), bits(base.log_mu.to_host()[perm]))


def ladder_dataset():
    rng = np.random.default_rng(51)
    temps = np.array([300.0, 306.0, 312.0])
    E, idx = _mbar_ref.ladder_energies(rng, temps, 300, offset=-1.0e3)
    perm = np.concatenate([rng.permutation(300) + 300 * k for k in range(3)])
    E, idx = E[perm], idx[perm]
    dtraj = np.digitize(E, np.quantile(E, [0.2, 0.4, 0.6, 0.8]))
    hop = idx[300:600].copy()
    hop[150:] = 2                                  # the second split hops to the top rung half way
    splits = {
        "a": {"energy": E[:300], "temperature_K": 300.0, "dtraj": dtraj[:300]},
        "b": {"energy": E[300:600], "state_index": hop, "dtraj": dtraj[300:600]},
        "c": {"energy": E[600:], "temperature_K": 312.0, "dtraj": dtraj[600:]},
    }
    ttrajs = [np.zeros(300, np.int64), hop, np.full(300, 2)]
    return {"splits": splits, "temperatures_K": temps.copy()}, E, temps, [dtraj[:300], dtraj[300:600], dtraj[600:]], ttrajs


def test_reweighter_tram_writes_the_weights_of_the_explicit_call(engine):
    dataset, E, temps, dtrajs, ttrajs = ladder_dataset()
    rw = reweight.Reweighter(303.0, mode="TRAM", lag=2, engine=engine)
    out = rw.apply(dataset)
    E_d = engine.to_device(E)
    u = engine.mbar_reduced_potentials(E_d, 1.0 / (R.KB * temps))
    ut = engine.mbar_reduced_potentials(E_d, [1.0 / (R.KB * 303.0)])
    ref = reweight.tram(dtrajs, ttrajs, u, 2, targets=ut, engine=engine)
    assert np.array_equal(bits(np.concatenate([out[k] for k in ("a", "b", "c")])), bits(ref.weights[0]))
    assert isinstance(rw.result, reweight.TRAMResult) and rw.result.n_iterations == ref.n_iterations
    assert set(dataset["frame_weights"]) == {"a", "b", "c"} and abs(sum(w.sum() for w in out.values()) - 1.0) <= 900 * R.ULP
    assert out["a"].sum() > out["c"].sum()        # frames near the reference temperature weigh more
    with pytest.raises(ValueError, match="lag"):
        reweight.Reweighter(303.0, mode="TRAM")
    with pytest.raises(ValueError, match="mode"):
        reweight.Reweighter(303.0, mode="WHAM")
    del dataset["splits"]["b"]["dtraj"]
    with pytest.raises(ValueError, match="dtraj"):
        rw.apply(dataset)


def test_reweighter_mbar_mode_is_unchanged(engine):
    dataset, E, temps, _, ttrajs = ladder_dataset()
    out = reweight.Reweighter(303.0, engine=engine).apply(dataset)
    named = reweight.Reweighter(303.0, mode="MBAR", engine=engine).apply(dataset)
    joint = reweight.temperature_weights(E, np.concatenate(ttrajs), temps, 303.0, engine=engine)
    got = np.concatenate([out[k] for k in ("a", "b", "c")])
    assert np.array_equal(bits(got), bits(joint)) and np.array_equal(bits(got), bits(np.concatenate([named[k] for k in "abc"])))
