"""Engine.hmm_* (csrc/hmm.hip) and markov_state_model.hmm against the numpy restatement of the contract
(tests/_hmm_ref.py) run in 80-bit floats on the same fp64 inputs.

Tolerances are derived, not fitted; the derivation of the E-step's depths is the comment block "rounding bounds" of
tests/_hmm_ref.py (depth_gamma, depth_C, depth_gamma0, depth_E, bound_logL).  The M-step, given the device's own C, E
and gamma0:
  B       a row sum of k terms is ceil(k / 256) additions of a thread, six shuffle levels and four waves; the
          quotient: ceil(k / 256) + 11
  A       row-normalised: n - 1 additions and the quotient: n.  Reversible: an entry f_ij / sum_j f_ij with
          f_ij = (c_ij + c_ji) / (c_i / x_i + c_j / x_j) is 2 n + 4 roundings from the device's own x; f is symmetric
          bit for bit, and x_i / sum_j f_ij differs from a constant by the stopping measure, so detailed balance holds
          within (2.1 maxerr + 16 ulp) of the flux; a sweep from the device's x moves it by at most maxerr plus the
          2 n + 8 roundings of a sweep
  p0      gamma0 / Q: 1
  pi      Grassmann-Taksar-Heyman has no subtraction: a stage adds at most n + 2 roundings to an entry, n - 1 stages,
          then an n-term dot product per component and the normalisation: n (n - 1)(n + 2) + n n + n + 1
One EM iteration = the E-step depth of the quantity plus the M-step depth of what is made of it; nothing is claimed
about the compounded error of a fit.

Exact: the case where every symbol has one hidden state (gamma is 0 / 1, C the integer lag counts of the lumped
labels); two calls; max_workgroups 0, 1, 2; lag 3 against lag 1 on the three pre-strided pieces (C and logL).

CASES (tests/_hmm_ref.py and below) are the smallest shapes at which each mechanism can fail: n = 1, 2, 3, 16; k = 1,
3, 63, 65, 130; sequence lengths 1, 2, L, L + 1, L + 2, 2 L + 1, 3 L + 5, mixed in one call; lag 1 and 3 on
trajectories of lengths that are no multiple of the lag, one shorter than the lag, one split by -1; a symbol never
observed; symbols with 1, 256 and 257 frames; zeros in A and B; a sequence of probability 0; 3 L steps with every
emission <= 1e-3; labels padded with poison past N."""
import functools

import numpy as np
import pytest

from pmarlo_amd import _lib
from pmarlo_amd.markov_state_model import hmm as H
from tests import _hmm_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
L = R.L
MAXERR = 1e-8


def _lag_case():
    rng = np.random.default_rng(5)
    A, B, p0 = R.random_model(2, 3, 11)
    dtrajs = [R.sample_labels(A, B, p0, T, 50 + i) for i, T in enumerate((3 * L + 5, 2, 100, L + 2))]
    dtrajs[2][37] = -1
    return A, B, p0, dtrajs, rng


def _special(name):
    """-> A, B, p0, labels, table, k"""
    if name in ("lag1", "lag3"):
        A, B, p0, dtrajs, _ = _lag_case()
        labels, table = H.lag_observations(dtrajs, 1 if name == "lag1" else 3, 3)
        return A, B, p0, labels, table, 3
    if name == "unseen_symbol":
        A, B, p0 = R.random_model(2, 4, 21)
        labels = R.sample_labels(A, B, p0, L + 7, 1)
        labels[labels == 3] = 1
        return A, B, p0, labels, R.single_rows([L + 7]), 4
    if name == "member_counts":                     # symbols with 1, 256 and 257 member frames
        A, B, p0 = R.random_model(2, 4, 22)
        labels = np.concatenate([np.full(1, 0), np.full(256, 1), np.full(257, 2), np.full(100, 3)]).astype(np.int32)
        np.random.default_rng(2).shuffle(labels)
        return A, B, p0, labels, R.single_rows([300, len(labels) - 300]), 4
    if name == "tiny_emissions":
        A, B, p0 = R.random_model(2, 3, 23)
        return A, B * 1e-3, p0, R.sample_labels(A, B, p0, 3 * L, 3), R.single_rows([3 * L]), 3
    raise KeyError(name)


SPECIAL = ["lag1", "lag3", "unseen_symbol", "member_counts", "tiny_emissions"]
ALL = sorted(R.CASES) + SPECIAL


@functools.lru_cache(maxsize=None)
def inputs(name):
    return R.case_inputs(name) if name in R.CASES else _special(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    A, B, p0, labels, table, k = inputs(name)
    return R.estep(A, B, p0, labels, table, k, LD)


def device_estep(engine, name, max_workgroups=0, poison=0):
    A, B, p0, labels, table, k = inputs(name)
    host = labels
    if poison:                                      # what lies past N must never be read
        host = np.concatenate([labels, np.full(poison, 2 ** 31 - 1, np.int32)])
        host[len(labels) + 1::2] = -7
    tables = engine.hmm_tables(engine.to_device(host), k, table, n=len(labels))
    out = engine.hmm_estep(tables, engine.to_device(A), engine.to_device(B), engine.to_device(p0),
                           max_workgroups=max_workgroups)
    return {key: (v.to_host() if hasattr(v, "to_host") else v) for key, v in out.items()}, tables


def check_estep(name, got):
    A, B, p0, labels, table, k = inputs(name)
    want = reference(name)
    n, lengths = A.shape[0], [int(x) for x in table[:, 2]]
    assert got["status"] == 0 and want["status"] == 0
    assert not np.isnan(got["gamma"]).any()
    R.check_close(got["gamma"], want["gamma"], R.depth_gamma(max(lengths), n), f"{name} gamma")
    R.check_close(got["C"], want["C"], R.depth_C(lengths, n), f"{name} C")
    R.check_close(got["gamma0"], want["gamma0"], R.depth_gamma0(lengths, n), f"{name} gamma0")
    members = int(np.bincount(labels[(labels >= 0) & (labels < k)], minlength=k).max())
    R.check_close(got["E"], want["E"], R.depth_E(lengths, n, members), f"{name} E")
    for q, T in enumerate(lengths):
        bound = R.bound_logL(T, n, want["S"][q])
        err = abs(float(LD(got["logL"][q]) - want["logL"][q]))
        print(f"{name} logL[{q}]: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    total = float(np.sum(want["logL"]))
    assert abs(got["total"] - total) <= sum(R.bound_logL(T, n, s) for T, s in zip(lengths, want["S"])) + \
        len(lengths) * R.ULP * float(np.sum(np.abs(want["logL"])))


def test_plan_and_limits(engine):
    plan = engine.hmm_plan(16, 1000, 3)
    assert plan["chunk"] == L == _lib.HMM_CHUNK and plan["padded_n"] == 16 and plan["n_chunks"] == 1000
    assert max(plan["product_lds_bytes"], plan["pass_lds_bytes"], plan["emission_lds_bytes"]) <= 160 * 1024
    assert engine.hmm_plan(3, 1000, 3)["padded_n"] == 4 and engine.hmm_plan(3, 10, 3, 2)["grid"] == 1
    assert engine.hmm_plan(1, 1000, 3, 2)["grid"] == 2
    with pytest.raises(NotImplementedError):
        engine.hmm_plan(_lib.HMM_MAX_HIDDEN + 1, 10, 1)


@pytest.mark.parametrize("name", ALL)
def test_estep_against_longdouble(engine, name):
    got, _ = device_estep(engine, name)
    check_estep(name, got)
    A, B, p0, labels, table, k = inputs(name)
    covered = np.zeros(len(labels), bool)
    for row in table:
        covered[row[0] + row[1] * np.arange(row[2])] = True
    assert not got["gamma"][~covered].any()                 # frames in no sequence keep zero rows
    if name == "unseen_symbol":
        assert not got["E"][:, 3].any()


@pytest.mark.parametrize("name", ["n2_k3_edges", "n16_k130", "lag3"])
def test_same_bits_for_every_grid_and_run(engine, name):
    base, _ = device_estep(engine, name)
    for mw, poison in ((0, 0), (1, 0), (2, 0), (0, 33)):
        got, _ = device_estep(engine, name, max_workgroups=mw, poison=poison)
        for key in ("gamma", "C", "gamma0", "logL", "E"):
            assert np.array_equal(got[key], base[key]), (key, mw, poison)
        assert got["total"] == base["total"]


def test_lag_against_prestrided_pieces(engine):
    A, B, p0 = R.random_model(3, 5, 31)
    traj = R.sample_labels(A, B, p0, 3 * L + 5, 9)
    dA, dB, dp = engine.to_device(A), engine.to_device(B), engine.to_device(p0)
    labels, table = H.lag_observations([traj], 3, 5)
    a = engine.hmm_estep(engine.hmm_tables(engine.to_device(labels), 5, table), dA, dB, dp)
    labels1, table1 = H.lag_observations([traj[0::3], traj[1::3], traj[2::3]], 1, 5)
    b = engine.hmm_estep(engine.hmm_tables(engine.to_device(labels1), 5, table1), dA, dB, dp)
    assert np.array_equal(a["C"].to_host(), b["C"].to_host())
    assert np.array_equal(a["logL"].to_host(), b["logL"].to_host())
    members = int(np.bincount(traj, minlength=5).max())
    R.check_close(a["E"].to_host(), b["E"].to_host().astype(LD), 2 * R.depth_E([len(traj) // 3 + 1], 3, members), "E")


def _exact_case(T=3 * L + 9, n=3, k=7, seed=0):
    rng = np.random.default_rng(seed)
    owner = np.arange(k) % n
    A, _, p0 = R.random_model(n, k, seed)
    B = np.zeros((n, k))
    B[owner, np.arange(k)] = rng.random(k) + 0.1
    B /= B.sum(axis=1, keepdims=True)
    labels = R.sample_labels(A, B, p0, T, seed)
    labels[77] = -1
    return A, B, p0, labels, owner


@pytest.mark.parametrize("lag", [1, 3])
def test_exact_case_equals_the_lumped_counts(engine, lag):
    A, B, p0, traj, owner = _exact_case()
    n, k = B.shape
    labels, table = H.lag_observations([traj], lag, k)
    tables = engine.hmm_tables(engine.to_device(labels), k, table)
    dA, dB, dp = engine.to_device(A), engine.to_device(B), engine.to_device(p0)
    got = engine.hmm_estep(tables, dA, dB, dp)
    lumped = np.where(labels >= 0, owner[np.clip(labels, 0, k - 1)], -1).astype(np.int32)
    hot = np.zeros((len(labels), n))
    hot[np.flatnonzero(labels >= 0), lumped[labels >= 0]] = 1.0
    assert np.array_equal(got["gamma"].to_host(), hot)
    counts, _ = engine.count_transitions(engine.to_device(lumped), n, lag, starts=[0, 78], stops=[77, len(labels)])
    counts = counts.to_host()
    assert counts.sum() == (77 - lag) + (len(labels) - 78 - lag)
    assert np.array_equal(got["C"].to_host(), counts.astype(np.float64))
    engine.hmm_mstep(got["C"], got["E"], got["gamma0"], tables["Q"], dA, dB, dp, reversible=False)
    assert np.array_equal(dA.to_host(), counts / counts.sum(axis=1, keepdims=True))


def test_zero_probability_sequence(engine):
    A, B, p0 = R.random_model(2, 3, 41)
    labels = np.concatenate([R.sample_labels(A, B, p0, T, 60 + i) for i, T in enumerate((L + 3, 2 * L + 1, 1, 40))])
    table = R.single_rows([L + 3, 2 * L + 1, 1, 40])
    B0 = B.copy()
    B0[:, 2] = 0.0
    B0 /= B0.sum(axis=1, keepdims=True)
    labels[(labels == 2)] = 1
    labels[L + 3 + L + 20] = 2                       # inside the second chunk of sequence 1
    tables = engine.hmm_tables(engine.to_device(labels), 3, table)
    out = engine.hmm_estep(tables, engine.to_device(A), engine.to_device(B0), engine.to_device(p0))
    want = R.estep(A, B0, p0, labels, table, 3, LD)
    assert out["status"] == _lib.HMM_ZERO_PROB == want["status"]
    logL, gamma = out["logL"].to_host(), out["gamma"].to_host()
    assert logL[1] == -np.inf and np.isfinite(logL[[0, 2, 3]]).all() and out["total"] == -np.inf
    for key in ("gamma", "C", "gamma0", "E"):
        assert not np.isnan(out[key].to_host()).any()
    assert not gamma[L + 3:L + 3 + 2 * L + 1].any()
    lengths = [L + 3, 2 * L + 1, 1, 40]
    R.check_close(gamma, want["gamma"], R.depth_gamma(max(lengths), 2), "gamma")
    R.check_close(out["C"].to_host(), want["C"], R.depth_C(lengths, 2), "C")
    R.check_close(out["gamma0"].to_host(), want["gamma0"], R.depth_gamma0(lengths, 2), "gamma0")


def test_bad_symbol_sets_its_bit(engine):
    A, B, p0 = R.random_model(2, 3, 42)
    labels = R.sample_labels(A, B, p0, L + 30, 1)
    labels[L + 10] = 3
    table = R.single_rows([20, L + 10])
    tables = engine.hmm_tables(engine.to_device(labels), 3, table)
    out = engine.hmm_estep(tables, engine.to_device(A), engine.to_device(B), engine.to_device(p0))
    assert out["status"] == _lib.HMM_BAD_SYMBOL
    assert np.isfinite(out["logL"].to_host()[0]) and out["logL"].to_host()[1] == -np.inf
    assert not out["gamma"].to_host()[20:].any() and not np.isnan(out["C"].to_host()).any()


def mstep_depths(n, k):
    return {"B": -(-k // 256) + 11, "A": n, "A_rev": 2 * n + 4, "p0": 1,
            "pi": n * (n - 1) * (n + 2) + n * n + n + 1}


@pytest.mark.parametrize("name", ["n1_k1", "n2_k3_edges", "n3_k65_zeros", "n16_k130", "unseen_symbol"])
@pytest.mark.parametrize("reversible", [False, True])
def test_mstep(engine, name, reversible):
    A, B, p0, labels, table, k = inputs(name)
    n, Q = A.shape[0], len(table)
    _, tables = device_estep(engine, name)
    dA, dB, dp = engine.to_device(A), engine.to_device(B), engine.to_device(p0)
    e = engine.hmm_estep(tables, dA, dB, dp)
    C, E, g0 = e["C"].to_host(), e["E"].to_host(), e["gamma0"].to_host()
    for stationary in (False, True):
        dA2, dB2, dp2 = engine.to_device(A), engine.to_device(B), engine.to_device(p0)
        out = engine.hmm_mstep(e["C"], e["E"], e["gamma0"], Q, dA2, dB2, dp2, reversible=reversible,
                               stationary=stationary, maxerr=MAXERR)
        assert out["status"] == 0
        A1, B1, p1, pi = dA2.to_host(), dB2.to_host(), dp2.to_host(), out["pi"].to_host()
        d = mstep_depths(n, k)
        R.check_close(B1, E.astype(LD) / E.astype(LD).sum(axis=1, keepdims=True), d["B"], "B")
        assert np.allclose(A1.sum(axis=1), 1.0, rtol=0, atol=(n + 2) * R.ULP)
        if name == "unseen_symbol":
            assert not B1[:, 3].any()
        if reversible:
            x1, _ = R.reversible_sweep(C, pi, LD)
            assert float(np.max(np.abs(x1 - pi) / pi)) <= MAXERR + (2 * n + 8) * R.ULP
            R.check_close(A1, R.transition_from_x(C, pi, LD), d["A_rev"], "A reversible")
            flux = pi[:, None] * A1
            assert float(np.max(np.abs(flux - flux.T) / np.maximum(flux, flux.T).clip(1e-300))) <= 2.1 * MAXERR + 16 * R.ULP
        else:
            CL = C.astype(LD)
            R.check_close(A1, CL / CL.sum(axis=1, keepdims=True), d["A"], "A")
            R.check_close(pi, R.stationary_gth(A1, LD), d["pi"], "pi")
        R.check_close(p1, pi.astype(LD) if stationary else g0.astype(LD) / Q, d["p0"], "p0")


@pytest.mark.parametrize("name", ["n2_k3_edges", "n3_k63", "lag3"])
def test_iterations_step_by_step(engine, name):
    A, B, p0, labels, table, k = inputs(name)
    n, lengths = A.shape[0], [int(x) for x in table[:, 2]]
    tables = engine.hmm_tables(engine.to_device(labels), k, table)
    dA, dB, dp = engine.to_device(A), engine.to_device(B), engine.to_device(p0)
    members = int(np.bincount(labels[(labels >= 0) & (labels < k)], minlength=k).max())
    d = mstep_depths(n, k)
    state, history, bounds = None, [], []
    cur = (A, B, p0)
    for _ in range(3):
        state = engine.hmm_iterations(tables, dA, dB, dp, 1, state=state, reversible=False)
        assert state["status"] == 0
        (A1, B1, p1, _), e, _ = R.em_step(*cur, labels, table, k, LD)
        got = (dA.to_host(), dB.to_host(), dp.to_host())
        R.check_close(got[0], A1, R.depth_C(lengths, n) + d["A"], "A after one iteration")
        R.check_close(got[1], B1, R.depth_E(lengths, n, members) + d["B"], "B after one iteration")
        R.check_close(got[2], p1, R.depth_gamma0(lengths, n) + d["p0"], "p0 after one iteration")
        bounds.append(sum(R.bound_logL(T, n, s) for T, s in zip(lengths, e["S"])) +
                      len(lengths) * R.ULP * float(np.sum(np.abs(e["logL"]))))
        assert abs(state["history"][0] - float(np.sum(e["logL"]))) <= bounds[-1]
        history.append(float(state["history"][0]))
        cur = got
    for i in range(2):                                # EM never lowers the likelihood
        assert history[i + 1] >= history[i] - (bounds[i] + bounds[i + 1])
    # several iterations in one call walk the same bits as one at a time
    dA2, dB2, dp2 = engine.to_device(A), engine.to_device(B), engine.to_device(p0)
    block = engine.hmm_iterations(tables, dA2, dB2, dp2, 3, reversible=False)
    assert np.array_equal(block["history"], np.asarray(history))
    assert np.array_equal(dA2.to_host(), cur[0]) and np.array_equal(dB2.to_host(), cur[1])


def test_converged_fit_is_a_fixed_point(engine):
    A, B, p0, labels, table, k = inputs("lag1")
    lengths = [int(x) for x in table[:, 2]]
    tables = engine.hmm_tables(engine.to_device(labels), k, table)
    dA, dB, dp = engine.to_device(A), engine.to_device(B), engine.to_device(p0)
    accuracy = 1e-3
    fit = engine.hmm_fit(tables, dA, dB, dp, reversible=False, accuracy=accuracy, maxit=400)
    assert fit["converged"] and fit["n_iterations"] == len(fit["likelihoods"]) <= 400
    cur = (dA.to_host(), dB.to_host(), dp.to_host())
    before = R.estep(*cur, labels, table, k, LD)
    (A1, B1, p1, _), _, _ = R.em_step(*cur, labels, table, k, LD)
    after = R.estep(A1, B1, p1, labels, table, k, LD)
    bound = sum(R.bound_logL(T, 2, s) for T, s in zip(lengths, before["S"]))
    gain = float(np.sum(after["logL"]) - np.sum(before["logL"]))
    print(f"gain of one more longdouble EM step: {gain:.3e}")
    assert -bound <= gain < accuracy + bound
    assert float(np.sum(before["logL"])) >= fit["likelihoods"][0]


def test_init_hmm_from_msm_is_a_valid_start():
    rng = np.random.default_rng(1)
    X = rng.random((6, 6)) * 0.02
    X[:3, :3] += 1.0
    X[3:, 3:] += 1.0
    X = X + X.T
    pi = X.sum(axis=1) / X.sum()
    A, B, p0 = H.init_hmm_from_msm(X / X.sum(axis=1, keepdims=True), pi, 2)
    for M in (A, B, p0[None, :]):
        assert (M > 0).all() and np.allclose(M.sum(axis=1), 1.0)
    assert A[0, 0] > 0.9 and A[1, 1] > 0.9
    assert {tuple(np.argmax(B, axis=0)[:3]), tuple(np.argmax(B, axis=0)[3:])} == {(0, 0, 0), (1, 1, 1)}


def _two_state_dtrajs():
    A = np.array([[0.97, 0.03], [0.05, 0.95]])
    B = np.array([[0.5, 0.3, 0.18, 0.01, 0.005, 0.005], [0.005, 0.005, 0.01, 0.2, 0.38, 0.4]])
    p0 = np.array([0.5, 0.5])
    return [R.sample_labels(A, B, p0, T, 70 + i) for i, T in enumerate((400, 250))], A, B


@pytest.mark.parametrize("entry", ["estimate_hmm", "coarse_grain_hmm"])
def test_end_to_end(entry):
    dtrajs, A, B = _two_state_dtrajs()
    n, k, lag = 2, 6, 2
    res = H.estimate_hmm(dtrajs, n, lag, k) if entry == "estimate_hmm" else H.coarse_grain_hmm(dtrajs, k, n, lag)
    assert res.transition_matrix.shape == (n, n) and res.output_probabilities.shape == (n, k)
    assert res.initial_distribution.shape == (n,) and res.stationary_distribution.shape == (n,)
    assert res.count_matrix.shape == (n, n) and res.timescales.shape == (n - 1,) and res.lag == lag
    for M in (res.transition_matrix, res.output_probabilities, res.initial_distribution[None, :],
              res.stationary_distribution[None, :], res.metastable_memberships):
        assert (M >= 0).all() and np.allclose(M.sum(axis=1), 1.0, atol=1e-12)
    assert res.metastable_memberships.shape == (k, n) and res.metastable_assignments.shape == (k,)
    assert len(set(res.metastable_assignments[:3])) == 1 and len(set(res.metastable_assignments[3:])) == 1
    assert res.metastable_assignments[0] != res.metastable_assignments[5]
    assert res.n_iterations >= 1 and res.converged and len(res.likelihoods) == res.n_iterations + 1
    assert res.likelihood >= res.likelihoods[0] and np.isfinite(res.likelihood)
    assert res.timescales[0] > lag
    flux = res.stationary_distribution[:, None] * res.transition_matrix
    assert np.allclose(flux, flux.T, rtol=1e-6, atol=0)
    gammas = res.hidden_state_probabilities()
    assert [g.shape for g in gammas] == [(400, n), (250, n)]
    assert all(np.allclose(g.sum(axis=1), 1.0, atol=1e-12) for g in gammas)


# ---- Viterbi -----------------------------------------------------------------------------------------------------
# The device maximises its own fp64 score of a path: 2 T logarithms, each within 2 ulp of itself, added in some order
# (2 T additions, every partial sum at most the total in magnitude, all terms having one sign).  Its score of any path
# is within eps = (2 T + 4) 2^-52 |score| of the true one, so the true score of the path it picks is within 2 eps of
# the true optimum.
def viterbi_bound(T, optimum):
    return 2 * (2 * T + 4) * R.ULP * abs(float(optimum)) * (1 + 1e-9)


def device_viterbi(engine, name, max_workgroups=0):
    A, B, p0, labels, table, k = inputs(name)
    tables = engine.hmm_tables(engine.to_device(labels), k, table)
    out = engine.hmm_viterbi(tables, engine.to_device(A), engine.to_device(B), engine.to_device(p0),
                             max_workgroups=max_workgroups)
    return out["path"].to_host(), out["logp"].to_host(), out["status"]


@pytest.mark.parametrize("name", ALL)
def test_viterbi_path_is_valid_and_optimal(engine, name):
    A, B, p0, labels, table, k = inputs(name)
    path, logp, status = device_viterbi(engine, name)
    assert status == 0
    covered = np.zeros(len(labels), bool)
    for q, row in enumerate(table):
        frames = row[0] + row[1] * np.arange(row[2])
        covered[frames] = True
        obs, got = labels[frames], path[frames]
        assert ((got >= 0) & (got < A.shape[0])).all()
        assert p0[got[0]] > 0 and (B[got, obs] > 0).all() and (A[got[:-1], got[1:]] > 0).all()      # valid
        _, best = R.viterbi(A, B, p0, obs, LD)
        mine = R.path_log_probability(A, B, p0, obs, got)
        bound = viterbi_bound(len(obs), best)
        assert best - mine <= bound and mine <= best + 1e-17 * len(obs) * abs(float(best))
        assert abs(float(LD(logp[q]) - mine)) <= bound
    assert (path[~covered] == -1).all()
    for mw in (1, 2):
        again = device_viterbi(engine, name, mw)
        assert np.array_equal(again[0], path) and np.array_equal(again[1], logp)


def test_viterbi_exact_case_is_forced(engine):
    A, B, p0, traj, owner = _exact_case()
    k = B.shape[1]
    for lag in (1, 3):
        labels, table = H.lag_observations([traj], lag, k)
        tables = engine.hmm_tables(engine.to_device(labels), k, table)
        out = engine.hmm_viterbi(tables, engine.to_device(A), engine.to_device(B), engine.to_device(p0))
        assert out["status"] == 0
        assert np.array_equal(out["path"].to_host(), np.where(labels >= 0, owner[np.clip(labels, 0, k - 1)], -1))


def test_viterbi_ties_and_zero_probability(engine):
    # every path is equally probable: the lowest index wins everywhere
    n, k, T = 4, 2, 2 * L + 3
    A, B, p0 = np.full((n, n), 0.25), np.full((n, k), 0.5), np.full(n, 0.25)
    labels = (np.arange(T + 5) % 2).astype(np.int32)
    table = R.single_rows([T, 5])
    B0 = np.array([[0.5, 0.5], [1.0, 0.0]])
    tables = engine.hmm_tables(engine.to_device(labels), k, table)
    out = engine.hmm_viterbi(tables, engine.to_device(A), engine.to_device(B), engine.to_device(p0))
    assert out["status"] == 0 and not out["path"].to_host().any()
    # a sequence of probability 0 gets -1 and -inf, the other one is decoded
    Az = np.array([[0.0, 1.0], [0.0, 1.0]])
    labels2 = np.zeros(T + 5, np.int32)
    labels2[L + 9] = 1
    labels2[T:] = 0
    tables = engine.hmm_tables(engine.to_device(labels2), k, table)
    out = engine.hmm_viterbi(tables, engine.to_device(Az), engine.to_device(B0), engine.to_device(np.array([0.5, 0.5])))
    path, logp = out["path"].to_host(), out["logp"].to_host()
    assert out["status"] == _lib.HMM_ZERO_PROB
    assert (path[:T] == -1).all() and logp[0] == -np.inf
    assert np.array_equal(path[T:], [1, 1, 1, 1, 1]) and np.isfinite(logp[1])


def test_result_viterbi_per_trajectory():
    dtrajs, A, B = _two_state_dtrajs()
    res = H.estimate_hmm(dtrajs, 2, 1, 6)
    paths, gammas = res.viterbi(), res.hidden_state_probabilities()
    assert [p.shape for p in paths] == [(400,), (250,)] and all(p.dtype == np.int32 for p in paths)
    for p, g in zip(paths, gammas):
        assert ((p == 0) | (p == 1)).all()
        assert np.mean(p == np.argmax(g, axis=1)) > 0.95          # the path follows the posterior almost everywhere
