"""The numpy restatement of the TRAM contract (tests/_tram_ref.py) against three independent answers, its fp64 form
against its longdouble form inside the derived bounds, and the device-free logic of reweight.tram.  CPU suite.

The three limits are solved at tol = 1e-12 and compared within (tol_a + tol_b) / (1 - rho): an iterate whose last
step moved by err lies within err / (1 - rho) of the fixed point of a map that contracts at rate rho, and rho is read
off the restatement's own last error ratios (R.contraction).  tol_b is the other side's own last step (0 for the exact
answer; MBAR's own tol for its Newton solve).  The other side is brought into our gauge (min f = 0) first.

The fp64 restatement against the longdouble one (R.rows_bound, R.pass_bound; derivation in tests/_tram_ref.py):
  rows_bound = (chain + 8 + X) 2^-52, X = max |g_j - g_i| over S_ij != 0; chain = m for numpy's row sum;
  pass_bound = (K + chain + 16) 2^-52 A, A = max(1, |a_l|, |u_ln - m_n| where inexact); chain = frames of the fullest
  state for numpy's reduceat."""
import importlib

import numpy as np
import pytest

from pmarlo_amd.device import Engine
from tests import _estimation_ref as E
from tests import _mbar_ref
from tests import _tram_ref as R

T = importlib.import_module("pmarlo_amd.reweight.tram")     # the package exports the function under the same name
LD = np.longdouble
TOL = 1e-12


def test_one_markov_state_is_mbar():
    prob, N_k = R.mbar_limit_case()
    r = R.solve(prob, tol=TOL)
    rho = R.contraction(r["history"])
    ref = _mbar_ref.solve(prob["u"], N_k, tol=TOL)
    diff = float(np.abs(r["f"][:, 0] - (ref["f"] - ref["f"].min())).max())
    print("m = 1:", r["n_iterations"], "iterations, rho", rho, "diff", diff)
    assert diff <= (TOL + TOL) / (1 - rho)
    assert np.array_equal(r["v"][:, 0], prob["C"][:, 0, 0])          # v = S / 2 exactly: the counts cancel


def test_one_ensemble_is_the_reversible_mle():
    prob = R.msm_limit_case()
    r = R.solve(prob, tol=TOL)
    rho = R.contraction(r["history"])
    P_ref, pi_ref = E.revmle_ld(prob["C"][0], 3000)
    _, pi_prev = E.revmle_ld(prob["C"][0], 2999)
    tol_b = float(np.abs(np.log(pi_ref) - np.log(pi_prev)).max())
    f_ref = -np.log(pi_ref)
    diff = float(np.abs(r["f"][0] - (f_ref - f_ref.min())).max())
    print("K = 1:", r["n_iterations"], "iterations, rho", rho, "diff", diff, "tol_b", tol_b)
    bound = (TOL + tol_b) / (1 - rho)
    assert diff <= bound
    P = R.transition_matrix(prob["S"], prob["N"], r["f"], r["v"], 0)
    assert np.abs(P.sum(axis=1) - 1).max() <= 8 * R.ULP
    # p_ij = S_ij / (v_i + v_j e^{f_j - f_i}): relative error of an entry <= the errors of ln v and f, each `bound`
    assert float(np.abs(P - P_ref).max()) <= 4 * bound
    pi = R.stationary(prob["N"], r["f"], 0)
    assert np.abs(pi[:, None] * P - (pi[:, None] * P).T).max() <= 8 * R.ULP


def test_state_only_bias_returns_the_known_populations():
    prob, pi = R.state_only_case()
    assert (prob["N"] == 0).sum() == 2
    r = R.solve(prob, tol=TOL)
    rho = R.contraction(r["history"])
    fs = R.target_state_f(np.zeros((1, r["d"].size)), r["d"], prob["state"], 5)[0]
    pop = np.exp(-(fs - fs.min()))
    pop /= pop.sum()
    diff = float(np.abs(np.log(pop) - np.log(pi)).max())
    print("state-only bias:", r["n_iterations"], "iterations, rho", rho, "diff", diff)
    assert diff <= (TOL + 0.0) / (1 - rho)
    assert np.isinf(r["v"][prob["N"] == 0]).sum() == 0 and (r["v"][prob["N"] == 0] == 0).all()


@pytest.mark.parametrize("shape", [(1, 1, 5), (2, 7, 3), (3, 65, 4), (8, 20, (300, 1, 257) + (5,) * 17)])
def test_fp64_restatement_stays_inside_the_bounds(shape):
    K, m, frames = shape
    prob, f, v = R.synthetic(K, m, frames, seed=100 + K)
    g = R.log_multipliers(f, v)
    chain_p = int(np.bincount(prob["state"]).max())
    for mode in ("multipliers", "counts"):
        R.check_rows(R.rows(prob["S"], g, f, prob["N"], prob["col"], mode),
                     R.rows(prob["S"], g, f, prob["N"], prob["col"], mode, LD), R.rows_bound(prob["S"], g, m), f)
    _, tab = R.rows(prob["S"], g, f, prob["N"], prob["col"], "counts")
    got = R.frame_pass(prob["u"], prob["state"], tab, m)
    R.check_pass(got, R.frame_pass(prob["u"], prob["state"], tab, m, LD),
                 R.pass_bound(prob["u"], prob["state"], tab, chain_p))
    assert got["status"] == 0


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_fp64_restatement_stays_inside_the_bounds_on_the_gpu_inputs(name):
    """The inputs the device is tested on, the same checks, numpy's chains in place of the device's: the bounds are
    not fitted to the device."""
    prob, f, v = R.case(name)
    m = f.shape[1]
    g = R.log_multipliers(f, v)
    for mode in ("multipliers", "counts"):
        R.check_rows(R.rows(prob["S"], g, f, prob["N"], prob["col"], mode),
                     R.rows(prob["S"], g, f, prob["N"], prob["col"], mode, LD), R.rows_bound(prob["S"], g, m), f)
    for f32 in (False, True):
        tab, want, u = R.host_tab(name, f32)
        R.check_pass(R.frame_pass(u, prob["state"], tab, m), want,
                     R.pass_bound(u, prob["state"], tab, int(np.bincount(prob["state"]).max())))


def test_restatement_follows_the_check_schedule():
    prob, _ = R.state_only_case()
    a, b = R.solve(prob, tol=1e-8, check_every=16), R.solve(prob, tol=1e-8, check_every=1)
    assert a["n_iterations"] % 16 == 0 and a["n_iterations"] - 16 < b["n_iterations"] <= a["n_iterations"]
    assert np.array_equal(a["history"][:b["n_iterations"]], b["history"])
    with pytest.raises(R.NotConverged):
        R.solve(prob, tol=1e-8, maxiter=20)


def test_pass_flags_bad_input_and_dead_frames():
    prob, f, v = R.synthetic(2, 3, 4, seed=5, inactive=0.0)
    _, tab = R.rows(prob["S"], R.log_multipliers(f, v), f, prob["N"], prob["col"], "counts")
    u = prob["u"].copy()
    u[1, 2] = np.nan
    assert R.frame_pass(u, prob["state"], tab, 3)["status"] & 1
    u = prob["u"].copy()
    u[:, 5] = np.inf
    p = R.frame_pass(u, prob["state"], tab, 3)
    assert p["status"] == 2 and (p["r"][:, 5] == 0).all()


# ---- the device-free logic of reweight.tram -----------------------------------------------------------------------
def test_fragments_break_where_a_replica_hops():
    d = [np.array([0, 1, 1, 0, 2, 2, 1]), np.array([1, 1, -1, 1, 0])]
    t = [np.array([0, 0, 1, 1, 1, 0, 0]), np.array([1, 1, 1, 1, 1])]
    fr = T.fragments(np.concatenate(d), np.concatenate(t), [7, 5], 2)
    assert fr[0][0].tolist() == [0, 5] and fr[0][1].tolist() == [2, 7]
    assert fr[1][0].tolist() == [2, 7, 10] and fr[1][1].tolist() == [5, 9, 12]      # the invalid frame 9 cuts
    C = R.counts_from_trajs(d, t, 2, 3, 1)
    assert C[0].sum() == 2 and C[1].sum() == 4 and C[0, 0, 1] == 1 and C[0, 2, 1] == 1
    assert C[1, 1, 0] == 2 and C[1, 0, 2] == 1 and C[1, 1, 1] == 1
    # a lag as long as a fragment leaves nothing
    assert R.counts_from_trajs(d, t, 2, 3, 2)[0].sum() == 0


def test_connected_set_drops_a_side_component_and_unvisited_states():
    # states 0, 1, 2 cycle; 4 and 5 exchange among themselves only; 3 is never visited; 6 is visited once, no return
    C = np.zeros((7, 7))
    C[0, 1] = C[1, 2] = C[2, 0] = 3
    C[4, 5] = C[5, 4] = 9
    C[2, 6] = 1
    visited = np.array([5, 5, 5, 0, 10, 10, 1])
    act = T.largest_connected_set(C, visited)
    assert act.tolist() == [0, 1, 2]
    lab = T.restrict_labels(np.array([0, 4, 2, 6, -1, 1, 5, 3]), act, 7)
    assert lab.tolist() == [0, -1, 2, -1, -1, 1, -1, -1]
    # equal sizes: the set with more frames wins
    C2 = np.zeros((4, 4))
    C2[0, 1] = C2[1, 0] = C2[2, 3] = C2[3, 2] = 1
    assert T.largest_connected_set(C2, np.array([1, 1, 2, 2])).tolist() == [2, 3]
    assert T.largest_connected_set(C2, np.array([1, 1, 1, 1])).tolist() == [0, 1]
    assert T.largest_connected_set(np.zeros((2, 2)), np.zeros(2)).size == 0


def test_dropped_frames_break_fragments():
    # the walk enters state 2 and an unassigned frame hides the way back: 2 is outside the connected set {0, 1}, and
    # no pair may be counted across the frames that leave with it
    d = np.array([0, 1, 0, 1, 2, -1, 0, 1, 0])
    t = np.zeros(9, np.int64)
    act = T.largest_connected_set(R.counts_from_trajs([d], [t], 1, 3, 1)[0], np.bincount(d[d >= 0]))
    assert act.tolist() == [0, 1]
    lab = T.restrict_labels(d, act, 3)
    assert lab.tolist() == [0, 1, 0, 1, -1, -1, 0, 1, 0]
    starts, stops = T.fragments(lab, t, [9], 1)[0]
    assert starts.tolist() == [0, 6] and stops.tolist() == [4, 9]
    C = R.counts_from_trajs([lab], [t], 1, 2, 2)
    assert C.sum() == 3                                    # (0,2) (1,3) and (6,8); none across frames 4 and 5


def test_unit_tables_name_every_segment_once():
    off, unit_ptr, unit_state = Engine._tram_units([0, 1, 1 + R.SEGMENT, 2 + 2 * R.SEGMENT, 7 + 2 * R.SEGMENT])
    assert unit_ptr.tolist() == [0, 1, 2, 4, 5] and unit_state.tolist() == [0, 1, 2, 2, 3]
    with pytest.raises(ValueError, match="at least one frame"):
        Engine._tram_units([0, 3, 3, 5])
