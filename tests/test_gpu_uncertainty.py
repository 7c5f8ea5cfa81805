"""Trajectory bootstrap on the device (msm_combine_counts, msm_row_normalise_batched, msm_reactive_flux_batched and
pmarlo_amd.conformations.UncertaintyQuantifier) against the numpy restatement in tests/_uncertainty_ref.py.

Integer results and the committors are held bit for bit; the flux totals to the 1e-9 test_gpu_tpt.py holds the
single-matrix kernel to; the end-to-end statistics to 1e-6 relative, the project's stated agreement of the device
spectrum (where pi comes from) with numpy's eigensolver."""
import functools

import numpy as np
import pytest

from oracle import npport
from pmarlo_amd import _lib
from pmarlo_amd.conformations import UncertaintyQuantifier
from pmarlo_amd.markov_state_model.pcca import pcca_memberships
from tests import _uncertainty_ref as R

pytestmark = pytest.mark.gpu

LDS_N = _lib.FLUX_LDS_MAX_N


# ---- counts --------------------------------------------------------------------------------------------------------
def _count_case(k, n_traj, frames):
    """Trajectories plus one of two frames (shorter than lag 3), and a multiplicity table with a row that is all on
    one trajectory and a row that is all on the short one."""
    trajs = R.trajectories(k, n_traj, frames, seed=k, coupling=0.1, check=False)
    trajs.append(np.array([k - 1, 0], np.int32))
    n_seg = len(trajs)
    rng = np.random.default_rng(k)
    mult = rng.multinomial(n_seg, np.full(n_seg, 1.0 / n_seg), size=9).astype(np.int32)
    mult[3] = 0
    mult[3, 1] = n_seg
    mult[5] = 0
    mult[5, n_seg - 1] = n_seg
    return trajs, mult


def _device_trajs(engine, trajs):
    sizes = np.asarray([t.size for t in trajs], np.int64)
    stops = np.cumsum(sizes)
    return engine.to_device(np.concatenate(trajs).astype(np.int32)), stops - sizes, stops


@pytest.mark.parametrize("lag", [1, 3])
@pytest.mark.parametrize("k,n_traj,frames", [(3, 2, 60), (12, 5, 400), (130, 3, 20000)])
def test_resampled_counts_and_normalisation(engine, k, n_traj, frames, lag):
    trajs, mult = _count_case(k, n_traj, frames)
    n_seg = len(trajs)
    labels, starts, stops = _device_trajs(engine, trajs)
    seg = engine.empty((n_seg, k, k), np.int64)
    for s in range(n_seg):
        engine.count_transitions(labels, k, lag, starts=starts[s:s + 1], stops=stops[s:s + 1],
                                 out=seg.view((k, k), offset_elems=s * k * k))
    C_seg = seg.to_host()
    want_seg = np.stack([npport._pair_counts([t], k, lag) for t in trajs]).astype(np.int64)
    assert np.array_equal(C_seg, want_seg)
    mult_d = engine.to_device(mult)
    C = engine.combine_counts(seg, mult_d)
    got = C.to_host()
    assert got.dtype == np.int64 and np.array_equal(got, np.tensordot(mult.astype(np.int64), C_seg, axes=1))
    for b in range(len(mult)):                                   # = counting the resampled list itself
        resample = [trajs[s] for s in range(n_seg) for _ in range(mult[b, s])]
        assert np.array_equal(got[b], npport._pair_counts(resample, k, lag).astype(np.int64)), b
    # two chunks of trajectories, the second added to the first
    h = n_seg // 2
    two = engine.combine_counts(seg.view((h, k, k)), mult_d)
    engine.combine_counts(seg.view((n_seg - h, k, k), offset_elems=h * k * k), mult_d, seg0=h, out=two, accumulate=True)
    assert np.array_equal(two.to_host(), got)
    # T = C / rowsum exactly, zero rows stay zero
    T, rowsum = engine.row_normalise_batched(C)
    rs = got.sum(axis=2)
    assert np.array_equal(rowsum.to_host(), rs)
    with np.errstate(invalid="ignore", divide="ignore"):
        want_T = np.where(rs[:, :, None] > 0, got / rs[:, :, None], 0.0)
    assert np.array_equal(T.to_host(), want_T)
    if lag == 3:
        assert not np.any(T.to_host()[5])                        # all on the two-frame trajectory: no pair at lag 3
    # the helper, in one piece and with a budget of one matrix per chunk
    for budget in (1 << 28, 1):
        Tb, rb = engine.bootstrap_transition_matrices(labels, starts, stops, k, lag, mult, chunk_bytes=budget)
        assert np.array_equal(Tb.to_host(), want_T) and np.array_equal(rb.to_host(), rs)


def test_combine_counts_more_trajectories_than_one_launch_takes(engine):
    rng = np.random.default_rng(0)
    n_seg, n_boot = 2 * _lib.COMBINE_MAX_SEG + 5, 6
    seg = rng.integers(0, 1 << 40, size=(n_seg, 7, 7), dtype=np.int64)
    mult = rng.integers(0, 9, size=(n_boot, n_seg)).astype(np.int32)
    got = engine.combine_counts(engine.to_device(seg), engine.to_device(mult)).to_host()
    assert np.array_equal(got, np.tensordot(mult.astype(np.int64), seg, axes=1))


# ---- batched reactive flux ---------------------------------------------------------------------------------------
def _sets(n):
    return ([0], [n - 1]) if n < 6 else ([0, 1, 2], [n - 1, n - 2])


@functools.lru_cache(maxsize=None)
def _flux_case(n):
    """300 matrices of order n with their stationary vectors, and the numpy reference of each.  The first seven are
    general chains with pi from the oracle's eigensolver; the others are reversible, where pi is the normalised row
    sum of the symmetric weights (checked against the eigensolver on one of them)."""
    Ts, pis = [], []
    for b in range(300):
        if b < 7:
            T = R.metastable_T(n, seed=1000 * n + b)
            pi = npport.stationary_distribution(T)
        else:
            W = R.metastable_T(n, seed=1000 * n + b)
            W = W + W.T
            T, pi = W / W.sum(axis=1, keepdims=True), W.sum(axis=1) / W.sum()
        Ts.append(T)
        pis.append(pi)
    np.testing.assert_allclose(pis[7], npport.stationary_distribution(Ts[7]), rtol=1e-9)
    A, B = _sets(n)
    refs = [npport.reactive_flux(T, pi, A, B) for T, pi in zip(Ts, pis)]
    role = np.zeros(n, np.int32)
    role[A], role[B] = 1, 2
    return np.stack(Ts), np.stack(pis), role, refs


@functools.lru_cache(maxsize=None)
def _single_committors(n):
    """Engine.reactive_flux on each matrix alone (session engine through get_engine)."""
    from pmarlo_amd.device import get_engine

    eng = get_engine()
    Ts, pis, role, _ = _flux_case(n)
    out = []
    for T, pi in zip(Ts, pis):
        o = eng.reactive_flux(eng.to_device(T), eng.to_device(pi), role, want_flux=False)
        assert not np.any(o["info"])
        out.append((o["qplus"].to_host(), o["qminus"].to_host()))
    return out


@pytest.mark.parametrize("batch", [1, 7, 300])
@pytest.mark.parametrize("n", [2, 12, LDS_N, LDS_N + 1, 200])
def test_reactive_flux_batched(n, batch):
    from pmarlo_amd.device import get_engine

    eng = get_engine()
    Ts, pis, role, refs = _flux_case(n)
    single = _single_committors(n)
    out = eng.reactive_flux_batched(eng.to_device(Ts[:batch]), eng.to_device(pis[:batch]), role)
    assert out["info"].shape == (batch, 2) and not np.any(out["info"])
    qp, qm, tot = out["qplus"].to_host(), out["qminus"].to_host(), out["totals"].to_host()
    for b in range(batch):
        assert np.array_equal(qp[b], single[b][0]) and np.array_equal(qm[b], single[b][1]), b
    want = np.asarray([[r["total_flux"], np.dot(pi, r["qminus"]), r["rate"], r["mfpt"]] for r, pi in zip(refs[:batch], pis)])
    np.testing.assert_allclose(tot, want, rtol=1e-9)
    # totals alone (the committors stay in the scratch): same numbers
    alone = eng.reactive_flux_batched(eng.to_device(Ts[:batch]), eng.to_device(pis[:batch]), role, want_committors=False)
    assert alone["qplus"] is None and np.array_equal(alone["totals"].to_host(), tot)


@pytest.mark.parametrize("n", [12, LDS_N + 1])
def test_reactive_flux_batched_singular_sample_is_isolated(engine, n):
    Ts, pis, role, _ = _flux_case(n)
    Ts, pis = Ts[:5].copy(), pis[:5].copy()
    clean = engine.reactive_flux_batched(engine.to_device(Ts), engine.to_device(pis), role)
    # uncoupled blocks, source and sink both in the first; the other states never move, so their rows of T - I (and of
    # the reversed chain's system, pi being uniform) are exactly zero: no pivot, whatever the rounding
    h = n // 2
    A, B = _sets(n)
    perm = np.r_[A, B, np.setdiff1d(np.arange(n), A + B)]       # source and sink states lead the first block
    blocks = np.zeros((n, n))
    blocks[:h, :h] = R.metastable_T(h, seed=1)
    blocks[h:, h:] = np.eye(n - h)
    Ts[2][np.ix_(perm, perm)] = blocks
    pis[2] = 1.0 / n
    out = engine.reactive_flux_batched(engine.to_device(Ts), engine.to_device(pis), role)
    assert np.all(out["info"][2] != 0) and not np.any(out["info"][[0, 1, 3, 4]])
    assert np.all(np.isnan(out["totals"].to_host()[2]))
    for key in ("qplus", "qminus", "totals"):
        got, want = out[key].to_host(), clean[key].to_host()
        assert np.array_equal(got[[0, 1, 3, 4]], want[[0, 1, 3, 4]]), key


def test_reactive_flux_batched_chunk_budget_does_not_change_the_result(engine):
    n = 200
    Ts, pis, role, _ = _flux_case(n)
    Td, pd = engine.to_device(Ts[:7]), engine.to_device(pis[:7])
    whole = engine.reactive_flux_batched(Td, pd, role)
    for budget in (1, 3 * (n * n + n) * 8):                      # one sample a call; three, with a remainder of one
        parts = engine.reactive_flux_batched(Td, pd, role, chunk_bytes=budget)
        assert np.array_equal(parts["info"], whole["info"])
        for key in ("qplus", "qminus", "totals"):
            assert np.array_equal(parts[key].to_host(), whole[key].to_host()), key


# ---- end to end ------------------------------------------------------------------------------------------------------
def _assert_stats(got, want, rtol=1e-6):
    assert got.n_samples == want["n_samples"] and got.method == "bootstrap"
    for f in ("mean", "std", "ci_lower", "ci_upper"):
        np.testing.assert_allclose(getattr(got, f), want[f], rtol=rtol, err_msg=f)


@functools.lru_cache(maxsize=None)
def _small_trajs():
    return R.trajectories(12, 5, 400, seed=1, lags=(1, 3), coupling=0.1)


@pytest.mark.parametrize("k,n_traj,frames,n_boot,lag", [(12, 5, 400, 50, 1), (12, 5, 400, 50, 3), (130, 3, 20000, 20, 3)])
def test_bootstrap_tpt_matches_reference(engine, k, n_traj, frames, n_boot, lag):
    trajs = _small_trajs() if k == 12 else R.trajectories(k, n_traj, frames, seed=1, lags=(lag,))
    A, B = _sets(k)
    want = R.bootstrap_tpt(trajs, A, B, n_boot, lag, np.random.default_rng(11))
    assert want["kept"].all()                                    # well-posed trajectories: the reference drops nothing
    uq = UncertaintyQuantifier(random_seed=11)
    got = uq.bootstrap_tpt(trajs, A, B, n_boot=n_boot, lag=lag)
    assert sorted(got) == ["mfpt", "rate", "total_flux"] and np.array_equal(uq.last_kept, want["kept"])
    for name in got:
        assert got[name].observable_name == name and isinstance(got[name].mean, float)
        _assert_stats(got[name], want[name])


def test_bootstrap_free_energies_matches_reference(engine):
    trajs = _small_trajs()
    want = R.bootstrap_free_energies(trajs, 310.0, 50, np.random.default_rng(12))
    got = UncertaintyQuantifier(random_seed=12).bootstrap_free_energies(trajs, T_K=310.0, n_boot=50)
    assert got.observable_name == "free_energies" and got.mean.shape == (12,)
    _assert_stats(got, want["free_energies"])


def test_bootstrap_macrostate_populations_matches_reference(engine):
    # every trajectory followed by its reversal: symmetric counts, a reversible estimate, which PCCA+ requires
    trajs = R.trajectories(12, 5, 400, seed=1, lags=(1,), coupling=0.1, palindrome=True)
    m, n_boot = 3, 50
    pops = []
    for _, T, pi in R.bootstrap_Tpi(trajs, n_boot, 1, np.random.default_rng(13)):
        chi = pcca_memberships(T, m, pi)
        pops.append(np.bincount(np.argmax(chi, axis=1), weights=pi, minlength=m))
    assert len(pops) == n_boot
    np.testing.assert_allclose(np.sum(pops, axis=1), 1.0, rtol=1e-12)
    got = UncertaintyQuantifier(random_seed=13).bootstrap_macrostate_populations(trajs, m, n_boot=n_boot, lag=1)
    assert got.observable_name == "macrostate_populations" and got.mean.shape == (m,)
    np.testing.assert_allclose(got.mean.sum(), 1.0, rtol=1e-9)
    _assert_stats(got, R._stats(pops, (2.5, 97.5)))


# ---- drop rule, failures, determinism ----------------------------------------------------------------------------
def _stuck_case():
    """One well-posed trajectory and one that never leaves state 2: a resample made of the second alone has empty
    rows.  With seed 0 the restated reference keeps 26 of 40 samples."""
    good = R.trajectories(6, 1, 300, seed=2, lags=(1,), coupling=0.1)[0]
    return [good, np.full(50, 2, np.int32)]


def test_dropped_samples_are_the_reference_s(engine):
    trajs = _stuck_case()
    want = R.bootstrap_tpt(trajs, [0], [5], 40, 1, np.random.default_rng(0))
    n_kept = int(want["kept"].sum())
    assert 0 < n_kept < 40
    uq = UncertaintyQuantifier(random_seed=0)
    got = uq.bootstrap_tpt(trajs, [0], [5], n_boot=40, lag=1)
    assert np.array_equal(uq.last_kept, want["kept"])
    for name in ("rate", "mfpt", "total_flux"):
        _assert_stats(got[name], want[name])


def test_all_samples_failing(engine, caplog):
    stuck = [np.full(30, 1, np.int32), np.full(20, 1, np.int32)]           # state 0 never occurs: its row is empty
    with caplog.at_level("WARNING", logger="pmarlo.conformations"):
        assert UncertaintyQuantifier(0).bootstrap_tpt(stuck, [0], [1], n_boot=8) == {}
    assert "All bootstrap samples failed" in caplog.text
    flip = [np.arange(40, dtype=np.int32) % 2]                              # period two: eigenvalues 1 and -1
    fe = UncertaintyQuantifier(0).bootstrap_free_energies(flip, n_boot=6)
    assert fe.n_samples == 0 and fe.mean.shape == (2,) and not np.any(fe.mean) and not np.any(fe.ci_upper)
    mp = UncertaintyQuantifier(0).bootstrap_macrostate_populations(flip, 2, n_boot=6)
    assert mp.n_samples == 0 and mp.mean.shape == (2,) and not np.any(mp.std)
    assert UncertaintyQuantifier(0).bootstrap_tpt(flip, [0], [1], n_boot=6) == {}


def test_errors(engine):
    uq = UncertaintyQuantifier(0)
    trajs = _small_trajs()
    with pytest.raises(ValueError):
        uq.bootstrap_tpt([], [0], [1])
    with pytest.raises(ValueError):
        uq.bootstrap_free_energies([np.full(10, -1)])
    with pytest.raises(ValueError):
        uq.bootstrap_tpt(trajs, [0, 1], [1, 2], n_boot=2)
    with pytest.raises(ValueError):
        uq.bootstrap_tpt(trajs, [0], [12], n_boot=2)
    with pytest.raises(ValueError):
        uq.bootstrap_tpt(trajs, [], [3], n_boot=2)


def test_equal_seeds_give_equal_results(engine):
    trajs = _small_trajs()
    a = UncertaintyQuantifier(random_seed=5).bootstrap_tpt(trajs, [0], [11], n_boot=30, lag=1)
    b = UncertaintyQuantifier(random_seed=5).bootstrap_tpt(trajs, [0], [11], n_boot=30, lag=1)
    assert a == b and a["rate"].n_samples == 30
    fa = UncertaintyQuantifier(random_seed=5).bootstrap_free_energies(trajs, n_boot=30)
    fb = UncertaintyQuantifier(random_seed=5).bootstrap_free_energies(trajs, n_boot=30)
    assert fa.to_dict() == fb.to_dict()
    other = UncertaintyQuantifier(random_seed=6).bootstrap_tpt(trajs, [0], [11], n_boot=30, lag=1)
    assert other["rate"].mean != a["rate"].mean
