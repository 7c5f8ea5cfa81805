"""The OPES restatement (tests/_opes_ref.py) against closed forms, and the conditions on the committed deposit sequences
that tests/test_gpu_opes.py and tests/test_gpu_opes_paths.py rely on.  CPU only."""

from __future__ import annotations

import numpy as np
import pytest

from pmarlo_amd import _lib
from tests import _opes_ref as O

L = np.longdouble


def test_merge_conserves_the_moments():
    par = O.Params(2, 1.0, 10.0, threshold=50.0)
    c = np.array([[0.3, -0.2], [0.5, 0.1]])
    s = np.array([[0.2, 0.3], [0.25, 0.2]])
    h = np.array([0.7, 1.9])
    run = O.replay(par, c, s, h, np.log(h), dtype=L)
    assert run.K.tolist() == [1, 1] and run.death.tolist() == [1, O.ALIVE] and run.chain.tolist() == [0, 1]
    m = run.live[0]
    hc, hs = L(h)[:, None] * L(c), L(h)[:, None] * (L(s) ** 2 + L(c) ** 2)
    assert abs(m[4] - L(h).sum()) <= 4 * np.finfo(L).eps * L(h).sum()
    np.testing.assert_allclose(np.asarray(m[4] * m[:2], np.float64), np.asarray(hc.sum(axis=0), np.float64), rtol=1e-15)
    np.testing.assert_allclose(np.asarray(m[4] * (m[2:4] ** 2 + m[:2] ** 2), np.float64),
                               np.asarray(hs.sum(axis=0), np.float64), rtol=1e-15)


def test_threshold_zero_is_a_plain_truncated_kde():
    x, periods = O.trajectory(5, 40, 2, True)
    par = O.Params(2, 1.0, 10.0, periods=periods, sigma0=[0.25, 0.25], threshold=0.0)
    run = O.replay(par, x, dtype=L)
    assert run.K.tolist() == list(range(1, 41)) and (run.death == O.ALIVE).all() and not run.chain.any()
    s = np.array([[2.9, 0.1], [-3.0, 0.3]])
    got = O.bias(run, par, s)
    rec = run.records
    for f in range(2):
        dp = L(s[f])[None, :] - rec[:, :2]
        dp[:, 0] -= L(periods[0]) * np.rint(dp[:, 0] / L(periods[0]))
        q = ((dp / rec[:, 2:4]) ** 2).sum(axis=1)
        G = np.where(q < L(par.cut2), rec[:, 4] * (np.exp(-q / 2) - L(par.v)), L(0))
        P = G.sum() / np.exp(rec[:, 5]).sum()
        want = L(par.kTp) * np.log(P / O.full_z(run, par) + L(par.eps))
        assert abs(got["bias"][f] - want) <= 1e-17 * max(1.0, abs(float(want)))


def test_one_kernel_z():
    par = O.Params(1, 2.0, 12.0, sigma0=[0.3])
    lw = float(np.log(0.5))                      # the record holds the fp64 logweight; W = exp of that number
    run = O.replay(par, np.array([[0.4]]), np.array([[0.3]]), [0.8], [lw], dtype=L)
    want = (L(1) - L(par.v)) / np.exp(L(lw)) * L(0.8)
    assert abs(run.Z[0] - want) <= 4 * np.finfo(L).eps * want
    # before the first deposit: V = kT p log(eps), which makes the first on-line weight eps^p
    first = O.replay(par, np.array([[0.4]]), dtype=L)
    assert abs(np.exp(first.records[0, 3]) - L(par.eps) ** L(par.p)) <= 8 * np.finfo(L).eps
    assert O.bias(first, par, [[0.0]], counts=[0])["bias"][0] == L(par.kTp) * np.log(L(par.eps))


@pytest.mark.parametrize("periodic", [False, True])
def test_gradient_is_the_central_difference(periodic):
    x, par, rec, run = O.case(2, periodic)
    cv, times = O.frames(2, periodic, 12)
    counts = O.counts_from_times(np.arange(O.T_DEPOSITS), times)
    got = O.bias(run, par, cv, counts)
    step = 1e-7
    for i in range(2):
        e = np.zeros(2)
        e[i] = step
        fd = (O.bias(run, par, cv + e, counts)["bias"] - O.bias(run, par, cv - e, counts)["bias"]) / L(2 * step)
        err = np.abs(np.asarray(fd - got["grad"][:, i], np.float64))
        assert (err <= 1e-6 * np.maximum(1.0, np.abs(np.asarray(got["grad"][:, i], np.float64)))).all(), (i, err)
    assert np.abs(np.asarray(got["grad"], np.float64)).max() > 1e-3


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("d", O.DIMS)
def test_committed_sequences_exercise_what_the_gpu_tests_rely_on(d, periodic):
    x, par, rec, run = O.case(d, periodic)
    assert O.T_DEPOSITS > _lib.METAD_TILE and run.journal.shape == (O.T_DEPOSITS, 2 * d + 1)
    assert run.chain.max() >= 2, "no deposit with a chain of two merges"
    if periodic:
        assert run.periodic_merges >= 1, "no merge across the periodic boundary"
    assert min(run.margins) >= 1e-9, min(run.margins)
    # some versions die, some live to the end, and the live set is what the journal says it is
    alive = np.nonzero(run.death == O.ALIVE)[0]
    assert 0 < alive.size == run.K[-1] < O.T_DEPOSITS and sorted(run.live_version.tolist()) == alive.tolist()
    # the incrementally updated Z is the full double sum
    zf = O.full_z(run, par)
    assert abs(run.Z[-1] - zf) <= 1e-16 * zf
    if d >= 2:
        assert run.K[-1] > 64      # more than one slot per lane in the nearest search


def test_committed_online_sequence_has_the_margins_too():
    """the on-line run (heights and shrinking widths formed from the state) decides its merges on other numbers than the
    record replay: the GPU test compares its journal integers exactly, so it needs the same margins"""
    x, par, online = O.online_case()
    assert min(online.margins) >= 1e-9, min(online.margins)
    assert online.chain.max() >= 2 and online.periodic_merges >= 1 and 0 < online.K[-1] < O.T_DEPOSITS
