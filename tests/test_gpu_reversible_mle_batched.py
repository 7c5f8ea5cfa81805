"""Batched reversible maximum-likelihood estimate on the GPU (msm_reversible_mle_batched) against its numpy
restatement (tests/_kis_ref.reversible_mle_packed: the active set, then oracle/npport.reversible_mle on
C[active, active] + 1e-3) on both launch paths: the symmetrised block in LDS up to
msm_reversible_mle_batched_lds_max_n(), streamed from the scratch above.

deeptime's MaximumLikelihoodMSM(reversible=True) is absent (parity unpinned); both sides iterate the published fixed
point, so at a tight stopping rule they agree to the 1e-9 tests/test_gpu_revmle.py holds the single-matrix kernel to,
whatever the iteration count."""
import functools

import numpy as np
import pytest

from oracle import npport
from pmarlo_amd import _lib
from tests import _kis_ref as R

pytestmark = pytest.mark.gpu

N_LDS = int(_lib.load().msm_reversible_mle_batched_lds_max_n())
N_DISTINCT = 3          # a batch cycles through this many count matrices: their references are computed once
# Four blocks on five states are four nearly closed single states: every such matrix needs tens of thousands of
# iterations (20792 to over 200000 at 1e-13 for seeds 0 .. 11).  These three are the quickest for the reference.
SEEDS = {5: (11, 1, 9)}


@functools.lru_cache(maxsize=None)
def _distinct_counts(k, d):
    C = R.block_counts(k, SEEDS[k][d] if k in SEEDS else 1000 * k + d)
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def _distinct_ref(k, d, maxerr):
    return R.reversible_mle_packed(_distinct_counts(k, d), maxerr=maxerr)


def _counts(k, b):
    return _distinct_counts(k, b % N_DISTINCT)


def _ref(k, b, maxerr):
    return _distinct_ref(k, b % N_DISTINCT, maxerr)


def _batch(k, batch):
    return np.stack([_counts(k, b) for b in range(batch)])


def _run(engine, C, **kw):
    out = engine.reversible_mle_batched(engine.to_device(np.ascontiguousarray(C, np.int64)), **kw)
    return {"T": out["T"].to_host(), "pi": out["pi"].to_host(), "active": out["active"].to_host(),
            "n_active": out["n_active"].to_host(), "iterations": out["iterations"], "err": out["err"]}


def _check_packed(got, b, ref, k, rtol=1e-9):
    n = ref["n_active"]
    assert got["n_active"][b] == n
    assert np.array_equal(got["active"][b], ref["active"])
    T, pi = got["T"][b], got["pi"][b]
    assert not np.any(T[n:]) and not np.any(T[:, n:]) and not np.any(pi[n:])          # the padding is exact
    np.testing.assert_allclose(T, ref["T"], rtol=rtol, atol=1e-15)
    np.testing.assert_allclose(pi, ref["pi"], rtol=rtol)
    np.testing.assert_allclose(T[:n, :n].sum(axis=1), 1.0, rtol=0, atol=1e-13)
    flux = pi[:n, None] * T[:n, :n]
    np.testing.assert_allclose(flux, flux.T, rtol=1e-9, atol=1e-18)                   # detailed balance


def test_lds_boundary_is_exported():
    assert 64 < N_LDS < 200
    lib = _lib.load()
    assert lib.msm_reversible_mle_batched_scratch_bytes(N_LDS, 7) == 0
    assert lib.msm_reversible_mle_batched_scratch_bytes(N_LDS + 1, 7) == 7 * (N_LDS + 1) ** 2 * 8


@pytest.mark.parametrize("batch", [1, 3, 33])
@pytest.mark.parametrize("k", [2, 5, 63, 64, 65, N_LDS, N_LDS + 1, 200])
def test_vs_reference_at_a_tight_stop(engine, k, batch):
    got = _run(engine, _batch(k, batch), maxerr=1e-13)
    assert got["T"].shape == (batch, k, k) and got["pi"].shape == (batch, k)
    for b in range(batch):
        _check_packed(got, b, _ref(k, b, 1e-13), k)
        assert got["err"][b] <= 1e-13


@pytest.mark.parametrize("k", [5, 64, N_LDS + 1])
def test_default_stopping_rule_and_cap(engine, k):
    batch = 3
    got = _run(engine, _batch(k, batch))
    for b in range(batch):
        ref = _ref(k, b, 1e-8)
        print(f"k={k} b={b}: {got['iterations'][b]} iterations (reference {ref['iterations']}), err {got['err'][b]:.3e}")
        assert abs(int(got["iterations"][b]) - ref["iterations"]) <= 1     # rounding next to the threshold
        assert got["err"][b] <= 1e-8
    capped = _run(engine, _batch(k, batch), maxerr=1e-300, maxiter=50)
    assert np.array_equal(capped["iterations"], np.full(batch, 50))


@functools.lru_cache(maxsize=None)
def _metastable_counts(seed):
    """Counts of 8 x 4000 frames of a four-block chain on 40 states that leaves a block once in 100 to 250 steps."""
    T = R.leaky_block_chain(40, 4, seed, (0.004, 0.006, 0.008, 0.01))
    return npport._pair_counts(R.trajectories(T, 8, 4000, seed + 1), 40, 1).astype(np.int64)


def test_uneven_batch(engine):
    """One matrix that is its own fixed point between matrices that need thousands of iterations: every matrix
    stops at its own count."""
    sym = R.block_counts(40, 7)
    sym = sym + sym.T
    C = np.stack([_metastable_counts(1), sym, _metastable_counts(2)])
    refs = [R.reversible_mle_packed(c) for c in C]
    assert refs[0]["iterations"] >= 1000 and refs[2]["iterations"] >= 1000 and refs[1]["iterations"] <= 3
    got = _run(engine, C)
    print("iterations", got["iterations"], "reference", [r["iterations"] for r in refs])
    assert got["iterations"][1] <= 3
    for b in range(3):
        assert abs(int(got["iterations"][b]) - refs[b]["iterations"]) <= 1
        assert got["err"][b] <= 1e-8
    reg = sym + R.ALPHA
    np.testing.assert_allclose(got["T"][1], reg / reg.sum(axis=1, keepdims=True), rtol=1e-12)
    np.testing.assert_allclose(got["pi"][1], reg.sum(axis=1) / reg.sum(), rtol=1e-12)


@pytest.mark.parametrize("k", [40, N_LDS + 1])
def test_batch_independence(engine, k):
    """Matrix b alone has the bits it has inside the batch."""
    C = _batch(k, 5)
    C[3, 1, :] = 0
    C[3, :, 1] = 0                                           # one with an inactive state
    together = _run(engine, C)
    for b in (0, 3, 4):
        alone = _run(engine, C[b:b + 1])
        for name in ("T", "pi", "active", "n_active", "iterations", "err"):
            assert np.array_equal(alone[name][0], together[name][b]), (name, b)


def _without(C, states):
    C = C.copy()
    C[states, :] = 0
    C[:, states] = 0
    return C


@pytest.mark.parametrize("k", [12, N_LDS + 1])
def test_inactive_states(engine, k):
    base = _counts(k, 0)
    cases = [_without(base, [0]), _without(base, [k - 1]), _without(base, [k // 2]), _without(base, [0, k // 2, k - 1]),
             _without(base, [s for s in range(k) if s not in (3, 4)]), np.zeros((k, k), np.int64), base.copy()]
    got = _run(engine, np.stack(cases), maxerr=1e-13)
    want_n = [k - 1, k - 1, k - 1, k - 3, 2, 0, k]
    assert got["n_active"].tolist() == want_n
    for b, C in enumerate(cases):
        ref = R.reversible_mle_packed(C, maxerr=1e-13) if b < len(cases) - 1 else _ref(k, 0, 1e-13)
        _check_packed(got, b, ref, k)
    assert got["active"][4].tolist() == [3, 4] + [-1] * (k - 2)
    # the empty matrix: nothing to iterate, a zero slot, and its neighbours are the estimates they are alone
    assert got["iterations"][5] == 0 and got["err"][5] == 0.0 and not np.any(got["T"][5]) and not np.any(got["pi"][5])
    assert np.all(got["active"][5] == -1)
    # a state that only receives (a column, no row) is active
    C = _without(base, [1])
    C[0, 1] = 4
    one = _run(engine, C[None], maxerr=1e-13)
    assert one["n_active"][0] == k
    _check_packed(one, 0, R.reversible_mle_packed(C, maxerr=1e-13), k)


@pytest.mark.parametrize("k", [12, N_LDS + 1])
def test_negative_count(engine, k):
    """A negative count makes that matrix's err infinite by arithmetic alone; the others are the estimates they are
    without it."""
    C = _batch(k, 3)
    C[1, 2, 5] = -3
    got = _run(engine, C, maxerr=1e-13)
    assert np.isposinf(got["err"][1]) and got["iterations"][1] == 0
    assert not np.any(got["T"][1]) and not np.any(got["pi"][1])
    for b in (0, 2):
        _check_packed(got, b, _ref(k, b, 1e-13), k)
        assert got["err"][b] <= 1e-13


def test_argument_errors(engine):
    with pytest.raises(TypeError):
        engine.reversible_mle_batched(engine.to_device(np.zeros((2, 3, 3))))
    with pytest.raises(ValueError, match="maxerr > 0"):
        engine.reversible_mle_batched(engine.to_device(np.zeros((1, 3, 3), np.int64)), maxerr=0.0)
    with pytest.raises(ValueError, match="alpha >= 0"):
        engine.reversible_mle_batched(engine.to_device(np.zeros((1, 3, 3), np.int64)), alpha=-1.0)
