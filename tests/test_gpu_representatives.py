"""RepresentativePicker on the device: the reference's recorded picks, edge shapes and ties against the numpy
restatement (exact picks), scores against bounds taken from the definitions, the grouping bit for bit, and the
errors that come from the device flags.

Score bounds (u = 2^-53, n_s members, d features):
  * centroid distance, absolute 4 n_s u sqrt(d) max|x|: two summation orders of the n_s-term weighted sums move a
    centroid coordinate by at most 2 n_s u max|x|, hence the distance by sqrt(d) times that; the rounding of the
    distance itself, (d + 4) u sqrt(d) max|x|, is below the other half for the n_s >= 256 used here.
  * medoid score, a sum of n_s non-negative terms, relative 4 (n_s + d) u: 2 n_s u for two orders of the sum and
    of the weight normalisation, 2 d u for the two distance evaluations."""

from __future__ import annotations

import numpy as np
import pytest

from pmarlo_amd import _lib
from pmarlo_amd.conformations import RepresentativePicker
from pmarlo_amd.markov_state_model import find_representatives
from tests import _representatives_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EDGE_SIZES = sorted({1, 2, 63, 64, 65, _lib.REP_TILE_I - 1, _lib.REP_TILE_I, _lib.REP_TILE_I + 1,
                     _lib.REP_TILE_J - 1, _lib.REP_TILE_J, _lib.REP_TILE_J + 1})


def _same_picks(got, want, method):
    if method == "diverse":
        assert got == want
    else:
        assert len(got) == len(want) and set(got) == set(want)
        assert {s: set(v) for s, v in R.by_state(got).items()} == {s: set(v) for s, v in R.by_state(want).items()}


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("name", [c[0] for c in R.GOLDEN_CASES])
def test_golden_picks(engine, golden, name, method):
    gold = [tuple(r) for r in golden("representatives.npz")[f"{name}/{method}/picks"].tolist()]
    x, dtrajs, state_ids, weights, n_reps = R.golden_case(name)
    got = RepresentativePicker().pick_representatives(x, list(dtrajs), state_ids, weights=weights, n_reps=n_reps,
                                                      method=method)
    _same_picks(got, gold, method)
    if method != "diverse":   # our order inside a state: ascending (score, frame)
        assert got == R.pick(x, dtrajs, state_ids, weights, n_reps, method)


def _edge_case(d, seed):
    """One state per size of EDGE_SIZES, shuffled, with labels -1 and >= k sprinkled in; two trajectories."""
    rng = np.random.default_rng(seed)
    k = len(EDGE_SIZES)
    labels = np.concatenate([np.full(n, s) for s, n in enumerate(EDGE_SIZES)] + [np.full(40, -1), np.full(40, k + 3)])
    rng.shuffle(labels)
    x = rng.standard_normal((labels.size, d)) + 2.0 * (labels[:, None] % 3)
    weights = rng.random(labels.size) + 0.05
    cut = labels.size // 3
    return x, [labels[:cut].copy(), labels[cut:].copy()], list(range(k)), weights


def _assert_exact_picks(got, x, dtrajs, state_ids, w, n_reps, method):
    """Equal lists.  Where the restatement's own scores leave the order of a state's picks undecided (neighbouring
    scores closer than 1e-9 relative: a mathematical tie that rounding breaks either way, as between the two members
    of a state of two and their midpoint), that state's picks must instead carry the same scores as the wanted ones
    to 1e-9; a `diverse` walk must then be the restatement's walk from the other nearest member."""
    want = R.pick(x, dtrajs, state_ids, w, n_reps, method)
    if got == want:
        return
    labels = np.concatenate(dtrajs)
    g, v = R.by_state(got), R.by_state(want)
    assert list(g) == list(v) and [r[0] for r in got] == [r[0] for r in want]
    for s in v:
        if g[s] == v[s]:
            continue
        frames = np.where(labels == s)[0]
        sc = R.scores_of(x, labels, s, w, method)
        if method == "diverse":
            assert R.ordering_margin(sc, 1) < 1e-9, (s, g[s], v[s])
            np.testing.assert_allclose(sc[np.searchsorted(frames, g[s][0])], sc.min(), rtol=1e-9, atol=0.0)
            assert g[s] == R.diverse_walk(x, frames, w, n_reps, start=g[s][0])
            continue
        assert R.ordering_margin(sc, n_reps) < 1e-9, (s, g[s], v[s])
        assert len(g[s]) == len(v[s]) == len(set(g[s]))
        sg = np.array([sc[np.searchsorted(frames, f)] for f in g[s]])
        sv = np.array([sc[np.searchsorted(frames, f)] for f in v[s]])
        np.testing.assert_allclose(sg, sv, rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("d", [1, 3, 10, 64, 65, 256])
def test_edge_shapes_exact_picks(engine, d, method):
    x, dtrajs, state_ids, weights = _edge_case(d, seed=d)
    picker = RepresentativePicker()
    for w in (None, weights):   # n_reps = 3 exceeds the states of 1 and 2 members
        got = picker.pick_representatives(x, dtrajs, state_ids, weights=w, n_reps=3, method=method)
        _assert_exact_picks(got, x, dtrajs, state_ids, w, 3, method)


def test_unsorted_repeated_and_sparse_state_ids(engine):
    rng = np.random.default_rng(11)
    labels = rng.choice([0, 5, 1999], size=700)
    x = rng.standard_normal((700, 4))
    ids = [1999, 0, 1999, 5]
    for method in R.METHODS:
        got = RepresentativePicker().pick_representatives(x, [labels], ids, n_reps=2, method=method)
        assert got == R.pick(x, [labels], ids, None, 2, method)
        assert [g[0] for g in got] == [1999, 1999, 0, 0, 1999, 1999, 5, 5]


@pytest.mark.parametrize("n,k", [(3000, 5), (2500, 1), (3100, 2000), (1, 3), (_lib.REP_GROUP_CHUNK + 1, 2)])
def test_grouping_is_np_where_bit_for_bit(engine, n, k):
    rng = np.random.default_rng(n + k)
    labels = rng.integers(-2, k + 2, size=n).astype(np.int32)   # some outside [0, k)
    if k == 2000:
        labels[rng.random(n) < 0.9] = 7   # most states empty, one large
    ld = engine.to_device(labels)
    runs = []
    for _ in range(2):
        off, mem = engine.group_by_label(ld, k)
        runs.append((off.to_host(), mem.to_host()))
    off, mem = runs[0]
    want = [np.where(labels == s)[0] for s in range(k)]
    assert off.dtype == np.int64 and mem.dtype == np.int32
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
    assert np.array_equal(mem[:off[-1]], np.concatenate(want))
    assert runs[1][0].tobytes() == off.tobytes() and runs[1][1][:off[-1]].tobytes() == mem[:off[-1]].tobytes()


def test_constant_features_give_the_lowest_frames_in_order(engine):
    n = 300
    labels = np.arange(n) % 2
    x = np.full((n, 1), 0.12345)
    got = RepresentativePicker().pick_representatives(x, [labels], [0], n_reps=3, method="diverse")
    assert [g[1] for g in got] == [0, 2, 4]
    for method in ("closest_to_centroid", "true_medoid"):
        got = RepresentativePicker().pick_representatives(x, [labels], [1, 0], n_reps=4, method=method)
        assert [g[1] for g in got] == [1, 3, 5, 7, 0, 2, 4, 6]


def test_duplicated_rows_take_the_lowest_frames(engine):
    rng = np.random.default_rng(5)
    base = rng.standard_normal((200, 6))
    x = base[rng.permutation(np.arange(400) // 2)]   # every row twice, scattered
    labels = rng.integers(0, 3, size=400)
    weights = np.ones(400)   # equal weights keep the two copies' scores the same bits
    for method in R.METHODS:
        got = RepresentativePicker().pick_representatives(x, [labels], [0, 1, 2], weights=weights, n_reps=6, method=method)
        assert got == R.pick(x, [labels], [0, 1, 2], weights, 6, method)


@pytest.mark.parametrize("weighted", [False, True])
def test_scores_within_the_bounds_of_the_definitions(engine, weighted):
    rng = np.random.default_rng(21)
    n, d, k = 3000, 10, 3
    labels = rng.integers(0, k, size=n)
    x = rng.standard_normal((n, d)) * 3.0 + labels[:, None]
    weights = rng.random(n) + 0.1 if weighted else None
    picker = RepresentativePicker()
    xmax = np.abs(x).max()
    for method in ("closest_to_centroid", "true_medoid", "diverse"):
        _, scores = picker.pick_representatives(x, [labels], range(k), weights=weights, n_reps=2, method=method,
                                                return_scores=True)
        for s in range(k):
            want = R.scores_of(x, labels, s, weights, method)
            ns = want.size
            assert scores[s].shape == want.shape
            if method == "true_medoid":
                err, bound = np.max(np.abs(scores[s] - want) / want), 4 * (ns + d) * U
            else:
                err, bound = np.max(np.abs(scores[s] - want)), 4 * ns * U * np.sqrt(d) * xmax
            print(f"{method} weighted={weighted} state {s} n_s={ns}: error {err:.3e} bound {bound:.3e}")
            assert err <= bound


def test_two_runs_give_identical_bytes(engine):
    x, dtrajs, state_ids, weights, n_reps = R.golden_case("n600_d3_weighted")
    for method in R.METHODS:
        a = RepresentativePicker().pick_representatives(x, list(dtrajs), state_ids, weights=weights, n_reps=n_reps,
                                                        method=method, return_scores=True)
        b = RepresentativePicker().pick_representatives(x, list(dtrajs), state_ids, weights=weights, n_reps=n_reps,
                                                        method=method, return_scores=True)
        assert a[0] == b[0]
        assert all(a[1][s].tobytes() == b[1][s].tobytes() for s in state_ids)


def test_weight_errors_come_from_the_first_offending_state(engine):
    rng = np.random.default_rng(2)
    labels = np.arange(90) % 3
    x = rng.standard_normal((90, 2))
    picker = RepresentativePicker()
    w = np.ones(90)
    w[labels == 2] = 0.0
    with pytest.raises(ValueError, match=r"Non-positive weight sum for state 2: 0\.0"):
        picker.pick_representatives(x, [labels], [0, 2, 1], weights=w)
    w[4] = -1.0   # state 1, listed after state 2
    with pytest.raises(ValueError, match="Non-positive weight sum for state 2"):
        picker.pick_representatives(x, [labels], [0, 2, 1], weights=w, method="true_medoid")
    with pytest.raises(ValueError, match="Negative weights for state 1"):
        picker.pick_representatives(x, [labels], [0, 1, 2], weights=w, method="diverse")
    w[7] = np.nan   # state 1 as well: the non-finite check comes first
    with pytest.raises(ValueError, match="Non-finite weights for state 1"):
        picker.pick_representatives(x, [labels], [1], weights=w)
    w[3] = np.inf   # state 0
    with pytest.raises(ValueError, match="Non-finite weights for state 0"):
        picker.pick_representatives(x, [labels], [0, 1], weights=w, method="diverse")
    with pytest.raises(ValueError, match="No frames found for state 3"):
        picker.pick_representatives(x, [labels], [0, 3], weights=np.ones(90))
    with pytest.raises(ValueError, match="No frames found for state 7"):   # before the weights of state 1
        picker.pick_representatives(x, [labels], [7, 1], weights=w)


def test_too_many_features_is_unsupported(engine):
    with pytest.raises(NotImplementedError, match="256"):
        RepresentativePicker().pick_representatives(np.zeros((4, 257)), [np.zeros(4, dtype=int)], [0])
    xd, ld = engine.to_device(np.zeros((4, 257))), engine.to_device(np.zeros(4, dtype=np.int32))
    off, mem = engine.group_by_label(ld, 1)
    with pytest.raises(NotImplementedError, match="d = 257"):
        engine.state_centroids(xd, off, mem)


def test_find_representatives_with_an_empty_state(engine):
    rng = np.random.default_rng(9)
    labels = rng.choice([0, 1, 3, 4], size=1300)   # state 2 is empty
    x = rng.standard_normal((1300, 5)) + labels[:, None]
    dtrajs = [labels[:500], labels[500:501], labels[501:]]
    frames, centroids = find_representatives(x, dtrajs, 5)
    assert frames[2] == (-1, -1) and centroids[2] is None
    for s in (0, 1, 3, 4):
        (_, g, traj, local), = R.pick(x, dtrajs, [s], None, 1, "closest_to_centroid")
        assert frames[s] == (traj, local)
        np.testing.assert_allclose(centroids[s], x[labels == s].mean(axis=0), rtol=1e-12, atol=1e-13)


def test_flux_and_committor_wrappers(engine):
    from oracle import npport
    from pmarlo_amd.markov_state_model.tpt import reactive_flux
    from tests.test_gpu_tpt import _metastable_T

    n = 12
    T = _metastable_T(n, seed=n)
    flux = reactive_flux(T, npport.stationary_distribution(T), [0, 1, 2], [n - 1, n - 2])
    rng = np.random.default_rng(4)
    labels = rng.integers(0, n, size=900)
    x = rng.standard_normal((900, 3)) + labels[:, None] * 0.5
    dtrajs = [labels[:300], labels[300:]]
    picker = RepresentativePicker()
    through = 0.5 * (flux.net_flux.sum(axis=1) + flux.net_flux.sum(axis=0))
    top = np.argsort(through)[::-1][:4]
    got = picker.pick_from_flux(flux.net_flux, x, dtrajs, top_n=4, n_reps_per_state=2)
    assert got == R.pick(x, dtrajs, top, None, 2, "closest_to_centroid")
    q = flux.forward_committor
    lo, hi = np.quantile(q, [0.3, 0.7])
    ts = np.where((q >= lo) & (q <= hi))[0]
    assert ts.size > 0
    got = picker.pick_from_committor_range(q, x, dtrajs, committor_range=(lo, hi), n_reps=5)
    assert got == R.pick(x, dtrajs, ts, None, 5, "diverse")
