"""pmarlo_amd.reweight: temperature_weights and Reweighter on the device, and the hand-over of the weights to
prepare_msm_discretization."""
import numpy as np
import pytest

from pmarlo_amd import reweight
from pmarlo_amd.analysis.msm import prepare_msm_discretization
from tests import _mbar_ref as R

pytestmark = pytest.mark.gpu

TEMPS = np.array([300.0, 306.0, 312.0])


def ladder_frames(seed, n_per=400):
    rng = np.random.default_rng(seed)
    return R.ladder_energies(rng, TEMPS, n_per, offset=-1.0e3)


def test_frame_order_does_not_change_a_bit(engine):
    E, idx = ladder_frames(21, 150)
    w_sorted = reweight.temperature_weights(E, idx, TEMPS, 303.0, engine=engine)
    perm = np.random.default_rng(22).permutation(E.size)
    w_shuffled = reweight.temperature_weights(E[perm], idx[perm], TEMPS, 303.0, engine=engine)
    assert np.array_equal(w_shuffled.view(np.uint64), w_sorted[perm].view(np.uint64))
    assert abs(w_sorted.sum() - 1.0) <= E.size * R.ULP and (w_sorted > 0).all()


def test_weights_match_the_restatement(engine):
    E, idx = ladder_frames(23, 150)
    w, res = reweight.temperature_weights(E, idx, TEMPS, 303.0, engine=engine, return_result=True)
    order = np.lexsort((E, idx))
    u = (1.0 / (R.KB * TEMPS))[:, None] * E[order][None, :]
    ut = (E[order] / (R.KB * 303.0))[None, :]
    N_k = np.bincount(idx)
    d = R.mbar_pass(u, N_k, res.f_k, np.longdouble)["d"]
    R.check_targets((res.target_f, w[order][None, :], res.ess), R.target_weights(ut, d, np.longdouble),
                    R.target_bound(u, N_k, res.f_k, ut, d))


def test_one_rung_at_the_target_is_uniform(engine):
    E, _ = ladder_frames(24, 100)
    E = E[:100]
    w = reweight.temperature_weights(E, np.zeros(100, np.int64), [300.0], 300.0, engine=engine)
    # c_n = -u_n - d_n is a constant up to one rounding of d_n at |u_n| and one of the difference
    assert (np.abs(w * 100 - 1.0) <= 4 * R.ULP * np.abs(E / (R.KB * 300.0)).max() + 16 * R.ULP).all()


def test_bias_enters_the_reduced_potential(engine):
    E, idx = ladder_frames(25, 100)
    rng = np.random.default_rng(26)
    bias = 2.0 * rng.random((3, E.size))
    w, res = reweight.temperature_weights(E, idx, TEMPS, 303.0, bias=bias, engine=engine, return_result=True)
    order = np.lexsort((bias[2], bias[1], bias[0], E, idx))
    u = (1.0 / (R.KB * TEMPS))[:, None] * (E[order][None, :] + bias[:, order])
    ref = R.solve(u, np.bincount(idx))
    assert res.n_passes == ref["n_passes"]
    np.testing.assert_allclose(res.f_k, ref["f"], rtol=0, atol=1e-8)
    assert abs(w.sum() - 1.0) <= E.size * R.ULP


def three_splits():
    rng = np.random.default_rng(31)
    E, idx = R.ladder_energies(rng, TEMPS, 400, offset=-1.0e3)
    X = np.stack([E + 30.0 * rng.standard_normal(E.size), rng.standard_normal(E.size)], axis=1)
    splits = {
        "train": {"X": X[:400], "energy": E[:400], "temperature_K": 300.0},
        "val": {"X": X[400:800], "energy": E[400:800], "state_index": np.full(400, 1)},
        "test": {"X": X[800:], "energy": E[800:], "temperature_K": 312.0},
    }
    return {"splits": splits, "temperatures_K": TEMPS.copy()}, E, idx


def test_reweighter_feeds_the_discretization(engine):
    dataset, E, idx = three_splits()
    out = reweight.Reweighter(303.0, engine=engine).apply(dataset)
    assert list(out) == ["train", "val", "test"] and set(dataset["frame_weights"]) == set(out)
    total = sum(float(w.sum()) for w in out.values())
    assert all(w.shape == (400,) and (w > 0).all() for w in out.values()) and abs(total - 1.0) <= 1200 * R.ULP
    joint = reweight.temperature_weights(E, idx, TEMPS, 303.0, engine=engine)
    for name, sl in (("train", slice(0, 400)), ("val", slice(400, 800)), ("test", slice(800, 1200))):
        assert np.array_equal(out[name], joint[sl]) and np.array_equal(dataset["frame_weights"][name], out[name])
    # frames near the reference temperature weigh more than those of the far rung
    assert out["train"].sum() > out["test"].sum()

    picked_up = prepare_msm_discretization(dataset, n_microstates=5, lag_time=1, random_state=0)
    explicit = prepare_msm_discretization({"splits": {k: {"X": v["X"]} for k, v in dataset["splits"].items()}},
                                          n_microstates=5, lag_time=1, random_state=0,
                                          frame_weights={k: v.copy() for k, v in out.items()})
    unweighted = prepare_msm_discretization({"splits": {k: {"X": v["X"]} for k, v in dataset["splits"].items()}},
                                            n_microstates=5, lag_time=1, random_state=0)
    # the same labels; the weighted count kernel adds with fp64 atomics, so two runs over the same arrays agree up to
    # the order of at most 399 positive terms per cell: twice (n - 1) 2^-53 of the cell
    for name in out:
        assert np.array_equal(picked_up.assignments[name], explicit.assignments[name])
    np.testing.assert_allclose(picked_up.counts, explicit.counts, rtol=400 * R.ULP, atol=0)
    assert abs(picked_up.counts.sum() - out["train"][:-1].sum()) <= 400 * R.ULP * out["train"].sum()
    assert unweighted.counts.sum() == 399.0


def test_reweighter_validates(engine):
    with pytest.raises(ValueError, match="splits"):
        reweight.Reweighter(300.0, engine=engine).apply({})
    with pytest.raises(ValueError, match="energy"):
        reweight.Reweighter(300.0, engine=engine).apply({"splits": {"a": {"X": np.zeros((3, 1))}}})
    with pytest.raises(ValueError, match="temperature_K"):
        reweight.Reweighter(300.0, engine=engine).apply({"splits": {"a": {"energy": np.zeros(3)}}})
