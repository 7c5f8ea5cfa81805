"""The weighted VAMP-2 restatement (tests/_deeptica_weighted_ref.py) against the reference's recorded values
(tests/golden/deeptica_weighted*): VAMP2Loss.forward(z0, zt, weights)'s loss, score, metrics and autograd output
gradients, and the reference network's fp32 parameter gradients under weights.  CPU only.

Tolerances are those of tests/test_deeptica_train_host.py: 1e-10 between two fp64 routes through the law (the golden
maker refused anything above 1e-12 where it ran), and `ref_dev_grad` for the reference's fp32 network."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

from tests import _deeptica_train_ref as T
from tests import _deeptica_weighted_ref as WR

GOLDEN_FILES = ("deeptica_weighted.npz", "deeptica_weighted_t3.npz", "deeptica_weighted_s600_0.npz",
                "deeptica_weighted_s600_1.npz", "deeptica_weighted_wide.npz")


@pytest.fixture(scope="module")
def gold(golden):
    arrays = {}
    for name in GOLDEN_FILES:
        arrays.update(golden(name))
    return arrays, json.loads((Path(__file__).parent / "golden" / "deeptica_weighted.json").read_text())


def test_the_cases_are_the_issue_s(gold):
    _, doc = gold
    assert sorted(doc["loss"]) == sorted(f"{s}__{p}" for s, p in WR.LOSS_CASES)
    shapes = {s: WR.loss_case(s)[0].shape for s in WR.SHAPE_KEYS}
    assert shapes == {"t1": (37, 3), "t2": (125, 17), "t3": (250, 64), "s257": (257, 5), "s600": (600, 33)}
    for s, p in WR.LOSS_CASES:
        w = WR.weights(s, shapes[s][0], p)
        assert np.count_nonzero(w > 0) >= shapes[s][1] + 2
        if p == "zeros":
            assert np.all(w[::3] == 0.0) and np.count_nonzero(w < 0) == 1
        if p == "float32":
            assert np.array_equal(w, w.astype(np.float32).astype(np.float64))
        if p == "chunk":
            assert np.all(w[256:512] == 0.0) and np.all(w[:256] > 0) and np.all(w[512:] > 0)


@pytest.mark.parametrize("shape_key,pattern", WR.LOSS_CASES)
def test_restated_weighted_loss_matches_the_reference(gold, shape_key, pattern):
    arrays, doc = gold
    Y0, Yt, w, opts = WR.case(shape_key, pattern)
    tag = f"{shape_key}__{pattern}"
    mine, ref = WR.vamp2_weighted(Y0, Yt, w, **opts), doc["loss"][tag]
    assert abs(mine["loss"] - ref["loss"]) <= 1e-10 * abs(ref["loss"])
    assert abs(mine["score"] - ref["score"]) <= 1e-10 * abs(ref["score"])
    assert list(mine["metrics"]) == list(ref["metrics"])
    for key, value in ref["metrics"].items():
        assert np.max(np.abs(np.asarray(mine["metrics"][key]) - np.asarray(value))) <= 1e-10 * np.max(np.abs(value))
    for g, rec in ((mine["grad0"], arrays[f"loss_g0__{tag}"]), (mine["grad_t"], arrays[f"loss_gt__{tag}"])):
        scale = max(float(np.max(np.abs(rec))), mine["term_scale"])
        assert np.max(np.abs(g - rec)) <= 1e-10 * scale
    # a pair without weight has no gradient, in the reference as here
    dead = np.asarray(w) <= 0
    assert np.all(mine["grad0"][dead] == 0.0) and np.all(arrays[f"loss_g0__{tag}"][dead] == 0.0)


def test_the_weighted_law_reduces_to_the_unweighted_one():
    Y0, Yt, opts = WR.loss_case("t2")
    plain, const = T.vamp2(Y0, Yt, **opts), WR.vamp2_weighted(Y0, Yt, np.full(Y0.shape[0], 3.0), **opts)
    assert abs(plain["loss"] - const["loss"]) <= 1e-12 * abs(plain["loss"])
    assert np.max(np.abs(plain["grad0"] - const["grad0"])) <= 1e-12 * plain["term_scale"]
    assert const["total_weight"] == 3.0 * Y0.shape[0] and abs(const["effective_pairs"] - Y0.shape[0]) <= 1e-9
    with pytest.raises(ValueError):
        WR.vamp2_weighted(Y0, Yt, np.zeros(Y0.shape[0]), **opts)


@pytest.mark.parametrize("name", WR.NET_CASES)
def test_restated_weighted_parameter_gradients_match_the_reference(gold, name):
    arrays, doc = gold
    rec = doc["grad"][f"{name}__a"]
    it, itau = T.pairs(name, "a")
    mine = WR.loss_grad_weighted(name, T.train_frames(name), it, itau, WR.net_weights(name))
    assert abs(mine["loss"] - rec["loss"]) <= 1e-5 * abs(rec["loss"])                # the reference's network is fp32
    for key, dev in rec["ref_dev_grad"].items():
        got = float(np.max(np.abs(mine["grads"][key] - arrays[f"grad__{name}__a__{key}"])))
        assert got <= dev * (1.0 + 1e-9) + 1e-300, (key, got, dev)
    # the weights did act: the unweighted gradient is another one
    plain = T.loss_grad(name, T.train_frames(name), it, itau)
    assert np.max(np.abs(plain["grad"] - mine["grad"])) > 1e-3 * np.max(np.abs(plain["grad"]))
