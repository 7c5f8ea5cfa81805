"""The weighted VAMP-2 loss on the device: msm_vamp2_loss_weighted, msm_mlp_loss_grad_weighted and the weights of the
curriculum trainer, against the fp64 restatement (tests/_deeptica_weighted_ref.py) and the reference's recorded
values (tests/golden/deeptica_weighted*).

Yardsticks are those of tests/test_gpu_deeptica_train.py: fp64 against fp64 to 1e-10 (of the value, or for a
gradient of the larger of its largest entry and the size of the terms it is the sum of); parameter gradients within
1e-3 `ref_dev_grad` of the restatement per tensor."""

from __future__ import annotations

import json
import logging
from pathlib import Path

import numpy as np
import pytest

from tests import _deeptica_ref as R
from tests import _deeptica_train_ref as T
from tests import _deeptica_weighted_ref as WR

from pmarlo_amd.features.deeptica import CurriculumConfig, DeepTICACurriculumTrainer, DeepTICAModel

pytestmark = pytest.mark.gpu

GOLDEN_FILES = ("deeptica_weighted.npz", "deeptica_weighted_t3.npz", "deeptica_weighted_s600_0.npz",
                "deeptica_weighted_s600_1.npz", "deeptica_weighted_wide.npz")


@pytest.fixture(scope="module")
def gold(golden):
    arrays = {}
    for name in GOLDEN_FILES:
        arrays.update(golden(name))
    return arrays, json.loads((Path(__file__).parent / "golden" / "deeptica_weighted.json").read_text())


_LAW = {}


def _law(shape_key, pattern):
    """The restatement of a loss case, computed once and shared."""
    if (shape_key, pattern) not in _LAW:
        Y0, Yt, w, opts = WR.case(shape_key, pattern)
        _LAW[shape_key, pattern] = WR.vamp2_weighted(Y0, Yt, w, **opts)
    return _LAW[shape_key, pattern]


def _model(name):
    c = R.case(name)
    return DeepTICAModel.from_arrays(c["config"], c["params"], c["mean"], c["std"])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _grad_err(got, want, term_scale):
    return float(np.max(np.abs(got - want))) / max(float(np.max(np.abs(want))), term_scale)


# ---- 1. the loss ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape_key,pattern", WR.LOSS_CASES)
def test_weighted_vamp2_loss(engine, gold, shape_key, pattern):
    arrays, doc = gold
    Y0, Yt, w, opts = WR.case(shape_key, pattern)
    tag = f"{shape_key}__{pattern}"
    want, ref = _law(shape_key, pattern), doc["loss"][tag]
    got = engine.vamp2_loss(engine.to_device(Y0), engine.to_device(Yt), weights=w, **opts)
    for key in ("loss", "score"):
        print(f"{tag}: {key} device {got[key]!r} restatement {want[key]!r} reference {ref[key]!r}")
        assert abs(got[key] - want[key]) <= 1e-10 * abs(want[key])
        assert abs(got[key] - ref[key]) <= 1e-10 * abs(ref[key])
    for key in ("total_weight", "effective_pairs"):
        print(f"{tag}: {key} device {got[key]!r} restatement {want[key]!r}")
        assert abs(got[key] - want[key]) <= 1e-10 * want[key]
    assert len(got["metrics"]) == 10 and set(got["metrics"]) == set(ref["metrics"])
    for key, value in got["metrics"].items():
        for other in (want["metrics"][key], ref["metrics"][key]):
            err = np.max(np.abs(np.asarray(value) - np.asarray(other)))
            scale = np.max(np.abs(np.asarray(other)))
            print(f"{tag}: {key} |device - other| / largest = {err / scale:.2e}")
            assert err <= 1e-10 * scale
    g0, gt = got["grad0"].to_host(), got["grad_t"].to_host()
    for mine, law, rec in ((g0, want["grad0"], arrays[f"loss_g0__{tag}"]), (gt, want["grad_t"], arrays[f"loss_gt__{tag}"])):
        e_law, e_ref = _grad_err(mine, law, want["term_scale"]), _grad_err(mine, rec, want["term_scale"])
        print(f"{tag}: gradient |device - restatement| = {e_law:.2e}, |device - reference| = {e_ref:.2e}")
        assert e_law <= 1e-10 and e_ref <= 1e-10
    assert np.max(np.abs(want["grad0"])) > 1e-6 * want["term_scale"]              # a gradient, not noise
    assert np.all(g0[w <= 0] == 0.0) and np.all(gt[w <= 0] == 0.0)               # no weight, no gradient
    nograd = engine.vamp2_loss(engine.to_device(Y0), engine.to_device(Yt), weights=w, want_grad=False, **opts)
    assert "grad0" not in nograd and nograd["loss"] == got["loss"]


def test_padded_outputs_and_device_weights(engine):
    """The outputs as the left block of a wider buffer whose other columns are NaN, the weights already on the
    device: the same bits as the plain call."""
    Y0, Yt, w, opts = WR.case("s257", "zeros")
    m, d = Y0.shape
    plain = engine.vamp2_loss(engine.to_device(Y0), engine.to_device(Yt), weights=w, **opts)
    wide0, widet = np.full((m, d + 3), np.nan), np.full((m, d + 3), np.nan)
    wide0[:, :d], widet[:, :d] = Y0, Yt
    got = engine.vamp2_loss(engine.to_device(wide0).view((m, d)), engine.to_device(widet).view((m, d)), ld=d + 3,
                            weights=engine.to_device(w), **opts)
    assert got["loss"] == plain["loss"] and got["effective_pairs"] == plain["effective_pairs"]
    assert np.array_equal(_bits(got["grad0"].to_host()), _bits(plain["grad0"].to_host()))


# ---- 2. properties of the law --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape_key,pattern", [("t2", "lognormal"), ("s600", "chunk")])
def test_only_the_ratios_of_the_weights_matter(engine, shape_key, pattern):
    Y0, Yt, w, opts = WR.case(shape_key, pattern)
    y0, yt = engine.to_device(Y0), engine.to_device(Yt)
    a, b = engine.vamp2_loss(y0, yt, weights=w, **opts), engine.vamp2_loss(y0, yt, weights=1e6 * w, **opts)
    assert abs(a["loss"] - b["loss"]) <= 1e-10 * abs(a["loss"])
    assert abs(b["total_weight"] - 1e6 * a["total_weight"]) <= 1e-10 * b["total_weight"]
    assert abs(a["effective_pairs"] - b["effective_pairs"]) <= 1e-10 * a["effective_pairs"]
    scale = _law(shape_key, pattern)["term_scale"]
    for key in ("grad0", "grad_t"):
        assert _grad_err(b[key].to_host(), a[key].to_host(), scale) <= 1e-10


@pytest.mark.parametrize("shape_key", ["t1", "s257", "s600"])
def test_constant_weights_are_the_unweighted_loss(engine, shape_key):
    Y0, Yt, opts = WR.loss_case(shape_key)
    y0, yt = engine.to_device(Y0), engine.to_device(Yt)
    plain = engine.vamp2_loss(y0, yt, **opts)
    got = engine.vamp2_loss(y0, yt, weights=np.full(Y0.shape[0], 0.37), **opts)
    assert "total_weight" not in plain and "effective_pairs" not in plain
    assert abs(got["loss"] - plain["loss"]) <= 1e-10 * abs(plain["loss"])
    assert abs(got["score"] - plain["score"]) <= 1e-10 * abs(plain["score"])
    assert abs(got["effective_pairs"] - Y0.shape[0]) <= 1e-10 * Y0.shape[0]
    scale = T.vamp2(Y0, Yt, **opts)["term_scale"]
    for key in ("grad0", "grad_t"):
        assert _grad_err(got[key].to_host(), plain[key].to_host(), scale) <= 1e-10


def test_integer_weights_are_repeated_rows(engine):
    """Weights in {1, 2, 3} at (125, 17) against the unweighted loss of the batch with pair s repeated k_s times; the
    gradient of pair s is k_s times the gradient of one of its copies."""
    Y0, Yt, opts = WR.loss_case("t2")
    m = Y0.shape[0]
    k = np.random.default_rng(17).integers(1, 4, size=m)
    assert set(k.tolist()) == {1, 2, 3}
    rows = np.repeat(np.arange(m), k)
    first = np.concatenate([[0], np.cumsum(k)[:-1]])                            # one copy of every pair
    got = engine.vamp2_loss(engine.to_device(Y0), engine.to_device(Yt), weights=k.astype(np.float64), **opts)
    rep = engine.vamp2_loss(engine.to_device(np.ascontiguousarray(Y0[rows])),
                            engine.to_device(np.ascontiguousarray(Yt[rows])), **opts)
    assert abs(got["loss"] - rep["loss"]) <= 1e-10 * abs(rep["loss"])
    assert got["total_weight"] == float(k.sum())
    scale = T.vamp2(Y0[rows], Yt[rows], **opts)["term_scale"]
    for key in ("grad0", "grad_t"):
        want = k[:, None] * rep[key].to_host()[first]
        assert _grad_err(got[key].to_host(), want, 3.0 * scale) <= 1e-10


def test_equal_calls_give_equal_bits(engine):
    Y0, Yt, w, opts = WR.case("s600", "lognormal")
    y0, yt = engine.to_device(Y0), engine.to_device(Yt)
    runs = [engine.vamp2_loss(y0, yt, weights=w, **opts) for _ in range(2)]
    assert runs[0]["loss"] == runs[1]["loss"] and runs[0]["effective_pairs"] == runs[1]["effective_pairs"]
    for key in ("grad0", "grad_t"):
        assert np.array_equal(_bits(runs[0][key].to_host()), _bits(runs[1][key].to_host()))


# ---- 3. errors -----------------------------------------------------------------------------------------------------
def test_weights_that_carry_nothing_are_refused(engine):
    Y0, Yt, w, opts = WR.case("t1", "lognormal")
    y0, yt = engine.to_device(Y0), engine.to_device(Yt)
    with pytest.raises(ValueError, match="sum to zero"):
        engine.vamp2_loss(y0, yt, weights=np.zeros(Y0.shape[0]), **opts)
    with pytest.raises(ValueError, match="sum to zero"):
        engine.vamp2_loss(y0, yt, weights=-w, **opts)                            # all clamped to 0
    bad = w.copy()
    bad[4] = np.nan
    with pytest.raises(ValueError, match="finite"):
        engine.vamp2_loss(y0, yt, weights=bad, **opts)
    with pytest.raises(ValueError, match="36 weights for 37"):
        engine.vamp2_loss(y0, yt, weights=w[:-1], **opts)
    with pytest.raises(TypeError):
        engine.vamp2_loss(y0, yt, weights=engine.to_device(w.astype(np.float32)), **opts)
    # on the device nothing is checked before the launch: the kernel's flag raises
    with pytest.raises(RuntimeError, match="weights"):
        engine.vamp2_loss(y0, yt, weights=engine.zeros((Y0.shape[0],), np.float64), **opts)
    with pytest.raises(RuntimeError, match="weights"):
        engine.vamp2_loss(y0, yt, weights=engine.to_device(bad), **opts)
    assert np.isfinite(engine.vamp2_loss(y0, yt, weights=w, **opts)["loss"])      # usable afterwards


# ---- 4. loss and parameter gradient --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WR.NET_CASES)
def test_weighted_mlp_loss_grad(engine, gold, name):
    arrays, doc = gold
    X, (it, itau), w = T.train_frames(name), T.pairs(name, "a"), WR.net_weights(name)
    law = WR.loss_grad_weighted(name, X, it, itau, w)
    rec = doc["grad"][f"{name}__a"]
    xd, spec = engine.to_device(X), _model(name).spec
    got = engine.mlp_loss_grad(xd, spec, it, itau, weights=w, want_outputs=True, **T.LOSS_OPTS)
    for key in ("loss", "score", "total_weight", "effective_pairs"):
        print(f"{name}: {key} device {got[key]!r} restatement {law[key]!r}")
        assert abs(got[key] - law[key]) <= 1e-10 * abs(law[key])
    c = R.case(name)
    by_key = T.unpack(c["config"], c["X"].shape[1], got["grad"].to_host())
    for key, dev in rec["ref_dev_grad"].items():
        e_law = float(np.max(np.abs(by_key[key] - law["grads"][key])))
        e_ref = float(np.max(np.abs(by_key[key] - arrays[f"grad__{name}__a__{key}"])))
        print(f"{name} {key}: |device - restatement| = {e_law / dev:.2e}, |device - reference| = {e_ref / dev:.3f} ref_dev_grad")
        assert e_law <= 1e-3 * dev
        assert e_ref <= 1.5 * dev
    # weights=None is today's function: the same bits with and without the keyword, and no weight figures
    plain = engine.mlp_loss_grad(xd, spec, it, itau, want_outputs=True, **T.LOSS_OPTS)
    again = engine.mlp_loss_grad(xd, spec, it, itau, weights=None, want_outputs=True, work=got["work"], **T.LOSS_OPTS)
    assert plain["loss"] == again["loss"] and "total_weight" not in again
    assert np.array_equal(_bits(plain["grad"].to_host()), _bits(again["grad"].to_host()))
    law_plain = T.loss_grad(name, X, it, itau)
    assert abs(plain["loss"] - law_plain["loss"]) <= 1e-10 * abs(law_plain["loss"])
    # the forward pass does not see the weights
    assert np.array_equal(_bits(plain["outputs"].to_host()), _bits(got["outputs"].to_host()))
    assert np.max(np.abs(plain["grad"].to_host() - got["grad"].to_host())) > 1e-3 * np.max(np.abs(law["grad"]))


# ---- 5. the trainer ------------------------------------------------------------------------------------------------
def test_weighted_train_steps_follow_the_law(engine):
    name = "flagship"
    model = _model(name)
    model.config["dropout"] = 0.1
    cfg = CurriculumConfig(seed=3, learning_rate=1e-3, weight_decay=1e-4, grad_clip_norm=1.0)
    trainer = DeepTICACurriculumTrainer(model, cfg, engine=engine)
    X = T.train_frames(name)
    trainer.set_frames(X)
    opts = {"eps": cfg.vamp_eps, "eps_abs": cfg.vamp_eps_abs, "alpha": cfg.vamp_alpha, "cond_reg": cfg.vamp_cond_reg}
    for which in ("a", "b"):
        it, itau = T.pairs(name, which)
        w = WR.net_weights(name, which)
        p0, m0, v0 = trainer.state()
        step = trainer.step
        out = trainer.train_step(it, itau, w)
        law = WR.loss_grad_weighted(name, X, it, itau, w, packed=p0, dropout=trainer.dropout, seed=3, step=step, opts=opts)
        p1, m1, v1, norm, norm_clipped, _ = T.adamw(p0, law["grad"], m0, v0, step + 1, 1e-3, wd=1e-4, clip=1.0)
        p, m, v = trainer.state()
        assert trainer.step == step + 1 and out["batch_size"] == len(it)
        assert abs(out["loss"] - law["loss"]) <= 1e-10 * abs(law["loss"])
        assert abs(out["effective_pairs"] - law["effective_pairs"]) <= 1e-10 * law["effective_pairs"]
        assert abs(out["grad_norm_preclip"] - norm) <= 1e-10 * norm
        assert abs(out["grad_norm"] - norm_clipped) <= 1e-10 * norm_clipped
        rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))       # noqa: E731
        print(f"step {step + 1}: m {rel(m, m1):.2e}, v {rel(v, v1):.2e} of the largest entry")
        assert rel(m, m1) <= 1e-12 and rel(v, v1) <= 1e-12
        assert np.all(np.abs(p.astype(np.float64) - p1.astype(np.float64)) <= T.ulp32(p1))
        assert np.any(p != p0)
    # evaluate weights batches by their total weight: one batch is the weighted loss itself
    it, itau = T.pairs(name, "a")
    w = WR.net_weights(name, "a")
    p0 = trainer.state()[0]
    law = WR.loss_grad_weighted(name, X, it, itau, w, packed=p0, opts=opts)
    ev = trainer.evaluate(it, itau, w)
    assert abs(ev["loss"] - law["loss"]) <= 1e-10 * abs(law["loss"])


def test_fit_with_and_without_weights(engine, caplog):
    keys = json.loads((Path(__file__).parent / "golden" / "deeptica_train.json").read_text())["history_keys"]
    seq = T.toy_sequence()[:600]
    cfg = CurriculumConfig(seed=1, tau_schedule=(2,), val_tau=2, epochs_per_tau=2, warmup_epochs=1, learning_rate=1e-2,
                           batch_size=128)

    def fresh():
        return DeepTICACurriculumTrainer(DeepTICAModel.initialize(T.TOY_CONFIG, np.zeros(7), np.ones(7), seed=1), cfg,
                                         engine=engine)

    plain = fresh().fit([seq])
    assert list(plain) == keys and len(plain) == 32

    rng = np.random.default_rng(3)
    fw = np.exp(rng.normal(size=600))
    trainer = fresh()
    hist = trainer.fit([seq], frame_weights=[fw])
    assert list(hist) == keys + ["weighted_loss", "effective_pairs_curve"] and hist["weighted_loss"] is True
    assert len(hist["effective_pairs_curve"]) == len(hist["loss_curve"]) == 2
    assert all(2.0 < e < 128.0 for e in hist["effective_pairs_curve"])           # Kish: below the batch size
    assert hist["loss_curve"] != plain["loss_curve"]
    # the validation part took the tail of the weights: evaluating with them gives the recorded best score
    split = 600 - trainer.val_pairs[0].size - 2
    assert np.array_equal(trainer.val_pair_weights, fw[split:][: trainer.val_pairs[0].size])
    assert trainer.evaluate(*trainer.val_pairs, trainer.val_pair_weights)["score"] == hist["best_val_score"]
    # constant frame weights train exactly as no weights do up to rounding of the loss
    const = fresh().fit([seq], frame_weights=[np.full(600, 2.0)])
    assert np.allclose(const["loss_curve"], plain["loss_curve"], rtol=1e-6)
    assert np.allclose(const["effective_pairs_curve"], [np.mean([128, 128, 128, 94])] * 2, rtol=1e-12)
    with pytest.raises(ValueError, match="one weight per frame"):
        fresh().fit([seq], frame_weights=[fw[:-1]])
    with pytest.raises(ValueError, match="no positive weight"):
        fresh().fit([seq], frame_weights=[np.zeros(600)])
    # a batch whose weight sits on two pairs is trained on, with a warning
    spiky = np.full(600, 1e-12)
    spiky[[10, 300]] = 1.0
    quiet = DeepTICACurriculumTrainer(DeepTICAModel.initialize(T.TOY_CONFIG, np.zeros(7), np.ones(7), seed=1),
                                      CurriculumConfig(seed=1, tau_schedule=(2,), val_tau=2, epochs_per_tau=1,
                                                       batch_size=512, shuffle=False), engine=engine)
    with caplog.at_level(logging.WARNING, logger="pmarlo_amd.features.deeptica.trainer"):
        quiet.fit([seq], frame_weights=[spiky])
    assert any("effective pairs" in r.getMessage() for r in caplog.records)
