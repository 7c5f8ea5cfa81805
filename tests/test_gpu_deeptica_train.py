"""DeepTICA training on the device: msm_vamp2_loss, msm_mlp_loss_grad, msm_adamw_step and the curriculum trainer
against the fp64 restatement (tests/_deeptica_train_ref.py) and the reference's recorded values
(tests/golden/deeptica_train.*).

Yardsticks.  The loss kernels are fp64 against fp64: 1e-10 of the largest entry (two fp64 routes through the law
differ by <= 2.5e-13 at cond 1.6e3, and the smallest term of the law, the condition penalty, is five orders above
1e-10).  Parameter gradients use `ref_dev_grad`, the distance of the reference's own fp32 gradient from the exact
law, per tensor: the device computes in fp64 and must sit within 1e-3 ref_dev_grad of the restatement and within
1.5 ref_dev_grad of the reference's gradient, as tests/test_gpu_deeptica.py does for the outputs."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

from tests import _deeptica_ref as R
from tests import _deeptica_train_ref as T

from pmarlo_amd.features.deeptica import CurriculumConfig, DeepTICACurriculumTrainer, DeepTICAModel
from pmarlo_amd.features.deeptica.trainer import lagged_pairs, lr_schedule, split_train_val

pytestmark = pytest.mark.gpu

GRAD_CASES = [(n, w) for n in R.CASES for w in ("a", "b")] + [("wide", "c")]


@pytest.fixture(scope="module")
def gold(golden):
    arrays = dict(golden("deeptica_train.npz"))
    for w in "abc":
        arrays.update(golden(f"deeptica_train_wide_{w}.npz"))
    return arrays, json.loads((Path(__file__).parent / "golden" / "deeptica_train.json").read_text())


def _model(name):
    """A fresh model of a case (training changes its parameters on the device)."""
    c = R.case(name)
    return DeepTICAModel.from_arrays(c["config"], c["params"], c["mean"], c["std"])


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _model(name)
        return cache[name]

    return get


_LAW = {}


def _law(name, which, **kw):
    """The restatement of a case and pair set, computed once and shared."""
    key = (name, which, json.dumps(kw, sort_keys=True))
    if key not in _LAW:
        it, itau = T.pairs(name, which)
        _LAW[key] = T.loss_grad(name, T.train_frames(name), it, itau, **kw)
    return _LAW[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / np.max(np.abs(want)))


def _by_key(name, packed):
    c = R.case(name)
    return T.unpack(c["config"], c["X"].shape[1], np.asarray(packed))


# ---- 1. the loss ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,pad", [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (2, 3)])
def test_vamp2_loss(engine, gold, i, pad):
    arrays, doc = gold
    Y0, Yt, opts = T.loss_case(i)
    m, d = Y0.shape
    want, ref = T.vamp2(Y0, Yt, **opts), doc["loss"][i]
    if pad:     # the outputs as the left block of a wider buffer whose other columns are NaN and must not be read
        wide0, widet = np.full((m, d + pad), np.nan), np.full((m, d + pad), np.nan)
        wide0[:, :d], widet[:, :d] = Y0, Yt
        got = engine.vamp2_loss(engine.to_device(wide0).view((m, d)), engine.to_device(widet).view((m, d)), ld=d + pad,
                                **opts)
    else:
        got = engine.vamp2_loss(engine.to_device(Y0), engine.to_device(Yt), **opts)
    for key in ("loss", "score"):
        print(f"case {i}: {key} device {got[key]!r} restatement {want[key]!r} reference {ref[key]!r}")
        assert abs(got[key] - want[key]) <= 1e-10 * abs(want[key])
        assert abs(got[key] - ref[key]) <= 1e-10 * abs(ref[key])
    assert set(got["metrics"]) == set(ref["metrics"])
    for key, value in got["metrics"].items():
        for other in (want["metrics"][key], ref["metrics"][key]):
            err = np.max(np.abs(np.asarray(value) - np.asarray(other)))
            scale = np.max(np.abs(np.asarray(other)))
            print(f"case {i}: {key} |device - other| / largest = {err / scale:.2e}")
            assert err <= 1e-10 * scale
    # the gradients, against the largest entry; where the two terms a gradient is the sum of cancel altogether
    # (two pairs, one output: the score is a constant) the largest entry is rounding noise, and the terms' size
    # takes its place
    g0, gt = got["grad0"].to_host(), got["grad_t"].to_host()
    for mine, law, rec in ((g0, want["grad0"], arrays[f"loss_g0__{i}"]), (gt, want["grad_t"], arrays[f"loss_gt__{i}"])):
        top = float(np.max(np.abs(law)))
        scale = top if top > 1e-6 * want["term_scale"] else want["term_scale"]
        e_law, e_ref = float(np.max(np.abs(mine - law))) / scale, float(np.max(np.abs(mine - rec))) / scale
        print(f"case {i}: gradient |device - restatement| = {e_law:.2e}, |device - reference| = {e_ref:.2e} of {scale:.3e}")
        assert e_law <= 1e-10 and e_ref <= 1e-10
    if i < 4:
        assert np.max(np.abs(want["grad0"])) > 1e-6 * want["term_scale"]      # a gradient, not noise
    nograd = engine.vamp2_loss(engine.to_device(Y0), engine.to_device(Yt), want_grad=False, **opts)
    assert "grad0" not in nograd and nograd["loss"] == engine.vamp2_loss(engine.to_device(Y0), engine.to_device(Yt),
                                                                           **opts)["loss"]


# ---- 2. loss and gradient, dropout off -----------------------------------------------------------------------------
def _check_grad(name, which, got_packed, law, gold, against_reference=True):
    arrays, doc = gold
    rec = doc["grad"][f"{name}__{which}"]
    got = _by_key(name, got_packed)
    for key, dev in rec["ref_dev_grad"].items():
        e_law = float(np.max(np.abs(got[key] - law["grads"][key])))
        msg = f"{name}/{which} {key}: |device - restatement| = {e_law:.3e} = {e_law / dev:.2e} ref_dev_grad"
        if against_reference:
            e_ref = float(np.max(np.abs(got[key] - arrays[f"grad__{name}__{which}__{key}"])))
            msg += f"; |device - reference| = {e_ref / dev:.3f} ref_dev_grad"
        print(msg)
        assert e_law <= 1e-3 * dev
        if against_reference:
            assert e_ref <= 1.5 * dev


@pytest.mark.parametrize("name,which", GRAD_CASES)
def test_loss_grad_without_dropout(engine, models, gold, name, which):
    X = T.train_frames(name)
    it, itau = T.pairs(name, which)
    law = _law(name, which)
    xd = engine.to_device(X)
    got = engine.mlp_loss_grad(xd, models(name).spec, it, itau, want_outputs=True, **T.LOSS_OPTS)
    rec = gold[1]["grad"][f"{name}__{which}"]
    for key in ("loss", "score"):
        print(f"{name}/{which}: {key} device {got[key]!r} restatement {law[key]!r} reference (fp32) {rec[key]!r}")
        assert abs(got[key] - law[key]) <= 1e-10 * abs(law[key])
    _check_grad(name, which, got["grad"].to_host(), law, gold)
    # the outputs are those of the inference kernel on the gathered rows, bit for bit
    rows = np.concatenate([it, itau])
    fwd = engine.mlp_forward(engine.to_device(np.ascontiguousarray(X[rows])), models(name).spec).to_host()
    out = got["outputs"].to_host()
    assert out.shape == fwd.shape and np.array_equal(_bits(out), _bits(fwd))
    # evaluation without the backward pass gives the same loss
    assert engine.mlp_loss_grad(xd, models(name).spec, it, itau, want_grad=False, **T.LOSS_OPTS)["loss"] == got["loss"]


def test_two_pairs_one_output_has_a_constant_score(engine, models, gold):
    """Case "one" with m = 2: the score is 1 / (1 + alpha + eps)^2 whatever the parameters are, so the gradient is an
    exact zero reached through cancelling terms of the size of the score (parameters and activations are O(1)):
    1e-10 of the score bounds it as it bounds every other fp64 quantity here."""
    it, itau = T.pairs("one", "d")
    law = _law("one", "d")
    got = engine.mlp_loss_grad(engine.to_device(T.train_frames("one")), models("one").spec, it, itau, **T.LOSS_OPTS)
    rec = gold[1]["grad"]["one__d"]
    assert rec["constant_score"]
    assert abs(got["score"] - law["score"]) <= 1e-10 * law["score"]
    g = got["grad"].to_host()
    print(f"one/d: largest gradient entry {np.max(np.abs(g)):.3e}, score {got['score']!r}")
    assert np.max(np.abs(g)) <= 1e-10 * got["score"]


# ---- 3. dropout ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "leaky", "flagship"])
def test_loss_grad_with_dropout(engine, models, gold, name):
    drop = T.dropout_of(name, 0.1)
    assert drop[0] == 0.1 and max(drop[1:]) > 0.0
    X, (it, itau) = T.train_frames(name), T.pairs(name, "a")
    xd = engine.to_device(X)
    seed, step = 0x1234567887654321, 7
    law = _law(name, "a", dropout=drop, seed=seed, step=step)
    got = engine.mlp_loss_grad(xd, models(name).spec, it, itau, dropout=drop, seed=seed, step=step, want_outputs=True,
                               **T.LOSS_OPTS)
    assert abs(got["loss"] - law["loss"]) <= 1e-10 * abs(law["loss"])
    assert _rel(got["outputs"].to_host(), law["outputs"]) <= 1e-10
    assert np.max(np.abs(law["outputs"] - _law(name, "a")["outputs"])) > 1e-3       # the masks did act
    g = got["grad"].to_host()
    _check_grad(name, "a", g, law, gold, against_reference=False)
    for other in ({"seed": seed, "step": step + 1}, {"seed": seed + 1, "step": step}):
        g2 = engine.mlp_loss_grad(xd, models(name).spec, it, itau, dropout=drop, **other, **T.LOSS_OPTS)["grad"].to_host()
        assert np.max(np.abs(g2 - g)) > 1e-3 * np.max(np.abs(g))


def test_refusals(engine, models):
    spec, xd = models("odd").spec, engine.to_device(T.train_frames("odd"))
    it, itau = T.pairs("odd", "a")
    with pytest.raises(ValueError, match="1.0"):
        engine.mlp_loss_grad(xd, spec, it, itau, dropout=[0.1, 0.0, 1.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        engine.mlp_loss_grad(xd, spec, it, itau, dropout=[0.1, 0.0])                 # one probability per site
    with pytest.raises(ValueError, match="1 frame pairs"):
        engine.mlp_loss_grad(xd, spec, it[:1], itau[:1])
    with pytest.raises(IndexError):
        engine.mlp_loss_grad(xd, spec, it, itau + 100)
    with pytest.raises(NotImplementedError, match="65"):
        engine.vamp2_loss(engine.zeros((4, 65), np.float64), engine.zeros((4, 65), np.float64))
    assert np.isfinite(engine.mlp_loss_grad(xd, spec, it, itau)["loss"])             # usable afterwards


# ---- 4. clip + AdamW -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64 * 1024 + 5])
@pytest.mark.parametrize("clip_kind,wd", [("above", 0.0), ("below", 1e-4), (None, 1e-4)])
def test_adamw_step(engine, n, clip_kind, wd):
    rng = np.random.default_rng(n)
    p = rng.normal(size=n).astype(np.float32)
    pd, md, vd = engine.to_device(p), engine.zeros((n,), np.float64), engine.zeros((n,), np.float64)
    lr = 3e-3
    for step in (1, 2, 3):
        g = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-8, 3, size=n)
        norm = float(np.sqrt(np.sum(g * g)))
        clip = {"above": 10.0 * norm, "below": 0.1 * norm, None: None}[clip_kind]
        p0, m0, v0 = pd.to_host(), md.to_host(), vd.to_host()
        got = engine.adamw_step(pd, engine.to_device(g), md, vd, step, lr=lr, weight_decay=wd, clip=clip)
        p1, m1, v1, norm_ref, norm_clipped, skipped = T.adamw(p0, g, m0, v0, step, lr, wd=wd, clip=clip)
        assert not got["skipped"] and not skipped
        assert abs(got["grad_norm_preclip"] - norm_ref) <= 1e-13 * norm_ref
        assert abs(got["grad_norm"] - norm_clipped) <= 1e-13 * norm_clipped
        if clip_kind == "below":
            assert got["grad_norm"] < 0.11 * got["grad_norm_preclip"]
        else:
            assert got["grad_norm"] == got["grad_norm_preclip"]
        # entry by entry, 1e-13 of the two terms the new moment is the sum of (for v, whose terms are positive, that
        # is 1e-13 of v itself; for m the terms may cancel, and the clip coefficient carries the last-bit
        # difference of two summation orders of the norm)
        coef = norm_clipped / norm_ref
        assert np.all(np.abs(md.to_host() - m1) <= 1e-13 * (0.9 * np.abs(m0) + 0.1 * np.abs(g) * coef))
        assert np.all(np.abs(vd.to_host() - v1) <= 1e-13 * np.abs(v1))
        assert np.all(np.abs(pd.to_host().astype(np.float64) - p1.astype(np.float64)) <= T.ulp32(p1))
        assert np.any(pd.to_host() != p0)
    # a non-finite gradient: nothing moves, the flag is up
    p0, m0, v0 = pd.to_host(), md.to_host(), vd.to_host()
    for poison in (np.nan, np.inf):
        g = rng.normal(size=n)
        g[n // 2] = poison
        got = engine.adamw_step(pd, engine.to_device(g), md, vd, 4, lr=lr, weight_decay=wd, clip=1.0)
        assert got["skipped"] and not np.isfinite(got["grad_norm_preclip"])
        assert np.array_equal(pd.to_host().view(np.uint32), p0.view(np.uint32))
        assert np.array_equal(_bits(md.to_host()), _bits(m0)) and np.array_equal(_bits(vd.to_host()), _bits(v0))


# ---- 5. reproducibility --------------------------------------------------------------------------------------------
def test_equal_calls_give_equal_bits(engine, models):
    X, (it, itau) = T.train_frames("wide"), T.pairs("wide", "a")
    xd = engine.to_device(X)
    runs = [engine.mlp_loss_grad(xd, models("wide").spec, it, itau, dropout=[0.1, 0.2, 0.2], seed=5, step=2,
                                 want_outputs=True, **T.LOSS_OPTS) for _ in range(2)]
    assert runs[0]["loss"] == runs[1]["loss"]
    for key in ("grad", "outputs"):
        assert np.array_equal(_bits(runs[0][key].to_host()), _bits(runs[1][key].to_host()))
    assert np.max(np.abs(runs[0]["grad"].to_host())) > 0.0


# ---- 6. the trainer ------------------------------------------------------------------------------------------------
def test_train_steps_follow_the_law(engine):
    name = "flagship"
    model = _model(name)
    model.config["dropout"] = 0.1                      # input dropout; the case brings its hidden dropout
    cfg = CurriculumConfig(seed=3, learning_rate=1e-3, weight_decay=1e-4, grad_clip_norm=1.0)
    trainer = DeepTICACurriculumTrainer(model, cfg, engine=engine)
    assert trainer.dropout == T.dropout_of(name, 0.1)
    X = T.train_frames(name)
    trainer.set_frames(X)
    opts = {"eps": cfg.vamp_eps, "eps_abs": cfg.vamp_eps_abs, "alpha": cfg.vamp_alpha, "cond_reg": cfg.vamp_cond_reg}
    for which in ("a", "b", "a", "b"):
        it, itau = T.pairs(name, which)
        p0, m0, v0 = trainer.state()
        step = trainer.step
        out = trainer.train_step(it, itau)
        law = T.loss_grad(name, X, it, itau, packed=p0, dropout=trainer.dropout, seed=3, step=step, opts=opts)
        p1, m1, v1, norm, norm_clipped, _ = T.adamw(p0, law["grad"], m0, v0, step + 1, 1e-3, wd=1e-4, clip=1.0)
        p, m, v = trainer.state()
        assert trainer.step == step + 1 and out["batch_size"] == len(it)
        assert abs(out["loss"] - law["loss"]) <= 1e-10 * abs(law["loss"])
        assert abs(out["grad_norm_preclip"] - norm) <= 1e-10 * norm
        assert abs(out["grad_norm"] - norm_clipped) <= 1e-10 * norm_clipped
        print(f"step {step + 1}: m {_rel(m, m1):.2e}, v {_rel(v, v1):.2e} of the largest entry; "
              f"p off by at most {np.max(np.abs(p.astype(np.float64) - p1) / T.ulp32(p1)):.2f} ulp")
        assert _rel(m, m1) <= 1e-12 and _rel(v, v1) <= 1e-12
        assert np.all(np.abs(p.astype(np.float64) - p1.astype(np.float64)) <= T.ulp32(p1))
        assert np.any(p != p0)


def test_a_poisoned_step_raises_and_changes_nothing(engine):
    """A NaN frame fails the loss's Cholesky ladder as in the reference (RuntimeError); a gradient that is not
    finite under a finite loss is the skipped update (FloatingPointError).  Neither moves p, m, v or the step."""

    class Poisoned(DeepTICACurriculumTrainer):
        def _call(self, idx_t, idx_tau, train):
            res = super()._call(idx_t, idx_tau, train)
            if train:
                g = res["grad"].to_host()
                g[3] = np.inf
                res["grad"].copy_from_host(g)
            return res

    X = np.array(T.train_frames("default"))
    for cls, frames, error in ((Poisoned, X, FloatingPointError), (DeepTICACurriculumTrainer, None, RuntimeError)):
        trainer = cls(_model("default"), CurriculumConfig(seed=0), engine=engine)
        if frames is None:
            frames = X.copy()
            frames[4, 2] = np.nan
        trainer.set_frames(frames)
        p0, m0, v0 = trainer.state()
        with pytest.raises(error):
            trainer.train_step(*T.pairs("default", "a"))
        p, m, v = trainer.state()
        assert trainer.step == 0 and np.array_equal(p.view(np.uint32), p0.view(np.uint32))
        assert np.array_equal(_bits(m), _bits(m0)) and np.array_equal(_bits(v), _bits(v0))


@pytest.mark.parametrize("seed", T.TOY_SEEDS)
def test_fit_on_the_toy_set(engine, gold, seed):
    """fit from the initial weights of the reference's run with this seed (recorded in the golden: the untrained
    score of this toy set ranges from 0.06 to 0.71 with the draw, so a gain can only be compared from a common
    start); batch order and everything after it are this trainer's."""
    arrays, doc = gold
    run = doc["toy"]["runs"][seed]
    assert run["seed"] == seed
    init = {k.split("__", 2)[2]: v for k, v in arrays.items() if k.startswith(f"toy_init__{seed}__")}
    seq = T.toy_sequence()
    cfg = CurriculumConfig(seed=seed, **T.TOY_TRAINER)
    # the untrained validation score, through the public pieces: the reference's own, up to its fp32 evaluation
    # (6e-8 amplified by a condition number of at most 1e3)
    split = split_train_val([seq.shape[0]], 5, cfg.val_fraction)[0]
    assert split == run["split"]
    blank = DeepTICACurriculumTrainer(DeepTICAModel.from_arrays(T.TOY_CONFIG, init, np.zeros(7), np.ones(7)), cfg,
                                      engine=engine)
    blank.set_frames(seq)
    untrained = blank.evaluate(*lagged_pairs([seq.shape[0] - split], 5, [split])[:2])["score"]
    print(f"seed {seed}: untrained {untrained!r}, the reference's {run['untrained']!r}")
    assert abs(untrained - run["untrained"]) <= 1e-4

    model = DeepTICAModel.from_arrays(T.TOY_CONFIG, init, np.zeros(7), np.ones(7))
    before = model.spec.params.copy()
    trainer = DeepTICACurriculumTrainer(model, cfg, engine=engine)
    history = trainer.fit([seq])
    assert list(history) == doc["history_keys"] and len(history) == 32
    for key in ("loss_curve", "objective_curve", "val_loss_curve", "val_score_curve", "learning_rate_curve",
                "grad_norm_mean_curve", "grad_norm_max_curve", "epochs", "cond_c00_curve", "var_z0_curve"):
        assert len(history[key]) == 6 == doc["toy"]["curve_length"], key
    assert history["learning_rate_curve"] == lr_schedule(1e-2, 1, 6)
    assert np.allclose(history["learning_rate_curve"], doc["toy"]["learning_rate_curve"], rtol=1e-15, atol=0.0)
    assert {str(k): v for k, v in history["pair_diagnostics"].items()} == doc["toy"]["pair_diagnostics"]
    assert model.training_history["best_val_score"] == history["best_val_score"]
    assert np.any(model.spec.params != before)
    # the returned model is the best one: evaluating it again gives the recorded score, to the bit
    assert trainer.evaluate(*trainer.val_pairs)["score"] == history["best_val_score"] == max(history["val_score_curve"])
    assert model.transform(seq[:64]).shape == (64, 2)
    # it learnt: at least half the gain the reference's trainer reached from the same start
    gain = run["best"] - run["untrained"]
    print(f"seed {seed}: best {history['best_val_score']:.4f}; the reference's best {run['best']:.4f}, gain {gain:.4f}")
    assert gain > 0.3
    assert history["best_val_score"] - untrained >= 0.5 * gain
