"""train_deeptica and train_cv_model on the device, against what one run of the reference's train_deeptica on the toy
sequence recorded (tests/golden/deeptica_weighted.*): the history's keys, the scaler, the pair diagnostics and the
untrained score, from the reference's own initial weights."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

from tests import _deeptica_train_ref as T

from pmarlo_amd.cv import train_cv_model
from pmarlo_amd.features.deeptica import DeepTICAConfig, DeepTICAModel, prepare_features, train_deeptica

pytestmark = pytest.mark.gpu

# the reference's history keys this engine does not write: none.  (It writes no summary, checkpoint or metrics
# files either, but the reference's run without a checkpoint directory records no key for them.)
KEYS_NOT_WRITTEN: tuple[str, ...] = ()


@pytest.fixture(scope="module")
def gold(golden):
    return dict(golden("deeptica_weighted.npz")), json.loads(
        (Path(__file__).parent / "golden" / "deeptica_weighted.json").read_text())["pipeline"]


def _config(doc, **over):
    fields = {k: (tuple(v) if isinstance(v, list) else v) for k, v in {**T.TOY_CONFIG, **doc["config"]}.items()}
    return DeepTICAConfig(**{**fields, **over})


def test_prepare_features(engine, gold):
    arrays, _ = gold
    seq = T.toy_sequence()
    halves = [seq[:700], seq[700:]]
    prep = prepare_features(halves, tau_schedule=(5, 0, 2), seed=4, engine=engine)
    assert prep.X.dtype == np.float32 and np.array_equal(prep.X, seq) and prep.x_device.shape == (2000, 7)
    assert (prep.tau_schedule, prep.input_dim, prep.seed) == ((5, 2), 7, 4) and not hasattr(prep, "Z")
    assert np.max(np.abs(prep.mean - arrays["toy_scaler_mean"])) <= 1e-12 * np.max(np.abs(arrays["toy_scaler_mean"]))
    assert np.max(np.abs(prep.scale / arrays["toy_scaler_scale"] - 1.0)) <= 1e-12
    # a constant column gets scale 1, as sklearn's scaler gives it
    flat = seq.copy()
    flat[:, 2] = 3.25
    prep = prepare_features([flat], tau_schedule=(2,), seed=0, engine=engine)
    assert prep.scale[2] == 1.0 and prep.mean[2] == 3.25 and np.all(prep.scale[[0, 1, 3]] != 1.0)
    with pytest.raises(ValueError, match="NaN"):
        bad = seq.copy()
        bad[5, 1] = np.nan
        prepare_features([bad], tau_schedule=(2,), seed=0, engine=engine)


def test_train_deeptica_on_the_toy_sequence(engine, gold):
    arrays, doc = gold
    seq = T.toy_sequence()
    init = {k.split("__", 1)[1]: v for k, v in arrays.items() if k.startswith("toy_init__")}
    cfg = _config(doc)
    pair_weights = np.linspace(0.5, 2.5, doc["pair_diagnostics_overall"]["usable_pairs"])
    model = train_deeptica([seq], None, cfg, weights=pair_weights, initial_state=init, engine=engine)
    assert isinstance(model, DeepTICAModel)
    hist = model.training_history
    assert list(hist) == [k for k in doc["history_keys"] if k not in KEYS_NOT_WRITTEN]
    assert hist["history_source"] == doc["history_source"] == "curriculum_trainer"
    assert np.max(np.abs(model.spec.mean - arrays["toy_scaler_mean"])) <= 1e-12 * np.max(np.abs(arrays["toy_scaler_mean"]))
    assert np.max(np.abs(model.spec.scale / arrays["toy_scaler_scale"] - 1.0)) <= 1e-12
    assert hist["pair_diagnostics_overall"] == doc["pair_diagnostics_overall"]
    assert hist["pair_diagnostics"]["overall"] == doc["pair_diagnostics_overall"]
    assert hist["usable_pairs"] == doc["usable_pairs"] and hist["pair_coverage"] == doc["pair_coverage"]
    print(f"vamp2_before {hist['vamp2_before']!r}, the reference's {doc['vamp2_before']!r}; "
          f"vamp2_after {hist['vamp2_after']!r}, the reference's {doc['vamp2_after']!r}")
    assert abs(hist["vamp2_before"] - doc["vamp2_before"]) <= 1e-6             # the reference forwards in fp32
    assert hist["vamp2_after"] > hist["vamp2_before"]
    # the pair weights are echoed (as the float32 values the reference keeps) and nothing else
    assert hist["weights_count"] == pair_weights.size
    assert hist["weights_mean"] == float(np.mean(pair_weights.astype(np.float32)))
    assert "weighted_loss" not in hist
    assert len(hist["loss_curve"]) == 6 and len(hist["output_variance"]) == 2 and len(hist["top_eigenvalues"]) == 2
    assert 1.0 >= hist["top_eigenvalues"][0] >= hist["top_eigenvalues"][1] > 0.0
    w = hist["whitening"]
    assert hist["output_mean"] == w["mean"] and hist["output_transform"] == w["transform"]
    assert hist["output_transform_applied"] is False and w["transform_applied"] is False
    assert np.allclose(hist["output_variance"], w["output_variance"], rtol=1e-12)
    assert model.config["hidden"] == (16, 8) and model.config["trainer_backend"] == "curriculum"
    # the model transforms, and whitens as the history says (computed, not applied: transform applies it)
    Y = model.transform(seq)
    raw = engine.mlp_forward(engine.to_device(seq), model.spec).to_host()
    assert Y.shape == (2000, 2) and np.all(np.isfinite(Y))
    assert np.allclose(raw.var(axis=0, ddof=1), hist["output_variance"], rtol=1e-12)
    assert np.max(np.abs(Y - raw)) > 1e-3
    json.dumps(hist)                                                           # the history is what save() writes


def test_train_deeptica_with_frame_weights(engine, gold):
    _, doc = gold
    seq = T.toy_sequence()[:800]
    fw = np.exp(0.5 * np.random.default_rng(8).normal(size=800))
    cfg = _config(doc, epochs_per_tau=1, trainer_backend="mlcolvar", seed=2)
    model = train_deeptica([seq[:500], seq[500:]], None, cfg, frame_weights=[fw[:500], fw[500:]], engine=engine)
    hist = model.training_history
    assert list(hist)[32:34] == ["weighted_loss", "effective_pairs_curve"]     # fit's, ahead of the finalising keys
    assert hist["weighted_loss"] is True and len(hist["effective_pairs_curve"]) == 2
    assert hist["history_source"] == "curriculum_trainer" and hist["weights_mean"] == 1.0
    assert hist["pairs_by_trajectory"] == [498 + 495, 298 + 295]
    plain = train_deeptica([seq[:500], seq[500:]], None, cfg, engine=engine).training_history
    assert plain["loss_curve"] != hist["loss_curve"] and plain["vamp2_before"] == hist["vamp2_before"]


def test_train_cv_model(engine):
    seq = T.toy_sequence()[:600]
    tica = train_cv_model(seq, lag_time=5, n_components=2, method="tica")
    Y = tica.transform(seq)
    assert Y.shape == (600, 2) and np.all(np.isfinite(Y))
    from pmarlo_amd.markov_state_model.reduction import tica_reduce

    assert np.array_equal(Y, tica_reduce(seq, lag=5, n_components=2))
    deep = train_cv_model(seq, lag_time=3, n_components=2, method="deeptica", hidden=(8,), epochs_per_tau=1,
                          batch_size=128, activation="tanh")
    assert isinstance(deep, DeepTICAModel) and deep.transform(seq).shape == (600, 2)
    assert deep.training_history["lag_used"] == 3
    with pytest.raises(ValueError, match="Unknown CV method"):
        train_cv_model(seq, method="vampnet")
