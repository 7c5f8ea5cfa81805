"""DeepTICA inference, the parts that need no device: the fp64 restatement against the reference's recorded outputs,
reading the reference's bundle, and the envelope errors (CPU suite)."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

from tests import _deeptica_ref as R

from pmarlo_amd.features.deeptica import DeepTICAModel, MLPSpec


@pytest.fixture(scope="module")
def gold(golden):
    return golden("deeptica.npz"), json.loads((Path(__file__).parent / "golden" / "deeptica.json").read_text())


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_the_reference(gold, name):
    """Pins tests/_deeptica_ref.py to the reference on machines without it: its distance from the recorded outputs
    is the recorded ref_dev (the reference's fp32 rounding), up to the last digits of the library calls."""
    arrays, doc = gold
    c = R.case(name)
    assert [k for k, _ in R.key_layout(c["config"], c["X"].shape[1])] == doc[name]["keys"]
    for which in ("raw", "final"):
        ref, dev = arrays[f"{which}__{name}"], doc[name]["ref_dev"][which]
        assert ref.shape == c[which].shape
        assert 0.0 < dev <= 1e-4 * doc[name]["scale"][which]
        assert np.max(np.abs(ref - c[which])) <= 1.01 * dev


def _write_bundle(path, c, params=None):
    import torch

    params = c["params"] if params is None else params
    path.with_suffix(".json").write_text(json.dumps({**c["config"], "learning_rate": 1e-3, "not_a_field": 1}))
    torch.save({"state_dict": {k: torch.from_numpy(np.array(v)) for k, v in params.items()}}, path.with_suffix(".pt"))
    torch.save({"mean": np.asarray(c["mean"]), "std": np.asarray(c["std"])}, path.with_suffix(".scaler.pt"))
    if c["history"]:
        path.with_suffix(".history.json").write_text(json.dumps(c["history"]))
    return path


def _from_arrays(c, params=None, config=None):
    return DeepTICAModel.from_arrays(c["config"] if config is None else config, c["params"] if params is None else params,
                                     c["mean"], c["std"], c["history"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_load_gives_the_spec_of_from_arrays(tmp_path, name):
    c = R.case(name)
    loaded = DeepTICAModel.load(_write_bundle(tmp_path / "model", c))
    built = _from_arrays(c)
    assert loaded.spec == built.spec
    assert loaded.training_history == (c["history"] or {})
    F, hidden, n_out = R.CASES[name][:3]
    assert built.spec.widths == (F, *R.hidden_of(c["config"]), n_out)
    assert built.spec.params.dtype == np.float32 and built.spec.params.size == built.spec.n_params()
    assert built.spec.head_activation == (not c["config"]["linear_head"])


def test_packing_order():
    """[ln gamma, beta], then per Linear W, b, [gamma, beta]: the order msm_mlp_forward documents."""
    c = R.case("odd")                   # hidden LayerNorms, dropout indices that skip
    keys = [k for k, _ in R.key_layout(c["config"], 33)]
    want = np.concatenate([c["params"][k].reshape(-1) for k in keys])
    assert np.array_equal(_from_arrays(c).spec.params, want)
    c = R.case("flagship")              # and the input LayerNorm in front
    keys = [k for k, _ in R.key_layout(c["config"], 64)]
    assert keys[:2] == ["ln.weight", "ln.bias"]
    assert np.array_equal(_from_arrays(c).spec.params, np.concatenate([c["params"][k].reshape(-1) for k in keys]))


@pytest.mark.parametrize("name,key", [("flagship", "inner.nn.4.bias"), ("flagship", "ln.weight"),
                                      ("flagship", "inner.nn.1.weight"), ("one", "inner.nn.2.weight")])
def test_missing_parameter_raises(tmp_path, name, key):
    c = R.case(name)
    assert key in c["params"]
    params = {k: v for k, v in c["params"].items() if k != key}
    with pytest.raises(ValueError):
        _from_arrays(c, params=params)
    with pytest.raises(ValueError):
        DeepTICAModel.load(_write_bundle(tmp_path / "model", c, params))


def test_inner_prefixed_bundle_loads(tmp_path):
    """A network saved inside one more wrapper: every key carries one more `inner.`, next to keys of the wrapper."""
    c = R.case("flagship")
    params = {"inner." + k: v for k, v in c["params"].items()}
    params["mean"] = np.zeros(3, np.float32)
    params["transform"] = np.eye(3, dtype=np.float32)
    assert DeepTICAModel.load(_write_bundle(tmp_path / "model", c, params)).spec == _from_arrays(c).spec


@pytest.mark.parametrize("change", [{"hidden": [128, 32]}, {"n_out": 4}, {"hidden": [128]}, {"layer_norm_hidden": False},
                                    {"linear_head": True}])
def test_width_mismatch_with_the_config_raises(change):
    c = R.case("flagship")
    with pytest.raises(ValueError):
        _from_arrays(c, config={**c["config"], **change})


def test_scaler_width_mismatch_raises():
    c = R.case("default")
    with pytest.raises(ValueError):
        DeepTICAModel.from_arrays(c["config"], c["params"], c["mean"][:-1], c["std"][:-1])


def _zeros(config, F):
    return {k: np.zeros(shape, np.float32) for k, shape in R.key_layout(config, F)}


@pytest.mark.parametrize("config,F,number", [
    ({"n_out": 3, "hidden": [257]}, 4, "257"),
    ({"n_out": 3, "hidden": [8]}, 257, "257"),
    ({"n_out": 2, "hidden": [4] * 8}, 4, "9"),
    ({"n_out": 65, "hidden": [8]}, 4, "65"),
])
def test_envelope_errors_need_no_device(config, F, number):
    with pytest.raises(NotImplementedError, match=number):
        DeepTICAModel.from_arrays(config, _zeros(config, F), np.zeros(F), np.ones(F))


def test_envelope_limits_themselves_are_accepted():
    config = {"n_out": 64, "hidden": [256] + [4] * 6}
    m = DeepTICAModel.from_arrays(config, _zeros(config, 256), np.zeros(256), np.ones(256))
    assert len(m.spec.widths) == 9 and isinstance(m.spec, MLPSpec)


def test_load_creates_no_engine(tmp_path, monkeypatch):
    import pmarlo_amd.device as device

    def boom(*a, **k):
        raise AssertionError("load must not touch the device")

    monkeypatch.setattr(device, "get_engine", boom)
    monkeypatch.setattr(device, "Engine", boom)
    DeepTICAModel.load(_write_bundle(tmp_path / "model", R.case("one")))
