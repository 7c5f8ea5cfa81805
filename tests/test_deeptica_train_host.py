"""DeepTICA training, the parts that need no device: the fp64 restatement (tests/_deeptica_train_ref.py) against
torch's fp64 autograd and against the reference's recorded values, and the Python layer of the trainer (schedule,
time split, pair sets, configuration, envelope, save / load, initialisation)."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

from tests import _deeptica_ref as R
from tests import _deeptica_train_ref as T

from pmarlo_amd.features.deeptica import CurriculumConfig, DeepTICAModel, MLPSpec
from pmarlo_amd.features.deeptica.model import dropout_sites, state_dict_layout
from pmarlo_amd.features.deeptica.trainer import lagged_pairs, lr_schedule, split_train_val


@pytest.fixture(scope="module")
def gold(golden):
    arrays = dict(golden("deeptica_train.npz"))
    for w in "abc":
        arrays.update(golden(f"deeptica_train_wide_{w}.npz"))
    return arrays, json.loads((Path(__file__).parent / "golden" / "deeptica_train.json").read_text())


# ---- the restatement against torch's autograd ------------------------------------------------------------------------
def _torch_loss(torch, z0, zt, eps, eps_abs, alpha, cond_reg):
    """The law of msm_vamp2_loss written with differentiable torch operators (fp64)."""
    m, d = z0.shape
    a0, at = z0 - z0.mean(0, keepdim=True), zt - zt.mean(0, keepdim=True)
    C00, Ctt, C0t = a0.T @ a0 / m, at.T @ at / m, a0.T @ at / m
    eye = torch.eye(d, dtype=torch.float64)

    def side(C):
        mu = torch.clamp(torch.trace(C), min=1e-12) / d
        A = (1.0 - alpha) * C + (alpha * mu + torch.maximum(mu * eps, mu * eps_abs)) * eye
        A = 0.5 * (A + A.T)
        w = torch.linalg.eigvalsh(A)
        return A, torch.clamp(w.max(), min=1e-12) / torch.clamp(w.min(), min=1e-12)

    A, cond0 = side(C00)
    B, condt = side(Ctt)
    left = torch.linalg.solve_triangular(torch.linalg.cholesky(A), C0t, upper=False)
    K = torch.linalg.solve_triangular(torch.linalg.cholesky(B), left.T, upper=False).T
    return -(K * K).sum() + cond_reg * (torch.log(torch.clamp(cond0, min=1.0)) + torch.log(torch.clamp(condt, min=1.0)))


def _torch_forward(torch, name, X, rows, params, masks):
    """The network in training mode with the given dropout factors, differentiable in `params` (fp64 tensors)."""
    c = R.case(name)
    config = c["config"]
    F = torch.nn.functional
    act = {"gelu": F.gelu, "gaussian": F.gelu, "relu": F.relu, "elu": F.elu, "selu": F.selu,
           "leaky_relu": F.leaky_relu}.get(config["activation"], torch.tanh)
    Z = (np.asarray(X, np.float64)[rows] - c["mean"]) / c["std"]
    x = torch.tensor(Z.astype(np.float32).astype(np.float64))
    if config.get("layer_norm_in"):
        x = F.layer_norm(x, (x.shape[1],), params["ln.weight"], params["ln.bias"], 1e-5)
    if masks is not None:
        x = x * torch.tensor(masks[0])
    layers = T.layers_of(config, x.shape[1])
    for i, (kw, kb, kg, kbeta) in enumerate(layers):
        x = x @ params[kw].T + params[kb]
        last = i == len(layers) - 1
        if kg is not None:
            x = F.layer_norm(x, (x.shape[1],), params[kg], params[kbeta], 1e-5)
        if not last or not config.get("linear_head"):
            x = act(x)
        if not last and masks is not None:
            x = x * torch.tensor(masks[i + 1])
    return x


@pytest.mark.parametrize("name", list(R.CASES))
def test_restated_gradients_match_autograd(name, gold):
    import torch

    drop = T.dropout_of(name, 0.1) if name in ("odd", "leaky", "flagship") else None
    X, (it, itau) = T.train_frames(name), T.pairs(name, "b" if name == "elu" else "a")
    which = "b" if name == "elu" else "a"
    seed, step = 11, 3
    mine = T.loss_grad(name, X, it, itau, dropout=drop, seed=seed, step=step)
    c = R.case(name)
    params = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in c["params"].items()}
    widths = [c["X"].shape[1]] + [c["params"][kw].shape[0] for kw, *_ in T.layers_of(c["config"], c["X"].shape[1])]
    masks = None
    if drop is not None:
        masks = [T.dropout_factor(seed, step, s, 2 * len(it), widths[s], drop[s]) for s in range(len(drop))]
        assert any((mk == 0).any() for mk in masks) and all((mk != 0).any() for mk in masks)
    Y = _torch_forward(torch, name, X, np.concatenate([it, itau]), params, masks)
    loss = _torch_loss(torch, Y[:len(it)], Y[len(it):], **{k: torch.tensor(v, dtype=torch.float64)
                                                            for k, v in T.LOSS_OPTS.items()})
    loss.backward()
    assert abs(float(loss.detach()) - mine["loss"]) <= 1e-12 * abs(mine["loss"])
    assert np.max(np.abs(Y.detach().numpy() - mine["outputs"])) <= 1e-12 * np.max(np.abs(mine["outputs"]))
    top = max(float(np.max(np.abs(g))) for g in mine["grads"].values())
    blind = gold[1]["grad"][f"{name}__{which}"]["zero_tensors"]
    for key, p in params.items():
        g = p.grad.numpy()
        # a tensor the loss cannot see has an exact zero gradient: its largest entry is noise, the case's stands in
        scale = top if key in blind else float(np.max(np.abs(g)))
        err = float(np.max(np.abs(g - mine["grads"][key])))
        print(f"{name} {key}: {err / scale:.2e} of the largest entry")
        assert err <= 1e-10 * scale


@pytest.mark.parametrize("i", range(len(T.LOSS_SHAPES)))
def test_restated_loss_matches_the_reference(gold, i):
    arrays, doc = gold
    Y0, Yt, opts = T.loss_case(i)
    mine, ref = T.vamp2(Y0, Yt, **opts), doc["loss"][i]
    assert abs(mine["loss"] - ref["loss"]) <= 1e-10 * abs(ref["loss"])
    assert abs(mine["score"] - ref["score"]) <= 1e-10 * abs(ref["score"])
    assert list(mine["metrics"]) == list(ref["metrics"])
    for key, value in ref["metrics"].items():
        assert np.max(np.abs(np.asarray(mine["metrics"][key]) - np.asarray(value))) <= 1e-10 * np.max(np.abs(value))
    for g, rec in ((mine["grad0"], arrays[f"loss_g0__{i}"]), (mine["grad_t"], arrays[f"loss_gt__{i}"])):
        top = float(np.max(np.abs(rec)))
        scale = top if top > 1e-6 * mine["term_scale"] else mine["term_scale"]
        assert np.max(np.abs(g - rec)) <= 1e-10 * scale


@pytest.mark.parametrize("name", list(R.CASES))
def test_restated_parameter_gradients_match_the_reference(gold, name):
    arrays, doc = gold
    for which in ["a", "b"] + (["c"] if name == "wide" else []) + (["d"] if name == "one" else []):
        rec = doc["grad"][f"{name}__{which}"]
        mine = T.loss_grad(name, T.train_frames(name), *T.pairs(name, which))
        assert abs(mine["loss"] - rec["loss"]) <= 1e-5 * abs(rec["loss"])            # the reference's network is fp32
        for key, dev in rec["ref_dev_grad"].items():
            got = float(np.max(np.abs(mine["grads"][key] - arrays[f"grad__{name}__{which}__{key}"])))
            assert got <= dev * (1.0 + 1e-9) + 1e-300, (which, key, got, dev)
    packed = T.loss_grad(name, T.train_frames(name), *T.pairs(name, "a"))["grad"]
    assert packed.shape == T.packed_params(name).shape


def test_masks_are_philox_words_against_the_threshold():
    f = T.dropout_factor(9, 4, 2, 40, 33, 0.25)
    assert f.shape == (40, 33) and set(np.unique(f)) == {0.0, 1.0 / 0.75}
    assert 0.15 < np.mean(f == 0.0) < 0.35
    assert np.array_equal(f, T.dropout_factor(9, 4, 2, 40, 33, 0.25))
    for other in (T.dropout_factor(10, 4, 2, 40, 33, 0.25), T.dropout_factor(9, 5, 2, 40, 33, 0.25),
                  T.dropout_factor(9, 4, 3, 40, 33, 0.25)):
        assert not np.array_equal(f, other)
    assert np.array_equal(f[:16, :32], T.dropout_factor(9, 4, 2, 16, 32, 0.25))     # a function of (slot, column) alone
    assert np.all(T.dropout_factor(9, 4, 2, 5, 7, 0.0) == 1.0)
    with pytest.raises(ValueError):
        T.dropout_factor(9, 4, 2, 5, 7, 1.0)


def test_adamw_restatement_matches_torch():
    import torch

    rng = np.random.default_rng(0)
    p = rng.normal(size=50).astype(np.float32)
    tp = torch.nn.Parameter(torch.tensor(p.astype(np.float64)))
    opt = torch.optim.AdamW([tp], lr=3e-3, weight_decay=1e-4)
    p64, m, v = p.astype(np.float64), np.zeros(50), np.zeros(50)
    for step in (1, 2, 3):
        g = rng.normal(size=50) * 10.0 ** rng.uniform(-4, 2, size=50)
        tp.grad = torch.tensor(g)
        torch.nn.utils.clip_grad_norm_([tp], 1.0)
        opt.step()
        # the restatement rounds p to fp32 each step; follow torch's fp64 trajectory through its pre-rounding value
        coef = min(1.0, 1.0 / (np.sqrt(np.sum(g * g)) + 1e-6))
        m = 0.9 * m + 0.1 * g * coef
        v = 0.999 * v + 0.001 * (g * coef) ** 2
        p64 = p64 * (1 - 3e-3 * 1e-4) - (3e-3 / (1 - 0.9 ** step)) * (m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** step) + 1e-8))
        assert np.max(np.abs(tp.detach().numpy() - p64)) <= 1e-12
    one = T.adamw(p, g, np.zeros(50), np.zeros(50), 1, 3e-3, wd=1e-4, clip=1.0)
    assert one[0].dtype == np.float32 and not one[5] and one[4] <= 1.0
    bad = g.copy()
    bad[7] = np.inf
    skipped = T.adamw(p, bad, m, v, 2, 3e-3)
    assert skipped[5] and np.array_equal(skipped[0], p) and np.array_equal(skipped[1], m)


# ---- the Python layer ------------------------------------------------------------------------------------------------
def test_schedule_split_and_pairs_match_the_reference(gold):
    doc = gold[1]["toy"]
    assert lr_schedule(1e-2, 1, 6) == doc["learning_rate_curve"]
    assert lr_schedule(1e-3, 5, 3) == [1e-3 / 3, 2e-3 / 3, 1e-3]              # warmup longer than the run
    assert lr_schedule(1e-3, 0, 0) == []
    assert split_train_val([2000], 5, 0.2) == [doc["runs"][0]["split"]]
    # 6 frames are too few for max_tau 5; 7 and 8 keep max_tau + 1 frames on each side of the cut
    assert split_train_val([7, 6, 8, 40], 5, 0.2) == [6, None, 6, 32]
    for tau in (2, 5):
        it, itau, diag = lagged_pairs([doc["runs"][0]["split"]], tau)
        assert diag == doc["pair_diagnostics"][str(tau)]
        assert np.array_equal(itau - it, np.full(it.size, tau)) and it[0] == 0 and itau[-1] == 1599
    it, itau, diag = lagged_pairs([5, 2, 4], 3, [0, 5, 7])
    assert it.tolist() == [0, 1, 7] and itau.tolist() == [3, 4, 10]
    assert diag["pairs_per_sequence"] == [2, 0, 1] and diag["short_sequences"] == [1] and diag["usable_pairs"] == 3
    with pytest.raises(ValueError):
        lagged_pairs([5], 0)


def test_curriculum_config_mirrors_the_reference():
    cfg = CurriculumConfig()
    assert (cfg.tau_schedule, cfg.val_tau, cfg.epochs_per_tau, cfg.warmup_epochs, cfg.batch_size) == ((2,), 2, 15, 5, 256)
    assert (cfg.learning_rate, cfg.weight_decay, cfg.val_fraction, cfg.grad_clip_norm) == (3e-4, 1e-4, 0.2, 1.0)
    assert (cfg.vamp_eps, cfg.vamp_eps_abs, cfg.vamp_alpha, cfg.vamp_cond_reg) == (1e-3, 1e-6, 0.15, 1e-4)
    cfg = CurriculumConfig(tau_schedule=(5, 0, 2), val_tau=0, val_fraction=1.5, warmup_epochs=-3)
    assert cfg.tau_schedule == (2, 5) and cfg.val_tau == 5 and cfg.val_fraction == 0.9 and cfg.warmup_epochs == 0
    assert CurriculumConfig(tau_schedule=(), val_tau=7).tau_schedule == (7,)
    for bad in ({"epochs_per_tau": 0}, {"batch_size": 0}, {"learning_rate": 0.0}):
        with pytest.raises(ValueError):
            CurriculumConfig(**bad)
    for gone in ("device", "checkpoint_dir", "num_workers"):
        assert not hasattr(cfg, gone)


def test_envelope_and_dropout_errors():
    with pytest.raises(NotImplementedError, match="257"):
        MLPSpec((257, 3), 0, False, False, True, np.zeros(0, np.float32)).check_envelope()
    with pytest.raises(NotImplementedError, match="65"):
        MLPSpec((4, 65), 0, False, False, True, np.zeros(0, np.float32)).check_envelope()
    with pytest.raises(NotImplementedError, match="9"):
        MLPSpec((4,) * 10, 0, False, False, True, np.zeros(0, np.float32)).check_envelope()
    assert dropout_sites({"hidden": [8, 4], "hidden_dropout": [0.2]}, 3) == [0.0, 0.2, 0.2]
    assert dropout_sites({"dropout": 0.3, "dropout_input": 0.1, "hidden_dropout": 0.05, "hidden": [8]}, 2) == [0.1, 0.05]
    assert dropout_sites({"dropout": -1.0, "linear_head": True}, 1) == [0.0]
    for bad in ({"dropout": 1.0}, {"hidden_dropout": [0.1, 1.5], "hidden": [8, 4]}):
        with pytest.raises(ValueError, match="0 <= p < 1"):
            dropout_sites(bad, 3 if "hidden" in bad else 1)


@pytest.mark.parametrize("name", ["flagship", "odd", "default", "linear_head"])
def test_save_load_round_trip(tmp_path, name):
    c = R.case(name)
    model = DeepTICAModel.from_arrays(c["config"], c["params"], c["mean"], c["std"], c["history"])
    assert [k for k, _ in state_dict_layout(c["config"], c["X"].shape[1])] == [k for k, _ in R.key_layout(c["config"], c["X"].shape[1])]
    state = model.state_dict()
    assert list(state) == list(c["params"]) and all(np.array_equal(state[k], c["params"][k]) for k in state)
    model.training_history["per_tau_objective_curve"] = {2: [0.1, 0.2]}       # an integer key, as fit leaves it
    model.save(tmp_path / "bundle" / name)
    back = DeepTICAModel.load(tmp_path / "bundle" / name)
    assert back == model and back.spec == model.spec
    assert np.array_equal(back.spec.params, T.packed_params(name))
    other = DeepTICAModel.from_arrays(c["config"], c["params"], c["mean"] + 1.0, c["std"], c["history"])
    assert other != model


def test_initialize():
    config = {"n_out": 3, "hidden": [16, 8], "activation": "tanh", "layer_norm_in": True, "layer_norm_hidden": True,
              "hidden_dropout": [0.1]}
    a = DeepTICAModel.initialize(config, np.zeros(7), np.ones(7), seed=4)
    b = DeepTICAModel.initialize(config, np.zeros(7), np.ones(7), seed=4)
    assert a == b and a != DeepTICAModel.initialize(config, np.zeros(7), np.ones(7), seed=5)
    assert a.spec.widths == (7, 16, 8, 3) and a.spec.params.size == a.spec.n_params()
    for key, value in a.state_dict().items():
        if value.ndim == 2:
            bound = 1.0 / np.sqrt(value.shape[1])
            assert np.all(np.abs(value) <= bound) and np.max(np.abs(value)) > 0.8 * bound
            bias = a.state_dict()[key.replace("weight", "bias")]
            assert np.all(np.abs(bias) <= bound) and np.any(bias != 0.0)
        elif key.endswith("weight"):
            assert np.all(value == 1.0)                                                  # LayerNorm gamma
    assert np.all(a.state_dict()["ln.bias"] == 0.0) and np.all(a.state_dict()["inner.nn.1.bias"] == 0.0)
