"""The host pieces of train_deeptica: build_pair_info, DeepTICAConfig, the CurriculumConfig mapping, vamp2_proxy and
the whitening block's shrunk covariance.  CPU only; expected values are worked out here or recorded from the
reference's run (tests/golden/deeptica_weighted.json)."""

from __future__ import annotations

import dataclasses
import json
from pathlib import Path

import numpy as np
import pytest

from tests import _deeptica_train_ref as T

from pmarlo_amd.features.deeptica import (CurriculumConfig, DeepTICAConfig, PairInfo, build_pair_info, train_deeptica,
                                          vamp2_proxy)
from pmarlo_amd.features.deeptica.training import curriculum_config, output_whitening_info, shrunk_covariance


def _trajs(*lengths):
    return [np.zeros((n, 3), np.float32) for n in lengths]


# ---- build_pair_info -------------------------------------------------------------------------------------------------
def test_derived_pairs_single_lag():
    info = build_pair_info(_trajs(6, 2, 5), [3])
    assert isinstance(info, PairInfo)
    assert info.idx_t.tolist() == [0, 1, 2, 8, 9] and info.idx_tau.tolist() == [3, 4, 5, 11, 12]
    assert info.idx_t.dtype == np.int64 and info.weights.dtype == np.float32 and info.weights.tolist() == [1.0] * 5
    assert info.diagnostics == {"usable_pairs": 5, "pair_coverage": 1.0, "total_possible_pairs": 5,
                                "short_trajectories": [1], "pairs_by_trajectory": [3, 0, 2], "lag_used": 3,
                                "expected_pairs": 5, "tau_schedule_used": [3]}
    assert list(info.diagnostics) == ["usable_pairs", "pair_coverage", "total_possible_pairs", "short_trajectories",
                                      "pairs_by_trajectory", "lag_used", "expected_pairs", "tau_schedule_used"]


def test_derived_pairs_of_a_curriculum_are_concatenated_lag_after_lag():
    info = build_pair_info(_trajs(4, 3), [2, 0, 1])                       # the non-positive lag is dropped
    assert info.idx_t.tolist() == [0, 1, 4] + [0, 1, 2, 4, 5]
    assert info.idx_tau.tolist() == [2, 3, 6] + [1, 2, 3, 5, 6]
    d = info.diagnostics
    assert d["tau_schedule_used"] == [2, 1] and d["lag_used"] == 2 and d["total_possible_pairs"] == 8
    assert d["usable_pairs"] == 8 and d["pair_coverage"] == 1.0 and d["pairs_by_trajectory"] == [5, 3]
    assert d["short_trajectories"] == []


def test_the_toy_run_s_diagnostics_are_the_reference_s():
    doc = json.loads((Path(__file__).parent / "golden" / "deeptica_weighted.json").read_text())
    info = build_pair_info([T.toy_sequence()], doc["pipeline"]["config"]["tau_schedule"])
    assert info.diagnostics == doc["pipeline"]["pair_diagnostics_overall"]


def test_given_pairs_are_validated_with_the_reference_s_messages():
    trajs = _trajs(5, 5)
    info = build_pair_info(trajs, [2], pairs=(np.array([[0, 1], [5, 6]]), np.array([[2, 3], [7, 9]])))
    assert info.idx_t.tolist() == [0, 1, 5, 6] and info.idx_tau.tolist() == [2, 3, 7, 9]
    assert info.diagnostics["usable_pairs"] == 4 and info.diagnostics["pair_coverage"] == 4 / 6
    assert info.diagnostics["pairs_by_trajectory"] == [2, 2]
    bad = {"Pair index arrays must have the same shape": ([0, 1], [2]),
           "Pair indices must be non-negative": ([-1, 1], [2, 3]),
           "Pair indices exceed available trajectory length": ([0, 1], [2, 10]),
           "Pair indices must represent positive time lags": ([0, 3], [2, 3])}
    for message, (a, b) in bad.items():
        with pytest.raises(ValueError, match=message):
            build_pair_info(trajs, [2], pairs=(np.array(a), np.array(b)))
    with pytest.raises(ValueError, match="Pair indices provided but no trajectories are available"):
        build_pair_info([], [2], pairs=(np.array([0]), np.array([1])))
    with pytest.raises(ValueError, match="Tau schedule must contain at least one positive lag"):
        build_pair_info(trajs, [0, -1])
    empty = build_pair_info(trajs, [2], pairs=(np.zeros(0), np.zeros(0)))
    assert empty.idx_t.size == 0 and empty.diagnostics["pair_coverage"] == 0.0


def test_weight_broadcasting():
    trajs = _trajs(6)
    assert build_pair_info(trajs, [2], weights=np.array([2.5])).weights.tolist() == [2.5] * 4
    w = build_pair_info(trajs, [2], weights=[[1, 2], [3, 4]]).weights
    assert w.tolist() == [1.0, 2.0, 3.0, 4.0] and w.dtype == np.float32
    with pytest.raises(ValueError, match="weights must match the number of lagged pairs"):
        build_pair_info(trajs, [2], weights=np.ones(3))
    assert build_pair_info(_trajs(2), [2], weights=np.ones(3)).weights.size == 0     # no pairs: no weights, no error


# ---- DeepTICAConfig ----------------------------------------------------------------------------------------------------
def test_config_defaults_are_the_reference_s():
    cfg = DeepTICAConfig(lag=4)
    assert dataclasses.asdict(cfg) == {
        "lag": 4, "n_out": 2, "hidden": (32, 16), "activation": "gelu", "learning_rate": 3e-4, "batch_size": 1024,
        "max_epochs": 200, "early_stopping": 25, "weight_decay": 1e-4, "log_every": 1, "seed": 0, "device": "cpu",
        "trainer_backend": "lightning", "val_frac": 0.1, "num_workers": 2, "lr_schedule": "cosine", "warmup_epochs": 5,
        "dropout": 0.0, "dropout_input": None, "hidden_dropout": (), "layer_norm_in": False, "layer_norm_hidden": False,
        "linear_head": False, "batches_per_epoch": 200, "gradient_clip_val": 1.0, "gradient_clip_algorithm": "norm",
        "tau_schedule": (), "val_tau": None, "epochs_per_tau": 15, "vamp_eps": 1e-3, "vamp_eps_abs": 1e-6,
        "vamp_alpha": 0.15, "vamp_cond_reg": 1e-4, "grad_norm_warn": None, "variance_warn_threshold": 1e-6,
        "mean_warn_threshold": 5.0}
    with pytest.raises(dataclasses.FrozenInstanceError):
        cfg.lag = 5
    with pytest.raises(TypeError):
        DeepTICAConfig()                                                   # lag is required


def test_config_small_data_and_backends():
    cfg = DeepTICAConfig.small_data(lag=3)
    assert (cfg.lag, cfg.n_out, cfg.hidden, cfg.dropout_input, cfg.hidden_dropout) == (3, 2, (32,), 0.15, (0.15,))
    assert cfg.layer_norm_in and cfg.layer_norm_hidden
    cfg = DeepTICAConfig.small_data(lag=3, hidden=(8, 4), dropout_input=1.7, hidden_dropout=[0.3, -0.2], seed=9,
                                    layer_norm_in=False)
    assert cfg.hidden == (8, 4) and cfg.dropout_input == 1.0 and cfg.hidden_dropout == (0.3, 0.0)
    assert cfg.seed == 9 and not cfg.layer_norm_in and cfg.layer_norm_hidden
    assert DeepTICAConfig(lag=1, trainer_backend="  CurriCulum ").trainer_backend == "curriculum"
    for name in ("lightning", "curriculum", "mlcolvar", "deeptime"):
        assert DeepTICAConfig(lag=1, trainer_backend=name).trainer_backend == name
    with pytest.raises(ValueError, match="trainer_backend must be one of: curriculum, deeptime, lightning, mlcolvar"):
        DeepTICAConfig(lag=1, trainer_backend="keras")


# ---- the CurriculumConfig mapping --------------------------------------------------------------------------------------
def test_curriculum_config_mapping():
    cfg = DeepTICAConfig(lag=7)
    got = curriculum_config(cfg, (7,))
    assert got == CurriculumConfig(tau_schedule=(7,), val_tau=7, epochs_per_tau=15, warmup_epochs=5, batch_size=1024,
                                   learning_rate=3e-4, weight_decay=1e-4, val_fraction=0.1, shuffle=True,
                                   grad_clip_norm=1.0, log_every=1, vamp_eps=1e-3, vamp_eps_abs=1e-6, vamp_alpha=0.15,
                                   vamp_cond_reg=1e-4, seed=0, max_batches_per_epoch=200)
    cfg = DeepTICAConfig(lag=7, tau_schedule=(5, 2, 5), val_tau=3, val_frac=1.5, gradient_clip_val=0.0,
                         batches_per_epoch=0, epochs_per_tau=0, warmup_epochs=-2, batch_size=0, weight_decay=-1.0,
                         log_every=0, vamp_cond_reg=-1.0, seed=11, learning_rate=1e-2)
    got = curriculum_config(cfg, cfg.tau_schedule)
    assert got.tau_schedule == (2, 5) and got.val_tau == 3 and got.val_fraction == 0.1
    assert got.grad_clip_norm is None and got.max_batches_per_epoch is None
    assert (got.epochs_per_tau, got.warmup_epochs, got.batch_size, got.weight_decay, got.log_every) == (1, 0, 1, 0.0, 1)
    assert got.vamp_cond_reg == 0.0 and got.seed == 11 and got.learning_rate == 1e-2 and got.shuffle

    class Bare:                                                            # any object with a few attributes will do
        lag = 4

    got = curriculum_config(Bare(), (4,))
    assert got.val_tau == 4 and got.batch_size == 256 and got.grad_clip_norm is None and got.seed == 0


# ---- vamp2_proxy and the whitening block -------------------------------------------------------------------------------
def test_vamp2_proxy_against_a_direct_computation():
    rng = np.random.default_rng(5)
    Y = np.cumsum(rng.normal(size=(300, 3)), axis=0)
    it = np.arange(290)
    itau = it + 10
    want = np.mean([np.corrcoef(Y[it, c], Y[itau, c])[0, 1] ** 2 for c in range(3)])
    got = vamp2_proxy(Y, it, itau)
    assert isinstance(got, float) and abs(got - want) <= 1e-9 * want          # the 1e-12 pad of each deviation
    assert vamp2_proxy(Y.astype(np.float32), it.tolist(), itau.tolist()) == pytest.approx(want, rel=1e-5)
    assert vamp2_proxy(Y, [], []) == 0.0 and vamp2_proxy(np.zeros((0, 3)), it, itau) == 0.0
    assert vamp2_proxy(Y, [3], [9]) == 0.0                                   # a single pair
    assert vamp2_proxy(np.ones((50, 2)), it[:40], itau[:40]) == 0.0          # constant outputs: 0 / 1e-12


def test_shrunk_covariance_and_whitening_block():
    rng = np.random.default_rng(6)
    Y = rng.normal(size=(400, 3)) @ np.array([[2.0, 0.3, 0.0], [0.0, 1.0, 0.5], [0.0, 0.0, 0.2]]) + [1.0, -2.0, 0.5]
    X = Y - Y.mean(axis=0)
    emp = X.T @ X / 400
    shrunk = 0.98 * emp + 0.02 * np.trace(emp) / 3 * np.eye(3)
    want = shrunk + 1e-5 * np.trace(shrunk) / 3 * np.eye(3)
    assert np.max(np.abs(shrunk_covariance(X) - want)) <= 1e-14 * np.max(np.abs(want))
    assert np.array_equal(shrunk_covariance(X[:1]), np.eye(3)) and shrunk_covariance(np.zeros((0, 3))).shape == (0, 0)
    idx_tau = np.arange(5, 400)
    info = output_whitening_info(Y, idx_tau)
    assert list(info) == ["output_variance", "var_zt", "cond_c00", "cond_ctt", "mean", "transform", "transform_applied"]
    Tm = np.asarray(info["transform"])
    assert np.max(np.abs(Tm @ want @ Tm.T - np.eye(3))) <= 1e-10                # the inverse square root
    lam = np.linalg.eigvalsh(want)
    assert abs(info["cond_c00"] - lam[-1] / lam[0]) <= 1e-10 * info["cond_c00"]
    assert np.allclose(info["output_variance"], Y.var(axis=0, ddof=1), rtol=1e-13)
    assert np.allclose(info["var_zt"], (Y[idx_tau] - Y.mean(axis=0)).var(axis=0, ddof=1), rtol=1e-13)
    assert np.allclose(info["mean"], Y.mean(axis=0), rtol=1e-15) and info["transform_applied"] is False
    assert info["cond_ctt"] > 1.0 and output_whitening_info(Y)["cond_ctt"] is None
    assert output_whitening_info(np.zeros((0, 2)))["transform"] == []
    # eigenvalues below the floor are clipped at it: a floor above all of them leaves I / sqrt(floor)
    flat = output_whitening_info(Y, eig_floor=100.0)
    assert np.max(np.abs(np.asarray(flat["transform"]) - 0.1 * np.eye(3))) <= 1e-14 and flat["cond_c00"] == 1.0


def test_train_deeptica_refuses_before_it_needs_a_device():
    with pytest.raises(ValueError, match="Expected at least one trajectory array for DeepTICA"):
        train_deeptica([], None, DeepTICAConfig(lag=2))

    class Cfg:
        trainer_backend = "keras"

    with pytest.raises(ValueError, match="Unsupported DeepTICA trainer backend 'keras'. Valid backends: curriculum, "
                                         "deeptime, lightning, mlcolvar"):
        train_deeptica([np.zeros((5, 2))], None, Cfg())


def test_train_cv_model_refuses_unknown_methods():
    from pmarlo_amd.cv import train_cv_model

    with pytest.raises(ValueError, match="Unknown CV method 'pca'. Choose 'tica' or 'deeptica'."):
        train_cv_model(np.zeros((5, 2)), method="pca")
