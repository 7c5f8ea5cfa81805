"""Regenerate tests/golden/deeptica_weighted*.npz / deeptica_weighted.json from the reference implementation.

Run in the build container only (the reference tree does not travel):

    PYTHONPATH=<reference checkout>/src python tests/golden/make_golden_deeptica_weighted.py

Recorded, all computed by the reference's own code:
  * weighted loss cases (tests/_deeptica_weighted_ref.LOSS_CASES): VAMP2Loss.forward(z0, zt, weights)'s loss, score
    and latest_metrics, and the gradients of the loss with respect to both outputs from torch's autograd (fp64).
    Every case must keep n_out + 2 positive weights and the restatement must sit within 1e-12 of the reference, or
    nothing is written;
  * for the network cases `one` and `wide`, pair set `a`, under log-normal weights: the fp32 parameter gradients of
    the reference network, by state_dict key, with loss and score, and `ref_dev_grad` per tensor -- the rules of
    make_golden_deeptica_train.py, its refusal of a ref_dev_grad of 0 or above 1e-4 included;
  * from one run of the reference's train_deeptica on T.toy_sequence(): the keys of training_history, in order,
    pair_diagnostics_overall, the scaler's mean_ / scale_, the initial weights and vamp2_before.
Arrays: deeptica_weighted.npz, and one file more per large shape (no committed file above 1 MiB).
Inputs, weights and parameters come from the seeded recipes and are NOT stored.  No reference source text is stored.
"""

from __future__ import annotations

import json
import sys
import warnings
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from pmarlo.features.deeptica._full import DeepTICAConfig, train_deeptica  # noqa: E402
from pmarlo.features.deeptica.core.history import vamp2_proxy  # noqa: E402
from pmarlo.features.deeptica.core.inputs import prepare_features  # noqa: E402
from pmarlo.features.deeptica.core.model import build_network  # noqa: E402
from pmarlo.features.deeptica.losses import VAMP2Loss  # noqa: E402
from sklearn.preprocessing import StandardScaler  # noqa: E402

from tests import _deeptica_ref as R  # noqa: E402
from tests import _deeptica_train_ref as T  # noqa: E402
from tests import _deeptica_weighted_ref as WR  # noqa: E402

warnings.filterwarnings("ignore")

TOY_PIPELINE = {"tau_schedule": (2, 5), "val_tau": 5, "epochs_per_tau": 3, "warmup_epochs": 1, "learning_rate": 1e-2,
                "batch_size": 256, "seed": 0, "trainer_backend": "curriculum", "num_workers": 0, "val_frac": 0.2}


def _tuples(config):
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in config.items()}


def loss_cases(arrays, doc):
    doc["loss"] = {}
    for shape_key, pattern in WR.LOSS_CASES:
        Y0, Yt, w, opts = WR.case(shape_key, pattern)
        assert int(np.count_nonzero(w > 0)) >= Y0.shape[1] + 2, (shape_key, pattern)
        z0 = torch.tensor(Y0, dtype=torch.float64, requires_grad=True)
        zt = torch.tensor(Yt, dtype=torch.float64, requires_grad=True)
        fn = VAMP2Loss(eps=opts["eps"], eps_abs=opts["eps_abs"], alpha=opts["alpha"], cond_reg=opts["cond_reg"])
        loss, score = fn(z0, zt, torch.tensor(w, dtype=torch.float64))
        loss.backward()
        g0, gt = z0.grad.numpy(), zt.grad.numpy()
        mine = WR.vamp2_weighted(Y0, Yt, w, **opts)
        scale = max(np.max(np.abs(g0)), np.max(np.abs(gt)), mine["term_scale"])
        dev = max(np.max(np.abs(mine["grad0"] - g0)), np.max(np.abs(mine["grad_t"] - gt))) / scale
        dev_loss = abs(mine["loss"] - float(loss)) / abs(float(loss))
        assert dev <= 1e-12 and dev_loss <= 1e-12, (shape_key, pattern, dev, dev_loss)
        tag = f"{shape_key}__{pattern}"
        arrays[f"loss_g0__{tag}"], arrays[f"loss_gt__{tag}"] = g0, gt
        doc["loss"][tag] = {"loss": float(loss), "score": float(score), "metrics": fn.latest_metrics,
                            "restatement_dev": float(dev), "restatement_dev_loss": float(dev_loss)}
        print("loss case", tag, float(loss), float(score), "restatement dev", dev, dev_loss)


def grad_cases(arrays, doc):
    doc["grad"] = {}
    for name in WR.NET_CASES:
        c = R.case(name)
        cfg = DeepTICAConfig(**_tuples(c["config"]))
        scaler = StandardScaler(with_mean=True, with_std=True)
        scaler.mean_, scaler.scale_ = c["mean"].copy(), c["std"].copy()
        scaler.n_features_in_ = int(c["mean"].shape[0])
        net = build_network(cfg, scaler, seed=0)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c["params"].items()}, strict=True)
        net.eval()
        X = T.train_frames(name)
        Z = torch.as_tensor(scaler.transform(np.asarray(X, dtype=np.float64)), dtype=torch.float32)
        it, itau = T.pairs(name, "a")
        w = WR.net_weights(name, "a")
        fn = VAMP2Loss(**T.LOSS_OPTS)
        loss, score = fn(net(Z[it]), net(Z[itau]), torch.tensor(w, dtype=torch.float64))
        loss.backward()
        mine = WR.loss_grad_weighted(name, X, it, itau, w)
        top = max(float(np.max(np.abs(g))) for g in mine["grads"].values())
        devs, blind = {}, []
        for key, p in net.named_parameters():
            g = p.grad.detach().numpy().astype(np.float64)
            arrays[f"grad__{name}__a__{key}"] = p.grad.detach().numpy()
            dev, scale = float(np.max(np.abs(g - mine["grads"][key]))), float(np.max(np.abs(mine["grads"][key])))
            if scale <= 1e-9 * top:              # a tensor the loss cannot see: an exact zero reached by cancellation
                assert 0.0 < dev <= 1e-5 * top, (name, key, dev, top)
                blind.append(key)
            else:
                assert 0.0 < dev <= 1e-4 * scale, (name, key, dev, scale)
            devs[key] = dev
        doc["grad"][f"{name}__a"] = {"loss": float(loss), "score": float(score), "ref_dev_grad": devs,
                                     "zero_tensors": blind}
        print(name, float(loss), max(devs.values()))


def pipeline(arrays, doc):
    seq = T.toy_sequence()
    cfg = DeepTICAConfig(**_tuples(T.TOY_CONFIG), **TOY_PIPELINE)
    prep = prepare_features([seq], tau_schedule=cfg.tau_schedule, seed=cfg.seed)
    net = build_network(cfg, prep.scaler, seed=cfg.seed)
    for key, value in net.state_dict().items():
        arrays[f"toy_init__{key}"] = value.detach().numpy().copy()
    model = train_deeptica([seq], None, cfg)
    hist = model.training_history
    # the network built above is the one the run started from: it reproduces the run's untrained score
    net.eval()
    with torch.no_grad():
        out0 = net(torch.as_tensor(prep.Z, dtype=torch.float32)).numpy().astype(np.float64)
    diag = hist["pair_diagnostics_overall"]
    n = seq.shape[0]
    it = np.concatenate([np.arange(n - tau) for tau in cfg.tau_schedule])
    itau = np.concatenate([np.arange(n - tau) + tau for tau in cfg.tau_schedule])
    assert float(vamp2_proxy(out0, it, itau)) == hist["vamp2_before"], (vamp2_proxy(out0, it, itau), hist["vamp2_before"])
    arrays["toy_scaler_mean"], arrays["toy_scaler_scale"] = np.asarray(prep.scaler.mean_), np.asarray(prep.scaler.scale_)
    doc["pipeline"] = {"config": TOY_PIPELINE | {"tau_schedule": list(TOY_PIPELINE["tau_schedule"])},
                       "history_keys": list(hist.keys()), "pair_diagnostics_overall": diag,
                       "vamp2_before": float(hist["vamp2_before"]), "vamp2_after": float(hist["vamp2_after"]),
                       "usable_pairs": hist["usable_pairs"], "pair_coverage": hist["pair_coverage"],
                       "history_source": hist["history_source"]}
    print("pipeline", doc["pipeline"]["history_keys"], hist["vamp2_before"], hist["vamp2_after"])


def main():
    arrays, doc = {}, {}
    loss_cases(arrays, doc)
    grad_cases(arrays, doc)
    pipeline(arrays, doc)
    (HERE / "deeptica_weighted.json").write_text(json.dumps(doc, indent=1) + "\n")
    groups = {"t3": "loss_g0__t3__ loss_gt__t3__", "s600_0": "loss_g0__s600__lognormal loss_gt__s600__lognormal "
              "loss_g0__s600__float32 loss_gt__s600__float32", "s600_1": "loss_g0__s600__zeros loss_gt__s600__zeros "
              "loss_g0__s600__chunk loss_gt__s600__chunk", "wide": "grad__wide__"}
    taken = set()
    for suffix, prefixes in groups.items():
        part = {k: v for k, v in arrays.items() if k.startswith(tuple(prefixes.split()))}
        taken |= set(part)
        np.savez_compressed(HERE / f"deeptica_weighted_{suffix}.npz", **part)
    np.savez_compressed(HERE / "deeptica_weighted.npz", **{k: v for k, v in arrays.items() if k not in taken})
    for path in sorted(HERE.glob("deeptica_weighted*")):
        assert path.stat().st_size < 1 << 20, path
        print("wrote", path.name, path.stat().st_size)


if __name__ == "__main__":
    main()
