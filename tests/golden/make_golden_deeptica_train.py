"""Regenerate tests/golden/deeptica_train.npz / deeptica_train.json from the reference implementation.

Run in the build container only (the reference tree does not travel):

    PYTHONPATH=<reference checkout>/src python tests/golden/make_golden_deeptica_train.py

Recorded, all computed by the reference's own code:
  * loss cases (tests/_deeptica_train_ref.LOSS_SHAPES): VAMP2Loss.forward's loss, score and latest_metrics, and the
    gradients of the loss with respect to both outputs from torch's autograd (fp64);
  * per network case and pair set: the fp32 parameter gradients of the reference network (build_network with the
    recipe's parameters, dropout off) under VAMP2Loss, by state_dict key, with loss and score; and `ref_dev_grad` per
    tensor, the largest distance of that fp32 gradient from the fp64 restatement -- the yardstick of the GPU tests.
    A case whose ref_dev_grad is 0 or above 1e-4 of the tensor's largest entry is refused: that is a kink of relu
    that fp32 and fp64 land on differently, and the test would show nothing;
  * the key list of DeepTICACurriculumTrainer._build_history;
  * the split, the pair diagnostics and the learning-rate curve of the toy run, and its untrained and best
    validation scores for the seeds T.TOY_SEEDS of the initialisation, with the initial weights of each run (the
    untrained score depends on the draw far more than on anything else, so the device run starts where the
    reference's did).
The arrays go to deeptica_train.npz, those of the widest case to deeptica_train_wide_{a,b,c}.npz.
Inputs and parameters come from the seeded recipes and are NOT stored.  No reference source text is stored.
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

from pmarlo.features.deeptica._full import DeepTICAConfig  # noqa: E402
from pmarlo.features.deeptica.core.model import build_network  # noqa: E402
from pmarlo.features.deeptica.losses import VAMP2Loss  # noqa: E402
from pmarlo.ml.deeptica.trainer import CurriculumConfig, DeepTICACurriculumTrainer  # noqa: E402
from sklearn.preprocessing import StandardScaler  # noqa: E402

from tests import _deeptica_ref as R  # noqa: E402
from tests import _deeptica_train_ref as T  # noqa: E402

warnings.filterwarnings("ignore")

PAIR_SETS = {name: ["a", "b"] for name in R.CASES}
PAIR_SETS["wide"].append("c")
PAIR_SETS["one"].append("d")


def loss_cases(arrays, doc):
    doc["loss"] = []
    for i in range(len(T.LOSS_SHAPES)):
        Y0, Yt, opts = T.loss_case(i)
        z0 = torch.tensor(Y0, dtype=torch.float64, requires_grad=True)
        zt = torch.tensor(Yt, dtype=torch.float64, requires_grad=True)
        fn = VAMP2Loss(eps=opts["eps"], eps_abs=opts["eps_abs"], alpha=opts["alpha"], cond_reg=opts["cond_reg"])
        loss, score = fn(z0, zt, torch.full((Y0.shape[0],), 1.0 / Y0.shape[0], dtype=torch.float32))
        loss.backward()
        arrays[f"loss_g0__{i}"], arrays[f"loss_gt__{i}"] = z0.grad.numpy(), zt.grad.numpy()
        mine = T.vamp2(Y0, Yt, **opts)
        dev = max(np.max(np.abs(mine["grad0"] - z0.grad.numpy())), np.max(np.abs(mine["grad_t"] - zt.grad.numpy())))
        scale = max(np.max(np.abs(z0.grad.numpy())), np.max(np.abs(zt.grad.numpy())))
        doc["loss"].append({"loss": float(loss), "score": float(score), "metrics": fn.latest_metrics,
                            "restatement_dev": float(dev / scale)})
        print("loss case", i, float(loss), float(score), "restatement dev", dev / scale)


def network(name):
    c = R.case(name)
    cfg = DeepTICAConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in c["config"].items()})
    scaler = StandardScaler(with_mean=True, with_std=True)
    scaler.mean_, scaler.scale_ = c["mean"].copy(), c["std"].copy()
    scaler.n_features_in_ = int(c["mean"].shape[0])
    net = build_network(cfg, scaler, seed=0)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c["params"].items()}, strict=True)
    net.eval()                                       # dropout off; gradients still flow
    return c, scaler, net


def grad_cases(arrays, doc):
    doc["grad"] = {}
    for name, sets in PAIR_SETS.items():
        c, scaler, net = network(name)
        X = T.train_frames(name)
        Z = torch.as_tensor(scaler.transform(np.asarray(X, dtype=np.float64)), dtype=torch.float32)
        for which in sets:
            it, itau = T.pairs(name, which)
            net.zero_grad(set_to_none=True)
            fn = VAMP2Loss(**T.LOSS_OPTS)
            m = len(it)
            loss, score = fn(net(Z[it]), net(Z[itau]), torch.full((m,), 1.0 / m, dtype=torch.float32))
            loss.backward()
            mine = T.loss_grad(name, X, it, itau)
            devs = {}
            # two pairs and one output: the score is the constant 1 / (1 + alpha + eps)^2 whatever the parameters
            # are, so the gradient is an exact zero that both sides reach through cancelling terms; there is no
            # ref_dev_grad to measure, and the reference's largest entry is recorded instead
            constant = m == 2 and R.CASES[name][2] == 1
            # a tensor the loss cannot see (a shift of every output leaves the centred covariances as they are: the
            # last bias, and the input LayerNorm's beta, of a network with a linear head and no hidden layer) has an
            # exact zero gradient too; it is told by its size against the case's largest gradient entry
            top = max(float(np.max(np.abs(g))) for g in mine["grads"].values())
            blind = []
            for key, p in net.named_parameters():
                g = p.grad.detach().numpy().astype(np.float64)
                arrays[f"grad__{name}__{which}__{key}"] = p.grad.detach().numpy()
                dev, scale = float(np.max(np.abs(g - mine["grads"][key]))), float(np.max(np.abs(mine["grads"][key])))
                if constant:
                    assert float(np.max(np.abs(g))) <= 1e-5 * float(score), (name, which, key, g)
                elif scale <= 1e-9 * top:
                    assert 0.0 < dev <= 1e-5 * top, (name, which, key, dev, top)
                    blind.append(key)
                else:
                    assert 0.0 < dev <= 1e-4 * scale, (name, which, key, dev, scale)
                devs[key] = dev
            doc["grad"][f"{name}__{which}"] = {"loss": float(loss), "score": float(score), "ref_dev_grad": devs,
                                               "constant_score": constant, "zero_tensors": blind}
            print(name, which, float(loss), max(d for d in devs.values()))


def toy(arrays, doc):
    runs = []
    for seed in T.TOY_SEEDS:
        seq = T.toy_sequence()
        cfg = DeepTICAConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in T.TOY_CONFIG.items()})
        scaler = StandardScaler()
        scaler.mean_, scaler.scale_, scaler.n_features_in_ = np.zeros(7), np.ones(7), 7
        net = build_network(cfg, scaler, seed=seed)
        for key, value in net.state_dict().items():         # the initial weights: the device run starts from them
            arrays[f"toy_init__{seed}__{key}"] = value.detach().numpy().copy()
        tr = DeepTICACurriculumTrainer(net, CurriculumConfig(device="cpu", seed=seed, **T.TOY_TRAINER))
        train, val = tr._prepare_train_val([seq], None)
        untrained = tr._evaluate(tr._build_validation_loader(val))["score"]
        hist = tr.fit([seq])
        runs.append({"seed": seed, "untrained": float(untrained), "best": float(hist["best_val_score"]),
                     "split": int(train[0].shape[0])})
        print("toy seed", seed, runs[-1])
    doc["history_keys"] = list(hist.keys())
    doc["toy"] = {"runs": runs, "learning_rate_curve": hist["learning_rate_curve"],
                  "pair_diagnostics": {str(k): v for k, v in hist["pair_diagnostics"].items()},
                  "curve_length": len(hist["val_score_curve"])}


def main():
    arrays, doc = {}, {}
    loss_cases(arrays, doc)
    grad_cases(arrays, doc)
    toy(arrays, doc)
    (HERE / "deeptica_train.json").write_text(json.dumps(doc, indent=1) + "\n")
    # the widest case's gradients go to a file per pair set: no committed file above 1 MiB
    wide = {w: {k: v for k, v in arrays.items() if k.startswith(f"grad__wide__{w}__")} for w in PAIR_SETS["wide"]}
    rest = {k: v for k, v in arrays.items() if not k.startswith("grad__wide__")}
    np.savez_compressed(HERE / "deeptica_train.npz", **rest)
    for w, part in wide.items():
        np.savez_compressed(HERE / f"deeptica_train_wide_{w}.npz", **part)
    print("wrote", HERE / "deeptica_train.json", HERE / "deeptica_train.npz", "and the wide case's files")


if __name__ == "__main__":
    main()
