"""The DeepTICA inference law in fp64 numpy, and the seeded recipes of the test cases.

`forward` / `transform` restate what the reference's DeepTICAModel.transform computes in evaluation mode
(S/features/deeptica/_full.py:283-309 over the network of S/features/deeptica/core/model.py:72-107, 355-368), with
every operation after the fp32 rounding of Z carried out in float64; `whiten` restates
pmarlo.ml.deeptica.whitening.apply_output_transform in plain numpy (no product code).  tests/golden/deeptica.json
records how far the reference's own fp32 evaluation lies from this restatement (`ref_dev`), which is the yardstick
of the GPU tests.

The recipes make, from a seed, the config, every parameter (fp32, LayerNorm gamma / beta well off (1, 0)), the
scaler and X of a case; nothing of them is stored."""

from __future__ import annotations

import zlib

import numpy as np
from scipy.special import erf

SELU_ALPHA = 1.6732632423543772848170429916717
SELU_SCALE = 1.0507009873554804934193349852946

# name: F, hidden, n_out, activation, layer_norm_in, layer_norm_hidden, linear_head, hidden_dropout, n, x dtype,
#       whitening ("none" | "ok" | "bad": metadata absent, consistent, inconsistent)
CASES = {
    "wide":        (256, (256, 128),       17, "gelu",       True,  True,  False, (),                   130, "f4", "none"),
    "odd":         (33,  (17, 16, 15, 4),  3,  "tanh",       False, True,  False, (0.1, 0.0, 0.2, 0.1), 130, "f8", "ok"),
    "one":         (1,   (5,),             1,  "tanh",       False, False, False, (),                   1,   "f8", "none"),
    "default":     (7,   (),               3,  "relu",       True,  False, False, (),                   15,  "f4", "none"),
    "linear_head": (64,  (32, 16),         17, "selu",       True,  False, True,  (),                   16,  "f4", "ok"),
    "selu":        (7,   (32, 16),         3,  "selu",       False, False, False, (),                   17,  "f8", "bad"),
    "leaky":       (33,  (5,),             1,  "leaky_relu", False, True,  False, (0.3,),               63,  "f4", "ok"),
    "unknown":     (7,   (5,),             3,  "swish",      True,  True,  False, (),                   65,  "f8", "none"),
    "flagship":    (64,  (128, 64),        3,  "gaussian",   True,  True,  False, (0.1, 0.1),           130, "f4", "ok"),
    "elu":         (64,  (32, 16),         3,  "elu",        False, False, False, (),                   16,  "f4", "none"),
}


def config_of(name: str) -> dict:
    F, hidden, n_out, act, ln_in, ln_hidden, linear_head, drop, n, xdt, wh = CASES[name]
    return {"lag": 5, "n_out": n_out, "hidden": list(hidden), "activation": act, "layer_norm_in": ln_in,
            "layer_norm_hidden": ln_hidden, "linear_head": linear_head, "hidden_dropout": list(drop)}


def hidden_of(config: dict) -> tuple:
    if config.get("linear_head"):
        return ()
    return tuple(config.get("hidden") or ()) or (32, 16)


def key_layout(config: dict, F: int):
    """[(key, shape), ...] of the network's state_dict in module order: the Sequential gives an index to every
    module, so LayerNorms, activations and dropouts with p > 0 make the Linear indices skip."""
    widths = (F, *hidden_of(config), int(config["n_out"]))
    drop = list(config.get("hidden_dropout") or ())
    transitions = len(widths) - 2
    if transitions > 0:
        drop = (drop or [0.0])
        drop = (drop + [drop[-1]] * transitions)[:transitions]
    keys = []
    if config.get("layer_norm_in"):
        keys += [("ln.weight", (F,)), ("ln.bias", (F,))]
    idx = 0
    for i in range(len(widths) - 1):
        keys += [(f"inner.nn.{idx}.weight", (widths[i + 1], widths[i])), (f"inner.nn.{idx}.bias", (widths[i + 1],))]
        idx += 1
        if i < len(widths) - 2:
            if config.get("layer_norm_hidden"):
                keys += [(f"inner.nn.{idx}.weight", (widths[i + 1],)), (f"inner.nn.{idx}.bias", (widths[i + 1],))]
                idx += 1
            idx += 1                                  # activation
            if drop[i] > 0:
                idx += 1
    return keys


def recipe(name: str) -> dict:
    """config, params {key: fp32 array}, scaler mean / std (fp64), X [n, F] and the training history of a case."""
    F, hidden, n_out, act, ln_in, ln_hidden, linear_head, drop, n, xdt, wh = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    config = config_of(name)
    params = {}
    for key, shape in key_layout(config, F):
        if len(shape) == 2:
            v = rng.normal(size=shape) * (1.3 / np.sqrt(shape[1]))
        elif key.endswith("weight"):
            v = rng.uniform(0.4, 1.7, size=shape) * rng.choice([-1.0, 1.0], size=shape)     # LayerNorm gamma
        elif key.startswith("ln.") or (key.replace("bias", "weight") in params
                                       and params[key.replace("bias", "weight")].ndim == 1):
            v = rng.normal(size=shape) * 0.6                                                 # LayerNorm beta
        else:
            v = rng.normal(size=shape) * 0.3
        params[key] = v.astype(np.float32)
    mean = rng.normal(size=F) * 2.0
    std = rng.uniform(0.5, 2.0, size=F)
    X = (mean + std * rng.normal(size=(n, F)) * 1.2).astype(np.dtype(xdt))
    history = None
    if wh != "none":
        A = rng.normal(size=(n_out, n_out)) * 0.3 + np.eye(n_out)
        history = {"output_mean": (rng.normal(size=n_out) * 0.2).tolist(), "output_transform": A.tolist(),
                   "output_transform_applied": False}
        if wh == "bad":
            history["output_mean"] = history["output_mean"] + [0.0]      # one entry too many
    return {"config": config, "params": params, "mean": mean, "std": std, "X": X, "history": history}


def _activation(name):
    key = (name or "").strip().lower()
    if key in ("gelu", "gaussian"):
        return lambda x: 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))
    if key in ("relu", "relu+"):
        return lambda x: np.maximum(x, 0.0)
    if key == "elu":
        return lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    if key == "selu":
        return lambda x: SELU_SCALE * np.where(x > 0, x, SELU_ALPHA * np.expm1(np.minimum(x, 0.0)))
    if key in ("leaky_relu", "lrelu"):
        return lambda x: np.where(x < 0, 0.01 * x, x)
    return np.tanh


def _layer_norm(x, gamma, beta):
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * gamma.astype(np.float64) + beta.astype(np.float64)


def forward(config: dict, params: dict, mean, std, X, head_activation=None) -> np.ndarray:
    """Raw network outputs [n, n_out] in float64 (steps 1-4).  head_activation: None follows the config (the head is
    activated unless linear_head, which also drops the hidden layers); a bool overrides it, which is how a network
    with hidden layers and a linear head -- one the C API allows and no config produces -- is stated."""
    head = (not config.get("linear_head")) if head_activation is None else bool(head_activation)
    Z = (np.asarray(X, np.float64) - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    x = Z.astype(np.float32).astype(np.float64)
    act = _activation(config.get("activation", "gelu"))
    if config.get("layer_norm_in"):
        x = _layer_norm(x, params["ln.weight"], params["ln.bias"])
    linear = [k for k, shape in key_layout(config, x.shape[1]) if len(shape) == 2]
    for i, key in enumerate(linear):
        idx = int(key.split(".")[2])
        x = x @ params[key].astype(np.float64).T + params[key.replace("weight", "bias")].astype(np.float64)
        if i < len(linear) - 1:
            if config.get("layer_norm_hidden"):
                x = _layer_norm(x, params[f"inner.nn.{idx + 1}.weight"], params[f"inner.nn.{idx + 1}.bias"])
            x = act(x)
        elif head:
            x = act(x)
    return x


def whiten(Y, mean, transform) -> np.ndarray:
    """Plain-numpy output whitening: (Y - mean) T, centred; with more frames than columns also decorrelated
    against the batch covariance through its Cholesky factor and centred again."""
    Y = np.asarray(Y, np.float64)
    mu, T = np.asarray(mean, np.float64), np.asarray(transform, np.float64)
    if mu.ndim != 1 or T.ndim != 2 or mu.shape[0] != T.shape[0] or Y.ndim != 2 or Y.shape[1] != mu.shape[0]:
        raise ValueError("inconsistent whitening metadata")
    u = (Y - mu) @ T
    if u.shape[0] == 0:
        return u
    u = u - u.mean(axis=0)
    if u.shape[0] > u.shape[1]:
        L = np.linalg.cholesky(u.T @ u / u.shape[0])
        u = np.linalg.solve(L.T, u.T).T
        u = u - u.mean(axis=0)
    return u


def transform(case: dict) -> np.ndarray:
    """Final outputs (step 5 on top of `forward`); inconsistent metadata leaves the raw outputs."""
    raw = forward(case["config"], case["params"], case["mean"], case["std"], case["X"])
    hist = case["history"] or {}
    if hist.get("output_mean") is None or hist.get("output_transform") is None or hist.get("output_transform_applied"):
        return raw
    try:
        return whiten(raw, hist["output_mean"], hist["output_transform"])
    except (ValueError, np.linalg.LinAlgError):
        return raw


_CACHE: dict = {}


def case(name: str) -> dict:
    """The recipe of a case with its restated raw and final outputs, computed once and shared (read only)."""
    if name not in _CACHE:
        c = recipe(name)
        c["raw"] = forward(c["config"], c["params"], c["mean"], c["std"], c["X"])
        c["final"] = transform(c)
        for v in (c["raw"], c["final"], c["X"]):
            v.setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]
