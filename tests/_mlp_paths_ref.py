"""The networks, frames and pair sets of the launch-path tests of the DeepTICA network kernels (csrc/mlp.hip,
mlp_vjp.hip, mlp_train.hip), and their law.  No new law: everything is composed from the fp64 restatements
tests/_deeptica_ref.forward, tests/_deeptica_train_ref.loss_grad (forward_train, vamp2, backward, dropout_factor)
and tests/_bias_ref.mlp_vjp.

NETS holds the networks at the edges of the envelope that no case of R.CASES reaches; they are drawn by R.recipe's
method (crc32-seeded, fp32 parameters, LayerNorm gamma / beta well away from (1, 0), a scaler that is not trivial) and
stay out of R.CASES, which the golden-parity tests parametrise over.  `case` also answers for a name of R.CASES, so
that "odd" and "leaky" can be run on longer frame arrays.

frames(name, n): T.train_frames' recipe at any length (a random walk pushed through a mixing, so that the VAMP score
is not trivial); every frame is distinct.  pairs(name, m, n): m lagged pairs drawn from n frames, with repeated frames
for certain.

`permuted` is the second route through the same law, identical in exact arithmetic: the hidden units of every layer
permuted (with the rows / columns of the neighbouring weights and the LayerNorm gamma / beta), the input features
permuted (with the scaler), the pair order permuted, the dropout masks carried along.  `unpermute_*` bring its
results back.  tests/test_mlp_paths_reference.py asserts that the two routes agree within 1e-12 of the largest entry
of every tensor: the law itself is two orders finer than the 1e-10 the device is held to.

Measured route distances (|route 1 - route 2| / largest entry, the largest over every shape of the host test: n = 1,
15, 16, 17, 130 and the second-trip sizes 8213 and 32 789 of a 256-CU device; m = 40, 128, 129, 256, 257, 300 with
dropout off and on, and m = 4107 for edge256):
    forward outputs                 deep8 3.0e-15   edge256 1.8e-15   head_off 3.4e-16   thin 3.2e-16
    vjp energy                      deep8 2.4e-15   edge256 1.3e-15   head_off 5.2e-16   thin 5.7e-16
    vjp gx (own and given gradient) deep8 7.2e-15   edge256 2.0e-15   head_off 6.5e-16   thin 0 (gx is an exact zero)
    R.forward against B.mlp_vjp     2.0e-15 at most (deep8)
    loss, score                     odd 2.7e-15   leaky 3.4e-15   deep8 1.8e-15   head_off 1.4e-15   edge256 3.5e-16
    training outputs                odd 1.7e-14   leaky 6.8e-16   deep8 9.9e-15   head_off 7.9e-16   edge256 1.3e-15
    parameter gradients, the worst tensor of each network:
        odd 3.1e-14 (inner.nn.15.bias, m = 257)         leaky 4.4e-14 (inner.nn.4.bias, m = 128, dropout)
        deep8 1.9e-13 (inner.nn.25.bias, m = 256)       head_off 3.0e-14 (inner.nn.2.bias, m = 129, dropout)
        edge256 8.9e-14 (inner.nn.8.bias, m = 4107, dropout)
    cond C00, cond Ctt              odd 16.3   leaky 1.0   deep8 20.4   head_off 12.0   edge256 63.8, against 1e4
All are under the 1e-12 asserted.  deep8's worst tensor is the bias of its tanh head: where the outputs vary little
over the frames, tanh' is nearly constant and that gradient is nearly the column sum of dL/dY, which is zero, so its
largest entry is small against its terms.  With the plain seed string "deep8" one output column had a spread of 0.04
and the routes differed by 1.2e-12 (m = 300); the seed string "deep8:3" (SALT) gives outputs whose columns spread by
0.16 to 0.43, and the figure above."""

from __future__ import annotations

import zlib

import numpy as np

from tests import _bias_ref as B
from tests import _deeptica_ref as R
from tests import _deeptica_train_ref as T

# name: widths (F ... n_out), activation, layer_norm_in, layer_norm_hidden, head_activation, hidden dropout, x dtype
NETS = {
    "deep8":    ((33, 17, 64, 65, 16, 15, 48, 5, 4), "tanh",       True,  True,  True,  (0.1, 0.0, 0.2, 0.1, 0.0, 0.1, 0.0), "f8"),
    "edge256":  ((255, 256, 63, 64),                 "gelu",       True,  True,  True,  (0.1, 0.1),                          "f4"),
    "head_off": ((7, 32, 16, 3),                     "selu",       False, False, False, (),                                  "f4"),
    "thin":     ((1, 1, 2, 1),                       "leaky_relu", True,  True,  True,  (),                                  "f8"),
}
SALT = {"deep8": ":3"}                       # name -> suffix of the seed string (see the docstring)
SEED, STEP = 0x0123456789ABCDEF, 11          # of every dropout draw here
CHUNK_M = (128, 129, 256, 257, 300)          # m of the chunk-boundary cases: 2m = 256, 258, 512, 514, 600
SIZES = (1, 15, 16, 17, 130)                 # n of the envelope cases


def _recipe(name: str) -> dict:
    widths, act, ln_in, ln_hidden, head, drop, xdt = NETS[name]
    F, n_out = widths[0], widths[-1]
    rng = np.random.default_rng(zlib.crc32((name + SALT.get(name, "")).encode()))
    config = {"lag": 5, "n_out": n_out, "hidden": list(widths[1:-1]), "activation": act, "layer_norm_in": ln_in,
              "layer_norm_hidden": ln_hidden, "linear_head": False, "hidden_dropout": list(drop)}
    params = {}
    for key, shape in R.key_layout(config, F):
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
    return {"config": config, "params": params, "mean": mean, "std": std, "head_activation": head,
            "xdtype": np.dtype(xdt)}


_CASES: dict = {}


def case(name: str) -> dict:
    """config, params {key: fp32}, scaler mean / std, head_activation, xdtype and widths of a network of NETS or of
    R.CASES; made once, read only."""
    if name not in _CASES:
        if name in NETS:
            c = _recipe(name)
        else:
            r = R.case(name)
            c = {"config": r["config"], "params": r["params"], "mean": r["mean"], "std": r["std"],
                 "head_activation": not r["config"].get("linear_head"), "xdtype": r["X"].dtype}
        F = c["mean"].shape[0]
        c["widths"] = (F, *R.hidden_of(c["config"]), int(c["config"]["n_out"]))
        _CASES[name] = c
    return _CASES[name]


def packed(c: dict) -> np.ndarray:
    """The fp32 parameters of a case in msm_mlp_forward's packed order."""
    return np.concatenate([c["params"][k].reshape(-1) for k, _ in R.key_layout(c["config"], c["widths"][0])])


def network(c: dict) -> dict:
    """The case as the device sees it (B.network): the arguments of MLPSpec, and the `net` of B.mlp_vjp."""
    act = {"gaussian": "gelu"}.get(c["config"]["activation"], c["config"]["activation"])
    return B.network(c["widths"], B.ACTIVATIONS.index(act), c["config"]["layer_norm_in"],
                     c["config"]["layer_norm_hidden"], c["head_activation"], packed(c), c["mean"], c["std"])


def dropout_of(name: str, p_in: float = 0.1) -> list:
    """[input, hidden 0, ...] of a case: T.dropout_of for any case of `case`."""
    config = case(name)["config"]
    n_hidden = len(R.hidden_of(config))
    drop = list(config.get("hidden_dropout") or ()) or [0.0]
    return [p_in] + (drop + [drop[-1]] * n_hidden)[:n_hidden]


def frames(name: str, n: int) -> np.ndarray:
    """n correlated frames of a case in its X dtype, around its scaler: T.train_frames' recipe at length n.  All
    frames are distinct."""
    c = case(name)
    F = c["widths"][0]
    rng = np.random.default_rng(zlib.crc32(f"{name}:frames:{n}".encode()))
    walk = np.cumsum(rng.normal(size=(n, F)), axis=0) / np.sqrt(max(n, 4) / 4.0)
    mix = rng.normal(size=(F, F)) / np.sqrt(F) + np.eye(F)
    X = (c["mean"] + c["std"] * ((walk + 0.3 * rng.normal(size=(n, F))) @ mix)).astype(c["xdtype"])
    assert np.unique(X, axis=0).shape[0] == n
    X.setflags(write=False)
    return X


def pairs(name: str, m: int, n: int):
    """m pairs (t, t + lag), lag in 1 .. 7, out of n frames, in no order; frame t[0] is used three times, and the
    last pair differs from the first in its lag (swapping the two is a change)."""
    rng = np.random.default_rng(zlib.crc32(f"{name}:pairs:{m}:{n}".encode()))
    t = rng.integers(0, n - 8, size=m)
    t[m // 2] = t[0]
    t[m - 1] = t[0]
    lag = rng.integers(1, 8, size=m)
    lag[m - 1] = lag[0] % 7 + 1
    return t.astype(np.int64), (t + lag).astype(np.int64)


# ---- the law, by composition ---------------------------------------------------------------------------------------
def forward(c: dict, X) -> np.ndarray:
    return R.forward(c["config"], c["params"], c["mean"], c["std"], X, head_activation=c["head_activation"])


def vjp(c: dict, X, gout=None, strength=1.0):
    """(energy [n], outputs [n, n_out], gx [n, F]) of msm_mlp_vjp."""
    energy, y, gx, _ = B.mlp_vjp(network(c), X, gout=gout, strength=strength)
    return energy, y, gx


def upstream(name: str, n: int) -> np.ndarray:
    """A given upstream gradient [n, n_out]."""
    rng = np.random.default_rng(zlib.crc32(f"{name}:gout:{n}".encode()))
    return rng.normal(size=(n, case(name)["widths"][-1]))


def loss_grad(c: dict, X, it, itau, dropout=None, masks=None) -> dict:
    """msm_mlp_loss_grad at T.LOSS_OPTS: T.loss_grad's dict (loss, score, metrics, outputs, grads by key, grad)."""
    return T.loss_grad(c, X, it, itau, dropout=dropout, seed=SEED, step=STEP, head_activation=c["head_activation"],
                       masks=masks)


def grad_scales(c: dict, law: dict) -> dict:
    """Per parameter tensor, the scale its error is measured in: the largest entry of the law's gradient.  One tensor
    has none: the bias of a linear head.  Its gradient is the column sums of dL/dY, an exact zero (the loss does not
    move when the outputs are shifted) reached through cancelling terms, so the largest entry is rounding noise; the
    largest column sum of |dL/dY| takes its place, as the terms' size does in tests/test_gpu_deeptica_train.py."""
    scales = {k: float(np.max(np.abs(g))) for k, g in law["grads"].items()}
    if not c["head_activation"]:
        dY = np.concatenate([law["grad0"], law["grad_t"]])
        scales[T.layers_of(c["config"], c["widths"][0])[-1][1]] = float(np.max(np.abs(dY).sum(axis=0)))
    return scales


def masks_of(c: dict, m: int, dropout) -> dict:
    """{site: [2m, width] factors} as forward_train draws them."""
    return {site: T.dropout_factor(SEED, STEP, site, 2 * m, c["widths"][site], p) for site, p in enumerate(dropout)}


# ---- the second route ----------------------------------------------------------------------------------------------
def permuted(c: dict, seed: int):
    """(the case with the input features and the hidden units of every layer permuted, the permutations): perms[i]
    is that of width i (the identity for the outputs); entry j of a permuted vector is entry perms[i][j] of the
    original."""
    rng = np.random.default_rng(seed)
    w = c["widths"]
    perms = [rng.permutation(k) for k in w[:-1]] + [np.arange(w[-1])]
    P = {}
    if c["config"].get("layer_norm_in"):
        P["ln.weight"], P["ln.bias"] = c["params"]["ln.weight"][perms[0]], c["params"]["ln.bias"][perms[0]]
    for i, (kw, kb, kg, kbeta) in enumerate(T.layers_of(c["config"], w[0])):
        P[kw] = np.ascontiguousarray(c["params"][kw][perms[i + 1]][:, perms[i]])
        P[kb] = c["params"][kb][perms[i + 1]]
        if kg is not None:
            P[kg], P[kbeta] = c["params"][kg][perms[i + 1]], c["params"][kbeta][perms[i + 1]]
    assert set(P) == set(c["params"])
    return {**c, "params": P, "mean": c["mean"][perms[0]], "std": c["std"][perms[0]]}, perms


def unpermute_columns(a, perm) -> np.ndarray:
    out = np.empty_like(a)
    out[..., perm] = a
    return out


def unpermute_grads(c: dict, grads: dict, perms) -> dict:
    out = {}
    if "ln.weight" in grads:
        out["ln.weight"], out["ln.bias"] = (unpermute_columns(grads[k], perms[0]) for k in ("ln.weight", "ln.bias"))
    for i, (kw, kb, kg, kbeta) in enumerate(T.layers_of(c["config"], c["widths"][0])):
        W = np.empty_like(grads[kw])
        W[np.ix_(perms[i + 1], perms[i])] = grads[kw]
        out[kw], out[kb] = W, unpermute_columns(grads[kb], perms[i + 1])
        if kg is not None:
            out[kg], out[kbeta] = unpermute_columns(grads[kg], perms[i + 1]), unpermute_columns(grads[kbeta], perms[i + 1])
    return out


def second_route_forward(c: dict, X, gout=None, strength=1.0, seed=1):
    """(outputs, energy, gx) of the permuted network on the permuted features, brought back."""
    c2, perms = permuted(c, seed)
    X2 = np.asarray(X)[:, perms[0]]
    energy, y, gx = vjp(c2, X2, gout=gout, strength=strength)
    return y, energy, unpermute_columns(gx, perms[0])


def second_route_loss_grad(c: dict, X, it, itau, dropout=None, seed=1) -> dict:
    """loss_grad with features, hidden units and pairs permuted (and the masks with them), brought back."""
    c2, perms = permuted(c, seed)
    m = len(it)
    sigma = np.random.default_rng(seed + 1).permutation(m)
    slots = np.concatenate([sigma, m + sigma])
    masks = None
    if dropout is not None:
        masks = {site: f[slots][:, perms[site]] for site, f in masks_of(c, m, dropout).items()}
    res = loss_grad(c2, np.asarray(X)[:, perms[0]], it[sigma], itau[sigma], dropout=dropout, masks=masks)
    back = np.empty_like(res["outputs"])
    back[slots] = res["outputs"]
    return {"loss": res["loss"], "score": res["score"], "metrics": res["metrics"], "outputs": back,
            "grads": unpermute_grads(c, res["grads"], perms)}


def rel(got, want) -> float:
    """|got - want| over the largest entry of want; 0 when both are all zero."""
    want = np.asarray(want, np.float64)
    err, top = float(np.max(np.abs(np.asarray(got, np.float64) - want))), float(np.max(np.abs(want)))
    return 0.0 if err == 0.0 else err / top if top > 0.0 else np.inf
