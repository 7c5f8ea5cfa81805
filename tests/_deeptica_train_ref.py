"""The DeepTICA training law in fp64 numpy, and the seeded recipes of the training test cases.

Restated here (no product code, no torch): the network in training mode with Philox dropout masks, the VAMP-2 loss
of the reference's VAMP2Loss.forward with uniform weights and its closed-form output gradient, the manual backward
pass, and gradient clip + AdamW -- everything include/msmhip.h states for msm_vamp2_loss, msm_mlp_loss_grad and
msm_adamw_step.  tests/test_deeptica_train_host.py pins the gradients against torch's fp64 autograd and the loss
against the reference's recorded values; the GPU tests compare the device against this module.

The networks are those of tests/_deeptica_ref.py (R.CASES).  Per case the training frames are 77 correlated frames
(a cumulative sum pushed through a random mixing, so the VAMP score is not trivial) and the pair sets
  a: all (t, t + 3): m = 74, nine groups of 16 slots and four more,
  b: 21 shuffled pairs with repeated frames,
  c: m = 16, whole groups only,
  d: m = 2 (case "one").
Nothing of them is stored."""

from __future__ import annotations

import zlib

import numpy as np
from scipy.special import erf

from oracle.npport import philox4x32
from tests import _deeptica_ref as R

N_FRAMES = 77
LOSS_OPTS = {"eps": 1e-3, "eps_abs": 1e-6, "alpha": 0.15, "cond_reg": 1e-4}
FLOOR = 1e-12

# (m, n_out, alpha, cond_reg) of the loss cases, then the smallest shape
LOSS_SHAPES = [(5, 3, 0.15, 1e-4), (37, 3, 0.0, 0.05), (125, 17, 0.15, 0.05), (250, 64, 0.3, 1e-4), (2, 1, 0.15, 1e-4)]


# ---- recipes -------------------------------------------------------------------------------------------------------
def loss_case(i: int):
    """Outputs (Y0, Yt) of loss case i: correlated, off-centre, columns of unequal scale."""
    m, d, alpha, cond_reg = LOSS_SHAPES[i]
    rng = np.random.default_rng(1000 + i)
    base = rng.normal(size=(m, d))
    mix = rng.normal(size=(d, d)) / np.sqrt(d) + np.eye(d)
    scale = rng.uniform(0.3, 3.0, size=d)
    Y0 = (base @ mix) * scale + rng.normal(size=d)
    Yt = (0.7 * base + 0.5 * rng.normal(size=(m, d))) @ mix * scale + rng.normal(size=d)
    return Y0, Yt, {"eps": 1e-3, "eps_abs": 1e-6, "alpha": alpha, "cond_reg": cond_reg}


def train_frames(name: str) -> np.ndarray:
    """77 correlated frames of a case in its X dtype, around the recipe's scaler."""
    c = R.case(name)
    F = c["X"].shape[1]
    rng = np.random.default_rng(zlib.crc32((name + ":train").encode()))
    walk = np.cumsum(rng.normal(size=(N_FRAMES, F)), axis=0) / np.sqrt(N_FRAMES / 4.0)
    mix = rng.normal(size=(F, F)) / np.sqrt(F) + np.eye(F)
    X = c["mean"] + c["std"] * ((walk + 0.3 * rng.normal(size=(N_FRAMES, F))) @ mix)
    X = X.astype(c["X"].dtype)
    X.setflags(write=False)
    return X


def pairs(name: str, which: str):
    rng = np.random.default_rng(zlib.crc32((name + ":pairs:" + which).encode()))
    if which == "a":
        t = np.arange(N_FRAMES - 3)
        return t, t + 3
    if which == "b":
        t = rng.integers(0, N_FRAMES - 8, size=21)
        t[5] = t[0]
        t[11] = t[0]                                       # repeated frames for certain
        return t, t + rng.integers(1, 8, size=21)
    if which == "c":
        t = 2 * np.arange(16)
        return t, t + 5
    if which == "d":
        return np.array([0, 5]), np.array([3, 9])
    raise KeyError(which)


def packed_params(name: str) -> np.ndarray:
    """The case's fp32 parameters in msm_mlp_forward's packed order (the state_dict's module order)."""
    c = R.case(name)
    return np.concatenate([c["params"][k].reshape(-1) for k, _ in R.key_layout(c["config"], c["X"].shape[1])])


def unpack(config: dict, F: int, packed: np.ndarray) -> dict:
    out, off = {}, 0
    for key, shape in R.key_layout(config, F):
        size = int(np.prod(shape))
        out[key] = packed[off:off + size].reshape(shape)
        off += size
    assert off == packed.size
    return out


def dropout_of(name: str, p_in: float = 0.1) -> list:
    """[input, hidden 0, ...]: the case's hidden dropout, the last value repeated, and the given input dropout."""
    config = R.case(name)["config"]
    n_hidden = len(R.hidden_of(config))
    drop = list(config.get("hidden_dropout") or ()) or [0.0]
    return [p_in] + (drop + [drop[-1]] * n_hidden)[:n_hidden]


# ---- the network in training mode ------------------------------------------------------------------------------------
def dropout_factor(seed: int, step: int, site: int, n_slots: int, width: int, p: float) -> np.ndarray:
    """[n_slots, width] of 1 / (1 - p) where the element is kept and 0 where it is dropped: kept iff word
    (column & 3) of Philox(key = seed, counter = (step, site, slot, column >> 2)) is >= floor(p 2^32)."""
    if p >= 1.0 or p < 0.0:
        raise ValueError(f"dropout probability {p}")
    thr = int(np.floor(p * 4294967296.0))
    if thr == 0:
        return np.ones((n_slots, width))
    blocks = (width + 3) // 4
    counter = np.zeros((n_slots, blocks, 4), np.uint32)
    counter[..., 0] = step
    counter[..., 1] = site
    counter[..., 2] = np.arange(n_slots, dtype=np.uint32)[:, None]
    counter[..., 3] = np.arange(blocks, dtype=np.uint32)[None, :]
    words = philox4x32(seed, counter).reshape(n_slots, blocks * 4)[:, :width]
    return np.where(words >= thr, 1.0 / (1.0 - p), 0.0)


def _act(name):
    key = (name or "").strip().lower()
    sq2pi = np.sqrt(2.0 * np.pi)
    if key in ("gelu", "gaussian"):
        return (lambda x: 0.5 * x * (1.0 + erf(x / np.sqrt(2.0))),
                lambda x: 0.5 * (1.0 + erf(x / np.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / sq2pi)
    if key in ("relu", "relu+"):
        return (lambda x: np.maximum(x, 0.0), lambda x: np.where(x <= 0.0, 0.0, 1.0))
    if key == "elu":
        return (lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0.0))),
                lambda x: np.where(x > 0, 1.0, np.exp(np.minimum(x, 0.0))))
    if key == "selu":
        return (lambda x: R.SELU_SCALE * np.where(x > 0, x, R.SELU_ALPHA * np.expm1(np.minimum(x, 0.0))),
                lambda x: R.SELU_SCALE * np.where(x > 0, 1.0, R.SELU_ALPHA * np.exp(np.minimum(x, 0.0))))
    if key in ("leaky_relu", "lrelu"):
        return (lambda x: np.where(x < 0, 0.01 * x, x), lambda x: np.where(x > 0, 1.0, 0.01))
    return (np.tanh, lambda x: 1.0 - np.tanh(x) ** 2)


def _ln_forward(x, gamma, beta):
    mu = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(axis=1, keepdims=True) + 1e-5)
    xhat = (x - mu) * rstd
    return xhat * gamma + beta, (xhat, rstd)


def _ln_backward(dy, cache, gamma):
    xhat, rstd = cache
    dxhat = dy * gamma
    dx = rstd * (dxhat - dxhat.mean(axis=1, keepdims=True) - xhat * (dxhat * xhat).mean(axis=1, keepdims=True))
    return dx, (dy * xhat).sum(axis=0), dy.sum(axis=0)


def layers_of(config: dict, F: int):
    """[(W key, b key, gamma key or None, beta key or None), ...] in layer order."""
    keys = [k for k, _ in R.key_layout(config, F)]
    shapes = dict(R.key_layout(config, F))
    out = []
    for k in keys:
        if k.startswith("inner.") and k.endswith("weight") and len(shapes[k]) == 2:
            out.append([k, k.replace("weight", "bias"), None, None])
        elif k.startswith("inner.") and k.endswith("weight"):
            out[-1][2], out[-1][3] = k, k.replace("weight", "bias")
    return out


def forward_train(config, params, mean, std, X, idx_t, idx_tau, dropout=None, seed=0, step=0, head_activation=None,
                  masks=None):
    """Outputs [2m, n_out] of the slots (t frames, then tau frames) and what the backward pass needs.  params: fp32
    arrays by key; dropout: None (evaluation) or [input, hidden 0, ...]; head_activation: as in R.forward; masks:
    {site: [2m, width] factors} used in place of dropout_factor's draw (a permuted route through the same law)."""
    draw = dropout_factor if masks is None else (lambda _seed, _step, site, *_: masks[site])
    head = (not config.get("linear_head")) if head_activation is None else bool(head_activation)
    rows = np.concatenate([np.asarray(idx_t), np.asarray(idx_tau)])
    Z = (np.asarray(X, np.float64)[rows] - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    x = Z.astype(np.float32).astype(np.float64)
    S2, F = x.shape
    act, _ = _act(config.get("activation", "gelu"))
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    tape = {"layers": []}
    if config.get("layer_norm_in"):
        x, tape["ln_in"] = _ln_forward(x, P["ln.weight"], P["ln.bias"])
    if dropout is not None:
        tape["mask_in"] = draw(seed, step, 0, S2, F, dropout[0])
        x = x * tape["mask_in"]
    layers = layers_of(config, F)
    for i, (kw, kb, kg, kbeta) in enumerate(layers):
        rec = {"a": x}
        x = x @ P[kw].T + P[kb]
        last = i == len(layers) - 1
        if kg is not None:
            x, rec["ln"] = _ln_forward(x, P[kg], P[kbeta])
        if not last or head:
            rec["h"] = x
            x = act(x)
        if not last and dropout is not None:
            rec["mask"] = draw(seed, step, i + 1, S2, x.shape[1], dropout[i + 1])
            x = x * rec["mask"]
        tape["layers"].append(rec)
    return x, tape


def backward(config, params, F, tape, dY) -> dict:
    """Gradients by key (fp64) from dL/d(outputs) [2m, n_out]."""
    _, dact = _act(config.get("activation", "gelu"))
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    grads = {}
    g = dY
    layers = layers_of(config, F)
    for i in reversed(range(len(layers))):
        kw, kb, kg, kbeta = layers[i]
        rec = tape["layers"][i]
        if "mask" in rec:
            g = g * rec["mask"]
        if "h" in rec:
            g = g * dact(rec["h"])
        if kg is not None:
            g, grads[kg], grads[kbeta] = _ln_backward(g, rec["ln"], P[kg])
        grads[kw] = g.T @ rec["a"]
        grads[kb] = g.sum(axis=0)
        g = g @ P[kw]
    if "mask_in" in tape:
        g = g * tape["mask_in"]
    if "ln_in" in tape:
        _, grads["ln.weight"], grads["ln.bias"] = _ln_backward(g, tape["ln_in"], P["ln.weight"])
    return grads


# ---- the loss ------------------------------------------------------------------------------------------------------------
def _side(C, eps, eps_abs, alpha, cond_reg):
    d = C.shape[0]
    tr = np.trace(C)
    clamped = not tr >= FLOOR
    mu = max(tr, FLOOR) / d
    ridge = max(mu * eps, mu * eps_abs)
    A = (1.0 - alpha) * C + (alpha * mu + ridge) * np.eye(d)
    A = 0.5 * (A + A.T)
    w, V = np.linalg.eigh(A)
    lmin, lmax = max(w[0], FLOOR), max(w[-1], FLOOR)
    cond = lmax / lmin
    pen = np.zeros((d, d))
    if cond > 1.0:
        if w[-1] > FLOOR:
            pen += cond_reg * np.outer(V[:, -1], V[:, -1]) / w[-1]
        if w[0] > FLOOR:
            pen -= cond_reg * np.outer(V[:, 0], V[:, 0]) / w[0]
    total, jitter, L = 0.0, 1e-8, None
    for _ in range(5):
        try:
            L = np.linalg.cholesky(A + total * np.eye(d))
            break
        except np.linalg.LinAlgError:
            total += jitter
            jitter *= 10.0
    if L is None:
        raise RuntimeError("Cholesky decomposition failed after retries")
    c = 0.0 if clamped else alpha + ridge / mu
    return A + total * np.eye(d), L, cond, lmin, lmax, pen, c


def vamp2(Y0, Yt, eps=1e-3, eps_abs=1e-6, alpha=0.15, cond_reg=1e-4):
    """loss, score, the ten metrics, dL/dY0, dL/dYt."""
    Y0, Yt = np.asarray(Y0, np.float64), np.asarray(Yt, np.float64)
    m, d = Y0.shape
    eps_abs, alpha, cond_reg = max(eps_abs, 0.0), min(max(alpha, 0.0), 1.0), max(cond_reg, 0.0)
    m0, mt = Y0.mean(axis=0), Yt.mean(axis=0)
    A0, At = Y0 - m0, Yt - mt
    C00, Ctt, C0t = A0.T @ A0 / m, At.T @ At / m, A0.T @ At / m
    A, LA, cond0, min0, max0, penA, cA = _side(C00, eps, eps_abs, alpha, cond_reg)
    B, LB, condt, mint, maxt, penB, cB = _side(Ctt, eps, eps_abs, alpha, cond_reg)
    Ai, Bi = np.linalg.inv(A), np.linalg.inv(B)
    K = np.linalg.solve(LB, np.linalg.solve(LA, C0t).T).T
    score = float(np.sum(K * K))
    penalty = cond_reg * (np.log(max(cond0, 1.0)) + np.log(max(condt, 1.0))) if cond_reg > 0 else 0.0
    GA = Ai @ C0t @ Bi @ C0t.T @ Ai + penA
    GB = Bi @ C0t.T @ Ai @ C0t @ Bi + penB
    G0t = -2.0 * Ai @ C0t @ Bi
    G00 = (1.0 - alpha) * GA + cA / d * np.trace(GA) * np.eye(d)
    Gtt = (1.0 - alpha) * GB + cB / d * np.trace(GB) * np.eye(d)
    g0 = (2.0 * A0 @ G00 + At @ G0t.T) / m
    gt = (2.0 * At @ Gtt + A0 @ G0t) / m
    # the size of the two terms each gradient is the sum of: what "the largest entry" means when they cancel
    term_scale = float(max(np.max(np.abs(2.0 * A0 @ G00)), np.max(np.abs(At @ G0t.T)), np.max(np.abs(2.0 * At @ Gtt)),
                           np.max(np.abs(A0 @ G0t))) / m)
    metrics = {"cond_C00": cond0, "cond_Ctt": condt, "var_z0": np.diag(C00).tolist(), "var_zt": np.diag(Ctt).tolist(),
               "mean_z0": m0.tolist(), "mean_zt": mt.tolist(), "eig_C00_min": min0, "eig_C00_max": max0,
               "eig_Ctt_min": mint, "eig_Ctt_max": maxt}
    return {"loss": -score + penalty, "score": score, "metrics": metrics, "grad0": g0, "grad_t": gt,
            "term_scale": term_scale}


def loss_grad(name, X, idx_t, idx_tau, packed=None, dropout=None, seed=0, step=0, opts=None, head_activation=None,
              masks=None):
    """The whole of msm_mlp_loss_grad for a case: vamp2's dict plus `outputs` [2m, n_out] and `grad` (packed, fp64)
    with `grads` (by key).  name: a case of R.CASES, or the case itself (a dict with config, params, mean, std as
    R.recipe makes them); head_activation: as in R.forward."""
    c = R.case(name) if isinstance(name, str) else name
    F = np.asarray(X).shape[1]
    params = c["params"] if packed is None else unpack(c["config"], F, np.asarray(packed, np.float32))
    Y, tape = forward_train(c["config"], params, c["mean"], c["std"], X, idx_t, idx_tau, dropout, seed, step,
                            head_activation, masks)
    m = len(idx_t)
    res = vamp2(Y[:m], Y[m:], **(opts or LOSS_OPTS))
    grads = backward(c["config"], params, F, tape, np.concatenate([res["grad0"], res["grad_t"]]))
    res["outputs"], res["grads"] = Y, grads
    res["grad"] = np.concatenate([grads[k].reshape(-1) for k, _ in R.key_layout(c["config"], F)])
    return res


# ---- clip + AdamW ----------------------------------------------------------------------------------------------------------
def adamw(p32, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, wd=1e-2, clip=None):
    """(p fp32, m, v, norm, norm after the clip, skipped).  A non-finite norm leaves everything as it is."""
    g = np.asarray(g, np.float64)
    norm = float(np.sqrt(np.sum(g * g)))
    if not np.isfinite(norm):
        return p32.copy(), m.copy(), v.copy(), norm, norm, True
    coef = min(1.0, clip / (norm + 1e-6)) if clip is not None and clip > 0 else 1.0
    g = g * coef
    m = betas[0] * m + (1.0 - betas[0]) * g
    v = betas[1] * v + (1.0 - betas[1]) * (g * g)
    p = p32.astype(np.float64) * (1.0 - lr * wd)
    p = p - (lr / (1.0 - betas[0] ** step)) * (m / (np.sqrt(v) / np.sqrt(1.0 - betas[1] ** step) + eps))
    return p.astype(np.float32), m, v, norm, norm * coef, False


def ulp32(p) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(p, np.float32)))


# ---- the toy data set of the trainer test ----------------------------------------------------------------------------------
TOY_CONFIG = {"lag": 5, "n_out": 2, "hidden": [16, 8], "activation": "tanh", "layer_norm_in": False, "layer_norm_hidden": False,
              "linear_head": False, "dropout": 0.0, "hidden_dropout": []}
TOY_TRAINER = {"tau_schedule": (2, 5), "val_tau": 5, "epochs_per_tau": 3, "warmup_epochs": 1, "learning_rate": 1e-2,
               "batch_size": 256}
TOY_SEEDS = (0, 1, 2)


def toy_sequence() -> np.ndarray:
    """2000 frames [2000, 7] float32 of a two-state hopping chain (flip probability 0.02) pushed through sines and
    squares into 7 noisy features.  One data set; TOY_SEEDS are the seeds of the initialisation and the shuffling."""
    rng = np.random.default_rng(7000)
    state = np.cumsum(rng.random(2000) < 0.02) % 2
    s = (2.0 * state - 1.0) + 0.25 * rng.normal(size=2000)
    cols = [np.sin((0.6 + 0.3 * k) * s + 0.5 * k) for k in range(4)] + [(s + 0.4 * k - 0.3) ** 2 for k in range(3)]
    X = np.stack(cols, axis=1) + 0.3 * rng.normal(size=(2000, 7))
    return X.astype(np.float32)
