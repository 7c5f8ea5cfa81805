"""The weighted VAMP-2 law in fp64 numpy, and the seeded recipes of the weighted test cases.

The law is that of msm_vamp2_loss_weighted in include/msmhip.h (VAMP2Loss.forward(z0, zt, weights) of the
reference): clamp the weights at 0, normalise them, weighted means and weighted centred covariances with correction
0, then the unweighted law from the regularisation on (tests/_deeptica_train_ref._side, shared, not restated), and
the closed-form output gradient what_s (2 (y0_s - mu0) G00 + (yt_s - mut) G0t') and its mirror.
tests/test_deeptica_weighted_reference.py pins this module against the reference's recorded loss, metrics and
autograd gradients (tests/golden/deeptica_weighted.*); the GPU tests compare the device against both.

Loss cases: the outputs of T.loss_case(1), (2), (3) -- (37, 3), (125, 17), (250, 64) -- and two shapes more by the
same recipe: (257, 5), two chunks of 256 pairs with a tail of one, and (600, 33), three chunks and three 16-wide tiles
per side with a tail tile of one.  Weight patterns: log-normal with sigma 1.5; the same rounded to float32; every
third pair 0 and one negative; and at (600, 33) a whole chunk, pairs 256..511, of zeros.  Every case keeps at least
n_out + 2 positive weights (with fewer the closed form and autograd part ways: the smallest eigenvalue is tied).
Nothing of them is stored."""

from __future__ import annotations

import zlib

import numpy as np

from tests import _deeptica_ref as R
from tests import _deeptica_train_ref as T

EXTRA_SHAPES = {"s257": (257, 5, 0.15, 1e-4), "s600": (600, 33, 0.15, 0.05)}
SHAPE_KEYS = ("t1", "t2", "t3", "s257", "s600")
PATTERNS = ("lognormal", "float32", "zeros")
LOSS_CASES = [(s, p) for s in SHAPE_KEYS for p in PATTERNS] + [("s600", "chunk")]
NET_CASES = ("one", "wide")


def loss_case(shape_key: str):
    """(Y0, Yt, opts) of a shape: T.loss_case's for t1..t3, the same recipe under other seeds for the two new ones."""
    if shape_key in ("t1", "t2", "t3"):
        return T.loss_case(int(shape_key[1]))
    m, d, alpha, cond_reg = EXTRA_SHAPES[shape_key]
    rng = np.random.default_rng(zlib.crc32(("weighted:" + shape_key).encode()))
    base = rng.normal(size=(m, d))
    mix = rng.normal(size=(d, d)) / np.sqrt(d) + np.eye(d)
    scale = rng.uniform(0.3, 3.0, size=d)
    Y0 = (base @ mix) * scale + rng.normal(size=d)
    Yt = (0.7 * base + 0.5 * rng.normal(size=(m, d))) @ mix * scale + rng.normal(size=d)
    return Y0, Yt, {"eps": 1e-3, "eps_abs": 1e-6, "alpha": alpha, "cond_reg": cond_reg}


def weights(tag: str, m: int, pattern: str) -> np.ndarray:
    """[m] float64 weights of a pattern; `tag` names the case the draw belongs to."""
    rng = np.random.default_rng(zlib.crc32(("weights:" + tag).encode()))
    w = np.exp(1.5 * rng.normal(size=m))
    if pattern == "lognormal":
        return w
    if pattern == "float32":
        return w.astype(np.float32).astype(np.float64)
    if pattern == "zeros":
        w[::3] = 0.0
        w[1] = -0.7
        return w
    if pattern == "chunk":
        w[256:512] = 0.0
        return w
    raise KeyError(pattern)


def case(shape_key: str, pattern: str):
    Y0, Yt, opts = loss_case(shape_key)
    return Y0, Yt, weights(shape_key, Y0.shape[0], pattern), opts


def vamp2_weighted(Y0, Yt, w, eps=1e-3, eps_abs=1e-6, alpha=0.15, cond_reg=1e-4):
    """T.vamp2's dict under per-pair weights, plus total_weight and effective_pairs."""
    Y0, Yt = np.asarray(Y0, np.float64), np.asarray(Yt, np.float64)
    d = Y0.shape[1]
    eps_abs, alpha, cond_reg = max(eps_abs, 0.0), min(max(alpha, 0.0), 1.0), max(cond_reg, 0.0)
    wc = np.clip(np.asarray(w, np.float64).reshape(-1), 0.0, None)
    W = float(wc.sum())
    if not (np.all(np.isfinite(wc)) and W > 0.0 and np.isfinite(W)):
        raise ValueError("weights must be finite and sum to a positive number")
    wh = (wc / W)[:, None]
    m0, mt = (wh * Y0).sum(axis=0), (wh * Yt).sum(axis=0)
    A0, At = Y0 - m0, Yt - mt
    C00, Ctt, C0t = A0.T @ (wh * A0), At.T @ (wh * At), A0.T @ (wh * At)
    A, LA, cond0, min0, max0, penA, cA = T._side(C00, eps, eps_abs, alpha, cond_reg)
    B, LB, condt, mint, maxt, penB, cB = T._side(Ctt, eps, eps_abs, alpha, cond_reg)
    Ai, Bi = np.linalg.inv(A), np.linalg.inv(B)
    K = np.linalg.solve(LB, np.linalg.solve(LA, C0t).T).T
    score = float(np.sum(K * K))
    penalty = cond_reg * (np.log(max(cond0, 1.0)) + np.log(max(condt, 1.0))) if cond_reg > 0 else 0.0
    GA = Ai @ C0t @ Bi @ C0t.T @ Ai + penA
    GB = Bi @ C0t.T @ Ai @ C0t @ Bi + penB
    G0t = -2.0 * Ai @ C0t @ Bi
    G00 = (1.0 - alpha) * GA + cA / d * np.trace(GA) * np.eye(d)
    Gtt = (1.0 - alpha) * GB + cB / d * np.trace(GB) * np.eye(d)
    parts = (2.0 * A0 @ G00, At @ G0t.T, 2.0 * At @ Gtt, A0 @ G0t)
    g0, gt = wh * (parts[0] + parts[1]), wh * (parts[2] + parts[3])
    term_scale = float(max(np.max(np.abs(wh * p)) for p in parts))
    metrics = {"cond_C00": cond0, "cond_Ctt": condt, "var_z0": np.diag(C00).tolist(), "var_zt": np.diag(Ctt).tolist(),
               "mean_z0": m0.tolist(), "mean_zt": mt.tolist(), "eig_C00_min": min0, "eig_C00_max": max0,
               "eig_Ctt_min": mint, "eig_Ctt_max": maxt}
    return {"loss": -score + penalty, "score": score, "metrics": metrics, "grad0": g0, "grad_t": gt,
            "term_scale": term_scale, "total_weight": W, "effective_pairs": W * W / float(np.sum(wc * wc))}


def net_weights(name: str, which: str = "a") -> np.ndarray:
    """Log-normal per-pair weights (sigma 1.5) of a network case's pair set."""
    return weights(f"{name}:{which}", len(T.pairs(name, which)[0]), "lognormal")


def loss_grad_weighted(name: str, X, idx_t, idx_tau, w, packed=None, dropout=None, seed=0, step=0, opts=None):
    """T.loss_grad with the weighted loss: the whole of msm_mlp_loss_grad_weighted for a case."""
    c = R.case(name)
    F = c["X"].shape[1]
    params = c["params"] if packed is None else T.unpack(c["config"], F, np.asarray(packed, np.float32))
    Y, tape = T.forward_train(c["config"], params, c["mean"], c["std"], X, idx_t, idx_tau, dropout, seed, step)
    m = len(idx_t)
    res = vamp2_weighted(Y[:m], Y[m:], w, **(opts or T.LOSS_OPTS))
    grads = T.backward(c["config"], params, F, tape, np.concatenate([res["grad0"], res["grad_t"]]))
    res["outputs"], res["grads"] = Y, grads
    res["grad"] = np.concatenate([grads[k].reshape(-1) for k, _ in R.key_layout(c["config"], F)])
    return res
