"""The bias-potential law in numpy: host-only companion of tests/test_bias_host.py and tests/test_gpu_bias.py.

Restated here (no product code, no torch), as include/msmhip.h states it for msm_featurize_spec_vjp, msm_mlp_vjp and
msm_bias_energy_forces:

table_from_spec   the record table of a canonical feature specification (records by kind, columns = positions)
incidence         the atom -> (record, slot) incidence in CSR form, entries record * 4 + slot ascending per atom
bond_vectors      the fp32 bond vectors of every record, flagged ones replaced by their minimum image in the
                  device's fp32 operation order (rule "round": tests/_pbc_ref.round_image; rule "search": the 27
                  images in the device's order, lowest index on a tie)
featurize_vjp     the featurizer's adjoint: closed-form Jacobians on those vectors widened to `dtype` (float64: what
                  the device is held to; longdouble: the yardstick of its rounding), zero where the forward's floor,
                  clamp or mask is active, summed per atom in ascending (record, slot) order
features          the forward on the same records in fp32 (through tests/_pbc_ref's geometry) or all in fp64
mlp_vjp           evaluation-mode forward of the network with its tape, then the adjoints of
                  tests/_deeptica_train_ref.backward carried on to the inputs: dE/dx = dZ / scale
energy_forces     the chain: E = strength sum y^2, CVs, F = -dE/dx
energy64          the same energy with nothing rounded to fp32: the function whose central differences the forces are
                  checked against

Every `*_vjp` also returns, per output, the sum of the absolute values of the terms it adds up: the scale a rounding
error is measured in."""

from __future__ import annotations

import numpy as np

from tests import _deeptica_ref as R
from tests import _deeptica_train_ref as T
from tests import _pbc_ref as P

DISTANCE, ANGLE, DIHEDRAL, CONTACT = range(4)
MIC, COSSIN = 1, 2
N_ATOMS = {DISTANCE: 2, ANGLE: 3, DIHEDRAL: 4, CONTACT: 2}
EPS = 1.0e-12
ACTIVATIONS = ("tanh", "gelu", "relu", "elu", "selu", "leaky_relu")


# ---- tables ------------------------------------------------------------------------------------------------------
def table_from_spec(spec):
    """(rec int32 [F, 8], param float32 [F], width): distances, angles, dihedrals, each at its position."""
    w = np.asarray(spec.feature_weights, np.float32)
    rows, par = [], []
    for kind, atoms, pos, pbc in ((DISTANCE, spec.distance_pairs, spec.distance_positions, spec.distance_pbc),
                                  (ANGLE, spec.angle_triplets, spec.angle_positions, spec.angle_pbc),
                                  (DIHEDRAL, spec.dihedral_quads, spec.dihedral_positions, spec.dihedral_pbc)):
        for a, p, f in zip(np.asarray(atoms), np.asarray(pos), np.asarray(pbc)):
            r = [kind, 0, 0, 0, 0, MIC if f else 0, int(p), 0]
            r[1:1 + len(a)] = [int(v) for v in a]
            rows.append(r)
            par.append(w[int(p)])
    return np.asarray(rows, np.int32).reshape(-1, 8), np.asarray(par, np.float32), int(w.size)


def incidence(rec, n_atoms: int):
    """(ptr int32 [A + 1], entries int32 [nnz]): atom a's entries are entries[ptr[a]:ptr[a + 1]], each
    record * 4 + slot, ascending.  Contacts (no gradient) and atoms outside [0, A) are not listed."""
    lists = [[] for _ in range(n_atoms)]
    for f, r in enumerate(np.asarray(rec)):
        kind = int(r[0])
        if kind in (DISTANCE, ANGLE, DIHEDRAL):
            for s in range(N_ATOMS[kind]):
                if 0 <= int(r[1 + s]) < n_atoms:
                    lists[int(r[1 + s])].append(4 * f + s)
    ptr = np.zeros(n_atoms + 1, np.int32)
    ptr[1:] = np.cumsum([len(v) for v in lists])
    return ptr, np.asarray([e for v in lists for e in v], np.int32)


# ---- bond vectors, fp32 ------------------------------------------------------------------------------------------
def _search_image(v, b):
    """The device's rule "search" in fp32: v [n, 3], b [n, 3, 3]."""
    one = np.float32
    r = P.round_image(v[:, None, :], b)[:, 0]
    inv = P.inverse_adjugate(b)
    col = [inv[:, 0, j] * inv[:, 0, j] + inv[:, 1, j] * inv[:, 1, j] + inv[:, 2, j] * inv[:, 2, j] for j in range(3)]
    radius = one(0.2401) / np.maximum(col[0], np.maximum(col[1], col[2]))
    best, best_d = r.copy(), np.full(r.shape[0], np.inf, np.float32)
    for idx in range(27):
        i, j, k = one(idx // 9 - 1), one((idx // 3) % 3 - 1), one(idx % 3 - 1)
        c = r + (i * b[:, 0, :] + j * b[:, 1, :] + k * b[:, 2, :]) if idx != 13 else r
        d = P._dot(c, c)
        take = d < best_d
        best[take], best_d[take] = c[take], d[take]
    near = P._dot(r, r) < radius
    best[near] = r[near]
    return best


def bond_vectors(rec, xyz, box=None, mic: str = "round"):
    """Per record the list of its bond vectors, float32 [n, 3] each, in the forward kernel's sign conventions."""
    x = np.asarray(xyz, np.float32)
    n = x.shape[0]
    b = None if box is None else np.ascontiguousarray(P._boxes(box, n, np.float32))
    wrap = (lambda v: P.round_image(v[:, None, :], b)[:, 0]) if mic == "round" else (lambda v: _search_image(v, b))
    out = []
    for r in np.asarray(rec):
        kind, i0, i1, i2, i3, flags = (int(v) for v in r[:6])
        if kind in (DISTANCE, CONTACT):
            vs = [x[:, i1] - x[:, i0]]
        elif kind == ANGLE:
            vs = [x[:, i0] - x[:, i1], x[:, i2] - x[:, i1]]
        else:
            vs = [x[:, i1] - x[:, i0], x[:, i2] - x[:, i1], x[:, i3] - x[:, i2]]
        if b is not None and flags & MIC:
            vs = [wrap(v) for v in vs]
        out.append(vs)
    return out


# ---- the featurizer's Jacobians ----------------------------------------------------------------------------------
def _jacobian(kind: int, vs, dtype):
    """(d value / d x_slot for every slot [n, 3], live [n] bool, cos, sin): `live` is False where the forward's
    floor, clamp or mask is active; cos / sin of a dihedral for the COSSIN chain rule."""
    eps = dtype(EPS)
    vs = [np.asarray(v, dtype) for v in vs]
    if kind == DISTANCE:
        q = P._dot(vs[0], vs[0])
        live = ~(q <= eps)
        j = vs[0] / np.sqrt(np.where(live, q, 1))[:, None]
        return [-j, j], live, None, None
    if kind == ANGLE:
        v1, v2 = vs
        q1, q2 = P._dot(v1, v1), P._dot(v2, v2)
        w = P._cross(v1, v2)
        ww = P._dot(w, w)
        c = P._dot(v1, v2) / (np.sqrt(np.maximum(q1, eps)) * np.sqrt(np.maximum(q2, eps)))
        live = ~((q1 <= eps) | (q2 <= eps) | (np.abs(c) >= 1) | (ww <= 0))
        nw = np.sqrt(np.where(live, ww, 1))
        g1 = P._cross(v1, w) / (np.where(live, q1, 1) * nw)[:, None]
        g2 = -P._cross(v2, w) / (np.where(live, q2, 1) * nw)[:, None]
        return [g1, -(g1 + g2), g2], live, None, None
    b0, b1, b2 = vs
    c0, c1 = P._cross(b0, b1), P._cross(b1, b2)
    q0, q1, qb = P._dot(c0, c0), P._dot(c1, c1), P._dot(b1, b1)
    live = ~((q0 <= eps) | (q1 <= eps) | (qb <= eps))
    s0, s1, sb = (np.where(live, q, 1) for q in (q0, q1, qb))
    nb = np.sqrt(sb)
    u0, u1 = c0 / np.sqrt(s0)[:, None], c1 / np.sqrt(s1)[:, None]
    x, y = P._dot(u0, u1), P._dot(P._cross(u0, u1), b1 / nb[:, None])
    live = live & ~((np.abs(x) + np.abs(y)) < eps)
    r = np.sqrt(np.where(live, x * x + y * y, 1))
    f1, f4 = -(nb / s0)[:, None] * c0, (nb / s1)[:, None] * c1
    s01, s21 = (P._dot(b0, b1) / sb)[:, None], (P._dot(b2, b1) / sb)[:, None]
    return [f1, -f1 - s01 * f1 + s21 * f4, -f4 + s01 * f1 - s21 * f4, f4], live, x / r, y / r


def featurize_vjp(rec, param, xyz, gfeat, box=None, mic="round", sign=1.0, col_off=0, width=None, dtype=np.float64):
    """(gxyz [n, A, 3], scale [n, A, 3]) in `dtype`: sign * sum_f gfeat[t, col(f)] d feature_f / d x_a, and the sum
    of the absolute terms.  A frame whose gradient block holds a non-finite value is NaN on all its atoms."""
    dtype = np.dtype(dtype).type
    rec = np.asarray(rec)
    x = np.asarray(xyz, np.float32)
    n, A = x.shape[:2]
    g = np.asarray(gfeat, dtype)
    width = int(rec[:, 6:8].max()) + 1 if width is None else int(width)
    out, scale = np.zeros((n, A, 3), dtype), np.zeros((n, A, 3), dtype)
    for r, par, vs in zip(rec, np.asarray(param, np.float32), bond_vectors(rec, x, box, mic)):
        kind, flags, col, col2 = int(r[0]), int(r[5]), int(r[6]), int(r[7])
        trig = kind == DIHEDRAL and bool(flags & COSSIN)
        atoms = [int(a) for a in r[1:1 + N_ATOMS.get(kind, 0)]]
        if kind not in (DISTANCE, ANGLE, DIHEDRAL) or not 0 <= col < width or (trig and not 0 <= col2 < width):
            continue
        if any(not 0 <= a < A for a in atoms):
            continue
        jac, live, cos, sin = _jacobian(kind, vs, dtype)
        coef = g[:, col_off + col]
        if trig:
            coef = coef * -sin + g[:, col_off + col2] * cos
        coef = coef * dtype(par)
        for a, j in zip(atoms, jac):
            term = np.where(live[:, None], coef[:, None] * j, 0)
            out[:, a] += term
            scale[:, a] += np.abs(term)
    bad = ~np.isfinite(g[:, col_off:col_off + width]).all(axis=1)
    out = dtype(sign) * out
    out[bad] = np.nan
    return out, scale


def features(rec, param, xyz, box=None, mic="round", dtype=np.float32):
    """[n, width]: the forward on the records.  fp32: the fp32 vectors through tests/_pbc_ref's geometry (the
    device's arithmetic); fp64: the same vectors widened, all later arithmetic fp64."""
    dtype = np.dtype(dtype).type
    rec = np.asarray(rec)
    x = np.asarray(xyz, np.float32)
    out = np.zeros((x.shape[0], int(rec[:, 6:8].max()) + 1), dtype)
    names = {DISTANCE: "distance", ANGLE: "angle", DIHEDRAL: "dihedral"}
    for r, par, vs in zip(rec, np.asarray(param, np.float32), bond_vectors(rec, x, box, mic)):
        kind, flags, col, col2 = int(r[0]), int(r[5]), int(r[6]), int(r[7])
        if kind == CONTACT:
            out[:, col] = (P._geometry("distance", [v[:, None].astype(dtype) for v in vs], dtype)[:, 0] <= dtype(par))
            continue
        val = P._geometry(names[kind], [v[:, None].astype(dtype) for v in vs], dtype)[:, 0]
        if kind == DIHEDRAL and flags & COSSIN:
            out[:, col], out[:, col2] = np.cos(val) * dtype(par), np.sin(val) * dtype(par)
        else:
            out[:, col] = val * dtype(par)
    return out


# ---- the network ---------------------------------------------------------------------------------------------------
def network(widths, activation, ln_in, ln_hidden, head_activation, packed, mean=None, scale=None) -> dict:
    """A network as the device sees it: widths, activation code, flags, the packed fp32 parameters, the scaler."""
    return {"widths": tuple(int(w) for w in widths), "activation": int(activation), "ln_in": bool(ln_in),
            "ln_hidden": bool(ln_hidden), "head_activation": bool(head_activation),
            "params": np.asarray(packed, np.float32).reshape(-1),
            "mean": None if mean is None else np.asarray(mean, np.float64),
            "scale": None if scale is None else np.asarray(scale, np.float64)}


def _unpack(net):
    w, p, off = net["widths"], net["params"], 0

    def take(*shape):
        nonlocal off
        size = int(np.prod(shape))
        out = p[off:off + size].reshape(shape)
        off += size
        return out

    ln = (take(w[0]), take(w[0])) if net["ln_in"] else None
    layers = []
    for i in range(len(w) - 1):
        W, b = take(w[i + 1], w[i]), take(w[i + 1])
        norm = (take(w[i + 1]), take(w[i + 1])) if net["ln_hidden"] and i + 2 < len(w) else None
        layers.append((W, b, norm))
    assert off == p.size
    return ln, layers


def _ln_backward_abs(dy, cache, gamma):
    xhat, rstd = cache
    d = np.abs(dy * gamma)
    return rstd * (d + d.mean(axis=1, keepdims=True) + np.abs(xhat) * (d * np.abs(xhat)).mean(axis=1, keepdims=True))


def mlp_vjp(net, X, gout=None, strength=1.0, dtype=np.float64, round_z=True):
    """(energy [n], y [n, n_out], gx [n, F], scale [n, F]) in `dtype`.  gout None: the upstream gradient is
    2 strength y.  round_z False: Z is not rounded to fp32 (energy64's network)."""
    dtype = np.dtype(dtype).type
    act, dact = T._act(ACTIVATIONS[net["activation"]])
    if dtype is np.longdouble:       # scipy's erf is fp64: only tanh networks have a longdouble yardstick
        assert net["activation"] == 0
    ln, layers = _unpack(net)
    cast = lambda a: np.asarray(a, dtype)      # noqa: E731
    Z = np.asarray(X, np.float64)
    if net["mean"] is not None:
        Z = (Z - net["mean"]) / net["scale"]
    x = cast(Z.astype(np.float32)) if round_z else cast(Z)
    tape = []
    ln_cache = None
    if ln is not None:
        x, ln_cache = T._ln_forward(x, cast(ln[0]), cast(ln[1]))
    for i, (W, b, norm) in enumerate(layers):
        rec = {}
        x = x @ cast(W).T + cast(b)
        last = i == len(layers) - 1
        if norm is not None:
            x, rec["ln"] = T._ln_forward(x, cast(norm[0]), cast(norm[1]))
        if not last or net["head_activation"]:
            rec["h"] = x
            x = act(x)
        tape.append(rec)
    y = x
    energy = dtype(strength) * (y * y).sum(axis=1)
    g = dtype(2.0) * dtype(strength) * y if gout is None else cast(gout)
    s = np.abs(g)
    for i in reversed(range(len(layers))):
        W, _b, norm = layers[i]
        rec = tape[i]
        if "h" in rec:
            d = dact(rec["h"])
            g, s = g * d, s * np.abs(d)
        if norm is not None:
            s = _ln_backward_abs(s, rec["ln"], cast(norm[0]))
            g = T._ln_backward(g, rec["ln"], cast(norm[0]))[0]
        g, s = g @ cast(W), s @ np.abs(cast(W))
    if ln is not None:
        s = _ln_backward_abs(s, ln_cache, cast(ln[0]))
        g = T._ln_backward(g, ln_cache, cast(ln[0]))[0]
    if net["scale"] is not None:
        g, s = g / cast(net["scale"]), s / np.abs(cast(net["scale"]))
    return energy, y, g, s


# the two golden networks, 23 -> 32 -> 16 -> 3: configs in the reference's fields, parameters from a seed
NETWORKS = {
    "tanh": {"lag": 5, "n_out": 3, "hidden": [32, 16], "activation": "tanh", "layer_norm_in": False,
             "layer_norm_hidden": False, "linear_head": False, "hidden_dropout": []},
    "ln_gelu": {"lag": 5, "n_out": 3, "hidden": [32, 16], "activation": "gelu", "layer_norm_in": True,
                "layer_norm_hidden": True, "linear_head": False, "hidden_dropout": []},
}
# networks of the adjoint-alone tests: the longdouble yardstick wants tanh (scipy's erf is fp64)
ADJOINT_NETWORKS = {"tanh": NETWORKS["tanh"], "ln_tanh": {**NETWORKS["ln_gelu"], "activation": "tanh"},
                    "ln_gelu": NETWORKS["ln_gelu"]}
_SEEDS = {"tanh": 2310, "ln_gelu": 2311, "ln_tanh": 2312}
N_FEATURES = 23


def network_params(name: str) -> dict:
    """{state_dict key: fp32 array} of a golden network, drawn as tests/_deeptica_ref.recipe draws its cases
    (LayerNorm gamma / beta well off (1, 0)); nothing of it is stored."""
    config = ADJOINT_NETWORKS[name]
    rng = np.random.default_rng(_SEEDS[name])
    params = {}
    for key, shape in R.key_layout(config, N_FEATURES):
        if len(shape) == 2:
            v = rng.normal(size=shape) * (1.3 / np.sqrt(shape[1]))
        elif key.endswith("weight"):
            v = rng.uniform(0.4, 1.7, size=shape) * rng.choice([-1.0, 1.0], size=shape)
        elif key.startswith("ln.") or params[key.replace("bias", "weight")].ndim == 1:
            v = rng.normal(size=shape) * 0.6
        else:
            v = rng.normal(size=shape) * 0.3
        params[key] = v.astype(np.float32)
    return params


def golden_network(name: str, mean, scale) -> dict:
    """A golden network as `network` describes it, with the given scaler."""
    config, params = ADJOINT_NETWORKS[name], network_params(name)
    packed = np.concatenate([params[k].reshape(-1) for k, _ in R.key_layout(config, N_FEATURES)])
    return network((N_FEATURES, 32, 16, 3), ACTIVATIONS.index(config["activation"]), config["layer_norm_in"],
                   config["layer_norm_hidden"], not config["linear_head"], packed, mean, scale)


adjoint_network = golden_network


# ---- the chain -------------------------------------------------------------------------------------------------------
def energy_forces(rec, param, net, xyz, box=None, mic="round", strength=10.0):
    """(E [n], cv [n, n_out], F [n, A, 3]) as the device computes them: fp32 features, Z rounded to fp32, fp64 after."""
    feats = features(rec, param, xyz, box, mic, np.float32)
    energy, y, gx, _ = mlp_vjp(net, feats, None, strength)
    force, _ = featurize_vjp(rec, param, xyz, gx, box, mic, sign=-1.0, width=feats.shape[1])
    return energy, y, force


def energy64(rec, param, net, xyz64, box=None, strength=10.0):
    """E [n] with every step in fp64 on fp64 coordinates [n, A, 3] (no box, or rule "round" through tests/_pbc_ref):
    a smooth function of the coordinates away from the minimum-image ties."""
    x = np.asarray(xyz64, np.float64)
    n = x.shape[0]
    rec = np.asarray(rec)
    b = None if box is None else np.ascontiguousarray(P._boxes(box, n, np.float64))
    feats = np.zeros((n, int(rec[:, 6:8].max()) + 1))
    names = {DISTANCE: "distance", ANGLE: "angle", DIHEDRAL: "dihedral"}
    for r, par in zip(rec, np.asarray(param, np.float64)):
        kind, i0, i1, i2, i3, flags, col = (int(v) for v in r[:7])
        if kind == DISTANCE:
            vs = [x[:, i1] - x[:, i0]]
        elif kind == ANGLE:
            vs = [x[:, i0] - x[:, i1], x[:, i2] - x[:, i1]]
        else:
            vs = [x[:, i1] - x[:, i0], x[:, i2] - x[:, i1], x[:, i3] - x[:, i2]]
        if b is not None and flags & MIC:
            vs = [P.round_image(v[:, None, :], b)[:, 0] for v in vs]
        feats[:, col] = P._geometry(names[kind], [v[:, None] for v in vs], np.float64)[:, 0] * par
    return mlp_vjp(net, feats, None, strength, round_z=False)[0]
