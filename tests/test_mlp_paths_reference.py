"""The law of the launch-path tests (tests/_mlp_paths_ref.py) checked against itself on the host: at every new
network and shape a second route that is identical in exact arithmetic -- features, hidden units and pairs permuted,
dropout masks carried along -- agrees with the first within 1e-12 of the largest entry of each tensor, two orders
under the 1e-10 that tests/test_gpu_mlp_paths.py holds the device to.  Every case that reaches the loss has cond C00
and cond Ctt <= 1e4.  CPU only; the second-trip shapes are taken at the nominal grid of a 256-CU device (the GPU test
takes them from the plan entry)."""

from __future__ import annotations

import numpy as np
import pytest

from tests import _deeptica_ref as R
from tests import _mlp_paths_ref as P

ROUTE = 1e-12
COND = 1e4
# rows of a second trip at 256 CUs: 2 workgroups per CU for edge256 (LDS alone), at most 8 for deep8 (LDS alone)
NOMINAL_TRIP = {"edge256": 16 * (256 * 2 + 1) + 5, "deep8": 16 * (256 * 8 + 1) + 5}


def test_the_networks_are_the_issue_s():
    assert {k: v[0] for k, v in P.NETS.items()} == {
        "deep8": (33, 17, 64, 65, 16, 15, 48, 5, 4), "edge256": (255, 256, 63, 64), "head_off": (7, 32, 16, 3),
        "thin": (1, 1, 2, 1)}
    assert not set(P.NETS) & set(R.CASES)
    assert len(P.case("deep8")["widths"]) - 1 == 8 and P.dropout_of("deep8") == [0.1, 0.1, 0.0, 0.2, 0.1, 0.0, 0.1, 0.0]
    assert P.dropout_of("edge256") == [0.1, 0.1, 0.1]
    head = P.case("head_off")
    assert not head["head_activation"] and len(head["widths"]) == 4 and not head["config"]["linear_head"]
    thin = P.case("thin")
    assert thin["config"]["layer_norm_in"] and thin["config"]["layer_norm_hidden"]
    assert P.case("deep8")["xdtype"] == np.float64 and P.case("edge256")["xdtype"] == np.float32
    for name in P.NETS:             # LayerNorm gamma / beta well away from (1, 0), parameters fp32, scaler not trivial
        c = P.case(name)
        assert all(v.dtype == np.float32 for v in c["params"].values())
        assert np.all(np.abs(c["mean"]) > 0) and np.all(c["std"] != 1.0)
        if c["config"]["layer_norm_in"]:
            assert np.all(np.abs(np.abs(c["params"]["ln.weight"]) - 1.0) > 0)
    assert P.case("odd")["params"] is R.case("odd")["params"]                   # R.CASES is read, not copied
    t, tau = P.pairs("deep8", 300, 400)
    assert np.unique(t).size < t.size and np.all(tau > t) and tau.max() < 400


def test_head_override_changes_no_existing_case():
    for name in R.CASES:
        c = R.case(name)
        explicit = R.forward(c["config"], c["params"], c["mean"], c["std"], c["X"],
                             head_activation=not c["config"].get("linear_head"))
        assert np.array_equal(explicit, c["raw"])
    c = P.case("head_off")
    X = P.frames("head_off", 17)
    on = R.forward(c["config"], c["params"], c["mean"], c["std"], X, head_activation=True)
    assert np.max(np.abs(on - P.forward(c, X))) > 1e-3                          # the override acts


@pytest.mark.parametrize("name", list(P.NETS))
def test_forward_and_vjp_routes_agree(name):
    c = P.case(name)
    sizes = P.SIZES + ((NOMINAL_TRIP[name],) if name in NOMINAL_TRIP else ())
    worst = {"outputs": 0.0, "energy": 0.0, "gx": 0.0, "restatements": 0.0}
    for n in sizes:
        X = P.frames(name, n)
        for gout in (None, P.upstream(name, n)):
            energy, y, gx = P.vjp(c, X, gout=gout, strength=2.5)
            # the forward of B.mlp_vjp against R.forward: two restatements of one law
            worst["restatements"] = max(worst["restatements"], P.rel(y, P.forward(c, X)))
            y2, energy2, gx2 = P.second_route_forward(c, X, gout=gout, strength=2.5, seed=n)
            for key, a, b in (("outputs", y2, y), ("energy", energy2, energy), ("gx", gx2, gx)):
                worst[key] = max(worst[key], P.rel(a, b))
        if name == "thin":          # a function of the LayerNorm betas alone: one row, and no gradient
            assert np.all(np.isfinite(y)) and np.all(y == y[0]) and np.all(gx == 0.0)
        else:
            assert np.unique(y, axis=0).shape[0] == n and np.max(np.abs(gx)) > 0.0
    print(f"{name}: route distance " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= ROUTE


def _loss_routes(name, m, n_frames, dropout):
    c = P.case(name)
    X = P.frames(name, n_frames)
    it, itau = P.pairs(name, m, n_frames)
    one = P.loss_grad(c, X, it, itau, dropout=dropout)
    two = P.second_route_loss_grad(c, X, it, itau, dropout=dropout, seed=m)
    dist = {"loss": abs(two["loss"] - one["loss"]) / abs(one["loss"]),
            "score": abs(two["score"] - one["score"]) / abs(one["score"]),
            "outputs": P.rel(two["outputs"], one["outputs"])}
    for key, scale in P.grad_scales(c, one).items():
        g = one["grads"][key]
        if scale == np.max(np.abs(g)):
            assert scale > 0.0, key
        else:                       # the bias of a linear head: an exact zero, measured in the size of its terms
            assert np.max(np.abs(g)) <= ROUTE * scale
        dist[key] = float(np.max(np.abs(two["grads"][key] - g))) / scale
    cond = max(one["metrics"]["cond_C00"], one["metrics"]["cond_Ctt"])
    worst = max(dist, key=dist.get)
    print(f"{name} m={m} dropout={'on' if dropout else 'off'}: cond {cond:.1f}; loss {dist['loss']:.1e}, score "
          f"{dist['score']:.1e}, outputs {dist['outputs']:.1e}, worst tensor {worst} {dist[worst]:.1e}")
    assert cond <= COND
    assert max(dist.values()) <= ROUTE
    return one


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("m", P.CHUNK_M)
@pytest.mark.parametrize("name", ["odd", "leaky", "deep8", "head_off"])
def test_chunk_boundary_routes_agree(name, m, drop):
    one = _loss_routes(name, m, m + 40, P.dropout_of(name) if drop else None)
    assert one["outputs"].shape[0] == 2 * m


@pytest.mark.parametrize("name", ["head_off", "deep8"])
def test_envelope_training_routes_agree(name):
    _loss_routes(name, 40, 80, None)
    _loss_routes(name, 40, 80, P.dropout_of(name))


def test_second_trip_training_routes_agree():
    rows = NOMINAL_TRIP["edge256"] + 1                  # 2m: the second-trip row count rounded up to even
    _loss_routes("edge256", rows // 2, 1500, P.dropout_of("edge256"))
