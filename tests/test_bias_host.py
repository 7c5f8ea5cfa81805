"""The bias potential without a device: the numpy restatement (tests/_bias_ref.py) against the reference's recorded
fp64 values (tests/golden/bias.*) and against central differences, the specification hash, the incidence builder, and
the host-side errors of CVBiasPotential.

Yardsticks.  bias.json records, per quantity, how far the restatement (fp32 features, Z rounded to fp32, fp64 after)
lies from the reference run in fp64: the restatement must reproduce that (1 % slack for another numpy's matmul).  The
all-fp64 energy of the restatement is the reference's fp64 energy up to rounding (1e-11 of the largest), so its
central differences (h = 1e-5 nm: truncation and cancellation both below 1e-6 of the largest force) are the fp64
forces, and the restatement's forces lie within the recorded force gap of them."""

from __future__ import annotations

import json

import numpy as np
import pytest

from pmarlo_amd.device import _table_from_spec, build_incidence
from pmarlo_amd.features.deeptica import (
    CVBiasPotential,
    DeepTICAModel,
    HarmonicExpansionBias,
    MLPSpec,
    create_cv_bias_potential,
    feature_spec_sha256,
)
from pmarlo_amd.features.deeptica.ts_feature_extractor import build_feature_extractor_module, canonicalize_feature_spec
from tests import _bias_ref as B
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLDEN / "bias.npz", allow_pickle=False)
    meta = json.loads((GOLDEN / "bias.json").read_text())
    raw = json.loads((GOLDEN / "pbc.json").read_text())["spec"]
    spec = canonicalize_feature_spec(raw)
    rec, param, _width = B.table_from_spec(spec)
    return g, meta, raw, spec, rec, param


def _box(g, case):
    return g[f"{case}_box"] if f"{case}_box" in g.files else None


@pytest.mark.parametrize("case", ["ortho", "tric", "nobox", "tric15"])
@pytest.mark.parametrize("net_name", list(B.NETWORKS))
def test_restatement_against_the_fp64_reference(gold, case, net_name):
    g, meta, _raw, _spec, rec, param = gold
    net = B.golden_network(net_name, g[f"{case}_mean"], g[f"{case}_scale"])
    E, cv, F = B.energy_forces(rec, param, net, g[f"{case}_xyz"], _box(g, case), "round", meta["strength"])
    key = f"{case}__{net_name}"
    for q, mine in (("energy", E), ("cv", cv), ("force", F)):
        want = g[f"{key}__{'E' if q == 'energy' else ('cv' if q == 'cv' else 'F')}64"]
        err, recorded = float(np.max(np.abs(mine - want))), meta["per_case"][key][q]["restatement_minus_ref64"]
        print(f"{key} {q}: |restatement - ref64| = {err:.3e}, recorded {recorded:.3e}")
        assert err <= 1.01 * recorded <= 1.01 * meta["gaps"]["restatement_minus_ref64"][q]
    if case == "tric15":
        assert not F[:, 12:].any()                       # unreferenced atoms: exact zeros


@pytest.mark.parametrize("case", ["ortho", "tric", "nobox"])
@pytest.mark.parametrize("net_name", list(B.NETWORKS))
def test_forces_against_central_differences(gold, case, net_name):
    g, meta, _raw, _spec, rec, param = gold
    k = meta["strength"]
    net = B.golden_network(net_name, g[f"{case}_mean"], g[f"{case}_scale"])
    xyz, box = g[f"{case}_xyz"][:4], (_box(g, case)[:4] if _box(g, case) is not None else None)
    E64 = B.energy64(rec, param, net, xyz.astype(np.float64), box, k)
    want_E = g[f"{case}__{net_name}__E64"][:4]
    assert np.max(np.abs(E64 - want_E)) <= 1e-11 * np.max(np.abs(want_E))
    _E, _cv, F = B.energy_forces(rec, param, net, xyz, box, "round", k)
    x64, h, fd = xyz.astype(np.float64), 1.0e-5, np.zeros(xyz.shape)
    for a in range(xyz.shape[1]):
        for c in range(3):
            xp, xm = x64.copy(), x64.copy()
            xp[:, a, c] += h
            xm[:, a, c] -= h
            fd[:, a, c] = -(B.energy64(rec, param, net, xp, box, k) - B.energy64(rec, param, net, xm, box, k)) / (2 * h)
    top = float(np.max(np.abs(fd)))
    err = float(np.max(np.abs(F - fd)))
    bound = meta["per_case"][f"{case}__{net_name}"]["force"]["restatement_minus_ref64"] + 1e-6 * top
    print(f"{case}/{net_name}: |F - central differences| = {err:.3e} of {top:.3g}, bound {bound:.3e}")
    assert err <= bound
    # and the differences are the reference's fp64 forces
    assert np.max(np.abs(fd - g[f"{case}__{net_name}__F64"][:4])) <= 1e-6 * top


def test_each_jacobian_against_central_differences():
    """One record of each kind (and the cos / sin pair): the closed forms are the derivatives of the forward, signs
    included.  Coordinates on a grid of 1/64 and a step of 1/1024 are exact in float32, and so are the bond vectors:
    the differences see truncation only (h^2 ~ 1e-6)."""
    rng = np.random.default_rng(5)
    x = (np.round(rng.normal(size=(6, 4, 3)) * 64.0) / 64.0).astype(np.float32)
    h = 1.0 / 1024.0
    for kind, flags, cols in ((B.DISTANCE, 0, (0, 0)), (B.ANGLE, 0, (0, 0)), (B.DIHEDRAL, 0, (0, 0)),
                              (B.DIHEDRAL, B.COSSIN, (0, 1))):
        rec = np.array([[kind, 0, 1, 2, 3, flags, *cols]], np.int32)
        par = np.array([1.5], np.float32)
        width = 2 if flags else 1
        g = rng.normal(size=(6, width))
        got, _ = B.featurize_vjp(rec, par, x, g, width=width)

        def value(xx):
            return (B.features(rec, par, xx, dtype=np.float64) * g).sum(axis=1)

        fd = np.zeros(x.shape)
        for a in range(4):
            for c in range(3):
                xp, xm = x.copy(), x.copy()
                xp[:, a, c] += np.float32(h)
                xm[:, a, c] -= np.float32(h)
                fd[:, a, c] = (value(xp) - value(xm)) / (2.0 * h)
        assert np.max(np.abs(got - fd)) <= 1e-4 * max(1.0, float(np.max(np.abs(got)))), (kind, flags)


def test_spec_hash_and_metadata(gold):
    _g, meta, raw, spec, _rec, _param = gold
    assert feature_spec_sha256(raw) == meta["feature_spec_sha256"]
    assert feature_spec_sha256({"features": np.arange(3), "k": np.float32(0.5)}) == feature_spec_sha256(
        {"k": 0.5, "features": [0, 1, 2]})
    ext = build_feature_extractor_module(spec)
    net = B.golden_network("tanh", np.zeros(23), np.ones(23))
    mlp = MLPSpec(net["widths"], net["activation"], net["ln_in"], net["ln_hidden"], net["head_activation"], net["params"])
    bias = create_cv_bias_potential(mlp, np.zeros(23), np.ones(23), feature_extractor=ext,
                                    feature_spec_hash=meta["feature_spec_sha256"], feature_names=list(spec.feature_names))
    assert bias.get_metadata() == {"bias_type": "harmonic_expansion", "bias_strength": 10.0,
                                   "feature_names": list(spec.feature_names), "n_features": 23,
                                   "cv_model_type": "MLPSpec", "feature_spec_sha256": meta["feature_spec_sha256"],
                                   "uses_pbc": True, "atom_count": 12}
    assert bytes(bias.feature_spec_hash_bytes()).decode("ascii") == meta["feature_spec_sha256"]
    assert bias.feature_spec_hash_bytes().dtype == np.uint8
    np.testing.assert_array_equal(HarmonicExpansionBias(2.0)([[1.0, 2.0], [0.0, 3.0]]), [10.0, 18.0])
    assert HarmonicExpansionBias().strength == 10.0


def test_incidence_builder(gold):
    _g, _meta, _raw, spec, rec, _param = gold
    table, _par, _w = _table_from_spec(spec)
    np.testing.assert_array_equal(table, rec)
    # a table with a contact, a repeated atom and an atom past A on top
    extra = np.array([[B.CONTACT, 0, 5, 0, 0, 0, 23, 0], [B.DISTANCE, 3, 3, 0, 0, 0, 24, 0],
                      [B.ANGLE, 1, 14, 2, 0, 0, 25, 0]], np.int32)
    for tab, A in ((rec, 12), (rec, 15), (np.concatenate([rec, extra]), 13), (rec[::-1].copy(), 12)):
        ptr, inc = build_incidence(tab, A)
        want_ptr, want_inc = B.incidence(tab, A)
        np.testing.assert_array_equal(ptr, want_ptr)
        np.testing.assert_array_equal(inc, want_inc)
        assert ptr.dtype == np.int32 and inc.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == inc.size
        seen = set()
        for a in range(A):
            mine = inc[ptr[a]:ptr[a + 1]]
            assert (np.diff(mine) > 0).all()                                  # ascending (record, slot)
            for code in mine:
                f, s = divmod(int(code), 4)
                assert tab[f, 0] != B.CONTACT and s < B.N_ATOMS[int(tab[f, 0])] and tab[f, 1 + s] == a
                seen.add(int(code))
        want = {4 * f + s for f in range(len(tab)) if tab[f, 0] != B.CONTACT
                for s in range(B.N_ATOMS[int(tab[f, 0])]) if tab[f, 1 + s] < A}
        assert seen == want and len(seen) == inc.size                        # every (record, slot) exactly once
    ptr, _inc = build_incidence(rec, 15)
    assert ptr[12] == ptr[13] == ptr[14] == ptr[15]                          # unreferenced atoms have none


def test_constructor_and_shape_errors_need_no_engine(gold, monkeypatch):
    _g, meta, _raw, spec, _rec, _param = gold
    import pmarlo_amd.device as device

    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")

    monkeypatch.setattr(device, "get_engine", no_engine)
    monkeypatch.setattr(device, "Engine", no_engine)
    ext = build_feature_extractor_module(spec)
    net = B.golden_network("ln_gelu", np.zeros(23), np.ones(23))
    mlp = MLPSpec(net["widths"], net["activation"], net["ln_in"], net["ln_hidden"], net["head_activation"], net["params"])
    kw = {"feature_extractor": ext, "feature_spec_hash": meta["feature_spec_sha256"]}
    with pytest.raises(ValueError, match="scaler_scale contains zero"):
        CVBiasPotential(mlp, np.zeros(23), np.r_[np.ones(22), 0.0], **kw)
    with pytest.raises(ValueError, match="unsupported bias type 'metadynamics'"):
        CVBiasPotential(mlp, np.zeros(23), np.ones(23), bias_type="metadynamics", **kw)
    with pytest.raises(TypeError, match="cv_model"):
        CVBiasPotential(object(), np.zeros(23), np.ones(23), **kw)
    with pytest.raises(TypeError, match="feature_extractor"):
        CVBiasPotential(mlp, np.zeros(23), np.ones(23), feature_extractor=object(), feature_spec_hash="x")
    with pytest.raises(ValueError, match="23 features but the scaler has 7"):
        CVBiasPotential(mlp, np.zeros(7), np.ones(7), **kw)
    config = dict(B.NETWORKS["ln_gelu"])
    model = DeepTICAModel.from_arrays(config, B.network_params("ln_gelu"), np.zeros(23), np.ones(23))
    bias = CVBiasPotential(model, np.zeros(23), np.ones(23), **kw)
    assert bias.get_metadata()["cv_model_type"] == "DeepTICAModel" and bias.spec.params.size == mlp.params.size
    box = np.eye(3)
    with pytest.raises(RuntimeError, match=r"positions tensor must have shape \(N, 3\)"):
        bias.forward(np.zeros((12, 2)), box)
    with pytest.raises(RuntimeError, match=r"positions tensor must have shape \(N, 3\)"):
        bias.compute_cvs(np.zeros(36), box)
    with pytest.raises(RuntimeError, match="expected at least 12 atoms, received 11"):
        bias.forward(np.zeros((11, 3)), box)
    with pytest.raises(RuntimeError, match="expected at least 12 atoms, received 5"):
        bias.energy_and_forces(np.zeros((4, 5, 3)), box)
    with pytest.raises(RuntimeError, match=r"box tensor must have shape \(3, 3\)"):
        bias.forward(np.zeros((12, 3)), np.eye(4))
    with pytest.raises(RuntimeError, match=r"box tensor must have shape \(3, 3\)"):
        bias.energy_and_forces(np.zeros((4, 12, 3)), np.zeros((3, 3, 3)))
