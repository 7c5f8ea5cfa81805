"""The bias potential on the device: msm_featurize_spec_vjp, msm_mlp_vjp and msm_bias_energy_forces through
Engine.featurize_spec_vjp / mlp_vjp / bias_energy_forces and CVBiasPotential, against the reference's recorded fp64
values (tests/golden/bias.*) and the numpy restatement (tests/_bias_ref.py).

Yardsticks, all recorded by tests/golden/make_golden_bias.py, none chosen here.
  * The chain (energy, CVs, forces) against the reference run in fp64: 4 x the recorded |restatement - ref64| per
    quantity (TOL).  The device differs from the restatement only by the rounding of acosf / atan2f inside the same
    error model (fp32 features, Z rounded to fp32); tests/test_gpu_pbc.py uses the same rule and the same factor.
  * Each adjoint alone against the restatement on identical inputs: 4 x the recorded |float64 - longdouble| of the
    restatement, in units of the sum of the absolute terms of each output: both sides are fp64
    evaluations of the same closed forms in the same order, and the longdouble run measures what fp64 rounding does
    to them.  The rule of tests/test_gpu_deeptica_train.py for parameter gradients (a fraction of the reference's own
    fp32 distance from the law) does not transfer to the network alone -- no fp32 reference of dE/dx of the bare
    network is recorded -- so the longdouble rule is used for the network too; its gelu variant has no longdouble
    yardstick (scipy's erf is fp64) and is held to the gap recorded for the tanh networks, LayerNorms included.
  * Energies of the network alone: two fp64 routes through sums of at most 71 terms, 1e-12 of the largest.
Where two device results must agree exactly, assert_array_equal."""

from __future__ import annotations

import json

import numpy as np
import pytest

from pmarlo_amd import _lib
from pmarlo_amd._lib import lib
from pmarlo_amd.device import FeatureTable
from pmarlo_amd.features.deeptica import CVBiasPotential, MLPSpec, feature_spec_sha256
from pmarlo_amd.features.deeptica.ts_feature_extractor import build_feature_extractor_module, canonicalize_feature_spec
from tests import _bias_ref as B
from tests import _pbc_ref as P
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = ("ortho", "tric", "nobox", "tric15")
CELLS = {"ortho": (2.0, 2.5, 3.0, 90.0, 90.0, 90.0), "tric": (2.4, 2.6, 2.9, 75.0, 98.0, 62.0)}
K = 10.0


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLDEN / "bias.npz", allow_pickle=False)
    meta = json.loads((GOLDEN / "bias.json").read_text())
    raw = json.loads((GOLDEN / "pbc.json").read_text())["spec"]
    spec = canonicalize_feature_spec(raw)
    rec, param, _width = B.table_from_spec(spec)
    assert meta["strength"] == K
    return g, meta, raw, spec, rec, param


@pytest.fixture(scope="module")
def tol(gold):
    gaps = gold[1]["gaps"]
    return ({q: 4.0 * v for q, v in gaps["restatement_minus_ref64"].items()},
            4.0 * gaps["featurize_vjp_f64_minus_longdouble"], 4.0 * gaps["mlp_vjp_f64_minus_longdouble"])


def _box(g, case):
    return g[f"{case}_box"] if f"{case}_box" in g.files else None


def mlp_spec(net) -> MLPSpec:
    return MLPSpec(net["widths"], net["activation"], net["ln_in"], net["ln_hidden"], net["head_activation"],
                   net["params"], net["mean"], net["scale"])


def make_bias(engine, gold, case, net_name):
    g, meta, raw, spec, _rec, _param = gold
    net = B.golden_network(net_name, g[f"{case}_mean"], g[f"{case}_scale"])
    return CVBiasPotential(mlp_spec(net), g[f"{case}_mean"], g[f"{case}_scale"],
                           feature_extractor=build_feature_extractor_module(spec, engine),
                           feature_spec_hash=feature_spec_sha256(raw), bias_strength=K), net


def table_of(engine, rec, param, width=None) -> FeatureTable:
    """A FeatureTable from raw records, in the order given (Engine.feature_table sorts by kind)."""
    rec, param = np.ascontiguousarray(rec, np.int32), np.ascontiguousarray(param, np.float32)
    width = int(rec[:, 6:8].max()) + 1 if width is None else width
    return FeatureTable(engine.to_device(rec), engine.to_device(param), width, int(rec[:, 1:5].max()),
                        bool((rec[:, 5] & B.MIC).any()), host_rec=rec)


def assert_adjoint(got, want, scale, gap, what):
    """|got - want| <= gap x (sum of the absolute terms), entry by entry; an entry without terms is exactly zero."""
    ratio = np.abs(got - want)[scale > 0] / scale[scale > 0]
    print(f"{what}: largest |device - restatement| / sum|terms| = {ratio.max():.3e}, bound {gap:.3e}")
    assert np.isfinite(got).all(), what
    assert not got[scale == 0].any(), what
    assert ratio.max() <= gap, what


def vjp(engine, table, xyz, gfeat, box=None, **kw) -> np.ndarray:
    xd = engine.to_device(np.ascontiguousarray(xyz, np.float32))
    return engine.featurize_spec_vjp(xd, table, engine.to_device(np.ascontiguousarray(gfeat, np.float64)), box=box,
                                     **kw).to_host()


# ------------------------------------------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("net_name", list(B.NETWORKS))
@pytest.mark.parametrize("case", CASES)
def test_golden_parity(engine, gold, tol, case, net_name):
    g, meta, _raw, spec, _rec, _param = gold
    bias, _net = make_bias(engine, gold, case, net_name)
    xyz, box = g[f"{case}_xyz"], _box(g, case)
    E, F = bias.energy_and_forces(xyz, box)
    cv = bias.compute_cvs(xyz, box)
    key = f"{case}__{net_name}"
    assert E.shape == (16,) and cv.shape == (16, 3) and F.shape == xyz.shape and F.dtype == np.float64
    for q, mine, want in (("energy", E, g[f"{key}__E64"]), ("cv", cv, g[f"{key}__cv64"]), ("force", F, g[f"{key}__F64"])):
        err = float(np.max(np.abs(mine - want)))
        print(f"{key} {q}: |device - ref64| = {err:.3e}, bound {tol[0][q]:.3e}, "
              f"ref32 is {meta['per_case'][key][q]['ref32_minus_ref64']:.3e} away, largest {np.max(np.abs(want)):.3g}")
        assert np.isfinite(mine).all()
        assert err <= tol[0][q], (key, q, err, tol[0][q])
    # the CVs are the forward kernels' bits
    xd = engine.to_device(xyz)
    feats = engine.featurize_spec(xd, engine.feature_table(spec), box=box)
    np.testing.assert_array_equal(cv, engine.mlp_forward(feats, bias.spec).to_host())
    if case == "tric15":
        np.testing.assert_array_equal(F[:, 12:], np.zeros((16, 3, 3)))
        assert not np.signbit(F[:, 12:]).any()
    # one frame: a scalar energy, (A, 3) forces, the batch's bits
    e0, f0 = bias.energy_and_forces(xyz[3], None if box is None else box[3])
    assert np.ndim(e0) == 0 and f0.shape == xyz.shape[1:]
    assert e0 == E[3] and bias.forward(xyz[3], None if box is None else box[3]) == E[3]
    np.testing.assert_array_equal(f0, F[3])
    np.testing.assert_array_equal(bias(xyz, box), E)


# ------------------------------------------------------------------------------------------------ 2. each adjoint alone
@pytest.mark.parametrize("case", CASES)
def test_featurizer_adjoint_alone(engine, gold, tol, case):
    g, _meta, _raw, spec, rec, param = gold
    xyz, box, gfeat = g[f"{case}_xyz"], _box(g, case), g[f"{case}_gfeat"]
    got = vjp(engine, engine.feature_table(spec), xyz, gfeat, box)
    want, scale = B.featurize_vjp(rec, param, xyz, gfeat, box)
    assert_adjoint(got, want, scale, tol[1], f"featurize_spec_vjp {case}")
    flipped = vjp(engine, engine.feature_table(spec), xyz, gfeat, box, sign=-1.0)
    np.testing.assert_array_equal(flipped, -got)


@pytest.mark.parametrize("upstream", ["given", "energy"])
@pytest.mark.parametrize("net_name", list(B.ADJOINT_NETWORKS))
def test_network_adjoint_alone(engine, gold, tol, net_name, upstream):
    g, _meta, _raw, spec, _rec, _param = gold
    case = "tric"
    net = B.adjoint_network(net_name, g[f"{case}_mean"], g[f"{case}_scale"])
    ms = mlp_spec(net)
    xd = engine.featurize_spec(engine.to_device(g[f"{case}_xyz"]), engine.feature_table(spec), box=_box(g, case))
    x = xd.to_host()
    up = g[f"{case}_gout"] if upstream == "given" else None
    got = engine.mlp_vjp(xd, ms, gout=engine.to_device(up) if up is not None else None, strength=K)
    energy, y, want, scale = B.mlp_vjp(net, x, up, K)
    assert_adjoint(got["gx"].to_host(), want, scale, tol[2], f"mlp_vjp {net_name} {upstream}")
    np.testing.assert_array_equal(got["outputs"].to_host(), engine.mlp_forward(xd, ms).to_host())
    e = got["energy"].to_host()
    assert np.max(np.abs(e - energy)) <= 1e-12 * np.max(np.abs(energy))
    # a float64 copy of the same inputs, and a wider input buffer: the same bits
    wide = np.full((16, 30), np.nan, np.float32)
    wide[:, :23] = x
    again = engine.mlp_vjp(engine.to_device(wide).view((16, 23)), ms, gout=engine.to_device(up) if up is not None else None,
                           strength=K, ld=30, want_energy=False, want_outputs=False)
    np.testing.assert_array_equal(again["gx"].to_host(), got["gx"].to_host())
    assert "energy" not in again and "outputs" not in again
    f64 = engine.mlp_vjp(engine.to_device(x.astype(np.float64)), ms, strength=K)
    if up is None:
        np.testing.assert_array_equal(f64["gx"].to_host(), got["gx"].to_host())


# ------------------------------------------------------------------------------------------------ 3. shapes
def test_ragged_groups_and_frame_independence(engine, gold):
    """n = 17 is one full group of 16 frames and a ragged one; every frame of the batch equals the frame run alone
    (n = 1), and the first 16 equal the batch of 16: energy, CVs and forces, bit for bit."""
    g, _meta, _raw, _spec, _rec, _param = gold
    for net_name in B.NETWORKS:
        bias, _ = make_bias(engine, gold, "tric", net_name)
        xyz = np.concatenate([g["tric_xyz"], g["tric_xyz"][4:5] + np.float32(0.25)])
        box = np.concatenate([g["tric_box"], g["tric_box"][4:5]])
        E, F = bias.energy_and_forces(xyz, box)
        cv = bias.compute_cvs(xyz, box)
        E16, F16 = bias.energy_and_forces(xyz[:16], box[:16])
        np.testing.assert_array_equal(E[:16], E16)
        np.testing.assert_array_equal(F[:16], F16)
        for t in (0, 7, 15, 16):
            e1, f1 = bias.energy_and_forces(xyz[t:t + 1], box[t:t + 1])
            np.testing.assert_array_equal(e1, E[t:t + 1])
            np.testing.assert_array_equal(f1, F[t:t + 1])
            np.testing.assert_array_equal(bias.compute_cvs(xyz[t], box[t]), cv[t:t + 1])
        # chunked evaluation (chunks of 5 frames: 5 + 5 + 5 + 2) gives the same bits
        eng, table = bias.feature_extractor._engine_table()
        res = eng.bias_energy_forces(eng.to_device(xyz), table, bias.spec, K, box=box, chunk=5)
        np.testing.assert_array_equal(res["energy"].to_host(), E)
        np.testing.assert_array_equal(res["force"].to_host(), F)
        np.testing.assert_array_equal(res["cv"].to_host(), cv)


def test_grid_stride_second_trip(engine, gold):
    """The adjoint kernel gives a block tiles of 64 frames and caps its grid at 16 blocks per CU
    (msm_featurize_spec_vjp: grid_for): from 64 x 16 x n_cu frames on a block takes a second trip.  The network
    kernel (one wave per 16 frames, capped at what is resident) is then many trips in."""
    g, _meta, _raw, _spec, _rec, _param = gold
    n = 64 * 16 * engine.info()["n_cu"] + 5
    bias, _ = make_bias(engine, gold, "tric", "tanh")
    small_E, small_F = bias.energy_and_forces(g["tric_xyz"], g["tric_box"])
    xd = engine.to_device(np.resize(g["tric_xyz"], (n, 12, 3)))
    bd = engine.to_device(np.resize(g["tric_box"], (n, 3, 3)).reshape(n, 9))
    eng, table = bias.feature_extractor._engine_table()
    res = eng.bias_energy_forces(xd, table, bias.spec, K, box=bd, chunk=n)        # one call, not chunks
    np.testing.assert_array_equal(res["energy"].to_host(), np.resize(small_E, n))
    np.testing.assert_array_equal(res["force"].to_host(), np.resize(small_F, (n, 12, 3)))


def test_small_unsorted_offset_and_trig_tables(engine, gold, tol):
    g, _meta, _raw, spec, rec, param = gold
    xyz, box = g["tric_xyz"], g["tric_box"]
    rng = np.random.default_rng(11)
    # a single record of each kind
    for r in (rec[0], rec[15], rec[19]):
        one = r.copy()[None]
        one[0, 6] = 0
        par = np.array([1.25], np.float32)
        gf = rng.normal(size=(16, 1))
        want, scale = B.featurize_vjp(one, par, xyz, gf, box)
        assert_adjoint(vjp(engine, table_of(engine, one, par), xyz, gf, box), want, scale, tol[1], f"kind {one[0, 0]} alone")
    assert sorted(int(k) for k in (rec[0, 0], rec[15, 0], rec[19, 0])) == [0, 1, 2]
    # an unsorted table: the same records, shuffled, give the sorted table's forces up to the order of the sums
    order = rng.permutation(len(rec))
    gf = g["tric_gfeat"]
    want, scale = B.featurize_vjp(rec[order], param[order], xyz, gf, box)
    assert_adjoint(vjp(engine, table_of(engine, rec[order], param[order]), xyz, gf, box), want, scale, tol[1], "unsorted")
    # col_off > 0 with ld > width: the block's neighbours (NaN) are not read
    wide = np.full((16, 40), np.nan)
    wide[:, 9:32] = gf
    base = vjp(engine, engine.feature_table(spec), xyz, gf, box)
    np.testing.assert_array_equal(vjp(engine, engine.feature_table(spec), xyz, wide, box, col0=9), base)
    # cos / sin emitters, interleaved (mode 1) and in blocks (mode 2), with distances in front
    for mode in (1, 2):
        table = engine.feature_table(pairs=[[0, 5], [2, 9]], quads=[[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]],
                                     dihedral_mode=mode)
        gf = rng.normal(size=(16, table.width))
        want, scale = B.featurize_vjp(table.host_rec, np.ones(5, np.float32), xyz, gf, box)
        assert table.width == 8 and (table.host_rec[2:, 5] & B.COSSIN).all()
        assert_adjoint(vjp(engine, table, xyz, gf, box), want, scale, tol[1], f"cos/sin mode {mode}")


def test_one_box_equals_the_same_box_repeated(engine, gold):
    g, _meta, _raw, _spec, _rec, _param = gold
    bias, _ = make_bias(engine, gold, "tric", "ln_gelu")
    xyz, box = g["tric_xyz"], g["tric_box"][2]
    E1, F1 = bias.energy_and_forces(xyz, box)
    En, Fn = bias.energy_and_forces(xyz, np.tile(box, (16, 1, 1)))
    np.testing.assert_array_equal(E1, En)
    np.testing.assert_array_equal(F1, Fn)
    for mic in ("round", "search"):
        eng, table = bias.feature_extractor._engine_table()
        gf = g["tric_gfeat"]
        np.testing.assert_array_equal(vjp(eng, table, xyz, gf, box, mic=mic),
                                      vjp(eng, table, xyz, gf, np.tile(box, (16, 1, 1)), mic=mic))


@pytest.mark.parametrize("name", ["tric", "ortho"])
def test_search_mode_on_stretched_chains(engine, gold, tol, name):
    """Chains with 0.6 nm bonds (tests/test_gpu_pbc.py's): in the skewed cell the rounding rule misses the true minimum
    image for some bond vectors, and the adjoint must follow the forward's choice."""
    g, _meta, _raw, spec, rec, param = gold
    rng = np.random.default_rng(7)
    xyz, box, _cells, _ = P.draw_frames(rng, CELLS[name], 16, spec, 12, 0.6)
    vs, vr = B.bond_vectors(rec, xyz, box, "search"), B.bond_vectors(rec, xyz, box, "round")
    differ = any((a != b).any() for u, w in zip(vs, vr) for a, b in zip(u, w))
    assert differ == (name == "tric")
    gf = g["tric_gfeat"]
    table = engine.feature_table(spec)
    for mic in ("search", "round"):
        want, scale = B.featurize_vjp(rec, param, xyz, gf, box, mic)
        assert_adjoint(vjp(engine, table, xyz, gf, box, mic=mic), want, scale, tol[1], f"{name} {mic}")
    # the chain under "search", against the restatement with the same images (TOL: see the module docstring)
    feats = B.features(rec, param, xyz, box, "search")
    net = B.golden_network("tanh", feats.mean(axis=0), feats.std(axis=0) + 0.05)
    bias = CVBiasPotential(mlp_spec(net), net["mean"], net["scale"], feature_extractor=build_feature_extractor_module(spec, engine),
                           feature_spec_hash="x", bias_strength=K)
    net = B.golden_network("tanh", bias.scaler_mean, bias.scaler_scale)          # the scaler as the potential keeps it
    E, F = bias.energy_and_forces(xyz, box, mic="search")
    wE, _cv, wF = B.energy_forces(rec, param, net, xyz, box, "search", K)
    print(f"search chain {name}: energy {np.max(np.abs(E - wE)):.3e} / {tol[0]['energy']:.3e}, "
          f"force {np.max(np.abs(F - wF)):.3e} / {tol[0]['force']:.3e}")
    assert np.max(np.abs(E - wE)) <= tol[0]["energy"] and np.max(np.abs(F - wF)) <= tol[0]["force"]


# ------------------------------------------------------------------------------------------------ 5. replay
def test_replay_and_graph_capture(engine, gold):
    g, _meta, _raw, _spec, _rec, _param = gold
    bias, _ = make_bias(engine, gold, "tric", "ln_gelu")
    xyz, box = g["tric_xyz"], g["tric_box"]
    first, second = bias.energy_and_forces(xyz, box), bias.energy_and_forces(xyz, box)
    np.testing.assert_array_equal(first[0], second[0])
    np.testing.assert_array_equal(first[1], second[1])
    # one MD step, captured: device-resident inputs, preallocated outputs and workspace
    xd, bd = engine.to_device(xyz[5:6]), engine.to_device(box[5:6].reshape(1, 9))
    E, F = bias.energy_and_forces_device(xd, bd)                                 # also uploads table and parameters
    want_E, want_F = E.to_host(), F.to_host()
    np.testing.assert_array_equal(want_E, first[0][5:6])
    np.testing.assert_array_equal(want_F, first[1][5:6])
    eng, table = bias.feature_extractor._engine_table()
    work = eng.bias_energy_forces(xd, table, bias.spec, K, box=bd)["work"]
    bufs = {"energy": engine.zeros((1,), np.float64), "cv": engine.zeros((1, 3), np.float64),
            "force": engine.zeros((1, 12, 3), np.float64), "work": work}
    engine.graph_begin()
    try:
        bias.energy_and_forces_device(xd, bd, **bufs)
    finally:
        graph = engine.graph_end()
    try:
        for _ in range(3):
            bufs["energy"].zero_()
            bufs["force"].zero_()
            engine.graph_launch(graph)
            engine.sync()
            np.testing.assert_array_equal(bufs["energy"].to_host(), want_E)
            np.testing.assert_array_equal(bufs["force"].to_host(), want_F)
            np.testing.assert_array_equal(bufs["cv"].to_host(), bias.compute_cvs(xyz[5], box[5]))
        # new coordinates in the same buffer: the replay follows them
        xd.copy_from_host(xyz[9:10])
        bd.copy_from_host(box[9:10].reshape(1, 9))
        engine.graph_launch(graph)
        engine.sync()
        np.testing.assert_array_equal(bufs["force"].to_host(), first[1][9:10])
    finally:
        engine.graph_destroy(graph)


# ------------------------------------------------------------------------------------------------ 6. degenerate geometry
def test_degenerate_geometry_contributes_exactly_zero(engine):
    """Exactly representable coordinates: atoms 0 and 1 coincide (a zero-length bond), atoms 2, 3, 4 sit on a line of
    the lattice (cos = -1 exactly), and the dihedral 2-3-4-5 has b0 parallel to b1 (no plane).  Stated divergence from
    torch, which returns 0, inf or NaN there: those features contribute exactly zero, the others are untouched."""
    xyz = np.zeros((3, 8, 3), np.float32)
    xyz[:, 0] = xyz[:, 1] = [0.5, 0.25, 0.75]
    xyz[:, 2], xyz[:, 3], xyz[:, 4] = [1, 0, 0], [2, 0, 0], [3, 0, 0]
    xyz[:, 5], xyz[:, 6], xyz[:, 7] = [3, 1, 0], [0.5, 1.5, -0.25], [-1, 0.5, 2]
    xyz[1] += np.float32(0.125)
    xyz[2] *= np.float32(2.0)
    sick = [[B.DISTANCE, 0, 1, 0, 0, 0], [B.ANGLE, 2, 3, 4, 0, 0], [B.ANGLE, 1, 0, 5, 0, 0],
            [B.DIHEDRAL, 2, 3, 4, 5, 0], [B.DIHEDRAL, 2, 3, 4, 5, B.COSSIN], [B.DIHEDRAL, 7, 0, 1, 6, 0]]
    sound = [[B.DISTANCE, 0, 5, 0, 0, 0], [B.DISTANCE, 2, 3, 0, 0, 0], [B.ANGLE, 0, 6, 7, 0, 0], [B.ANGLE, 3, 4, 5, 0, 0],
             [B.DIHEDRAL, 4, 5, 6, 7, 0], [B.DIHEDRAL, 0, 2, 5, 7, B.COSSIN]]

    def records(rows):
        rec, col = [], 0
        for r in rows:
            trig = r[0] == B.DIHEDRAL and r[5] & B.COSSIN
            rec.append(r + [col, col + 1 if trig else 0])
            col += 2 if trig else 1
        return np.asarray(rec, np.int32), col

    rec_all, w_all = records(sound + sick)
    rec_ok, w_ok = records(sound)
    rng = np.random.default_rng(3)
    gf = rng.normal(size=(3, w_all))
    par_all = rng.uniform(0.5, 2.0, size=len(rec_all)).astype(np.float32)
    got = vjp(engine, table_of(engine, rec_all, par_all, w_all), xyz, gf)
    ok = vjp(engine, table_of(engine, rec_ok, par_all[:len(rec_ok)], w_ok), xyz, gf[:, :w_ok])
    assert np.isfinite(got).all() and np.abs(ok).max() > 0.1
    np.testing.assert_array_equal(got, ok)
    only = vjp(engine, table_of(engine, records(sick)[0], par_all[len(rec_ok):], records(sick)[1]), xyz, gf[:, w_ok:])
    np.testing.assert_array_equal(only, np.zeros_like(only))
    want, _scale = B.featurize_vjp(rec_all, par_all, xyz, gf)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))           # the restatement has the same rule


# ------------------------------------------------------------------------------------------------ 7. non-finite frames
def test_non_finite_frames_are_isolated(engine, gold):
    g, _meta, _raw, _spec, _rec, _param = gold
    for net_name in B.NETWORKS:
        bias, _ = make_bias(engine, gold, "tric", net_name)
        xyz, box = g["tric_xyz"].copy(), g["tric_box"].copy()
        clean_E, clean_F = bias.energy_and_forces(xyz, box)
        clean_cv = bias.compute_cvs(xyz, box)
        xyz[3, 7, 1] = np.nan                                   # a NaN coordinate
        box[11] = 0.0                                           # a singular box (device boxes are taken as they are)
        box[12, 1] = box[12, 0] * 2.0                           # rank 2
        xd, bd = engine.to_device(xyz), engine.to_device(box.reshape(16, 9))
        eng, table = bias.feature_extractor._engine_table()
        res = eng.bias_energy_forces(xd, table, bias.spec, K, box=bd)
        E, F, cv = res["energy"].to_host(), res["force"].to_host(), res["cv"].to_host()
        bad = np.zeros(16, bool)
        bad[[3, 11, 12]] = True
        assert np.isnan(E[bad]).all() and np.isnan(F[bad]).all() and np.isnan(cv[bad]).all()
        np.testing.assert_array_equal(E[~bad], clean_E[~bad])
        np.testing.assert_array_equal(F[~bad], clean_F[~bad])
        np.testing.assert_array_equal(cv[~bad], clean_cv[~bad])
    # the adjoint alone: a non-finite upstream gradient poisons its own frame, all atoms of it
    gf = g["tric_gfeat"].copy()
    gf[2, 5], gf[9, 22] = np.inf, np.nan
    got = vjp(eng, table, g["tric_xyz"], gf, g["tric_box"])
    base = vjp(eng, table, g["tric_xyz"], g["tric_gfeat"], g["tric_box"])
    assert np.isnan(got[[2, 9]]).all()
    keep = np.setdiff1d(np.arange(16), [2, 9])
    np.testing.assert_array_equal(got[keep], base[keep])


# ------------------------------------------------------------------------------------------------ 8. contacts
def test_contacts_contribute_nothing(engine, gold):
    g, _meta, _raw, _spec, _rec, _param = gold
    xyz, box = g["tric_xyz"], g["tric_box"]
    kw = {"pairs": [[0, 5], [2, 9]], "triplets": [[1, 2, 3]], "quads": [[4, 5, 6, 7]]}
    with_c = engine.feature_table(**kw, contacts=[[0, 3], [2, 11], [5, 6]], rcut=0.4)
    without = engine.feature_table(**kw)
    gf = np.random.default_rng(8).normal(size=(16, with_c.width))
    assert with_c.width == without.width + 3
    np.testing.assert_array_equal(vjp(engine, with_c, xyz, gf, box), vjp(engine, without, xyz, gf[:, :without.width], box))
    # an incidence that does list the contacts (hand-made) still gets nothing from them
    as_distances = with_c.host_rec.copy()
    as_distances[as_distances[:, 0] == B.CONTACT, 0] = B.DISTANCE
    ptr, inc = B.incidence(as_distances, 12)
    listed = FeatureTable(with_c.rec, with_c.param, with_c.width, 11, True, host_rec=with_c.host_rec)
    listed._inc[12] = (engine.to_device(ptr), engine.to_device(inc))
    assert inc.size == len(B.incidence(with_c.host_rec, 12)[1]) + 6
    np.testing.assert_array_equal(vjp(engine, listed, xyz, gf, box), vjp(engine, with_c, xyz, gf, box))


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_launch_nothing(engine, gold):
    g, _meta, _raw, spec, _rec, _param = gold
    xyz, box = g["tric_xyz"], g["tric_box"]
    xd = engine.to_device(xyz)
    table = engine.feature_table(spec)
    feats = engine.featurize_spec(xd, table, box=box)
    sentinel = np.full((16, 12, 3), 7.0)
    force = engine.to_device(sentinel)
    for widths, text in (((23, 257, 3), "width 257 of layer 1 (at most 256 is supported)"),
                         ((23, 32, 65), "65 outputs (at most 64 are supported)")):
        ms = MLPSpec(widths, 0, False, False, True, np.zeros(widths[0] * widths[1] + widths[1] + widths[1] * widths[2]
                                                              + widths[2], np.float32))
        with pytest.raises(NotImplementedError) as err:
            engine.mlp_vjp(feats, ms)
        assert text in str(err.value) and "msm_mlp_vjp" in str(err.value)
        with pytest.raises(NotImplementedError) as err:
            engine.bias_energy_forces(xd, table, ms, K, box=box, force=force)
        assert text in str(err.value)
        wd = np.ascontiguousarray(widths, np.int32)
        p = engine.zeros((ms.params.size,), np.float32)
        work = engine.zeros((1 << 16,), np.float64)
        ptr, inc = table.incidence(12)
        st = lib.msm_bias_energy_forces(engine.handle, xd.ptr, 16, 12, None, 0, table.rec.ptr, table.param.ptr, 23, ptr.ptr,
                                        inc.ptr, 0, None, None, 2, wd.ctypes.data, 0, 0, 0, 1, p.ptr, p.size, K, work.ptr,
                                        work.nbytes, engine.zeros((16,), np.float64).ptr, None, 3, force.ptr)
        msg = lib.msm_last_error(engine.handle).decode()
        assert st == _lib.MSM_ERR_UNSUPPORTED and text in msg and "msm_bias_energy_forces" in msg
    bias, net = make_bias(engine, gold, "tric", "tanh")
    ms, wd = bias.spec, np.ascontiguousarray(bias.spec.widths, np.int32)
    params, mean, scale = engine._mlp_on_device(ms)
    ptr, inc = table.incidence(12)
    gx = engine.to_device(np.full((16, 23), 7.0))
    need = int(lib.msm_mlp_vjp_workspace(16, 3, wd.ctypes.data, 0, 0, 1))
    assert need == 16 * (32 + 16 + 3) * 8
    work = engine.zeros((need // 8,), np.float64)
    st = lib.msm_mlp_vjp(engine.handle, feats.ptr, 0, 16, 23, 23, mean.ptr, scale.ptr, 3, wd.ctypes.data, 0, 0, 0, 1,
                         params.ptr, params.size, None, 0, K, None, None, 3, gx.ptr, 23, work.ptr, need - 8)
    assert st == _lib.MSM_ERR_INVALID and "workspace" in lib.msm_last_error(engine.handle).decode()
    st = lib.msm_bias_energy_forces(engine.handle, xd.ptr, 16, 12, None, 0, table.rec.ptr, table.param.ptr, 23, ptr.ptr,
                                    inc.ptr, 0, mean.ptr, scale.ptr, 3, wd.ctypes.data, 0, 0, 0, 1, params.ptr, params.size,
                                    K, work.ptr, work.nbytes, engine.zeros((16,), np.float64).ptr, None, 3, force.ptr)
    assert st == _lib.MSM_ERR_INVALID and "workspace" in lib.msm_last_error(engine.handle).decode()
    gd = engine.to_device(g["tric_gfeat"])
    st = lib.msm_featurize_spec_vjp(engine.handle, xd.ptr, 16, 12, None, 0, table.rec.ptr, table.param.ptr, 23, 23, 0,
                                    gd.ptr, 23, 1, ptr.ptr, inc.ptr, 1.0, force.ptr)
    msg = lib.msm_last_error(engine.handle).decode()
    assert st == _lib.MSM_ERR_INVALID and "exceed" in msg and "msm_featurize_spec_vjp" in msg
    with pytest.raises(ValueError, match="exceed"):
        engine.featurize_spec_vjp(xd, table, gd, box=box, col0=1)
    short = engine.to_device(xyz[:, :11].copy())
    with pytest.raises(RuntimeError, match="expected at least 12 atoms, received 11"):
        bias.energy_and_forces_device(short, engine.to_device(box.reshape(16, 9)))
    with pytest.raises(ValueError, match="out of range"):
        engine.featurize_spec_vjp(short, table, gd, box=box)
    with pytest.raises(ValueError, match="mic"):
        engine.featurize_spec_vjp(xd, table, gd, box=box, mic="nearest")
    engine.sync()
    np.testing.assert_array_equal(force.to_host(), sentinel)                    # nothing was launched
    np.testing.assert_array_equal(gx.to_host(), np.full((16, 23), 7.0))
    E, _F = bias.energy_and_forces(xyz, box)                                     # usable afterwards
    assert np.isfinite(E).all()


# ------------------------------------------------------------------------------------------------ 10. no scratch
def test_new_kernels_use_no_scratch(tmp_path):
    from tests.test_code_objects import _kernel_scratch

    sizes = {name: size for name, size in _kernel_scratch(tmp_path).items()
             if "spec_vjp_kernel" in name or "mlp_vjp_kernel" in name}
    assert len(sizes) == 4, sizes                  # round / search, float32 / float64
    assert not any(sizes.values()), sizes
