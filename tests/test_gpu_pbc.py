"""Periodic boundaries on the device: msm_box_from_cell and msm_featurize_spec (csrc/featurize.hip, csrc/pbc.h)
through Engine.box_from_cell / Engine.featurize_spec, the device feature extractor and the registry featurizers.

Yardsticks.  The golden outputs (tests/golden/pbc.npz) are the reference extractor's, fp32 on fp32 inputs; pbc.json
records per kind the largest |fp32 restatement - reference|.  The device differs from that restatement only by the
rounding of acosf / atan2f (the restatement rounds them correctly), inside the same error model, so the device is
held to 4 x the recorded value per kind (TOL), dihedrals modulo 2 pi and scaled by |weight|.  The same TOL serves
where the yardstick is an fp64 computation on the same fp32 inputs (lattice invariance, search mode): the recorded
values ARE fp32-against-fp32 differences of this arithmetic at these coordinate magnitudes (|x| <= 3 box lengths),
and the stretched chains of the search tests have the same absolute coordinate error over four times longer bond
vectors, i.e. better conditioned angles.  Where two device results must agree exactly, assert_array_equal."""

from __future__ import annotations

import json

import numpy as np
import pytest

from pmarlo_amd import _lib
from pmarlo_amd._lib import lib
from pmarlo_amd.features.deeptica.ts_feature_extractor import build_feature_extractor_module, canonicalize_feature_spec
from tests import _pbc_ref as ref
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

KINDS = ("distance", "angle", "dihedral")
CELLS = {"ortho": (2.0, 2.5, 3.0, 90.0, 90.0, 90.0), "tric": (2.4, 2.6, 2.9, 75.0, 98.0, 62.0),
         "octa": (3.0, 3.0, 3.0, 70.53, 109.47, 70.53)}


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLDEN / "pbc.npz", allow_pickle=False)
    meta = json.loads((GOLDEN / "pbc.json").read_text())
    spec = canonicalize_feature_spec(meta["spec"])
    tol = {k: 4.0 * v for k, v in meta["max_abs_fp32_restatement_minus_reference"].items()}
    return g, meta, spec, tol


@pytest.fixture(scope="module")
def stretched(gold):
    """Chains with 0.6 nm bonds: long enough for the rounding rule to miss the true minimum image in the skewed cells."""
    _g, _meta, spec, _tol = gold
    rng = np.random.default_rng(7)
    out = {}
    for name, cell in CELLS.items():
        xyz, box, cells, _ = ref.draw_frames(rng, cell, 32, spec, 12, 0.6)
        assert ref.well_conditioned(spec, xyz, box).all()
        out[name] = (xyz, box, cells, ref.extract(spec, xyz, box, mic="round", dtype=np.float64),
                     ref.extract(spec, xyz, box, mic="search", dtype=np.float64))
    return out


def kind_errors(spec, got, want) -> dict[str, float]:
    w = np.asarray(spec.feature_weights, np.float64)
    out = {}
    for kind in KINDS:
        pos = np.asarray(getattr(spec, f"{kind}_positions"))
        d = np.asarray(got, np.float64)[:, pos] - np.asarray(want, np.float64)[:, pos]
        if kind == "dihedral":
            d = ref.wrap_to_pi(d / w[pos]) * np.abs(w[pos])
        out[kind] = float(np.abs(d).max()) if d.size else 0.0
    return out


def assert_within(spec, got, want, tol, what):
    err = kind_errors(spec, got, want)
    print(what, {k: f"{v:.3e} / {tol[k]:.3e}" for k, v in err.items()})
    assert np.isfinite(got).all(), what
    for kind in KINDS:
        assert err[kind] <= tol[kind], (what, kind, err[kind], tol[kind])


def flagged_columns(spec) -> np.ndarray:
    f = np.zeros(spec.n_features, bool)
    for kind in KINDS:
        f[getattr(spec, f"{kind}_positions")[getattr(spec, f"{kind}_pbc")]] = True
    return f


def run(engine, spec_or_table, xyz, box=None, mic="round") -> np.ndarray:
    return engine.featurize_spec(engine.to_device(np.ascontiguousarray(xyz, np.float32)), spec_or_table, box=box,
                                 mic=mic).to_host()


# ---------------------------------------------------------------------------------------------- golden
@pytest.mark.parametrize("name", list(CELLS))
def test_round_mode_matches_the_reference_extractor(engine, gold, name):
    g, _meta, spec, tol = gold
    xyz, box, want = g[f"{name}_xyz"], g[f"{name}_box"], g[f"{name}_out"]
    got = run(engine, spec, xyz, box, "round")
    assert got.shape == want.shape and got.dtype == np.float32
    assert_within(spec, got, want, tol, f"golden {name}")
    # the module's forward, one frame at a time as the reference's, and its batch transform
    module = build_feature_extractor_module(spec, engine)
    assert module.feature_count == 23 and module.atom_count == 12 and module.use_pbc
    for t in (0, 31, 63):
        one = module.forward(xyz[t], box[t])
        assert one.shape == (23,)
        np.testing.assert_array_equal(one, got[t])
        np.testing.assert_array_equal(module(xyz[t], box[t]), one)
    np.testing.assert_array_equal(module.transform(xyz, box).to_host(), got)
    with pytest.raises(RuntimeError, match="shape"):
        module.forward(xyz[0].reshape(-1), box[0])
    with pytest.raises(RuntimeError, match="atoms"):
        module.forward(xyz[0, :5], box[0])


def test_box_from_cell_on_the_device(engine, gold):
    g, _meta, _spec, _tol = gold
    cells = np.concatenate([g[f"{name}_cell"] for name in CELLS] + [np.array([[2.0, 3.0, 4.0, 90.0, 90.0, 120.0]])])
    got = engine.box_from_cell(cells).to_host()
    want = ref.box_from_cell(cells)
    assert got.shape == (cells.shape[0], 9) and got.dtype == np.float32
    # fp64 arithmetic, one rounding: at most one fp32 ulp from the rounded fp64 host value (device libm vs host libm)
    np.testing.assert_allclose(got.reshape(-1, 3, 3), want.astype(np.float32), rtol=2.0 ** -23, atol=0)
    ortho = got[:64].reshape(-1, 3, 3)
    assert (ortho[:, ~np.eye(3, dtype=bool)] == 0.0).all()          # exactly diagonal
    np.testing.assert_array_equal(got[:64], g["ortho_box"].reshape(64, 9))
    dev = engine.box_from_cell(engine.to_device(cells))             # device-resident cells
    np.testing.assert_array_equal(dev.to_host(), got)
    with pytest.raises(ValueError):
        engine.box_from_cell(np.zeros((3, 5)))


# ---------------------------------------------------------------------------------------------- known answers
def test_known_answers(engine, golden):
    L = 3.0
    two = np.array([[[0.1, 0.2, 0.3], [L - 0.1, 0.2, 0.3]]], np.float32)
    spec = [{"type": "distance", "atoms": [0, 1]}, {"type": "distance", "atoms": [0, 1], "pbc": False}]
    for mic in ("round", "search"):
        out = run(engine, spec, two, np.eye(3) * L, mic)
        np.testing.assert_allclose(out[0], [0.2, L - 0.2], atol=1e-6)
    cube = golden("featurizer.npz")["cube_xyz"]
    spec = [{"type": "distance", "atoms": [0, 1]}, {"type": "angle", "atoms": [0, 1, 2]},
            {"type": "dihedral", "atoms": [0, 1, 2, 3]}]
    for mic in ("round", "search"):
        out = run(engine, spec, cube, np.eye(3) * 10.0, mic)
        np.testing.assert_allclose(out[0], [1.0, np.pi / 2, np.pi / 2], atol=1e-6)
    # the same cube with its atoms in four different images of a box of side 10
    moved = cube + np.array([[10, 0, 0], [0, -10, 0], [0, 0, 10], [-10, 10, 0]], np.float32)[None]
    np.testing.assert_allclose(run(engine, spec, moved, np.eye(3) * 10.0)[0], [1.0, np.pi / 2, np.pi / 2], atol=1e-5)


# ---------------------------------------------------------------------------------------------- lattice invariance
@pytest.mark.parametrize("mic", ["round", "search"])
def test_lattice_invariance(engine, gold, mic):
    g, _meta, spec, tol = gold
    xyz, box = g["tric_xyz"], g["tric_box"]
    rng = np.random.default_rng(3)
    shifts = rng.integers(-1, 2, size=(xyz.shape[0], xyz.shape[1], 3))
    shifts[:, 0] = [1, -1, 1]               # no atom pair of the spec keeps its relative image everywhere
    shifts[:, 1::2] *= -1
    moved = (xyz.astype(np.float64) + np.einsum("tai,tij->taj", shifts, box.astype(np.float64))).astype(np.float32)
    a, b = run(engine, spec, xyz, box, mic), run(engine, spec, moved, box, mic)
    flagged = flagged_columns(spec)
    assert flagged.sum() == 19
    masked = spec.feature_weights * 0          # compare flagged columns only: zero the others on both sides
    assert_within(spec, np.where(flagged, b, masked), np.where(flagged, a, masked), tol, f"lattice {mic}")
    assert (np.abs(a - b)[:, ~flagged].max(axis=0) > 1.0e-2).all()      # unflagged features see the displacement


# ---------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_no_box_and_flags_off_are_bit_identical_to_the_per_kind_kernels(engine, gold, mode):
    g, _meta, _spec, _tol = gold
    xyz, box = g["octa_xyz"], g["octa_box"]
    rng = np.random.default_rng(mode)
    pairs = rng.integers(0, 12, size=(9, 2))
    triplets = np.array([[0, 1, 2], [3, 7, 11], [5, 4, 9]])
    quads = np.array([[0, 1, 2, 3], [4, 6, 8, 10], [11, 3, 7, 1], [2, 2, 5, 6]])      # one with a zero-length bond
    xd = engine.to_device(xyz)
    want = engine.featurize(xd, pairs=pairs, triplets=triplets, quads=quads, dihedral_mode=mode).to_host()
    kw = dict(pairs=pairs, triplets=triplets, quads=quads, dihedral_mode=mode)
    on, off = engine.feature_table(periodic=True, **kw), engine.feature_table(periodic=False, **kw)
    assert on.width == want.shape[1] == off.width and on.any_mic and not off.any_mic
    for mic in ("round", "search"):
        np.testing.assert_array_equal(engine.featurize_spec(xd, on, box=None, mic=mic).to_host(), want)
        np.testing.assert_array_equal(engine.featurize_spec(xd, off, box=box, mic=mic).to_host(), want)
    # flags off inside the kernel too: the box reaches the launch because another record is flagged
    mixed = engine.feature_table(spec=[{"type": "distance", "atoms": [0, 1]}]
                                 + [{"type": "distance", "atoms": [int(i), int(j)], "pbc": False} for i, j in pairs])
    got = engine.featurize_spec(xd, mixed, box=box).to_host()
    np.testing.assert_array_equal(got[:, 1:], want[:, :9])
    assert np.abs(got[:, 0] - engine.featurize(xd, pairs=[[0, 1]]).to_host()[:, 0]).max() > 0.1


def test_one_box_equals_the_same_box_repeated(engine, gold):
    g, _meta, spec, _tol = gold
    xyz, box = g["tric_xyz"], g["tric_box"][5]
    for mic in ("round", "search"):
        one = run(engine, spec, xyz, box, mic)
        np.testing.assert_array_equal(one, run(engine, spec, xyz, np.tile(box, (64, 1, 1)), mic))
        # and device-resident, in both accepted shapes
        xd = engine.to_device(xyz)
        dbox = engine.to_device(box.reshape(1, 9))
        table = engine.feature_table(spec)
        np.testing.assert_array_equal(engine.featurize_spec(xd, table, box=dbox, mic=mic).to_host(), one)
        np.testing.assert_array_equal(engine.featurize_spec(xd, table, box=dbox.view((1, 3, 3)), mic=mic).to_host(), one)


# ---------------------------------------------------------------------------------------------- search mode
@pytest.mark.parametrize("name", ["tric", "octa"])
def test_search_mode_finds_the_true_minimum_image(engine, gold, stretched, name):
    g, _meta, spec, tol = gold
    xyz, box, _cells, want_round, want_search = stretched[name]
    differs = np.abs(ref.wrap_to_pi(want_round - want_search)).max(axis=0) > 1.0e-3
    for kind in KINDS:                                   # the inputs do tell the two rules apart, in every kind
        assert differs[getattr(spec, f"{kind}_positions")].any(), kind
    assert_within(spec, run(engine, spec, xyz, box, "search"), want_search, tol, f"search {name}")
    assert_within(spec, run(engine, spec, xyz, box, "round"), want_round, tol, f"round {name}")
    # on the golden inputs (short bonds, inside the radius where the 27 images are not tried) the rules agree
    assert_within(spec, run(engine, spec, g[f"{name}_xyz"], g[f"{name}_box"], "search"), g[f"{name}_out"], tol,
                  f"search on golden {name}")


def test_search_equals_round_on_an_orthorhombic_box(engine, gold, stretched):
    g, _meta, spec, _tol = gold
    for xyz, box in ((g["ortho_xyz"], g["ortho_box"]), stretched["ortho"][:2]):
        np.testing.assert_array_equal(run(engine, spec, xyz, box, "search"), run(engine, spec, xyz, box, "round"))


# ---------------------------------------------------------------------------------------------- launch paths
def test_single_feature_single_frame_single_kind(engine, gold):
    g, _meta, spec, tol = gold
    xyz, box, want = g["tric_xyz"], g["tric_box"], g["tric_out"]
    full = run(engine, spec, xyz, box)
    # F = 1: 256 frames' boxes per tile trip would fit; here 64 frames, one block
    one = run(engine, [{"type": "dihedral", "atoms": [0, 1, 2, 3]}], xyz, box)
    np.testing.assert_array_equal(one[:, 0], full[:, 3])
    # n = 1
    np.testing.assert_array_equal(run(engine, spec, xyz[17:18], box[17:18]), full[17:18])
    # a table of a single kind: the 15 distances at their weights
    pos = spec.distance_positions
    dist = [{"type": "distance", "atoms": [int(i), int(j)], "pbc": bool(p), "weight": float(w)}
            for (i, j), p, w in zip(spec.distance_pairs, spec.distance_pbc, spec.feature_weights[pos])]
    np.testing.assert_array_equal(run(engine, dist, xyz, box), full[:, pos])
    assert_within(spec, full, want, tol, "tric again")


@pytest.mark.parametrize("n", [70_000, 200_000])
def test_grid_stride_second_trip(engine, gold, n):
    """F = 23.  n = 70 000 is 1.61 M elements, more than the 256 x 16 x n_cu threads of a capped grid of one element
    per thread.  The kernel gives a block a tile of 1024 // 23 = 44 frames, so its capped grid of 16 n_cu blocks
    takes a second trip from 44 x 16 x n_cu frames on: n = 200 000 is beyond that."""
    g, _meta, spec, _tol = gold
    n_cu = engine.info()["n_cu"]
    assert 70_000 * 23 > n_cu * 16 * 256 and 200_000 > 44 * 16 * n_cu
    xyz, box = np.resize(g["octa_xyz"], (n, 12, 3)), np.resize(g["octa_box"], (n, 3, 3))
    small = run(engine, spec, g["octa_xyz"], g["octa_box"], "search")
    xd, table = engine.to_device(xyz), engine.feature_table(spec)
    big = engine.featurize_spec(xd, table, box=engine.to_device(box.reshape(n, 9)), mic="search").to_host()
    np.testing.assert_array_equal(big, np.resize(small, (n, 23)))
    one = engine.featurize_spec(xd, table, box=g["octa_box"][0], mic="round").to_host()      # n_box = 1 at scale
    np.testing.assert_array_equal(one[::64], np.tile(one[0], (len(one[::64]), 1)))
    np.testing.assert_array_equal(one[:64], run(engine, spec, g["octa_xyz"], g["octa_box"][0]))


def test_tile_shapes_and_unsorted_table(engine, gold):
    """The tile of a block is 1024 // F frames, at least 1 and at most 256: F = 1 with more frames than one tile
    holds, F = 1056 > 1024 (one frame per tile, several passes of the block over it), F = 4 (exactly 256 frames);
    and a table whose records are not grouped by kind, which the kernel must compute all the same."""
    from pmarlo_amd.device import FeatureTable, _table_from_spec

    g, _meta, spec, _tol = gold
    xyz, box = np.resize(g["tric_xyz"], (600, 12, 3)), np.resize(g["tric_box"], (600, 3, 3))
    xd, bd = engine.to_device(xyz), engine.to_device(box.reshape(600, 9))
    full = engine.featurize_spec(xd, engine.feature_table(spec), box=bd, mic="search").to_host()
    np.testing.assert_array_equal(full[64:128], full[:64])
    one = engine.featurize_spec(xd, engine.feature_table([{"type": "angle", "atoms": [0, 5, 11]}]), box=bd, mic="search")
    np.testing.assert_array_equal(one.to_host()[:, 0], full[:, 11])
    four = _meta["spec"]["features"][:4]
    np.testing.assert_array_equal(engine.featurize_spec(xd, four, box=bd, mic="search").to_host(), full[:, :4])
    wide = [dict(e, name=None) for _ in range(46) for e in _meta["spec"]["features"]][:1056]
    got = engine.featurize_spec(xd, wide, box=bd, mic="search").to_host()
    assert got.shape == (600, 1056)
    np.testing.assert_array_equal(got, np.tile(full, (1, 46))[:, :1056])
    # the same 23 records in the order of the spec (kinds interleaved), then reversed
    rec, param, width = _table_from_spec(spec)
    order = np.argsort(rec[:, 6], kind="stable")
    assert (np.diff(rec[order, 0]) < 0).any()
    for perm in (order, order[::-1]):
        table = FeatureTable(engine.to_device(rec[perm]), engine.to_device(param[perm]), width, 11, True)
        np.testing.assert_array_equal(engine.featurize_spec(xd, table, box=bd, mic="search").to_host(), full)


def test_col0_ld_and_trig_emit(engine, gold):
    g, _meta, spec, _tol = gold
    xyz, box = g["tric_xyz"], g["tric_box"]
    xd = engine.to_device(xyz)
    full = run(engine, spec, xyz, box)
    sentinel = np.float32(-77.5)
    wide = engine.to_device(np.full((64, 40), sentinel, np.float32))
    out = engine.featurize_spec(xd, spec, box=box, out=wide, col0=9)
    assert out is wide
    host = wide.to_host()
    np.testing.assert_array_equal(host[:, 9:32], full)
    assert (host[:, :9] == sentinel).all() and (host[:, 32:] == sentinel).all()
    # cos / sin into non-adjacent columns (mode 2: cos block | sin block; mode 1: interleaved), flagged
    quads = spec.dihedral_quads
    rad = engine.featurize_spec(xd, engine.feature_table(quads=quads), box=box).to_host()
    for mode in (1, 2):
        trig = engine.featurize_spec(xd, engine.feature_table(quads=quads, dihedral_mode=mode), box=box).to_host()
        cos, sin = (trig[:, 0::2], trig[:, 1::2]) if mode == 1 else (trig[:, :4], trig[:, 4:])
        # fp32 cos / sin of the fp32 angle against the exact value: 4 ulp of 1, OpenCL's bound for these functions
        np.testing.assert_allclose(cos, np.cos(rad.astype(np.float64)), atol=4.0 * 2.0 ** -23)
        np.testing.assert_allclose(sin, np.sin(rad.astype(np.float64)), atol=4.0 * 2.0 ** -23)
    # weight 1 and the spec's own flags: the weighted columns are that result times the weight, one fp32 product
    pos = spec.dihedral_positions
    unw = run(engine, [{"type": "dihedral", "atoms": [int(a) for a in q], "pbc": bool(p)}
                       for q, p in zip(quads, spec.dihedral_pbc)], xyz, box)
    np.testing.assert_array_equal(unw * spec.feature_weights[pos][None, :], full[:, pos])
    np.testing.assert_array_equal(unw[:, spec.dihedral_pbc], rad[:, spec.dihedral_pbc])


# ---------------------------------------------------------------------------------------------- degenerate inputs
def test_zero_length_flagged_bond_stays_finite(engine):
    xyz = np.zeros((3, 4, 3), np.float32)
    xyz[:, 1] = xyz[:, 0] = [0.3, 0.4, 0.5]               # atoms 0 and 1 coincide
    xyz[:, 2] = [0.5, 0.4, 0.5]
    xyz[:, 3] = [0.5, 0.6, 0.7]
    kw = dict(pairs=[[0, 1]], triplets=[[0, 1, 2]], quads=[[0, 1, 2, 3]])
    xd = engine.to_device(xyz)
    want = engine.featurize(xd, **kw).to_host()
    for mic in ("round", "search"):
        got = engine.featurize_spec(xd, engine.feature_table(**kw), box=np.eye(3) * 2.0, mic=mic).to_host()
        assert np.isfinite(got).all()
        np.testing.assert_array_equal(got, want)          # eps = 1e-12 under the fp32 sum, as the per-kind kernels
    assert want[0, 0] == np.sqrt(np.float32(1.0e-12)) and want[0, 2] == 0.0


def test_singular_device_box_gives_nan_in_flagged_columns_only(engine, gold):
    g, _meta, spec, _tol = gold
    xyz, box = g["tric_xyz"][:6], g["tric_box"][:6].copy()
    good = run(engine, spec, xyz, box)
    box[1] = 0.0
    box[2, 1] = box[2, 0] * 2.0                            # rank 2
    box[4, 2, 2] = np.nan
    box[5, 0, 1] = np.inf
    xd, table = engine.to_device(xyz), engine.feature_table(spec)
    flagged = flagged_columns(spec)
    for mic in ("round", "search"):
        got = engine.featurize_spec(xd, table, box=engine.to_device(box.reshape(6, 9)), mic=mic).to_host()
        for t in (1, 2, 4, 5):
            assert np.isnan(got[t, flagged]).all(), (mic, t)
            np.testing.assert_array_equal(got[t, ~flagged], good[t, ~flagged])
        if mic == "round":
            np.testing.assert_array_equal(got[[0, 3]], good[[0, 3]])
    np.testing.assert_array_equal(run(engine, spec, xyz, g["tric_box"][:6]), good)       # the next launch is sound
    one = engine.featurize_spec(xd, table, box=engine.to_device(np.zeros((1, 9), np.float32))).to_host()
    assert np.isnan(one[:, flagged]).all() and np.isfinite(one[:, ~flagged]).all()


def test_host_side_errors(engine, gold):
    g, _meta, spec, _tol = gold
    xyz, box = g["tric_xyz"][:5], g["tric_box"][:5]
    xd = engine.to_device(xyz)
    bad = box.copy()
    bad[3] = 0.0
    with pytest.raises(ValueError, match="determinant"):
        engine.featurize_spec(xd, spec, box=bad)
    with pytest.raises(ValueError, match="determinant"):
        engine.featurize_spec(xd, spec, box=-box[0])
    bad = box.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        engine.featurize_spec(xd, spec, box=bad)
    with pytest.raises(ValueError, match="boxes"):
        engine.featurize_spec(xd, spec, box=box[:2])
    with pytest.raises(ValueError, match="boxes"):
        engine.featurize_spec(xd, spec, box=engine.to_device(box[:3].reshape(3, 9)))
    with pytest.raises(ValueError, match="shape"):
        engine.featurize_spec(xd, spec, box=np.eye(4))
    with pytest.raises(ValueError, match="mic"):
        engine.featurize_spec(xd, spec, box=box, mic="nearest")
    with pytest.raises(ValueError, match="out of range"):
        engine.featurize_spec(xd, [{"type": "distance", "atoms": [0, 12]}], box=box)
    with pytest.raises(ValueError, match="exceed"):
        engine.featurize_spec(xd, spec, box=box, out=engine.empty((5, 30), np.float32), col0=8)
    with pytest.raises(ValueError, match="exceed"):
        engine.featurize_spec(xd, spec, box=box, out=engine.empty((5, 30), np.float32), col0=-1)
    dup = canonicalize_feature_spec([{"type": "distance", "atoms": [0, 1]}, {"type": "angle", "atoms": [0, 1, 2]}])
    object.__setattr__(dup, "angle_positions", np.array([0]))
    with pytest.raises(ValueError, match="share an output position"):
        engine.feature_table(dup)
    object.__setattr__(dup, "angle_positions", np.array([2]))
    with pytest.raises(ValueError, match="position outside"):
        engine.feature_table(dup)
    with pytest.raises(ValueError, match="dihedral_mode"):
        engine.feature_table(quads=[[0, 1, 2, 3]], dihedral_mode=3)
    with pytest.raises(ValueError, match="empty"):
        engine.feature_table()


def test_library_argument_checks(engine, gold):
    """MSM_ERR_INVALID with a message, before anything is launched."""
    g, _meta, spec, _tol = gold
    n, A = 4, 12
    xd = engine.to_device(g["tric_xyz"][:n])
    bd = engine.to_device(g["tric_box"][:n].reshape(n, 9))
    table = engine.feature_table(spec)
    out = engine.empty((n, 23), np.float32)

    def call(xyz=xd.ptr, box=bd.ptr, n_box=n, rec=table.rec.ptr, param=table.param.ptr, F=23, width=23,
             mic=_lib.MIC_ROUND, o=out.ptr, ld=23, col_off=0):
        st = lib.msm_featurize_spec(engine.handle, xyz, n, A, box, n_box, rec, param, F, width, mic, o, ld, col_off)
        return st, lib.msm_last_error(engine.handle).decode()

    assert call()[0] == _lib.MSM_OK
    for kw, word in ((dict(n_box=2), "n_box"), (dict(n_box=0), "n_box"), (dict(box=None, n_box=1), "n_box"),
                     (dict(mic=2), "mic"), (dict(mic=-1), "mic"), (dict(ld=22), "exceed"), (dict(col_off=1), "exceed"),
                     (dict(col_off=-1, ld=40), "exceed"), (dict(xyz=None), "NULL"), (dict(rec=None), "NULL"),
                     (dict(param=None), "NULL"), (dict(o=None), "NULL"), (dict(rec=table.rec.ptr + 4), "aligned")):
        st, msg = call(**kw)
        assert st == _lib.MSM_ERR_INVALID and word in msg and "msm_featurize_spec" in msg, (kw, st, msg)
    assert call(box=None, n_box=0)[0] == _lib.MSM_OK
    assert lib.msm_box_from_cell(engine.handle, None, 3, out.ptr) == _lib.MSM_ERR_INVALID
    assert "NULL" in lib.msm_last_error(engine.handle).decode()
    assert lib.msm_box_from_cell(engine.handle, None, 0, None) == _lib.MSM_OK
    # a record whose column lies outside [0, width) writes nothing; one with an atom outside [0, A) writes NaN
    rec = np.array([[0, 0, 1, 0, 0, 0, 5, 0], [0, 0, 99, 0, 0, 0, 1, 0], [0, 2, 3, 0, 0, 0, 0, 0]], np.int32)
    tiny = engine.to_device(np.full((n, 2), -1.0, np.float32))
    drec, dpar = engine.to_device(rec), engine.to_device(np.ones(3, np.float32))
    st = lib.msm_featurize_spec(engine.handle, xd.ptr, n, A, None, 0, drec.ptr, dpar.ptr, 3, 2, 0, tiny.ptr, 2, 0)
    assert st == _lib.MSM_OK
    host = tiny.to_host()
    assert np.isnan(host[:, 1]).all()
    np.testing.assert_array_equal(host[:, 0], engine.featurize(xd, pairs=[[2, 3]]).to_host()[:, 0])
    engine.sync()


# ---------------------------------------------------------------------------------------------- registry
def test_registry_featurizers_follow_the_cell(gold, tmp_path):
    from pmarlo_amd.api.features import compute_features
    from pmarlo_amd.features import featurize_trajectory
    from pmarlo_amd.io.dcd import load_dcd, write_dcd
    from pmarlo_amd.io.pdb import Topology, Trajectory
    from pmarlo_amd.markov_state_model.features import compute_msm_features

    g, _meta, _spec, tol = gold
    xyz, cells = g["tric_xyz"], g["tric_cell"]
    # four residues of N, CA, C: three phi, three psi, four C-alpha
    top = Topology(["N", "CA", "C"] * 4, ["ALA"] * 12, np.repeat(np.arange(4), 3), ["A"] * 12)
    path = tmp_path / "cell.dcd"
    write_dcd(path, xyz, cells)
    traj = load_dcd(path, top=top)                       # a DCD with cell records, as a user would meet it
    xyz = traj.xyz                                       # Angstrom on disk: the coordinates the device sees
    bare = Trajectory(xyz, top)
    box = ref.box_from_cell(traj.unitcell).astype(np.float32)
    phi, psi = top.phi_indices(), top.psi_indices()
    ca = top.select("name CA")
    ca_pairs = [[int(ca[i]), int(ca[j])] for i in range(4) for j in range(i + 1, 4)]
    spec = canonicalize_feature_spec(
        [{"type": "distance", "atoms": [0, 11]}] + [{"type": "dihedral", "atoms": q.tolist()} for q in np.vstack([phi, psi])]
        + [{"type": "distance", "atoms": p} for p in ca_pairs])
    want = ref.extract(spec, xyz, box, mic="search", dtype=np.float64)
    specs = ["distance_pair(i=0, j=11)", "phi_psi", "contacts_pair(i=0, j=11, rcut=0.5)"]
    X, cols, periodic = compute_features(traj, specs)
    assert X.shape == (64, 8) and len(cols) == 8 and periodic.tolist() == [False] + [True] * 6 + [False]
    assert_within(spec, np.hstack([X[:, :7], want[:, 7:]]), want, tol, "registry")
    d = want[:, 0]
    assert (np.abs(d - 0.5) > 1.0e-4).all()               # no distance sits on the cutoff
    np.testing.assert_array_equal(X[:, 7], (d <= 0.5).astype(float))
    cad = featurize_trajectory(traj, "ca_distances")
    assert_within(spec, np.hstack([want[:, :7], cad]), want, tol, "ca_distances")
    pp = featurize_trajectory(traj, "phi_psi")
    np.testing.assert_array_equal(pp, X[:, 1:7].astype(np.float32))
    # periodic=False, and a trajectory without a cell, give today's numbers exactly
    off = ["distance_pair(i=0, j=11, periodic=False)", "contacts_pair(i=0, j=11, rcut=0.5, periodic=False)"]
    Xo, _, _ = compute_features(traj, off)
    Xb, _, _ = compute_features(bare, [s.replace(", periodic=False", "") for s in off])
    np.testing.assert_array_equal(Xo, Xb)
    assert np.abs(Xo[:, 0] - X[:, 0]).max() > 0.5          # the cell did matter
    np.testing.assert_array_equal(featurize_trajectory(traj, "ca_distances", periodic=False),
                                  featurize_trajectory(bare, "ca_distances"))
    np.testing.assert_array_equal(featurize_trajectory(traj, "phi_psi", periodic=False),
                                  featurize_trajectory(bare, "phi_psi"))
    # the `contacts` feature type of the MSM layer: C-alpha distances of residue pairs >= 3 apart -> (CA0, CA3)
    con = compute_msm_features([traj], feature_type="contacts").features
    assert con.shape == (64, 1)
    assert_within(spec, np.hstack([want[:, :9], con, want[:, 10:]]), want, tol, "contacts")
    con_off = compute_msm_features([traj], feature_type="contacts", periodic=False).features
    np.testing.assert_array_equal(con_off, compute_msm_features([bare], feature_type="contacts").features)
