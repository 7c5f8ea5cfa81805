"""Periodic boundaries on the host (CPU suite): the numpy restatement of the minimum-image extractor against the
reference's outputs (tests/golden/pbc.npz, written by make_golden_pbc.py), the feature-spec canonicaliser against
the reference's metadata and error conditions, cell -> box vectors, and the unit cell's way through Trajectory, the
DCD / PDB loaders and the feature cache key."""

from __future__ import annotations

import json
from types import SimpleNamespace

import numpy as np
import pytest

from pmarlo_amd.api.features import feature_cache_file
from pmarlo_amd.features.deeptica.ts_feature_extractor import (
    FeatureSpecError,
    NormalizedFeatureSpec,
    canonicalize_feature_spec,
)
from pmarlo_amd.io.dcd import iterload, load_dcd, write_dcd
from pmarlo_amd.io.pdb import Topology, Trajectory, cell_to_vectors, load_pdb
from tests import _pbc_ref as ref
from tests.conftest import GOLDEN

SPEC_FIELDS = ("distance_pairs", "distance_positions", "distance_pbc", "angle_triplets", "angle_positions", "angle_pbc",
               "dihedral_quads", "dihedral_positions", "dihedral_pbc", "feature_weights")
KINDS = ("distance", "angle", "dihedral")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "pbc.npz", allow_pickle=False), json.loads((GOLDEN / "pbc.json").read_text())


def kind_errors(spec, got, want) -> dict[str, float]:
    """max |got - want| per kind; dihedrals modulo 2 pi on the unweighted angle, scaled by |weight|."""
    w = np.asarray(spec.feature_weights, np.float64)
    out = {}
    for kind in KINDS:
        pos = np.asarray(getattr(spec, f"{kind}_positions"))
        d = np.asarray(got, np.float64)[:, pos] - np.asarray(want, np.float64)[:, pos]
        if kind == "dihedral":
            d = ref.wrap_to_pi(d / w[pos]) * np.abs(w[pos])
        out[kind] = float(np.abs(d).max()) if d.size else 0.0
    return out


def test_restatement_matches_the_reference_within_the_recorded_values(gold):
    g, meta = gold
    spec = SimpleNamespace(**{k: g[k] for k in SPEC_FIELDS})
    recorded = meta["max_abs_fp32_restatement_minus_reference"]
    for name in meta["boxes"]:
        xyz, box, want = g[f"{name}_xyz"], g[f"{name}_box"], g[f"{name}_out"]
        assert (ref.tie_margin(spec, xyz, box) >= 1.0e-3).all()
        err = kind_errors(spec, ref.extract(spec, xyz, box, mic="round", dtype=np.float32), want)
        err64 = kind_errors(spec, ref.extract(spec, xyz, box, mic="round", dtype=np.float64), want)
        print(name, "fp32", err, "fp64", err64)
        for kind in KINDS:
            assert err[kind] <= recorded[kind], (name, kind, err[kind], recorded[kind])
            assert err64[kind] <= 2.0 * recorded[kind], (name, kind, err64[kind])   # the reference's own fp32 error
    assert all(0.0 < recorded[k] < 1.0e-3 for k in KINDS), recorded


def test_wrapping_matters_in_the_golden_inputs(gold):
    g, meta = gold
    spec = SimpleNamespace(**{k: g[k] for k in SPEC_FIELDS})
    for name in meta["boxes"]:
        plain = ref.extract(spec, g[f"{name}_xyz"], None, dtype=np.float32)
        want = g[f"{name}_out"]
        flagged = np.zeros(want.shape[1], bool)
        for kind in KINDS:
            flagged[g[f"{kind}_positions"][g[f"{kind}_pbc"]]] = True
        assert (np.abs(plain - want)[:, flagged].max(axis=0) > 1.0e-2).all()       # every flagged entry wraps somewhere
        # and no unflagged entry does: dihedral 8 (weight 1) needs no modulo here, both sides come from atan2
        assert np.abs(plain - want)[:, ~flagged].max() <= max(meta["max_abs_fp32_restatement_minus_reference"].values())


def test_canonicalize_reproduces_the_reference_metadata(gold):
    g, meta = gold
    spec = canonicalize_feature_spec(meta["spec"])
    assert isinstance(spec, NormalizedFeatureSpec)
    assert list(spec.feature_names) == meta["feature_names"]
    assert spec.use_pbc is meta["use_pbc"] and spec.atom_count == meta["atom_count"] and spec.n_features == 23
    for k in SPEC_FIELDS:
        got = getattr(spec, k)
        assert got.shape == g[k].shape and got.dtype == g[k].dtype, k
        np.testing.assert_array_equal(got, g[k], err_msg=k)
    # a bare list defaults to pbc on; use_pbc of the result is "any entry flagged"
    bare = canonicalize_feature_spec([{"type": "distance", "indices": (0, 4)}, {"type": "Torsion ", "atoms": [1, 2, 3, 0]}])
    assert bare.use_pbc and bare.feature_names == ("feature_0", "feature_1") and bare.atom_count == 5
    assert bare.distance_pbc.tolist() == [True] and bare.dihedral_positions.tolist() == [1]
    assert bare.angle_triplets.shape == (0, 3) and bare.angle_positions.shape == (0,)
    off = canonicalize_feature_spec({"use_pbc": False, "features": [{"type": "angle", "atoms": [0, 1, 2], "weight": "2.5"}]})
    assert not off.use_pbc and off.feature_weights.tolist() == [2.5] and off.feature_weights.dtype == np.float32
    mixed = canonicalize_feature_spec({"use_pbc": False, "features": [{"type": "angle", "atoms": [0, 1, 2], "pbc": True}]})
    assert mixed.use_pbc and mixed.angle_pbc.tolist() == [True]


@pytest.mark.parametrize("spec, match", [
    ({"use_pbc": True}, "missing 'features'"),
    ({"features": 3}, "must be a sequence"),
    (7, "must be a sequence"),
    ([], "at least one entry"),
    ([["distance", 0, 1]], "must be a mapping"),
    ([{"atoms": [0, 1]}], "missing 'type'"),
    ([{"type": "distance"}], "missing 'atom_indices'"),
    ([{"type": "distance", "atoms": 5}], "sequence of integers"),
    ([{"type": "distance", "atoms": [0, 1], "weight": "heavy"}], "must be numeric"),
    ([{"type": "distance", "atoms": [0, 1], "weight": None}], "must be numeric"),
    ([{"type": "rmsd", "atoms": [0, 1]}], "unsupported feature type"),
    ([{"type": "distance", "atoms": [0, 1, 2]}], "exactly 2"),
    ([{"type": "angle", "atoms": [0, 1]}], "exactly 3"),
    ([{"type": "dihedral", "atoms": [0, 1, 2]}], "exactly 4"),
    ([{"type": "distance", "atoms": [0, -1]}], "non-negative"),
])
def test_canonicalize_error_conditions(spec, match):
    with pytest.raises(FeatureSpecError, match=match):
        canonicalize_feature_spec(spec)
    assert issubclass(FeatureSpecError, ValueError)


def test_box_from_cell_known_answers():
    L = 3.0
    cells = np.array([[2.0, 2.0, 2.0, 90.0, 90.0, 90.0],
                      [2.0, 3.0, 4.0, 90.0, 90.0, 120.0],
                      [L, L, L, 70.53, 109.47, 70.53]])
    box = ref.box_from_cell(cells)
    np.testing.assert_array_equal(box[0], np.diag([2.0, 2.0, 2.0]))          # exactly diagonal: cos 90 is cleaned
    np.testing.assert_allclose(box[1], [[2.0, 0, 0], [-1.5, 1.5 * np.sqrt(3.0), 0], [0, 0, 4.0]], atol=1e-12)
    octa = L * np.array([[1.0, 0, 0], [1 / 3, 2 * np.sqrt(2) / 3, 0], [-1 / 3, np.sqrt(2) / 3, np.sqrt(6) / 3]])
    np.testing.assert_allclose(box[2], octa, atol=2.0e-4 * L)                 # the angles carry two decimals
    inv = ref.inverse_adjugate(box)
    np.testing.assert_allclose(np.einsum("nij,njk->nik", box, inv), np.broadcast_to(np.eye(3), (3, 3, 3)), atol=1e-14)
    np.testing.assert_allclose(inv, np.linalg.inv(box), rtol=1e-13, atol=1e-15)
    # lengths and angles come back
    for b, c in zip(box, cells):
        lengths = np.linalg.norm(b, axis=1)
        np.testing.assert_allclose(lengths, c[:3], rtol=1e-12)
        cosines = [b[1] @ b[2] / (lengths[1] * lengths[2]), b[0] @ b[2] / (lengths[0] * lengths[2]),
                   b[0] @ b[1] / (lengths[0] * lengths[1])]
        np.testing.assert_allclose(np.degrees(np.arccos(cosines)), c[3:], atol=1e-9)
    np.testing.assert_array_equal(cell_to_vectors(cells), box)                # the package's host version


def test_brute_force_agrees_with_rounding_where_rounding_is_right(gold):
    g, meta = gold
    spec = SimpleNamespace(**{k: g[k] for k in SPEC_FIELDS})
    xyz, box = g["ortho_xyz"], g["ortho_box"]
    a = ref.extract(spec, xyz, box, mic="round", dtype=np.float64)
    b = ref.extract(spec, xyz, box, mic="search", dtype=np.float64)
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    # a vector along the long diagonal of a 62-degree cell: rounding keeps a longer image, the brute force does not
    tric = ref.box_from_cell([2.4, 2.6, 2.9, 90.0, 90.0, 62.0])
    v = (0.45 * tric[0, 0] + 0.45 * tric[0, 1])[None, None]
    assert np.linalg.norm(ref.round_image(v, tric)) > np.linalg.norm(ref.brute_min_image(v, tric)[0]) + 0.1


def _traj(n=7, cell=True, seed=0):
    rng = np.random.default_rng(seed)
    top = Topology(["N", "CA", "C", "O"], ["ALA"] * 4, np.zeros(4, dtype=int), ["A"] * 4)
    xyz = rng.uniform(0.0, 2.0, size=(n, 4, 3)).astype(np.float32)
    cells = None
    if cell:
        cells = np.tile([2.4, 2.6, 2.9, 75.0, 98.0, 62.0], (n, 1)) * (1.0 + 0.01 * np.arange(n))[:, None]
    return Trajectory(xyz, top, cells), top


def test_trajectory_without_a_cell():
    traj, top = _traj(cell=False)
    assert traj.unitcell is None and traj.unitcell_lengths is None and traj.unitcell_angles is None
    assert traj.unitcell_vectors is None
    assert Trajectory(traj.xyz, top).unitcell is None             # the two-argument constructor
    assert traj[2:5].unitcell is None and traj[3].unitcell is None


def test_trajectory_cell_views_and_slicing():
    traj, top = _traj()
    cells = traj.unitcell
    assert cells.dtype == np.float64 and cells.shape == (7, 6)
    np.testing.assert_array_equal(traj.unitcell_lengths, cells[:, :3])
    np.testing.assert_array_equal(traj.unitcell_angles, cells[:, 3:])
    np.testing.assert_array_equal(traj.unitcell_vectors, ref.box_from_cell(cells))
    assert traj.unitcell_vectors.shape == (7, 3, 3)
    for view in (traj.unitcell_lengths, traj.unitcell_angles, traj.unitcell_vectors):
        with pytest.raises(ValueError):
            view[0, 0] = 1.0
    np.testing.assert_array_equal(traj[1:6:2].unitcell, cells[1:6:2])
    one = traj[4]
    assert one.n_frames == 1
    np.testing.assert_array_equal(one.unitcell, cells[4:5])
    np.testing.assert_array_equal(traj[[0, 6]].unitcell, cells[[0, 6]])
    with pytest.raises(ValueError, match="unitcell"):
        Trajectory(traj.xyz, top, cells[:3])


def test_cell_survives_dcd_and_pdb(tmp_path):
    traj, top = _traj(n=11)
    p = tmp_path / "cell.dcd"
    write_dcd(p, traj.xyz, traj.unitcell)
    back = load_dcd(p, top=top)
    np.testing.assert_allclose(back.unitcell, traj.unitcell, rtol=1e-15)
    np.testing.assert_allclose(load_dcd(p, top=top, stride=3).unitcell, traj.unitcell[::3], rtol=1e-15)
    chunks = list(iterload(p, top=top, chunk=4))
    assert [c.n_frames for c in chunks] == [4, 4, 3]
    np.testing.assert_allclose(np.concatenate([c.unitcell for c in chunks]), traj.unitcell, rtol=1e-15)
    bare = tmp_path / "bare.dcd"
    write_dcd(bare, traj.xyz)
    assert load_dcd(bare, top=top).unitcell is None and all(c.unitcell is None for c in iterload(bare, top=top, chunk=4))
    # PDB: one CRYST1 record, repeated per model; three decimals of Angstrom and two of a degree survive
    pdb = tmp_path / "cell.pdb"
    traj[:3].save_pdb(pdb)
    assert pdb.read_text().startswith("CRYST1")
    got = load_pdb(pdb)
    assert got.n_frames == 3 and got.unitcell.shape == (3, 6)
    np.testing.assert_allclose(got.unitcell, np.tile(traj.unitcell[0], (3, 1)), atol=5.1e-3)
    np.testing.assert_allclose(got.unitcell[:, :3], np.tile(traj.unitcell[0, :3], (3, 1)), atol=5.1e-5)
    np.testing.assert_allclose(got.xyz, traj.xyz[:3], atol=5.1e-5)
    nocell = tmp_path / "nocell.pdb"
    Trajectory(traj.xyz[:2], top).save_pdb(nocell)
    assert "CRYST1" not in nocell.read_text() and load_pdb(nocell).unitcell is None


def test_cache_key_follows_the_cell(tmp_path):
    traj, top = _traj()
    plain = Trajectory(traj.xyz, top)
    specs = ["phi_psi"]
    key_plain = feature_cache_file(plain, specs, str(tmp_path))
    key_cell = feature_cache_file(traj, specs, str(tmp_path))
    other = Trajectory(traj.xyz, top, traj.unitcell * 1.001)
    assert key_cell != key_plain and feature_cache_file(other, specs, str(tmp_path)) != key_cell
    assert feature_cache_file(Trajectory(traj.xyz, top, traj.unitcell.copy()), specs, str(tmp_path)) == key_cell
    # the key of a cell-less trajectory is the one from before cells existed: an object without the attribute at all
    legacy = SimpleNamespace(xyz=plain.xyz, topology=top, n_frames=plain.n_frames, n_atoms=plain.n_atoms)
    assert feature_cache_file(legacy, specs, str(tmp_path)) == key_plain
