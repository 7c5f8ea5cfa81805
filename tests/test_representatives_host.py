"""Host side of the representative picker: the numpy restatement against the reference's recorded picks, the
frame lookup / locator arithmetic, every error raised before a device call, and the PDB writer.  No GPU."""

from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from pmarlo_amd.conformations import (RepresentativePicker, TrajectoryFrameLocator, TrajectorySegment,
                                      build_frame_index_lookup)
from pmarlo_amd.io import Topology, Trajectory, load_pdb
from tests import _representatives_ref as R


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("name", [c[0] for c in R.GOLDEN_CASES])
def test_restatement_reproduces_the_reference_picks(golden, name, method):
    g = golden("representatives.npz")
    assert float(g[f"{name}/{method}/margin"]) >= 1e-9
    gold = [tuple(r) for r in g[f"{name}/{method}/picks"].tolist()]
    x, dtrajs, state_ids, weights, n_reps = R.golden_case(name)
    mine = R.pick(x, dtrajs, state_ids, weights, n_reps, method)
    if method == "diverse":
        assert mine == gold
    else:   # the reference's order inside a state is what argpartition leaves
        assert set(mine) == set(gold) and len(mine) == len(gold)
        assert {s: set(v) for s, v in R.by_state(mine).items()} == {s: set(v) for s, v in R.by_state(gold).items()}


def test_lookup_maps_global_to_local():
    lookup = build_frame_index_lookup([np.array([0, 1, 0]), np.array([2, 1])])
    assert np.array_equal(lookup.state_by_global_frame, [0, 1, 0, 2, 1])
    assert np.array_equal(lookup.trajectory_index, [0, 0, 0, 1, 1])
    assert np.array_equal(lookup.local_frame_index, [0, 1, 2, 0, 1])
    assert lookup.to_local_indices(4) == (1, 1)
    assert lookup.n_frames == 5
    assert np.array_equal(lookup.frames_for_state(1), [1, 4])
    with pytest.raises(IndexError, match="out of bounds for lookup of length 5"):
        lookup.to_local_indices(5)


def test_lookup_with_an_empty_trajectory_in_the_middle():
    lookup = build_frame_index_lookup([np.array([3]), np.array([], dtype=int), np.array([4, 5])])
    assert np.array_equal(lookup.trajectory_index, [0, 2, 2])
    assert np.array_equal(lookup.local_frame_index, [0, 0, 1])


def test_lookup_rejects_bad_input():
    with pytest.raises(ValueError, match="non-empty sequence"):
        build_frame_index_lookup([])
    with pytest.raises(ValueError, match="one-dimensional"):
        build_frame_index_lookup([np.zeros((2, 2), dtype=int)])


def test_segment_applies_the_stride_and_the_locator_resolves():
    seg = TrajectorySegment(path=Path("fake.dcd"), start=0, stop=10, local_start=100, local_stride=5)
    other = TrajectorySegment(path=Path("next.dcd"), start=10, stop=12, local_start=0)
    locator = TrajectoryFrameLocator(segments=(seg, other))
    assert locator.resolve(3) == (Path("fake.dcd"), 115)
    assert locator.resolve(11) == (Path("next.dcd"), 1)
    with pytest.raises(IndexError, match="does not map to any known trajectory segment"):
        locator.resolve(12)
    with pytest.raises(ValueError, match="local_stride must be positive"):
        TrajectorySegment(path=Path("fake.dcd"), start=0, stop=1, local_start=0, local_stride=0)


def test_errors_raised_before_any_device_call(tmp_path):
    picker = RepresentativePicker()
    dtrajs = [np.array([0, 1, 0]), np.array([2, 1])]
    x = np.zeros((5, 2))
    with pytest.raises(ValueError, match=r"Feature matrix row count does not match total number of frames \(4 != 5\)"):
        picker.pick_representatives(x[:4], dtrajs, [0])
    with pytest.raises(ValueError, match=r"Weights vector length does not match total number of frames \(3 != 5\)"):
        picker.pick_representatives(x, dtrajs, [0], weights=np.ones(3))
    with pytest.raises(ValueError, match="Method 'medoid' has been renamed"):
        picker.pick_representatives(x, dtrajs, [0], method="medoid")
    with pytest.raises(ValueError, match="Unknown method: nearest"):
        picker.pick_representatives(x, dtrajs, [0], method="nearest")
    with pytest.raises(NotImplementedError, match="at most 256 features"):
        picker.pick_representatives(np.zeros((5, 257)), dtrajs, [0])
    with pytest.raises(ValueError, match="No frames found for state -1"):
        picker.pick_representatives(x, dtrajs, [-1])
    with pytest.raises(ValueError, match="non-empty sequence"):
        picker.pick_representatives(x, [], [0])
    assert picker.pick_representatives(x, dtrajs, []) == []
    with pytest.raises(ValueError, match=r"No states found in committor range \(0.4, 0.6\)"):
        picker.pick_from_committor_range(np.array([0.0, 1.0, 0.9]), x, dtrajs)
    with pytest.raises(ValueError, match="topology_path is required"):
        picker.extract_structures([(0, 0, 0, 0)], None, str(tmp_path), trajectory_locator=TrajectoryFrameLocator(()))
    with pytest.raises(FileNotFoundError, match="required for representative extraction does not exist"):
        picker.extract_structures([(0, 0, 0, 0)], None, str(tmp_path), topology_path=tmp_path / "none.pdb",
                                  trajectory_locator=TrajectoryFrameLocator(()))
    with pytest.raises(IndexError, match="Trajectory index 3 is out of bounds for state 0"):
        picker.extract_structures([(0, 0, 3, 0)], [[]], str(tmp_path))
    with pytest.raises(IndexError, match="Local frame 2 out of bounds for trajectory 0"):
        picker.extract_structures([(0, 0, 0, 2)], [[object()]], str(tmp_path))
    with pytest.raises(ValueError, match="missing trajectory index"):
        picker.extract_structures([(0, 0, None, 0)], [[object()]], str(tmp_path))


class _Frame:
    def __init__(self, text):
        self.text = text

    def save_pdb(self, path):
        Path(path).write_text(self.text)


def test_extract_structures_duck_typed_uses_local_indices(tmp_path):
    trajectories = [[_Frame(f"t0 f{i}") for i in range(3)], [_Frame(f"t1 f{i}") for i in range(3)]]
    saved = RepresentativePicker().extract_structures([(5, 4, 1, 1)], trajectories, str(tmp_path / "structures"),
                                                      prefix="test")
    assert [Path(p).name for p in saved] == ["test_005_000004.pdb"]
    assert Path(saved[0]).read_text() == "t1 f1"


def test_save_pdb_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    top = Topology(["N", "CA", "HD11", "ZN", "O"], ["ALA", "ALA", "LEU", "ZN", "HOH"], np.array([0, 0, 1, 2, 3]),
                   ["A", "A", "A", "B", "B"], np.array([7, 7, 8, 120, 9001]))
    xyz = rng.uniform(-9.0, 9.0, size=(3, 5, 3)).astype(np.float32)
    path = tmp_path / "out.pdb"
    Trajectory(xyz, top).save_pdb(path)
    back = load_pdb(path)
    assert back.n_frames == 3
    assert back.topology.atom_names == top.atom_names
    assert back.topology.res_names == top.res_names
    assert back.topology.chain_ids == top.chain_ids
    assert np.array_equal(back.topology.res_index, top.res_index)
    assert np.array_equal(back.topology.res_seq, top.res_seq)
    assert back.topology.elements == top.elements
    # 8.3f prints Angstrom to 1e-3 (half of it is the rounding); float32 nm adds a few 1e-6 A
    assert np.max(np.abs(back.xyz.astype(np.float64) - xyz.astype(np.float64))) * 10.0 <= 1e-3
    lines = path.read_text().splitlines()
    assert all(len(ln) == 78 for ln in lines if ln.startswith("ATOM")) and lines[-1] == "END"


def test_extract_structures_with_locator_reads_the_strided_frame(tmp_path):
    from pmarlo_amd.io import write_dcd

    rng = np.random.default_rng(8)
    top = Topology(["N", "CA", "C"], ["GLY"] * 3, np.zeros(3, dtype=int), ["A"] * 3)
    xyz = rng.uniform(-2.0, 2.0, size=(7, 3, 3)).astype(np.float32)
    Trajectory(xyz[:1], top).save_pdb(tmp_path / "top.pdb")
    write_dcd(tmp_path / "traj.dcd", xyz)
    # global frames 10 .. 12 are every second frame of the file, from its frame 1 on
    locator = TrajectoryFrameLocator((TrajectorySegment(tmp_path / "traj.dcd", start=10, stop=13, local_start=1,
                                                        local_stride=2),))
    saved = RepresentativePicker().extract_structures([(0, 12, 0, 2), (3, 10, 0, 0)], None, str(tmp_path / "locator"),
                                                      prefix="loc", topology_path=tmp_path / "top.pdb",
                                                      trajectory_locator=locator)
    assert [Path(p).name for p in saved] == ["loc_000_000012.pdb", "loc_003_000010.pdb"]
    for path, frame in zip(saved, (5, 1)):
        back = load_pdb(path)
        assert back.n_frames == 1 and back.topology.atom_names == ["N", "CA", "C"]
        assert np.max(np.abs(back.xyz[0].astype(np.float64) - xyz[frame])) * 10.0 <= 1e-3
    with pytest.raises(IndexError, match="does not map to any known trajectory segment"):
        RepresentativePicker().extract_structures([(0, 13, 0, 0)], None, str(tmp_path / "locator"),
                                                  topology_path=tmp_path / "top.pdb", trajectory_locator=locator)
    with pytest.raises(FileNotFoundError, match="does not exist for state 4"):
        gone = TrajectoryFrameLocator((TrajectorySegment(tmp_path / "gone.dcd", start=0, stop=1, local_start=0),))
        RepresentativePicker().extract_structures([(4, 0, 0, 0)], None, str(tmp_path / "locator"),
                                                  topology_path=tmp_path / "top.pdb", trajectory_locator=gone)
