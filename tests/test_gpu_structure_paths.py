"""The three kernels of csrc/structure.hip (Shrake-Rupley SASA, Baker-Hubbard presence, Kabsch-Sander DSSP) on every
launch path, against the fp32 oracle (oracle/npport.py, exact equality: the same operations in the same order) and
against the float64 brackets of tests/_structure_ref.py, which do not depend on the order of operations.  What the
oracle itself gives on geometries whose answer is known (sheets, a bulge, G / I helices, prolines, chain breaks,
chignolin) is pinned on the CPU in tests/test_structure_oracle.py.

Paths (n_cu is read from the engine):
  DSSP   one lane per frame, 64 per workgroup: n = 1, 63, 64 (one full wave), 65 (a second workgroup with one lane),
         130 (two full waves and a partial one); neighbouring lanes hold different folds, a jittered copy and the
         all-zero frame, so the lanes diverge in the ladder loops; host frame chunks (MSM_DSSP_CHUNK = 64 at n = 150:
         launches of 64, 64 and 22 frames); every residue count at which a loop bound first admits an iteration
         (R = 1, 2, 4, 5, 6, 7; R = 0 is empty); backbone rows with -1; prolines at both ends.
  SASA   P = 1, 63, 64, 65, 100, 960 bit for bit; P = 2048, 4096 (LDS above 48 KiB: the opt-in) bit for bit and
         inside the float64 bracket; P = 4097 refused; the grid-stride loop (n A > 32 n_cu items); A = 1, 64, 65;
         exactly 384 neighbours (the list is full) and 385 (refused, and the next call is served).
  H-bond n = 1 ... 257 frames (frame chunks of 16 or 17 with different counts); Tn = 1, 255, 256, 257;
         Tn = 262144 + 5 (the triplet grid-stride); Tn = 0, n = 0; the all-zero frame and D = H.

Frozen inputs and measured shares (CPU, asserted in tests/test_structure_oracle.py):
  sheet placements (rotation about the strand axis, shift along it, separation): parallel (15 deg, 0.0 A, 4.8 A),
    antiparallel (15 deg, -1.0 A, 4.8 A); 114 and 394 placements of the sweep give 0EEEEEE0 | 0EEEEEE0;
  DSSP frames ambiguous by the float64 energy table (|E + 0.5| < 2e-3 or |CA - CA| within 1e-4 A of 9 A): 27 of 1350
    (2.0 %), per group at most 6 of 150 (4 %); the bound on excluded frames is 5 %;
  SASA points within 1e-5 nm of a neighbour's surface: 1 of 115200 on the cloud (A = 120, box 1.2 nm, P = 960);
  hydrogen-bond cases within 1e-6 nm / 1e-5 rad of a cutoff: 0 for every n of the frame-chunk test.

Found by these tests and fixed (structure features): a NaN cosine (D = H, H = A, coincident CA atoms: the
all-zero frame) was clamped to -1 by fminf(fmaxf()) and counted as a 180 degree bond / bend where mdtraj's np.clip
keeps the NaN and counts nothing; the oracle's min() over the four distances of an energy dropped the < 0.5 A rule
when the hydrogen position is NaN, where dssp.cpp tests each distance on its own."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import npport

from . import _structure_gen as sg
from . import _structure_ref as sref
from .test_structure_oracle import _water_free_dipeptide

pytestmark = pytest.mark.gpu

ACUT = np.float32(2 * np.pi / 3)


@pytest.fixture(scope="module")
def chig(golden):
    return golden("chignolin.npz")


# ---------------------------------------------------------------------------------------------------------
# DSSP
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dssp_cases(chig):
    """name -> (frames [150, A, 3], table, chain, proline, oracle codes [150, R]); the oracle runs once per group and
    the tests take prefixes (the frames are independent of each other)."""
    out = {}
    for name, grp in sg.dssp_groups(chig).items():
        frames = sg.dssp_frames(grp)
        out[name] = (frames, grp[1], grp[2], grp[3], npport.dssp_codes(frames, grp[1], grp[2], grp[3]))
    return out


def _assert_dssp(got, want, frames, bb, chain, pro, tag):
    """Exact equality with the oracle; a differing frame is excused only if the float64 table shows it ambiguous, and
    at most 5 % of the frames."""
    assert got.shape == want.shape and got.dtype == np.uint8, tag
    bad = np.nonzero((got != want).any(axis=1))[0]
    for t in bad:
        assert sref.dssp_frame_ambiguous(frames[t], bb, chain, pro), (tag, int(t), got[t], want[t])
    assert len(bad) <= 0.05 * len(want), (tag, bad)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_dssp_full_and_partial_waves(engine, dssp_cases, n):
    seen = set()
    for name, (frames, bb, chain, pro, want) in dssp_cases.items():
        got = engine.dssp(engine.to_device(frames[:n]), bb, chain, pro)
        _assert_dssp(got, want[:n], frames, bb, chain, pro, (name, n))
        seen |= set(np.unique(got).tolist())
    if n >= 63:        # the frames reach every code: sheets, bridges, the three helices, turns and bends
        assert seen == set(range(8)), seen


def test_dssp_known_folds(engine, chig):
    """The kernel's codes on geometries whose answer is stated (and derived in tests/test_structure_oracle.py), one call
    per residue count: E on residues 1 ... 6 of both strands of a parallel and an antiparallel pair, one ladder joined
    across the inserted residue of the bulge, G and I and H helices, no H across a stretched bond or a change of chain,
    strand - turn - strand on chignolin's first model."""
    E8 = [0, 3, 3, 3, 3, 3, 3, 0]
    bb, chain, pro = sg.sheet_tables()
    sheets = np.stack([sg.two_strands("parallel"), sg.two_strands("antiparallel")]).astype(np.float32)
    assert engine.dssp(engine.to_device(sheets), bb, chain, pro).tolist() == [E8 + E8, E8 + E8]
    bb, chain, pro = sg.sheet_tables(8, 9)
    got = engine.dssp(engine.to_device(sg.bulge().astype(np.float32)[None]), bb, chain, pro)
    assert got[0].tolist() == E8 + [0, 3, 3, 3, 3, 3, 3, 3, 0]
    bb, chain, pro = sg.table(12)
    helices = np.stack([sg.helix(12, pp) for pp in (sg.ALPHA, sg.HELIX_310, sg.HELIX_PI)]).astype(np.float32)
    got = engine.dssp(engine.to_device(helices), bb, chain, pro)
    assert got.tolist() == [[0] + [c] * 10 + [0] for c in (1, 4, 5)]
    bb, chain, pro = sg.table(14)
    broken = np.stack([sg.helix(14), sg.helix(14, stretch_after=6)]).astype(np.float32)
    cut = [0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0]
    assert engine.dssp(engine.to_device(broken), bb, chain, pro).tolist() == [[0] + [1] * 12 + [0], cut]
    chain[7:] = 1
    assert engine.dssp(engine.to_device(broken), bb, chain, pro).tolist() == [cut, cut]
    got = engine.dssp(engine.to_device(chig["xyz"]), chig["backbone"], chig["chain"], chig["proline"])
    np.testing.assert_array_equal(got, chig["dssp_codes"])
    assert got[0].tolist() == [0, 3, 3, 6, 6, 6, 6, 3, 3, 0]


def test_dssp_neighbouring_lanes_hold_different_folds(dssp_cases):
    """What makes the runs above a test of divergent lanes: within every group the oracle's codes of frame t and t + 1
    differ for about half of the t or more, and the all-zero frames are among them."""
    for name, (frames, bb, chain, pro, want) in dssp_cases.items():
        differ = (want[1:] != want[:-1]).any(axis=1)
        assert differ.mean() > 0.4, (name, differ.mean())
        assert not frames[2].any() and not frames[8].any() and frames[5].any()


@pytest.mark.parametrize("chunk,launches", [("64", (64, 64, 22)), ("100", (128, 22)), ("1", (64, 64, 22))])
def test_dssp_frame_chunks(engine, dssp_cases, monkeypatch, chunk, launches):
    """The host loop over frame chunks: the scratch is laid out per launch ([array][residue][frame of the launch]) and
    the frame and code pointers advance by the chunk.  The seam is clamped to at least 64 and rounded up to a multiple
    of 64."""
    assert sum(launches) == sg.DSSP_N_MAX
    for name in ("chignolin", "bulge", "helices"):
        frames, bb, chain, pro, want = dssp_cases[name]
        xd = engine.to_device(frames)
        monkeypatch.delenv("MSM_DSSP_CHUNK", raising=False)
        whole = engine.dssp(xd, bb, chain, pro)
        monkeypatch.setenv("MSM_DSSP_CHUNK", chunk)
        got = engine.dssp(xd, bb, chain, pro)
        np.testing.assert_array_equal(got, whole)
        _assert_dssp(got, want, frames, bb, chain, pro, (name, chunk))


@pytest.mark.parametrize("R", [1, 2, 4, 5, 6, 7])
def test_dssp_small_residue_counts(engine, chig, R):
    """R at which the loops first run: turns need i + 3 < R, bends i + 2 < R with i >= 2, helices and bridges
    i + 4 < R with i >= 1, pi helices i + 5 < R."""
    bb, chain, pro = sg.table(R)
    folded = np.stack([sg.helix(R, pp) for pp in (sg.ALPHA, sg.HELIX_310, sg.HELIX_PI)]).astype(np.float32)
    frames = sg.interleave(folded, 40 + R, 18)
    got = engine.dssp(engine.to_device(frames), bb, chain, pro)
    _assert_dssp(got, npport.dssp_codes(frames, bb, chain, pro), frames, bb, chain, pro, ("helices", R))
    # the first R residues of the hairpin (138 atoms, a table that is no arange), and of it with a proline
    frames = sg.interleave(chig["xyz"], 50 + R, 18)
    for p in (np.zeros(R, np.uint8), (np.arange(R) == R // 2).astype(np.uint8)):
        got = engine.dssp(engine.to_device(frames), chig["backbone"][:R], chig["chain"][:R], p)
        want = npport.dssp_codes(frames, chig["backbone"][:R], chig["chain"][:R], p)
        _assert_dssp(got, want, frames, chig["backbone"][:R], chig["chain"][:R], p, ("chignolin", R))


def test_dssp_without_residues_or_frames(engine):
    xd = engine.to_device(np.zeros((3, 8, 3), np.float32))
    got = engine.dssp(xd, np.zeros((0, 4), np.int32), [], [])
    assert got.shape == (3, 0) and got.dtype == np.uint8
    bb, chain, pro = sg.table(2)
    assert engine.dssp(engine.to_device(np.zeros((0, 8, 3), np.float32)), bb, chain, pro).shape == (0, 2)


@pytest.mark.parametrize("rows", [[6], [0], [13], [6, 7], [0, 13], list(range(14))],
                         ids=["middle", "first", "last", "two-in-a-row", "both-ends", "all"])
def test_dssp_incomplete_backbone_rows(engine, dssp_cases, rows):
    """A row with a -1 (any of the four atoms): never bonded, a chain break, code 0, and no atom -1 is read."""
    frames, bb, chain, pro, _ = dssp_cases["stretched"]
    frames = frames[:66]
    xd = engine.to_device(frames)
    for col in range(4):
        holed = bb.copy()
        holed[rows, col] = -1
        got = engine.dssp(xd, holed, chain, pro)
        want = npport.dssp_codes(frames, holed, chain, pro)
        _assert_dssp(got, want, frames, holed, chain, pro, (rows, col))
        assert (got[:, rows] == 0).all()
    with pytest.raises(ValueError):
        bad = bb.copy()
        bad[3, 1] = -2
        engine.dssp(xd, bad, chain, pro)


# ---------------------------------------------------------------------------------------------------------
# SASA
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud120():
    return sg.cloud(2, 120, 1.2, 5)


def _sasa(engine, xyz, radii, P):
    return engine.featurize_sasa(engine.to_device(xyz), radii, npport.sasa_sphere_points(P)).to_host()


@pytest.mark.parametrize("P", [1, 63, 64, 65, 100, 960])
def test_sasa_point_counts_bit_for_bit(engine, cloud120, P):
    xyz, radii = cloud120
    got = _sasa(engine, xyz, radii, P)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, npport.shrake_rupley_atoms(xyz, radii, P))


@pytest.mark.parametrize("P", [2048, 4096])
def test_sasa_many_points_take_the_lds_opt_in(engine, cloud120, P):
    """4 x 384 neighbours x 16 B + 12 P B of LDS: 49152 B at P = 2048, above the 48 KiB a kernel gets unasked."""
    assert 4 * 384 * 16 + 12 * P > 48 * 1024 - 1
    xyz, radii = cloud120[0][:1], cloud120[1]
    got = _sasa(engine, xyz, radii, P)
    np.testing.assert_array_equal(got, npport.shrake_rupley_atoms(xyz, radii, P))
    lo, hi, n_amb = sref.sasa_bracket(xyz, radii, npport.sasa_sphere_points(P))
    counts = sref.sasa_counts(got, radii, P)
    assert n_amb <= 1e-3 * counts.size * P, n_amb
    assert (lo <= counts).all() and (counts <= hi).all(), np.nonzero((counts < lo) | (counts > hi))
    # afterwards a small P is served as before
    np.testing.assert_array_equal(_sasa(engine, xyz, radii, 64), npport.shrake_rupley_atoms(xyz, radii, 64))


def test_sasa_refuses_more_than_4096_points(engine, cloud120):
    xyz, radii = cloud120
    xd = engine.to_device(xyz)
    with pytest.raises(ValueError):
        engine.featurize_sasa(xd, radii, np.zeros((4097, 3), np.float32))
    with pytest.raises(ValueError):
        engine.featurize_sasa(xd, radii, np.zeros((0, 3), np.float32))
    np.testing.assert_array_equal(_sasa(engine, xyz, radii, 63), npport.shrake_rupley_atoms(xyz, radii, 63))


def test_sasa_grid_stride(engine):
    """More (frame, atom) items than the grid has waves (8 n_cu workgroups of 4): every wave takes a second item.  Eight
    distinct frames in a permuted tiling, so that an item computed from the wrong frame or atom shows."""
    n_cu = engine.info()["n_cu"]
    A, P = 230, 96
    xyz8, radii = sg.cloud(8, A, 1.5, 17)
    n = max(40, -(-32 * n_cu // A) + 5)
    order = np.random.default_rng(3).permutation(n) % 8
    assert n * A > 32 * n_cu and len(set(order[:8].tolist())) > 3
    want8 = npport.shrake_rupley_atoms(xyz8, radii, P)
    got = _sasa(engine, xyz8[order], radii, P)
    np.testing.assert_array_equal(got, want8[order])
    lo, hi, _ = sref.sasa_bracket(xyz8[:1], radii, npport.sasa_sphere_points(P))
    counts = sref.sasa_counts(got[order == 0], radii, P)
    assert (lo <= counts).all() and (counts <= hi).all()


@pytest.mark.parametrize("A", [1, 64, 65])
def test_sasa_atom_counts_around_one_wave(engine, A):
    xyz, radii = sg.cloud(3, A, 0.9, 23 + A)
    got = _sasa(engine, xyz, radii, 100)
    np.testing.assert_array_equal(got, npport.shrake_rupley_atoms(xyz, radii, 100))
    if A == 1:
        np.testing.assert_allclose(got[:, 0], 4 * np.pi * float(radii[0]) ** 2, rtol=1e-6)


def _shell(n_shell):
    """The atom at the origin with n_shell atoms 0.05 nm from it (every radius 0.3 nm: each atom is a neighbour of each
    other one), and three atoms far away that are nobody's neighbour."""
    xyz = sg.shell_cluster(n_shell)
    far = np.float32([[[5, 0, 0], [0, 6, 0], [5, 5, 5]]])
    return np.concatenate([xyz[:, :200], far[:, :2], xyz[:, 200:], far[:, 2:]], axis=1), np.full(n_shell + 4, np.float32(0.3))


def test_sasa_neighbour_list_full_and_overflowing(engine, cloud120):
    """384 neighbours fill the list exactly; 385 are refused (a handled error: the list writes are guarded), and the
    engine serves the next call."""
    P = 96
    xyz, radii = _shell(384)
    d = np.linalg.norm(xyz[0, :, None, :] - xyz[0, None, :, :], axis=2)
    assert (((d < 0.6) & (d > 0)).sum(axis=1)[[0, 1, 250]] == 384).all() and (d[d > 0] > 1e-3).all()
    want = npport.shrake_rupley_atoms(xyz, radii, P)
    assert want[0, 0] == 0.0 and (want[0, 1:] > 0).sum() > 100            # the centre is buried, the shell is not
    np.testing.assert_array_equal(_sasa(engine, xyz, radii, P), want)
    over, radii_over = _shell(385)
    with pytest.raises(NotImplementedError, match="384"):
        _sasa(engine, over, radii_over, P)
    np.testing.assert_array_equal(_sasa(engine, xyz, radii, P), want)
    np.testing.assert_array_equal(_sasa(engine, cloud120[0], cloud120[1], P),
                                  npport.shrake_rupley_atoms(cloud120[0], cloud120[1], P))


# ---------------------------------------------------------------------------------------------------------
# hydrogen bonds
# ---------------------------------------------------------------------------------------------------------
def _assert_hbonds(engine, frames, trip):
    got = engine.hbond_presence(engine.to_device(frames), trip, 0.25, ACUT)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, npport.baker_hubbard_presence(frames, trip))
    lo, hi, n_amb = sref.hbond_bracket(frames, trip)
    assert n_amb <= 0.01 * max(1, len(frames) * len(trip)), n_amb
    assert (lo <= got).all() and (got <= hi).all(), np.nonzero((got < lo) | (got > hi))
    return got


@pytest.mark.parametrize("n", [1, 15, 16, 31, 32, 33, 100, 257])
def test_hbond_frame_chunks(engine, chig, n):
    """Frame chunks of at least 16 frames: one chunk below n = 32, two at 32 and 33, 6 at 100, 16 at 257 (with 420
    triplets).  Frames 16 ... 31 of every 48 hold no bond at all, so a chunk that is skipped, counted twice or cut at
    the wrong frame changes the sums."""
    got = _assert_hbonds(engine, sg.hbond_frames(chig["xyz"], n), chig["triplets"])
    assert got.sum() > 0


@pytest.mark.parametrize("Tn", [1, 255, 256, 257])
def test_hbond_triplet_counts_around_one_workgroup(engine, chig, Tn):
    trip = chig["triplets"][np.random.default_rng(9).permutation(420)]
    bonded = np.nonzero(chig["hbond_presence"][np.random.default_rng(9).permutation(420)])[0]
    trip[[0, 254, 255, 256]] = trip[bonded[:4]]                # bonded triplets at the edges of the workgroup
    got = _assert_hbonds(engine, chig["xyz"], trip[:Tn])
    assert got[0] > 0 and got[-1] > 0


def test_hbond_triplet_grid_stride(engine):
    """More triplets than 1024 workgroups of 256 lanes: the last five belong to lanes 0 ... 4 on their second turn.
    Random index triplets over 6 atoms, degenerate ones (D = H, H = A, D = A) included."""
    Tn = 262144 + 5
    xyz = _water_free_dipeptide().xyz[:2].copy()
    xyz[1, 3] = [0.12, 0.17, 0.0]
    rng = np.random.default_rng(21)
    trip = rng.integers(0, 6, size=(Tn, 3))
    trip[-5:] = [[0, 1, 3], [0, 1, 4], [0, 1, 3], [2, 1, 3], [0, 1, 3]]
    got = _assert_hbonds(engine, xyz, trip)
    assert got[-5:].tolist() == npport.baker_hubbard_presence(xyz, trip[-5:]).tolist() and got[-1] == 1 and got[-5] == 1
    degenerate = (trip[:, 0] == trip[:, 1]) | (trip[:, 1] == trip[:, 2]) | (trip[:, 0] == trip[:, 2])
    assert degenerate.sum() > Tn // 3 and not got[degenerate].any()
    assert got[~degenerate].sum() > 500


def test_hbond_without_triplets_or_frames(engine, chig):
    xd = engine.to_device(chig["xyz"])
    got = engine.hbond_presence(xd, np.zeros((0, 3), int), 0.25, ACUT)
    assert got.shape == (0,) and got.dtype == np.int64
    empty = engine.to_device(np.zeros((0, 138, 3), np.float32))
    np.testing.assert_array_equal(engine.hbond_presence(empty, chig["triplets"], 0.25, ACUT), np.zeros(420, np.int64))


def test_degenerate_frames_hold_no_bond_and_no_bend(engine, chig):
    """0 / 0 in the cosine: the all-zero frame, and D = H.  mdtraj's clip keeps the NaN and the comparison is false."""
    zero = np.zeros((3, 138, 3), np.float32)
    got = _assert_hbonds(engine, zero, chig["triplets"])
    assert not got.any()
    same = np.array(chig["xyz"][:5])
    same[:, chig["triplets"][:, 1]] = same[:, chig["triplets"][:, 0]]              # every hydrogen onto its donor
    got = _assert_hbonds(engine, same, chig["triplets"])
    assert not got.any()
    mixed = np.concatenate([chig["xyz"][:2], zero[:1], chig["xyz"][2:4]])
    got = _assert_hbonds(engine, mixed, chig["triplets"])
    np.testing.assert_array_equal(got, npport.baker_hubbard_presence(chig["xyz"][:4], chig["triplets"]))
    for R in (7, 10, 16):
        bb, chain, pro = sg.table(R)
        z = np.zeros((2, 4 * R, 3), np.float32)
        codes = engine.dssp(engine.to_device(z), bb, chain, pro)
        np.testing.assert_array_equal(codes, npport.dssp_codes(z, bb, chain, pro))
        assert not (codes == 7).any()
