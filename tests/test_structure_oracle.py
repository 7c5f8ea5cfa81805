"""CPU checks of the structure-feature restatements (oracle/npport.py: Shrake-Rupley, Baker-Hubbard, DSSP) against
closed forms and constructed geometries (sheets, a bulge, the three helix types, prolines, chain breaks, the chignolin
hairpin of tests/golden/chignolin.npz), of the float64 references the GPU tests judge with (tests/_structure_ref.py), and
of the host logic of pmarlo_amd.features.structure (bond triplets, backbone tables).  mdtraj is absent from the build container, so these algorithms are parity-unpinned restatements
(S/features/builtins.py:171-250 is the call site they serve)."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import npport
from pmarlo_amd.features import structure as st
from pmarlo_amd.io.pdb import Topology, Trajectory, load_pdb


def test_sphere_points_are_on_the_unit_sphere_and_cover_it():
    p = npport.sasa_sphere_points(960)
    assert p.shape == (960, 3) and p.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(p.astype(np.float64), axis=1), 1.0, atol=2e-7)
    assert abs(p.astype(np.float64).mean(axis=0)).max() < 2e-3          # evenly spread
    np.testing.assert_array_equal(p, st.sphere_points(960))


def test_sasa_closed_forms():
    R = np.float32(0.17 + 0.14)
    one = npport.shrake_rupley_atoms(np.zeros((1, 1, 3), np.float32), [R])
    np.testing.assert_allclose(one[0, 0], 4 * np.pi * float(R) ** 2, rtol=1e-6)
    # two equal spheres at distance d: each loses the cap of height R - d / 2
    d = 0.4
    two = npport.shrake_rupley_atoms(np.array([[[0, 0, 0], [d, 0, 0]]], np.float32), [R, R])
    exact = 4 * np.pi * float(R) ** 2 - 2 * np.pi * float(R) * (float(R) - d / 2)
    np.testing.assert_allclose(two[0], exact, rtol=6e-3)                  # 960 points: a few per mille
    # far apart: untouched; one inside the other: the inner one is buried
    far = npport.shrake_rupley_atoms(np.array([[[0, 0, 0], [5, 0, 0]]], np.float32), [R, R])
    np.testing.assert_allclose(far[0], one[0, 0], rtol=1e-6)
    nested = npport.shrake_rupley_atoms(np.array([[[0, 0, 0], [0.01, 0, 0]]], np.float32), [0.2, 0.5])
    assert nested[0, 0] == 0.0 and nested[0, 1] == pytest.approx(4 * np.pi * 0.25, rel=1e-6)


def test_residue_sums_follow_atom_order():
    areas = np.arange(12, dtype=np.float32).reshape(2, 6)
    res = np.array([0, 0, 1, 2, 2, 2])
    out = st.residue_sums(areas, res, 3)
    np.testing.assert_array_equal(out, [[1, 2, 12], [13, 8, 30]])
    assert out.dtype == np.float32


def _water_free_dipeptide():
    # N-H ... O=C geometry along x: donor N at 0, H at 0.1, acceptor O at 0.29 (H...O 0.19 nm, angle 180 degrees),
    # a second acceptor off-axis (angle ~ 90 degrees), and a carbon that is never an acceptor
    names = ["N", "H", "CA", "O", "O2", "C"]
    top = Topology(names, ["GLY", "GLY", "GLY", "ALA", "ALA", "ALA"], np.array([0, 0, 0, 1, 1, 1]), ["A"] * 6,
                   elements=["N", "H", "C", "O", "O", "C"])
    xyz = np.array([[[0, 0, 0], [0.1, 0, 0], [-0.1, 0.1, 0], [0.29, 0, 0], [0.1, 0.2, 0], [0.4, 0, 0]]], np.float32)
    return Trajectory(np.repeat(xyz, 5, axis=0), top)


def test_hbond_triplets_and_presence_oracle():
    traj = _water_free_dipeptide()
    trip = st.hbond_triplets(traj)
    # one N-H donor; acceptors N, O, O2 minus the donor itself
    np.testing.assert_array_equal(trip, [[0, 1, 3], [0, 1, 4]])
    counts = npport.baker_hubbard_presence(traj.xyz, trip)
    np.testing.assert_array_equal(counts, [5, 0])        # the off-axis oxygen fails the angle (and the distance)
    # bend the bond in two of the frames: H ... O stays short, the angle drops below 120 degrees
    xyz = traj.xyz.copy()
    xyz[:2, 3] = [0.12, 0.17, 0.0]
    counts = npport.baker_hubbard_presence(xyz, trip)
    assert counts[0] == 3


def _ideal_helix(n_res):
    """Backbone of an ideal alpha helix (phi -57, psi -47): N, CA, C, O per residue, nm."""
    # per-residue cylindrical coordinates of N, CA, C, O for an alpha helix: radius (A), angle offset (deg), rise (A)
    cyl = {"N": (1.55, -27.0, -0.93), "CA": (2.28, 0.0, 0.0), "C": (1.66, 26.0, 1.07), "O": (1.98, 30.0, 2.28)}
    pts = []
    for r in range(n_res):
        for nm in ("N", "CA", "C", "O"):
            rad, ang, z = cyl[nm]
            th = np.radians(100.0 * r + ang)
            pts.append([rad * np.cos(th), rad * np.sin(th), 1.5 * r + z])
    return (np.asarray(pts, np.float32) / 10.0)[None]


def test_dssp_oracle_on_an_ideal_helix_and_a_straight_strand():
    n_res = 16
    xyz = _ideal_helix(n_res)
    bb = np.arange(4 * n_res).reshape(n_res, 4)
    codes = npport.dssp_codes(xyz, bb, np.zeros(n_res, int), np.zeros(n_res, bool))[0]
    assert (codes[1:-1] == 1).sum() >= n_res - 4, codes       # H everywhere but the caps
    assert codes[0] != 1 and codes[-1] != 1
    # a fully extended single strand has no partner: no bridge, no helix
    ext = np.zeros((1, 4 * n_res, 3), np.float32)
    for r in range(n_res):
        s = 1.0 if r % 2 == 0 else -1.0
        ext[0, 4 * r + 0] = [0.38 * r - 0.12, 0.03 * s, 0]
        ext[0, 4 * r + 1] = [0.38 * r, 0.06 * s, 0]
        ext[0, 4 * r + 2] = [0.38 * r + 0.13, 0.02 * s, 0]
        ext[0, 4 * r + 3] = [0.38 * r + 0.15, -0.10 * s, 0]
    codes = npport.dssp_codes(ext, bb, np.zeros(n_res, int), np.zeros(n_res, bool))[0]
    assert not np.isin(codes, [1, 2, 3, 4, 5]).any(), codes


def test_backbone_table_keeps_protein_residues_with_a_full_backbone(golden, tmp_path):
    g = golden("real_assets.npz")
    (tmp_path / "p.pdb").write_bytes(bytes(g["pdb_text"]))
    traj = load_pdb(tmp_path / "p.pdb")
    keep, table, chain, proline = st.backbone_table(traj.topology)
    assert len(keep) == len(g["pdb_ca"]) == 223 and table.shape == (223, 4)
    np.testing.assert_array_equal(table[:, 1], g["pdb_ca"])
    names = np.asarray(traj.topology.atom_names)
    assert (names[table[:, 0]] == "N").all() and (names[table[:, 3]] == "O").all()
    assert proline.sum() == sum(traj.topology.res_names[a] == "PRO" for a in table[:, 1])


def test_dssp_oracle_on_the_reference_asset_is_mostly_helix(golden, tmp_path):
    """3GD8 (aquaporin-4) is an alpha-helical membrane protein: the PDB header lists eight helices."""
    g = golden("real_assets.npz")
    (tmp_path / "p.pdb").write_bytes(bytes(g["pdb_text"]))
    traj = load_pdb(tmp_path / "p.pdb")
    keep, table, chain, proline = st.backbone_table(traj.topology)
    codes = npport.dssp_codes(traj.xyz[:1], table, chain, proline)[0]
    helix = np.isin(codes, [1, 4, 5]).mean()
    sheet = np.isin(codes, [2, 3]).mean()
    assert 0.55 < helix < 0.85 and sheet < 0.08, (helix, sheet)


def test_feature_registry_has_the_structure_features():
    from pmarlo_amd.features.base import get_feature, parse_feature_spec

    for name in ("sasa", "hbonds_count", "ssfrac"):
        assert get_feature(name).name == name
    assert parse_feature_spec("hbonds:all") == ("hbonds_count", {})
    assert parse_feature_spec("secondary:dssp") == ("ssfrac", {})
    assert parse_feature_spec("sasa") == ("sasa", {})


# ---------------------------------------------------------------------------------------------------------
# DSSP on geometries whose answer is known (tests/_structure_gen.py), the float64 references of
# tests/_structure_ref.py against the fp32 oracle, and degenerate frames.
#
# Sheet placements (rotation of the separation direction about the strand axis, shift along it, separation), from the
# sweep of _structure_gen.search_sheet_placement with npport.dssp_codes (rotation in 15 degree steps, shift in
# 0.5 Angstrom steps, separation 4.6, 4.8, 5.0, 5.2 Angstrom; about 30 s, so the sweep itself is no test): 114
# placements give 0EEEEEE0 | 0EEEEEE0 for the parallel pair (rotation 15 and 30 degrees, shift -1.5 ... 1.5 at 4.6) and
# 394 for the antiparallel pair.  Frozen, from the inside of the two regions: parallel (15, 0.0, 4.8), antiparallel
# (15, -1.0, 4.8).  The test below walks the sweep-grid neighbours of each (parallel: towards rotation 30, rotation 0
# is outside the region).
# ---------------------------------------------------------------------------------------------------------
from . import _structure_gen as sg  # noqa: E402
from . import _structure_ref as sref  # noqa: E402


def _codes1(frame, bb, chain, pro):
    return npport.dssp_codes(np.asarray(frame, np.float32)[None], bb, chain, pro)[0]


@pytest.fixture(scope="module")
def chig(golden):
    return golden("chignolin.npz")


@pytest.mark.parametrize("kind", ["parallel", "antiparallel"])
def test_dssp_oracle_two_strand_sheets_are_E(kind):
    """Kabsch-Sander: a ladder of consecutive bridges is E on both strands; the end residues cannot be tested for a
    bridge (TestBridge needs i - 1 and i + 1 on the same chain) and stay 0."""
    bb, chain, pro = sg.sheet_tables()
    want = [0, 3, 3, 3, 3, 3, 3, 0] * 2
    assert _codes1(sg.two_strands(kind), bb, chain, pro).tolist() == want
    # the frozen placement is no lucky corner of the sweep: its neighbours on the sweep grid give the same codes
    rot, shift, sep = sg.SHEET_PLACEMENT[kind]
    for dr in ((0.0, 15.0) if kind == "parallel" else (-15.0, 0.0, 15.0)):
        for ds in (-0.5, 0.0, 0.5):
            for dd in (-0.2, 0.0, 0.2):
                xyz = sg.two_strands(kind, (rot + dr, shift + ds, sep + dd))
                assert _codes1(xyz, bb, chain, pro).tolist() == want, (dr, ds, dd)
    # one strand alone, and the pair pulled apart, have no partner
    assert not np.isin(_codes1(sg.two_strands(kind)[:32], *sg.table(8)), [2, 3]).any()
    assert not np.isin(_codes1(sg.two_strands(kind, (rot, shift, 8.0)), bb, chain, pro), [2, 3]).any()


def test_dssp_oracle_sheet_types_are_told_apart():
    """The two-chain tables joined into one chain change nothing for a sheet, but a parallel pair read with the second
    strand's residues reversed is no sheet: parallel and antiparallel bridges are different bond patterns."""
    bb, chain, pro = sg.sheet_tables()
    xyz = sg.two_strands("parallel")
    rev = bb.copy()
    rev[8:] = bb[8:][::-1]
    assert not np.array_equal(_codes1(xyz, rev, chain, pro), _codes1(xyz, bb, chain, pro))


def test_dssp_oracle_bulge_joins_two_ladders():
    """One residue inserted in the second strand splits the antiparallel ladder in two (the partner index jumps by 2);
    DSSP joins ladders across a gap of fewer than 3 residues on one strand, and the joined ladder covers the inserted
    residue, which has no bridge of its own: E on it is the bulge rule and nothing else."""
    bb, chain, pro = sg.sheet_tables(8, 9)
    codes = _codes1(sg.bulge(), bb, chain, pro)
    assert codes.tolist() == [0, 3, 3, 3, 3, 3, 3, 0] + [0, 3, 3, 3, 3, 3, 3, 3, 0]
    assert codes[8 + sg.BULGE_AT] == 3
    # a chain break next to the inserted residue forbids the join: the inserted residue is no E any more
    cut = chain.copy()
    cut[8 + sg.BULGE_AT:] = 2
    assert _codes1(sg.bulge(), bb, cut, pro)[8 + sg.BULGE_AT] != 3


@pytest.mark.parametrize("phi_psi,code", [(sg.ALPHA, 1), (sg.HELIX_310, 4), (sg.HELIX_PI, 5)], ids=["H", "G", "I"])
def test_dssp_oracle_helix_types(phi_psi, code):
    """alpha: i + 4 -> i bonds (H); 3-10: i + 3 -> i (G); pi: i + 5 -> i (I).  Two consecutive n-turns at i - 1 and i
    mark residues i ... i + n - 1, so every residue but the two caps carries the code."""
    codes = _codes1(sg.helix(12, phi_psi), *sg.table(12))
    assert codes.tolist() == [0] + [code] * 10 + [0]


def test_dssp_oracle_proline_in_a_helix():
    """A proline has no amide hydrogen: the 4-turn that its N-H would close (at p - 4) is absent, and with it the two
    minimal helices that need that turn (those of the turn pairs (p - 5, p - 4) and (p - 4, p - 3)).  In a 6-residue
    helix (turns at 0 and 1, one minimal helix on residues 1 ... 4) a proline at 4 removes the turn at 0: no residue is
    H, the remaining turn at 1 leaves T on 2 ... 4.  In a long helix the neighbouring minimal helices (turn pairs
    (p - 6, p - 5) on residues p - 5 ... p - 2 and (p - 3, p - 2) on p - 2 ... p + 1) overlap the gap, which is why
    Kabsch and Sander let a single missing bond pass: H stays unbroken."""
    bb, chain, pro = sg.table(6)
    assert _codes1(sg.helix(6), bb, chain, pro).tolist() == [0, 1, 1, 1, 1, 0]
    pro[4] = 1
    assert _codes1(sg.helix(6), bb, chain, pro).tolist() == [0, 0, 6, 6, 6, 0]
    bb, chain, pro = sg.table(14)
    pro[7] = 1
    assert _codes1(sg.helix(14), bb, chain, pro).tolist() == [0] + [1] * 12 + [0]
    # three prolines in a row remove the turns at 2, 3, 4: minimal helices remain at 1 (turns 0, 1: residues 1 ... 4)
    # and from 6 on (turns 5, 6: residues 6 ... 9); residue 5 lies inside no turn (the turn at 1 spans 2 ... 4, the
    # turn at 5 spans 6 ... 8) and a helix bends by about 90 degrees over CA(3), CA(5), CA(7): S
    pro[:] = 0
    pro[[6, 7, 8]] = 1
    assert _codes1(sg.helix(14), bb, chain, pro).tolist() == [0, 1, 1, 1, 1, 7] + [1] * 7 + [0]


@pytest.mark.parametrize("how", ["stretched", "two-chains"])
def test_dssp_oracle_no_helix_across_a_chain_break(how):
    """A C - N distance above 2.5 Angstrom, or a change of chain, between residues 6 and 7 of a 14-residue helix: no
    n-turn may span the break, so the turns at 3 ... 6 are absent and H ends at 5 and resumes at 8."""
    bb, chain, pro = sg.table(14)
    xyz = sg.helix(14, stretch_after=6 if how == "stretched" else None)
    if how == "two-chains":
        chain[7:] = 1
    codes = _codes1(xyz, bb, chain, pro)
    assert codes.tolist() == [0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0]
    if how == "stretched":                  # 2.4 Angstrom is no break
        assert _codes1(sg.helix(14, stretch_after=6, stretch_to=2.4), bb, chain, pro)[6] != 0


def test_dssp_oracle_chignolin_is_a_hairpin(chig):
    """All 18 NMR models: the turn on residues 4 and 5 in every model, a bridge or a strand on both sides of it in most,
    model 0 strand - turn - strand; equal to the recorded codes."""
    codes = npport.dssp_codes(chig["xyz"], chig["backbone"], chig["chain"], chig["proline"])
    np.testing.assert_array_equal(codes, chig["dssp_codes"])
    assert codes[0].tolist() == [0, 3, 3, 6, 6, 6, 6, 3, 3, 0]
    assert (codes[:, 4:6] == 6).all()
    paired = np.isin(codes[:, :4], [2, 3]).any(axis=1) & np.isin(codes[:, 6:], [2, 3]).any(axis=1)
    assert paired.sum() >= 15, paired
    assert not np.isin(codes, [1, 4, 5]).any()


def test_dssp_oracle_incomplete_backbone_rows():
    """A backbone row with a -1 means what a residue on a chain of its own, far from everything, means: no bond, no
    hydrogen placed from it, a break on both sides, code 0.  The far residue goes through the code that existed before
    rows with -1 were accepted."""
    bb, chain, pro = sg.table(14)
    xyz = sg.helix(14).astype(np.float32)
    for rows in ([6], [0], [13], [6, 7], [0, 13]):
        holed = bb.copy()
        holed[rows, 2] = -1                                    # the C atom is missing
        far = xyz.copy()
        ch = chain.copy()
        for k, r in enumerate(rows):
            far[4 * r:4 * r + 4] += np.float32(100.0 + 10.0 * k)
            ch[r] = 7 + k
        want = _codes1(far, bb, ch, pro)
        got = _codes1(xyz, holed, chain, pro)
        np.testing.assert_array_equal(got, want)
        assert (got[rows] == 0).all()
    assert (_codes1(xyz, np.full_like(bb, -1), chain, pro) == 0).all()
    # tables without -1 are untouched by the extension: the rows above equal the plain helix where no row is missing
    assert _codes1(xyz, bb, chain, pro).tolist() == [0] + [1] * 12 + [0]


def test_dssp_oracle_small_residue_counts():
    """Fewer residues than a loop needs: R < 5 gives only 0 (a turn needs i + 3 < R and marks i + 1 ... i + 2)."""
    for R in (1, 2, 3):
        assert (_codes1(sg.helix(R), *sg.table(R)) == 0).all()
    assert _codes1(sg.helix(4, sg.HELIX_310), *sg.table(4)).tolist() == [0, 6, 6, 0]
    assert _codes1(sg.helix(5), *sg.table(5)).tolist() == [0, 6, 6, 6, 0]
    assert npport.dssp_codes(np.zeros((3, 4, 3), np.float32), np.zeros((0, 4), int), [], []).shape == (3, 0)


def test_dssp_ambiguous_share_of_the_gpu_test_frames(chig):
    """The frames tests/test_gpu_structure_paths.py runs: at most 5 % may be ambiguous by the float64 energy table
    (an energy within 2e-3 of -0.5, a CA distance within 1e-4 Angstrom of 9).  Measured: 27 of 1350 (2.0 %)."""
    total = ambiguous = 0
    for name, grp in sg.dssp_groups(chig).items():
        frames = sg.dssp_frames(grp)
        flags = [sref.dssp_frame_ambiguous(f, grp[1], grp[2], grp[3]) for f in frames]
        assert np.mean(flags) <= 0.05, (name, int(np.sum(flags)))
        total += len(flags)
        ambiguous += int(np.sum(flags))
        assert not sref.dssp_frame_ambiguous(frames[2], grp[1], grp[2], grp[3])       # the all-zero frame: NaN, no near miss
        assert not frames[2].any()
    assert ambiguous == 27 and total == 1350, (ambiguous, total)


def test_kabsch_sander_table_agrees_with_the_codes():
    """The float64 table explains the codes of the constructed helices: i + n -> i is below -0.5 for the helix's own n
    on every residue, and the table's CA distances are those of the geometry."""
    for phi_psi, stride in ((sg.ALPHA, 4), (sg.HELIX_310, 3), (sg.HELIX_PI, 5)):
        xyz = sg.helix(12, phi_psi)
        E, ca, _ = sref.kabsch_sander_table(xyz, *sg.table(12))
        assert (np.diagonal(E, -stride) < -0.5 - sref.KS_ENERGY_TOL).all(), (stride, np.diagonal(E, -stride))
        np.testing.assert_allclose(ca[0, 1], 3.8, atol=0.05)
        assert np.isnan(E[3, 3]) and np.isnan(E[4, 3]) and not np.isnan(E[3, 4])
    bb, chain, pro = sg.table(12)
    pro[5] = 1
    assert (sref.kabsch_sander_table(sg.helix(12), bb, chain, pro)[0][5, [0, 1, 2, 3, 6, 7]] == 0.0).all()


def test_sasa_reference_brackets_the_oracle(chig):
    """Float64 point counts, ambiguous points (within 1e-5 nm of a neighbour's surface) counted both ways, bracket the
    fp32 oracle's counts; at most 0.1 % of the points are ambiguous.  Measured: 1 of 115200 on the random cloud."""
    xyz, radii = sg.cloud(1, 120, 1.2, 5)
    P = 960
    lo, hi, n_amb = sref.sasa_bracket(xyz, radii, npport.sasa_sphere_points(P))
    counts = sref.sasa_counts(npport.shrake_rupley_atoms(xyz, radii, P), radii, P)
    assert (lo <= counts).all() and (counts <= hi).all()
    assert n_amb <= 1e-3 * counts.size * P and n_amb == 1
    assert counts.min() < P // 4 and counts.max() > P // 2             # buried and exposed atoms
    # chignolin, model 0, with the recorded areas
    radii = chig["sasa_radii"]
    lo, hi, n_amb = sref.sasa_bracket(chig["xyz"][:1], radii, npport.sasa_sphere_points(P))
    counts = sref.sasa_counts(chig["sasa_model0_960"][None], radii, P)
    assert (lo <= counts).all() and (counts <= hi).all()
    assert n_amb <= 1e-3 * counts.size * P
    assert (counts == 0).any() and (counts > P // 3).any()          # buried backbone atoms, exposed side-chain atoms
    # the bracket is tight: moving every count by one leaves it
    assert not ((lo <= counts + 1) & (counts + 1 <= hi)).all()
    # closed form: two equal spheres, the cap of height R - d / 2 is lost
    R, d = 0.31, 0.4
    lo, hi, _ = sref.sasa_bracket(np.array([[[0, 0, 0], [d, 0, 0]]], np.float32), [R, R], npport.sasa_sphere_points(4096))
    np.testing.assert_allclose(lo[0] / 4096.0, 1.0 - (R - d / 2) / (2 * R), atol=2e-3)


@pytest.mark.parametrize("n", [1, 15, 16, 31, 32, 33, 100, 257])
def test_hbond_reference_brackets_the_oracle(chig, n):
    """The frames of the GPU test: float64 distance and vector angle, ambiguous cases (distance within 1e-6 nm or angle
    within 1e-5 rad of the cutoff) counted both ways, bracket the oracle's counts; at most 1 % are ambiguous.
    Measured: none ambiguous for any n; 341 bonded (triplet, frame) cases at n = 257."""
    frames = sg.hbond_frames(chig["xyz"], n)
    counts = npport.baker_hubbard_presence(frames, chig["triplets"])
    lo, hi, n_amb = sref.hbond_bracket(frames, chig["triplets"])
    assert (lo <= counts).all() and (counts <= hi).all()
    assert n_amb <= 0.01 * counts.size * n and n_amb == 0
    if n >= 32:
        per16 = [npport.baker_hubbard_presence(frames[s:s + 16], chig["triplets"]).sum() for s in (0, 16)]
        assert per16[0] > 0 and per16[1] == 0                        # the chunks differ
    if n == 257:
        assert counts.sum() == 341


def test_hbond_reference_on_the_recorded_models(chig):
    counts = npport.baker_hubbard_presence(chig["xyz"], chig["triplets"])
    np.testing.assert_array_equal(counts, chig["hbond_presence"])
    lo, hi, n_amb = sref.hbond_bracket(chig["xyz"], chig["triplets"])
    assert (lo <= counts).all() and (counts <= hi).all() and n_amb <= 0.01 * 18 * 420
    assert counts.sum() == 34 and (counts / 18.0 > 0.1).sum() == 7
    # a case put on the cutoff is ambiguous, and only that one
    xyz = np.zeros((1, 3, 3), np.float32)
    xyz[0, 0] = [-0.1, 0, 0]
    xyz[0, 2] = [0.25, 0, 0]
    lo, hi, n_amb = sref.hbond_bracket(xyz, [[0, 1, 2]])
    assert (lo[0], hi[0], n_amb) == (0, 1, 1)


def test_degenerate_frames_count_nothing():
    """An all-zero frame (the classic junk frame) and a frame with D = H give 0 / 0 for the cosine.  mdtraj clips, which
    keeps the NaN, and compares, which is false: no hydrogen bond and no bend.  The float64 reference agrees (a
    degenerate triplet has angle 0), and the oracle's answer does not depend on the run."""
    trip = np.array([[0, 1, 3], [0, 1, 4], [2, 1, 3], [0, 0, 3], [0, 1, 1]])
    zero = np.zeros((2, 6, 3), np.float32)
    np.testing.assert_array_equal(npport.baker_hubbard_presence(zero, trip), 0)
    lo, hi, _ = sref.hbond_bracket(zero, trip)
    assert not lo.any() and not hi.any()
    same = _water_free_dipeptide().xyz.copy()
    same[:, 0] = same[:, 1]                                     # D = H
    got = npport.baker_hubbard_presence(same, trip)
    np.testing.assert_array_equal(got[[0, 1, 3, 4]], 0)       # [2, 1, 3] has another donor and is a plain bond
    assert got[2] == 5
    lo, hi, _ = sref.hbond_bracket(same, trip)
    assert (lo <= got).all() and (got <= hi).all()
    for R in (7, 10, 16):
        bb, chain, pro = sg.table(R)
        z = np.zeros((1, 4 * R, 3), np.float32)
        first = npport.dssp_codes(z, bb, chain, pro)
        assert not (first == 7).any()                           # no bend: kappa is NaN
        np.testing.assert_array_equal(first, npport.dssp_codes(z.copy(), bb, chain, pro))
