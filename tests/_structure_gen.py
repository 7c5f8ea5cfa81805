"""Constructed backbone geometries for the structure-feature tests (numpy only): strands, sheets, a bulge, helices and
chain breaks built from (phi, psi) lists by internal-coordinate placement, plus the frame mixers the GPU tests use.

Coordinates are float64 nanometres, atoms in the order N, CA, C, O per residue (the backbone table of residue r is
[4 r, 4 r + 1, 4 r + 2, 4 r + 3]).  Bond lengths (Angstrom) N-CA 1.458, CA-C 1.525, C-N 1.329, C=O 1.231; angles
N-CA-C 111.0, CA-C-N 116.2, C-N-CA 121.7, CA-C-O 120.5 degrees; omega 180; O at the dihedral psi + 180.

Sheet placements.  The second strand of a two-strand sheet is placed relative to the first by (rotation of the
separation direction about the strand axis, shift along the axis, separation).  The rotation is measured in the basis
(u, v) with u the z axis made orthogonal to the strand axis a and v = a x u.  `search_sheet_placement` sweeps rotation
in 15 degree steps, shift in 0.5 Angstrom steps and separation 4.6 ... 5.2 Angstrom and returns every placement for which
a given DSSP gives E on residues 1-6 of both strands; SHEET_PLACEMENT holds the frozen choice (see the docstring of
tests/test_structure_oracle.py for what the sweep found)."""

from __future__ import annotations

import numpy as np

N_CA, CA_C, C_N, C_O = 1.458, 1.525, 1.329, 1.231
ANG_N_CA_C, ANG_CA_C_N, ANG_C_N_CA, ANG_CA_C_O = 111.0, 116.2, 121.7, 120.5

ALPHA = (-57.0, -47.0)
HELIX_310 = (-49.0, -26.0)
HELIX_PI = (-57.0, -70.0)
BETA_PARALLEL = (-119.0, 113.0)
BETA_ANTIPARALLEL = (-139.0, 135.0)

# kind -> (rotation in degrees, shift along the axis in Angstrom, separation in Angstrom); frozen from the sweep
SHEET_PLACEMENT = {"parallel": (15.0, 0.0, 4.8), "antiparallel": (15.0, -1.0, 4.8)}


def _place(a, b, c, bond, angle_deg, dihedral_deg):
    """The point d with |d - c| = bond, angle(b, c, d) = angle and dihedral(a, b, c, d) = dihedral."""
    th, ph = np.radians(angle_deg), np.radians(dihedral_deg)
    bc = c - b
    bc /= np.linalg.norm(bc)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    d2 = np.array([-bond * np.cos(th), bond * np.sin(th) * np.cos(ph), bond * np.sin(th) * np.sin(ph)])
    return c + d2[0] * bc + d2[1] * m + d2[2] * n


def backbone(phi, psi, cn_bond=None):
    """N, CA, C, O of len(phi) residues, float64 nm [4 R, 3].  phi[0] and psi[-1] only orient the end atoms.
    `cn_bond[r]` (Angstrom) overrides the length of the peptide bond C(r) - N(r + 1)."""
    R = len(phi)
    cn = [C_N] * R if cn_bond is None else list(cn_bond)
    out = np.zeros((R, 4, 3))
    n = np.zeros(3)
    ca = np.array([N_CA, 0.0, 0.0])
    th = np.radians(ANG_N_CA_C)
    c = ca + CA_C * np.array([-np.cos(th), np.sin(th), 0.0])
    for r in range(R):
        out[r, 0], out[r, 1], out[r, 2] = n, ca, c
        out[r, 3] = _place(n, ca, c, C_O, ANG_CA_C_O, psi[r] + 180.0)
        if r + 1 < R:
            n2 = _place(n, ca, c, cn[r], ANG_CA_C_N, psi[r])
            ca2 = _place(ca, c, n2, N_CA, ANG_C_N_CA, 180.0)
            c2 = _place(c, n2, ca2, CA_C, ANG_N_CA_C, phi[r + 1])
            n, ca, c = n2, ca2, c2
    return out.reshape(4 * R, 3) / 10.0


def regular(n_res, phi_psi, **kw):
    return backbone([phi_psi[0]] * n_res, [phi_psi[1]] * n_res, **kw)


def table(n_res):
    """Backbone table, chain ids and proline flags of n_res complete residues on one chain."""
    return np.arange(4 * n_res, dtype=np.int32).reshape(n_res, 4), np.zeros(n_res, np.int32), np.zeros(n_res, np.uint8)


def _rotate(x, axis, angle, origin):
    """Rodrigues rotation of the points x about the line through `origin` along `axis`."""
    k = axis / np.linalg.norm(axis)
    d = x - origin
    return origin + d * np.cos(angle) + np.cross(k, d) * np.sin(angle) + np.outer(d @ k, k) * (1.0 - np.cos(angle))


def strand_frame(strand):
    """Axis a of a strand (first to last CA), and the basis (u, v) the rotation of a placement is measured in."""
    ca = strand[1::4]
    a = ca[-1] - ca[0]
    a /= np.linalg.norm(a)
    u = np.array([0.0, 0.0, 1.0]) - a[2] * a
    u /= np.linalg.norm(u)
    return a, u, np.cross(a, u)


def two_strands(kind, placement=None, n_res=8):
    """Two strands of n_res residues on two chains, float64 nm [8 n_res, 3]: the second a translated copy (parallel)
    or a copy flipped by pi about the separation direction (antiparallel)."""
    rot, shift, sep = SHEET_PLACEMENT[kind] if placement is None else placement
    first = regular(n_res, BETA_PARALLEL if kind == "parallel" else BETA_ANTIPARALLEL)
    a, u, v = strand_frame(first)
    s = np.cos(np.radians(rot)) * u + np.sin(np.radians(rot)) * v
    second = first.copy()
    if kind == "antiparallel":
        second = _rotate(second, s, np.pi, first.mean(axis=0))
    second = second + (sep * s + shift * a) / 10.0
    return np.concatenate([first, second], axis=0)


def sheet_tables(n_a=8, n_b=8):
    bb, chain, pro = table(n_a + n_b)
    chain[n_a:] = 1
    return bb, chain, pro


def search_sheet_placement(kind, codes_fn, n_res=8):
    """Every (rotation, shift, separation) of the sweep for which codes_fn(xyz float32 [1, A, 3], bb, chain, proline)
    gives 0 E E E E E E 0 on both strands, in sweep order."""
    bb, chain, pro = sheet_tables(n_res, n_res)
    want = np.array(([0] + [3] * (n_res - 2) + [0]) * 2)
    hits = []
    for sep in (4.6, 4.8, 5.0, 5.2):
        for rot in np.arange(0.0, 360.0, 15.0):
            for shift in np.arange(-4.0, 4.01, 0.5):
                xyz = two_strands(kind, (rot, shift, sep), n_res).astype(np.float32)[None]
                if np.array_equal(codes_fn(xyz, bb, chain, pro)[0], want):
                    hits.append((float(rot), float(shift), float(sep)))
    return hits


BULGE_AT = 4   # the inserted residue's position in the second strand


def bulge():
    """The antiparallel pair with one residue inserted between residues 3 and 4 of the second strand (which becomes
    9 residues long): the eight paired residues stay where they are, the new one loops out of the sheet plane by
    2 Angstrom, within reach (C - N < 2.5 Angstrom) of both neighbours, its C=O parallel to its predecessor's so that
    the amide hydrogen of the residue after it stays where it was."""
    xyz = two_strands("antiparallel") * 10.0
    first, second = xyz[:32].reshape(8, 4, 3), xyz[32:].reshape(8, 4, 3)
    rot = SHEET_PLACEMENT["antiparallel"][0]
    a, u, v = strand_frame(xyz[:32])
    s = np.cos(np.radians(rot)) * u + np.sin(np.radians(rot)) * v
    w = np.cross(a, s)
    c_prev, o_prev, n_next = second[BULGE_AT - 1, 2], second[BULGE_AT - 1, 3], second[BULGE_AT, 0]
    e = (n_next - c_prev) / np.linalg.norm(n_next - c_prev)
    mid = 0.5 * (c_prev + n_next)
    half = 1.23                                        # half the N ... C distance inside one residue
    ins = np.zeros((4, 3))
    ins[0] = mid + 2.0 * w - half * e
    ins[2] = mid + 2.0 * w + half * e
    ins[1] = mid + (2.0 + np.sqrt(N_CA ** 2 - half ** 2)) * w
    ins[3] = ins[2] + C_O * (o_prev - c_prev) / np.linalg.norm(o_prev - c_prev)
    second = np.concatenate([second[:BULGE_AT], ins[None], second[BULGE_AT:]], axis=0)
    return np.concatenate([first.reshape(-1, 3), second.reshape(-1, 3)], axis=0) / 10.0


def helix(n_res=12, phi_psi=ALPHA, stretch_after=None, stretch_to=2.6):
    """A regular helix; `stretch_after = r` lengthens the peptide bond C(r) - N(r + 1) to `stretch_to` Angstrom."""
    cn = None
    if stretch_after is not None:
        cn = [C_N] * n_res
        cn[stretch_after] = stretch_to
    return regular(n_res, phi_psi, cn_bond=cn)


# ---------------------------------------------------------------------------------------------------------
# frame mixers
# ---------------------------------------------------------------------------------------------------------
def jitter(frames, sigma, seed):
    """Every frame of float32 [n, A, 3] plus its own Gaussian noise; sigma (nm) is a scalar or one value per frame."""
    frames = np.asarray(frames, np.float32)
    rng = np.random.default_rng(seed)
    sig = np.broadcast_to(np.asarray(sigma, np.float64), (frames.shape[0],))
    return (frames + rng.standard_normal(frames.shape) * sig[:, None, None]).astype(np.float32)


def interleave(folded, seed, n):
    """n frames float32 [n, A, 3] in which neighbours differ: frame t is a fold (cycling through `folded`) with 0.01 nm of
    Gaussian jitter of its own (t % 3 == 0: mostly still folded), the same with 0.02 ... 0.03 nm (t % 3 == 1: mostly
    opened up), or (t % 3 == 2) alternately all zero and a fold as constructed (each in turn).  A prefix of the result is the result
    for a smaller n."""
    folded = np.asarray(folded, np.float32)
    rng = np.random.default_rng(seed)
    out = np.zeros((n,) + folded.shape[1:], np.float32)
    for t in range(n):
        base = folded[(t // 3) % folded.shape[0]]
        if t % 3 == 0:
            out[t] = base + (rng.standard_normal(base.shape) * 0.01).astype(np.float32)
        elif t % 3 == 1:
            out[t] = base + (rng.standard_normal(base.shape) * rng.uniform(0.02, 0.03)).astype(np.float32)
        elif t % 6 == 5:
            out[t] = folded[(t // 6) % folded.shape[0]]
    return out


def shell_cluster(n_shell, shell_radius=0.05, seed=0):
    """One atom at the origin and n_shell atoms on a sphere of `shell_radius` nm around it (golden spiral, so that no
    two coincide), float32 [1, 1 + n_shell, 3]."""
    i = np.arange(n_shell, dtype=np.float64)
    y = 1.0 - (2.0 * i + 1.0) / n_shell
    r = np.sqrt(1.0 - y * y)
    ph = i * np.pi * (3.0 - np.sqrt(5.0))
    pts = np.stack([np.cos(ph) * r, y, np.sin(ph) * r], axis=1) * shell_radius
    return np.concatenate([np.zeros((1, 3)), pts], axis=0).astype(np.float32)[None]


# ---------------------------------------------------------------------------------------------------------
# the inputs the CPU and the GPU tests share (the CPU test asserts the ambiguous shares of exactly these)
# ---------------------------------------------------------------------------------------------------------
DSSP_N_MAX = 150          # the GPU tests run prefixes of these frames: n = 1, 63, 64, 65, 130, and 150 in chunks of 64


def dssp_groups(chig):
    """name -> (folded frames float32 [m, A, 3], backbone table, chain, proline, seed): one group per call shape (one
    call has one residue count and one table).  `chig` is tests/golden/chignolin.npz."""
    f32 = np.float32
    groups = {"chignolin": (np.asarray(chig["xyz"]), chig["backbone"], chig["chain"], chig["proline"], 11)}
    bb, chain, pro = sheet_tables()
    sheets = np.stack([two_strands("parallel"), two_strands("antiparallel")]).astype(f32)
    groups["sheets"] = (sheets, bb, chain, pro, 12)
    bb, chain, pro = sheet_tables(8, 9)
    groups["bulge"] = (bulge().astype(f32)[None], bb, chain, pro, 13)
    bb, chain, pro = table(12)
    helices = np.stack([helix(12, ALPHA), helix(12, HELIX_310), helix(12, HELIX_PI)]).astype(f32)
    groups["helices"] = (helices, bb, chain, pro, 14)
    for name, at in (("proline-first", 0), ("proline-middle", 6), ("proline-last", 11)):
        p = pro.copy()
        p[at] = 1
        groups[name] = (helices, bb, chain, p, 15 + at)
    bb, chain, pro = table(14)
    broken = np.stack([helix(14), helix(14, stretch_after=6)]).astype(f32)
    groups["stretched"] = (broken, bb, chain, pro, 27)
    c2 = chain.copy()
    c2[7:] = 1
    groups["two-chains"] = (broken, bb, c2, pro, 28)
    return groups


def dssp_frames(group, n=DSSP_N_MAX):
    folded, bb, chain, pro, seed = group
    return interleave(folded, seed, n)


def hbond_frames(chig_xyz, n, seed=5):
    """n frames float32 [n, A, 3] from the chignolin models (model t % 18), each with 0.005 nm of jitter of its own.
    Frames 16 ... 31 of every 48 are blown up by 1.5 about the centroid, which breaks every hydrogen bond: the kernel's
    frame chunks (16 or 17 frames) see different counts."""
    base = np.asarray(chig_xyz, np.float32)
    out = jitter(base[np.arange(n) % base.shape[0]], 0.005, seed)
    for t in range(n):
        if (t // 16) % 3 == 1:
            c = out[t].mean(axis=0, keepdims=True)
            out[t] = c + (out[t] - c) * np.float32(1.5)
    return out


SASA_RADII = np.float32([0.26, 0.31, 0.295, 0.292, 0.32])     # element radii + 0.14 nm probe, as test_gpu_structure.py


def cloud(n, A, box, seed):
    """n frames of A uniformly random atoms in a cube of `box` nm, and a radius per atom."""
    rng = np.random.default_rng(seed)
    return (rng.random((n, A, 3)) * box).astype(np.float32), rng.choice(SASA_RADII, size=A)
