"""Float64 references for the structure kernels that do not depend on the order of operations (numpy only), so that a
disagreement between csrc/structure.hip and its fp32 restatement in oracle/npport.py can be judged by a third party.

Each reference sorts the decisions the fp32 code takes into certain ones and ambiguous ones (the quantity is so close to
its threshold that fp32 rounding may decide either way) and returns a bracket: the count without and the count with the
ambiguous decisions.  A correct fp32 result lies inside the bracket.  The margins are far above the fp32 error of the
quantities (coordinates of about 1 nm: 6e-8 relative, a handful of operations) and far below their spread."""

from __future__ import annotations

import numpy as np

SASA_TOL = 1e-5          # nm: distance of a sphere point to the nearest neighbour's surface
HB_DIST_TOL = 1e-6       # nm
HB_ANGLE_TOL = 1e-5      # rad
KS_ENERGY_TOL = 2e-3     # kcal/mol around -0.5 (the energy is rounded to 1e-3 before the comparison)
KS_CA_TOL = 1e-4         # Angstrom around the 9 Angstrom pair cutoff


def sasa_bracket(xyz, radii, points, tol=SASA_TOL):
    """Accessible sphere points per (frame, atom) in float64: (lo, hi, n_ambiguous) with lo counting the points
    farther than `tol` outside every other atom's sphere and hi those not deeper than `tol` inside one.  `radii`
    include the probe.  Every other atom is tested: an atom beyond R_i + R_j cannot contain a point anyway."""
    xyz = np.asarray(xyz, np.float32).astype(np.float64)
    radii = np.asarray(radii, np.float32).astype(np.float64)
    pts = np.asarray(points, np.float32).astype(np.float64)
    n, A, _ = xyz.shape
    lo = np.zeros((n, A), np.int64)
    hi = np.zeros((n, A), np.int64)
    for t in range(n):
        fr = xyz[t]
        for i in range(A):
            c = fr[i] + radii[i] * pts                                            # [P, 3]
            others = np.arange(A) != i
            if not others.any():
                lo[t, i] = hi[t, i] = len(pts)
                continue
            d = np.linalg.norm(c[:, None, :] - fr[others][None, :, :], axis=2) - radii[others][None, :]
            margin = d.min(axis=1)                                                # < 0: inside some sphere
            lo[t, i] = int((margin > tol).sum())
            hi[t, i] = int((margin >= -tol).sum())
    return lo, hi, int((hi - lo).sum())


def sasa_counts(areas, radii, n_points):
    """The integer point counts behind fp32 areas ((4 pi / P) R_i^2 n_accessible)."""
    r = np.asarray(radii, np.float32).astype(np.float64)
    return np.rint(np.asarray(areas, np.float64) / (4.0 * np.pi / n_points * r * r)[None, :]).astype(np.int64)


def hbond_bracket(xyz, triplets, distance_cutoff=0.25, angle_cutoff=np.float32(2.0 * np.pi / 3.0),
                  dist_tol=HB_DIST_TOL, angle_tol=HB_ANGLE_TOL):
    """Frames per (donor, hydrogen, acceptor) triplet with |H - A| < cutoff and angle(D, H, A) > cutoff, float64, the
    angle from the vectors H -> D and H -> A (atan2 of |cross| and dot; 0 for a degenerate triplet, which is absent):
    (lo, hi, n_ambiguous) with a (triplet, frame) ambiguous when it is not excluded for certain by either criterion and
    its distance lies within dist_tol or its angle within angle_tol of the cutoff."""
    xyz = np.asarray(xyz, np.float32).astype(np.float64)
    trip = np.asarray(triplets, int).reshape(-1, 3)
    D, H, Ac = xyz[:, trip[:, 0]], xyz[:, trip[:, 1]], xyz[:, trip[:, 2]]
    u, v = D - H, Ac - H
    dist = np.linalg.norm(v, axis=2)
    ang = np.arctan2(np.linalg.norm(np.cross(u, v), axis=2), (u * v).sum(axis=2))
    dc, ac = float(distance_cutoff), float(angle_cutoff)
    sure = (dist < dc - dist_tol) & (ang > ac + angle_tol)
    possible = (dist < dc + dist_tol) & (ang > ac - angle_tol)
    lo, hi = sure.sum(axis=0).astype(np.int64), possible.sum(axis=0).astype(np.int64)
    return lo, hi, int((hi - lo).sum())


def kabsch_sander_table(frame, backbone, chain, proline):
    """Float64 Kabsch-Sander energies E[donor, acceptor] (kcal/mol, NaN where DSSP evaluates none: donor == acceptor,
    donor == acceptor + 1, an incomplete residue) and CA-CA distances (Angstrom) of one frame (nm)."""
    fr = np.asarray(frame, np.float32).astype(np.float64) * 10.0
    bb = np.asarray(backbone, int).reshape(-1, 4)
    R = bb.shape[0]
    full = (bb >= 0).all(axis=1)
    bb = np.where(bb >= 0, bb, 0)
    N, CA, C, O = (fr[bb[:, k]] for k in range(4))
    H = N.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(1, R):
            if not proline[r] and chain[r - 1] == chain[r] and full[r] and full[r - 1]:
                H[r] = N[r] + (C[r - 1] - O[r - 1]) / np.linalg.norm(C[r - 1] - O[r - 1])

        def dm(a, b):
            return np.linalg.norm(a[:, None, :] - b[None, :, :], axis=2)

        dHO, dHC, dNC, dNO = dm(H, O), dm(H, C), dm(N, C), dm(N, O)
        E = 27.888 * (-1.0 / dHO + 1.0 / dHC - 1.0 / dNC + 1.0 / dNO)
        dmin = np.fmin(np.fmin(dHO, dHC), np.fmin(dNC, dNO))          # a NaN distance is no hit, as in dssp.cpp
        E = np.where(dmin < 0.5, -9.9, np.maximum(E, -9.9))
    E[np.asarray(proline, bool)] = 0.0
    d, a = np.indices((R, R))
    E[(d == a) | (d == a + 1) | ~full[:, None] | ~full[None, :]] = np.nan
    ca = dm(CA, CA)
    ca[~full[:, None] | ~full[None, :]] = np.nan
    return E, ca, dmin


def dssp_frame_ambiguous(frame, backbone, chain, proline, e_tol=KS_ENERGY_TOL, ca_tol=KS_CA_TOL):
    """Whether fp32 rounding may change a decision of DSSP on this frame: an energy within e_tol of -0.5 (for a pair
    within the CA cutoff), or a CA-CA distance within ca_tol of 9 Angstrom."""
    E, ca, _ = kabsch_sander_table(frame, backbone, chain, proline)
    with np.errstate(invalid="ignore"):
        near_ca = np.abs(ca - 9.0) < ca_tol
        near_e = (np.abs(E + 0.5) < e_tol) & (ca < 9.0 + ca_tol)
    return bool(near_ca.any() or near_e.any())
