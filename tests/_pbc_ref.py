"""Host-only companion of tests/test_pbc_reference.py and tests/test_gpu_pbc.py (numpy, no GPU).

box_from_cell      cell parameters -> box vectors in mdtraj's convention (rows a, b, c; a along x, b in the xy-plane;
                   components within 1e-6 of zero set to zero), fp64
extract            the feature extractor of csrc/featurize.hip's spec kernel restated: the reference extractor's
                   arithmetic in its operation order, in fp32 (dtype=np.float32: what the device is held to) or fp64,
                   with the minimum image by the reference's rounding rule (mic="round") or by brute force over the
                   images in [-2, 2]^3 in fp64 (mic="search"; only with dtype=np.float64)
brute_min_image    that brute force: the shortest image and the gap to the second shortest length
tie_margin         the distance of every flagged fractional component of an input from a half-integer: where it is
                   not small, fp32 and fp64 round the same way and the "round" image is unambiguous
search_gap         the smallest gap between the best and second-best image length over the flagged bond vectors
bond_vectors       the raw (unwrapped) bond vectors of every entry, with their flags
draw_frames        seeded test input: frames of a random-walk chain whose atoms are displaced by lattice vectors of a
                   breathing box, each frame redrawn until it is well conditioned (see `well_conditioned`)

A `spec` is anything with the fields of NormalizedFeatureSpec (numpy arrays or CPU torch tensors)."""

from __future__ import annotations

import itertools

import numpy as np

EPS = 1.0e-12
_SHIFTS = np.asarray(list(itertools.product(range(-2, 3), repeat=3)), dtype=np.float64)     # [125, 3]


def box_from_cell(cell) -> np.ndarray:
    c = np.asarray(cell, np.float64).reshape(-1, 6)
    rad = np.pi / 180.0
    ca, cb, cg, sg = np.cos(c[:, 3] * rad), np.cos(c[:, 4] * rad), np.cos(c[:, 5] * rad), np.sin(c[:, 5] * rad)
    box = np.zeros((c.shape[0], 3, 3))
    box[:, 0, 0] = c[:, 0]
    box[:, 1, 0] = c[:, 1] * cg
    box[:, 1, 1] = c[:, 1] * sg
    box[:, 2, 0] = c[:, 2] * cb
    box[:, 2, 1] = c[:, 2] * (ca - cb * cg) / sg
    box[:, 2, 2] = np.sqrt(c[:, 2] ** 2 - box[:, 2, 0] ** 2 - box[:, 2, 1] ** 2)
    box[np.abs(box) < 1.0e-6] = 0.0
    return box


def inverse_adjugate(box: np.ndarray) -> np.ndarray:
    """[n, 3, 3] -> inverse by the adjugate over the determinant, in the dtype of `box` (the device's closed form)."""
    b = box
    c00 = b[:, 1, 1] * b[:, 2, 2] - b[:, 1, 2] * b[:, 2, 1]
    c01 = b[:, 1, 2] * b[:, 2, 0] - b[:, 1, 0] * b[:, 2, 2]
    c02 = b[:, 1, 0] * b[:, 2, 1] - b[:, 1, 1] * b[:, 2, 0]
    det = b[:, 0, 0] * c00 + b[:, 0, 1] * c01 + b[:, 0, 2] * c02
    inv = np.empty_like(b)
    inv[:, 0, 0] = c00 / det
    inv[:, 0, 1] = (b[:, 0, 2] * b[:, 2, 1] - b[:, 0, 1] * b[:, 2, 2]) / det
    inv[:, 0, 2] = (b[:, 0, 1] * b[:, 1, 2] - b[:, 0, 2] * b[:, 1, 1]) / det
    inv[:, 1, 0] = c01 / det
    inv[:, 1, 1] = (b[:, 0, 0] * b[:, 2, 2] - b[:, 0, 2] * b[:, 2, 0]) / det
    inv[:, 1, 2] = (b[:, 0, 2] * b[:, 1, 0] - b[:, 0, 0] * b[:, 1, 2]) / det
    inv[:, 2, 0] = c02 / det
    inv[:, 2, 1] = (b[:, 0, 1] * b[:, 2, 0] - b[:, 0, 0] * b[:, 2, 1]) / det
    inv[:, 2, 2] = (b[:, 0, 0] * b[:, 1, 1] - b[:, 0, 1] * b[:, 1, 0]) / det
    return inv


def _vec_mat(v: np.ndarray, m: np.ndarray) -> np.ndarray:
    """Row vectors v [n, k, 3] times matrices m [n, 3, 3], summed left to right in the dtype of the operands."""
    m = m[:, None]
    return np.stack([v[..., 0] * m[..., 0, j] + v[..., 1] * m[..., 1, j] + v[..., 2] * m[..., 2, j] for j in range(3)],
                    axis=-1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _boxes(box, n: int, dtype) -> np.ndarray:
    b = np.asarray(box, dtype).reshape(-1, 3, 3)
    return np.broadcast_to(b, (n, 3, 3)) if b.shape[0] == 1 else b


def fractional(v: np.ndarray, box: np.ndarray) -> np.ndarray:
    return _vec_mat(v, inverse_adjugate(np.ascontiguousarray(box)))


def round_image(v: np.ndarray, box: np.ndarray) -> np.ndarray:
    f = fractional(v, box)
    return _vec_mat(f - np.rint(f), box)


def brute_min_image(v: np.ndarray, box: np.ndarray):
    """v [n, k, 3], box [n, 3, 3], fp64 -> (shortest image [n, k, 3], gap to the second-shortest length [n, k]).
    The images are those of the round-reduced vector shifted by every lattice vector in [-2, 2]^3."""
    r = round_image(np.asarray(v, np.float64), np.asarray(box, np.float64))
    shifts = np.einsum("si,nij->nsj", _SHIFTS, np.asarray(box, np.float64))          # [n, 125, 3]
    cand = r[:, :, None, :] + shifts[:, None, :, :]                                    # [n, k, 125, 3]
    length = np.sqrt(_dot(cand, cand))
    order = np.argsort(length, axis=-1)
    best = np.take_along_axis(cand, order[..., :1, None], axis=2)[:, :, 0]
    two = np.take_along_axis(length, order[..., :2], axis=-1)
    return best, two[..., 1] - two[..., 0]


def _np(a, dtype=None):
    return np.asarray(a, dtype=dtype)


def bond_vectors(spec, xyz: np.ndarray, dtype=np.float64):
    """[(kind, positions, flags, [bond vector arrays [n, m, 3]])] with the reference's sign conventions:
    distance x_j - x_i; angle x_i - x_j and x_k - x_j; dihedral b0, b1, b2 along the chain."""
    x = np.asarray(xyz, dtype)
    out = []
    p = _np(spec.distance_pairs, np.int64)
    if len(p):
        out.append(("distance", _np(spec.distance_positions, np.int64), _np(spec.distance_pbc, bool),
                    [x[:, p[:, 1]] - x[:, p[:, 0]]]))
    t = _np(spec.angle_triplets, np.int64)
    if len(t):
        out.append(("angle", _np(spec.angle_positions, np.int64), _np(spec.angle_pbc, bool),
                    [x[:, t[:, 0]] - x[:, t[:, 1]], x[:, t[:, 2]] - x[:, t[:, 1]]]))
    q = _np(spec.dihedral_quads, np.int64)
    if len(q):
        out.append(("dihedral", _np(spec.dihedral_positions, np.int64), _np(spec.dihedral_pbc, bool),
                    [x[:, q[:, 1]] - x[:, q[:, 0]], x[:, q[:, 2]] - x[:, q[:, 1]], x[:, q[:, 3]] - x[:, q[:, 2]]]))
    return out


def _geometry(kind: str, vs, dtype) -> np.ndarray:
    """acos and atan2 are evaluated in fp64 on the `dtype` argument and rounded once: the correctly rounded value,
    the same on every host whatever vector maths library its numpy was built with."""
    eps = dtype(EPS)
    norm = lambda a: np.sqrt(np.maximum(_dot(a, a), eps))      # noqa: E731
    if kind == "distance":
        return norm(vs[0])
    if kind == "angle":
        c = _dot(vs[0], vs[1]) / (norm(vs[0]) * norm(vs[1]))
        return np.arccos(np.clip(c, dtype(-1.0), dtype(1.0)).astype(np.float64)).astype(dtype)
    b0, b1, b2 = vs
    c0, c1 = _cross(b0, b1), _cross(b1, b2)
    c0 = c0 / norm(c0)[..., None]
    c1 = c1 / norm(c1)[..., None]
    b1u = b1 / norm(b1)[..., None]
    x, y = _dot(c0, c1), _dot(_cross(c0, c1), b1u)
    ok = (np.abs(x) + np.abs(y)) >= eps
    ang = np.arctan2(np.where(ok, y, 0).astype(np.float64), np.where(ok, x, 1).astype(np.float64))
    return np.where(ok, ang, 0).astype(dtype)


def extract(spec, xyz, box=None, mic: str = "round", dtype=np.float32, weighted: bool = True) -> np.ndarray:
    """[n, F] in `dtype`: every entry at its position, times its weight; flagged bond vectors wrapped when a box is
    given.  mic="search" is the fp64 brute force."""
    if mic == "search" and dtype != np.float64:
        raise ValueError("the brute-force minimum image is an fp64 yardstick")
    dtype = np.dtype(dtype).type
    x = np.asarray(xyz, dtype)
    n = x.shape[0]
    w = _np(spec.feature_weights, dtype)
    out = np.zeros((n, w.size), dtype)
    b = None if box is None else np.ascontiguousarray(_boxes(box, n, dtype))
    for kind, pos, flags, vs in bond_vectors(spec, x, dtype):
        if b is not None and flags.any():
            wrap = (lambda v: round_image(v, b)) if mic == "round" else (lambda v: brute_min_image(v, b)[0])
            vs = [np.where(flags[None, :, None], wrap(v), v) for v in vs]
        out[:, pos] = _geometry(kind, vs, dtype)
    return out * w[None, :] if weighted else out


def tie_margin(spec, xyz, box) -> np.ndarray:
    """[n]: per frame, the smallest distance of a flagged fractional component from a half-integer (fp64)."""
    x = np.asarray(xyz, np.float64)
    b = np.ascontiguousarray(_boxes(box, x.shape[0], np.float64))
    margin = np.full(x.shape[0], np.inf)
    for _kind, _pos, flags, vs in bond_vectors(spec, x):
        for v in vs:
            f = fractional(v, b)[:, flags]
            if f.size:
                margin = np.minimum(margin, np.abs(np.abs(f - np.floor(f)) - 0.5).reshape(x.shape[0], -1).min(axis=1))
    return margin


def search_gap(spec, xyz, box, kinds=("distance", "angle", "dihedral")) -> np.ndarray:
    """[n]: per frame, the smallest gap between the best and the second-best image length over the flagged bond
    vectors of the given kinds (fp64)."""
    x = np.asarray(xyz, np.float64)
    b = np.ascontiguousarray(_boxes(box, x.shape[0], np.float64))
    gap = np.full(x.shape[0], np.inf)
    for kind, _pos, flags, vs in bond_vectors(spec, x):
        if kind in kinds and flags.any():
            for v in vs:
                gap = np.minimum(gap, brute_min_image(v[:, flags], b)[1].min(axis=1))
    return gap


def wrap_to_pi(d: np.ndarray) -> np.ndarray:
    """Differences of angles modulo 2 pi, into [-pi, pi)."""
    return (np.asarray(d, np.float64) + np.pi) % (2.0 * np.pi) - np.pi


def random_chain(rng, n_atoms: int, bond: float) -> np.ndarray:
    """Random walk with bond length `bond` +- 10 % and no bend closer to collinear than cos = 0.9."""
    pos = [np.zeros(3)]
    prev = None
    while len(pos) < n_atoms:
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        if prev is not None and abs(float(d @ prev)) > 0.9:
            continue
        pos.append(pos[-1] + d * bond * rng.uniform(0.9, 1.1))
        prev = d
    return np.asarray(pos)


def wrapped_frame(rng, cell, n_atoms: int, bond: float):
    """(xyz float32 [A, 3], box float32 [3, 3], cell float64 [6]): the cell's lengths scaled by a common factor in
    [0.98, 1.02], a chain at a random origin inside the box, every atom then displaced by an integer combination
    (coefficients in {-1, 0, 1}) of the box vectors."""
    c = np.asarray(cell, np.float64).copy()
    c[:3] *= rng.uniform(0.98, 1.02)
    box = box_from_cell(c)[0].astype(np.float32)
    shifts = rng.integers(-1, 2, size=(n_atoms, 3)).astype(np.float64)
    origin = rng.uniform(0.0, 1.0, size=3) @ box
    xyz = (random_chain(rng, n_atoms, bond) + origin + shifts @ box.astype(np.float64)).astype(np.float32)
    return xyz, box, c


def torsion_lengths(spec, xyz, box, mic: str = "round") -> np.ndarray:
    """[n]: per frame, the smallest of |b1|, |b0 x b1| and |b1 x b2| over the torsions, on the vectors the
    extractor works with (flagged ones wrapped by `mic`), fp64."""
    x = np.asarray(xyz, np.float64)
    b = np.ascontiguousarray(_boxes(box, x.shape[0], np.float64))
    wrap = (lambda v: round_image(v, b)) if mic == "round" else (lambda v: brute_min_image(v, b)[0])
    least = np.full(x.shape[0], np.inf)
    for kind, _pos, flags, vs in bond_vectors(spec, x):
        if kind == "dihedral":
            b0, b1, b2 = (np.where(flags[None, :, None], wrap(v), v) for v in vs)
            for length in (np.linalg.norm(b1, axis=-1), np.linalg.norm(_cross(b0, b1), axis=-1),
                           np.linalg.norm(_cross(b1, b2), axis=-1)):
                least = np.minimum(least, length.min(axis=1))
    return least


def well_conditioned(spec, xyz, box) -> np.ndarray:
    """[n] bool: every flagged fractional component >= 1e-3 from a half-integer (the rounding rule is unambiguous);
    the best and second-best image lengths of every flagged angle / torsion bond vector >= 1e-3 nm apart (the true
    minimum image is unambiguous); |b1| and both plane normals of every torsion >= 1e-3 nm under either rule."""
    return ((tie_margin(spec, xyz, box) >= 1.0e-3) & (search_gap(spec, xyz, box, ("angle", "dihedral")) >= 1.0e-3)
            & (torsion_lengths(spec, xyz, box, "round") >= 1.0e-3) & (torsion_lengths(spec, xyz, box, "search") >= 1.0e-3))


def draw_frames(rng, cell, n: int, spec, n_atoms: int, bond: float):
    """n well-conditioned frames: (xyz [n, A, 3] f32, box [n, 3, 3] f32, cells [n, 6] f64, frames redrawn)."""
    xyz = np.empty((n, n_atoms, 3), np.float32)
    box = np.empty((n, 3, 3), np.float32)
    cells = np.empty((n, 6), np.float64)
    redrawn = 0
    for t in range(n):
        while True:
            xyz[t], box[t], cells[t] = wrapped_frame(rng, cell, n_atoms, bond)
            if well_conditioned(spec, xyz[t:t + 1], box[t:t + 1])[0]:
                break
            redrawn += 1
    return xyz, box, cells, redrawn
