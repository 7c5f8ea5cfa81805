"""Host-only companion of tests/test_gpu_superpose.py and tests/test_superpose_host.py (numpy fp64, no GPU).

kabsch / superpose_ref   rigid-body superposition by SVD of the correlation matrix with the determinant correction
                         (Kabsch 1978): the mathematical definition csrc/superpose.hip is tested against
recovered_rotation       the least-squares LINEAR map between two coordinate sets, whose determinant tells a proper
                         rotation from a reflection
rigid_cloud              seeded test input: random rigid motions of a Gaussian cloud plus noise
path_of                  the launch rule of superpose.hip restated from the named constants of pmarlo_amd/_lib.py"""

from __future__ import annotations

import numpy as np

U24 = 2.0 ** -24     # unit round-off of fp32


def kabsch(x: np.ndarray, r: np.ndarray):
    """Proper rotation R (3 x 3, det +1), centroids and RMSD of the best fit of x [S, 3] onto r [S, 3]:
    minimises sum_i |R (x_i - c) - (r_i - c_ref)|^2."""
    x = np.asarray(x, np.float64)
    r = np.asarray(r, np.float64)
    c, c_ref = x.mean(axis=0), r.mean(axis=0)
    xc, rc = x - c, r - c_ref
    H = xc.T @ rc                                    # H[a, b] = sum_i x_i[a] r_i[b]
    U, s, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    if d == 0.0:
        d = 1.0
    D = np.diag([1.0, 1.0, d])
    R = Vt.T @ D @ U.T
    resid = xc @ R.T - rc
    return R, c, c_ref, float(np.sqrt(max(0.0, (resid ** 2).sum() / x.shape[0])))


def superpose_ref(xyz: np.ndarray, sel, ref: np.ndarray):
    """xyz [n, A, 3], sel [S] indices, ref [S, 3] -> (aligned float64 [n, A, 3], rmsd float64 [n])."""
    xyz = np.asarray(xyz, np.float64)
    sel = np.asarray(sel, dtype=int)
    out = np.empty_like(xyz)
    rmsd = np.empty(xyz.shape[0])
    for f in range(xyz.shape[0]):
        R, c, c_ref, rmsd[f] = kabsch(xyz[f, sel], ref)
        out[f] = (xyz[f] - c) @ R.T + c_ref
    return out, rmsd


def recovered_rotation(src: np.ndarray, dst: np.ndarray) -> np.ndarray:
    """Least-squares linear map L with (dst - mean) ~ (src - mean) L^T; needs atoms that span 3-space after
    centring (the callers check the rank)."""
    a = np.asarray(src, np.float64)
    b = np.asarray(dst, np.float64)
    a = a - a.mean(axis=0)
    b = b - b.mean(axis=0)
    L, *_ = np.linalg.lstsq(a, b, rcond=None)
    return L.T


def random_rotation(rng) -> np.ndarray:
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def rigid_cloud(seed: int, n: int, A: int, spread: float = 1.0, offset: float = 5.0, noise: float = 0.05):
    """(xyz float32 [n, A, 3], base float32 [A, 3]): every frame is a random rigid motion of one Gaussian cloud
    (sigma = spread nm, translated by up to `offset` nm) plus `noise` * spread of Gaussian noise."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((A, 3)) * spread
    xyz = np.empty((n, A, 3))
    for f in range(n):
        xyz[f] = base @ random_rotation(rng).T + rng.uniform(-offset, offset, 3)
    xyz += noise * spread * rng.standard_normal(xyz.shape)
    return xyz.astype(np.float32), (base + rng.uniform(-offset, offset, 3)).astype(np.float32)


def unsorted_selection(seed: int, A: int, S: int) -> np.ndarray:
    """S distinct indices in [0, A), not in ascending order (S >= 2), the last atom A - 1 among them."""
    rng = np.random.default_rng(seed)
    rest = rng.permutation(A - 1)[: S - 1]
    sel = rng.permutation(np.concatenate([rest, [A - 1]])).astype(np.int32)
    return sel[::-1].copy() if S >= 2 and np.all(np.diff(sel) > 0) else sel


def path_of(A: int, S: int, full: bool) -> tuple[str, int, int]:
    """(kernel, frames per LDS tile, lanes per frame in the accumulate pass) as superpose.hip picks them."""
    from pmarlo_amd import _lib

    lanes = 8 if S <= _lib.SUPERPOSE_NARROW_SEL else 64
    if not full:
        return "rmsd", 0, lanes
    if A > _lib.SUPERPOSE_LDS_ATOMS:
        return "stream", 0, lanes
    return "tile", min(_lib.SUPERPOSE_TILE_FRAMES, _lib.SUPERPOSE_TILE_FLOATS // (3 * A)), lanes
