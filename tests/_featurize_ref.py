"""Exact references, conditioning and seeded inputs for the featurizer kernels of csrc/featurize.hip
(tests/test_featurize_reference.py on the host, tests/test_gpu_featurize_paths.py on the device).

The exact law of every kind is evaluated on the fp32 coordinates widened to np.longdouble: no fp32 re-run.
  distance  |x_j - x_i|
  angle     atan2(|v1 x v2|, v1.v2), with sin(theta) = |v1 x v2| / (|v1||v2|) as its conditioning
  dihedral  atan2((c0 x c1).b1 / |b1|, c0.c1) in (-pi, pi], with s = min(sin(b0, b1), sin(b1, b2))
  contact   d <= rcut, with the margin |d - rcut|
  rg        sqrt(mean |r - mean r|^2)
The class of an entry (finite, NaN, +inf, -inf) comes from the fp32 restatements of oracle/npport.py, which carry the
reference's NaN rules (np.maximum and np.clip keep NaN as torch.clamp_min and torch.clamp do).

Yardsticks, with u = 2^-24.  The device runs the reference's fp32 operation order, so its error is bounded the way the
fp32 restatement's is: relative u for a distance, u / sin(theta) for an angle (acos of a cosine known to a few u; the
slope of acos is 1 / sin, and at sin < sqrt(u) the error of acos(1 - O(u)) is O(sqrt(u))), u / s for a dihedral (the
cross products b0 x b1 and b1 x b2 cancel to a fraction s of their terms).  K_D, K_A, K_T below are the largest
  |d32 - d| / (u d),   |a32 - a| max(sin, sqrt(u)) / u,   |t32 - t| (mod 2 pi) max(s, sqrt(u)) / u
of the restatement over every input this module generates (`measure_yardsticks`, asserted by the host test); the
device is held to TWICE those: the factor covers contracted multiply-adds in the dot and cross products and the device's
acosf / atan2f / cosf / sinf, a few ulp each.  Dihedral inputs keep s >= S_MIN > sqrt(u): below that the cross products
have no correct digit left and no bound of this form exists (the generator redraws such frames)."""

from __future__ import annotations

import functools

import numpy as np

from oracle import npport

LD = np.longdouble
U = 2.0 ** -24
SQRT_U = 2.0 ** -12
PI32 = np.float32(np.pi)
PI_LD = np.arctan2(LD(0), LD(-1))
EPS_ROOT = np.sqrt(np.float32(1.0e-12))          # the floored length of a zero bond, one correctly rounded fp32 sqrt

N_ACC, A_ACC = 4099, 12                          # accuracy inputs: frames, atoms
REGIMES = {"o1": 0.0, "off50": 50.0, "off1000": 1000.0}
COUNTS = (1, 7, 64, 65)                          # records per table; the tables of 1, 7, 64 are prefixes of the 65
N_TRIP, M_TRIP = 4081, 257                       # second grid-stride trip: 1,048,817 elements
WIDTH = {"distance": 2, "angle": 3, "dihedral": 4}
S_MIN = 5.0e-4                                   # smallest s a dihedral input keeps (2 sqrt(u))
RCUT = 0.9

# measured by measure_yardsticks() on the inputs below (longdouble reference), rounded up in the last digit
K_D, K_A, K_T = 2.59, 7.17, 5.76


# ---------------------------------------------------------------------------------------------- exact laws
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _norm(a):
    return np.sqrt((a * a).sum(-1))


def exact_distance(xyz, pairs):
    x, p = np.asarray(xyz, np.float32).astype(LD), np.asarray(pairs)
    return _norm(x[:, p[:, 1]] - x[:, p[:, 0]])


def exact_angle(xyz, triplets):
    """(theta, sin theta); three coincident or collinear atoms give sin = 0 and theta = 0 or pi (atan2(0, dot))."""
    x, t = np.asarray(xyz, np.float32).astype(LD), np.asarray(triplets)
    v1, v2 = x[:, t[:, 0]] - x[:, t[:, 1]], x[:, t[:, 2]] - x[:, t[:, 1]]
    c = _norm(_cross(v1, v2))
    den = _norm(v1) * _norm(v2)
    with np.errstate(invalid="ignore", divide="ignore"):
        sin = np.where(den > 0, c / np.where(den > 0, den, 1), 0)
    return np.arctan2(c, (v1 * v2).sum(-1)), sin


def exact_dihedral(xyz, quads):
    """(t in (-pi, pi], s)."""
    x, q = np.asarray(xyz, np.float32).astype(LD), np.asarray(quads)
    b0, b1, b2 = x[:, q[:, 1]] - x[:, q[:, 0]], x[:, q[:, 2]] - x[:, q[:, 1]], x[:, q[:, 3]] - x[:, q[:, 2]]
    c0, c1 = _cross(b0, b1), _cross(b1, b2)
    nb = _norm(b1)
    with np.errstate(invalid="ignore", divide="ignore"):
        y = (_cross(c0, c1) * b1).sum(-1) / np.where(nb > 0, nb, 1)
        t = np.arctan2(y, (c0 * c1).sum(-1))
        d0, d1 = _norm(b0) * nb, nb * _norm(b2)
        s = np.minimum(np.where(d0 > 0, _norm(c0) / np.where(d0 > 0, d0, 1), 0),
                       np.where(d1 > 0, _norm(c1) / np.where(d1 > 0, d1, 1), 0))
    return np.where(t <= -PI_LD, t + 2 * PI_LD, t), s


def exact_rg(xyz):
    x = np.asarray(xyz, np.float32).astype(LD)
    c = x - x.mean(axis=1, keepdims=True)
    return np.sqrt((c * c).sum(axis=2).mean(axis=1))


def wrap_diff(a, b):
    """|a - b| modulo 2 pi, in longdouble."""
    d = np.abs(np.asarray(a).astype(LD) - np.asarray(b).astype(LD))
    return np.minimum(d, np.abs(2 * PI_LD - d))


def bound_distance(d, k=2 * K_D):
    return k * U * np.asarray(d, LD)


def bound_conditioned(sin, k):
    return k * U / np.maximum(np.asarray(sin, LD), SQRT_U)


# ---------------------------------------------------------------------------------------------- classes
FINITE, NAN, PINF, NINF = 0, 1, 2, 3


def classes(a):
    a = np.asarray(a)
    return np.where(np.isnan(a), NAN, np.where(a == np.inf, PINF, np.where(a == -np.inf, NINF, FINITE))).astype(np.int8)


def restate(kind, xyz, table, mode=0, rcut=RCUT):
    """The fp32 restatement of one per-kind entry point, in its column layout."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if kind == "distance":
            return npport.distances(xyz, table)
        if kind == "angle":
            return npport.angles(xyz, table)
        if kind == "contact":
            return npport.contacts(xyz, table, rcut)
        t = npport.dihedrals(xyz, table)
        t = np.where(t <= -PI32, t + np.float32(2 * np.pi), t).astype(np.float32)     # builtins.py:11-14, as the kernel
    if mode == 0:
        return t
    cs = np.stack([np.cos(t), np.sin(t)], axis=-1).astype(np.float32)
    return cs.reshape(t.shape[0], -1) if mode == 1 else np.hstack([cs[..., 0], cs[..., 1]])


# ---------------------------------------------------------------------------------------------- generators
def records(kind, m, A=A_ACC, seed=0):
    """m records of distinct atoms in [0, A): the first lists its atoms in descending order, the second is its
    reverse, the rest are random subsets in random order (half of the pairs then descend); with m > 3 every atom
    occurs in several records."""
    w = WIDTH["distance" if kind == "contact" else kind]
    rng = np.random.default_rng([seed, w, m])
    rec = np.stack([rng.permutation(A)[:w] for _ in range(m)]).astype(np.int32)
    rec[0] = np.arange(A - 1, A - 1 - w, -1)
    if m > 1:
        rec[1] = rec[0][::-1]
    return rec


def _chain(rng, n, A, lo, hi):
    """Nearly straight chains: atom a at a L e + delta w_a, delta log-uniform in [lo, hi) per frame: every triplet
    of a frame is nearly parallel or antiparallel with sin = O(delta)."""
    e = rng.normal(size=(n, 1, 3))
    e /= np.linalg.norm(e, axis=-1, keepdims=True)
    delta = np.exp(rng.uniform(np.log(lo), np.log(hi), size=(n, 1, 1)))
    step = rng.uniform(0.3, 0.7, size=(n, 1, 1))
    return np.arange(A)[None, :, None] * step * e + delta * rng.normal(size=(n, A, 3)) + rng.normal(size=(n, 1, 3))


@functools.lru_cache(maxsize=None)
def inputs(kind, regime, n=N_ACC, m=max(COUNTS), A=A_ACC):
    """(xyz float32 [n, A, 3], table int32 [m, width]) of one kind and coordinate regime, read-only.  One frame in
    eight is a nearly straight chain (angles: delta in [1e-7, 1e-2); dihedrals: [2e-3, 2e-2), and a frame in which a
    record's s falls below S_MIN after the rounding to fp32 is drawn again as a bulk frame); contacts: in one
    frame in five the first pair sits at rcut (1 +- g), g log-uniform in [1e-7, 1e-2)."""
    table = records(kind, m, A)
    rng = np.random.default_rng([11, sorted(WIDTH).index(kind) if kind in WIDTH else 3, int(REGIMES[regime]), n, m])
    x = rng.normal(size=(n, A, 3))
    if kind == "contact":
        x *= 0.5
        hard = np.arange(n) % 5 == 2
        i, j = table[0]
        e = rng.normal(size=(n, 3))
        e /= np.linalg.norm(e, axis=-1, keepdims=True)
        g = np.exp(rng.uniform(np.log(1e-7), np.log(1e-2), size=n)) * rng.choice([-1.0, 1.0], size=n)
        x[hard, j] = x[hard, i] + (RCUT * (1.0 + g))[hard, None] * e[hard]
    elif kind in ("angle", "dihedral"):
        hard = np.arange(n) % 8 == 3
        lo, hi = (1e-7, 1e-2) if kind == "angle" else (2e-3, 2e-2)
        x[hard] = _chain(rng, int(hard.sum()), A, lo, hi)
    xyz = (x + REGIMES[regime]).astype(np.float32)
    if kind == "dihedral":
        for _ in range(20):
            bad = (exact_dihedral(xyz, table)[1] < S_MIN).any(axis=1)
            if not bad.any():
                break
            xyz[bad] = (rng.normal(size=(int(bad.sum()), A, 3)) + REGIMES[regime]).astype(np.float32)
        assert not bad.any()
    xyz.setflags(write=False)
    table.setflags(write=False)
    return xyz, table


@functools.lru_cache(maxsize=None)
def exact(kind, regime, n=N_ACC, m=max(COUNTS), rows=None):
    """The exact law on inputs(kind, regime, n, m), computed once: distance d; (theta, sin); (t, s); contact (d,)."""
    xyz, table = inputs(kind, regime, n, m)
    if rows is not None:
        xyz = xyz[list(rows)]
    out = {"distance": exact_distance, "contact": exact_distance, "angle": exact_angle, "dihedral": exact_dihedral}[kind](xyz, table)
    for a in (out if isinstance(out, tuple) else (out,)):
        a.setflags(write=False)
    return out


def trip_rows(n=N_TRIP):
    """Rows of the second-trip checks: the first, the last two and 200 random ones."""
    rng = np.random.default_rng(257)
    return tuple(sorted({0, n - 2, n - 1} | set(rng.choice(n, 200, replace=False).tolist())))


def rg_frames(A, offset, n=37):
    rng = np.random.default_rng([5, A, int(offset)])
    return (rng.normal(size=(n, A, 3)) + offset).astype(np.float32)


def nonfinite_frames(n=300, A=A_ACC):
    """(bad xyz, clean xyz, bad-atom mask [n, A]): single coordinates of chosen atoms set to NaN, +inf, -inf; frame 40
    has two atoms at +inf in x (inf - inf), frame 41 a fully NaN atom, frame 100 a NaN and an inf, the last frame a NaN."""
    rng = np.random.default_rng(300)
    clean = rng.normal(size=(n, A, 3)).astype(np.float32)
    bad = clean.copy()
    for t, a, c, v in ((3, 2, 0, np.nan), (10, 5, 1, np.inf), (17, 7, 2, -np.inf), (40, 1, 0, np.inf), (40, 4, 0, np.inf),
                       (41, 0, 0, np.nan), (41, 0, 1, np.nan), (41, 0, 2, np.nan), (100, 11, 1, np.nan),
                       (100, 3, 2, np.inf), (177, 9, 0, -np.inf), (177, 8, 0, np.inf), (n - 1, 6, 2, np.nan)):
        bad[t, a, c] = v
    return bad, clean, ~np.isfinite(bad).all(axis=2)


def collinear_triplets():
    """(xyz [n, 3, 3], parallel [n], c [n]): vertex (atom 1) at the origin, atom 0 at 2^p v and atom 2 at m 2^p v with
    v a vector of small integers, m in +-{1, 2, 3}, p in {-8, 0, 9, 30}.  Every product and sum of the three dot
    products is exact in fp32 in any order and with or without contraction, so c = dot / (n1 n2), the unclamped
    cosine returned here, is fixed by two correctly rounded square roots, one product and one division: it is 1 or
    -1 exactly for some v, beyond for others (the clamp works) and inside (-1, 1) for the rest."""
    rng = np.random.default_rng(9)
    v = rng.integers(-9, 10, size=(200, 3))
    v = np.vstack([v[(v != 0).any(axis=1)], [[3, 4, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1], [2, 3, 6]]]).astype(np.float64)
    xyz, par = [], []
    for p in (-8, 0, 9, 30):
        for m in (1, 2, 3, -1, -2, -3):
            fr = np.zeros((len(v), 3, 3))
            fr[:, 0], fr[:, 2] = v * 2.0 ** p, m * v * 2.0 ** p
            xyz.append(fr)
            par.append(np.full(len(v), m > 0))
    xyz = np.concatenate(xyz).astype(np.float32)
    v1, v2 = xyz[:, 0], xyz[:, 2]
    n1, n2 = np.sqrt((v1 * v1).sum(-1, dtype=np.float32)), np.sqrt((v2 * v2).sum(-1, dtype=np.float32))
    return xyz, np.concatenate(par), ((v1 * v2).sum(-1, dtype=np.float32) / (n1 * n2)).astype(np.float32)


def planar_dihedrals():
    """(xyz [n, 4, 3], trans [n], lifted [n]): four atoms with small integer coordinates (times 2^p) in a coordinate plane,
    b1 along an axis: c0 and c1 are exact multiples of the third axis, x = c0.c1 is -1 (trans) or +1 (cis) and y is an
    exact zero.  That zero is +0.0: an exact cancellation rounds to +0, and -0.0 would need all three products of the
    last dot product to be -0, which no finite planar input gives.  The -pi branch of atan2 is reached instead by
    the `lifted` copies of the trans cases, whose last atom is 2^-30 above or below the plane: y = -+2^-30 / |b2|,
    x = -1 to rounding, and atan2 rounds to -+float32(pi)."""
    xyz, trans, lifted = [], [], []
    for a in range(3):
        for b in range(3):
            if a == b:
                continue
            ea, eb, ec = np.eye(3)[a], np.eye(3)[b], np.eye(3)[3 - a - b]
            for length in (1.0, -2.0):
                for al, be, ga, de in ((0, 1, 0, -1), (0, -1, 0, 1), (1, 2, -1, -3), (-2, -1, 3, 2), (0, 1, 0, 1),
                                       (0, -1, 0, -2), (1, 3, 2, 1), (-1, -2, 0, -1)):
                    for p in (-6, 0, 11):
                        for lift in ((0.0,) if be * de > 0 or p else (0.0, 2.0 ** -30, -2.0 ** -30)):
                            p1 = np.array([1.0, -2.0, 3.0]) * (lift == 0)
                            p2 = p1 + length * ea
                            xyz.append(np.stack([p1 + al * ea + be * eb, p1, p2, p2 + ga * ea + de * eb + lift * ec]) * 2.0 ** p)
                            trans.append(be * de < 0)
                            lifted.append(lift != 0)
    return np.asarray(xyz, np.float32), np.asarray(trans), np.asarray(lifted)


def dihedral_xy32(xyz, quads, eps=1e-12):
    """x and y of oracle.npport.dihedrals (the same fp32 operations) ahead of its mask and atan2."""
    xyz, q, e = np.asarray(xyz, np.float32), np.asarray(quads), np.float32(eps)
    b0, b1, b2 = xyz[:, q[:, 1]] - xyz[:, q[:, 0]], xyz[:, q[:, 2]] - xyz[:, q[:, 1]], xyz[:, q[:, 3]] - xyz[:, q[:, 2]]
    c0, c1 = np.cross(b0, b1), np.cross(b1, b2)
    c0 = c0 / np.sqrt(np.maximum((c0 * c0).sum(-1), e))[..., None]
    c1 = c1 / np.sqrt(np.maximum((c1 * c1).sum(-1), e))[..., None]
    b1u = b1 / np.sqrt(np.maximum((b1 * b1).sum(-1), e))[..., None]
    return (c0 * c1).sum(-1), (np.cross(c0, c1) * b1u).sum(-1)


def collinear_quads():
    """xyz [n, 4, 3]: four atoms on one line through integer points, in several orders and scales: c0 = c1 = 0 exactly,
    the floor holds the norms at sqrt(eps), x = y = 0 and the extractor's mask gives the angle 0."""
    out = []
    for v in ([1, 0, 0], [1, 2, 3], [-2, 5, 1]):
        for ks in ((0, 1, 2, 3), (3, 1, 2, 0), (0, 2, 1, 5), (-1, 4, 2, 2)):
            for p in (-4, 0, 8):
                out.append((np.array([2.0, -1.0, 4.0]) + np.outer(ks, v)) * 2.0 ** p)
    return np.asarray(out, np.float32)


def reads_bad(mask, table):
    """[n, m]: record f of frame t reads an atom with a non-finite coordinate."""
    return mask[:, np.asarray(table)].any(axis=2)


# ---------------------------------------------------------------------------------------------- yardsticks
def k_values(kind, xyz, table, ex):
    """Per entry K of the fp32 restatement against the exact law `ex` (the module docstring has the definitions)."""
    got = restate(kind, xyz, table).astype(LD)
    if kind == "distance":
        return np.abs(got - ex) / (U * ex)
    if kind == "angle":
        return np.abs(got - ex[0]) * np.maximum(ex[1], SQRT_U) / U
    return wrap_diff(got, ex[0]) * np.maximum(ex[1], SQRT_U) / U


def every_input():
    """(kind, regime, n, m, rows) of every generated input the accuracy bounds are applied to."""
    for kind in WIDTH:
        for regime in REGIMES:
            yield kind, regime, N_ACC, max(COUNTS), None
        yield kind, "off50", N_TRIP, M_TRIP, trip_rows()


def measure_yardsticks():
    """{kind: (largest K, fraction of entries with sin < 0.01 per input)}."""
    out = {}
    for kind, regime, n, m, rows in every_input():
        xyz, table = inputs(kind, regime, n, m)
        ex = exact(kind, regime, n, m, rows)
        k = k_values(kind, xyz if rows is None else xyz[list(rows)], table, ex)
        frac = float((ex[1] < 0.01).mean()) if kind != "distance" else 1.0
        worst, fracs = out.get(kind, (0.0, []))
        out[kind] = (max(worst, float(k.max())), fracs + [frac])
    return out
