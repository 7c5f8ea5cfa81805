"""Host-only companions of tests/test_gpu_cov_paths.py (numpy, no GPU).

exact_moments / exact_column_sums   the lagged covariance moments and the column sums of csrc/cov.hip as plain
                                    per-segment slicing, in int64 when the centred data are integers
small / wide / fp64_only            data for which every product and every partial sum of the moments is an exact fp64
                                    number, so a correct kernel is BIT-equal to the reference in any summation order
cov_path                            the launch rule of cov.hip restated (build_frametab, dispatch_cov, launch_cov,
                                    launch_cov_blocked and the head / ring / tail split inside a wave)
CASES                               the table the GPU test runs; each row names the branch it is there to reach, and
                                    tests/test_cov_reference.py proves with cov_path that it does

The constants below restate cov.hip; a change there has to be made here too (the CPU test compares the two wherever
the library says something about its path, the GPU test wherever the results depend on it)."""

from __future__ import annotations

import numpy as np

SEG_INLINE = 16          # MSM_SEG_INLINE
K_WAVES = 4              # frame waves of a workgroup
K_GROUP = 4              # frames per matrix instruction
K_DEPTH = 3              # groups in flight in the interior ring
MIN_GROUPS_PER_WAVE = 4
FLAVOURS = ("plain", "symmetric", "onesided")
SENTINEL = 2.0 ** 100    # finite, exact in fp32 and fp64: a read of a pad column or of a frame outside the segments
BIG = 2 ** 25 + 1        # not an fp32 number


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def clip_segments(n: int, segs):
    """(start, stop) clipped to [0, n]; None is the one segment [0, n).  Empty ones stay in the list (length <= 0)."""
    if segs is None:
        return [(0, int(n))]
    return [(max(0, int(a)), min(int(n), int(b))) for a, b in segs]


def _centred(X, shift, impute_nan: bool):
    X = np.asarray(X, np.float64)
    Z = X - np.asarray(shift, np.float64)[None, :]
    nan = np.isnan(X)
    if nan.any():
        if not impute_nan:
            raise ValueError("NaN in the data and impute_nan is off")
        Z = np.where(nan, 0.0, Z)
    if Z.size and np.all(Z == np.rint(Z)) and np.abs(Z).max() < 2.0 ** 31:
        return Z.astype(np.int64)        # integer data: int64 arithmetic, exact by construction
    return Z


def _gram(x, y):
    """x'y.  Integers: int64 sums of row blocks short enough that a block's fp64 matrix product is exact (every partial
    sum below 2^53 in magnitude), which is int64 arithmetic at the speed of the BLAS.  Floats: the plain product."""
    if x.dtype != np.int64:
        return x.T @ y
    out = np.zeros((x.shape[1], y.shape[1]), np.int64)
    if x.shape[0] == 0:
        return out
    peak = max(1, int(np.abs(x).max())) * max(1, int(np.abs(y).max()))
    assert peak <= 2 ** 53, "a single product is not an fp64 number"
    rows = max(1, 2 ** 53 // peak)
    for r0 in range(0, x.shape[0], rows):
        out += (x[r0:r0 + rows].astype(np.float64).T @ y[r0:r0 + rows].astype(np.float64)).astype(np.int64)
    return out


def exact_moments(X, segs, lag: int, shift, flavour: str = "plain", impute_nan: bool = False) -> dict:
    """M00 [F, F], M0t [F, F], sx [F], sy [F] (float64) and T (int) of the frames X [n, F] about `shift`.

    Per segment [a, b) longer than the lag: x = Z[a:b-lag], y = Z[a+lag:b] and
        plain      M00 = x'x + y'y     M0t = x'y
        symmetric  M00 = x'x + y'y     M0t = (x'y + y'x) / 2
        onesided   M00 = x'x           M0t = x'y
    sx = sum of x, sy = sum of y, T = number of pairs, in every flavour.  lag = 0 is the instantaneous covariance."""
    if flavour not in FLAVOURS:
        raise ValueError(flavour)
    n, F = np.shape(X)
    Z = _centred(X, shift, impute_nan)
    M00 = np.zeros((F, F), Z.dtype)
    M0t = np.zeros((F, F), Z.dtype)
    sx = np.zeros(F, Z.dtype)
    sy = np.zeros(F, Z.dtype)
    T = 0
    for a, b in clip_segments(n, segs):
        if b - a <= lag:
            continue
        x, y = Z[a:b - lag], Z[a + lag:b]
        T += b - a - lag
        sx += x.sum(axis=0)
        sy += y.sum(axis=0)
        M00 += _gram(x, x)
        if flavour != "onesided":
            M00 += _gram(y, y)
        M0t += _gram(x, y)
    M0t = M0t.astype(np.float64)
    if flavour == "symmetric":
        M0t = (M0t + M0t.T) / 2.0
    return {"M00": M00.astype(np.float64), "M0t": M0t, "sx": sx.astype(np.float64), "sy": sy.astype(np.float64),
            "T": int(T)}


def exact_column_sums(X, segs, shift) -> np.ndarray:
    """[count | S1 | S2] (3F float64) over ALL frames of the segments, the short ones included: what
    msm_moments_from_lagged rebuilds from the plain lagged moments and the segment edges."""
    n, F = np.shape(X)
    Z = _centred(X, shift, False)
    cnt = 0
    s1 = np.zeros(F, Z.dtype)
    s2 = np.zeros(F, Z.dtype)
    for a, b in clip_segments(n, segs):
        if b <= a:
            continue
        cnt += b - a
        s1 += Z[a:b].sum(axis=0)
        s2 += (Z[a:b] * Z[a:b]).sum(axis=0)
    return np.concatenate([np.full(F, float(cnt)), s1.astype(np.float64), s2.astype(np.float64)])


def brute_moments(X, segs, lag: int, shift, flavour: str = "plain") -> dict:
    """exact_moments as a triple loop over pairs and features (tiny shapes only): no slicing, no matrix product."""
    n, F = np.shape(X)
    Z = _centred(X, shift, False)
    M00 = [[0] * F for _ in range(F)]
    Mxy = [[0] * F for _ in range(F)]
    sx, sy, T = [0] * F, [0] * F, 0
    for a, b in clip_segments(n, segs):
        for t in range(a, b - lag):
            T += 1
            for i in range(F):
                xi, yi = Z[t, i].item(), Z[t + lag, i].item()
                sx[i] += xi
                sy[i] += yi
                for j in range(F):
                    M00[i][j] += xi * Z[t, j].item()
                    if flavour != "onesided":
                        M00[i][j] += yi * Z[t + lag, j].item()
                    Mxy[i][j] += xi * Z[t + lag, j].item()
    M00, Mxy = np.array(M00, np.float64).reshape(F, F), np.array(Mxy, np.float64).reshape(F, F)
    if flavour == "symmetric":
        Mxy = (Mxy + Mxy.T) / 2.0
    return {"M00": M00, "M0t": Mxy, "sx": np.array(sx, np.float64), "sy": np.array(sy, np.float64), "T": T}


def magnitude_bound(X, segs, lag: int, shift) -> float:
    """An upper bound of |every partial sum| any summation order of any flavour can meet: the moments of |z|, with
    the symmetric accumulation sum (|x| + |y|)(|x| + |y|)' = M00 + M0t + M0t' as the largest of them."""
    Za = np.abs(_centred(X, shift, True)).astype(np.float64)
    m = exact_moments(Za, segs, lag, np.zeros(Za.shape[1]), "plain")
    return float((m["M00"] + m["M0t"] + m["M0t"].T).max(initial=0.0))


# ---------------------------------------------------------------------------------------------------------------------
# data: integers, so that sums are exact below 2^53 whatever their order
# ---------------------------------------------------------------------------------------------------------------------
def small(n: int, F: int, seed: int):
    """Integers in [-3, 3]; column 1 is t % 5, which makes M0t asymmetric.  -> (X float64, integer shift)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, size=(n, F)).astype(np.float64)
    if F > 1:
        X[:, 1] = np.arange(n) % 5
    return X, rng.integers(-2, 3, size=F).astype(np.float64)


def wide(n: int, F: int, seed: int):
    """Integers in [-4095, 4095]: fp32 numbers whose products and sums pass 2^24 at once."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-4095, 4096, size=(n, F)).astype(np.float64)
    if F > 1:
        X[:, 1] = (np.arange(n) % 5) * 1000.0
    return X, rng.integers(-100, 101, size=F).astype(np.float64)


def fp64_only(n: int, F: int, seed: int, among=None):
    """`small` plus at most four frames (of `among`, default all) that hold +-(2^25 + 1) in one column each (distinct
    columns, so no sum of squares collects more than one of them): an input narrowed to fp32 loses the + 1."""
    X, shift = small(n, F, seed)
    rng = np.random.default_rng(seed + 7)
    among = np.arange(n) if among is None else np.asarray(among)
    k = min(4, F, len(among))
    frames = rng.choice(among, size=k, replace=False)
    cols = rng.choice(F, size=k, replace=False)
    for q, (t, c) in enumerate(zip(frames, cols)):
        X[t, c] = BIG if q % 2 == 0 else -BIG
    return X, shift


FAMILIES = {"small": small, "wide": wide, "fp64_only": fp64_only}


def case_data(row: dict):
    """(X [n, F] float64 holding numbers of the row's dtype, shift [F]) of a resolved row."""
    if row["family"] == "fp64_only" and row["dtype"] != "f64":
        raise ValueError("the fp64-only family needs fp64 input")
    if row["family"] == "fp64_only":     # the large values go to frames the moments read
        live = [np.arange(a, b) for a, b in clip_segments(row["n"], row["segs"]) if b - a > row["lag"]]
        return fp64_only(row["n"], row["F"], row["seed"], among=np.concatenate(live))
    return FAMILIES[row["family"]](row["n"], row["F"], row["seed"])


# ---------------------------------------------------------------------------------------------------------------------
# the launch rule
# ---------------------------------------------------------------------------------------------------------------------
def _ceil_to(v: int, m: int) -> int:
    return -(-v // m) * m


def build_frametab(n: int, segs, lag: int):
    """Live segments (longer than the lag, clipped), their padded prefix and the pair count; None when there are more
    than SEG_INLINE of them (MSM_ERR_UNSUPPORTED)."""
    live, prefix, pairs = [], [0], 0
    for a, b in clip_segments(n, segs):
        if b - a <= lag:
            continue
        if len(live) == SEG_INLINE:
            return None
        live.append((a, b))
        prefix.append(prefix[-1] + _ceil_to(b - a, K_GROUP))
        pairs += b - a - lag
    return {"segs": live, "prefix": prefix, "total": prefix[-1], "pairs": pairs}


def _pieces(ft: dict, lag: int, fpw: int, n_waves: int, vec_ring: bool):
    """Every (wave, segment) piece of the partition with its head / ring / tail group counts."""
    out = []
    for w in range(n_waves):
        q0, q_end = w * fpw, min((w + 1) * fpw, ft["total"])
        seg = 0
        while q0 < q_end:
            while seg + 1 < len(ft["segs"]) and q0 >= ft["prefix"][seg + 1]:
                seg += 1
            a, b = ft["segs"][seg]
            q_hi = min(q_end, ft["prefix"][seg + 1])
            length = b - a
            o_b, o_e = q0 - ft["prefix"][seg], q_hi - ft["prefix"][seg]
            o_i0 = o_i1 = o_b
            if vec_ring:
                if o_b < lag:
                    o_i0 = o_b + _ceil_to(lag - o_b, 4)
                lim = length - lag - 3
                o_i1 = o_i0 + _ceil_to(lim - o_i0, 4) if lim > o_i0 else o_i0
                o_i0 = min(o_i0, o_e)
                o_i1 = max(min(o_i1, o_e), o_i0)
            n_groups = (o_i1 - o_i0) // 4
            ring = n_groups if n_groups >= 2 * K_DEPTH else 0
            out.append({"wave": w, "seg": seg, "o_b": o_b, "o_e": o_e, "len": length, "head": (o_i0 - o_b) // 4,
                        "ring": ring, "short": n_groups - ring, "tail": (o_e - o_i1) // 4})
            q0 = q_hi
    return out


def cov_path(n: int, F: int, ld: int, itemsize: int, aligned: bool, segs, lag: int, flavour: str, n_cu: int) -> dict:
    """What msm_lagged_moments[_reversible|_onesided] launches for this call.  `aligned`: the base pointer is a fresh
    allocation; otherwise it lies one element past one."""
    assert flavour in FLAVOURS and ld >= F >= 1 and lag >= 0
    ft = build_frametab(n, segs, lag)
    if ft is None:
        return {"status": "unsupported"}
    if ft["total"] == 0:
        return {"status": "empty", "pairs": 0}
    sym = flavour == "symmetric"
    p = {"status": "ok", "pairs": ft["pairs"], "total": ft["total"], "n_live": len(ft["segs"]),
         "one_sided": flavour == "onesided"}
    groups = ft["total"] // K_GROUP
    off = 0 if aligned else 1
    if F > 64:
        n_fb = (F + 63) // 64
        n_tasks = n_fb * n_fb + n_fb * (n_fb + 1) // 2
        chunks = max(1, n_cu * 2 // n_tasks)
        if chunks * 4 * 4 > groups:
            chunks = max(1, groups // 16)
        fpw = _ceil_to(-(-ft["total"] // (chunks * 4)), K_GROUP)
        chunks = -(-ft["total"] // (fpw * 4))
        p.update(blocked=True, NT=4, n_fb=n_fb, n_tasks=n_tasks, chunks=chunks, blocks=chunks, split=False,
                 vec=F % 64 == 0 and ld % 4 == 0 and off % 4 == 0, sym_kernel=False, symmetrise=sym,
                 frames_per_wave=fpw, pieces=_pieces(ft, lag, fpw, chunks * 4, False))
        return p
    NT = (F + 15) // 16
    blocks = n_cu
    if blocks * K_WAVES * MIN_GROUPS_PER_WAVE > groups:
        blocks = max(1, groups // (K_WAVES * MIN_GROUPS_PER_WAVE))
    fpw = _ceil_to(-(-ft["total"] // (blocks * K_WAVES)), K_GROUP)
    blocks = -(-ft["total"] // (fpw * K_WAVES))
    vec = NT != 3 and F == 16 * NT and ld % NT == 0 and off % NT == 0 and ld * 4 * itemsize < 2 ** 31
    p.update(blocked=False, NT=NT, n_fb=0, n_tasks=0, chunks=0, blocks=blocks, split=NT >= 3, vec=vec,
             sym_kernel=sym and NT >= 3, symmetrise=sym and NT < 3, frames_per_wave=fpw,
             pieces=_pieces(ft, lag, fpw, blocks * K_WAVES, vec))
    return p


def reached(p: dict, lag: int) -> dict:
    """The branches of a path in the vocabulary of a row's `reach`."""
    if p["status"] != "ok":
        return {"status": p["status"]}
    pieces = p["pieces"]
    per_wave: dict = {}
    for q in pieces:
        per_wave.setdefault(q["wave"], set()).add(q["seg"])
    return {
        "status": "ok", "NT": p["NT"], "vec": p["vec"], "split": p["split"], "blocked": p["blocked"],
        "n_fb": p["n_fb"], "sym_kernel": p["sym_kernel"], "symmetrise": p["symmetrise"], "n_live": p["n_live"],
        "ring": {q["ring"] for q in pieces if q["ring"]},
        "short": {q["short"] for q in pieces if q["short"]} if p["vec"] and not p["blocked"] else set(),
        "head": any(q["head"] for q in pieces), "tail": any(q["tail"] for q in pieces),
        "mid_start": any(0 < q["o_b"] < lag for q in pieces),                 # a chunk that starts inside the head
        "span": max(len(s) for s in per_wave.values()),                       # segments under one wave
        "tiny_seg": any(q["len"] < K_GROUP for q in pieces),
        "lag_gt_fpw": lag > p["frames_per_wave"],
        "multi_block": p["blocks"] > 1,
    }


def covers(got: dict, want: dict) -> list:
    """The entries of a row's `reach` that a path does not deliver (empty: all reached).  Sets are lower bounds,
    `span` is a minimum, everything else is compared for equality."""
    miss = []
    for k, v in want.items():
        g = got.get(k)
        if g is None:
            miss.append((k, v, g))
            continue
        ok = (v <= g) if isinstance(v, (set, frozenset)) else (g >= v) if k == "span" else (g == v)
        if not ok:
            miss.append((k, v, g))
    return miss


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
ITEMSIZE = {"f32": 4, "f64": 8}
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
CASES: list = []


def _row(name, n, F, lag, reach, *, ld=None, dtype="f32", aligned=True, segs=None, flavour="plain", family="small",
         pick=None):
    assert name not in {r["name"] for r in CASES}, name
    CASES.append({"name": name, "n": n, "F": F, "lag": lag, "ld": F if ld is None else ld, "dtype": dtype,
                  "aligned": aligned, "segs": segs, "flavour": flavour, "family": family, "reach": reach,
                  "pick": pick, "seed": 1000 + len(CASES)})


# -- one segment, one workgroup: the ring at 6, 7 and 8 groups ---------------------------------------------------
# total = 124 padded frames -> blocks = 1, 32 frames per wave whatever n_cu.  Wave 0 loses its first group(s) to the
# weighted head (o_b = 0 < lag), waves 1 and 2 are all interior (8 groups), wave 3 ends in the weighted tail.
_RING_BASES = [   # (n, lag, ring lengths, too-short interior runs)
    (121, 1, {6, 7, 8}, set()),     # len = 1 mod 4
    (122, 2, {6, 7, 8}, set()),     # len = 2 mod 4
    (123, 3, {6, 7, 8}, set()),     # len = 3 mod 4
    (124, 4, {6, 7, 8}, set()),     # len = 0 mod 4
    (124, 5, {6, 8}, {5}),          # wave 0 starts at offset 8, wave 3 keeps 5 interior groups: run_general
    (124, 0, {7, 8}, set()),        # lag 0: no head at all
    (97, 1, {6, 7}, {3}),           # total = 100: 28 frames per wave, 16 for the last one
    (113, 1, {7, 8}, {4}),          # total = 116, len = 1 mod 4: the last group holds one frame
]
_q = 0
for _NT in (1, 2, 4):
    for _dtype in ("f32", "f64"):
        for _flavour in FLAVOURS:
            for _rep in range(2):
                _n, _lag, _ring, _short = _RING_BASES[_q % len(_RING_BASES)]
                _fam = ("small", "wide", "fp64_only")[_q % 3] if _dtype == "f64" else ("small", "wide")[_q % 2]
                _F = 16 * _NT
                _row(f"ring-nt{_NT}-{_dtype}-{_flavour}-n{_n}-lag{_lag}", _n, _F, _lag,
                     {"NT": _NT, "vec": True, "blocked": False, "split": _NT >= 3, "ring": _ring, "short": _short,
                      "sym_kernel": _flavour == "symmetric" and _NT >= 3,
                      "symmetrise": _flavour == "symmetric" and _NT < 3, "multi_block": False},
                     ld=_F + (4 if _q % 2 else 0), dtype=_dtype, flavour=_flavour, family=_fam)
                _q += 1

# -- guarded loads: F below the tile, ld or the pointer off the vector's alignment, NT = 3 -----------------------
_SEGS_MIXED = [(-5, 9), (9, 12), (14, 15), (20, 41), (41, 43), (50, 57), (60, 66), (66, 71), (80, 300)]   # n = 131
_GUARDED = [   # (F, ld, aligned, NT)
    (1, 1, True, 1), (13, 13, True, 1), (15, 19, False, 1),
    (17, 17, True, 2), (32, 33, True, 2), (32, 32, False, 2), (20, 22, True, 2),
    (33, 33, True, 3), (40, 44, True, 3), (48, 48, True, 3), (48, 51, False, 3),
    (49, 49, True, 4), (64, 66, True, 4), (64, 64, False, 4), (50, 52, True, 4), (64, 68, False, 4),
]
for _i, (_F, _ld, _al, _NT) in enumerate(_GUARDED):
    for _j, _dtype in enumerate(("f32", "f64")):
        _flavour = FLAVOURS[(_i + _j) % 3]
        _fam = ("small", "wide", "fp64_only")[(_i + _j) % 3] if _dtype == "f64" else ("wide", "small")[_i % 2]
        _row(f"guarded-F{_F}-ld{_ld}-{'al' if _al else 'mis'}-{_dtype}-{_flavour}", 131, _F, 1 + _i % 4,
             {"NT": _NT, "vec": False, "blocked": False, "split": _NT >= 3, "ring": set(),
              "sym_kernel": _flavour == "symmetric" and _NT >= 3, "symmetrise": _flavour == "symmetric" and _NT < 3},
             ld=_ld, dtype=_dtype, aligned=_al, segs=_SEGS_MIXED, flavour=_flavour, family=_fam)
# the missing (NT, flavour) pairs of the guarded kernels, on one segment with the one-pair lag
for _F, _NT, _flavour, _dtype in ((13, 1, "symmetric", "f32"), (20, 2, "plain", "f64"), (40, 3, "onesided", "f32"),
                                  (50, 4, "symmetric", "f64"), (50, 4, "plain", "f32"), (40, 3, "plain", "f64"),
                                  (40, 3, "symmetric", "f32"), (20, 2, "onesided", "f32"), (20, 2, "symmetric", "f64"),
                                  (13, 1, "onesided", "f64"), (13, 1, "plain", "f32"), (50, 4, "onesided", "f64")):
    _row(f"onepair-F{_F}-{_dtype}-{_flavour}", 70, _F, 69,
         {"NT": _NT, "vec": False, "ring": set(), "lag_gt_fpw": True, "mid_start": True},
         dtype=_dtype, flavour=_flavour, family="wide")

# -- segment structure on the vector kernels ------------------------------------------------------------------
# sixteen live segments of every length class, gaps, clipping at both ends and short ones that are skipped
_SEGS_16 = [(-3, 5), (5, 6), (8, 11), (11, 18), (20, 22), (22, 28), (30, 39), (39, 49), (49, 51), (60, 71), (71, 75),
            (75, 76), (80, 85), (85, 91), (91, 98), (100, 103), (103, 111), (111, 120), (130, 142), (150, 900)]
for _F, _dtype, _flavour, _lag, _live in ((16, "f32", "plain", 1, 16), (32, "f64", "symmetric", 2, 16),
                                          (64, "f32", "symmetric", 2, 16), (64, "f64", "onesided", 2, 16),
                                          (64, "f32", "plain", 3, 14)):
    _segs = _SEGS_16 if _lag != 1 else _SEGS_16[:12] + _SEGS_16[14:]     # lag 1 keeps the two-frame segments alive
    _row(f"segments-F{_F}-{_dtype}-{_flavour}-lag{_lag}", 170, _F, _lag,
         {"vec": True, "n_live": _live, "span": 3, "tiny_seg": _lag < 3, "tail": True,
          "head": True}, dtype=_dtype, segs=_segs, flavour=_flavour, family="wide" if _F == 64 else "small")
# lag beyond a wave's chunk, chunks that start inside the head, more than one workgroup
for _F, _dtype, _flavour, _n, _lag in ((16, "f64", "plain", 203, 61), (32, "f32", "onesided", 202, 62),
                                       (64, "f64", "symmetric", 201, 63), (64, "f32", "plain", 200, 60),
                                       (48, "f32", "symmetric", 203, 61), (100, "f32", "plain", 202, 62)):
    _row(f"longlag-F{_F}-{_dtype}-{_flavour}", _n, _F, _lag,
         {"lag_gt_fpw": True, "mid_start": True, "multi_block": True, "vec": _F in (16, 32, 64)},
         dtype=_dtype, flavour=_flavour, family="fp64_only" if _dtype == "f64" else "wide")
# lag = len - 1 on the vector kernels: one pair, everything is head and tail
for _F, _dtype, _flavour in ((16, "f32", "symmetric"), (32, "f64", "plain"), (64, "f32", "onesided")):
    _row(f"onepair-vec-F{_F}-{_dtype}-{_flavour}", 37, _F, 36, {"vec": True, "ring": set(), "short": set()},
         dtype=_dtype, flavour=_flavour)

# -- the blocked kernel (F > 64) -----------------------------------------------------------------------------------
_SEGS_BLK = [(0, 77), (77, 79), (90, 131), (131, 134), (140, 400)]    # n = 190
for _F, _ld, _al, _nfb, _vec in ((65, 65, True, 2, False), (100, 104, True, 2, False), (128, 128, True, 2, True),
                                 (128, 132, True, 2, True), (128, 130, True, 2, False), (128, 128, False, 2, False),
                                 (129, 129, True, 3, False), (192, 192, True, 3, True), (150, 152, False, 3, False)):
    for _j, _dtype in enumerate(("f32", "f64")):
        _flavour = FLAVOURS[(_F + _ld + _j) % 3]
        _row(f"blocked-F{_F}-ld{_ld}-{'al' if _al else 'mis'}-{_dtype}-{_flavour}", 190, _F, 2 + _j,
             {"blocked": True, "n_fb": _nfb, "vec": _vec, "symmetrise": _flavour == "symmetric", "sym_kernel": False,
              "span": 2}, ld=_ld, dtype=_dtype, aligned=_al, segs=_SEGS_BLK, flavour=_flavour,
             family=("small", "wide")[_j] if _dtype == "f32" else ("wide", "fp64_only")[_F % 2])

# -- long rings: n depends on the device -----------------------------------------------------------------------------
# One segment of n = 4 n_cu * 4 g - 4 frames gives every wave g groups: g - 1 in wave 0 (the head), g in the middle,
# g - 2 in the last wave (its chunk is one group short and ends in the tail group).  g = 11 -> {9, 10, 11}: every
# residue mod 3 with at least two trips of the steady loop.  resolve() finds n with cov_path.
for _F, _dtype, _flavour, _fam, _lag, _ring, _ld in (
        (64, "f32", "plain", "wide", 1, {9, 10, 11}, 64), (64, "f64", "symmetric", "fp64_only", 2, {9, 10, 11}, 68),
        (32, "f64", "onesided", "wide", 3, {9, 10, 11}, 34), (16, "f32", "symmetric", "small", 4, {9, 10, 11}, 16),
        (64, "f32", "symmetric", "wide", 50, {9, 11}, 64)):
    _row(f"longring-F{_F}-{_dtype}-{_flavour}-lag{_lag}", None, _F, _lag,
         {"vec": True, "ring": _ring, "multi_block": True, "mid_start": _lag > 44, "lag_gt_fpw": _lag > 44},
         ld=_ld, dtype=_dtype, flavour=_flavour, family=_fam, pick={"groups": 11})

N_CU_CHECKED = (256, 304, 64)


def row_path(row: dict, n_cu: int) -> dict:
    return cov_path(row["n"], row["F"], row["ld"], ITEMSIZE[row["dtype"]], row["aligned"], row["segs"], row["lag"],
                    row["flavour"], n_cu)


def resolve(row: dict, n_cu: int) -> dict:
    """The row with a concrete n: rows with `pick` take the largest n near 16 n_cu g at which cov_path delivers the
    row's `reach` on a device of n_cu compute units."""
    if row["pick"] is None:
        return row
    n0 = K_WAVES * n_cu * K_GROUP * row["pick"]["groups"]
    for n in range(n0, n0 - 64, -1):
        r = dict(row, n=n)
        if not covers(reached(row_path(r, n_cu), r["lag"]), r["reach"]):
            return r
    raise AssertionError(f"{row['name']}: no n near {n0} reaches {row['reach']} at n_cu = {n_cu}")


def case_ids():
    return [r["name"] for r in CASES]
