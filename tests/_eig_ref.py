"""Launch-path rule, prescribed-spectrum inputs and shared checks for pmarlo_amd/csrc/eig.hip (TEST INFRASTRUCTURE).

The three single-workgroup solvers of eig.hip (msm_tica_solve, msm_eigh, msm_onesided_tica_eigenvalues) pick their code
path from the matrix order and the data alone.  `tica_path`, `eigh_path` and `onesided_path` restate that choice from
the launchers' own byte formulas; the builders make inputs whose spectrum is prescribed, so the truth needs no
eigensolve: the products are formed in np.longdouble and rounded to float64 once.  The check functions take solver
outputs as numpy arrays, so tests/test_eig_reference.py (numpy, CPU) and tests/test_gpu_eig_paths.py (device) share
them.  Nothing here is imported by the product."""

from __future__ import annotations

import functools

import numpy as np

from oracle import npport
from tests import _gen

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble

# ---- the launch-path rule (eig.hip: kEigThreads, kTriMax, kTriLd and the three LDS budgets) ----------------------
THREADS = 1024
TRI_MAX = 64
TRI_LD = 65
TICA_LDS_BUDGET = 150 * 1024
EIGH_LDS_BUDGET = 140 * 1024
ONESIDED_LDS_BUDGET = 140 * 1024
MAX_ORDER = 256
JACOBI_MAX_SWEEPS = 40     # the cap every caller of jacobi_eigh passes: a count of 40 means the loop ran out
# a workgroup's 160 KiB of LDS also hold the kernels' own __shared__ structs (sizeof JacobiShared, TriShared): every
# kernel that can reach the tridiagonal solver carries both, tica_solve_kernel<2> only the first
LDS_PER_WORKGROUP = 160 * 1024
STATIC_LDS_JACOBI = 5808
STATIC_LDS_TRI = 5808 + 21808


def lds_cap(budget: int, static_bytes: int) -> int:
    return min(budget, LDS_PER_WORKGROUP - static_bytes)


def row_stride(n: int) -> int:
    """ld of every launcher: the tridiagonal solver's fixed stride up to 64, an odd stride above."""
    return TRI_LD if n <= TRI_MAX else (n | 1)


def jacobi_variant(n: int, ld: int) -> str:
    """Which Jacobi runs on an n x n problem of row stride ld (the test at the head of jacobi_eigh)."""
    if n < 2:
        return "none"
    mh = n // 2
    if n % 2 == 0 and 4 <= mh <= 32 and mh * mh <= THREADS and mh * n <= 2 * THREADS and n * ld < 65536:
        return "pipelined"
    return "generic"


def tica_path(F: int, rank: int | None = None) -> dict:
    """msm_tica_solve for order F when C00 keeps `rank` directions (None or F: full rank)."""
    ld = row_stride(F)
    mat_bytes = F * ld * 8
    lds_mats = 4 if 4 * mat_bytes <= lds_cap(TICA_LDS_BUDGET, STATIC_LDS_TRI) else (
        2 if 2 * mat_bytes <= lds_cap(TICA_LDS_BUDGET, STATIC_LDS_JACOBI) else 0)
    fused = lds_mats == 4 and F <= TRI_MAX
    full = rank is None or rank == F
    r = F if full else int(rank)
    if full:
        first = "ldl_registers" if fused else "cholesky_pair"
    else:
        first = "jacobi_" + jacobi_variant(F, ld)
    # the tridiagonal solver is tried when all four matrices sit in LDS and the problem fits it; it refuses any
    # stride but its own (order 1 returns before that test)
    tri = lds_mats == 4 and r <= TRI_MAX and (ld == TRI_LD or r == 1) and r >= 1
    return {"ld": ld, "lds_mats": lds_mats, "fused": fused,
            "kernel": "fused" if fused else {4: "lds4", 2: "lds2", 0: "global"}[lds_mats],
            "first": first, "second": "tridiag" if tri else "jacobi_" + jacobi_variant(r, ld),
            "second_fallback": "jacobi_" + jacobi_variant(r, ld), "tail": "lds" if fused else "generic"}


def eigh_path(n: int) -> dict:
    ld = row_stride(n)
    lds = (3 if n <= TRI_MAX else 2) * n * ld * 8
    use_lds = lds <= lds_cap(EIGH_LDS_BUDGET, STATIC_LDS_TRI)
    tri = use_lds and n <= TRI_MAX
    return {"ld": ld, "storage": "lds" if use_lds else "global", "solver": "tridiag" if tri else "jacobi",
            "jacobi": jacobi_variant(n, ld)}


def onesided_path(F: int) -> dict:
    ld = row_stride(F)
    use_lds = 4 * F * ld * 8 <= lds_cap(ONESIDED_LDS_BUDGET, STATIC_LDS_TRI)
    return {"ld": ld, "storage": "lds" if use_lds else "global",
            "solver": "tridiag" if use_lds and F <= TRI_MAX else "jacobi", "jacobi": jacobi_variant(F, ld)}


# ---- orthogonal factors good to long-double rounding --------------------------------------------------------------
def _orthogonal(n: int, rng) -> np.ndarray:
    """Random orthogonal n x n matrix in np.longdouble: float64 QR, then two Newton-Schulz steps in long double
    (the defect of the float64 factor, ~1e-15, squares away to the long-double rounding level)."""
    q = np.linalg.qr(rng.normal(size=(n, n)))[0].astype(LD)
    eye = np.eye(n, dtype=LD)
    for _ in range(2):
        q = np.dot(q, (3 * eye - np.dot(q.T, q)) / 2)
    return q


@functools.lru_cache(maxsize=None)
def _orthogonal_cached(n: int, seed: int) -> np.ndarray:
    q = _orthogonal(n, np.random.default_rng(seed))
    q.setflags(write=False)
    return q


# ---- msm_eigh: A = Q diag(w) Q' ------------------------------------------------------------------------------------
def eigh_case(name: str, n: int, w, *, seed: int = 0, kind: str = "separated", exp2: int = 0, A=None,
              lopsided: bool = False, expect_sweeps: str | None = None) -> dict:
    """kind: "separated" (relative and absolute bounds) or "absolute" (graded / clustered: absolute bound only).
    exp2: the matrix and the truth are multiplied by 2**exp2 (exact).  A: an explicit matrix instead of the product.
    lopsided: the input handed to the solver is not symmetric (each off-diagonal pair holds 2 a_ij and 0), its
    symmetric part is A bit for bit.  expect_sweeps: "zero" (tridiagonal result accepted), "positive" (rejected)."""
    w = np.sort(np.asarray(w, np.float64))
    if A is None:
        q = _orthogonal_cached(n, 7000 + seed)
        A = np.dot(q * w.astype(LD)[None, :], q.T)
        A = np.asarray(0.5 * (A + A.T), np.float64)
    else:
        A = np.array(A, np.float64)
    A = np.ldexp(A, exp2)
    w = np.ldexp(w, exp2)
    a_in = A
    if lopsided:
        rng = np.random.default_rng(seed)
        upper = np.triu(np.ones((n, n), bool), 1)
        pick = upper & (rng.random((n, n)) < 0.5)
        keep = pick | (upper & ~pick).T    # per pair: the upper or the lower entry
        a_in = np.where(np.eye(n, dtype=bool), A, np.where(keep, 2.0 * A, 0.0))
        assert np.array_equal(0.5 * (a_in + a_in.T), A) and not np.array_equal(a_in, a_in.T)
    wmax = float(np.abs(w).max()) if n else 0.0
    lapack_err = float(np.abs(np.linalg.eigh(A)[0] - w).max())
    return {"name": name, "n": n, "w": w, "A": A, "A_in": np.ascontiguousarray(a_in), "kind": kind, "wmax": wmax,
            "lapack_err": lapack_err, "tol": max(n * EPS * wmax, 10.0 * lapack_err), "path": eigh_path(n),
            "expect_sweeps": expect_sweeps}


def check_eigh(w, v, case: dict, margin: float = 1.0) -> dict:
    """w ascending [n], v [n, n] or None.  Returns the measured figures."""
    n, truth, A, wmax = case["n"], case["w"], case["A"], case["wmax"]
    w = np.asarray(w, np.float64)
    assert w.shape == (n,) and np.all(np.isfinite(w))
    assert np.all(np.diff(w) >= 0), "eigenvalues not ascending"
    err = float(np.abs(w - truth).max())
    assert err <= margin * case["tol"], (case["name"], err, case["tol"])
    if case["kind"] == "separated":
        np.testing.assert_allclose(w, truth, rtol=1e-12, atol=1e-13 * wmax, err_msg=case["name"])
    fig = {"err": err}
    if v is not None:
        v = np.asarray(v, np.float64)
        assert v.shape == (n, n) and np.all(np.isfinite(v))
        orth = float(np.abs(v.T @ v - np.eye(n)).max())
        res = float(np.abs(A @ v - v * w[None, :]).max())
        assert orth <= 1e-12, (case["name"], orth)
        assert res <= 1e-11 * wmax, (case["name"], res, wmax)
        fig.update(orth=orth, res=res)
    return fig


def _separated(n, seed):
    """n distinct values in [-1, 2], neighbours at least 1 / (2 n) apart."""
    rng = np.random.default_rng(100 + seed)
    w = -1.0 + 3.0 * (np.arange(n) + rng.uniform(0.25, 0.75, n)) / max(n, 1)
    return w


def _with_cluster(n, seed, rel):
    """_separated with the three middle values replaced by c (1 + rel), c the middle one (about 0.5)."""
    w = _separated(n, seed)
    i = n // 2
    w[i - 1:i + 2] = w[i] * (1.0 + np.asarray(rel))
    return w


@functools.lru_cache(maxsize=None)
def eigh_cases() -> tuple:
    cs = []
    for n in (4, 6, 7, 9, 63, 66, 91, 92, 94, 95, 255, 256):
        cs.append(eigh_case(f"separated-{n}", n, _separated(n, n), seed=n,
                            expect_sweeps="zero" if n <= TRI_MAX else None))
    for n in (8, 33, 64, 100):
        cs.append(eigh_case(f"triple-{n}", n, _with_cluster(n, n, [0.0, 0.0, 0.0]), seed=n, kind="absolute",
                            expect_sweeps="positive" if n <= TRI_MAX else None))
    for n in (32, 64):
        for g in (1e-6, 1e-8, 1e-10):
            cs.append(eigh_case(f"cluster-{n}-{g:g}", n, _with_cluster(n, n + 1, [0.0, g, 2 * g]),
                                seed=n + 1, kind="absolute"))
    for n in (64, 128):
        cs.append(eigh_case(f"graded-{n}", n, np.logspace(0, -14, n), seed=n + 2, kind="absolute"))
    for n in (16, 100):
        for e in (200, -200):
            cs.append(eigh_case(f"scaled-{n}-2^{e}", n, _separated(n, n + 3), seed=n + 3, exp2=e))
    cs.append(eigh_case("zero-8", 8, np.zeros(8), A=np.zeros((8, 8)), kind="absolute"))
    cs.append(eigh_case("identity-8", 8, np.ones(8), A=np.eye(8), kind="absolute"))
    d = np.array([3.0, -1.0, 0.5, -2.0, 0.0, 7.0, -0.25])
    cs.append(eigh_case("diagonal-7", 7, d, A=np.diag(d)))
    cs.append(eigh_case("one-by-one", 1, [-2.5], A=[[-2.5]]))
    cs.append(eigh_case("two-by-two", 2, [2.0 - 0.75, 2.0 + 0.75], A=[[2.0, 0.75], [0.75, 2.0]]))
    cs.append(eigh_case("lopsided-12", 12, _separated(12, 12), seed=12, lopsided=True))
    cs.append(eigh_case("lopsided-70", 70, _separated(70, 70), seed=70, lopsided=True))
    return tuple(cs)


# ---- msm_tica_solve: the pencil C0t r = lambda C00 r with prescribed eigenvalues ---------------------------------
def spread_lambda(r: int) -> np.ndarray:
    """r eigenvalues over [-0.6, 0.97] whose magnitudes are 0.94 / r >= 1e-3 apart; every other one of those with
    |lambda| <= 0.6 is negative.  Returned by descending magnitude."""
    step = 0.94 / r
    mag = 0.97 - step * np.arange(r)
    neg = (mag <= 0.6) & (np.arange(r) % 2 == 1)
    return np.where(neg, -mag, mag)


def clustered_lambda(r: int) -> np.ndarray:
    """Three equal eigenvalues and one pair 1e-12 apart inside an otherwise spread spectrum."""
    lam = spread_lambda(r)
    lam[2:5] = lam[2]
    lam[7] = lam[6] - 1e-12 * np.sign(lam[6])
    order = np.argsort(-np.abs(lam), kind="stable")
    return lam[order]


@functools.lru_cache(maxsize=None)
def _tica_core(F: int, r: int, s2_key: tuple, lam_key: tuple, seed: int):
    """G (r x F, long double) with C00 = G' diag(sgn) G and C0t = G' diag(lam) G, both rounded to float64 once.
    G = Q S U' B': U, Q orthogonal r x r, S = sqrt|s2|, B the first r columns of an orthogonal F x F matrix (B = I
    at full rank).  Q leaves the last direction alone, so a last direction that is cut (or negative) decouples and
    the kept pencil has exactly the eigenvalues lam[:-1]."""
    s2 = np.asarray(s2_key, LD)
    lam = np.asarray(lam_key, LD)
    U = _orthogonal_cached(r, 9000 + seed)
    Q = np.eye(r, dtype=LD)
    if r > 1:
        Q[:r - 1, :r - 1] = _orthogonal_cached(r - 1, 9500 + seed)
    G = np.dot(Q * np.sqrt(np.abs(s2))[None, :], U.T)
    if r < F:
        G = np.dot(G, _orthogonal_cached(F, 9900 + seed)[:, :r].T)
    sgn = np.sign(s2)
    C00 = np.dot(G.T * sgn[None, :], G)
    C0t = np.dot(G.T * lam[None, :], G)
    C00 = 0.5 * (C00 + C00.T)
    C0t = 0.5 * (C0t + C0t.T)
    for a in (G, C00, C0t):
        a.setflags(write=False)
    return G, C00, C0t


def tica_case(name: str, F: int, *, rank: int | None = None, lam=None, cond: float = 1e2, s2=None, seed: int = 0,
              mean: bool = False, scale: bool = False, kinetic_map: bool = True, epsilon: float = 1e-6,
              T: float = 0.5, clustered: bool = False) -> dict:
    """One input of msm_tica_solve and what it must return.

    rank: C00 = B C00^ B' of that rank (None: full).  lam: the pencil's eigenvalues (default spread_lambda).  cond:
    cond(C00) on its range, eigenvalues logspace(0, -log10 cond); s2: the eigenvalues of C00 themselves instead --
    the LAST one may be below epsilon or negative (indefinite C00), it decouples from the rest.  mean: |mu_i| <=
    3 sqrt(C00_ii); scale: a per-feature divisor folded into the moments.  T: the pair count written into the
    moments, which are always encoded for T = 0.5 (w = 1); T <= 0 must give rank 0 and zeros."""
    r = F if rank is None else int(rank)
    if s2 is None:
        s2 = np.logspace(0.0, -np.log10(cond), r) if r > 1 else np.ones(1)
    s2 = np.asarray(s2, np.float64)
    lam = (clustered_lambda(r) if clustered else spread_lambda(r)) if lam is None else np.asarray(lam, np.float64)
    G, C00, C0t = _tica_core(F, r, tuple(s2.tolist()), tuple(lam.tolist()), seed)
    # deeptime's cut, restated: epsilon, raised to -min + 1e-16 when C00 has a negative eigenvalue
    eps_eff = max(epsilon, -float(s2.min()) + 1e-16) if s2.min() < 0 else epsilon
    kept = np.abs(s2) >= eps_eff
    assert kept[:-1].all() or r == 1, "only the last direction may be cut"
    rng = np.random.default_rng(31 * seed + F)
    d00 = np.abs(np.diag(C00)).astype(np.float64)
    mu = (rng.uniform(-3.0, 3.0, F) * np.sqrt(d00)) if mean else np.zeros(F)
    sc = rng.uniform(0.25, 4.0, F) if scale else None
    D = np.ones(F, LD) if sc is None else sc.astype(LD)
    mm = np.outer(mu.astype(LD), mu.astype(LD))
    M00 = (C00 + mm) * np.outer(D, D)
    M0t = (C0t + mm) * np.outer(D, D) / 2
    sxy = mu.astype(LD) * D / 2
    moments = np.concatenate([np.asarray(M00, np.float64).ravel(), np.asarray(M0t, np.float64).ravel(),
                              np.asarray(sxy, np.float64), np.asarray(sxy, np.float64), [float(T)]])
    truth = lam[kept]
    truth = truth[np.argsort(-np.abs(truth), kind="stable")]
    k_rank = int(kept.sum())
    cond_kept = float(np.abs(s2).max() / np.abs(s2[kept]).min()) if k_rank else 1.0
    kappa = cond_kept * (1.0 + float(np.max(mu * mu / d00))) if k_rank else 1.0
    tol = max(F * EPS * kappa, 1e-11)
    # gap of every kept eigenvalue to its neighbours in magnitude (the order the solver sorts by)
    mag = np.abs(truth)
    gap = np.full(k_rank, np.inf)
    if k_rank > 1:
        dm = -np.diff(mag)
        gap[:-1] = np.minimum(gap[:-1], dm)
        gap[1:] = np.minimum(gap[1:], dm)
    # groups of eigenvalues closer than 1e-9: compared as invariant subspaces
    groups, start = [], 0
    for j in range(1, k_rank + 1):
        if j == k_rank or mag[j - 1] - mag[j] > 1e-9:
            groups.append((start, j))
            start = j
    for a, b in groups:     # the gap that matters for a group is the one to its outside neighbours
        outer = min(mag[a - 1] - mag[a] if a > 0 else np.inf, mag[b - 1] - mag[b] if b < k_rank else np.inf)
        gap[a:b] = outer
    zero = not T > 0 or k_rank == 0
    return {"name": name, "F": F, "rank": 0 if zero else k_rank, "moments": moments, "scale": sc, "mu": mu,
            "epsilon": epsilon, "kinetic_map": bool(kinetic_map), "T": float(T), "lam": truth, "tol": tol,
            "kappa": kappa, "gap": gap, "groups": groups, "clustered": bool(clustered) or any(b - a > 1 for a, b in groups),
            "G": np.asarray(G[kept], np.float64), "sgn": np.sign(s2[kept]), "C00": np.asarray(C00, np.float64),
            "C0t": np.asarray(C0t, np.float64), "zero": zero,
            "rnorm": float(1.0 / np.sqrt(np.abs(s2[kept]).min())) if k_rank else 1.0, "path": tica_path(F, None if k_rank == F else k_rank)}


def moments_dict(case: dict, T=None) -> dict:
    F, v = case["F"], case["moments"]
    return {"Mxx": v[:F * F].reshape(F, F), "Mxy_half": v[F * F:2 * F * F].reshape(F, F),
            "sx": v[2 * F * F:2 * F * F + F], "sy": v[2 * F * F + F:2 * F * F + 2 * F],
            "T": v[2 * F * F + 2 * F] if T is None else T}


def numpy_tica(case: dict) -> dict:
    """npport.tica_from_moments on the case, in the layout of the device outputs (the second, independent
    reference; cached in the case)."""
    if "ref" not in case:
        F = case["F"]
        model = npport.tica_from_moments(moments_dict(case, T=0.5), epsilon=case["epsilon"],
                                         scaling="kinetic_map" if case["kinetic_map"] else None, scale=case["scale"])
        r = model["rank"]
        eig, W = np.zeros(F), np.zeros((F, F))
        eig[:r] = model["eigenvalues"]
        W[:, :r] = model["coefficients"]
        case["ref"] = {"eig": eig, "W": W, "mean": model["mean"], "rank": r}
    return case["ref"]


def whitened_matrix(case: dict) -> np.ndarray:
    """L' C0t L of the case, L = spd_inv_split(C00) as npport.tica_from_moments forms it (rank x rank)."""
    s, V = np.linalg.eigh(case["C00"])
    order = np.argsort(np.abs(s))[::-1]
    s, V = s[order][:case["rank"]], V[:, order][:, :case["rank"]]
    L = V / np.sqrt(s)[None, :]
    Ct = L.T @ case["C0t"] @ L
    return 0.5 * (Ct + Ct.T)


def check_tica(out, case: dict, margin: float = 1.0) -> dict:
    """out = (eig [F], W [F, F], mean [F], rank) as numpy arrays / int.  `margin` scales the eigenvalue bound (the
    CPU test holds numpy to a tenth of it).  Returns the measured figures."""
    eig, W, mean, rank = out
    eig, W, mean, rank = np.asarray(eig, np.float64), np.asarray(W, np.float64), np.asarray(mean, np.float64), int(rank)
    F, r, tol, km = case["F"], case["rank"], case["tol"], case["kinetic_map"]
    name = case["name"]
    assert eig.shape == (F,) and W.shape == (F, F) and mean.shape == (F,)
    assert rank == r, (name, "rank", rank, r)
    assert np.all(eig[r:] == 0.0) and np.all(W[:, r:] == 0.0), (name, "columns past the rank are not exactly zero")
    if case["zero"]:
        assert np.all(eig == 0.0) and np.all(W == 0.0)
        assert np.all(mean == (case["mu"] if case["T"] > 0 else 0.0)), (name, "mean")
        return {"err": 0.0}
    assert np.all(np.isfinite(eig)) and np.all(np.isfinite(W))
    mu = case["mu"]
    assert np.all(np.abs(mean - mu) <= 8 * EPS * np.maximum(np.abs(mu), 1e-300) + 0.0), (name, "mean")
    lam = case["lam"]
    got = eig[:r]
    if case["clustered"]:
        err = float(np.abs(np.sort(got) - np.sort(lam)).max())
        assert np.all(np.diff(np.abs(got)) <= tol), (name, "not sorted by magnitude")
    else:
        err = float(np.abs(got - lam).max())
    assert err <= margin * tol, (name, "eigenvalues", err, tol)
    # invariants in the whitened coordinates: C00 = G' sgn G and C0t = G' lam0 G exactly (before the one rounding),
    # so W' C00 W = Y' sgn Y and W' C0t W = Y' lam0 Y with Y = G W; the exact answer is Y = signed diagonal (times
    # lambda with the kinetic map), rotated inside a cluster only
    Wr = W[:, :r]
    Y = case["G"] @ Wr
    p = lam ** 2 if km else np.ones(r)
    i00 = float(np.abs(Wr.T @ case["C00"] @ Wr - np.diag(p)).max())
    i0t = float(np.abs(Wr.T @ case["C0t"] @ Wr - np.diag(p * lam)).max())
    y00 = float(np.abs((Y.T * case["sgn"][None, :]) @ Y - np.diag(p)).max())
    # the float64 products above lose F eps |W|' |C| |W| themselves, which the whitened form does not
    slack = F * EPS * float((np.abs(Wr).T @ np.abs(case["C00"]) @ np.abs(Wr)).max())
    assert y00 <= tol, (name, "W' C00 W (whitened form)", y00, tol)
    assert i00 <= tol + slack, (name, "W' C00 W", i00, tol, slack)
    assert i0t <= tol + slack, (name, "W' C0t W", i0t, tol, slack)
    # sign rule: the largest-magnitude entry of a column is positive before the kinetic scaling
    top = Wr[np.argmax(np.abs(Wr), axis=0), np.arange(r)]
    want_sign = np.sign(got) if km else np.ones(r)
    assert np.all(np.sign(top) == want_sign), (name, "sign rule", np.nonzero(np.sign(top) != want_sign)[0])
    # columns against the numpy port up to sign, and against the construction (Y = signed diagonal); inside a
    # cluster the invariant subspace (W_g W_g') instead of single columns
    # A whitened perturbation E (|E|_2 <= tol, what the eigenvalue bound allows) turns a column of Y by at most
    # |E|_2 / gap (Davis-Kahan), and W = R Y with |R|_2 = rnorm.  The port's own error is held to a tenth of the
    # bound by the CPU test, hence 1.1 when the two are compared with each other.
    ref = numpy_tica(case)
    assert ref["rank"] == r
    Wn = ref["W"][:, :r]
    rn = case["rnorm"]
    worst = 0.0
    for a, b in case["groups"]:
        bound = tol / min(case["gap"][a], 1.0)
        if b - a == 1:
            s = np.sign(np.dot(Wr[:, a], Wn[:, a])) or 1.0
            dn = float(np.linalg.norm(s * Wr[:, a] - Wn[:, a])) / rn
            off = Y[:, a].copy()
            off[a] = abs(off[a]) - (abs(lam[a]) if km else 1.0)
            dy = float(np.linalg.norm(off))
        else:
            dn = float(np.linalg.norm(Wr[:, a:b] @ Wr[:, a:b].T - Wn[:, a:b] @ Wn[:, a:b].T, 2)) / rn ** 2
            Yo = Y[:, a:b].copy()
            Yo[a:b] = 0.0
            dy = float(np.linalg.norm(Yo, 2))
        assert dy <= bound, (name, "columns against the construction", (a, b), dy, bound)
        assert dn <= 1.1 * bound, (name, "columns against the numpy port", (a, b), dn, bound)
        worst = max(worst, dy / bound, dn / bound)
    return {"err": err, "w00": y00, "w0t": i0t, "cols": worst}


def _variants(base_name, F, **kw):
    """The three input variants (plain, scaled, with a mean) x kinetic map on / off."""
    out = []
    for km in (True, False):
        for vname, vkw in (("plain", {}), ("scale", {"scale": True}), ("mean", {"mean": True})):
            out.append(tica_case(f"{base_name}-{vname}-{'km' if km else 'raw'}", F, kinetic_map=km, **vkw, **kw))
    return out


FULL_RANK_F = (1, 2, 3, 7, 8, 16, 17, 33, 63, 64, 65, 66, 69, 70, 71, 97, 98, 128, 255, 256)
COND4_F = (64, 69, 97, 256)
DEFICIENT = ((5, 1), (8, 5), (9, 6), (63, 50), (64, 60), (65, 64), (65, 40), (66, 64), (69, 33), (80, 70), (100, 37),
             (256, 200))
CLUSTERED = ((16, None), (64, None), (65, 64))


@functools.lru_cache(maxsize=None)
def tica_full_rank_cases(F: int) -> tuple:
    cs = _variants(f"full-{F}", F, seed=F)
    if F in COND4_F:
        cs += _variants(f"full-{F}-cond1e4", F, seed=F, cond=1e4, epsilon=1e-12)
    return tuple(cs)


@functools.lru_cache(maxsize=None)
def tica_deficient_cases() -> tuple:
    return tuple(tica_case(f"rank-{F}-{r}-{'km' if km else 'raw'}", F, rank=r, seed=F + r, kinetic_map=km,
                           mean=km, scale=not km)
                 for F, r in DEFICIENT for km in (True, False))


def _cut_s2(F, small):
    return np.concatenate([np.logspace(0.0, -2.0, F - 1), [small]])


@functools.lru_cache(maxsize=None)
def tica_cut_cases() -> tuple:
    """The smallest C00 eigenvalue just above (kept, full rank) and just below (cut) epsilon = 1e-6, away from the
    fused path."""
    return tuple(tica_case(f"cut-{F}-{small:g}", F, s2=_cut_s2(F, small), seed=F + 1)
                 for F in (70, 100) for small in (1.5e-6, 0.6e-6))


@functools.lru_cache(maxsize=None)
def tica_clustered_cases() -> tuple:
    return tuple(tica_case(f"clustered-{F}-{r or F}", F, rank=r, seed=F + 2, clustered=True) for F, r in CLUSTERED)


@functools.lru_cache(maxsize=None)
def tica_indefinite_cases() -> tuple:
    return tuple(tica_case(f"indefinite-{F}", F, s2=_cut_s2(F, -1e-3), seed=F + 3) for F in (6, 70))


@functools.lru_cache(maxsize=None)
def tica_zero_cases() -> tuple:
    """All-zero moments with T > 0 (rank 0, zeros: the numpy port raises there) and T = 0 on real moments."""
    cs = []
    for F in (6, 70):
        z = tica_case(f"zero-moments-{F}", F, seed=F)
        z = dict(z, moments=np.concatenate([np.zeros(2 * F * F + 2 * F), [0.5]]), rank=0, zero=True, mu=np.zeros(F))
        cs.append(z)
        cs.append(tica_case(f"T-zero-{F}", F, seed=F, mean=True, T=0.0))
    cs.append(tica_case("T-negative-6", 6, seed=6, T=-3.0))
    return tuple(cs)


def all_tica_cases() -> list:
    cs = [c for F in FULL_RANK_F for c in tica_full_rank_cases(F)]
    cs += tica_deficient_cases() + tica_cut_cases() + tica_clustered_cases() + tica_indefinite_cases()
    return cs + list(tica_zero_cases())


# ---- msm_onesided_tica_eigenvalues ---------------------------------------------------------------------------------
ONESIDED_F = (1, 2, 63, 64, 65, 66, 67, 128, 256)
ONESIDED_LAG = 5


@functools.lru_cache(maxsize=None)
def onesided_case(F: int, constant_column: int | None = None) -> dict:
    n = max(2000, 8 * F)
    X = _gen.correlated_series(n, F, 4000 + F).astype(np.float64)
    if constant_column is not None:
        X[:, constant_column] = 3.0    # an exact zero row and column of C0 and Ct: the clip branch
    idx = np.arange(n - ONESIDED_LAG)
    want = npport.estimate_top_eigenvalues(X, idx, idx + ONESIDED_LAG, F)
    big = F >= 64
    return {"name": f"onesided-{F}" + ("" if constant_column is None else "-const"), "F": F, "X": X, "idx": idx,
            "lag": ONESIDED_LAG, "want": want, "rtol": 1e-8 if big else 1e-9, "atol": 1e-11 if big else 1e-12,
            "path": onesided_path(F)}


def check_onesided(ev, case: dict) -> dict:
    ev = np.asarray(ev, np.float64)
    assert ev.shape == case["want"].shape and np.all(np.isfinite(ev))
    np.testing.assert_allclose(ev, case["want"], rtol=case["rtol"], atol=case["atol"], err_msg=case["name"])
    return {"err": float(np.abs(ev - case["want"]).max())}
