"""Dispatch rule, block schedule and inputs for the device-wide eigensolver of pmarlo_amd/csrc/eig_large.h (TEST
INFRASTRUCTURE).

msm_eigh, msm_tica_solve and msm_onesided_tica_eigenvalues run the one-workgroup code of eig.hip up to order 256 and
the block Jacobi of eig_large.h from 257 to 2048.  `dispatch`, `layout` and `block_schedule` restate that rule and the
tournament over block pairs; `block_jacobi` restates the method itself in numpy (pivot problems by LAPACK), so the
schedule, the exact treatment of the pivot blocks and the padding can be checked without a device.  The inputs come
from the builders of tests/_eig_ref.py, whose bounds are used unchanged; the `path` field those builders attach
describes the dispatch below 257 and means nothing here.  Nothing in this file is imported by the product."""

from __future__ import annotations

import functools

import numpy as np

from tests import _eig_ref as er

EPS = er.EPS
B = 32                      # block width (kBjB)
PIVOT = 2 * B               # order of a pivot problem
SMALL_MAX = 256             # up to here: the one-workgroup solvers
MAX_ORDER = 2048            # kBjMaxOrder
SWEEP_CAP = er.JACOBI_MAX_SWEEPS


def dispatch(n: int) -> str:
    if n < 1:
        return "invalid"
    return "one_workgroup" if n <= SMALL_MAX else ("block_jacobi" if n <= MAX_ORDER else "unsupported")


def layout(n: int) -> dict:
    """Sizes the launcher derives from the order: blocks, padded order, workgroups of the pivot launch (pairs, the
    bye of an odd block count included), rounds per sweep, launches per sweep (two for the convergence test, three
    per round) and the dynamic LDS of the pivot kernel (three 64 x 65 fp64 matrices)."""
    nb = -(-n // B)
    nbp = nb + (nb & 1)
    return {"nb": nb, "npad": nb * B, "pairs": nbp // 2, "rounds": nbp - 1, "launches_per_sweep": 2 + 3 * (nbp - 1),
            "pivot_lds_bytes": 3 * PIVOT * (PIVOT + 1) * 8}


def scratch_bytes(n: int, nmats: int) -> int:
    """bj_scratch_bytes: nmats padded matrices (2 for msm_eigh, 5 for the TICA and one-sided solves), Q and the new
    diagonal of every pair, the partial sums of the convergence test, two eigenvalue and two order arrays, control
    words."""
    L = layout(n)
    npad, m, nb = L["npad"], L["pairs"], L["nb"]
    return (nmats * npad * npad + m * PIVOT * PIVOT + m * PIVOT + 2 * nb + 2 * npad) * 8 + (2 * npad + 8) * 4 + 64


def pivot_pair(rnd: int, i: int, npad: int) -> tuple:
    """eig.hip's pivot_pair (on block indices here); npad even, index npad - 1 never moves."""
    if i == 0:
        return rnd, npad - 1
    ring = npad - 1
    return (rnd + i) % ring, (rnd - i) % ring


def block_schedule(n: int) -> list:
    """One sweep: a list of rounds, each a list of block pairs (p, q) in workgroup order.  A pair with the padding
    player of an odd block count is a bye and is left out."""
    L = layout(n)
    nb, nbp = L["nb"], L["nb"] + (L["nb"] & 1)
    return [[pq for pq in (pivot_pair(r, i, nbp) for i in range(nbp // 2)) if pq[1] < nb] for r in range(nbp - 1)]


def _near_identity(d: np.ndarray, Q: np.ndarray):
    """Columns of Q (and d with them) permuted so that the large entries sit on the diagonal (greedy).  A Jacobi
    solve of a nearly diagonal pivot problem yields a Q near the identity, which is what lets the block iteration
    converge; LAPACK sorts by eigenvalue and so shuffles indices between the two blocks of a pair."""
    k = len(d)
    W = np.abs(Q).copy()
    perm = np.zeros(k, int)
    for _ in range(k):
        i, j = np.unravel_index(np.argmax(W), W.shape)
        perm[i] = j
        W[i, :] = -1.0
        W[:, j] = -1.0
    return d[perm], Q[:, perm]


def block_jacobi(A: np.ndarray, active: int | None = None):
    """The method of eig_large.h in numpy: zero-padded matrix, the schedule above, per pair Q from the 64 x 64 pivot
    problem (LAPACK here, jacobi_eigh on the device), A <- Q'AQ with the pivot blocks written as diag + exact zeros,
    V <- VQ; jacobi_converged's test ahead of every sweep.  -> (w ascending, V columns, sweeps)."""
    n = A.shape[0]
    L = layout(n)
    npad = L["npad"]
    active = n if active is None else active
    M = np.zeros((npad, npad))
    M[:n, :n] = 0.5 * (A + A.T)
    V = np.eye(npad)
    sched = block_schedule(n)
    sweeps = 0
    for _ in range(SWEEP_CAP):
        sq = M[:n, :n] ** 2
        dia = float(np.trace(sq))
        off = float((sq - np.diag(np.diag(sq))).sum())     # exactly 0 for a diagonal matrix
        tol = active * EPS
        if off <= tol * tol * (dia + off) or off == 0.0:
            break
        sweeps += 1
        for rnd in sched:
            for p, q in rnd:
                if min(p, q) * B >= active:
                    continue
                idx = np.r_[p * B:(p + 1) * B, q * B:(q + 1) * B]
                S = M[np.ix_(idx, idx)]
                S = np.triu(S) + np.triu(S, 1).T
                # padded indices: jacobi_rotation skips their (zero) pivots, so Q is the identity there and the
                # padding keeps its place; LAPACK would sort its zero eigenvalues in among the others
                real = idx < n
                d, Q = np.zeros(PIVOT), np.eye(PIVOT)
                d[real], Q[np.ix_(real, real)] = _near_identity(*np.linalg.eigh(S[np.ix_(real, real)]))
                M[:, idx] = M[:, idx] @ Q
                M[idx, :] = Q.T @ M[idx, :]
                M[np.ix_(idx, idx)] = np.diag(d)
                V[:, idx] = V[:, idx] @ Q
    w = np.diag(M)[:n]
    order = np.argsort(w, kind="stable")
    return w[order], V[:n, :n][:, order], sweeps


# ---- msm_eigh -------------------------------------------------------------------------------------------------------
SEPARATED_N = (257, 258, 287, 288, 289, 320, 512)
N300 = 300


def separated_case(n: int) -> dict:
    return er.eigh_case(f"separated-{n}", n, er._separated(n, n), seed=n)


def _block_diagonal(n: int, seed: int):
    """Blocks of width B on the diagonal (the last one ragged), each Q_b diag(w_b) Q_b' in long double: every rotation
    between two blocks is skipped.  -> (A, w)."""
    w = er._separated(n, seed)
    rng = np.random.default_rng(seed)
    w = w[rng.permutation(n)]
    A = np.zeros((n, n), er.LD)
    for b0 in range(0, n, B):
        k = min(B, n - b0)
        q = er._orthogonal_cached(k, 7700 + seed + b0)
        A[b0:b0 + k, b0:b0 + k] = np.dot(q * w[b0:b0 + k].astype(er.LD)[None, :], q.T)
    return np.asarray(0.5 * (A + A.T), np.float64), w


@functools.lru_cache(maxsize=None)
def n300_cases() -> tuple:
    """The shapes of er.eigh_cases() that stress a Jacobi solver, at one ragged order above the old cap.  All share
    one orthogonal factor (seed), so the long-double product is formed once per spectrum."""
    n, s = N300, N300
    cs = [er.eigh_case("triple-300", n, er._with_cluster(n, s, [0.0, 0.0, 0.0]), seed=s, kind="absolute"),
          er.eigh_case("cluster-300-1e-10", n, er._with_cluster(n, s + 1, [0.0, 1e-10, 2e-10]), seed=s, kind="absolute"),
          er.eigh_case("graded-300", n, np.logspace(0, -14, n), seed=s, kind="absolute"),
          er.eigh_case("scaled-300-2^200", n, er._separated(n, s + 3), seed=s, exp2=200),
          er.eigh_case("scaled-300-2^-200", n, er._separated(n, s + 3), seed=s, exp2=-200),
          er.eigh_case("lopsided-300", n, er._separated(n, s + 4), seed=s, lopsided=True),
          er.eigh_case("zero-300", n, np.zeros(n), A=np.zeros((n, n)), kind="absolute"),
          er.eigh_case("identity-300", n, np.ones(n), A=np.eye(n), kind="absolute")]
    d = er._separated(n, s + 5)[np.random.default_rng(s).permutation(n)]
    d[7] = 0.0    # a real eigenvalue 0: padding is dropped by index, never by value
    cs.append(er.eigh_case("diagonal-300", n, d, A=np.diag(d)))
    Ab, wb = _block_diagonal(n, s + 6)
    cs.append(er.eigh_case("blockdiag-300", n, wb, A=Ab))
    return tuple(cs)


CAP_REFLECTORS = 3


@functools.lru_cache(maxsize=None)
def cap_case() -> dict:
    """n = 2048 in float64: A = H3 H2 H1 D H1 H2 H3 with Householder reflectors H = I - 2 v v' / v'v and D a known
    diagonal, O(n^2) work.  The same updates are repeated in long double; E = A - A_longdouble is the construction's
    own rounding and moves no eigenvalue by more than ||E||_F (Weyl), so the bound is n eps |w|_inf + ||E||_F.
    check_eigh's absolute branch applies it together with the orthogonality and residual invariants."""
    n = MAX_ORDER
    rng = np.random.default_rng(2048)
    w = er._separated(n, 2048)
    d = w[rng.permutation(n)]
    A, Al = np.diag(d), np.diag(d.astype(er.LD))
    for _ in range(CAP_REFLECTORS):
        v = rng.normal(size=n)
        for M, vv in ((A, v), (Al, v.astype(er.LD))):
            beta = 2 / np.dot(vv, vv)
            M -= beta * np.outer(vv, np.dot(vv, M))
            M -= beta * np.outer(np.dot(M, vv), vv)
    A = 0.5 * (A + A.T)
    Al = 0.5 * (Al + Al.T)
    construction = float(np.sqrt(np.sum((A.astype(er.LD) - Al) ** 2)))
    w = np.sort(w)
    wmax = float(np.abs(w).max())
    return {"name": "cap-2048", "n": n, "w": w, "A": A, "A_in": np.ascontiguousarray(A), "kind": "absolute",
            "wmax": wmax, "construction": construction, "tol": n * EPS * wmax + construction, "expect_sweeps": None}


# ---- msm_tica_solve -------------------------------------------------------------------------------------------------
FULL_F = (257, 320, 384)
DEFICIENT = ((320, 200), (300, 256))


@functools.lru_cache(maxsize=None)
def tica_full_case(F: int) -> dict:
    return er.tica_case(f"full-{F}", F, seed=F, mean=True, scale=True)


@functools.lru_cache(maxsize=None)
def tica_deficient_case(F: int, r: int) -> dict:
    return er.tica_case(f"rank-{F}-{r}", F, rank=r, seed=F + r, mean=True)


@functools.lru_cache(maxsize=None)
def tica_300_cases() -> dict:
    F = N300
    return {"cut": er.tica_case("cut-300", F, s2=er._cut_s2(F, 0.6e-6), seed=F + 1),
            "indefinite": er.tica_case("indefinite-300", F, s2=er._cut_s2(F, -1e-3), seed=F + 1),
            "raw": er.tica_case("full-300-raw", F, seed=F + 1, kinetic_map=False),
            "T-zero": er.tica_case("T-zero-300", F, seed=F + 1, mean=True, T=0.0)}


ONESIDED_F = (257, 320)
