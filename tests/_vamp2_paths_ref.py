"""The cases of the launch-path tests of the VAMP-2 loss kernels (csrc/mlp_train.hip: column sums, fp64 MFMA moments,
the one-workgroup solve, the output gradients; plain and weighted), and a second route through their law.

The law stays tests/_deeptica_train_ref.vamp2 and tests/_deeptica_weighted_ref.vamp2_weighted; nothing here changes
what they return.  `second_route` computes the same quantities another way: weights, means, centred outputs and the
three moment matrices in np.longdouble; each side's regularised matrix rounded once to fp64 and taken apart by
np.linalg.eigh (by a longdouble cyclic Jacobi where CASES asks for it: eigh's small eigenvalues carry eps * l_max, too
coarse for a graded matrix); the jitter ladder climbed while the smallest eigenvalue of A + total I is not above
d * eps * l_max, no Cholesky anywhere; A^-1 = V diag(1 / (w + total)) V', score = tr(A^-1 C0t B^-1 C0t'), and the
gradients from the closed forms of include/msmhip.h, all in longdouble.

Inputs: `outputs(m, d, salt)` is T.loss_case's recipe at any shape, seeded by crc32 of "vamp2:m:d" + salt as
tests/_mlp_paths_ref seeds its draws.  A salt is the first of "", ":1", ":2", ... at which the case passes the
conditions of tests/test_vamp2_paths_reference.py (cond <= 64, eigenvector sensitivity eps l_max / gap <= 1e-12 for
both extreme eigenvalues of both sides, plain and under the case's weights); SALT lists the shapes that needed one.
Special inputs (constant outputs, one constant output, graded column scales) are built from those.

CASES is the one table both test files read.  A case is a dict:
    m, d, salt     the shape and the seed salt
    inputs         "recipe", "constant" (every output a power of two), "one_constant" (output d // 2 is 0.5),
                   "graded" (column scales 1e-4 .. 1)
    opts           eps, eps_abs, alpha, cond_reg as the device gets them (unclamped)
    weights        the weight pattern of the weighted run ("mild": uniform in [0.5, 1.5); the patterns of
                   tests/_deeptica_weighted_ref.weights; "first", "last": all weight on one pair; "pow2": powers of
                   two, so that weighted sums of powers of two stay exact); every case also runs unweighted unless
                   `only` says otherwise
    compare        "all", or "loss": loss, score, penalty and metrics only (the penalty has no direction, or there is
                   no gradient to speak of)
    group          the group its distances are reported under
    bound          the largest admitted device-to-law distance: 1e-10, the project's yardstick, wherever the two routes
                   agree within 1e-12; otherwise 100 x `route`, the measured route disagreement written beside it.
                   In those cases the law is the coarser side (LAPACK's eigh and inverse lose eps l_max in a small
                   eigenvalue), so the device is also held to 1e-10 of the second route, whose Jacobi is longdouble:
                   the matrices are graded, a Jacobi method finds the eigenvalues of a positive definite matrix to
                   eps d cond(D A D) with D A D its scaling to a unit diagonal (Demmel and Veselic), and the host test
                   asserts cond(D A D) <= 4e3 (measured: 1.6e3 at most), which leaves 64 * 2.2e-16 * 4e3 = 5.7e-11
    expect         for branch cases: per side the ladder's final `total`, `clamped`, and the penalty halves present;
                   `zero`: the covariances vanish and `assert_zero_case` takes the place of the distances
    only           "weighted" for the cases that have no plain run
    jacobi         the second route takes its eigenpairs from the longdouble Jacobi

Measured on the host (tests/test_vamp2_paths_reference.py prints them): see the figures in DESIGN.md, "VAMP-2 loss
and AdamW launch paths"."""

from __future__ import annotations

import zlib

import numpy as np

from tests import _deeptica_train_ref as T
from tests import _deeptica_weighted_ref as WR

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
CHUNK = 256                                  # MSM_MLP_CHUNK: pairs per partial sum
TILE = 16                                    # the MFMA tile of the moments kernels
LDS_SWITCH = 48 * 1024                       # the solve asks for 2 d^2 8 bytes of LDS; above this it must opt in
ROUTE, YARDSTICK = 1e-12, 1e-10
COND_ORDINARY = 64.0
COND_SCALED = 4e3                            # of D A D, for the cases with a bound of their own (see `bound`)
SENSITIVITY = 1e-12
FLOOR = T.FLOOR
LADDER = (0.0, 1e-8, 1.1e-7, 1.11e-6, 1.111e-5)

WIDTHS = (1, 2, 15, 16, 17, 32, 33, 48, 49, 55, 56, 63, 64)        # at m = 257
ROWS = (1, 2, 255, 256, 257, 512, 513, 770)                        # at d in ROW_WIDTHS
ROW_WIDTHS = (1, 17, 64)
PATTERN_SHAPES = [(m, d) for m in (257, 770) for d in (16, 56, 64)]
BRANCH_WIDTHS = (5, 64)

# a case whose covariances vanish: the trace clamp, no penalty direction, and zeros where `assert_zero_case` looks
ZERO = {"total": 0.0, "clamped": True, "halves": (False, False), "zero": True}

# (m, d) -> salt: the first of "", ":1", ... at which every run of the shape passes the input conditions
SALT = {(255, 64): ":3", (256, 64): ":5", (257, 48): ":2", (257, 55): ":4", (257, 56): ":1", (257, 63): ":7", (257, 64): ":6",
        (513, 64): ":8", (770, 56): ":111", (770, 64): ":33"}


# ---- inputs ----------------------------------------------------------------------------------------------------------
def outputs(m: int, d: int, salt: str = ""):
    """(Y0, Yt) by T.loss_case's recipe: correlated, off-centre, columns of unequal scale."""
    rng = np.random.default_rng(zlib.crc32(f"vamp2:{m}:{d}{salt}".encode()))
    base = rng.normal(size=(m, d))
    mix = rng.normal(size=(d, d)) / np.sqrt(d) + np.eye(d)
    scale = rng.uniform(0.3, 3.0, size=d)
    Y0 = (base @ mix) * scale + rng.normal(size=d)
    Yt = (0.7 * base + 0.5 * rng.normal(size=(m, d))) @ mix * scale + rng.normal(size=d)
    return Y0, Yt


def weights_of(c: dict) -> np.ndarray:
    m, pattern = c["m"], c["weights"]
    tag = f"vamp2:{m}:{c['d']}"
    if pattern == "mild":
        return 0.5 + np.random.default_rng(zlib.crc32(("weights:" + tag).encode())).uniform(size=m)
    if pattern == "pow2":                    # 64 each of 0.5, 1, 2, 4 and one 32: W = 512, so w / W is exact too
        w = 2.0 ** (np.arange(m) % 4 - 1)
        w[m - 1] = 32.0 if m == 257 else w[m - 1]
        return w
    if pattern in ("first", "last"):
        w = np.zeros(m)
        w[0 if pattern == "first" else m - 1] = 2.0
        return w
    if pattern == "chunk0":                  # the first chunk carries nothing
        w = WR.weights(tag, m, "lognormal")
        w[:CHUNK] = 0.0
        return w
    return WR.weights(tag, m, pattern)


_INPUTS: dict = {}


def inputs(name: str):
    """(Y0, Yt, weights) of a case; made once, read only."""
    if name not in _INPUTS:
        c = CASES[name]
        m, d = c["m"], c["d"]
        Y0, Yt = outputs(m, d, c["salt"])
        if c["inputs"] == "constant":
            Y0, Yt = np.empty((m, d)), np.empty((m, d))
            Y0[:], Yt[:] = 2.0 ** (np.arange(d) % 9 - 4), -(2.0 ** (np.arange(d) % 7 - 2))
        elif c["inputs"] == "one_constant":
            Y0[:, d // 2], Yt[:, d // 2] = 0.5, 0.5
        elif c["inputs"] == "graded":
            grade = 10.0 ** np.linspace(-4.0, 0.0, d)
            Y0, Yt = Y0 * grade, Yt * grade
        w = weights_of(c)
        for a in (Y0, Yt, w):
            a.setflags(write=False)
        _INPUTS[name] = (Y0, Yt, w)
    return _INPUTS[name]


# ---- the case table --------------------------------------------------------------------------------------------------
def _case(m, d, *, inputs="recipe", opts=None, weights="mild", compare="all", group="widths", bound=YARDSTICK,
          route=None, expect=None, only=None, jacobi=False):
    o = {"eps": 1e-3, "eps_abs": 1e-6, "alpha": 0.3, "cond_reg": 0.05 if d % 2 else 1e-4}
    o.update(opts or {})
    if m < d + 2 and inputs == "recipe":     # fewer pairs than outputs: the smallest eigenvalue is tied
        o["cond_reg"] = 0.0
    return {"m": m, "d": d, "salt": SALT.get((m, d), ""), "inputs": inputs, "opts": o, "weights": weights,
            "compare": compare, "group": group, "bound": bound, "route": route, "expect": expect, "only": only,
            "jacobi": jacobi}


def _table() -> dict:
    t = {}
    for d in WIDTHS:
        t[f"w{d}"] = _case(257, d)
    for d in ROW_WIDTHS:
        for m in ROWS:
            if m == 257:
                continue                     # the width sweep has it
            if m == 1:                       # one pair: the trace clamp
                t[f"r{m}x{d}"] = _case(m, d, group="rows", weights="pow2",
                                       expect=dict(ZERO))
            else:
                t[f"r{m}x{d}"] = _case(m, d, group="rows")
    for m, d in PATTERN_SHAPES:
        for pattern in WR.PATTERNS + (("chunk0",) if m > 2 * CHUNK else ()):
            # log-normal weights leave about m / 9.5 effective pairs: at m = 257 fewer than 56 outputs, the small
            # eigenvalues crowd (no salt up to 200 separates them), and the case runs without the penalty
            t[f"p{m}x{d}_{pattern}"] = _case(m, d, weights=pattern, group="weights", only="weighted",
                                             opts={"cond_reg": 0.0} if m < 5 * d else None)
        for pattern in ("first", "last"):    # one pair carries everything: the covariances vanish, no direction
            t[f"p{m}x{d}_{pattern}"] = _case(m, d, weights=pattern, group="weights", only="weighted", compare="loss",
                                             opts={"cond_reg": 0.0},
                                             expect=dict(ZERO))
    zero = {"eps": 0.0, "eps_abs": 0.0, "alpha": 0.0}
    for d in BRANCH_WIDTHS:
        t[f"b_constant{d}"] = _case(257, d, inputs="constant", weights="pow2", group="branches",
                                    expect=dict(ZERO))
        t[f"b_ladder{d}"] = _case(257, d, inputs="one_constant", opts={**zero, "cond_reg": 0.05}, group="branches",
                                  weights="pow2", jacobi=True,
                                  expect={"total": 1e-8, "clamped": False, "halves": (True, False)},
                                  **LADDER_BOUNDS[d])
        t[f"b_nocond{d}"] = _case(257, d, opts={"cond_reg": 0.0}, group="branches",
                                  expect={"total": 0.0, "clamped": False, "halves": (False, False)})
        t[f"b_alpha1_{d}"] = _case(257, d, opts={"alpha": 1.0, "cond_reg": 0.05}, group="branches",
                                   expect={"total": 0.0, "clamped": False, "halves": (False, False)})
    t["b_graded64"] = _case(257, 64, inputs="graded", opts={"eps": 1e-7, "eps_abs": 0.0, "alpha": 0.0, "cond_reg": 1e-4},
                            group="branches", jacobi=True, **GRADED_BOUNDS)
    return t


# bound = 100 x route, the measured disagreement of the two routes (the larger of the plain and the weighted run)
# ladder, d = 64: 3.9e-13 plain, 4.1e-12 weighted (both gradients; A + 1e-8 I has cond 1e9 in the constant output's
# direction).  d = 5: 1.2e-14, inside ROUTE.  graded: 7.5e-9 plain, 4.6e-9 weighted (eig_Ctt_min, cond_Ctt: eigh leaves
# eps l_max = 2e-16 in an eigenvalue of 5e-9 l_max, the longdouble Jacobi does not).
LADDER_BOUNDS = {5: {"bound": YARDSTICK, "route": None}, 64: {"bound": 4.1e-10, "route": 4.1e-12}}
GRADED_BOUNDS = {"bound": 7.5e-7, "route": 7.5e-9}

CASES: dict = {}


def _fill():
    CASES.clear()
    CASES.update(_table())


def ordinary(name: str) -> bool:
    """A case by the plain recipe with pairs enough for its outputs, some covariance left in the regularised matrix
    and weight on more than one pair: cond <= COND_ORDINARY is asked of these."""
    c = CASES[name]
    return (c["inputs"] == "recipe" and c["m"] >= c["d"] + 2 and c["opts"]["alpha"] < 1.0
            and c["weights"] not in ("first", "last"))


def runs(name: str) -> tuple:
    """The runs of a case: False (plain), True (weighted)."""
    only = CASES[name]["only"]
    return (True,) if only == "weighted" else (False,) if only == "plain" else (False, True)


def paths(name: str, weighted: bool, chunk: int = CHUNK) -> tuple:
    """(chunks, ragged last chunk, tiles a side, ragged last tile, LDS request above the switch, weighted)"""
    c = CASES[name]
    m, d = c["m"], c["d"]
    return (-(-m // chunk), m % chunk != 0, -(-d // TILE), d % TILE != 0, 2 * d * d * 8 > LDS_SWITCH, weighted)


def assert_every_path(chunk: int):
    """The table reaches, weighted and not: 1, 2, 3 and 4 chunks (one and two of them full and ragged, three and four ragged), each at 1, 2 and 4 tiles a side and
    on both sides of the LDS switch; at two chunks 1 to 4 tiles a side, each with a full and a ragged last tile; and
    every named branch of the solve at d = 5 and d = 64."""
    seen = {paths(name, weighted, chunk) for name in CASES for weighted in runs(name)}
    for weighted in (False, True):
        for chunks in (1, 2, 3, 4):
            mine = {p for p in seen if p[0] == chunks and p[5] == weighted}
            assert {p[2] for p in mine} >= {1, 2, 4}, (chunks, weighted)
            assert {p[4] for p in mine} == {False, True}, (chunks, weighted)
            assert {p[1] for p in mine} == ({False, True} if chunks < 3 else {True}), (chunks, weighted)
        for tiles in (1, 2, 3, 4):
            assert {p[3] for p in seen if p[0] == 2 and p[2] == tiles and p[5] == weighted} == {False, True}, tiles
        for d in BRANCH_WIDTHS:
            lds = 2 * d * d * 8 > LDS_SWITCH
            assert lds == (d == 64)
            for kind, expect in (("constant", ZERO), ("ladder", {"total": 1e-8, "halves": (True, False)}),
                                 ("nocond", {"halves": (False, False)}), ("alpha1_", {"halves": (False, False)})):
                c = CASES[f"b_{kind}{d}"]
                assert weighted in runs(f"b_{kind}{d}") and all(c["expect"][k] == v for k, v in expect.items())
    assert any(c["expect"] and c["expect"].get("zero") and c["m"] == 1 for c in CASES.values())


def workspace_doubles(m: int, d: int, weighted: bool) -> int:
    """vamp_work's layout: per chunk 2d column sums and 3 d^2 moments; G (3 d^2), the means (2d), ten d x d
    matrices; under weights two sums per chunk and the two totals."""
    chunks = -(-m // CHUNK)
    n = chunks * 2 * d + chunks * 3 * d * d + 3 * d * d + 2 * d + 10 * d * d
    return n + (chunks * 2 + 2 if weighted else 0)


# ---- the law, and what it rests on ---------------------------------------------------------------------------------
_LAW: dict = {}


def law(name: str, weighted: bool) -> dict:
    """The law of a run (T.vamp2 or WR.vamp2_weighted), computed once and shared; `penalty` added from its metrics."""
    if (name, weighted) not in _LAW:
        Y0, Yt, w = inputs(name)
        o = CASES[name]["opts"]
        res = WR.vamp2_weighted(Y0, Yt, w, **o) if weighted else T.vamp2(Y0, Yt, **o)
        res["penalty"] = penalty_of(res["metrics"], o["cond_reg"])
        _LAW[name, weighted] = res
    return _LAW[name, weighted]


def penalty_of(metrics: dict, cond_reg: float) -> float:
    cond_reg = max(cond_reg, 0.0)
    if not cond_reg > 0.0:
        return 0.0
    return cond_reg * (np.log(max(metrics["cond_C00"], 1.0)) + np.log(max(metrics["cond_Ctt"], 1.0)))


def law_sides(name: str, weighted: bool) -> list:
    """What T._side did on each side of a run, from the law's own arithmetic: (total, clamped, (v_max half, v_min
    half), eigenvalues of the regularised matrix, cond of the factorised matrix A + total I scaled to a unit diagonal)."""
    Y0, Yt, w = inputs(name)
    o = CASES[name]["opts"]
    eps, eps_abs, alpha, cond_reg = o["eps"], max(o["eps_abs"], 0.0), min(max(o["alpha"], 0.0), 1.0), max(o["cond_reg"], 0.0)
    m, d = Y0.shape
    if weighted:
        wc = np.clip(w, 0.0, None)
        wh = (wc / float(wc.sum()))[:, None]
        A0, At = Y0 - (wh * Y0).sum(axis=0), Yt - (wh * Yt).sum(axis=0)
    else:
        A0, At = Y0 - Y0.mean(axis=0), Yt - Yt.mean(axis=0)
    out = []
    for X in (A0, At):
        C = X.T @ (wh * X) if weighted else X.T @ X / m
        tr = np.trace(C)
        mu = max(tr, FLOOR) / d
        A = (1.0 - alpha) * C + (alpha * mu + max(mu * eps, mu * eps_abs)) * np.eye(d)
        A = 0.5 * (A + A.T)
        side = T._side(C, eps, eps_abs, alpha, cond_reg)
        total = float(np.mean(np.diag(side[0]) - np.diag(A)))
        ev = np.linalg.eigh(A)[0]
        halves = (bool(side[2] > 1.0 and ev[-1] > FLOOR and cond_reg > 0.0),
                  bool(side[2] > 1.0 and ev[0] > FLOOR and cond_reg > 0.0))
        scale = 1.0 / np.sqrt(np.diag(side[0]))
        out.append((total, not tr >= FLOOR, halves, ev, float(np.linalg.cond(side[0] * np.outer(scale, scale)))))
    return out


def sensitivity(ev, halves=(True, True)) -> float:
    """eps l_max / gap for the worse of the extreme eigenvalues of an ascending spectrum whose penalty half (v_max,
    v_min) is present; 0 when none is."""
    ev = np.asarray(ev, np.float64)
    gaps = [g for g, on in ((ev[-1] - ev[-2], halves[0]), (ev[1] - ev[0], halves[1])) if on] if ev.size > 1 else []
    if not gaps:
        return 0.0
    return float(EPS64 * ev[-1] / min(gaps)) if min(gaps) > 0.0 else np.inf


# ---- the second route ------------------------------------------------------------------------------------------------
def jacobi_ld(A):
    """Eigenvalues (ascending) and eigenvectors of a symmetric matrix by cyclic Jacobi in longdouble."""
    A = np.array(A, LD)
    d = A.shape[0]
    V = np.eye(d, dtype=LD)
    for _ in range(60):
        rotated = False
        for p in range(d - 1):
            for q in range(p + 1, d):
                apq = A[p, q]
                if not abs(apq) > LD(1e-21) * np.sqrt(abs(A[p, p] * A[q, q])):
                    continue
                rotated = True
                theta = (A[q, q] - A[p, p]) / (2 * apq)
                t = (1 if theta >= 0 else -1) / (abs(theta) + np.sqrt(theta * theta + 1))
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                Ap, Aq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * Ap - s * Aq, s * Ap + c * Aq
                Ap, Aq = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * Ap - s * Aq, s * Ap + c * Aq
                A[p, q] = A[q, p] = 0
                Vp, Vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * Vp - s * Vq, s * Vp + c * Vq
        if not rotated:
            break
    else:
        raise RuntimeError("Jacobi did not converge")
    w = np.diag(A).copy()
    order = np.argsort(w)
    return w[order], V[:, order]


def _side2(C, eps, eps_abs, alpha, cond_reg, jacobi):
    d = C.shape[0]
    I = np.eye(d, dtype=LD)
    tr = np.trace(C)
    clamped = not tr >= FLOOR
    mu = max(tr, LD(FLOOR)) / d
    ridge = max(mu * eps, mu * eps_abs)
    A = (1 - LD(alpha)) * C + (alpha * mu + ridge) * I
    A = (A + A.T) / 2
    if jacobi:
        w, V = jacobi_ld(A)
    else:
        w, V = np.linalg.eigh(A.astype(np.float64))
        w, V = w.astype(LD), V.astype(LD)
    lmin, lmax = max(w[0], LD(FLOOR)), max(w[-1], LD(FLOOR))
    cond = lmax / lmin
    halves = (bool(cond > 1 and w[-1] > FLOOR and cond_reg > 0), bool(cond > 1 and w[0] > FLOOR and cond_reg > 0))
    pen = np.zeros((d, d), LD)
    if halves[0]:
        pen += cond_reg * np.outer(V[:, -1], V[:, -1]) / w[-1]
    if halves[1]:
        pen -= cond_reg * np.outer(V[:, 0], V[:, 0]) / w[0]
    total = None
    for rung in LADDER:
        if w[0] + rung > d * EPS64 * max(abs(w[-1]), abs(w[0])):
            total = rung
            break
    if total is None:
        raise RuntimeError("not positive definite after the ladder")
    Ai = (V / (w + total)) @ V.T
    c = LD(0) if clamped else alpha + ridge / mu
    return {"Ai": Ai, "cond": cond, "lmin": lmin, "lmax": lmax, "pen": pen, "c": c, "total": float(total),
            "clamped": clamped, "halves": halves, "ev": w.astype(np.float64)}


def second_route(Y0, Yt, w=None, eps=1e-3, eps_abs=1e-6, alpha=0.15, cond_reg=1e-4, jacobi=False) -> dict:
    """The dict of the law by the route of the module docstring, with `sides` (what each side's solve did)."""
    Y0, Yt = np.asarray(Y0, LD), np.asarray(Yt, LD)
    m, d = Y0.shape
    eps_abs, alpha, cond_reg = max(eps_abs, 0.0), min(max(alpha, 0.0), 1.0), max(cond_reg, 0.0)
    wc = np.ones(m, LD) if w is None else np.clip(np.asarray(w, LD).reshape(-1), 0, None)
    W = wc.sum()
    wh = (wc / W)[:, None]
    m0, mt = (wh * Y0).sum(axis=0), (wh * Yt).sum(axis=0)
    A0, At = Y0 - m0, Yt - mt
    C00, Ctt, C0t = A0.T @ (wh * A0), At.T @ (wh * At), A0.T @ (wh * At)
    a = _side2(C00, eps, eps_abs, alpha, cond_reg, jacobi)
    b = _side2(Ctt, eps, eps_abs, alpha, cond_reg, jacobi)
    Ai, Bi = a["Ai"], b["Ai"]
    AiC = Ai @ C0t
    AiCBi = AiC @ Bi
    score = np.trace(AiCBi @ C0t.T)
    penalty = cond_reg * (np.log(max(a["cond"], LD(1))) + np.log(max(b["cond"], LD(1)))) if cond_reg > 0 else LD(0)
    GA = AiCBi @ AiC.T + a["pen"]
    GB = AiCBi.T @ C0t @ Bi + b["pen"]
    G0t = -2 * AiCBi
    I = np.eye(d, dtype=LD)
    G00 = (1 - LD(alpha)) * GA + a["c"] / d * np.trace(GA) * I
    Gtt = (1 - LD(alpha)) * GB + b["c"] / d * np.trace(GB) * I
    g0 = wh * (2 * A0 @ G00 + At @ G0t.T)
    gt = wh * (2 * At @ Gtt + A0 @ G0t)
    f = lambda x: np.asarray(x, np.float64)                                     # noqa: E731
    metrics = {"cond_C00": float(a["cond"]), "cond_Ctt": float(b["cond"]), "var_z0": f(np.diag(C00)).tolist(),
               "var_zt": f(np.diag(Ctt)).tolist(), "mean_z0": f(m0).tolist(), "mean_zt": f(mt).tolist(),
               "eig_C00_min": float(a["lmin"]), "eig_C00_max": float(a["lmax"]), "eig_Ctt_min": float(b["lmin"]),
               "eig_Ctt_max": float(b["lmax"])}
    res = {"loss": float(-score + penalty), "score": float(score), "penalty": float(penalty), "metrics": metrics,
           "grad0": f(g0), "grad_t": f(gt),
           "sides": [(s["total"], s["clamped"], s["halves"], s["ev"]) for s in (a, b)]}
    if w is not None:
        res["total_weight"], res["effective_pairs"] = float(W), float(W * W / np.sum(wc * wc))
    return res


def second(name: str, weighted: bool) -> dict:
    Y0, Yt, w = inputs(name)
    c = CASES[name]
    return second_route(Y0, Yt, w if weighted else None, jacobi=c["jacobi"], **c["opts"])


# ---- distances -------------------------------------------------------------------------------------------------------
def _rel(got, want) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, scale = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
    return err / scale if scale > 0.0 else err


def distances(got: dict, want: dict, compare: str = "all") -> dict:
    """|got - want| of loss, score, penalty, every metric and (compare "all") both gradients, each as a fraction of
    the largest entry of `want` (an exact zero: the absolute distance); a gradient whose two terms cancel -- its
    largest entry is under 1e-6 of want's term_scale -- is measured in term_scale, as test_vamp2_loss does."""
    dist = {key: _rel(got[key], want[key]) for key in ("loss", "score", "penalty")}
    for key in ("total_weight", "effective_pairs"):
        if key in want:
            dist[key] = _rel(got[key], want[key])
    assert set(got["metrics"]) == set(want["metrics"]) and len(want["metrics"]) == 10
    for key, value in want["metrics"].items():
        dist[key] = _rel(got["metrics"][key], value)
    if compare == "all":
        for key in ("grad0", "grad_t"):
            top = float(np.max(np.abs(want[key])))
            scale = top if top > 1e-6 * want["term_scale"] else want["term_scale"]
            err = float(np.max(np.abs(np.asarray(got[key]) - want[key])))
            dist[key] = err / scale if scale > 0.0 else err
    return dist


def assert_zero_case(res: dict, means: dict, tol: float = 1e-20):
    """A run whose covariances vanish (constant outputs, one pair, all weight on one pair): loss, score and penalty 0,
    cond 1, the eigenvalues on the floor, zero variances and a zero gradient, the means those of `means`.  Exact
    zeros in exact arithmetic; `tol` (absolute, twenty orders under an ordinary score) admits the 1e-32 that a
    normalised weight vector not summing to exactly 1 leaves in the law's covariances."""
    for key in ("loss", "score", "penalty"):
        assert abs(res[key]) <= tol, (key, res[key])
    mt = res["metrics"]
    assert mt["cond_C00"] == 1.0 and mt["cond_Ctt"] == 1.0
    assert all(mt[k] == FLOOR for k in ("eig_C00_min", "eig_C00_max", "eig_Ctt_min", "eig_Ctt_max"))
    assert np.max(np.abs(mt["var_z0"])) <= tol and np.max(np.abs(mt["var_zt"])) <= tol
    for key in ("mean_z0", "mean_zt"):
        assert _rel(mt[key], means[key]) <= YARDSTICK
    for key in ("grad0", "grad_t"):
        if key in res:
            assert np.max(np.abs(np.asarray(res[key]))) <= tol, key


_fill()
