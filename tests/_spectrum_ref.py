"""Exact references, chain generators and the launch-path rule of msm_spectrum (test infrastructure only).

Reversible chains T = D^-1 C (C symmetric, D = diag of its row sums) have everything the solver reports in closed
form or through a backward-stable symmetric eigensolve: pi = rowsum / total, the eigenvalues of T are those of
D^-1/2 C D^-1/2, and the left eigenvectors are x = D^1/2 u for its eigenvectors u.  `spectrum_path` restates which
code path `plan_persist` / `spectrum_impl` (pmarlo_amd/csrc/msm.hip) and the finishing step take for a shape; the GPU
tests check it against the library's MSM_SPEC_DEBUG lines."""

from __future__ import annotations

import re

import numpy as np

from oracle import npport

# ---------------------------------------------------------------------------------------------------------------
# the launch-path rule (plan_persist and spectrum_impl; side_by_side: the finish of spec_step_kernel)
# ---------------------------------------------------------------------------------------------------------------
K_MAX_P = 32
LDS_W_BYTES = 96 * 1024                              # W of the loop's step kernel in LDS up to here
LDS_W_ATTR_BYTES = 12 * 1024                         # above this the step kernel asks for more dynamic LDS
PERSIST_BUDGET = (160 - 24 - 4) * 1024 // 8          # doubles of LDS for the persistent kernel's T / Z / W
XCDS, CUS_PER_XCD = 8, 32
SOLVE_WAVES = 1024 // 64


def engine_p(k: int, n_its: int = 0, n_vecs: int = 0, p: int | None = None, n_watch: int | None = None):
    """(p, n_watch) as Engine._spectrum chooses them."""
    n_vecs = int(min(n_vecs, 32, k))
    watch = int(n_watch) if n_watch is not None else max(n_its + 1, n_vecs, 1)
    if p is None:
        p = min(32, max(watch + 6, 8))
    return int(min(p, 32, k)), watch


def spectrum_path(n_max: int, p: int, batch: int, n_watch: int, n_cu: int = XCDS * CUS_PER_XCD) -> dict:
    """The branches msm_spectrum takes for a batch of `batch` matrices of order <= n_max at subspace width p."""
    budget = PERSIST_BUDGET
    fixed = n_max * (p | 1)
    cols = (budget - fixed) // (n_max + p + 2) if budget > fixed + 8 * (n_max + p + 2) else 0
    cols = min(cols, n_max)

    def fits(c):
        return n_max * (c | 1) + fixed + c * p <= budget

    while cols >= 8 and not fits(cols):
        cols -= 1
    G = per_xcd = groups = 0
    if cols >= 8:
        G = -(-n_max // cols)
        while cols > 1 and (n_max + cols - 2) // (cols - 1) == G and fits(cols - 1):
            cols -= 1
        per_xcd = CUS_PER_XCD // G if G <= CUS_PER_XCD else 0
        groups = batch if batch <= XCDS * per_xcd else 0
    persistent = groups >= 1 and -(-groups // XCDS) * G * XCDS <= n_cu
    w_bytes = n_max * p * 8
    nw = min(n_watch, p)
    per = p * p + 3 * p
    return {
        "first_cols": cols if G == 0 else None,
        "cols": cols if G else 0, "G": G, "per_xcd": per_xcd, "groups": groups if persistent else 0,
        "persistent": persistent,
        "lds_w": w_bytes <= LDS_W_BYTES,
        "lds_attr": LDS_W_ATTR_BYTES < w_bytes <= LDS_W_BYTES,
        "w_bytes": w_bytes,
        "apply": 8 if p <= 8 else 16 if p <= 16 else 24 if p <= 24 else 32,
        "apply_blocks": (n_max + 255) // 256,
        "side_by_side": (nw + 1) * per <= 3 * K_MAX_P * K_MAX_P and nw + 1 <= SOLVE_WAVES,
    }


def loop_batch(n_max: int, p: int) -> int:
    """The smallest batch of this shape that no longer gets a persistent launch."""
    per_xcd = spectrum_path(n_max, p, 1, 1)["per_xcd"]
    return XCDS * per_xcd + 1


_FIRST = re.compile(r"msm_spectrum: n=(\d+) p=(\d+) first cols=(-?\d+)")
_PERSIST = re.compile(r"msm_spectrum: persistent launch n=(\d+) p=(\d+) cols=(\d+) G=(\d+) groups=(\d+) lds=\d+ -> (.*)$")


def parse_debug(text: str) -> list[dict]:
    """The MSM_SPEC_DEBUG lines of a run: one entry per msm_spectrum call that iterated, with its persistent launch
    (or None)."""
    calls = []
    for line in text.splitlines():
        m = _FIRST.search(line)
        if m:
            calls.append({"n": int(m[1]), "p": int(m[2]), "persist": None})
            continue
        m = _PERSIST.search(line)
        if m:
            assert calls and calls[-1]["persist"] is None, f"persistent line without its first line: {line}"
            assert (calls[-1]["n"], calls[-1]["p"]) == (int(m[1]), int(m[2])), line
            calls[-1]["persist"] = {"cols": int(m[3]), "G": int(m[4]), "groups": int(m[5]), "result": m[6].strip()}
    return calls


def check_debug(text: str, batch: int, n_watch: int) -> list[dict]:
    """Every call in the log took the persistent launch exactly when spectrum_path says so, with its cols / G / groups."""
    calls = parse_debug(text)
    assert calls, "no MSM_SPEC_DEBUG lines: the library did not iterate, or stopped reading the variable"
    for c in calls:
        want = spectrum_path(c["n"], c["p"], batch, n_watch)
        if want["persistent"]:
            assert c["persist"] is not None, f"restated rule says persistent, library looped: {c} vs {want}"
            got = c["persist"]
            assert (got["cols"], got["G"], got["groups"]) == (want["cols"], want["G"], want["groups"]), (got, want)
            assert got["result"] == "no error", got
        else:
            assert c["persist"] is None, f"restated rule says loop, library launched persistent: {c} vs {want}"
    return calls


# ---------------------------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------------------------
def _sym(a):
    return np.triu(a) + np.triu(a, 1).T


def block_counts(k: int, n_blocks: int, leak: float, seed: int, *, bipartite: tuple[int, ...] = (),
                 identical: bool = False, chain: bool = False, density: float = 1.0) -> np.ndarray:
    """Symmetric non-negative counts of a metastable chain: `n_blocks` blocks with dense random weight inside, `leak`
    times the mean inside weight between blocks (all pairs, or neighbouring blocks only with chain=True).  Blocks in
    `bipartite` carry their weight only between their two halves (plus 1e-2 of it inside each half): a Ritz value near
    -1.  identical=True repeats one block and couples every pair of blocks by the same constant, so the slow
    eigenvalue is exactly (n_blocks - 1)-fold."""
    rng = np.random.default_rng(seed)
    bounds = np.linspace(0, k, n_blocks + 1).astype(int)
    if identical:
        assert k % n_blocks == 0
        w = k // n_blocks
        blk = _sym(rng.random((w, w)) + 0.1)
        C = np.kron(np.eye(n_blocks), blk) + leak * (np.ones((k, k)) - np.kron(np.eye(n_blocks), np.ones((w, w))))
        return C
    C = np.zeros((k, k))
    for b in range(n_blocks):
        s, e = bounds[b], bounds[b + 1]
        w = e - s
        blk = _sym(rng.random((w, w)) * (rng.random((w, w)) < density) + 0.05)
        if b in bipartite:
            h = w // 2
            mask = np.zeros((w, w))
            mask[:h, h:] = 1.0
            mask[h:, :h] = 1.0
            blk = blk * (mask + 1e-2 * (1.0 - mask))
        C[s:e, s:e] = blk
    mean_in = C.sum() / sum((bounds[b + 1] - bounds[b]) ** 2 for b in range(n_blocks))
    out = _sym(rng.random((k, k))) * leak * mean_in
    if chain:
        near = np.abs(np.searchsorted(bounds, np.arange(k), "right")[:, None]
                      - np.searchsorted(bounds, np.arange(k), "right")[None, :]) == 1
        out = out * near
    same = np.searchsorted(bounds, np.arange(k), "right")
    out[same[:, None] == same[None, :]] = 0.0
    return C + out


def rownorm(C: np.ndarray) -> np.ndarray:
    return C / C.sum(axis=1, keepdims=True)


def drift_chain(k: int, seed: int, eps: float = 0.03, n_blocks: int = 3) -> np.ndarray:
    """A non-reversible chain: metastable blocks with a cyclic drift between them (a complex slow pair)."""
    rng = np.random.default_rng(seed)
    w = k // n_blocks
    P = np.zeros((k, k))
    for b in range(n_blocks):
        e = k if b == n_blocks - 1 else w * (b + 1)
        blk = rng.random((e - w * b, e - w * b)) + 0.2
        P[w * b:e, w * b:e] = rownorm(blk)
    shift = np.zeros((k, k))
    for i in range(k):
        shift[i, (i + w) % k] = 1.0
    return (1.0 - eps) * P + eps * shift


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def sign_fix(x: np.ndarray) -> np.ndarray:
    """Unit 2-norm, the component of largest magnitude positive (lowest index on ties): the kernel's convention."""
    x = x / np.linalg.norm(x)
    lead = int(np.argmax(np.abs(x)))
    return x if x[lead] > 0 else -x


def reversible_reference(C: np.ndarray, n_its: int, lag: float = 1.0, n_vecs: int = 0) -> dict:
    """Exact spectrum data of T = rownorm(C) for a symmetric non-negative C (every row sum > 0)."""
    C = np.asarray(C, dtype=np.float64)
    assert np.array_equal(C, C.T) and (C >= 0).all()
    row = C.sum(axis=1)
    assert (row > 0).all()
    n = C.shape[0]
    dh = np.sqrt(row)
    S = C / dh[:, None] / dh[None, :]
    if n_vecs:
        ev, U = np.linalg.eigh(S)
    else:
        ev, U = np.linalg.eigvalsh(S), None
    order = np.argsort(-np.abs(ev), kind="stable")          # descending magnitude: the solver's order
    ev = ev[order]
    eig = np.full(n_its, np.nan)
    ts = np.full(n_its, np.nan)
    if n_its:
        e, t = npport.reversible_its_from_counts(C, int(max(1, lag)), n_its)
        eig[:e.size], ts[:t.size] = e, t
    out = {"ev": ev, "pi": row / row.sum(), "its_eig": eig, "its_ts": ts, "vecs": [], "gaps": []}
    for q in range(min(n_vecs, n)):
        x = sign_fix(dh * U[:, order[q]])
        others = np.delete(ev, q)
        gap = float(np.min(np.minimum(np.abs(others - ev[q]), np.abs(np.abs(others) - abs(ev[q]))))) if n > 1 else 1.0
        out["vecs"].append(x)
        out["gaps"].append(gap)
    return out


def nonreversible_reference(T: np.ndarray, m: int) -> dict:
    """The m leading eigenvalues of T by magnitude with their condition numbers 1 / |y^H x| (unit x, y), and pi."""
    import scipy.linalg

    w, vl, vr = scipy.linalg.eig(T, left=True, right=True)
    order = np.argsort(-np.abs(w), kind="stable")
    w, vl, vr = w[order], vl[:, order], vr[:, order]
    cond = np.empty(len(w))
    for i in range(len(w)):
        x = vr[:, i] / np.linalg.norm(vr[:, i])
        y = vl[:, i] / np.linalg.norm(vl[:, i])
        cond[i] = 1.0 / abs(np.vdot(y, x))
    i1 = int(np.argmin(np.abs(w - 1.0)))
    pi = np.real(vl[:, i1])
    return {"ev": w[:m], "cond": cond[:m], "pi": pi / pi.sum()}


# ---------------------------------------------------------------------------------------------------------------
# the shape table: every branch of the path table and both sides of each threshold
# ---------------------------------------------------------------------------------------------------------------
def _case(name, k, *, batch=1, p=None, n_its=3, n_vecs=0, orders=None, gen="blocks", note=""):
    pe, watch = engine_p(k, n_its, n_vecs, p)
    return {"name": name, "k": k, "batch": batch, "p": p, "n_its": n_its, "n_vecs": n_vecs, "orders": orders,
            "gen": gen, "p_eff": pe, "watch": watch, "path": spectrum_path(k, pe, batch, watch), "note": note}


def _table():
    cases = [
        _case("g1_p8", 64, p=8, n_its=3, n_vecs=2),
        _case("g1_p9_bipartite", 96, p=9, n_its=4, n_vecs=3, gen="bipartite"),
        _case("persist_k200", 200, n_its=3, n_vecs=3),
        _case("persist_k255_p16", 255, p=16, n_its=5, n_vecs=2),
        _case("persist_k256_p17", 256, p=17, n_its=5, n_vecs=2),
        _case("persist_k257_p24_bipartite", 257, p=24, n_its=6, gen="bipartite"),
        _case("persist_k300_p25", 300, p=25, n_its=6, n_vecs=4),
        _case("persist_k400_identical", 400, n_its=3, gen="identical"),
        _case("persist_g32_k544", 544, p=12, n_its=5, n_vecs=2),
        _case("loop_lds_g33_k545", 545, p=12, n_its=5, n_vecs=2),
        _case("loop_lds_k511_its10", 511, n_its=10, n_vecs=3),
        _case("loop_glob_k513_p32", 513, p=32, n_its=3, n_vecs=2, gen="bipartite"),
        _case("loop_lds_k384_p32_96k", 384, p=32, n_its=10, n_vecs=3),
        _case("loop_glob_k385_p32_96k", 385, p=32, n_its=10, n_vecs=3),
        _case("loop_lds_k700_its10", 700, n_its=10, n_vecs=2),
        _case("loop_lds_k1000_p10", 1000, p=10, n_its=3, n_vecs=3),
        _case("loop_lds_k1228_96k", 1228, p=10, n_its=3, n_vecs=2),
        _case("loop_glob_k1229_96k", 1229, p=10, n_its=3, n_vecs=2),
        _case("loop_glob_k1300_p32", 1300, p=32, n_its=10, n_vecs=2),
        _case("loop_glob_k2000_p10", 2000, p=10, n_its=3, n_vecs=2),
        _case("loop_glob_k2000_p32", 2000, p=32, n_its=10),
    ]
    # batches on both sides of the persistent limit batch <= 8 * per_xcd (k = 200: ten groups of three per XCD)
    for k, p in ((200, 10), (544, 12)):
        lb = loop_batch(k, p)
        cases.append(_case(f"batch_persist_k{k}_b{lb - 1}", k, batch=lb - 1, p=p, n_its=3, n_vecs=2))
        cases.append(_case(f"batch_loop_k{k}_b{lb}", k, batch=lb, p=p, n_its=3, n_vecs=2))
    # W of the loop at 12 KB (no LDS attribute) and one row more
    for k in (192, 193):
        cases.append(_case(f"batch_loop_w12k_k{k}", k, batch=loop_batch(k, 8), p=8, n_its=3))
    # ragged batches (orders n_max, n_max - 1, 257, p + 2, p, 2, 1) on both paths
    for k, p in ((544, 12), (300, 12)):
        orders = [k, k - 1, 257, p + 2, p, 2, 1]
        cases.append(_case(f"ragged_persist_k{k}", k, batch=len(orders), p=p, n_its=4, n_vecs=2, orders=orders))
        lb = loop_batch(k, p)
        more = orders + [k - 3 - i for i in range(lb - len(orders))]
        cases.append(_case(f"ragged_loop_k{k}", k, batch=lb, p=p, n_its=4, n_vecs=2, orders=more))
    return cases


CASES = _table()


def case_counts(case: dict, n: int, seed: int) -> np.ndarray:
    """Symmetric counts of order n for a table case (tiny orders of a ragged batch: a dense random chain)."""
    if n < 16:
        return _sym(np.random.default_rng(seed).random((n, n)) + 0.05)
    if case["gen"] == "identical":
        return block_counts(n, 4, 0.006, seed, identical=True)
    if case["gen"] == "bipartite":
        return block_counts(n, max(3, case["n_its"] + 1), 0.3, seed, chain=True, bipartite=(0,))
    return block_counts(n, case["n_its"] + 2, 0.3, seed, chain=True)


def case_orders(case: dict) -> list[int]:
    return list(case["orders"]) if case["orders"] else [case["k"]] * case["batch"]
