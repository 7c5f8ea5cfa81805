"""numpy restatement of the TRAM contract (include/msmhip.h, "TRAM"; Wu, Paul, Wehmeyer, Noe 2016): the two row sums,
the frame pass, the update, the solver on the device's schedule, the transition matrices; the inputs the CPU and GPU
tests share; the rounding bounds both hold results to.

Every step takes a `dtype`: np.float64 is the restatement proper, np.longdouble (80-bit on x86, eps 1.1e-19) the
near-exact yardstick the device is compared with.
"""
from __future__ import annotations

import functools

import numpy as np

ULP = 2.0 ** -52
SEGMENT = 256                  # frames of a pass unit (MSM_TRAM_SEGMENT); the GPU tests check it against tram_plan
KB = 0.00831446261815324       # kJ / mol / K


# ---- the steps ---------------------------------------------------------------------------------------------------
def log_multipliers(f, v, dtype=np.float64):
    """g = ln v + f, -inf where v = 0."""
    f, v = np.asarray(f).astype(dtype), np.asarray(v).astype(dtype)
    with np.errstate(divide="ignore"):
        return np.where(v > 0, np.log(np.where(v > 0, v, 1)) + f, -np.inf).astype(dtype)


def rows(S, g, f, N, col, mode, dtype=np.float64):
    """mode "multipliers": out = sum_j S_ij / (1 + exp(g_j - g_i)); mode "counts": out = sum_j S_ij / (1 + exp(g_i -
    g_j)) + (N_i - col_i); terms with S_ij = 0 skipped, inactive pairs (N = 0) give 0 -> (out, ln out + f)."""
    S, g, f = (np.asarray(a).astype(dtype) for a in (S, g, f))
    N, col = np.asarray(N).astype(dtype), np.asarray(col).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        x = g[:, None, :] - g[:, :, None]                    # [k, i, j] = g_j - g_i
        if mode == "counts":
            x = -x
        term = np.where(S != 0, S / (1 + np.exp(np.where(S != 0, x, 0))), 0)
    out = term.sum(axis=2)
    if mode == "counts":
        out = out + (N - col)
    out = np.where(N > 0, out, 0).astype(dtype)
    with np.errstate(divide="ignore"):
        lnout = np.where(out > 0, np.log(np.where(out > 0, out, 1)) + f, -np.inf).astype(dtype)
    return out, lnout


def frame_pass(u, state, tab, m, dtype=np.float64):
    """Step 3 over u [K, N] with Markov states `state` [N] (any order) at tab = ln R + f [K, m]
    -> dict(d [N], r [K, N], s [K, m], status)."""
    u, tab = np.asarray(u).astype(dtype), np.asarray(tab).astype(dtype)
    state = np.asarray(state, np.int64)
    status = 0
    if np.isnan(u).any() or np.isneginf(u).any():
        status |= 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mn = u.min(axis=0)
        a = tab[:, state] - (u - mn[None, :])
        M = np.max(np.where(np.isnan(a), -np.inf, a), axis=0)
        e = np.exp(a - M[None, :])
        Ssum = e.sum(axis=0)
        d = (M + np.log(Ssum)) - mn
        r = e * (1 / Ssum)[None, :]
    bad = (np.isnan(u) | np.isneginf(u)).any(axis=0)
    dead = ~np.isfinite(d) | bad
    if (dead & ~bad).any():
        status |= 2
    r[:, dead] = 0
    d = np.where(bad, np.nan, np.where(dead, -np.inf, d)).astype(dtype)      # no finite term: d_n = -inf
    order = np.argsort(state, kind="stable")
    cnt = np.bincount(state, minlength=m)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    s = np.zeros((u.shape[0], m), dtype)
    has = cnt > 0
    s[:, has] = np.add.reduceat(r[:, order], starts[has], axis=1)
    return {"d": d, "r": r, "s": s, "status": status}


def update(N, tab, s, v, f, dtype=np.float64):
    """Steps 4 and 5 -> (f_new, g_new, err)."""
    tab, s, f = (np.asarray(a).astype(dtype) for a in (tab, s, f))
    act = np.asarray(N) > 0
    fn = f.copy()
    with np.errstate(divide="ignore"):
        fn[act] = tab[act] - np.log(s[act])
    fn[act] = fn[act] - fn[act].min()
    err = float(np.abs(fn[act] - f[act]).max())
    return fn, log_multipliers(fn, v, dtype), err


def iteration(prob, f, v, dtype=np.float64):
    """One iteration from (f, v) -> (f_new, v_new, err, pass result)."""
    g = log_multipliers(f, v, dtype)
    v1, g1 = rows(prob["S"], g, f, prob["N"], prob["col"], "multipliers", dtype)
    _, tab = rows(prob["S"], g1, f, prob["N"], prob["col"], "counts", dtype)
    p = frame_pass(prob["u"], prob["state"], tab, prob["N"].shape[1], dtype)
    fn, _, err = update(prob["N"], tab, p["s"], v1, f, dtype)
    return fn, v1, err, p


class NotConverged(RuntimeError):
    pass


def start(prob, f0=None, dtype=np.float64):
    K, m = prob["N"].shape
    f = np.zeros((K, m), dtype) if f0 is None else np.repeat(np.asarray(f0).astype(dtype)[:, None], m, axis=1)
    v = (np.asarray(prob["S"]).astype(dtype).sum(axis=2) / 2).astype(dtype)
    return f, v


def solve(prob, tol=1e-10, maxiter=100_000, check_every=16, f0=None, dtype=np.float64):
    """The device's schedule: `check_every` iterations, then one look at err; stop at the first checked iteration
    with err <= tol -> dict(f, v, d, n_iterations, err, history [every iteration's err])."""
    f, v = start(prob, f0, dtype)
    it, hist = 0, []
    while it < maxiter:
        for _ in range(min(check_every, maxiter - it)):
            f, v, err, p = iteration(prob, f, v, dtype)
            hist.append(err)
            it += 1
        if err <= tol:
            return {"f": f, "v": v, "d": p["d"], "n_iterations": it, "err": err, "history": np.asarray(hist)}
    raise NotConverged(f"tram: err {err:.3e} > tol {tol:.1e} after {it} iterations")


def contraction(history, floor=1e-13):
    """rho: the largest ratio err[t] / err[t-1] over the last 8 iterations whose err is above `floor` (below it the
    differences are rounding), at most 1 - 2^-10."""
    h = np.asarray(history, np.float64)
    h = h[h > floor][-9:]
    if h.size < 2:
        return 0.5
    return float(min(max((h[1:] / h[:-1]).max(), 0.0), 1 - 2.0 ** -10))


def transition_matrix(S, N, f, v, k, dtype=np.float64):
    """p_ij = S_ij / (v_i + v_j exp(f_j - f_i)), i != j, active states; all divided by the largest off-diagonal row
    sum where that exceeds 1; p_ii = 1 - sum; inactive rows and columns zero."""
    Sk, fk, vk = (np.asarray(a[k]).astype(dtype) for a in (S, f, v))
    act = np.asarray(N[k]) > 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        den = vk[:, None] + vk[None, :] * np.exp(np.where(act[None, :] & act[:, None], fk[None, :] - fk[:, None], 0))
        ok = (Sk != 0) & act[:, None] & act[None, :]
        P = np.where(ok, Sk / np.where(ok, den, 1), 0)
    np.fill_diagonal(P, 0)
    top = P.sum(axis=1).max()
    if top > 1:
        P = P / top
    P[np.diag_indices_from(P)] = np.where(act, 1 - P.sum(axis=1), 0)
    return P


def stationary(N, f, k, dtype=np.float64):
    act = np.asarray(N[k]) > 0
    fk = np.asarray(f[k]).astype(dtype)
    pi = np.where(act, np.exp(-np.where(act, fk - fk[act].min(), 0)), 0)
    return pi / pi.sum()


def target_state_f(ut, d, state, m, dtype=np.float64):
    """f_i^t = -logsumexp_{n in i} (-u_t[n] - d_n) for the rows of ut [T, N] -> [T, m]."""
    ut, d = np.asarray(ut).astype(dtype), np.asarray(d).astype(dtype)
    out = np.full((ut.shape[0], m), np.inf, dtype)
    for i in range(m):
        c = -ut[:, state == i] - d[None, state == i]
        if c.shape[1]:
            mx = c.max(axis=1)
            out[:, i] = -(mx + np.log(np.exp(c - mx[:, None]).sum(axis=1)))
    return out


# ---- the rounding bounds -------------------------------------------------------------------------------------------
# In the manner of _mbar_ref.pass_bound: operations counted, times 2^-52, times the largest exponent argument.
#
# Rows.  A term is S_ij / (1 + exp(x)), x = +-(g_j - g_i).  The inputs g are given; the difference rounds once at
# |x| <= 2 max|g|, exp turns that absolute error into the same relative error of exp(x) and adds one ulp of its own,
# 1 + exp(x), the division and the final log add one each.  So a term carries (4 + |x|) ulp relative, and since all
# terms (and N - col) are >= 0 so does their sum, plus the summation itself: `chain` additions in sequence on the
# longest path.  The device adds ceil(m / 64) terms per lane, then 6 shuffle levels, then N - col: chain =
# ceil(m / 64) + 7.  numpy's sum is pairwise in blocks; m additions bound it whatever the blocking.
#     rows_bound = (chain + 8 + X) * 2^-52,    X = max |g_j - g_i| over the pairs with S_ij != 0 (0 without any)
# relative for `out`, and absolute for ln out + f after adding two roundings at max(1, |ln out|, |f|, |ln out + f|).
#
# Pass.  The exponent argument is a_l - M with a_l = tab_l - (u_ln - m_n).  As in MBAR the inner difference is exact
# when u_ln and m_n lie within a factor 2 (Sterbenz), else it rounds at |u_ln - m_n|; the outer difference rounds at
# |a_l|; a_l - M at its own size.  With A = max(1, |a_l| over the finite entries, |u_ln - m_n| where that is not exact)
# an argument carries a few 2^-52 A; per r_l there are the K terms of S and a fixed number of roundings (a, a - M,
# exp, 1 / S, the product; for d_n also M + log S, log, - m_n): FIXED_OPS = 16 covers them.  s_i^k adds `chain`
# additions: on the device 16 (a chain of a wave's row sum) + 2 + 3 (chains, waves) + the units of the state; in
# numpy's reduceat the frames of the state.
#     pass_bound = (K + chain + FIXED_OPS) * 2^-52 * A
# relative for s, absolute (plus one ulp of |d_n|) for d_n.
#
# Iteration.  One full iteration from the same (f, v): v carries rows_bound (relative), so g carries it absolutely,
# x twice that, a term of step 2 twice that relatively (|d/dx ln(1 / (1 + e^x))| <= 1) on top of its own rows_bound:
# ln R carries 3 rows_bound.  f_new = tab - ln s adds pass_bound and two roundings at max(1, |f|); the gauge
# subtracts another entry with the same error:
#     iteration_bound = 2 * (3 * rows_bound + pass_bound + 2 * 2^-52 * max(1, |tab|, |ln s|, |f|))
FIXED_OPS = 16


def rows_chain_device(m):
    return -(-m // 64) + 7


def rows_bound(S, g, chain):
    S, g = np.asarray(S, np.float64), np.asarray(g, np.float64)
    with np.errstate(invalid="ignore"):
        x = np.abs(g[:, None, :] - g[:, :, None])[S != 0]
    x = x[np.isfinite(x)]
    return (chain + 8 + (float(x.max()) if x.size else 0.0)) * ULP


def arg_magnitude(u, state, tab):
    u, tab = np.asarray(u, np.float64), np.asarray(tab, np.float64)
    mn = u.min(axis=0)[None, :]
    with np.errstate(invalid="ignore"):
        sh = u - mn
        a = np.abs(tab[:, state] - sh)
        lo, hi = np.minimum(np.abs(u), np.abs(mn)), np.maximum(np.abs(u), np.abs(mn))
        exact = (np.sign(u) == np.sign(mn)) & (hi <= 2 * lo)                   # Sterbenz
    a = a[np.isfinite(a)]
    rounded = sh[np.isfinite(sh) & ~exact]
    return max(1.0, float(a.max()) if a.size else 0.0, float(rounded.max()) if rounded.size else 0.0)


def pass_chain_device(state, m):
    return 21 + int(-(-np.bincount(np.asarray(state, np.int64), minlength=m).max() // SEGMENT))


def pass_bound(u, state, tab, chain):
    return (np.asarray(u).shape[0] + chain + FIXED_OPS) * ULP * arg_magnitude(u, state, tab)


def iteration_bound(prob, f, v, rows_chain, pass_chain):
    g = log_multipliers(f, v)
    v1, g1 = rows(prob["S"], g, f, prob["N"], prob["col"], "multipliers")
    _, tab = rows(prob["S"], g1, f, prob["N"], prob["col"], "counts")
    rb = max(rows_bound(prob["S"], g, rows_chain), rows_bound(prob["S"], g1, rows_chain))
    pb = pass_bound(prob["u"], prob["state"], tab, pass_chain)
    s = frame_pass(prob["u"], prob["state"], tab, tab.shape[1])["s"]
    act = prob["N"] > 0
    mag = max(1.0, float(np.abs(tab[act]).max()), float(np.abs(np.log(s[act])).max()), float(np.abs(f[act]).max()))
    return 2 * (3 * rb + pb + 2 * ULP * mag)


def check_rows(got, want, bound, f):
    """got, want: (out, ln out + f); `out` relative, ln out + f absolute with two roundings at its magnitudes."""
    out, lnout = (np.asarray(a, np.longdouble) for a in got)
    out_r, ln_r = (np.asarray(a, np.longdouble) for a in want)
    pos = out_r > 0
    assert np.array_equal(out[~pos], out_r[~pos]) and np.array_equal(lnout[~pos], ln_r[~pos])       # 0 and -inf
    if pos.any():
        err = (np.abs(out - out_r)[pos] / out_r[pos]).astype(np.float64)
        assert (err <= bound).all(), ("rows", float(err.max() / bound))
        mag = np.maximum(1.0, np.maximum(np.abs(ln_r[pos]), np.maximum(np.abs(np.asarray(f, np.longdouble)[pos]),
                                                                         np.abs(ln_r[pos] - np.asarray(f)[pos]))))
        err = np.abs(lnout[pos] - ln_r[pos]).astype(np.float64)
        tol = bound + 2 * ULP * mag.astype(np.float64)
        assert (err <= tol).all(), ("ln rows", float((err / tol).max()))


def check_pass(got, want, bound):
    """got: fp64 (d or None, s); want: the longdouble pass.  d_n absolute `bound` + one ulp of |d_n|; s relative."""
    if got["d"] is not None:
        d_ref = np.asarray(want["d"], np.longdouble)
        live = np.isfinite(d_ref)
        assert np.array_equal(np.isfinite(got["d"]), live)
        tol_d = bound + ULP * np.abs(d_ref[live]).astype(np.float64)
        err_d = np.abs(np.asarray(got["d"], np.longdouble)[live] - d_ref[live]).astype(np.float64)
        assert (err_d <= tol_d).all(), ("d", float((err_d / tol_d).max()))
    s_ref = np.asarray(want["s"], np.longdouble)
    s = np.asarray(got["s"], np.longdouble)
    big = s_ref > np.finfo(np.float64).tiny
    assert (np.abs(s[~big]) <= 2 * np.finfo(np.float64).tiny).all()
    err_s = (np.abs(s - s_ref)[big] / s_ref[big]).astype(np.float64)
    assert (err_s <= bound).all(), ("s", float(err_s.max() / bound))


# ---- inputs ------------------------------------------------------------------------------------------------------
def problem(counts, u, state, thermo):
    """The solver's inputs from count matrices [K, m, m], u [K, N], Markov and thermodynamic state per frame."""
    C = np.asarray(counts, np.float64)
    K, m = C.shape[0], C.shape[1]
    N = np.zeros((K, m))
    np.add.at(N, (np.asarray(thermo), np.asarray(state)), 1.0)
    prob = {"C": C, "S": C + C.transpose(0, 2, 1), "col": C.sum(axis=1), "N": N, "u": np.asarray(u),
            "state": np.asarray(state, np.int64), "thermo": np.asarray(thermo, np.int64)}
    for a in prob.values():
        a.setflags(write=False)
    return prob


def counts_from_trajs(dtrajs, ttrajs, K, m, lag):
    """Sliding-window counts per ensemble; a pair (t, t + lag) counts in k only inside a stretch of constant ttraj = k
    with valid (>= 0) labels throughout."""
    C = np.zeros((K, m, m))
    for d, t in zip(dtrajs, ttrajs):
        d, t = np.asarray(d), np.asarray(t)
        brk = np.concatenate([[0], np.nonzero((t[1:] != t[:-1]) | (d[1:] < 0) | (d[:-1] < 0))[0] + 1, [d.size]])
        for a, b in zip(brk[:-1], brk[1:]):
            if d[a] >= 0 and b - a > lag:
                np.add.at(C[t[a]], (d[a:b - lag], d[a + lag:b]), 1.0)
    return C


def metropolis_chain(n):
    """A chain on the states with n > 0, nearest neighbours among them, reversible w.r.t. n (zero rows elsewhere)."""
    n = np.asarray(n, np.float64)
    act = np.nonzero(n > 0)[0]
    P = np.zeros((n.size, n.size))
    for a, b in zip(act[:-1], act[1:]):
        P[a, b] = 0.5 * min(1.0, n[b] / n[a])
        P[b, a] = 0.5 * min(1.0, n[a] / n[b])
    P[act, act] = 1.0 - P[act].sum(axis=1)
    return P


@functools.lru_cache(maxsize=None)
def state_only_case():
    """The known answer: u depends on the frame's Markov state only, u[k, n] = ln pi_i - ln n_i^k + c_k, and C^k =
    diag(n^k) P^k with P^k reversible w.r.t. n^k.  The unbiased populations are pi.  One pair is inactive."""
    rng = np.random.default_rng(11)
    pi = rng.dirichlet(np.full(5, 2.0))
    n = np.array([[7, 12, 3, 0, 5], [2, 9, 14, 6, 1], [4, 0, 8, 11, 10]])       # n_i^k; (0, 3) and (2, 1) inactive
    c = np.array([0.3, -1.2, 2.0])
    state = np.concatenate([np.repeat(np.arange(5), n[k]) for k in range(3)])
    thermo = np.repeat(np.arange(3), n.sum(axis=1))
    with np.errstate(divide="ignore"):
        u = np.log(pi)[None, state] - np.log(n.astype(np.float64))[:, state] + c[:, None]
    C = np.stack([n[k][:, None] * metropolis_chain(n[k]) for k in range(3)])
    pi.setflags(write=False)
    return problem(C, u, state, thermo), pi


def double_well(x):
    return 2.0 * (x * x - 1.0) ** 2


@functools.lru_cache(maxsize=None)
def umbrella_case(windows=3, frames=150, bins=6, lag=1, seed=3):
    """Umbrella sampling of a double well by Metropolis chains, one per window, binned into Markov states; bins no
    window visited are dropped.  -> (problem, dtrajs, ttrajs, u blocks, target row [1, N] (the unbiased well))."""
    rng = np.random.default_rng(seed)
    centres = np.linspace(-1.2, 1.2, windows)
    kappa = 6.0
    edges = np.linspace(-1.8, 1.8, bins + 1)
    xs = []
    for c in centres:
        x, traj = c, np.empty(frames)
        for t in range(frames):
            y = x + 0.4 * rng.standard_normal()
            dE = double_well(y) + 0.5 * kappa * (y - c) ** 2 - double_well(x) - 0.5 * kappa * (x - c) ** 2
            if dE <= 0 or rng.random() < np.exp(-dE):
                x = y
            traj[t] = x
        xs.append(traj)
    raw = [np.clip(np.digitize(x, edges) - 1, 0, bins - 1) for x in xs]
    seen = np.unique(np.concatenate(raw))
    relabel = np.full(bins, -1)
    relabel[seen] = np.arange(seen.size)
    dtrajs = [relabel[r] for r in raw]
    ttrajs = [np.full(frames, k) for k in range(windows)]
    ublocks = [double_well(x)[None, :] + 0.5 * kappa * (x[None, :] - centres[:, None]) ** 2 for x in xs]
    C = counts_from_trajs(dtrajs, ttrajs, windows, seen.size, lag)
    prob = problem(C, np.concatenate(ublocks, axis=1), np.concatenate(dtrajs), np.concatenate(ttrajs))
    target = double_well(np.concatenate(xs))[None, :]
    target.setflags(write=False)
    return prob, dtrajs, ttrajs, ublocks, target


@functools.lru_cache(maxsize=None)
def mbar_limit_case():
    """m = 1: TRAM is MBAR.  Three harmonic states; any counts do (they cancel): C^k = [[N_k - 1]]."""
    from tests import _mbar_ref

    u, N_k = _mbar_ref.harmonic(np.random.default_rng(21), np.array([40, 25, 60]))
    thermo = np.repeat(np.arange(3), N_k)
    return problem((N_k - 1.0)[:, None, None], u, np.zeros(u.shape[1], np.int64), thermo), N_k


@functools.lru_cache(maxsize=None)
def msm_limit_case():
    """K = 1, u = 0: TRAM is the reversible maximum-likelihood MSM of the counts of one trajectory."""
    rng = np.random.default_rng(31)
    T = np.array([[0.80, 0.15, 0.05, 0.00], [0.10, 0.70, 0.15, 0.05], [0.05, 0.10, 0.75, 0.10], [0.00, 0.10, 0.20, 0.70]])
    d = np.empty(600, np.int64)
    d[0] = 0
    for t in range(1, d.size):
        d[t] = rng.choice(4, p=T[d[t - 1]])
    C = counts_from_trajs([d], [np.zeros(d.size, np.int64)], 1, 4, 1)
    return problem(C, np.zeros((1, d.size)), d, np.zeros(d.size, np.int64))


SOLVE_CASES = ("umbrella_small", "umbrella", "mbar_limit", "msm_limit", "state_only")
TARGET_CASES = ("umbrella_small", "umbrella", "state_only")          # those with target rows


def solve_case(name):
    """(problem, target rows [T, N] or None) of a named solver input."""
    if name == "umbrella_small":
        c = umbrella_case()
        return c[0], c[4]
    if name == "umbrella":
        c = umbrella_case(4, 500, 12)
        return c[0], c[4]
    if name == "mbar_limit":
        return mbar_limit_case()[0], None
    if name == "msm_limit":
        return msm_limit_case(), None
    prob, _ = state_only_case()
    return prob, np.zeros((1, prob["u"].shape[1]))


@functools.lru_cache(maxsize=None)
def solution(name, tol=1e-10, longdouble=True):
    """The restatement's solve of a named input, in longdouble by default; shared and read-only."""
    r = solve(solve_case(name)[0], tol=tol, dtype=np.longdouble if longdouble else np.float64)
    for key in ("f", "v", "d", "history"):
        r[key].setflags(write=False)
    return r


# fixed-(f, v) inputs of the rows and pass tests: (K, m, frames per Markov state, fill of S)
def synthetic(K, m, frames, seed, *, fill=0.3, inactive=0.2, zero_row=True, scale=1.0, offset=0.0):
    """Random problem at a random (f, v): frames[i] frames in Markov state i (an int: the same for all), drawn from
    random ensembles; a share `inactive` of the pairs without frames (and without counts); with `zero_row`, one active
    state of ensemble 0 has an all-zero S row.  u = offset + scale * N(0, 1) + a state and ensemble dependent shift."""
    rng = np.random.default_rng(seed)
    frames = np.full(m, frames) if np.isscalar(frames) else np.asarray(frames)
    state = np.repeat(np.arange(m), frames)
    allowed = rng.random((K, m)) >= inactive
    allowed[rng.integers(K, size=m), np.arange(m)] = True             # every state is drawn somewhere
    thermo = np.array([rng.choice(np.nonzero(allowed[:, i])[0]) for i in state])
    N = np.zeros((K, m))
    np.add.at(N, (thermo, state), 1.0)
    act = N > 0
    C = rng.integers(1, 9, size=(K, m, m)) * (rng.random((K, m, m)) < fill)
    C = C * act[:, :, None] * act[:, None, :]
    if zero_row and m > 1:
        i0 = int(np.nonzero(act[0])[0][0])
        C[0, i0, :] = 0
        C[0, :, i0] = 0
    C = C.astype(np.float64)
    # keep col_i <= N_i: scale every ensemble's counts down where needed
    colsum = C.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.where(act & (colsum > 0), colsum / np.where(act, N, 1), 0).max(axis=1)
    C = C / np.maximum(worst, 1.0)[:, None, None]
    u = offset + scale * rng.standard_normal((K, state.size)) + rng.standard_normal((K, m))[:, state]
    prob = problem(C, u, state, thermo)
    f = np.where(act, rng.standard_normal((K, m)), 0.0)
    v = np.where(act, prob["S"].sum(axis=2) / 2 * np.exp(0.3 * rng.standard_normal((K, m))), 0.0)
    f.setflags(write=False)
    v.setflags(write=False)
    return prob, f, v


# ---- the fixed-(f, v) inputs of the rows, pass and update tests: the smallest at which each mechanism can fail -----------
CASES = {
    # name: (K, m, frames per Markov state)
    "k1_m1": (1, 1, 5),
    "k2_m1": (2, 1, SEGMENT + 1),
    "k2_m63": (2, 63, 3), "k2_m64": (2, 64, 3), "k2_m65": (2, 65, 3),           # wave edges of a row
    "k3_m130": (3, 130, 2),                                                     # three trips of a row; 98 workgroups
    "k64_m5": (64, 5, 40),                                                      # the limit of K
    "segments": (3, 4, (1, SEGMENT, SEGMENT + 1, 2 * SEGMENT + 88)),            # the unit edges
    "ladder": (8, 4, None),
    "inf": (4, 6, 30),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, f, v) of a named input at a fixed random (f, v); read-only and shared."""
    K, m, frames = CASES[name]
    seed = 2000 + sorted(CASES).index(name)
    if name == "ladder":
        from tests._mbar_ref import ladder_energies

        rng = np.random.default_rng(seed)
        temps = np.linspace(300.0, 330.0, K)
        E, thermo = ladder_energies(rng, temps, 120)
        state = np.digitize(E, np.quantile(E, [0.25, 0.5, 0.75]))
        order = np.argsort(state, kind="stable")
        E, thermo, state = E[order], thermo[order], state[order]
        u = (1.0 / (KB * temps))[:, None] * E[None, :]
        N = np.zeros((K, m))
        np.add.at(N, (thermo, state), 1.0)
        C = np.floor(N[:, :, None] * N[:, None, :] / np.maximum(N.sum(axis=1), 1)[:, None, None] * 0.5)
        prob = problem(C, u, state, thermo)
        f = np.where(N > 0, rng.standard_normal((K, m)), 0.0)
        v = np.where(N > 0, prob["S"].sum(axis=2) / 2 * np.exp(0.3 * rng.standard_normal((K, m))), 0.0)
        return prob, f, v
    prob, f, v = synthetic(K, m, frames, seed, inactive=0.0 if name in ("k1_m1", "k2_m1") else 0.2)
    if name == "inf":                     # a third of the frames are forbidden in an ensemble that did not draw them
        u = prob["u"].copy()
        n = np.arange(u.shape[1])
        k = (prob["thermo"] + 1 + n % (K - 1)) % K
        u[k[::3], n[::3]] = np.inf
        prob = problem(prob["C"], u, prob["state"], prob["thermo"])
    return prob, f, v


def offsets(prob):
    return np.concatenate([[0], np.cumsum(np.bincount(prob["state"], minlength=prob["N"].shape[1]))])


@functools.lru_cache(maxsize=None)
def host_tab(name, f32=False):
    """The fp64 table ln R + f both the device pass and its yardstick are given, and the longdouble pass at it."""
    prob, f, v = case(name)
    g = log_multipliers(f, v)
    _, g1 = rows(prob["S"], g, f, prob["N"], prob["col"], "multipliers")
    _, tab = rows(prob["S"], g1, f, prob["N"], prob["col"], "counts")
    u = prob["u"].astype(np.float32).astype(np.float64) if f32 else prob["u"]
    return tab, frame_pass(u, prob["state"], tab, tab.shape[1], np.longdouble), u
