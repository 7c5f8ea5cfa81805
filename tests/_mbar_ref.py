"""numpy restatement of the MBAR contract (include/msmhip.h, "MBAR frame weights"; Shirts & Chodera 2008): the pass,
the solver on exactly the prescribed path, the target weights; the inputs the CPU and GPU tests share; the rounding
bound both hold results to.

The pass takes a `dtype`: np.float64 is the restatement proper, np.longdouble (80-bit on x86, eps 1.1e-19) the
near-exact yardstick the device is compared with.
"""
from __future__ import annotations

import functools

import numpy as np

ULP = 2.0 ** -52
KB = 0.00831446261815324       # kJ / mol / K, the constant the package uses for kT
TRIP = 256                     # frames of a workgroup trip (MSM_MBAR_THREADS); the GPU tests check it against mbar_plan
ARMIJO = 1e-4
MIN_STEP = 2.0 ** -20
SLACK_ULPS = 64.0


def mbar_pass(u, N_k, f, dtype=np.float64, want_gram=True):
    """One pass at free energies f over u [K, N] -> dict(d [N], W [K, N], s [K], G [K, K] or None, obj, status)."""
    u = np.asarray(u).astype(dtype)
    N_k = np.asarray(N_k)
    f = np.asarray(f).astype(dtype)
    status = 0
    if np.isnan(u).any() or np.isneginf(u).any():
        status |= 1
    lnN = np.log(N_k.astype(dtype))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = u.min(axis=0)                                  # the per-frame shift
        b = (f[:, None] - (u - m[None, :])) + lnN[:, None]
        M = np.nanmax(np.where(np.isnan(b), -np.inf, b), axis=0)
        e = np.exp(b - M[None, :])
        S = e.sum(axis=0)
        d = (M + np.log(S)) - m
        W = e / (N_k.astype(dtype)[:, None] * S[None, :])
    dead = ~np.isfinite(d)
    if dead.any():
        status |= 2
        W[:, dead] = 0
    return {"d": d, "W": W, "s": W.sum(axis=1), "G": W @ W.T if want_gram else None,
            "obj": d[~dead].sum(), "status": status}


def state_offsets(N_k):
    return np.concatenate([[0], np.cumsum(np.asarray(N_k, np.int64))])


def initial_guess(u, N_k):
    """f_k = mean of u_kn over state k's own frames (frames are grouped by state), minus the value for state 0."""
    off = state_offsets(N_k)
    mean = np.array([np.asarray(u[k, off[k]:off[k + 1]], np.float64).mean() for k in range(len(N_k))])
    return mean - mean[0]


class NotConverged(RuntimeError):
    pass


def armijo_ok(phi_try, phi0, alpha, slope, scale):
    """Phi(f - alpha x) <= Phi(f) - 1e-4 alpha g.x, up to SLACK_ULPS ulp of the magnitudes Phi is summed from."""
    return phi_try <= phi0 - ARMIJO * alpha * slope + SLACK_ULPS * ULP * scale


def solve(u, N_k, tol=1e-10, maxiter=100, pass_fn=None, newton_fn=None, f0=None):
    """The prescribed path.  pass_fn(f, want_gram) -> (s, G, obj) and newton_fn(s, G) -> x let another implementation
    of the two device steps run under the same driver; the defaults are the fp64 restatement.
    Returns dict(f, n_iterations, n_passes, residual)."""
    N_k = np.asarray(N_k, np.float64)
    K, N = N_k.size, float(N_k.sum())

    if pass_fn is None:
        def pass_fn(f, want_gram):
            r = mbar_pass(u, N_k, f, np.float64, want_gram)
            return r["s"], r["G"], float(r["obj"])
    if newton_fn is None:
        def newton_fn(s, G):
            H = np.diag(N_k * s) - np.outer(N_k, N_k) * G
            return np.linalg.solve(H[1:, 1:], (N_k * (s - 1.0))[1:])

    f = np.array(initial_guess(u, N_k) if f0 is None else f0, np.float64)
    it, passes = 0, 1
    s, G, obj = pass_fn(f, False)
    while True:
        g = N_k * (s - 1.0)
        residual = float(np.abs(g).max() / N)
        if residual <= tol:
            return {"f": f, "n_iterations": it, "n_passes": passes, "residual": residual}
        if it >= maxiter:
            raise NotConverged(f"mbar: residual {residual:.3e} > tol {tol:.1e} after {it} iterations")
        it += 1
        if it <= 2:                                        # self-consistent step, re-gauged
            f = f - np.log(s)
            f = f - f[0]
            s, G, obj = pass_fn(f, it >= 2)
            passes += 1
            continue
        if K < 2:
            raise NotConverged("mbar: a single state did not converge")
        x = newton_fn(s, G)
        slope = float(np.dot(g[1:], x))
        phi0 = obj - float(np.dot(N_k, f))
        scale = abs(obj) + float(np.dot(N_k, np.abs(f)))
        alpha = 1.0
        while True:
            trial = f.copy()
            trial[1:] -= alpha * x
            first = alpha == 1.0                           # the full step carries the Gram matrix: it is the next pass
            s_t, G_t, obj_t = pass_fn(trial, first)
            passes += 1
            if armijo_ok(obj_t - float(np.dot(N_k, trial)), phi0, alpha, slope, scale):
                break
            alpha *= 0.5
            if alpha < MIN_STEP:
                raise NotConverged("mbar: the line search failed (step below 2^-20)")
        f = trial
        if first:
            s, G, obj = s_t, G_t, obj_t
        else:
            s, G, obj = pass_fn(f, True)
            passes += 1


def target_weights(ut, d, dtype=np.float64):
    """Rows of ut [T, N] against the log denominators d [N] -> (f_t [T], w [T, N], ess [T])."""
    ut = np.asarray(ut).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = -ut - np.asarray(d).astype(dtype)[None, :]
        mx = c.max(axis=1)
        lse = mx + np.log(np.exp(c - mx[:, None]).sum(axis=1))
        w = np.exp(c - lse[:, None])
    return -lse, w, 1.0 / (w * w).sum(axis=1)


# ---- the rounding bound ------------------------------------------------------------------------------------------
# An exponent argument after the per-frame shift is b_k - M with b_k = (f_k - (u_kn - m_n)) + ln N_k.  The inner
# difference is exact when u_kn and m_n lie within a factor 2 of each other (Sterbenz), as they do on a ladder at
# large |u|; otherwise it rounds at |u_kn - m_n|.  The outer difference and the sum round at their results, which
# are the argument up to ln N_k.  So with A = max(1, |b_k| over the finite entries, |u_kn - m_n| where that difference
# is not exact) the absolute error of an argument is a few 2^-52 A; exp turns it into the same relative error of e_k,
# and exp / log themselves are good to 1 ulp (the device math library documents 1 ulp for both in fp64).
# Per output the operations that add such an error are the K terms of the logsumexp, the ceil(log2 N) levels of the
# sum over frames (the device adds 16-term chains, then trips, waves and workgroups: at the shapes tested the chains
# beyond the first are shorter than log2 N), and a fixed number around them (the roundings of b, b - M, M + log S,
# the final subtraction, 1 / S, two products, exp and log at one ulp each, the 16-term chain): FIXED = 32 covers
# those.
FIXED_OPS = 32


def n_ops(K, N):
    return K + int(np.ceil(np.log2(max(N, 1)))) + FIXED_OPS


def arg_magnitude(u, N_k, f):
    u, f = np.asarray(u, np.float64), np.asarray(f, np.float64)
    m = u.min(axis=0)[None, :]
    with np.errstate(invalid="ignore"):
        sh = u - m
        b = np.abs((f[:, None] - sh) + np.log(np.asarray(N_k, np.float64))[:, None])
        lo, hi = np.minimum(np.abs(u), np.abs(m)), np.maximum(np.abs(u), np.abs(m))
        exact = (np.sign(u) == np.sign(m)) & (hi <= 2 * lo)                    # Sterbenz
    b = b[np.isfinite(b)]
    rounded = sh[np.isfinite(sh) & ~exact]
    return max(1.0, float(b.max()) if b.size else 0.0, float(rounded.max()) if rounded.size else 0.0)


def pass_bound(u, N_k, f):
    """Relative bound for s and G, absolute bound for d_n - (M + log S) parts: n_ops * 2^-52 * A."""
    K, N = np.asarray(u).shape
    return n_ops(K, N) * ULP * arg_magnitude(u, N_k, f)


def check_pass(got, want, bound, K):
    """got: fp64 results (dict with d, s, G or None, obj); want: the longdouble pass of the same inputs.
    d_n: absolute `bound` plus one ulp of |d_n| (the subtraction of m_n and the stored fp64 number).
    s, G: relative `bound` (G doubles it: a product of two W).  obj: absolute, sum of the d_n bounds plus
    n_ops ulp of sum |d_n| for the summation itself."""
    d_ref = np.asarray(want["d"], np.longdouble)
    tol_d = bound + ULP * np.abs(d_ref).astype(np.float64)
    err_d = np.abs(np.asarray(got["d"], np.longdouble) - d_ref).astype(np.float64)
    assert (err_d <= tol_d).all(), ("d", float((err_d / tol_d).max()))
    s_ref = np.asarray(want["s"], np.longdouble)
    err_s = (np.abs(np.asarray(got["s"], np.longdouble) - s_ref) / s_ref).astype(np.float64)
    assert (err_s <= bound).all(), ("s", float(err_s.max() / bound))
    if got["G"] is not None:
        G_ref = np.asarray(want["G"], np.longdouble)
        # sums of positive products: the error is relative to the entry; entries below the smallest normal are skipped
        big = G_ref > np.finfo(np.float64).tiny
        err_G = (np.abs(np.asarray(got["G"], np.longdouble) - G_ref)[big] / G_ref[big]).astype(np.float64)
        assert (err_G <= 2 * bound).all(), ("G", float(err_G.max() / (2 * bound)))
    sum_abs = float(np.abs(d_ref).sum())
    N = d_ref.size
    tol_obj = float(tol_d.sum()) + n_ops(K, N) * ULP * sum_abs
    err_obj = abs(float(np.longdouble(got["obj"]) - np.longdouble(want["obj"])))
    assert err_obj <= tol_obj, ("obj", err_obj / tol_obj)


def target_bound(u, N_k, f, ut, d):
    """The exponent argument of a target weight is c_n - lse, c_n = -u_tn - d_n.  Its absolute error: that of the
    stored d_n (pass_bound plus one ulp of |d_n|), one rounding of the difference of two numbers up to
    max(|u_tn|, |d_n|), and the logsumexp over N frames, n_ops(1, N) operations on arguments up to
    max(1, |c_n - lse|)."""
    ut, d = np.asarray(ut, np.float64), np.asarray(d, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = -ut - d[None, :]
        lse = np.log(np.exp(c - c.max(axis=1)[:, None]).sum(axis=1)) + c.max(axis=1)
        arg = np.abs(c - lse[:, None])
    mag = max(float(np.abs(d).max()), float(np.abs(ut[np.isfinite(ut)]).max()))
    arg = max(1.0, float(arg[np.isfinite(arg)].max()))
    return pass_bound(u, N_k, f) + 2 * ULP * mag + n_ops(1, d.size) * ULP * arg


def check_targets(got, want, bound):
    """(f_t, w, ess) in fp64 against the longdouble evaluation: w relative (exp turns the argument's absolute error
    into a relative one), f_t absolute plus one ulp of itself, ess relative at twice the bound (squares)."""
    ft, w, ess = (np.asarray(a, np.longdouble) for a in got)
    ft_r, w_r, ess_r = (np.asarray(a, np.longdouble) for a in want)
    big = w_r > np.finfo(np.float64).tiny
    err_w = (np.abs(w - w_r)[big] / w_r[big]).astype(np.float64)
    assert (err_w <= bound).all(), ("w", float(err_w.max() / bound))
    assert (np.abs(w[~big]) <= np.finfo(np.float64).tiny * 2).all()
    err_f = np.abs(ft - ft_r).astype(np.float64)
    assert (err_f <= bound + ULP * np.abs(ft_r).astype(np.float64)).all(), ("f_t", float(err_f.max() / bound))
    err_e = (np.abs(ess - ess_r) / ess_r).astype(np.float64)
    assert (err_e <= 2 * bound).all(), ("ess", float(err_e.max() / (2 * bound)))


# ---- inputs ------------------------------------------------------------------------------------------------------
def harmonic(rng, N_k, spacing=0.5, kappa=None):
    """K harmonic states u_k(x) = kappa_k (x - c_k)^2 / 2 on a line; N_k[k] frames drawn from state k, grouped."""
    N_k = np.asarray(N_k, np.int64)
    K = N_k.size
    c = spacing * np.arange(K)
    kappa = np.full(K, 4.0) if kappa is None else np.asarray(kappa, np.float64)
    x = np.concatenate([c[k] + rng.standard_normal(N_k[k]) / np.sqrt(kappa[k]) for k in range(K)])
    return 0.5 * kappa[:, None] * (x[None, :] - c[:, None]) ** 2, N_k


def ladder_energies(rng, temperatures, n_per, offset=-4.0e4, cv=10.0):
    """One potential energy per frame of a replica ladder: E ~ N(offset + cv (T - T_0), k_B T^2 cv), grouped by rung."""
    T = np.asarray(temperatures, np.float64)
    E = np.concatenate([offset + cv * (t - T[0]) + np.sqrt(KB * t * t * cv) * rng.standard_normal(n_per) for t in T])
    return E, np.repeat(np.arange(T.size), n_per)


def ladder(rng, n_rungs=8, n_per=120):
    T = np.linspace(300.0, 330.0, n_rungs)
    E, _ = ladder_energies(rng, T, n_per)
    return (1.0 / (KB * T))[:, None] * E[None, :], np.full(n_rungs, n_per, np.int64)


def spread(N, K):
    """N frames over K states, as evenly as integers allow."""
    return np.array([N // K + (1 if k < N % K else 0) for k in range(K)], np.int64)


CASES = {
    # name: (K, N or N_k, max_workgroups); the smallest shapes at which each mechanism can fail
    "k1_n1": (1, 1, 0), "k1_n5": (1, 5, 0),
    "k2_n63": (2, 63, 0), "k2_n64": (2, 64, 0), "k2_n65": (2, 65, 0),                 # wave edges
    "k16_n257": (16, 257, 0), "k17_n257": (17, 257, 0),                               # Gram tile edge
    "k64_n1000": (64, 1000, 0),                                                       # the limit
    "two_wg": (3, TRIP + 1, 0),                                                       # one trip + 1: two workgroups
    "stride": (3, 5 * TRIP + 3, 2),                                                   # grid-stride loop, ragged tail
    "unequal": (5, (300, 1, 57, 120, 33), 0),                                         # a state with a single frame
    "ladder": (8, 8 * 120, 0),                                                        # large magnitudes
    "inf": (4, 150, 0),                                                               # +inf entries in some states
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(u [K, N] f64, N_k, max_workgroups) of a named input; read-only and shared."""
    K, shape, max_wg = CASES[name]
    rng = np.random.default_rng(1000 + sorted(CASES).index(name))
    if name == "ladder":
        u, N_k = ladder(rng)
    else:
        N_k = np.asarray(shape, np.int64) if isinstance(shape, tuple) else spread(shape, K)
        u, N_k = harmonic(rng, N_k, spacing=0.2 if K > 8 else 0.5)
    if name == "inf":                # states 2 and 3 forbid a third of the other states' frames
        off = state_offsets(N_k)
        u = u.copy()
        u[2, off[0]:off[1]:3] = np.inf
        u[3, off[1] + 1:off[2]:3] = np.inf
        u[2, off[3]::3] = np.inf
    u.setflags(write=False)
    N_k.setflags(write=False)
    return u, N_k, max_wg


@functools.lru_cache(maxsize=None)
def solution(name, f32=False):
    """The restatement's solve of a named input (of its fp32-rounded values with f32)."""
    u, N_k, _ = case(name)
    r = solve(u.astype(np.float32).astype(np.float64) if f32 else u, N_k)
    r["f"].setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def fixed_f(name, f32=False):
    """The f the pass tests run at: the solution perturbed by a seeded 1e-3, so that s != 1."""
    f = solution(name, f32)["f"]
    rng = np.random.default_rng(7)
    out = f + 1e-3 * rng.standard_normal(f.size)
    out.setflags(write=False)
    return out


F32_CASES = ("unequal", "k17_n257", "ladder")
SOLVER_CASES = ("ladder", "unequal", "k64_n1000")


def targets(name):
    """Two unsampled target rows for a named input: between the first two states, and beyond the last."""
    u, N_k, _ = case(name)
    if name == "ladder":
        E = u[0] * (KB * 300.0)
        return np.stack([E / (KB * 302.0), E / (KB * 333.0)])
    return np.stack([0.5 * (u[0] + u[min(1, u.shape[0] - 1)]), 1.1 * u[-1]])
