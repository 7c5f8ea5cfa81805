"""The OPES law in numpy: host-only companion of tests/test_opes_reference.py, tests/test_gpu_opes.py and
tests/test_gpu_opes_paths.py.  No product code, no device code.

Restated here as include/msmhip.h states it for msm_opes_deposit and msm_opes_bias; `dtype` is the arithmetic (float64,
or longdouble: the yardstick the device is held to).  The constants epsilon, cutoff^2, v = exp(-cutoff^2 / 2) and
threshold^2 are constants of the law, formed in fp64 and handed to either arithmetic as the fp64 numbers they are.

    G(s; c, sigma, h) = h (exp(-q / 2) - v) where q = sum_i (dp_i / sigma_i)^2 < cutoff^2, else 0
    P(s) = sum_live G(s) / W,  V(s) = kT p log(P(s) / Z + eps);  no deposit yet: V = kT p log(eps)

`replay` runs a deposit sequence one deposit at a time: the incoming kernel merges into its nearest live kernel (by that
kernel's own sigma, lowest slot on a tie) while the distance is below the threshold, the merged kernel keeps the
taker's slot and is tested again; a chain merge keeps the lower slot and the last live slot fills the higher.  The sum
S = sum_k sum_k' G_k'(c_k) loses the pairs of every kernel removed and gains those of the kernel added; Z = S / (W K).
It also records what the GPU tests rely on: the length of every merge chain, the merges across a periodic boundary and
the relative margin of every merge decision and nearest-neighbour choice."""

from __future__ import annotations

import numpy as np

EPS = float(np.finfo(np.float64).eps)
ALIVE = 2**31 - 1


class Params:
    def __init__(self, d, kT, barrier, biasfactor=None, periods=None, sigma0=None, cutoff=None, threshold=1.0,
                 epsilon=None, fixed_sigma=False):
        self.d, self.kT = int(d), float(kT)
        gamma = float(barrier) / self.kT if biasfactor is None else float(biasfactor)
        self.gamma = gamma
        self.p = 1.0 if np.isinf(gamma) else 1.0 - 1.0 / gamma
        self.eps = float(np.exp(-float(barrier) / (self.kT * self.p))) if epsilon is None else float(epsilon)
        self.cutoff = float(np.sqrt(2.0 * float(barrier) / (self.kT * self.p))) if cutoff is None else float(cutoff)
        self.cut2 = self.cutoff * self.cutoff
        self.v = float(np.exp(-0.5 * self.cut2))
        self.threshold = float(threshold)
        self.thr2 = self.threshold * self.threshold
        self.periods = np.zeros(self.d) if periods is None else np.asarray(periods, np.float64).reshape(self.d)
        self.sigma0 = None if sigma0 is None else np.broadcast_to(np.asarray(sigma0, np.float64), (self.d,)).copy()
        self.fixed_sigma = bool(fixed_sigma)
        self.kTp = self.kT * self.p


def min_image(a, b, periods, t):
    """a - b, brought to the minimum image on periodic axes: dp -= P rint(dp / P)."""
    dp = np.asarray(a, t) - np.asarray(b, t)
    for i, P in enumerate(periods):
        if P > 0:
            dp[..., i] = dp[..., i] - t(P) * np.rint(dp[..., i] / t(P))
    return dp


def kernel_values(s, c, sg, h, par, t, grad=False):
    """G_k(s) [K] of the kernels (c [K, d], sg [K, d], h [K]) at the point s [d]; with grad also dG_k / ds [K, d]."""
    dp = min_image(np.asarray(s, t)[None, :], c, par.periods, t)
    z = dp / sg
    q = (z * z).sum(axis=1) if z.shape[1] == 1 else np.add.reduce(z * z, axis=1)
    inside = q < t(par.cut2)
    e = np.exp(-t(0.5) * np.where(inside, q, t(0)))
    G = np.where(inside, h * (e - t(par.v)), t(0))
    if not grad:
        return G
    dG = np.where(inside[:, None], -(h * e)[:, None] * (z / sg), t(0))
    return G, dG


def value(acc, W, Z, par, t):
    x = (acc / W) / Z + t(par.eps)
    return t(par.kTp) * np.log(x), x


class Run:
    """The outcome of `replay`: journal (centre, sigma, height per version), death [T] (ALIVE while living), the
    per-deposit W, Z, neff, K, the live kernels with their versions, the deposit records, and the events."""


def replay(par: Params, centers, sigmas=None, heights=None, logweights=None, dtype=np.longdouble) -> Run:
    """Replays T deposits.  With sigmas / heights / logweights None the deposits are made on line at `centers`:
    logweight = V(s) / kT, w = h = exp(logweight), sigma from sigma0 (rescaled by neff unless fixed_sigma)."""
    t = np.dtype(dtype).type
    cen = np.asarray(centers, np.float64)
    T, d = cen.shape
    online = heights is None
    live_c, live_s, live_h, live_v = [], [], [], []
    W, W2, S, Z = t(0), t(0), t(0), t(1)
    run = Run()
    run.journal = np.zeros((T, 2 * d + 1), t)
    run.death = np.full(T, ALIVE, np.int64)
    run.W, run.Z, run.neff = np.zeros(T, t), np.zeros(T, t), np.zeros(T, t)
    run.K = np.zeros(T, np.int64)
    run.records = np.zeros((T, 2 * d + 2), t)
    run.chain, run.periodic_merges, run.margins = np.zeros(T, np.int64), 0, []

    def pairs(xc, xs, xh, hole):
        """sum over the live slots k != hole of G_x(c_k) + G_k(c_x), one minimum image for both directions"""
        keep = [k for k in range(len(live_h)) if k != hole]
        if not keep:
            return t(0)
        c, sg, h = np.stack([live_c[k] for k in keep]), np.stack([live_s[k] for k in keep]), np.asarray([live_h[k] for k in keep], t)
        dp = min_image(xc[None, :], c, par.periods, t)
        qx, qk = ((dp / xs[None, :]) ** 2).sum(axis=1), ((dp / sg) ** 2).sum(axis=1)
        gx = np.where(qx < t(par.cut2), xh * (np.exp(-t(0.5) * qx) - t(par.v)), t(0))
        gk = np.where(qk < t(par.cut2), h * (np.exp(-t(0.5) * qk) - t(par.v)), t(0))
        return (gx + gk).sum()

    for j in range(T):
        c = cen[j].astype(t)
        if online:
            V = t(par.kTp) * np.log(t(par.eps))
            if live_h:
                G = kernel_values(c, np.stack(live_c), np.stack(live_s), np.asarray(live_h, t), par, t)
                V = value(G.sum(), W, Z, par, t)[0]
            lw = V / t(par.kT)
            h = np.exp(lw)
            sg = par.sigma0.astype(t)
        else:
            sg, h, lw = np.asarray(sigmas[j], np.float64).astype(t), t(heights[j]), t(logweights[j])
        w = np.exp(lw)
        W, W2 = W + w, W2 + w * w
        neff = ((t(1) + W) * (t(1) + W)) / (t(1) + W2)
        if online and not par.fixed_sigma:
            f = (neff * t(d + 2) / t(4)) ** (-t(1) / t(d + 4))
            sg = par.sigma0.astype(t) * f
            for i in range(d):
                h = h * (t(par.sigma0[i]) / sg[i])
        run.records[j] = np.concatenate([c, sg, [h, lw]])
        home = -1
        for _it in range(len(live_h) + 1):
            others = [k for k in range(len(live_h)) if k != home]
            if not others:
                break
            dp = min_image(c[None, :], np.stack([live_c[k] for k in others]), par.periods, t)
            q = ((dp / np.stack([live_s[k] for k in others])) ** 2).sum(axis=1)
            order = np.argsort(q, kind="stable")
            best = order[0]
            if order.size > 1:
                run.margins.append(float((q[order[1]] - q[best]) / max(q[order[1]], t(np.finfo(np.float64).tiny))))
            if par.thr2 > 0:
                run.margins.append(float(abs(q[best] - t(par.thr2)) / t(par.thr2)))
            if not q[best] < t(par.thr2):
                break
            k = others[best]
            tc, ts, th = live_c[k], live_s[k], live_h[k]
            S = S - (pairs(tc, ts, th, home) - th * (t(1) - t(par.v)))
            run.death[live_v[k]] = j
            run.chain[j] += 1
            raw = c - tc
            dl = min_image(c, tc, par.periods, t)
            if np.any(raw != dl):
                run.periodic_merges += 1
            hm = th + h
            s2 = (th * (ts * ts) + h * (sg * sg)) / hm + ((th * h) / (hm * hm)) * (dl * dl)
            c, sg, h = tc + (h / hm) * dl, np.sqrt(s2), hm
            if home < 0:
                home = k
            else:
                freed, last = max(home, k), len(live_h) - 1
                home = min(home, k)
                if freed != last:
                    live_c[freed], live_s[freed], live_h[freed], live_v[freed] = live_c[last], live_s[last], live_h[last], live_v[last]
                for lst in (live_c, live_s, live_h, live_v):
                    lst.pop()
        if home < 0:
            live_c.append(c), live_s.append(sg), live_h.append(h), live_v.append(j)
        else:
            live_c[home], live_s[home], live_h[home], live_v[home] = c, sg, h, j
        S = S + (pairs(c, sg, h, -1) - h * (t(1) - t(par.v)))
        K = len(live_h)
        Z = S / (W * t(K))
        run.journal[j] = np.concatenate([c, sg, [h]])
        run.W[j], run.Z[j], run.neff[j], run.K[j] = W, Z, neff, K
    run.live = np.concatenate([np.stack(live_c), np.stack(live_s), np.asarray(live_h, t)[:, None]], axis=1) if live_h \
        else np.zeros((0, 2 * d + 1), t)
    run.live_version = np.asarray(live_v, np.int64)
    run.S = S
    return run


def full_z(run: Run, par: Params, c: int | None = None, dtype=np.longdouble):
    """Z after c deposits (None: all) by the full double sum over the live versions of the journal."""
    t = np.dtype(dtype).type
    T = run.journal.shape[0]
    c = T if c is None else c
    d = (run.journal.shape[1] - 1) // 2
    alive = np.nonzero((np.arange(T) < c) & (run.death >= c))[0]
    J = run.journal[alive].astype(t)
    total = t(0)
    for k in range(alive.size):
        total = total + kernel_values(J[k, :d], J[:, :d], J[:, d:2 * d], J[:, 2 * d], par, t).sum()
    return total / (run.W[c - 1].astype(t) * t(alive.size))


def bias(run: Run, par: Params, cv, counts=None, dtype=np.longdouble, journal=None, death=None, W=None, Z=None):
    """{"bias" [n], "grad" [n, d], "mag" [n] = P / Z (the sum behind the logarithm)} of the frames cv [n, d]; frame f
    sees the versions j < counts[f] <= death_j and W, Z of deposit counts[f] - 1 (None: all deposits).  A frame with a
    non-finite CV is NaN.  `journal`, `death`, `W`, `Z` replace the run's own (the device's, to test a stage alone)."""
    t = np.dtype(dtype).type
    journal = run.journal if journal is None else journal
    death = run.death if death is None else death
    W = run.W if W is None else W
    Z = run.Z if Z is None else Z
    T = journal.shape[0]
    d = (journal.shape[1] - 1) // 2
    cv = np.asarray(cv, np.float64).reshape(-1, d)
    n = cv.shape[0]
    counts = np.full(n, T, np.int64) if counts is None else np.clip(np.asarray(counts, np.int64), 0, T)
    V, g, mag = np.zeros(n, t), np.zeros((n, d), t), np.zeros(n, t)
    J = np.asarray(journal).astype(t)
    for f in range(n):
        if not np.isfinite(cv[f]).all():
            V[f], g[f] = np.nan, np.nan
            continue
        c = counts[f]
        if c == 0:
            V[f] = t(par.kTp) * np.log(t(par.eps))
            continue
        alive = np.nonzero((np.arange(T) < c) & (np.asarray(death) >= c))[0]
        G, dG = kernel_values(cv[f].astype(t), J[alive, :d], J[alive, d:2 * d], J[alive, 2 * d], par, t, grad=True)
        Wc, Zc = t(W[c - 1]), t(Z[c - 1])
        V[f], x = value(G.sum(), Wc, Zc, par, t)
        mag[f] = (G.sum() / Wc) / Zc
        g[f] = t(par.kTp) * (((dG.sum(axis=0) / Wc) / Zc) / x)
    return {"bias": V, "grad": g, "mag": mag, "count": counts}


def counts_from_times(kernel_times, frame_times) -> np.ndarray:
    """A frame sees the deposits made strictly before its time."""
    return np.searchsorted(np.asarray(kernel_times, np.float64), np.asarray(frame_times, np.float64), side="left").astype(np.int32)


def normalise(logw):
    m = logw.max()
    lw = logw - (m + np.log(np.exp(logw - m).sum()))
    w = np.exp(lw)
    return w, lw, float(1.0 / np.sum(w * w))


def trajectory(seed: int, T: int, d: int, periodic: bool):
    """The committed deposit sequence of the tests: a slow random walk (so that neighbouring deposits merge, in chains
    where the walk turns back) that crosses the periodic boundary of axis 0 when `periodic`."""
    rng = np.random.default_rng(seed)
    P = 2.0 * np.pi
    step = rng.normal(scale=0.22 / np.sqrt(d), size=(T, d))
    x = np.cumsum(step, axis=0) + (np.pi - 0.3 if periodic else 0.0)
    periods = np.zeros(d)
    if periodic:
        periods[0] = P
        x[:, 0] = (x[:, 0] + np.pi) % P - np.pi
    return x, periods


# ---- the committed cases of the GPU tests ------------------------------------------------------------------------------
SEED, T_DEPOSITS, KT, BARRIER, SIGMA0 = 3, 300, 1.0, 10.0, 0.25
DIMS = (1, 2, 3, 8)
_CASES: dict = {}


def case(d: int, periodic: bool):
    """(centres [T, d], Params, records [T, 2 d + 2] fp64, the 80-bit replay of those records), computed once.  The
    records are those of an on-line run (widths shrinking with neff) made in fp64: a KERNELS file in all but name."""
    key = (d, bool(periodic))
    if key not in _CASES:
        x, periods = trajectory(SEED, T_DEPOSITS, d, periodic)
        par = Params(d, KT, BARRIER, periods=periods, sigma0=np.full(d, SIGMA0))
        rec = np.ascontiguousarray(replay(par, x, dtype=np.float64).records, np.float64)
        run = replay(par, rec[:, :d], rec[:, d:2 * d], rec[:, 2 * d], rec[:, 2 * d + 1], dtype=np.longdouble)
        _CASES[key] = (x, par, rec, run)
    return _CASES[key]


def online_case():
    """(centres, Params, the 80-bit ON-LINE run with shrinking widths) of the d = 2 periodic sequence, computed once:
    what tests/test_gpu_opes.py holds the device's on-line deposits to."""
    if "online" not in _CASES:
        x, par, _rec, _run = case(2, True)
        _CASES["online"] = (x, par, replay(par, x, dtype=np.longdouble))
    return _CASES["online"]


def frames(d: int, periodic: bool, n: int, seed: int = 11):
    """(cv [n, d], times [n]): frames near the walker's position at their own times; deposit j is made at time j."""
    x, _par, _rec, _run = case(d, periodic)
    rng = np.random.default_rng(seed + 7 * d + n)
    times = np.sort(rng.uniform(-1.0, T_DEPOSITS + 1.0, size=n))
    times[: min(n, 3)] = [0.0, 17.0, float(T_DEPOSITS)][: min(n, 3)]      # exactly at a deposit's time, and after all
    at = np.clip(np.floor(times).astype(np.int64), 0, T_DEPOSITS - 1)
    cv = x[at] + rng.normal(scale=0.1, size=(n, d))
    return cv, times
