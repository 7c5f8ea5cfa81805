"""Restatement of the effective-count contract (include/msmhip.h, msm_effective_counts) in numpy and Python ints.

Two forms of the statistical inefficiency of every cell:

* `dense_inefficiencies`: the literal float loop of the documented algorithm (mean-removed indicator series,
  autocovariance per lag over the sub-sequences, truncation at the first non-positive value decided in floating
  point, as deeptime 0.4.5 does);
* `position_inefficiencies`: the exact form the device computes.  Per cell only the positions of its occurrences
  are used: S_l = occurrence pairs of one sub-sequence at rank distance l, A_l / B_l = occurrences with tail / head
  distance >= l, Q_l = S_l N^2 - c N (A_l + B_l) + c^2 n_l in Python ints; the sign of Q_l decides the truncation,
  and every summand Q_l (M - l) / (N^2 n_l M) is one correctly rounded quotient of two integers, added by
  math.fsum.  It also reports the truncation lags.

Neither is deeptime's code; parity with deeptime's own numbers is not pinned anywhere."""

from __future__ import annotations

import math

import numpy as np


def sticky_chain(rng, n, k, stay):
    """n labels in [0, k): the previous label with probability `stay`, else a uniform one."""
    out = np.empty(n, np.int64)
    out[0] = rng.integers(k)
    jump = rng.random(n) >= stay
    new = rng.integers(k, size=n)
    for t in range(1, n):
        out[t] = new[t] if jump[t] else out[t - 1]
    return out


def regime_chain(rng, n, switch):
    """n labels in [0, 4) driven by a hidden two-regime switch (probability `switch` per step): state 0 goes to 1 in
    one regime and to 2 in the other; every other state goes to 0 or 3 with equal odds.  The targets of row 0 come
    in runs about 1 / switch frames long, so its cells have a long autocorrelation."""
    out = np.empty(n, np.int64)
    flip = rng.random(n) < switch
    coin = rng.random(n) < 0.5
    state, regime = 0, 0
    for t in range(n):
        out[t] = state
        regime ^= int(flip[t])
        state = (1 + regime) if state == 0 else (0 if coin[t] else 3)
    return out


def split_valid(dtrajs, k):
    """The trajectories cut at labels outside [0, k): a list of int arrays (what _concat_dtrajs' segments are)."""
    out = []
    for d in dtrajs:
        a = np.asarray(d).astype(np.int64)
        if a.size == 0:
            continue
        ok = (a >= 0) & (a < k)
        edges = np.flatnonzero(np.diff(np.concatenate([[0], ok.astype(np.int8), [0]])))
        out += [a[s:e] for s, e in zip(edges[::2], edges[1::2])]
    return out


def sliding_counts(trajs, k, lag):
    C = np.zeros((k, k), np.int64)
    for a in trajs:
        if a.size > lag:
            np.add.at(C, (a[:-lag], a[lag:]), 1)
    return C


def rows_of(trajs, k, lag):
    """rows[i] = list of target arrays, one per trajectory that starts in i at least once (time order)."""
    rows = [[] for _ in range(k)]
    for a in trajs:
        if a.size <= lag:
            continue
        src, dst = a[:-lag], a[lag:]
        for i in np.unique(src):
            rows[int(i)].append(dst[src == i])
    return rows


def dense_inefficiencies(trajs, k, lag, mact=1.0):
    """si f64 [k, k] by the literal float loop (0 where C = 0)."""
    C = sliding_counts(trajs, k, lag)
    rows = rows_of(trajs, k, lag)
    si = np.zeros((k, k))
    for i in range(k):
        for j in np.flatnonzero(C[i]):
            X = [(t == j).astype(np.float64) for t in rows[i]]
            flat = np.concatenate(X)
            mean, x2m = flat.mean(), (flat ** 2).mean()
            X0 = [x - mean for x in X]
            M = max(len(x) for x in X)
            corrsum = 0.0
            for l in range(M):
                acf, n = 0.0, 0.0
                for x in X0:
                    if len(x) > l:
                        acf += np.sum(x[0:len(x) - l] * x[l:len(x)])
                        n += float(len(x) - l)
                acf /= n
                if acf <= 0:
                    break
                if l > 0:
                    corrsum += acf * (1.0 - float(l) / float(M))
            si[i, j] = 1.0 / (2 * (0.5 + mact * corrsum / x2m))
    return si


def position_inefficiencies(trajs, k, lag, mact=1.0):
    """(si f64 [k, k], truncation lags int32 [k, k], C int64 [k, k]) by the exact position form."""
    C = sliding_counts(trajs, k, lag)
    rows = rows_of(trajs, k, lag)
    si = np.zeros((k, k))
    trunc = np.zeros((k, k), np.int32)
    for i in range(k):
        if not rows[i]:
            continue
        lens = np.array([len(t) for t in rows[i]], np.int64)
        N, M = int(lens.sum()), int(lens.max())
        tgt = np.concatenate(rows[i])
        first = np.repeat(np.cumsum(lens) - lens, lens)          # row rank of the head of each member's sub-sequence
        last = np.repeat(np.cumsum(lens), lens)                  # one past its end
        rank = np.arange(N, dtype=np.int64)
        sorted_lens = np.sort(lens)
        suffix = np.concatenate([np.cumsum(sorted_lens[::-1])[::-1], [0]])
        for j in np.flatnonzero(C[i]):
            occ = np.flatnonzero(tgt == j)
            c = int(occ.size)
            r, e = rank[occ], last[occ]
            tails = np.sort(e - 1 - r)
            heads = np.sort(r - first[occ])
            terms, l_star = [], M
            for l in range(M):
                at = np.searchsorted(r, r + l)
                hit = at < c
                S = int(np.count_nonzero((r[at[hit]] == r[hit] + l) & (r[hit] + l < e[hit])))
                A = c - int(np.searchsorted(tails, l))
                B = c - int(np.searchsorted(heads, l))
                q = int(np.searchsorted(sorted_lens, l, side="right"))      # sub-sequences with length <= l
                n_l = int(suffix[q]) - l * (len(lens) - q)
                Q = S * N * N - c * N * (A + B) + c * c * n_l
                if Q <= 0:
                    l_star = l
                    break
                if l > 0:
                    terms.append((Q * (M - l)) / (N * N * n_l * M))
            corrsum = math.fsum(terms)
            si[i, j] = 1.0 / (1.0 + 2.0 * mact * corrsum * N / c)
            trunc[i, j] = l_star
    return si, trunc, C


def average_counts(C, si, average):
    """Ceff f64 [k, k] from the sliding counts and the inefficiencies."""
    Cf = C.astype(np.float64)
    if average == "none":
        return Cf * si
    if average == "all":
        return Cf * ((Cf * si).sum() / Cf.sum()) if Cf.sum() > 0 else Cf * 0.0
    if average == "row":
        N = Cf.sum(axis=1)
        w = np.divide((Cf * si).sum(axis=1), N, out=np.zeros_like(N), where=N > 0)
        return Cf * w[:, None]
    raise ValueError(average)


def effective_reference(dtrajs, k, lag, average="row", mact=1.0):
    """(Ceff, si, C, truncation lags) of the exact form for a list of label arrays."""
    si, trunc, C = position_inefficiencies(split_valid(dtrajs, k), k, lag, mact)
    return average_counts(C, si, average), si, C, trunc
