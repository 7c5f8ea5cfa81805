"""numpy restatement of the reactive-pathway rule of include/msmhip.h (msm_reactive_pathways_*), and a seeded
generator of reversible chains with their TPT in numpy.  TEST INFRASTRUCTURE: never imported by the product.

The restatement knows nothing of launches, heaps or workgroups: a dense arg-max Dijkstra (np.argmax returns the
first maximum, i.e. the lowest index) on the (n + 2) x (n + 2) work matrix, the three set-up sums as sequential
chains (np.cumsum adds left to right)."""

from __future__ import annotations

import numpy as np

RUNNING, FRACTION, NO_PATH, MAXITER = range(4)


def _chain_sum(v: np.ndarray) -> float:
    """v[0] + v[1] + ... in ascending index, one fp64 chain (0.0 for an empty vector)."""
    v = np.asarray(v, np.float64)
    return float(np.cumsum(v)[-1]) if v.size else 0.0


def work_matrix(net: np.ndarray, role: np.ndarray):
    """(G, total): the net flux with the virtual source n and the virtual sink n + 1."""
    net = np.asarray(net, np.float64)
    n = net.shape[0]
    G = np.zeros((n + 2, n + 2))
    G[:n, :n] = net
    for a in np.flatnonzero(np.asarray(role) == 1):
        G[n, a] = _chain_sum(net[a, :])
    for b in np.flatnonzero(np.asarray(role) == 2):
        G[b, n + 1] = _chain_sum(net[:, b])
    return G, _chain_sum(G[n, :n])


def widest_path(G: np.ndarray, src: int, dst: int):
    """(path, cap) of the max-min path src -> dst, or (None, 0.0).  Ties go to the lowest index."""
    N = G.shape[0]
    width = np.zeros(N)
    width[src] = np.inf
    prev = np.full(N, -1)
    done = np.zeros(N, bool)
    while True:
        i = int(np.argmax(np.where(done, -1.0, width)))
        w = width[i]
        if done[i] or not w > 0.0:
            return None, 0.0
        if i == dst:
            break
        done[i] = True
        cand = np.minimum(w, G[i])
        better = ~done & (cand > width)
        width[better] = cand[better]
        prev[better] = i
    path = [dst]
    while path[-1] != src:
        path.append(int(prev[path[-1]]))
    return path[::-1], float(width[dst])


def pathways(net, role, fraction: float = 0.99, maxiter: int = 10_000):
    """(paths, caps, status) by the rule; every path found is returned."""
    G, total = work_matrix(net, role)
    n = G.shape[0] - 2
    paths, caps, got = [], [], 0.0
    while True:
        if not total > 0.0:
            return paths, np.asarray(caps, float), NO_PATH
        if not got < fraction * total * (1.0 - 1e-14):
            return paths, np.asarray(caps, float), FRACTION
        if len(paths) >= int(maxiter):
            return paths, np.asarray(caps, float), MAXITER
        path, cap = widest_path(G, n, n + 1)
        if path is None or cap <= 1e-14 * total:
            return paths, np.asarray(caps, float), NO_PATH
        for a, b in zip(path[:-1], path[1:]):
            G[a, b] = max(0.0, G[a, b] - cap)
        paths.append([int(v) for v in path[1:-1]])
        caps.append(cap)
        got = got + cap


# ---- reversible chains -----------------------------------------------------------------------------------------
def reversible_chain(n: int, seed: int, mask: float | None = None):
    """(T, pi): S symmetric uniform random, an optional symmetric zero mask of the given density,
    S += 3 diag(rowsum) + 1e-3 I, T = S / rowsum, pi proportional to rowsum."""
    rng = np.random.default_rng(seed)
    S = rng.random((n, n))
    S = 0.5 * (S + S.T)
    if mask is not None:
        M = rng.random((n, n)) < mask
        M = np.triu(M, 1)
        S[M | M.T] = 0.0
    S = S + 3.0 * np.diag(S.sum(axis=1)) + 1e-3 * np.eye(n)
    rs = S.sum(axis=1)
    return S / rs[:, None], rs / rs.sum()


def tpt_numpy(T: np.ndarray, pi: np.ndarray, source, sink):
    """Committors, gross and net flux in numpy (the dense algorithm of markov_state_model/tpt.py)."""
    n = T.shape[0]
    role = np.zeros(n, np.int32)
    role[list(source)] = 1
    role[list(sink)] = 2
    inter = role == 0
    W = np.where(inter[:, None], T - np.eye(n), np.eye(n))
    qp = np.linalg.solve(W, (role == 2).astype(float))
    Tb = (pi[None, :] * T.T) / pi[:, None]
    Wb = np.where(inter[:, None], Tb - np.eye(n), np.eye(n))
    qm = np.linalg.solve(Wb, (role == 1).astype(float))
    gross = (pi * qm)[:, None] * T * qp[None, :]
    np.fill_diagonal(gross, 0.0)
    net = np.maximum(0.0, gross - gross.T)
    return {"role": role, "qplus": qp, "qminus": qm, "gross": gross, "net": net}


def chain_case(n: int, n_source: int, n_sink: int, seed: int, mask: float | None = None):
    """The generator's case: the first n_source states are the source, the last n_sink the sink.
    Returns (T, pi, source, sink, role, net)."""
    T, pi = reversible_chain(n, seed, mask)
    source, sink = list(range(n_source)), list(range(n - n_sink, n))
    out = tpt_numpy(T, pi, source, sink)
    return T, pi, source, sink, out["role"], out["net"]


# (n, sources, sinks, fraction, mask, maxiter): the shapes the restatement was checked on against the host walk
TABLE = [
    (12, 1, 1, 0.99, None, 10_000),
    (37, 3, 2, 0.99, 0.5, 10_000),
    (62, 1, 1, 0.9, 0.7, 10_000),
    (63, 1, 1, 0.9, 0.7, 10_000),
    (130, 2, 2, 0.8, 0.5, 10_000),
    (500, 1, 1, 0.99, None, 60),
    (1022, 1, 1, 0.99, None, 3),
    (1023, 1, 1, 0.99, None, 3),
]
