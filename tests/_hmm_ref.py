"""numpy restatement of the HMM contract (include/msmhip.h, "HMM"): the scaled forward-backward pass in the sequential
order and in the chunked order of the device, the emission sums, the M-step, Viterbi, brute-force enumeration; the
inputs the CPU and GPU tests share; the rounding bounds both hold results to.

Every step takes a `dtype`: np.float64 is the restatement proper, np.longdouble (80-bit on x86, eps 1.1e-19) the
near-exact yardstick the device is compared with.
"""
from __future__ import annotations

import itertools

import numpy as np

ULP = 2.0 ** -52
L = 64                         # steps of a chunk (MSM_HMM_CHUNK); the GPU tests check it against hmm_plan
SEGMENT = 256                  # member frames of an emission unit
BAD_SYMBOL, ZERO_PROB, EMPTY_STATE, BAD_TABLE, NOT_CONVERGED = 1, 2, 4, 8, 16


# ---- sequences ---------------------------------------------------------------------------------------------------
def lag_observations_loop(dtrajs, lag, k):
    """The plain loop: (labels, [(start, stride, length)])."""
    labels, rows, off = [], [], 0
    for d in dtrajs:
        d = [int(x) for x in d]
        t = 0
        while t < len(d):
            if not 0 <= d[t] < k:
                t += 1
                continue
            e = t
            while e < len(d) and 0 <= d[e] < k:
                e += 1
            for s in range(min(lag, e - t)):
                rows.append((off + t + s, lag, len(range(t + s, e, lag))))
            t = e
        labels += d
        off += len(d)
    return np.asarray(labels, np.int32), np.asarray(rows, np.int64).reshape(-1, 3)


def observations(labels, row):
    start, stride, length = (int(x) for x in row)
    return np.asarray(labels)[start + stride * np.arange(length)]


def chunks_of(T, chunk=L):
    """[(t0, t1)] inclusive: chunk c covers t = 1 + cL .. min((c + 1) L, T - 1)."""
    return [(1 + c * chunk, min((c + 1) * chunk, T - 1)) for c in range(-(-(T - 1) // chunk))]


# ---- one sequence ------------------------------------------------------------------------------------------------
def forward_backward(A, B, p0, obs, dtype=np.float64):
    """The sequential order of the contract -> dict(gamma [T, n], C [n, n], logL, dead, S = sum |ln c_t|)."""
    A, B, p0 = (np.asarray(x).astype(dtype) for x in (A, B, p0))
    T, n = len(obs), A.shape[0]
    zero = dict(gamma=np.zeros((T, n), dtype), C=np.zeros((n, n), dtype), logL=dtype(-np.inf), dead=True, S=0.0)
    alpha, c = np.zeros((T, n), dtype), np.zeros(T, dtype)
    u = p0 * B[:, obs[0]]
    for t in range(T):
        if t:
            u = (alpha[t - 1] @ A) * B[:, obs[t]]
        c[t] = u.sum()
        if not c[t] > 0:
            return zero
        alpha[t] = u / c[t]
    beta = np.ones((T, n), dtype)
    C = np.zeros((n, n), dtype)
    for t in range(T - 1, 0, -1):
        v = B[:, obs[t]] * beta[t] / c[t]
        C += alpha[t - 1][:, None] * A * v[None, :]
        beta[t - 1] = A @ v
    return dict(gamma=alpha * beta, C=C, logL=np.log(c).sum(dtype=dtype), dead=False, S=float(np.abs(np.log(c)).sum()))


def _pow2_rescale(P):
    mx = P.max()
    if mx > 0 and np.isfinite(mx):
        return np.ldexp(P, -(int(np.frexp(mx)[1]) - 1))      # 2^-ilogb(max): exact
    return P


def forward_backward_chunked(A, B, p0, obs, dtype=np.float64, chunk=L):
    """The chunked order of the device: chunk products rescaled by powers of two, the boundary vectors, the replay of
    every chunk with the backward side restoring alpha^ . beta^ = 1 at every step."""
    A, B, p0 = (np.asarray(x).astype(dtype) for x in (A, B, p0))
    T, n = len(obs), A.shape[0]
    zero = dict(gamma=np.zeros((T, n), dtype), C=np.zeros((n, n), dtype), logL=dtype(-np.inf), dead=True)
    cks = chunks_of(T, chunk)
    prods = []
    for t0, t1 in cks:
        P = np.eye(n, dtype=dtype)
        for t in range(t0, t1 + 1):
            P = _pow2_rescale((P @ A) * B[None, :, obs[t]])
        prods.append(P)
    u = p0 * B[:, obs[0]]
    c0 = u.sum()
    if not c0 > 0:
        return zero
    a = u / c0
    gamma, C, logL = np.zeros((T, n), dtype), np.zeros((n, n), dtype), np.log(c0)
    gamma[0] = a
    entry = []
    for P in prods:
        entry.append(a)
        u = a @ P
        s = u.sum()
        if not s > 0:
            return zero
        a = u / s
    exits, w = [None] * len(cks), np.ones(n, dtype)
    for ci in range(len(cks) - 1, -1, -1):
        exits[ci] = w
        u = prods[ci] @ w
        w = u / u.sum()
    for ci, (t0, t1) in enumerate(cks):
        al, a, lsum = [entry[ci]], entry[ci], dtype(0)
        for t in range(t0, t1 + 1):
            u = (a @ A) * B[:, obs[t]]
            c = u.sum()
            a = u / c
            lsum = lsum + np.log(c)
            al.append(a)
        w = exits[ci] / (a * exits[ci]).sum()
        Cp = np.zeros((n, n), dtype)
        for t in range(t1, t0 - 1, -1):
            gamma[t] = al[t - t0 + 1] * w
            ap = al[t - t0]
            X = A * (B[:, obs[t]] * w)[None, :]
            wn = X.sum(axis=1)
            Z = (ap * wn).sum()
            Cp += (ap[:, None] * X) / Z
            w = wn / Z
        if ci == 0:
            gamma[0] = entry[0] * w
        C += Cp
        logL = logL + lsum
    return dict(gamma=gamma, C=C, logL=logL, dead=False)


def brute_force(A, B, p0, obs):
    """All n^T hidden paths, in longdouble -> dict(likelihood, gamma, C, best log-probability, best paths)."""
    A, B, p0 = (np.asarray(x).astype(np.longdouble) for x in (A, B, p0))
    T, n = len(obs), A.shape[0]
    like, gamma, C = np.longdouble(0), np.zeros((T, n), np.longdouble), np.zeros((n, n), np.longdouble)
    best, best_paths = np.longdouble(0), []
    for path in itertools.product(range(n), repeat=T):
        p = p0[path[0]] * B[path[0], obs[0]]
        for t in range(1, T):
            p = p * A[path[t - 1], path[t]] * B[path[t], obs[t]]
        like += p
        for t in range(T):
            gamma[t, path[t]] += p
        for t in range(1, T):
            C[path[t - 1], path[t]] += p
        if p > best:
            best, best_paths = p, [path]
        elif p == best:
            best_paths.append(path)
    return dict(likelihood=like, gamma=gamma / like if like > 0 else gamma, C=C / like if like > 0 else C,
                best=best, best_paths=best_paths)


# ---- all sequences -----------------------------------------------------------------------------------------------
def estep(A, B, p0, labels, table, k, dtype=np.float64, chunked=False, chunk=L):
    """-> dict(gamma [N, n], C, gamma0, logL [Q], E [n, k], status, dead [Q], S [Q]); sequences added in ascending
    order."""
    labels = np.asarray(labels)
    n, N = np.asarray(A).shape[0], len(labels)
    gamma, C, g0 = np.zeros((N, n), dtype), np.zeros((n, n), dtype), np.zeros(n, dtype)
    logL, dead, status = np.zeros(len(table), dtype), np.zeros(len(table), bool), 0
    S = np.zeros(len(table))
    for q, row in enumerate(table):
        obs = observations(labels, row)
        if ((obs < 0) | (obs >= k)).any():
            status |= BAD_SYMBOL
            logL[q], dead[q] = -np.inf, True
            continue
        r = (forward_backward_chunked(A, B, p0, obs, dtype, chunk) if chunked else forward_backward(A, B, p0, obs, dtype))
        logL[q], dead[q], S[q] = r["logL"], r["dead"], r.get("S", 0.0)
        if r["dead"]:
            status |= ZERO_PROB
            continue
        frames = int(row[0]) + int(row[1]) * np.arange(int(row[2]))
        gamma[frames] = r["gamma"]
        C += r["C"]
        g0 += r["gamma"][0]
    E = np.zeros((n, k), dtype)
    ok = (labels >= 0) & (labels < k)
    for y in range(k):
        E[:, y] = gamma[ok & (labels == y)].sum(axis=0, dtype=dtype)
    return dict(gamma=gamma, C=C, gamma0=g0, logL=logL, E=E, status=status, dead=dead, S=S)


def reversible_sweep(C, x, dtype=np.float64):
    """One sweep of the fixed point on the row sums: x_i' = sum_j (c_ij + c_ji) / (c_i / x_i + c_j / x_j), normalised."""
    C, x = np.asarray(C).astype(dtype), np.asarray(x).astype(dtype)
    C2, c = C + C.T, C.sum(axis=1)
    v = np.where(x > 0, c / np.where(x > 0, x, 1), 0)
    den = v[:, None] + v[None, :]
    ok = (C2 > 0) & (den > 0)
    f = np.where(ok, C2 / np.where(ok, den, 1), 0)
    xn = f.sum(axis=1)
    return xn / xn.sum(), f


def reversible_mle(C, dtype=np.float64, maxerr=1e-8, maxiter=100_000):
    C = np.asarray(C).astype(dtype)
    C2 = C + C.T
    x = C2.sum(axis=1) / C2.sum()
    for _ in range(maxiter):
        xn, _ = reversible_sweep(C, x, dtype)
        mid = 0.5 * (x + xn)
        err = np.max(np.where(mid > 0, np.abs(x - xn) / np.where(mid > 0, mid, 1), 0))
        x = xn
        if err <= maxerr:
            break
    return transition_from_x(C, x, dtype), x


def transition_from_x(C, x, dtype=np.float64):
    _, f = reversible_sweep(C, x, dtype)
    return f / f.sum(axis=1, keepdims=True)


def stationary_gth(A, dtype=np.float64):
    """Grassmann-Taksar-Heyman elimination: the stationary vector without a subtraction."""
    G = np.array(A, dtype=dtype)
    n = G.shape[0]
    for m in range(n - 1, 0, -1):
        s = G[m, :m].sum()
        G[:m, m] /= s
        G[:m, :m] += G[:m, m][:, None] * G[m, :m][None, :]
    pi = np.zeros(n, dtype)
    pi[0] = 1
    for m in range(1, n):
        pi[m] = pi[:m] @ G[:m, m]
    return pi / pi.sum()


def mstep(C, E, gamma0, Q, dtype=np.float64, reversible=True, stationary=False, maxerr=1e-8):
    """-> (A, B, p0, pi).  A state without mass is not handled here (the tests that meet one check it by hand)."""
    C, E, gamma0 = (np.asarray(x).astype(dtype) for x in (C, E, gamma0))
    B = E / E.sum(axis=1, keepdims=True)
    if reversible:
        A, pi = reversible_mle(C, dtype, maxerr)
    else:
        A = C / C.sum(axis=1, keepdims=True)
        pi = stationary_gth(A, dtype)
    return A, B, (pi if stationary else gamma0 / dtype(Q)), pi


def em_step(A, B, p0, labels, table, k, dtype=np.float64, reversible=False, stationary=False):
    e = estep(A, B, p0, labels, table, k, dtype)
    alive = int((~e["dead"]).sum())
    return mstep(e["C"], e["E"], e["gamma0"], len(table), dtype, reversible, stationary), e, alive


# ---- Viterbi -----------------------------------------------------------------------------------------------------
def viterbi(A, B, p0, obs, dtype=np.float64):
    """The most probable hidden path in the (max, +) semiring, ties to the lowest index -> (path, log-probability);
    (None, -inf) for a sequence of probability 0."""
    with np.errstate(divide="ignore"):
        lA, lB, lp = (np.log(np.asarray(x).astype(dtype)) for x in (A, B, p0))
    T, n = len(obs), lA.shape[0]
    d = lp + lB[:, obs[0]]
    back = np.zeros((T, n), np.int64)
    for t in range(1, T):
        m = d[:, None] + lA
        back[t] = np.argmax(m, axis=0)
        d = m[back[t], np.arange(n)] + lB[:, obs[t]]
    if not d.max() > -np.inf:
        return None, dtype(-np.inf)
    path = [int(np.argmax(d))]
    for t in range(T - 1, 0, -1):
        path.append(int(back[t][path[-1]]))
    return np.asarray(path[::-1]), d.max()


def path_log_probability(A, B, p0, obs, path, dtype=np.longdouble):
    with np.errstate(divide="ignore"):
        lA, lB, lp = (np.log(np.asarray(x).astype(dtype)) for x in (A, B, p0))
    v = lp[path[0]] + lB[path[0], obs[0]]
    for t in range(1, len(obs)):
        v = v + lA[path[t - 1], path[t]] + lB[path[t], obs[t]]
    return v


# ---- rounding bounds ---------------------------------------------------------------------------------------------
# Every quantity of the E-step is built from sums, products and quotients of non-negative numbers, so relative errors
# add without amplification: a quantity is within D 2^-52 of its exact value (relative), D the longest chain of
# roundings from the inputs.  Vectors that are normalised before use (alpha^, the boundary vectors, beta^) are
# tracked by their DIRECTION error e, the elementwise relative error up to a common factor; a normalised ratio of
# such vectors has relative error <= 2 e plus its own roundings.  With n hidden states, chunks of L steps and nc
# chunks in the sequence:
#   alpha^_0 = p0 o b_0 / c_0                          e = 2 (product, quotient)
#   chunk product, per step (P A) diag(b)              n + 1 (n-term dot product, product); the rescaling is exact
#   boundary vector, per chunk  a P / sum              L (n + 1) + n + 1
#   replay, per step  (alpha^ A) o b / c               n + 2
#   beta^ at the chunk's end  w / (alpha^ . w)         1
#   walk back, per step  v = b o w, x = A v, sum, / Z  n + 2
#   gamma_t = alpha^_t o beta^_t                       2 (e(alpha^_t) + e(beta^_t)) + n + 3
# The two direction errors of a frame add up to at most 3 + (nc - 1)(L (n + 1) + n + 1) + min(L, T - 1)(n + 2): the
# boundary vectors cover the other nc - 1 chunks between them, the replay and the walk back the frame's own chunk.
def depth_gamma(T, n, chunk=L):
    if T == 1:
        return n + 3
    nc = -(-(T - 1) // chunk)
    return 2 * (3 + (nc - 1) * (chunk * (n + 1) + n + 1) + min(chunk, T - 1) * (n + 2)) + n + 3


def depth_C(lengths, n, chunk=L):
    """A term alpha^_{t-1}(i) A_ij b_t(j) beta^_t(j) / Z is a gamma with four more roundings; then the chunk's terms,
    the sequence's chunks and the sequences are added."""
    T = max(lengths)
    return depth_gamma(T, n, chunk) + 4 + min(chunk, max(T - 1, 1)) + -(-(T - 1) // chunk) + len(lengths)


def depth_gamma0(lengths, n, chunk=L):
    return depth_gamma(max(lengths), n, chunk) + len(lengths)


def depth_E(lengths, n, max_members, chunk=L):
    """A unit's 256 rows: chains of 16, a tree of 4 chains, 4 waves (21 additions deep); then the symbol's units."""
    return depth_gamma(max(lengths), n, chunk) + 21 + -(-max_members // SEGMENT)


def bound_logL(T, n, S, chunk=L):
    """Absolute.  Inside a chunk the product of the c_t telescopes to sum(a_c M_c) up to (n + 2) roundings a step and
    the n of sum alpha^ = 1; the entry vector a_c carries twice its direction error plus its normalisation (n + 1).
    Nothing telescopes across chunks, so the direction errors 2 + c (L (n + 1) + n + 1) of the entry vectors add up.
    Every ln is taken to 2 ulp of itself and the T + nc additions each round a partial sum that is at most
    S = sum |ln c_t|."""
    nc = -(-(T - 1) // chunk)
    per = chunk * (n + 1) + n + 1
    chain = (n + 1) + nc * (5 + 2 * n) + nc * (nc - 1) * per + (T - 1) * (n + 2)
    return ULP * (chain + (T + nc + 2) * S)


def check_close(got, want, depth, what):
    """|got - want| <= depth ulp of want, elementwise; want in longdouble."""
    got, want = np.asarray(got).astype(np.longdouble), np.asarray(want).astype(np.longdouble)
    err = np.abs(got - want)
    tol = depth * ULP * np.abs(want) + 1e-300
    worst = float(np.max(np.where(want != 0, err / np.where(want != 0, np.abs(want), 1), err))) / ULP
    print(f"{what}: worst {worst:.1f} ulp, bound {depth} ulp")
    assert (err <= tol).all(), f"{what}: worst {worst:.1f} ulp exceeds the bound of {depth} ulp"


# ---- inputs ------------------------------------------------------------------------------------------------------
def random_model(n, k, seed, zeros=False, dtype=np.float64):
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) + 0.1 + 2.0 * np.eye(n)
    B = rng.random((n, k)) + 0.05
    if zeros and n > 1:
        A[0, n - 1] = 0.0
        B[rng.random((n, k)) < 0.3] = 0.0
        B[:, 0] += 0.1
        B[np.arange(n), np.arange(n) % k] += 0.1       # no row and no column of B is empty
        B[0, :] += (B.sum(axis=0) == 0) * 0.1
    p0 = rng.random(n) + 0.1
    return (A / A.sum(axis=1, keepdims=True)).astype(dtype), (B / B.sum(axis=1, keepdims=True)).astype(dtype), \
        (p0 / p0.sum()).astype(dtype)


def sample_labels(A, B, p0, T, seed):
    rng = np.random.default_rng(seed)
    n, k = B.shape
    s = rng.choice(n, p=p0 / p0.sum())
    out = np.empty(T, np.int32)
    for t in range(T):
        out[t] = rng.choice(k, p=B[s] / B[s].sum())
        s = rng.choice(n, p=A[s] / A[s].sum())
    return out


def single_rows(lengths):
    """Consecutive sequences of the given lengths at stride 1."""
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return np.stack([starts, np.ones(len(lengths), np.int64), np.asarray(lengths)], axis=1).astype(np.int64)


# name -> (n, k, sequence lengths (one call), zeros in A and B); the lengths walk every chunk count and remainder
CASES = {
    "n1_k1": (1, 1, [1, 2, L, L + 1], False),
    "n2_k3_edges": (2, 3, [1, 2, L, L + 1, L + 2, 2 * L + 1, 3 * L + 5], False),
    "n3_k63": (3, 63, [L + 2, 1, 2 * L + 1], False),
    "n3_k65_zeros": (3, 65, [3 * L + 5, 2, L], True),
    "n16_k130": (16, 130, [2 * L + 1, 1, L + 1], False),
    "n16_k3_zeros": (16, 3, [L + 2, 3 * L + 5], True),
}


def case_inputs(name):
    n, k, lengths, zeros = CASES[name]
    seed = sorted(CASES).index(name)
    A, B, p0 = random_model(n, k, seed, zeros)
    # sampled from the model itself, so that every sequence has positive probability under it, zeros or not
    labels = np.concatenate([sample_labels(A, B, p0, T, 100 * seed + i) for i, T in enumerate(lengths)])
    return A, B, p0, labels.astype(np.int32), single_rows(lengths), k
