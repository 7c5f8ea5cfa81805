"""TEST INFRASTRUCTURE ONLY: generators, exact references and tolerance helpers for the dense estimation, CK and
TPT kernels (msm.hip's count -> T chain, revmle.hip, ck.hip, tpt.hip).

Nothing here is tuned on the device.  Every tolerance is one of
  1. exact (integer counts below 2^53, correctly rounded division, the fma chains restated in oracle/msm_oracle.c),
  2. a rounding bound with the number of terms as its argument (sum_bound, product_bound), u = 2^-53,
  3. a multiple (8) of the reference implementation's own error against a longdouble truth, with a stated floor.
tests/test_estimation_reference.py checks the references, the closed forms and the conditions the GPU tests rely on
(condition numbers, |E| >= 1e-3, row sums of the generated stochastic matrices) on a machine without a GPU."""

from __future__ import annotations

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
PAD = 3                      # every strided case: ld = n + PAD, batch strides larger than rows * ld
MARGIN = 8.0                 # rule 3: the kernel may be this much worse than the reference implementation


# ---------------------------------------------------------------------------------------------------------
# tolerance helpers
# ---------------------------------------------------------------------------------------------------------
def sum_bound(m: int) -> float:
    """Relative error of a float64 sum of m non-negative terms in ANY order: m - 1 additions, each within u."""
    return max(int(m) - 1, 0) * U


def product_bound(factors: int) -> float:
    """Relative error of a float64 product of `factors` factors against the exact product (the issue's count:
    one u per factor, which covers the factors - 1 multiplications)."""
    return int(factors) * U


def assert_within(got, want, rtol, what="", atol=0.0):
    """|got - want| <= rtol |want| + atol, compared in longdouble; NaN or inf on either side fails."""
    g, w = np.asarray(got, LD), np.asarray(want, LD)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.isfinite(g).all() and np.isfinite(w).all(), f"{what}: non-finite value"
    err = np.abs(g - w)
    lim = LD(rtol) * np.abs(w) + np.asarray(atol, LD)
    lim = np.broadcast_to(lim, err.shape)
    bad = err > lim
    if bad.any():
        i = np.unravel_index(int(np.argmax(err - lim)), err.shape) if err.ndim else ()
        raise AssertionError(f"{what}: |{float(g[i])!r} - {float(w[i])!r}| = {float(err[i]):.3e} > {float(lim[i]):.3e}"
                             f" at {i} ({int(bad.sum())} of {bad.size} entries)")


def assert_sum_close(got, want, m, what=""):
    assert_within(got, want, sum_bound(m), what)


def rel_dev(a, truth):
    """max |a - truth| / |truth| over the non-zero entries of truth; entries where truth is 0 must be 0 exactly."""
    a, t = np.asarray(a, LD), np.asarray(truth, LD)
    assert a.shape == t.shape
    zero = t == 0
    assert np.array_equal(a[zero], t[zero]), "a structural zero of the truth is not zero"
    if zero.all():
        return 0.0
    return float(np.max(np.abs(a[~zero] - t[~zero]) / np.abs(t[~zero])))


def rule3_limit(ref_err: float, floor: float) -> float:
    return max(MARGIN * ref_err, floor)


# ---------------------------------------------------------------------------------------------------------
# padded buffers: NaN everywhere, payload written into it
# ---------------------------------------------------------------------------------------------------------
def pad2d(a, ld=None):
    """a [r, c] -> NaN buffer [r, ld] with a in its leading columns (ld = c + PAD by default)."""
    a = np.asarray(a, np.float64)
    if a.ndim == 1:
        a = a[:, None]
    ld = a.shape[1] + PAD if ld is None else ld
    buf = np.full((a.shape[0], ld), np.nan)
    buf[:, :a.shape[1]] = a
    return buf


def pad_batch(mats, rows, cols, ld, stride):
    """list of [r_b <= rows, c_b <= cols] -> flat NaN buffer of len(mats) * stride doubles, matrix b at b * stride
    with row stride ld."""
    assert ld >= cols and stride >= rows * ld
    buf = np.full(len(mats) * stride, np.nan)
    for b, m in enumerate(mats):
        m = np.asarray(m, np.float64)
        v = buf[b * stride:b * stride + rows * ld].reshape(rows, ld)
        v[:m.shape[0], :m.shape[1]] = m
    return buf


def batch_view(buf, b, rows, ld, stride):
    return buf[b * stride:b * stride + rows * ld].reshape(rows, ld)


def batch_padding_mask(batch, rows, cols, ld, stride):
    """True on every double of the flat buffer that lies outside all rows x cols payload areas."""
    mask = np.ones(batch * stride, bool)
    for b in range(batch):
        batch_view(mask, b, rows, ld, stride)[:, :cols] = False
    return mask


# ---------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------
def stochastic(n, seed, m=None, floor=0.0):
    """Dense row-stochastic [n, m or n] matrix whose exact row sums are within 4u of 1 (the largest entry of each
    row absorbs the rounding residual)."""
    rng = np.random.default_rng(seed)
    R = rng.random((n, n if m is None else m)) + floor
    T = R / R.sum(axis=1, keepdims=True)
    for _ in range(2):
        res = (LD(1) - T.astype(LD).sum(axis=1)).astype(np.float64)
        T[np.arange(n), T.argmax(axis=1)] += res
    return T


def reversible_chain(n, seed):
    """Dense reversible chain (T, pi): a symmetric positive flux matrix, row-normalised."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, n)) + 0.05
    X = X + X.T
    T = X / X.sum(axis=1, keepdims=True)
    pi = X.sum(axis=1) / X.sum()
    return T, pi


def stationary_ld(T, iters=None):
    """Stationary vector of a dense positive chain as float64: power iteration in longdouble from uniform."""
    T = np.asarray(T, LD)
    n = T.shape[0]
    p = np.full(n, LD(1) / n)
    for _ in range(iters or 400):
        q = p @ T
        q /= q.sum()
        if np.max(np.abs(q - p)) < LD(1e-19):
            p = q
            break
        p = q
    return p.astype(np.float64)


def mode0_counts(k, dtype, seed, zero_rows=True):
    """Mode-0 input: small counts, a few entries up to 2^40, all-zero rows (0, k - 1 and two inside, for k > 2; with
    zero_rows=False only the two inside, and the first and the last row carry T_ii >= 0.1 instead) and every seventh
    row with T_ii >= 0.1 (int64: T_ii = 1/2 up to the integer division; float64: 1/3)."""
    rng = np.random.default_rng(seed)
    C = rng.integers(0, 50, size=(k, k)).astype(np.float64)
    for i, j in zip(rng.integers(0, k, 6), rng.integers(0, k, 6)):
        C[i, j] = float(2 ** 40 - int(rng.integers(0, 1000)))
    floating = np.dtype(dtype) == np.float64
    if floating:
        C = C + rng.random((k, k))
    for i in sorted(set(range(0, k, 7)) | {k - 1}):
        C[i, i] = 0.0
        off = C[i].sum()
        C[i, i] = (0.5 * off if floating else off) if off > 0 else 1.0
    if k > 2:
        C[[0, k - 1, k // 3, k // 2] if zero_rows else [k // 3, k // 2]] = 0
    return np.ascontiguousarray(C.astype(dtype))


def mode1_inactive(k):
    """Inactive states of the mode-1 cases: 0, 1023, 1024, k - 1 and a run of min(70, k // 3) in the middle."""
    idx = {i for i in (0, 1023, 1024, k - 1) if 0 <= i < k}
    run = min(70, k // 3)
    idx |= set(range(k // 2, k // 2 + run))
    return np.asarray(sorted(idx), int)


def mode1_counts(k, dtype, seed, *, variant="planted", epsilon=1e-12):
    """Mode-1 input -> (C, info).  variant: 'planted' (inactive states as mode1_inactive, one state with column
    counts but an empty row, and for float64 one state whose rowsum + colsum is exactly `epsilon` and one an ulp
    above it), 'all' (every state active) or 'zero' (C = 0).  Counts are integers, so every row sum is exact."""
    rng = np.random.default_rng(seed)
    info = {"epsilon": epsilon}
    if variant == "zero":
        return np.zeros((k, k), dtype), info
    C = rng.integers(0, 4, size=(k, k)).astype(np.float64)
    C[np.arange(k), np.arange(k)] += 1.0          # every state starts with a count of its own
    if variant == "all" or k == 1:
        return np.ascontiguousarray(C.astype(dtype)), info
    dead = mode1_inactive(k)
    C[dead, :] = 0.0
    C[:, dead] = 0.0
    alive = np.setdiff1d(np.arange(k), dead)
    if alive.size >= 3:
        s = int(alive[alive.size // 3])
        C[s, :] = 0.0                               # incoming counts only: active, denominator ka * alpha
        C[alive[0], s] += 2.0
        info["column_only"] = s
    if np.dtype(dtype) == np.float64 and dead.size >= 3:
        half = 0.5 * epsilon
        e_at, e_above = int(dead[1]), int(dead[2])
        C[e_at, e_at] = half                                  # rowsum + colsum == epsilon: inactive (strict >)
        C[e_above, e_above] = np.nextafter(half, 1.0)         # one ulp of epsilon above it: active
        assert half + half == epsilon and 2 * np.nextafter(half, 1.0) == np.nextafter(epsilon, 1.0)
        info.update(at_epsilon=e_at, above_epsilon=e_above)
    return np.ascontiguousarray(C.astype(dtype)), info


def mode1_reference(C, alpha, epsilon):
    """(active, inv_map, T_active in longdouble) by the published rule: rowsum + colsum > epsilon, then
    (C_act + alpha) / (rowsum_act + ka alpha)."""
    Cf = np.asarray(C, np.float64)
    k = Cf.shape[0]
    tot = Cf.sum(axis=1) + Cf.sum(axis=0)           # integers (and two dyadic entries): exact in any order
    active = np.nonzero(tot > epsilon)[0]
    inv = np.full(k, -1, np.int32)
    inv[active] = np.arange(active.size, dtype=np.int32)
    Ca = Cf[np.ix_(active, active)].astype(LD)
    rows = Cf[active].astype(LD).sum(axis=1)
    T = (Ca + LD(alpha)) / (rows + LD(active.size) * LD(alpha))[:, None] if active.size else np.zeros((0, 0), LD)
    return active.astype(np.int32), inv, T


def embed_reference(T_act_padded, inv_map, pi_act):
    """npport.ml_msm's embedding: identity on inactive states, the active block elsewhere, pi = 0 outside."""
    inv = np.asarray(inv_map)
    k = inv.size
    act = np.nonzero(inv >= 0)[0]
    T = np.eye(k)
    T[np.ix_(act, act)] = np.asarray(T_act_padded)[:act.size, :act.size]
    pi = np.zeros(k)
    if pi_act is not None:
        pi[act] = np.asarray(pi_act)[:act.size]
    return T, pi


def power_ld(T, squarings):
    P = np.asarray(T, LD)
    for _ in range(squarings):
        P = P @ P
    return P


def matpow_ld(P, f):
    """P^f by repeated right-multiplication in longdouble."""
    P = np.asarray(P, LD)
    out = P.copy()
    for _ in range(f - 1):
        out = out @ P
    return out


def revmle_counts(n, seed, blocks=4):
    """Asymmetric positive counts with metastable blocks (the shape tests/test_gpu_revmle.py uses)."""
    rng = np.random.default_rng(seed)
    C = rng.poisson(0.3, size=(n, n)).astype(float)
    w = max(1, n // blocks)
    for b in range(blocks):
        s = slice(b * w, (b + 1) * w if b < blocks - 1 else n)
        C[s, s] += rng.poisson(6.0, size=C[s, s].shape)
    return C + 1e-3


def banded_circulant_counts(n):
    """Offsets 0, +1, -1, +7 with weights 5, 2, 1, 0.5 (asymmetric, connected, five non-zeros per row of C + C')."""
    C = np.zeros((n, n))
    i = np.arange(n)
    for off, w in ((0, 5.0), (1, 2.0), (-1, 1.0), (7, 0.5)):
        C[i, (i + off) % n] += w
    return C


def revmle_ld(C, maxiter):
    """npport.reversible_mle restated in longdouble on the non-zero pattern of C + C', exactly `maxiter`
    iterations -> (T, pi) as longdouble.  States without any flux keep a self-loop, as the kernel's do."""
    C = np.asarray(C, np.float64)
    n = C.shape[0]
    C2 = C + C.T                                     # the kernel's first rounding is part of the operation
    r, cidx = np.nonzero(C2 > 0)                     # row-major: r is sorted
    w = C2[r, cidx].astype(LD)
    c = C.astype(LD).sum(axis=1) if n < 2000 else np.asarray([C[i].astype(LD).sum() for i in range(n)], LD)
    starts = np.searchsorted(r, np.arange(n))
    has = np.diff(np.append(starts, r.size)) > 0

    def rowsum(vals):
        out = np.zeros(n, LD)
        if vals.size:
            red = np.add.reduceat(vals, starts[has])
            out[has] = red
        return out

    def flux(x):
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(x > 0, c / np.where(x > 0, x, LD(1)), LD(0))
        den = v[r] + v[cidx]
        ok = den > 0
        return np.where(ok, w / np.where(ok, den, LD(1)), LD(0))

    x = rowsum(w)
    x = x / x.sum()
    for _ in range(maxiter):
        x = rowsum(flux(x))
        x = x / x.sum()
    f = flux(x)
    rs = rowsum(f)
    T = np.zeros((n, n), LD) if n < 2000 else None
    vals = np.where(rs[r] > 0, f / np.where(rs[r] > 0, rs[r], LD(1)), LD(0))
    if T is not None:
        T[r, cidx] = vals
        lone = np.nonzero(rs == 0)[0]
        T[lone, lone] = 1
        return T, x
    return (r, cidx, vals), x                        # large orders: the non-zeros only


# ---------------------------------------------------------------------------------------------------------
# linear solves
# ---------------------------------------------------------------------------------------------------------
SOLVE_SHAPES = [(1, 1), (2, 1), (63, 1), (64, 3), (65, 2), (257, 1), (1025, 5)]


def solve_system(n, nrhs):
    """The seeded system of the solve tests: default_rng(n) normals, A[0,0] = 0 for n > 1 (forces a row swap)."""
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, n))
    if n > 1:
        A[0, 0] = 0.0
    B = rng.standard_normal((n, nrhs))
    return A, B


def cond_inf(A):
    A = np.asarray(A, np.float64)
    return float(np.abs(A).sum(axis=1).max() * np.abs(np.linalg.inv(A)).sum(axis=1).max())


def backward_error(A, X, B):
    """omega = max_j ||A x_j - b_j||inf / (||A||inf ||x_j||inf + ||b_j||inf), residual in longdouble."""
    A_, X_, B_ = (np.asarray(v, LD) for v in (A, X, B))
    X_ = X_.reshape(A_.shape[0], -1)
    B_ = B_.reshape(A_.shape[0], -1)
    R = np.abs(A_ @ X_ - B_).max(axis=0)
    den = np.abs(A_).sum(axis=1).max() * np.abs(X_).max(axis=0) + np.abs(B_).max(axis=0)
    return float(np.max(R / den))


def solve_limit(A, B):
    """Rule 3 for A X = B: (limit, omega of np.linalg.solve)."""
    n = A.shape[0]
    ref = backward_error(A, np.linalg.solve(A, B), B)
    return rule3_limit(ref, n * U), ref


def tied_pivot_matrix(n=48, seed=48):
    """+-1 entries: every column's pivot search starts among ties."""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], size=(n, n)), rng.integers(-4, 5, size=(n, 2)).astype(float)


def singular_cases(n=40):
    """(name, A, B): an exactly zero column at 0, n/2, n-1, and two equal rows of small integers."""
    rng = np.random.default_rng(1234)
    out = []
    for c in (0, n // 2, n - 1):
        A = rng.standard_normal((n, n))
        A[:, c] = 0.0
        out.append((f"zero_column_{c}", A, rng.standard_normal((n, 1))))
    A = rng.integers(-3, 4, size=(n, n)).astype(float)
    A[n - 7] = A[5]
    out.append(("equal_rows", A, rng.integers(-3, 4, size=(n, 1)).astype(float)))
    return out


def solve_ld(A, B):
    """Gaussian elimination with partial pivoting in longdouble (small systems: the truth of the closed forms)."""
    A = np.array(A, LD)
    n = A.shape[0]
    X = np.array(B, LD).reshape(n, -1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            X[[k, p]] = X[[p, k]]
        l = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= l[:, None] * A[k, k:][None, :]
        X[k + 1:] -= l[:, None] * X[k][None, :]
    for k in range(n - 1, -1, -1):
        X[k] = (X[k] - A[k, k + 1:] @ X[k + 1:]) / A[k, k]
    return X.reshape(np.shape(B))


# ---------------------------------------------------------------------------------------------------------
# TPT: committor systems, birth-death closed forms
# ---------------------------------------------------------------------------------------------------------
def committor_systems(T, pi, role):
    """(W+, r+, W-, r-) exactly as committor_system_kernel forms them in float64 (identity rows on A and B)."""
    T, pi, role = np.asarray(T, np.float64), np.asarray(pi, np.float64), np.asarray(role)
    n = T.shape[0]
    eye = np.eye(n)
    Wf = T - eye
    Wb = pi[None, :] * T.T / pi[:, None] - eye
    fixed = role != 0
    Wf[fixed] = eye[fixed]
    Wb[fixed] = eye[fixed]
    return Wf, (role == 2).astype(float), Wb, (role == 1).astype(float)


def roles(n, seed=None):
    """role vector: state 0 the source, n - 1 the sink; with a seed, ~10 % more of each (n >= 20)."""
    role = np.zeros(n, np.int32)
    role[0], role[n - 1] = 1, 2
    if seed is not None and n >= 20:
        rng = np.random.default_rng(seed)
        pick = rng.permutation(np.arange(1, n - 1))[:n // 5]
        role[pick[:pick.size // 2]] = 1
        role[pick[pick.size // 2:]] = 2
    return role


def birth_death(n, seed):
    """Nearest-neighbour chain (T, pi as float64; a, b, pi_ld in longdouble of the float64 rates): p(i,i+1) = a_i,
    p(i,i-1) = b_i.  The rates are multiples of 1/64, so 1 - a - b and T - I are exact and the float64 chain is the
    ideal one the closed forms describe."""
    rng = np.random.default_rng(seed)
    a = rng.integers(4, 26, n) / 64.0
    b = rng.integers(4, 26, n) / 64.0
    a[-1] = 0.0
    b[0] = 0.0
    T = np.zeros((n, n))
    i = np.arange(n - 1)
    T[i, i + 1] = a[:-1]
    T[i + 1, i] = b[1:]
    T[np.arange(n), np.arange(n)] = 1.0 - a - b
    a_, b_ = a.astype(LD), b.astype(LD)
    pi = np.ones(n, LD)
    for j in range(1, n):
        pi[j] = pi[j - 1] * a_[j - 1] / b_[j]
    pi /= pi.sum()
    return T, pi.astype(np.float64), a_, b_, pi


def birth_death_qplus(a_ld, pi_ld):
    """Forward committor from state 0 to state n - 1: harmonic in the resistances 1 / (pi_l a_l)."""
    r = 1 / (pi_ld[:-1] * a_ld[:-1])
    q = np.concatenate(([LD(0)], np.cumsum(r)))
    return q / q[-1]


def birth_death_mfpt(a_ld, b_ld, pi_ld):
    """m(i -> i+1) = sum_{l<=i} pi_l / (pi_i a_i), m(i -> i-1) = sum_{l>=i} pi_l / (pi_i b_i); sums along the path."""
    n = pi_ld.size
    up = np.cumsum(pi_ld)[:-1] / (pi_ld[:-1] * a_ld[:-1])                   # i -> i + 1, i = 0 .. n-2
    down = np.cumsum(pi_ld[::-1])[::-1][1:] / (pi_ld[1:] * b_ld[1:])        # i -> i - 1, i = 1 .. n-1
    M = np.zeros((n, n), LD)
    for i in range(n):
        for j in range(n):
            M[i, j] = up[i:j].sum() if j > i else down[j:i].sum() if j < i else 0
    return M


def mfpt_systems(T):
    """[(A_t, ones)] exactly as mfpt_system_kernel forms them: I - T with row and column t removed."""
    T = np.asarray(T, np.float64)
    n = T.shape[0]
    out = []
    for t in range(n):
        keep = np.arange(n) != t
        out.append((np.eye(n - 1) - T[np.ix_(keep, keep)], np.ones(n - 1)))
    return out


def closed_class_chains():
    """Dyadic chains (every elimination step is exact, so a singular system meets an exact zero pivot).
    -> [(name, T, expected singular targets)].  With two closed classes every target leaves one class whole, so
    every system is singular; with one closed class and two transient states only the transient targets are."""
    two = np.array([[0.5, 0.5, 0, 0, 0],
                    [0.25, 0.75, 0, 0, 0],
                    [0.125, 0.125, 0.5, 0.125, 0.125],
                    [0, 0, 0, 0.75, 0.25],
                    [0, 0, 0, 0.5, 0.5]])
    one = np.array([[0.5, 0.5, 0, 0],
                    [0.25, 0.75, 0, 0],
                    [0.25, 0, 0.5, 0.25],
                    [0, 0.25, 0.25, 0.5]])
    return [("two_closed", two, [0, 1, 2, 3, 4]), ("one_closed_two_transient", one, [2, 3])]


def lump_reference(T, pi, macro, n_macro):
    """(T_macro, pi_macro) in longdouble: F[A][B] = sum_{i in A} pi_i sum_{j in B} T_ij, rows normalised (zero
    rows stay zero); populations renormalised."""
    T_, pi_ = np.asarray(T, LD), np.asarray(pi, LD)
    macro = np.asarray(macro)
    n = T_.shape[0]
    cols = np.zeros((n, n_macro), LD)
    for B in range(n_macro):
        sel = macro == B
        if sel.any():
            cols[:, B] = T_[:, sel].sum(axis=1)
    cols *= pi_[:, None]
    F = np.zeros((n_macro, n_macro), LD)
    p = np.zeros(n_macro, LD)
    for A in range(n_macro):
        sel = macro == A
        if sel.any():
            F[A] = cols[sel].sum(axis=0)
            p[A] = pi_[sel].sum()
    rs = F.sum(axis=1)
    F = F / np.where(rs == 0, LD(1), rs)[:, None]
    s = p.sum()
    return F, (p / s if s > 0 else p)


def lump_assignment(n, n_macro, seed, empty=None):
    """micro -> macro map with every macrostate used (except `empty`), in a shuffled order."""
    rng = np.random.default_rng(seed)
    used = np.asarray([m for m in range(n_macro) if m != empty])
    assert n >= used.size
    macro = np.concatenate([used, rng.choice(used, size=n - used.size)])
    return rng.permutation(macro).astype(np.int32)


def ck_perturbation(n, seed):
    """E with 1e-3 <= |E_ij| <= 3e-3 and random signs."""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], size=(n, n)) * rng.uniform(1e-3, 3e-3, size=(n, n))


CK_FACTORS = [3, 1, 2, 3, 5]


def ck_case(n, seed):
    """(T1, Tk [F, n, n], E [F, n, n]): Tk[i] = round(T1^f_i in longdouble) + E_i; the entry of factor 1 is T1
    itself (E = 0), the two entries of factor 3 share one E.  Every Tk entry stays inside [0, 1]."""
    T1 = stochastic(n, seed)
    Tk, Es = [], []
    for i, f in enumerate(CK_FACTORS):
        E = np.zeros((n, n)) if f == 1 else ck_perturbation(n, 1000 * seed + f)
        if n == 1:
            E = -np.abs(E)                           # T1 = [[1]]: keep Tk inside [0, 1] for the multinomial noise
        Tk.append(T1.copy() if f == 1 else matpow_ld(T1, f).astype(np.float64) + E)
        Es.append(E)
    return T1, np.stack(Tk), np.stack(Es)


def ck_mse_reference(T1, Tk, factors):
    return [((matpow_ld(T1, f) - np.asarray(Tk[i], LD)) ** 2).mean() for i, f in enumerate(factors)]


def ck_mse_rtol(f, n):
    """2 f n u / 1e-3 (the power's rounding against |E| >= 1e-3, entering the squares twice) + n^2 u (the sum)."""
    return 2.0 * f * n * U / 1e-3 + n * n * U


def multinomial_se_ld(P, counts):
    P_, N = np.asarray(P, LD), np.asarray(counts, np.float64)
    n = P_.shape[0]
    N = np.where(np.isfinite(N) & (N > 0.0), N, 1.0).astype(LD)
    return np.sqrt(((P_ * (1 - P_)).sum(axis=1) / N).sum() / (LD(n) * n))


def diff_norms_ld(P, Q):
    P_, Q_ = np.asarray(P, LD), np.asarray(Q, LD)
    d = np.asarray(P, np.float64) - np.asarray(Q, np.float64)      # the kernel's (rounded) difference is the term
    d_ = d.astype(LD)
    return np.asarray([np.abs(d_).sum(), np.abs(Q_).sum(), (d_ * d_).sum()], LD)


DIFF_SHAPES = [(1, 1), (1, 5000), (300, 7), (64, 64)]
