"""TICA reduction: mirror of pmarlo.markov_state_model.reduction
(S/markov_state_model/reduction.py:13-40 _preprocess, :77-110 tica_reduce, :152 reduce_features)
and of FeaturesMixin._maybe_apply_tica (S/markov_state_model/_features.py:181-231)."""

from __future__ import annotations

from typing import Optional, List, Sequence

import numpy as np

from ..device import get_engine
from ..pipeline import MSMPipeline, TicaModel

__all__ = ["tica_reduce", "pca_reduce", "vamp_reduce", "reduce_features", "tica_fit_transform_trajectories",
           "preprocess_params"]


def _as_matrix(X) -> np.ndarray:
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    if X.ndim != 2:
        raise ValueError(f"Expected 2D array, got shape {X.shape}")
    return np.ascontiguousarray(X)


def preprocess_params(X, scale: bool = True):
    """(mean, divisor) of _preprocess (imputed-mean NaNs, population std, zero std -> 1)."""
    eng = get_engine()
    pipe = MSMPipeline(eng)
    mu, sigma, _, _ = pipe.standardise_params(eng.to_device(_as_matrix(X)), scale=scale)
    return mu.to_host(), sigma.to_host()


def tica_reduce(X: np.ndarray, lag: int = 1, n_components: int = 2, scale: bool = True) -> np.ndarray:
    """TICA(lagtime=lag, dim=n_components).fit([X_prep]).transform(X_prep) -> (N, d) float64."""
    Xm = _as_matrix(X)
    if Xm.size == 0:
        return np.zeros((Xm.shape[0], 0))
    eng = get_engine()
    pipe = MSMPipeline(eng)
    xd = eng.to_device(Xm)
    model = pipe.tica_fit(xd, int(lag), int(n_components), scale=scale)
    rank = int(model.rank.to_host()[0])
    if rank == 0:
        raise ValueError("TICA: covariance matrix has zero rank")
    model.dim = min(int(n_components), rank)
    return np.ascontiguousarray(pipe.tica_transform(model, xd).to_host(), dtype=float)


def _gen_batches(n: int, batch_size: int, min_batch_size: int):
    """sklearn.utils.gen_batches: slices of batch_size, a short tail merged into the last slice."""
    start = 0
    for _ in range(int(n // batch_size)):
        end = start + batch_size
        if end + min_batch_size > n:
            continue
        yield start, end
        start = end
    if start < n:
        yield start, n


def _incremental_pca(eng, pipe, xd, n: int, F: int, n_components: int, batch_size: int, mu, sigma, inv_sigma, has_nan):
    """sklearn IncrementalPCA(n_components, batch_size).fit_transform on the preprocessed data, batch by batch as
    partial_fit does (S/markov_state_model/reduction.py:69-73): the SVD of
    [singular values x components | centred batch | mean correction] is taken through its F x F Gram matrix --
    the batch's second moments come from the matrix-core moments kernel (one segment per batch, the frames stay on the
    device), the F x F eigenproblem from the device Jacobi solver; signs as svd_flip(u_based_decision=False)."""
    sd = sigma.to_host()
    comps = np.zeros((0, F))
    sv = np.zeros((0,))
    mean = np.zeros(F)
    seen = 0
    for a, b in _gen_batches(n, batch_size, n_components):
        mom = pipe.tica_moments(xd, 0, mu, segments=[(a, b)], assume_finite=not has_nan, symmetric=True).to_host()
        nb = b - a
        S = 0.5 * mom[:F * F].reshape(F, F) / np.outer(sd, sd)          # sum z z' of the batch
        sz = mom[2 * F * F:2 * F * F + F] / sd                            # sum z
        mb = sz / nb
        total = seen + nb
        gram = S - nb * np.outer(mb, mb)                                  # centred about the batch mean
        if seen:
            corr = np.sqrt((seen / total) * nb) * (mean - mb)
            gram = gram + (comps.T * (sv ** 2)) @ comps + np.outer(corr, corr)
        gram = 0.5 * (gram + gram.T)
        w, V, _ = eng.eigh(eng.to_device(np.ascontiguousarray(gram)))
        w, V = w.to_host(), V.to_host()
        order = np.argsort(-w, kind="stable")[:n_components]
        vt = V[:, order].T
        vt = vt * np.sign(vt[np.arange(vt.shape[0]), np.argmax(np.abs(vt), axis=1)])[:, None]
        comps, sv = vt, np.sqrt(np.maximum(w[order], 0.0))
        mean = (seen * mean + sz) / total
        seen = total
    Wfull = np.zeros((F, F))
    Wfull[:, :n_components] = comps.T
    Y = eng.project(xd, mu, inv_sigma, eng.to_device(Wfull), n_components, mean2=eng.to_device(mean))
    return np.asarray(Y.to_host(), dtype=float)


def pca_reduce(X: np.ndarray, n_components: int = 2, batch_size: Optional[int] = None, scale: bool = True) -> np.ndarray:
    """_preprocess + sklearn PCA(n_components).fit_transform (S/markov_state_model/reduction.py:43-74) on the
    GPU: second moments on the matrix cores (lag 0), Jacobi eigendecomposition of the F x F covariance
    (sklearn's covariance_eigh solver: ddof = 1, components by descending variance, each component's
    largest-magnitude loading made positive), projection on the matrix cores.  With ``batch_size`` the reference
    switches to IncrementalPCA: `_incremental_pca` walks the same batches."""
    if batch_size is not None:
        Xm = _as_matrix(X)
        n, F = Xm.shape
        n_components, batch_size = int(n_components), int(batch_size)
        if not 1 <= n_components <= F:
            raise ValueError(f"n_components={n_components} invalid for n_features={F}, need more rows than columns for "
                             "IncrementalPCA processing")
        if n_components > batch_size or n_components > n:
            raise ValueError(f"n_components={n_components} must be less or equal to the batch number of samples "
                             f"{min(batch_size, n)}")
        eng = get_engine()
        pipe = MSMPipeline(eng)
        xd = eng.to_device(Xm)
        mu, sigma, inv_sigma, has_nan = pipe.standardise_params(xd, scale=scale)
        return _incremental_pca(eng, pipe, xd, n, F, n_components, batch_size, mu, sigma, inv_sigma, has_nan)
    Xm = _as_matrix(X)
    n, F = Xm.shape
    n_components = int(n_components)
    if not 1 <= n_components <= min(n, F):
        raise ValueError(f"n_components={n_components} must be between 1 and min(n_samples, n_features)={min(n, F)}")
    eng = get_engine()
    pipe = MSMPipeline(eng)
    xd = eng.to_device(Xm)
    mu, sigma, inv_sigma, has_nan = pipe.standardise_params(xd, scale=scale)
    mom = pipe.tica_moments(xd, 0, mu, assume_finite=not has_nan, symmetric=True).to_host()
    sd = sigma.to_host()
    S = 0.5 * mom[:F * F].reshape(F, F)                      # sum (x - mu)(x - mu)'
    delta = mom[2 * F * F:2 * F * F + F] / float(n)          # residual mean of the centred data (~1e-17)
    C = (S - n * np.outer(delta, delta)) / np.outer(sd, sd) / max(n - 1, 1)
    C = 0.5 * (C + C.T)
    w, V, _ = eng.eigh(eng.to_device(C))
    w, V = w.to_host(), V.to_host()
    order = np.argsort(-w, kind="stable")[:n_components]
    comps = V[:, order]
    top = np.argmax(np.abs(comps), axis=0)
    comps = comps * np.sign(comps[top, np.arange(comps.shape[1])])[None, :]
    Wfull = np.zeros((F, F))
    Wfull[:, :n_components] = comps
    # z - mean(z): the preprocessed columns are centred up to rounding; fold the residual in as mean2
    mean2 = eng.to_device(delta / sd)
    Y = eng.project(xd, mu, inv_sigma, eng.to_device(Wfull), n_components, mean2=mean2)
    return np.asarray(Y.to_host(), dtype=float)


def _whitener(eng, C: np.ndarray, epsilon: float) -> np.ndarray:
    """deeptime's spd_inv_split: C = V S V' (device Jacobi), keep s > epsilon, L = V S^-1/2 with the
    largest-magnitude entry of every column made positive."""
    w, V, _ = eng.eigh(eng.to_device(0.5 * (C + C.T)))
    w, V = w.to_host(), V.to_host()
    order = np.argsort(-w, kind="stable")
    w, V = w[order], V[:, order]
    keep = w > epsilon
    if not keep.any():
        raise ValueError("VAMP: covariance matrix has zero rank")
    V = V[:, keep]
    V = V * np.sign(V[np.argmax(np.abs(V), axis=0), np.arange(V.shape[1])])[None, :]
    return V / np.sqrt(w[keep])[None, :]


def vamp_reduce(X: np.ndarray, lag: int = 1, n_components: int = 2, scale: bool = True,
                epsilon: float = 1e-6) -> np.ndarray:
    """_preprocess + deeptime VAMP(lagtime, dim, epsilon).fit([X_prep]).transform(X_prep)
    (S/markov_state_model/reduction.py:113-148), restated from the published estimator (Wu & Noe,
    J. Nonlinear Sci. 30, 2020; deeptime 0.4.5 is absent: parity unpinned):

      C00 = cov(X[:-lag]), Ctt = cov(X[lag:]), C0t = cross-covariance (window means removed, 1/T),
      K = L0' C0t Lt with the whiteners L = V S^-1/2 of C00 / Ctt (eigenvalues <= epsilon dropped),
      K = U' S W'; the transform is the left singular functions (x - mean0) L0 U'[:, :dim].

    On the device: both moment passes over the frames (fp64 matrix cores), the Jacobi eigensolves of C00,
    Ctt and K K', the projection of all frames.  The F x F glue between them is host arithmetic.  Signs:
    the largest-magnitude loading of every component is positive (LAPACK's SVD signs are arbitrary)."""
    Xm = _as_matrix(X)
    n, F = Xm.shape
    lag = int(lag)
    if lag < 1 or n <= lag:
        raise ValueError(f"VAMP needs 1 <= lag < n_frames (lag={lag}, n_frames={n})")
    eng = get_engine()
    pipe = MSMPipeline(eng)
    xd = eng.to_device(Xm)
    mu, sigma, inv_sigma, has_nan = pipe.standardise_params(xd, scale=scale)
    both = pipe.tica_moments(xd, lag, mu, assume_finite=not has_nan).to_host()
    head = pipe.tica_moments(xd, 0, mu, segments=[(0, n - lag)], assume_finite=not has_nan).to_host()
    sd = sigma.to_host()
    T = float(both[-1])
    S00 = 0.5 * head[:F * F].reshape(F, F)                       # sum over X[:-lag] of z z'
    Stt = both[:F * F].reshape(F, F) - S00                       # the remainder: sum over X[lag:]
    S0t = both[F * F:2 * F * F].reshape(F, F)
    m0 = both[2 * F * F:2 * F * F + F] / T
    mt = both[2 * F * F + F:2 * F * F + 2 * F] / T
    norm = np.outer(sd, sd)
    C00 = (S00 / T - np.outer(m0, m0)) / norm
    Ctt = (Stt / T - np.outer(mt, mt)) / norm
    C0t = (S0t / T - np.outer(m0, mt)) / norm
    L0, Lt = _whitener(eng, C00, epsilon), _whitener(eng, Ctt, epsilon)
    K = L0.T @ C0t @ Lt
    w, U, _ = eng.eigh(eng.to_device(np.ascontiguousarray(K @ K.T)))      # left singular vectors of K
    order = np.argsort(-w.to_host(), kind="stable")
    dim = int(min(n_components, L0.shape[1], Lt.shape[1]))
    comps = L0 @ U.to_host()[:, order[:dim]]
    comps = comps * np.sign(comps[np.argmax(np.abs(comps), axis=0), np.arange(dim)])[None, :]
    Wfull = np.zeros((F, F))
    Wfull[:, :dim] = comps
    Y = eng.project(xd, mu, inv_sigma, eng.to_device(Wfull), dim, mean2=eng.to_device(m0 / sd))
    return np.asarray(Y.to_host(), dtype=float)


def reduce_features(X: np.ndarray, method: str = "pca", n_components: int = 2, lag: int = 1, scale: bool = True,
                    **kwargs) -> np.ndarray:
    """Unified interface (reduction.py:152-197): "pca" (default, as in the reference), "tica", "vamp"."""
    method = str(method).lower()
    if method == "pca":
        return pca_reduce(X, n_components=n_components, scale=scale, **kwargs)
    if method == "tica":
        return tica_reduce(X, lag=lag, n_components=n_components, scale=scale, **kwargs)
    if method == "vamp":
        return vamp_reduce(X, lag=lag, n_components=n_components, scale=scale, **kwargs)
    raise ValueError(f"Unknown reduction method: {method}")


def tica_fit_transform_trajectories(features: np.ndarray, traj_lengths: Sequence[int], n_components_hint: int,
                                    lag: int) -> tuple[np.ndarray, TicaModel]:
    """_maybe_apply_tica: dims clamped to [2, 5], fit on the list of trajectories (no
    standardisation there), transform each, drop the last ``lag`` frames of each, vstack."""
    n_components = int(max(2, min(5, n_components_hint)))
    drop = int(max(0, lag or 0))          # lag 0: fitted at lag 1, nothing dropped (_features.py:200, 216-231)
    lag = int(max(1, lag or 1))
    Xm = _as_matrix(features)
    edges = np.concatenate([[0], np.cumsum([int(v) for v in traj_lengths])])
    if edges[-1] != Xm.shape[0]:
        raise ValueError("trajectory lengths do not add up to the number of feature rows")
    segs = [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
    eng = get_engine()
    pipe = MSMPipeline(eng)
    xd = eng.to_device(Xm)
    # deeptime removes the data mean itself; no scaling: sigma = 1
    mu, _, _, has_nan = pipe.standardise_params(xd, scale=False)
    one = eng.to_device(np.ones(Xm.shape[1]))
    mom = pipe.tica_moments(xd, lag, mu, segments=segs, assume_finite=not has_nan, symmetric=True)
    model = pipe.tica_solve(mom, mu, one, one, lag, n_components, all_pairs=True)   # the model goes to the caller whole
    model.dim = min(n_components, int(model.rank.to_host()[0]))
    Y = pipe.tica_transform(model, xd, assume_finite=not has_nan).to_host()
    keep: List[np.ndarray] = []
    for a, b in segs:
        keep.append(Y[a:b - drop] if b - a > drop else np.empty((0, Y.shape[1])))
    return (np.vstack(keep) if keep else Y), model
