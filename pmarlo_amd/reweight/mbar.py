"""MBAR (Shirts & Chodera, J. Chem. Phys. 129, 124105, 2008) on the device: the solver's driver and the ladder case.

The matrix of reduced potentials stays on the device.  Per iteration one streaming pass (Engine.mbar_pass) reduces it
to s [K], G [K, K] and the objective; the reduced Newton system is built and solved there too, and only those
O(K^2) bytes cross to the host, which does the line search bookkeeping.  The path is fixed ("MBAR frame
weights"), so that another implementation of the same contract takes the same number of passes.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import numpy as np

from .. import _lib
from ..analysis.fes import BOLTZMANN_CONSTANT_KJ_PER_MOL
from ..device import DeviceArray, Engine, get_engine

__all__ = ["MBARResult", "mbar", "temperature_weights"]

_ULP = 2.0 ** -52
_ARMIJO = 1e-4
_MIN_STEP = 2.0 ** -20
_SLACK_ULPS = 64.0      # rounding slack of the Armijo test, in ulp of the magnitudes Phi is summed from


@dataclass
class MBARResult:
    f_k: np.ndarray                      # [K] free energies of the sampled states, f_0 = 0
    log_denominator: DeviceArray         # [N] d_n = logsumexp_k (f_k + ln N_k - u_kn), on the device
    n_iterations: int
    n_passes: int
    residual: float                      # max_k |N_k (s_k - 1)| / N at f_k
    target_f: np.ndarray | None = None   # [T]
    weights: np.ndarray | None = None    # [T, N], every row sums to 1
    ess: np.ndarray | None = None        # [T] Kish effective sample sizes


def _on_device(eng: Engine, a: Any, what: str) -> DeviceArray:
    if isinstance(a, DeviceArray):
        if a.dtype not in (np.float32, np.float64) or len(a.shape) != 2:
            raise ValueError(f"{what} must be a float32 / float64 [states, frames] matrix")
        return a
    arr = np.asarray(a)
    if arr.ndim == 1:
        arr = arr[None, :]
    if arr.ndim != 2:
        raise ValueError(f"{what} must be a [states, frames] matrix, got shape {arr.shape}")
    if arr.dtype != np.float32:
        arr = arr.astype(np.float64, copy=False)
    return eng.to_device(np.ascontiguousarray(arr))


def mbar(u_kn, N_k, *, targets=None, tol: float = 1e-10, maxiter: int = 100, engine: Engine | None = None) -> MBARResult:
    """Solve the MBAR equations for reduced potentials u_kn [K, N] (host array or DeviceArray, float32 / float64;
    frames grouped by the state that drew them, N_k[k] of them from state k) and, with `targets` [T, N], evaluate
    unsampled states.  +inf potentials are allowed.  ValueError: N_k that do not sum to N, a sampled state without
    frames, NaN or -inf potentials, a frame forbidden in every state.  RuntimeError: no convergence to
    max_k |N_k (s_k - 1)| / N <= tol within `maxiter` iterations (self-consistent and Newton steps alike)."""
    eng = engine if engine is not None else get_engine()
    u = _on_device(eng, u_kn, "u_kn")
    K, N = u.shape
    counts = np.asarray(N_k)
    if counts.shape != (K,) or not np.all(counts == np.floor(counts)):
        raise ValueError(f"N_k must hold {K} whole numbers, one per row of u_kn")
    counts = counts.astype(np.int64)
    if (counts <= 0).any():
        raise ValueError(f"every sampled state needs frames: N_k[{int(np.argmax(counts <= 0))}] is not positive")
    if int(counts.sum()) != N:
        raise ValueError(f"N_k sums to {int(counts.sum())}, u_kn has {N} frames")
    if K > _lib.MBAR_MAX_K:
        raise NotImplementedError(f"mbar: {K} sampled states, at most {_lib.MBAR_MAX_K} are supported")
    Nk = counts.astype(np.float64)
    Nk_d, lnN_d = eng.to_device(Nk), eng.to_device(np.log(Nk))
    f_d = eng.empty((K,), np.float64)
    passes = 0

    def run(f, want_gram, want_logden=True):
        # -> (s on the host, G, obj, s on the device, d_n): d_n travels with every pass that can become the last one
        nonlocal passes
        passes += 1
        f_d.copy_from_host(f)
        r = eng.mbar_pass(u, f_d, lnN_d, want_gram=want_gram, want_logden=want_logden)
        return r["s"].to_host(), r["G"], float(r["obj"].to_host()[0]), r["s"], r["logden"]

    off = np.concatenate([[0], np.cumsum(counts)])
    mean = eng.mbar_state_means(u, off).to_host()
    if not np.isfinite(mean).all():
        eng.mbar_pass(u, eng.zeros((K,), np.float64), lnN_d, want_gram=False, want_logden=False)   # names NaN / -inf
        raise ValueError("mbar: a state's own frames hold a non-finite reduced potential")
    f = mean - mean[0]
    it = 0
    s, G, obj, s_d, logden = run(f, False)
    while True:
        g = Nk * (s - 1.0)
        residual = float(np.abs(g).max() / N)
        if residual <= tol:
            break
        if it >= maxiter:
            raise _lib.MsmError(f"mbar: residual {residual:.3e} > tol {tol:.1e} after {it} iterations (MSM_ERR_NOCONV)")
        it += 1
        if it <= 2:                                    # self-consistent step, re-gauged
            f = f - np.log(s)
            f = f - f[0]
            s, G, obj, s_d, logden = run(f, it >= 2)
            continue
        if K < 2:
            raise _lib.MsmError("mbar: a single state did not converge")
        x = eng.mbar_newton_step(s_d, G, Nk_d)
        slope = float(np.dot(g[1:], x))
        phi0 = obj - float(np.dot(Nk, f))
        scale = abs(obj) + float(np.dot(Nk, np.abs(f)))
        alpha = 1.0
        while True:
            trial = f.copy()
            trial[1:] -= alpha * x
            first = alpha == 1.0                       # the full step carries the Gram matrix: it is the next pass
            s_t, G_t, obj_t, s_td, logden_t = run(trial, first, first)
            if obj_t - float(np.dot(Nk, trial)) <= phi0 - _ARMIJO * alpha * slope + _SLACK_ULPS * _ULP * scale:
                break
            alpha *= 0.5
            if alpha < _MIN_STEP:
                raise _lib.MsmError("mbar: the line search failed (step below 2^-20)")
        f = trial
        if first:
            s, G, obj, s_d, logden = s_t, G_t, obj_t, s_td, logden_t
        else:
            s, G, obj, s_d, logden = run(f, True)
    res = MBARResult(f_k=f, log_denominator=logden, n_iterations=it, n_passes=passes, residual=residual)
    if targets is not None:
        ut = _on_device(eng, targets, "targets")
        if ut.shape[1] != N:
            raise ValueError(f"targets must have {N} frames per row, got {ut.shape[1]}")
        ft, w, ess = eng.mbar_weights(ut, logden)
        res.target_f, res.weights, res.ess = ft.to_host(), w.to_host(), ess.to_host()
    return res


def temperature_weights(energies, state_index, temperatures_K, target_temperature_K, *, bias=None, tol: float = 1e-10,
                        maxiter: int = 100, engine: Engine | None = None, return_result: bool = False):
    """Weights that carry the frames of a temperature ladder to `target_temperature_K`.

    energies [N] (kJ / mol), one potential energy per frame; state_index [N] the rung that drew the frame, into
    temperatures_K [K]; bias [K, N] (kJ / mol, optional) the bias energy of frame n under rung k's bias.  Frames may
    come in any order; the weights [N] come back in the caller's order and sum to 1.  Rungs no frame was drawn from
    are left out of the solve.  u_kn = (E_n + bias_kn) / (k_B T_k) is built on the device."""
    eng = engine if engine is not None else get_engine()
    E = np.asarray(energies, np.float64).reshape(-1)
    idx = np.asarray(state_index).reshape(-1)
    T = np.asarray(temperatures_K, np.float64).reshape(-1)
    if idx.shape != E.shape:
        raise ValueError(f"state_index has {idx.size} entries, energies {E.size}")
    if E.size == 0:
        raise ValueError("temperature_weights: no frames")
    if not np.all(idx == np.floor(idx)) or idx.min() < 0 or idx.max() >= T.size:
        raise ValueError(f"state_index must hold whole numbers in [0, {T.size})")
    if not (np.isfinite(T).all() and (T > 0).all() and np.isfinite(target_temperature_K) and target_temperature_K > 0):
        raise ValueError("temperatures must be positive and finite")
    idx = idx.astype(np.int64)
    B = None
    if bias is not None:
        B = np.asarray(bias, np.float64)
        if B.shape != (T.size, E.size):
            raise ValueError(f"bias must have shape {(T.size, E.size)}, got {B.shape}")
    # frames grouped by rung and, inside a rung, ordered by their own values: the order the sums are taken in, and
    # with it every bit of the result, does not depend on the order the caller passes the frames in
    keys = ([] if B is None else [B[k] for k in range(T.size - 1, -1, -1)]) + [E, idx]
    order = np.lexsort(keys)
    counts = np.bincount(idx, minlength=T.size)
    used = np.nonzero(counts)[0]
    beta = 1.0 / (BOLTZMANN_CONSTANT_KJ_PER_MOL * T[used])
    E_d = eng.to_device(E[order])
    bias_d = None
    if B is not None:
        bias_d = eng.to_device(np.ascontiguousarray(B[used][:, order]))
    u = eng.mbar_reduced_potentials(E_d, beta, bias_d)
    ut = eng.mbar_reduced_potentials(E_d, [1.0 / (BOLTZMANN_CONSTANT_KJ_PER_MOL * float(target_temperature_K))])
    res = mbar(u, counts[used], targets=ut, tol=tol, maxiter=maxiter, engine=eng)
    w = np.empty(E.size, np.float64)
    w[order] = res.weights[0]
    return (w, res) if return_result else w
