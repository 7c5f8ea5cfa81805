"""numpy restatement of the trajectory bootstrap (pmarlo_amd.conformations.uncertainty) and test trajectories for it.

The three bootstrap methods follow the rules the module states: the reference's draw order from one generator,
sliding counts per trajectory (npport._pair_counts), T = C / rowsum with zero rows kept zero, pi from
npport.stationary_distribution, TPT from npport.reactive_flux, and the same drop rules (second-largest eigenvalue
modulus above 1 - 1e-9, non-finite pi; for TPT an empty count row or a singular committor system)."""

from __future__ import annotations

import numpy as np
import scipy.linalg
from scipy.sparse.csgraph import connected_components

from oracle import npport

BOLTZMANN_J_PER_K = 1.380649e-23
AVOGADRO_PER_MOL = 6.02214076e23


# ---- test trajectories ------------------------------------------------------------------------------------------
def metastable_T(n, seed, n_macro=4, coupling=0.02):
    """Row-stochastic matrix of n_macro metastable blocks (tests/test_gpu_tpt.py's _metastable_T with the weight of
    the cells between the blocks as a parameter)."""
    rng = np.random.default_rng(seed)
    n_macro = max(1, min(n_macro, n))
    C = rng.random((n, n)) * coupling
    per = n // n_macro
    for b in range(n_macro):
        s = slice(b * per, (b + 1) * per if b < n_macro - 1 else n)
        C[s, s] += rng.random((C[s, s].shape)) + 0.2
    return C / C.sum(axis=1, keepdims=True)


def simulate(T, n_frames, rng):
    cdf = np.cumsum(T, axis=1)
    cdf[:, -1] = 1.0
    u = rng.random(n_frames)
    x = np.empty(n_frames, np.int32)
    x[0] = int(u[0] * T.shape[0]) % T.shape[0]
    for t in range(1, n_frames):
        x[t] = np.searchsorted(cdf[x[t - 1]], u[t], side="right")
    return x


def well_posed(traj, k, lag):
    """No empty row and an irreducible count graph for this trajectory alone at this lag."""
    C = npport._pair_counts([traj], k, lag)
    return bool(C.sum(axis=1).min() > 0) and connected_components(C > 0, connection="strong")[0] == 1


def trajectories(k, n_traj, frames, seed, lags=(1,), coupling=0.02, palindrome=False, check=True):
    """n_traj trajectories of `frames` frames from a metastable chain on k states.  palindrome: every trajectory is
    followed by its own reversal (2 * frames frames), which makes its sliding counts symmetric at every lag, hence
    the estimated matrix reversible: what PCCA+ asks for.  check: assert that every single trajectory is well posed
    at every lag in `lags`; every resample is then, and the restated reference drops nothing."""
    T = metastable_T(k, seed, coupling=coupling)
    rng = np.random.default_rng(seed + 1)
    out = []
    for _ in range(n_traj):
        x = simulate(T, frames, rng)
        out.append(np.concatenate([x, x[::-1]]) if palindrome else x)
    if check:
        for x in out:
            for lag in lags:
                assert well_posed(x, k, lag), "choose other lengths / seeds: a single trajectory is not well posed"
    return out


# ---- the bootstrap ------------------------------------------------------------------------------------------------
def draw_resamples(rng, n_traj, n_boot):
    """Index lists in the reference's call order: n_traj scalar draws per sample, sample by sample."""
    return [[int(rng.integers(0, n_traj)) for _ in range(n_traj)] for _ in range(n_boot)]


def n_states(dtrajs):
    return int(max(int(np.max(d)) for d in dtrajs if np.size(d))) + 1


def rebuild_msm(dtrajs, k, lag):
    """(C, T, pi, unique): _rebuild_msm with the stationary vector from the oracle and the uniqueness rule."""
    C = npport._pair_counts(dtrajs, k, lag)
    rs = C.sum(axis=1, keepdims=True)
    rs[rs == 0] = 1.0
    T = C / rs
    if k == 1:
        return C, T, np.ones(1), True
    w = np.sort(np.abs(scipy.linalg.eigvals(T)))[::-1]
    pi = npport.stationary_distribution(T)
    return C, T, pi, bool(w[1] <= 1.0 - 1e-9) and bool(np.all(np.isfinite(pi)))


def _stats(samples, ci):
    a = np.array(samples)
    return {"mean": np.mean(a, axis=0), "std": np.std(a, axis=0), "ci_lower": np.percentile(a, ci[0], axis=0),
            "ci_upper": np.percentile(a, ci[1], axis=0), "n_samples": len(samples)}


def bootstrap_msms(dtrajs, n_boot, lag, rng):
    k = n_states(dtrajs)
    return [rebuild_msm([dtrajs[i] for i in idx], k, lag) for idx in draw_resamples(rng, len(dtrajs), n_boot)]


def bootstrap_tpt(dtrajs, source, sink, n_boot, lag, rng, ci=(2.5, 97.5)):
    """{"kept": mask, "rate" / "mfpt" / "total_flux": stats}; the stats are missing when every sample is dropped."""
    kept, rows = [], []
    for C, T, pi, unique in bootstrap_msms(dtrajs, n_boot, lag, rng):
        ok = unique and C.sum(axis=1).min() > 0
        if ok:
            try:
                f = npport.reactive_flux(T, pi, source, sink)
                rows.append([f["rate"], f["mfpt"], f["total_flux"]])
            except np.linalg.LinAlgError:
                ok = False
        kept.append(ok)
    out = {"kept": np.asarray(kept)}
    if rows:
        a = np.asarray(rows)
        out.update(rate=_stats(a[:, 0], ci), mfpt=_stats(a[:, 1], ci), total_flux=_stats(a[:, 2], ci))
    return out


def bootstrap_free_energies(dtrajs, T_K, n_boot, rng, ci=(2.5, 97.5)):
    kT = BOLTZMANN_J_PER_K * T_K * AVOGADRO_PER_MOL / 1000.0
    msms = bootstrap_msms(dtrajs, n_boot, 1, rng)
    kept = np.asarray([m[3] for m in msms])
    fe = [-kT * np.log(np.maximum(pi, 1e-10)) for _, _, pi, unique in msms if unique]
    return {"kept": kept, "free_energies": _stats(fe, ci) if fe else None}


def bootstrap_Tpi(dtrajs, n_boot, lag, rng):
    """The kept samples' (index, T, pi): what the macrostate bootstrap hands to PCCA+."""
    return [(b, T, pi) for b, (_, T, pi, unique) in enumerate(bootstrap_msms(dtrajs, n_boot, lag, rng)) if unique]
