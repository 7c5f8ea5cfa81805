"""TRAM (Wu, Paul, Wehmeyer, Noe, PNAS 113, E3221, 2016) on the device: multi-ensemble Markov models and frame weights.

MBAR treats every frame as an independent draw from its ensemble's equilibrium; TRAM assumes equilibrium only inside
a Markov state and couples the K ensembles through the bias energies and through one reversible Markov model per
ensemble.  The matrix of reduced potentials and the K count matrices stay on the device; an iteration is two row-sum
launches, one streaming pass and one update (Engine.tram_solve, csrc/tram.hip), and only one error word per check
interval crosses to the host.  The contract is in include/msmhip.h and DESIGN.md ("TRAM").
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Sequence

import numpy as np

from ..device import DeviceArray, Engine, get_engine
from ..markov_state_model.results import MSMEstimate

__all__ = ["TRAMResult", "tram", "tram_from_counts", "fragments", "largest_connected_set", "restrict_labels"]


@dataclass
class TRAMResult:
    f_ik: np.ndarray                     # [K, m] local free energies, min over the active pairs = 0; NaN: inactive
    log_v: np.ndarray                    # [K, m] log Lagrange multipliers (-inf where v = 0), NaN: inactive
    f_k: np.ndarray                      # [K] -logsumexp_i (-f_ik)
    active_set: np.ndarray               # [m] the caller's label of every Markov state of the model
    count_matrices: np.ndarray           # [K, m, m]
    state_counts: np.ndarray             # [K, m] N_i^k
    log_mu: DeviceArray                  # [N] -d_n in the caller's frame order, on the device (-inf: frame left out)
    n_iterations: int
    err: float
    n_markov_states: int                 # size of the caller's state space (>= m)
    target_f: np.ndarray | None = None   # [T]
    weights: np.ndarray | None = None    # [T, N], every row sums to 1
    ess: np.ndarray | None = None        # [T] Kish effective sample sizes
    target_state_f: np.ndarray | None = None   # [T, m] configurational free energies of the targets
    _device: dict = field(default_factory=dict, repr=False)

    def msm(self, k: int) -> MSMEstimate:
        """The reversible Markov model of sampled ensemble k, embedded in the caller's state space as
        finalize_transition_and_stationary embeds its own: T = I and pi = 0 outside the states active in k."""
        K = self.f_ik.shape[0]
        if not 0 <= int(k) < K:
            raise ValueError(f"k must be in [0, {K})")
        d = self._device
        eng: Engine = d["engine"]
        P = eng.tram_transition_matrices(d["S"], d["N"], d["f"], d["v"], int(k)).to_host()
        act = np.nonzero(self.state_counts[k] > 0)[0]
        full = self.active_set[act].astype(int)
        n = self.n_markov_states
        T, pi, cm = np.eye(n), np.zeros(n), np.zeros((n, n))
        T[np.ix_(full, full)] = P[np.ix_(act, act)]
        fk = self.f_ik[k, act]
        p = np.exp(-(fk - fk.min()))
        pi[full] = p / p.sum()
        cm[np.ix_(full, full)] = self.count_matrices[k][np.ix_(act, act)]
        return MSMEstimate(cm, T, pi, full)


# ---- the host logic of tram(), free of the device ------------------------------------------------------------------
def fragments(labels: np.ndarray, thermo: np.ndarray, lengths: Sequence[int], K: int) -> list[tuple[np.ndarray, np.ndarray]]:
    """Cuts the concatenated trajectories (`lengths` frames each) into maximal fragments of constant `thermo` and
    valid (>= 0) label -> for every ensemble k the (starts, stops) of its fragments, in frame coordinates."""
    labels, thermo = np.asarray(labels), np.asarray(thermo)
    n = labels.size
    out = []
    if n == 0:
        return [(np.zeros(0, np.int64), np.zeros(0, np.int64)) for _ in range(K)]
    valid = labels >= 0
    cut = np.zeros(n + 1, bool)                      # cut[t]: a fragment boundary in front of frame t
    cut[np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))])] = True
    cut[1:n] |= (thermo[1:] != thermo[:-1]) | (valid[1:] != valid[:-1])
    bounds = np.nonzero(cut)[0]
    starts, stops = bounds[:-1], bounds[1:]
    keep = valid[starts]
    starts, stops = starts[keep], stops[keep]
    for k in range(K):
        mine = thermo[starts] == k
        out.append((starts[mine].astype(np.int64), stops[mine].astype(np.int64)))
    return out


def largest_connected_set(total_counts: np.ndarray, visited: np.ndarray) -> np.ndarray:
    """The largest strongly connected set of the summed count matrix among the visited states (most states; the
    most frames, then the lowest label, between sets of equal size) -> ascending state labels."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    C = np.asarray(total_counts)
    visited = np.asarray(visited)
    seen = np.nonzero(visited > 0)[0]
    if seen.size == 0:
        return seen
    _, lab = connected_components(csr_matrix(C[np.ix_(seen, seen)] > 0), directed=True, connection="strong")
    size = np.bincount(lab)
    frames = np.bincount(lab, weights=visited[seen])
    first = np.full(size.size, seen.size)
    np.minimum.at(first, lab, np.arange(seen.size))
    best = np.lexsort((first, -frames, -size))[0]
    return seen[lab == best]


def restrict_labels(labels: np.ndarray, active: np.ndarray, n_states: int) -> np.ndarray:
    """Labels renumbered to 0 .. len(active) - 1; every other frame gets -1."""
    table = np.full(n_states + 1, -1, np.int64)      # the last slot takes the invalid labels
    table[np.asarray(active, np.int64)] = np.arange(len(active))
    labels = np.asarray(labels, np.int64)
    return table[np.where((labels >= 0) & (labels < n_states), labels, n_states)]


def _host_matrix(a: Any, what: str) -> np.ndarray:
    if isinstance(a, DeviceArray):
        a = a.to_host()
    elif isinstance(a, (list, tuple)):
        a = np.concatenate([np.atleast_2d(np.asarray(b)) for b in a], axis=1)
    arr = np.asarray(a)
    if arr.ndim == 1:
        arr = arr[None, :]
    if arr.ndim != 2:
        raise ValueError(f"{what} must be a [states, frames] matrix, got shape {arr.shape}")
    return arr if arr.dtype == np.float32 else arr.astype(np.float64, copy=False)


def _canonical_order(u: np.ndarray, state: np.ndarray, thermo: np.ndarray) -> np.ndarray:
    """Frames grouped by Markov state and ordered inside a state by the ensemble that drew them and their own values:
    the order the sums are taken in, and with it every bit of the result, does not depend on the caller's order."""
    own = u[thermo, np.arange(state.size)]
    order = np.lexsort((own, thermo, state))
    s, t, o = state[order], thermo[order], own[order]
    if ((s[1:] == s[:-1]) & (t[1:] == t[:-1]) & (o[1:] == o[:-1])).any():       # ties: all rows decide
        order = np.lexsort(tuple(u[k] for k in range(u.shape[0] - 1, -1, -1)) + (thermo, state))
    return order


def tram_from_counts(counts, u_kn, markov_state, thermo_state, *, targets=None, f0=None, tol: float = 1e-10,
                     maxiter: int = 100_000, check_every: int = 16, engine: Engine | None = None,
                     _full: tuple | None = None) -> TRAMResult:
    """Solve the TRAM equations for count matrices `counts` [K, m, m] (fp64, may be non-integer), reduced potentials
    u_kn [K, N] (+inf allowed), and per frame its Markov state and the ensemble that drew it; frames in any order.
    With `targets` [T, N], evaluate unsampled ensembles.  f0 [K] starts f_i^k at f0[k] (default 0; MBARResult.f_k
    is a good one).  ValueError: a Markov state without frames, col_i^k > N_i^k, counts where N_i^k = 0, negative
    counts, shapes that do not match, NaN or -inf in u, a frame forbidden in every ensemble that holds its state.
    MsmError: no convergence to max |f_new - f_old| <= tol within `maxiter` iterations."""
    eng = engine if engine is not None else get_engine()
    C = np.asarray(counts, np.float64)
    if C.ndim != 3 or C.shape[1] != C.shape[2]:
        raise ValueError(f"counts must have shape [K, m, m], got {C.shape}")
    K, m = C.shape[0], C.shape[1]
    u = _host_matrix(u_kn, "u_kn")
    state, thermo = np.asarray(markov_state).reshape(-1), np.asarray(thermo_state).reshape(-1)
    N = u.shape[1]
    if u.shape[0] != K or state.size != N or thermo.size != N:
        raise ValueError(f"shapes do not match: counts {C.shape}, u_kn {u.shape}, markov_state {state.size}, "
                         f"thermo_state {thermo.size}")
    if N == 0:
        raise ValueError("tram: no frames")
    if not (np.all(state == np.floor(state)) and np.all(thermo == np.floor(thermo))) or state.min() < 0 or \
            state.max() >= m or thermo.min() < 0 or thermo.max() >= K:
        raise ValueError(f"markov_state must hold whole numbers in [0, {m}) and thermo_state in [0, {K})")
    state, thermo = state.astype(np.int64), thermo.astype(np.int64)
    if np.isnan(u).any():
        raise ValueError("tram: the reduced potentials hold NaN")
    if not np.isfinite(C).all() or (C < 0).any():
        raise ValueError("tram: counts must be finite and not negative")
    per_state = np.bincount(state, minlength=m)
    if (per_state == 0).any():
        raise ValueError(f"tram: Markov state {int(np.argmax(per_state == 0))} has no frames")
    Nki = np.zeros((K, m))
    np.add.at(Nki, (thermo, state), 1.0)
    S, col = C + C.transpose(0, 2, 1), C.sum(axis=1)
    if ((S.sum(axis=2) > 0) & (Nki == 0)).any():
        k, i = np.argwhere((S.sum(axis=2) > 0) & (Nki == 0))[0]
        raise ValueError(f"tram: ensemble {k} has counts in Markov state {i} but drew no frame there")
    if (col > Nki * (1 + 1e-12)).any():
        k, i = np.argwhere(col > Nki * (1 + 1e-12))[0]
        raise ValueError(f"tram: ensemble {k} counts {col[k, i]} transitions into Markov state {i} "
                         f"but drew {int(Nki[k, i])} frames there")
    col = np.minimum(col, Nki)
    ut = None
    if targets is not None:
        ut = _host_matrix(targets, "targets")
        if ut.shape[1] != N:
            raise ValueError(f"targets must have {N} frames per row, got {ut.shape[1]}")
    f = np.zeros((K, m))
    if f0 is not None:
        f0 = np.asarray(f0, np.float64).reshape(-1)
        if f0.shape != (K,) or not np.isfinite(f0).all():
            raise ValueError(f"f0 must hold {K} finite numbers")
        f += f0[:, None]

    order = _canonical_order(u, state, thermo)
    tables = eng.tram_tables(np.concatenate([[0], np.cumsum(per_state)]))
    u_d = eng.to_device(np.ascontiguousarray(u[:, order]))
    S_d, N_d, col_d = eng.to_device(S), eng.to_device(Nki), eng.to_device(col)
    f_d, v_d = eng.to_device(f), eng.to_device(S.sum(axis=2) / 2)
    sol = eng.tram_solve(u_d, tables, S_d, N_d, col_d, f_d, v_d, tol=tol, maxiter=maxiter, check_every=check_every)

    act = Nki > 0
    f_ik, v = f_d.to_host(), v_d.to_host()
    with np.errstate(divide="ignore"):
        log_v = np.where(act, np.log(np.where(v > 0, v, 1.0)), np.nan)
        log_v[act & (v == 0)] = -np.inf
    f_ik = np.where(act, f_ik, np.nan)
    f_k = np.array([-_logsumexp(-f_ik[k, act[k]]) if act[k].any() else np.inf for k in range(K)])
    n_full, frames, active_set = (N, np.arange(N), np.arange(m)) if _full is None else _full
    d = np.full(n_full, np.inf)
    d[frames[order]] = sol["logden"].to_host()
    res = TRAMResult(f_ik=f_ik, log_v=log_v, f_k=f_k, active_set=np.asarray(active_set), count_matrices=C,
                     state_counts=Nki, log_mu=eng.to_device(-d), n_iterations=sol["n_iterations"], err=sol["err"],
                     n_markov_states=m,
                     _device={"engine": eng, "S": S_d, "N": N_d, "f": f_d, "v": v_d})
    if ut is not None:
        ft, w, ess = eng.mbar_weights(eng.to_device(np.ascontiguousarray(ut[:, order])), sol["logden"])
        w = w.to_host()
        res.target_f, res.ess = ft.to_host(), ess.to_host()
        with np.errstate(divide="ignore"):
            res.target_state_f = res.target_f[:, None] - np.log(np.add.reduceat(w, tables["host_offsets"][:-1], axis=1))
        res.weights = np.zeros((ut.shape[0], n_full))
        res.weights[:, frames[order]] = w
    return res


def _logsumexp(a: np.ndarray) -> float:
    mx = a.max()
    return float(mx + np.log(np.exp(a - mx).sum()))


def tram(dtrajs, ttrajs, u_kn, lag: int, *, n_markov_states: int | None = None, targets=None, f0=None,
         tol: float = 1e-10, maxiter: int = 100_000, check_every: int = 16, engine: Engine | None = None) -> TRAMResult:
    """TRAM from trajectories: dtrajs and ttrajs are lists of equal-length integer arrays (Markov state, negative:
    unassigned; ensemble the frame was drawn in), u_kn one [K, N] matrix over the concatenated frames or a list of
    [K, N_t] blocks.  A pair (t, t + lag) is counted in C^k only inside a maximal fragment of constant ttraj = k and
    valid label (the device count kernel, one call per ensemble).  The Markov states are then restricted to the
    largest strongly connected set of sum_k C^k; frames outside get weight 0 and break fragments, and the counts are
    rebuilt once on the restricted labels.  The rest is tram_from_counts."""
    eng = engine if engine is not None else get_engine()
    if len(dtrajs) != len(ttrajs) or not len(dtrajs):
        raise ValueError("tram needs as many ttrajs as dtrajs, and at least one")
    lengths = [np.asarray(d).size for d in dtrajs]
    if any(np.asarray(t).size != n for t, n in zip(ttrajs, lengths)):
        raise ValueError("every ttraj must be as long as its dtraj")
    if int(lag) < 1:
        raise ValueError("lag must be >= 1")
    labels = np.concatenate([np.asarray(d).reshape(-1) for d in dtrajs]).astype(np.int64)
    thermo = np.concatenate([np.asarray(t).reshape(-1) for t in ttrajs]).astype(np.int64)
    u = _host_matrix(u_kn, "u_kn")
    K, N = u.shape
    if labels.size != N:
        raise ValueError(f"u_kn has {N} frames, the trajectories {labels.size}")
    if N == 0 or thermo.min() < 0 or thermo.max() >= K:
        raise ValueError(f"ttrajs must hold ensemble indices in [0, {K})")
    n_states = int(labels.max()) + 1 if n_markov_states is None else int(n_markov_states)
    if n_states < 1 or labels.max() >= n_states:
        raise ValueError("no valid Markov state label" if n_states < 1 else
                         f"a label is outside [0, {n_states})")

    def count(lab: np.ndarray, m: int) -> np.ndarray:
        lab_d = eng.to_device(lab.astype(np.int32))
        C = np.zeros((K, m, m))
        for k, (starts, stops) in enumerate(fragments(lab, thermo, lengths, K)):
            long_enough = stops - starts > int(lag)
            if long_enough.any():
                out, _ = eng.count_transitions(lab_d, m, int(lag), starts=starts[long_enough], stops=stops[long_enough])
                C[k] = out.to_host()
        return C

    visited = np.bincount(labels[labels >= 0], minlength=n_states)
    C = count(labels, n_states)
    active = largest_connected_set(C.sum(axis=0), visited)
    if active.size == 0:
        raise ValueError("tram: no frame carries a valid Markov state label")
    restricted = labels
    if active.size < n_states:
        restricted = restrict_labels(labels, active, n_states)
        C = count(restricted, active.size)
    frames = np.nonzero(restricted >= 0)[0]
    ut = None
    if targets is not None:
        ut = _host_matrix(targets, "targets")
        if ut.shape[1] != N:
            raise ValueError(f"targets must have {N} frames per row, got {ut.shape[1]}")
        ut = ut[:, frames]
    res = tram_from_counts(C, u[:, frames], restricted[frames], thermo[frames], targets=ut, f0=f0, tol=tol,
                           maxiter=maxiter, check_every=check_every, engine=eng, _full=(N, frames, active))
    res.n_markov_states = n_states
    return res
