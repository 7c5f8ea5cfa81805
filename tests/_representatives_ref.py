"""Seeded inputs and a plain numpy restatement of the four representative-picking methods.

The restatement follows the definitions, not the device code: np.where groups, weighted centroid
sum(w x) / sum(w), direct-difference Euclidean distances, medoid score sum_j w^_j |x_i - x_j| with
w^ = w / sum(w) (1 / n without weights).  Tie rule: equal scores go to the lowest frame; the two smallest-n
methods return ascending (score, frame); `diverse` is the max-min walk with np.argmin / np.argmax."""

from __future__ import annotations

import numpy as np

METHODS = ("closest_to_centroid", "true_medoid", "diverse")

# (name, N, d, k, trajectory lengths, weighted, n_reps): the golden cases
GOLDEN_CASES = (
    ("n600_d3_plain", 600, 3, 7, (250, 1, 349), False, 1),
    ("n600_d3_weighted", 600, 3, 7, (250, 1, 349), True, 4),
    ("n2500_d10_weighted", 2500, 10, 5, (2500,), True, 3),
    ("n900_d65_plain", 900, 65, 4, (400, 500), False, 2),
)


def make_case(N, d, k, lengths, weighted, seed=7):
    """Gaussian clusters whose centres are 3 sigma draws; state k // 2 is emptied and left out of state_ids."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, k, size=N)
    centres = 3.0 * rng.standard_normal((k, d))
    x = centres[labels] + rng.standard_normal((N, d))
    weights = rng.random(N) + 0.1 if weighted else None
    gone = k // 2
    if k > 1:
        labels[labels == gone] = (gone + 1) % k
    state_ids = [s for s in range(k) if s != gone or k == 1]
    assert sum(lengths) == N
    dtrajs = np.split(labels.astype(np.int64), np.cumsum(lengths)[:-1])
    return x, dtrajs, state_ids, weights


def golden_case(name):
    for case in GOLDEN_CASES:
        if case[0] == name:
            _, N, d, k, lengths, weighted, n_reps = case
            return make_case(N, d, k, lengths, weighted) + (n_reps,)
    raise KeyError(name)


# ---- the restatement ---------------------------------------------------------------------------------------
def state_weights(weights, frames):
    if weights is None:
        return np.full(len(frames), 1.0 / len(frames))
    w = np.asarray(weights, dtype=np.float64)[frames]
    return w / w.sum()


def centroid(xs, weights, frames):
    w = np.ones(len(frames)) if weights is None else np.asarray(weights, dtype=np.float64)[frames]
    return (w[:, None] * xs).sum(axis=0) / w.sum()


def distances(xs, point):
    diff = xs - point
    return np.sqrt((diff * diff).sum(axis=1))


def centroid_scores(x, frames, weights):
    xs = np.asarray(x, dtype=np.float64)[frames]
    return distances(xs, centroid(xs, weights, frames))


def medoid_scores(x, frames, weights):
    xs = np.asarray(x, dtype=np.float64)[frames]
    w = state_weights(weights, frames)
    return np.array([np.sum(w * distances(xs, xs[i])) for i in range(len(frames))])


def smallest(scores, frames, n):
    order = np.lexsort((frames, scores))
    return [int(frames[i]) for i in order[:min(n, len(frames))]]


def diverse_walk(x, frames, weights, n, margins=None, start=None):
    """`start`: a frame to begin the walk from in place of the member nearest the centroid."""
    xs = np.asarray(x, dtype=np.float64)[frames]
    dist = centroid_scores(x, frames, weights)
    picked = [int(np.argmin(dist)) if start is None else int(np.searchsorted(frames, start))]
    if margins is not None and len(frames) > 1:
        two = np.sort(dist)[:2]
        margins.append(_gap(two[0], two[1]))
    mind = np.full(len(frames), np.inf)
    for _ in range(min(n, len(frames)) - 1):
        mind = np.minimum(mind, distances(xs, xs[picked[-1]]))
        mind[picked] = -np.inf
        if margins is not None and len(frames) - len(picked) > 1:
            two = np.sort(mind)[-2:]
            margins.append(_gap(two[0], two[1]))
        picked.append(int(np.argmax(mind)))
    return [int(frames[i]) for i in picked]


def _gap(lo, hi):
    return float((hi - lo) / hi) if hi > 0 else 0.0


def selection_margin(scores, n):
    """Relative gap between the n-th smallest score and the next (inf when the whole state is taken)."""
    if n >= len(scores):
        return np.inf
    s = np.sort(scores)
    return _gap(s[n - 1], s[n])


def ordering_margin(scores, n):
    """Smallest relative gap between neighbours among the n + 1 smallest scores: below it the ORDER of the picks is
    undecided (1-D medoid scores of an even-sized state are equal at the two medians, whatever the rounding does)."""
    s = np.sort(scores)[:n + 1]
    return min((_gap(a, b) for a, b in zip(s[:-1], s[1:])), default=np.inf)


def scores_of(x, labels, state, weights, method):
    frames = np.where(np.asarray(labels) == state)[0]
    return medoid_scores(x, frames, weights) if method == "true_medoid" else centroid_scores(x, frames, weights)


def pick(x, dtrajs, state_ids, weights=None, n_reps=1, method="closest_to_centroid", margins=None):
    """[(state, global frame, trajectory, local frame)], state by state in the order of state_ids."""
    labels = np.concatenate([np.asarray(t) for t in dtrajs])
    lengths = [len(t) for t in dtrajs]
    traj = np.repeat(np.arange(len(dtrajs)), lengths)
    local = np.arange(len(labels)) - np.repeat(np.cumsum([0] + lengths[:-1]), lengths)
    out = []
    for s in state_ids:
        frames = np.where(labels == s)[0]
        if frames.size == 0:
            raise ValueError(f"No frames found for state {s}")
        if method == "diverse":
            got = diverse_walk(x, frames, weights, n_reps, margins)
        else:
            sc = medoid_scores(x, frames, weights) if method == "true_medoid" else centroid_scores(x, frames, weights)
            if margins is not None:
                margins.append(selection_margin(sc, n_reps))
            got = smallest(sc, frames, n_reps)
        out += [(int(s), g, int(traj[g]), int(local[g])) for g in got]
    return out


def by_state(reps):
    groups: dict = {}
    for s, g, _, _ in reps:
        groups.setdefault(int(s), []).append(int(g))
    return groups
