"""The laws, the seeded inputs and the C ABI wrappers of tests/test_gpu_rep_sil_paths.py (kernels of
pmarlo_amd/csrc/representatives.hip and silhouette.hip).

The laws are plain numpy in np.longdouble and follow the definitions of include/msmhip.h ("representative frames of a
state" and the two silhouette blocks), not the device code: np.where groups, centroid sum(w x) / sum(w), distances as
direct differences under the root, the medoid score sum_j w^_j |x_i - x_j|, the two selection rules, and the
silhouette coefficient with its NaN rule.  tests/test_rep_sil_paths_reference.py checks them on the CPU against the
fp64 restatements (_representatives_ref.py, _silhouette_ref.py) and against sklearn, measures what a plain fp64
evaluation loses against them (the yardstick of the GPU bounds), and asserts the margins that make an exact
comparison of picks meaningful.

NaN rules.
  selection   a NaN never wins a pick.  `smallest`: ascending (score, frame) over the members whose score is not NaN
              (+inf may be picked), -1 for the rest of the row.  `diverse`: start at the smallest non-NaN score (the
              first member if every score is NaN); mind_i = min(mind_i, |x_i - x_pick|) keeps NaN; the next pick is
              the largest non-NaN mind among the members not taken, the lowest frame on ties; -1 from the round on in
              which no such member is left.
  silhouette  a_i and the cluster means are ordinary IEEE sums; b_i is a NaN-propagating minimum over the other
              OCCUPIED clusters (occupancy from the counts); den = max(a_i, b_i) propagates NaN; s_i = 0 only for a
              singleton, where no other cluster is occupied and where den == 0; otherwise (b_i - a_i) / den.
"""

from __future__ import annotations

import functools

import numpy as np

from tests._silhouette_ref import recipe_labels, silhouette_samples_ref  # noqa: F401  (re-exported)

LD = np.longdouble
U = 2.0 ** -53
INT32_MAX = np.iinfo(np.int32).max
SIL_ATOL = 1e-10
SCORE_RTOL = 1e-10
MIN_MARGIN = 1e-6


# ---- the laws ------------------------------------------------------------------------------------------------------
def group_ref(labels, k):
    """(offsets int64 [k + 1], members int32 [offsets[k]]): np.where(labels == s) for s = 0 .. k-1 in turn."""
    labels = np.asarray(labels)
    want = [np.where(labels == s)[0] for s in range(k)]
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64)
    members = np.concatenate(want).astype(np.int32) if k else np.zeros(0, np.int32)
    return offsets, members


def centroid_law(x, frames, weights=None):
    """(sum(w x) / sum(w), sum(w)) in longdouble."""
    xs = np.asarray(x, LD)[frames]
    w = np.ones(len(frames), LD) if weights is None else np.asarray(weights, LD)[frames]
    ws = w.sum()
    return (w[:, None] * xs).sum(axis=0) / ws, ws


def distance_law(xs, point):
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.asarray(xs, LD) - np.asarray(point, LD)
        return np.sqrt((diff * diff).sum(axis=1))


def centroid_scores_law(x, frames, weights=None):
    return distance_law(np.asarray(x)[frames], centroid_law(x, frames, weights)[0])


def medoid_scores_law(x, frames, weights=None, rows=None):
    """sum_j w^_j |x_i - x_j| over the members j, for the member positions `rows` (all by default)."""
    xs = np.asarray(x, LD)[frames]
    w = np.ones(len(frames), LD) if weights is None else np.asarray(weights, LD)[frames]
    w = w / w.sum()
    rows = range(len(frames)) if rows is None else rows
    return np.array([np.sum(w * distance_law(xs, xs[i])) for i in rows], LD)


def smallest_law(scores, frames, n):
    """Row of n picks: ascending (score, frame) over the non-NaN scores, then -1."""
    scores = np.asarray(scores)
    frames = np.asarray(frames)
    ok = np.flatnonzero(~np.isnan(scores))
    order = ok[np.lexsort((frames[ok], scores[ok]))][:n]
    return [int(frames[i]) for i in order] + [-1] * (n - len(order))


def _rel_gap(lo, hi):
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return np.inf
    return float((hi - lo) / hi) if hi > 0 else (0.0 if hi == lo else np.inf)


def smallest_margin(scores, n):
    """Smallest relative gap between neighbours among the n + 1 smallest non-NaN scores."""
    s = np.sort(np.asarray(scores)[~np.isnan(scores)])[:n + 1]
    return min((_rel_gap(a, b) for a, b in zip(s[:-1], s[1:])), default=np.inf)


def diverse_law(x, frames, scores, n, margins=None, score_margin=True):
    """Row of n picks of the max-min walk from the smallest score; `margins` collects the relative gap between the two
    best candidates of every round (of the first round, the two smallest scores, only with `score_margin`: scores
    handed to the device as they are leave nothing to rounding)."""
    frames = np.asarray(frames)
    ns = len(frames)
    n_sel = min(n, ns)
    out = [-1] * n
    if n_sel == 0:
        return out
    xs = np.asarray(x, LD)[frames]
    scores = np.asarray(scores)
    ok = np.flatnonzero(~np.isnan(scores))
    first = int(ok[np.lexsort((ok, scores[ok]))][0]) if ok.size else 0
    if margins is not None and score_margin and ok.size > 1:
        two = np.sort(scores[ok])[:2]
        margins.append(_rel_gap(two[0], two[1]))
    taken = np.zeros(ns, bool)
    taken[first] = True
    out[0] = int(frames[first])
    mind = np.full(ns, np.inf, LD)
    sel = first
    for r in range(1, n_sel):
        dist = distance_law(xs, xs[sel])
        mind = np.where((dist < mind) | np.isnan(dist), dist, mind)
        cand = np.flatnonzero(~taken & ~np.isnan(mind))
        if cand.size == 0:
            break
        best = mind[cand].max()
        if margins is not None and cand.size > 1:
            two = np.sort(mind[cand])[-2:]
            margins.append(_rel_gap(two[0], two[1]))
        sel = int(cand[mind[cand] == best][0])
        taken[sel] = True
        out[r] = int(frames[sel])
    return out


def silhouette_law(X, labels, k):
    """s_i in longdouble under the NaN rule of the module docstring; labels in [0, k)."""
    X = np.asarray(X, LD)
    labels = np.asarray(labels).astype(np.int64)
    n, d = X.shape
    counts = np.bincount(labels, minlength=k)
    occupied = np.flatnonzero(counts > 0)
    order = np.argsort(labels, kind="stable")
    starts = (np.cumsum(counts) - counts)[occupied]
    col_of = np.full(k, -1, np.int64)
    col_of[occupied] = np.arange(occupied.size)
    Xs = X[order]
    out = np.zeros(n, LD)
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, n, 256):
            i1 = min(n, i0 + 256)
            d2 = np.zeros((i1 - i0, n), LD)
            for f in range(d):
                diff = X[i0:i1, f, None] - Xs[None, :, f]
                d2 += diff * diff
            sums = np.add.reduceat(np.sqrt(d2), starts, axis=1)
            rows = np.arange(i1 - i0)
            own = col_of[labels[i0:i1]]
            n_own = counts[labels[i0:i1]]
            a = sums[rows, own] / np.maximum(n_own - 1, 1)
            mean = sums / counts[occupied][None, :].astype(LD)
            mean[rows, own] = np.inf
            b = mean.min(axis=1)
            den = np.maximum(a, b)
            ok = (n_own > 1) & (occupied.size > 1) & ~(den == 0)
            out[i0:i1] = np.where(ok, (b - a) / np.where(ok, den, LD(1)), LD(0))
    return out


# ---- layouts -------------------------------------------------------------------------------------------------------
def strided(X, ld):
    """Rows `ld` apart, NaN in the padding columns."""
    X = np.asarray(X, np.float64)
    buf = np.full((X.shape[0], ld), np.nan, np.float64)
    buf[:, :X.shape[1]] = X
    return buf


def pow2_at_least(d):
    c = 1
    while c < d:
        c <<= 1
    return c


# ---- seeded inputs -------------------------------------------------------------------------------------------------
CENTROID_D = (1, 2, 3, 5, 64, 65, 255, 256)
MEDOID_D = (1, 7, 8, 9, 16, 17, 255, 256)
MEDOID_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 257)
JUNK_LABELS = (-1, None, INT32_MAX)   # None stands for k


def centroid_sizes(d):
    """0, 1, R - 1, R, R + 1, 1000 with R = 256 / cw row lanes (duplicates are separate states)."""
    r = 256 // pow2_at_least(d)
    return (0, 1, max(r - 1, 0), r, r + 1, 1000)


def score_sizes(d):
    """Centroid-mode scores: an empty state, one member, R + 1 members (a row-lane tail), and 256, 300 and 1000."""
    r = 256 // pow2_at_least(d)
    return (0, 1, r + 1, 256, 300, 1000)


@functools.lru_cache(maxsize=None)
def state_case(d, sizes, seed):
    """One state per entry of `sizes` (shuffled frames), labels -1, k and INT32_MAX sprinkled in (37 each), positive
    weights.  Returns (x [n, d], labels int32 [n], k, weights [n]), read-only."""
    rng = np.random.default_rng(seed)
    k = len(sizes)
    parts = [np.full(n, s, np.int64) for s, n in enumerate(sizes)]
    parts += [np.full(37, k if j is None else j, np.int64) for j in JUNK_LABELS]
    labels = np.concatenate(parts)
    rng.shuffle(labels)
    x = rng.standard_normal((labels.size, d)) + 2.0 * (labels[:, None] % 3)
    w = rng.random(labels.size) + 0.05
    labels = labels.astype(np.int32)
    for a in (x, labels, w):
        a.setflags(write=False)
    return x, labels, k, w


def group_labels(n, k, seed):
    """Labels for the grouping test: state 0 in every chunk of 1024 (its first frame), state k - 1 (k >= 3) only in
    the last chunk (its last frame, which in a chunk of one frame takes the place of state 0), state 1 (k >= 4)
    without a frame, -1, k and INT32_MAX mixed in."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, k, size=n).astype(np.int64)
    junk = rng.random(n)
    labels[junk < 0.02] = -1
    labels[(junk >= 0.02) & (junk < 0.04)] = k
    labels[(junk >= 0.04) & (junk < 0.06)] = INT32_MAX
    labels[[2, 3, 5]] = (-1, k, INT32_MAX)
    labels[np.arange(0, n, 1024)] = 0
    if k >= 3:
        labels[labels == k - 1] = 0
        labels[n - 1] = k - 1
    if k >= 4:
        labels[labels == 1] = 2
    return labels.astype(np.int32)


SELECT_SIZES = (0, 1, 2, 256, 257, 1000)
SELECT_REPS = (1, 3, 257, 600)
SELECT_D = 3


@functools.lru_cache(maxsize=None)
def select_case(seed=13):
    """300 states: two rounds of SELECT_SIZES, then 288 states of 1 .. 40 members; d = 3.  The scores are pre-set: a
    permutation of 1 + 1e-3 * (0 .. n_s - 1) per state, so the law orders them with gaps of about 1e-3.  The seed is the
    first of 3 .. 13 whose diverse walks of 600 rounds keep a margin above 3e-6 (5.5e-6) between the two best candidates."""
    rng = np.random.default_rng(seed)
    sizes = list(SELECT_SIZES) * 2 + [int(v) for v in rng.integers(1, 41, size=288)]
    k = len(sizes)
    labels = np.concatenate([np.full(n, s, np.int64) for s, n in enumerate(sizes)])
    rng.shuffle(labels)
    x = rng.standard_normal((labels.size, SELECT_D)) * 3.0
    offsets, members = group_ref(labels, k)
    scores = np.empty(labels.size)
    for s in range(k):
        ns = sizes[s]
        scores[offsets[s]:offsets[s + 1]] = 1.0 + 1e-3 * rng.permutation(ns)
    labels = labels.astype(np.int32)
    for a in (x, labels, scores, offsets, members):
        a.setflags(write=False)
    return x, labels, k, tuple(sizes), offsets, members, scores


def select_states(n_states):
    """The listed states of a select call: state 5 (1000 members) alone, or all 300 in a shuffled order."""
    if n_states == 1:
        return np.array([5], np.int32)
    return np.random.default_rng(n_states).permutation(300).astype(np.int32)


@functools.lru_cache(maxsize=None)
def select_rows(mode, n_reps, n_states):
    """The law's picks [n_states, n_reps] for select_case, and (diverse) the smallest margin met on the way."""
    x, _, _, _, offsets, members, scores = select_case()
    rows, margins = [], []
    for s in select_states(n_states):
        frames = members[offsets[s]:offsets[s + 1]]
        sc = scores[offsets[s]:offsets[s + 1]]
        if mode == "smallest":
            rows.append(smallest_law(sc, frames, n_reps))
            margins.append(smallest_margin(sc, n_reps))
        else:
            rows.append(diverse_law(x, frames, sc, n_reps, margins))
    return np.array(rows, np.int32).reshape(len(rows), n_reps), (min(margins) if margins else np.inf)


# pre-set score patterns of test_select_preset_scores: name -> function of (n_s, rng) giving the scores
def _one_nan(ns, rng):
    s = 1.0 + rng.permutation(ns) * 1e-3
    s[ns // 2] = np.nan
    return s


def _inf_among(ns, rng):
    s = 1.0 + rng.permutation(ns) * 1e-3
    s[::3] = np.inf
    return s


def _signed_zeros(ns, rng):
    s = 1.0 + rng.permutation(ns) * 1e-3
    s[[1, 4, 7]] = (0.0, -0.0, 0.0)
    return s


PRESET_SCORES = {
    "all_nan": lambda ns, rng: np.full(ns, np.nan),
    "one_nan": _one_nan,
    "inf_among_finite": _inf_among,
    "all_inf": lambda ns, rng: np.full(ns, np.inf),
    "signed_zeros": _signed_zeros,
}
PRESET_SIZE = 300   # members per state: more than one trip of the 256-thread loops


@functools.lru_cache(maxsize=None)
def preset_case(seed=4):
    """One state of PRESET_SIZE members per pattern of PRESET_SCORES, in that order; d = 3."""
    rng = np.random.default_rng(seed)
    k = len(PRESET_SCORES)
    labels = rng.permutation(np.repeat(np.arange(k), PRESET_SIZE))
    x = rng.standard_normal((labels.size, 3)) * 3.0
    offsets, members = group_ref(labels, k)
    scores = np.concatenate([fn(PRESET_SIZE, rng) for fn in PRESET_SCORES.values()])
    return x, labels.astype(np.int32), k, offsets, members, scores


@functools.lru_cache(maxsize=None)
def nan_feature_case(seed=6):
    """Three states of 40 members, d = 4, pre-set scores 1 + 1e-3 * permutation.  State 0: every score NaN, features
    finite.  State 1: a NaN coordinate in a member that is not the first pick.  State 2: a NaN coordinate in the
    member with the smallest score."""
    rng = np.random.default_rng(seed)
    k, ns = 3, 40
    labels = rng.permutation(np.repeat(np.arange(k), ns))
    x = rng.standard_normal((labels.size, 4)) * 3.0
    offsets, members = group_ref(labels, k)
    scores = np.concatenate([1.0 + 1e-3 * rng.permutation(ns) for _ in range(k)])
    scores[offsets[0]:offsets[1]] = np.nan
    s1 = scores[offsets[1]:offsets[2]]
    x[members[offsets[1] + int(np.argsort(s1)[7])], 2] = np.nan
    s2 = scores[offsets[2]:offsets[3]]
    x[members[offsets[2] + int(np.argmin(s2))], 0] = np.nan
    return x, labels.astype(np.int32), k, offsets, members, scores


@functools.lru_cache(maxsize=None)
def picker_nan_case(seed=12):
    """240 frames in three states, d = 3, a NaN coordinate in the sixth frame of state 1.  Returns (x, the same
    without the NaN, labels, the frames of state 1, the NaN frame)."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 3, size=240)
    clean = rng.standard_normal((240, 3)) + 2.0 * labels[:, None]
    frames1 = np.where(labels == 1)[0]
    bad = int(frames1[5])
    x = clean.copy()
    x[bad, 1] = np.nan
    return x, clean, labels, frames1, bad


# full-path exact-pick inputs: (name, d, sizes, seed, n_reps); the CPU test asserts their margins.  No state of two: without
# weights its two members are equally far from their midpoint, a tie of the law itself that no seed removes (states of
# two are selected from in select_case and scored in the medoid cases)
PICK_CASES = (
    ("d3", 3, (1, 3, 65, 129, 300), 31, 3),
    ("d17", 17, (1, 3, 63, 128, 257), 32, 3),
)


def pick_case(name):
    for nm, d, sizes, seed, n_reps in PICK_CASES:
        if nm == name:
            return state_case(d, sizes, seed) + (n_reps,)
    raise KeyError(name)


# ---- silhouette inputs ---------------------------------------------------------------------------------------------
def sorted_sizes(n, k):
    """Cluster sizes in cluster order that add up to n: where they fit, a cluster of 64, an empty one, one of 65 and a
    singleton in front (the tile boundary, an empty cluster between occupied ones), the rest spread evenly."""
    if n == 2:
        return [1] + [0] * (k - 2) + [1]
    head = [64, 0, 65, 1] if (k >= 5 and n >= 130 + 2 * (k - 4)) else [1, 0][:max(0, min(2, k - 1))]
    rest_k = k - len(head)
    rest = n - sum(head)
    base = [rest // rest_k + (1 if j < rest % rest_k else 0) for j in range(rest_k)]
    return head + base


# (k, d, n) of the k <= 32 entry: every k, d and n of the issue against every other
SORTED_K, SORTED_D, SORTED_N = (2, 3, 31, 32), (1, 3, 96, 97, 128), (2, 255, 256, 257, 1000)
SORTED_SHAPES = tuple((k, d, n) for k in SORTED_K for d in SORTED_D for n in SORTED_N)


@functools.lru_cache(maxsize=None)
def sorted_case(k, d, n, seed=0):
    """Points sorted by cluster (offsets from sorted_sizes), cluster centres 2 apart, unit noise; with the law."""
    rng = np.random.default_rng(1000 * k + 10 * d + n + seed)
    sizes = sorted_sizes(n, k)
    assert sum(sizes) == n and len(sizes) == k
    labels = np.repeat(np.arange(k), sizes)
    centres = 2.0 * rng.standard_normal((k, d))
    X = centres[labels] + rng.standard_normal((n, d))
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    law = silhouette_law(X, labels, k)
    for a in (X, labels, offsets, law):
        a.setflags(write=False)
    return X, labels, offsets, law


def _labels_from_sizes(sizes, rng, shuffle=True):
    labels = np.repeat(np.arange(len(sizes)), sizes)
    return rng.permutation(labels) if shuffle else labels


# msm_silhouette_samples: name -> (d, cluster sizes in id order, shuffled frames?)
SAMPLES_SHAPES = {
    "n3_d1": (1, (2, 1), True),
    "n127_d7": (7, (40, 0, 50, 1, 36), True),
    "n128_d8": (8, (40, 0, 50, 1, 37), True),
    "n129_d9": (9, (40, 0, 50, 1, 38), True),
    "singletons_16": (3, (30,) + (1,) * 16 + (100,), True),
    "singletons_17": (3, (30,) + (1,) * 17 + (100,), True),
    "rows_1024": (3, (500, 524, 30), True),
    "rows_1025": (3, (500, 525, 30), True),
    "cut_group_of_1024": (3, (1024, 300), True),
}


@functools.lru_cache(maxsize=None)
def samples_case(name):
    d, sizes, shuffle = SAMPLES_SHAPES[name]
    rng = np.random.default_rng(sum(sizes) + 7 * d)
    labels = _labels_from_sizes(sizes, rng, shuffle)
    X = rng.standard_normal((labels.size, d)) + 1.5 * labels[:, None]
    law = silhouette_law(X, labels, len(sizes))
    for a in (X, labels, law):
        a.setflags(write=False)
    return X, labels, len(sizes), law


# non-finite coordinates: name -> (frame's cluster, value); clusters of 70, 1, 90, 60 and 0, 80 members, sorted
NONFINITE = {"nan_in_middle_cluster": (2, np.nan), "inf_in_middle_cluster": (2, np.inf), "nan_in_singleton": (1, np.nan)}
NONFINITE_SIZES = (70, 1, 90, 60, 0, 80)


@functools.lru_cache(maxsize=None)
def nonfinite_case(name):
    cluster, value = NONFINITE[name]
    rng = np.random.default_rng(17)
    k = len(NONFINITE_SIZES)
    labels = np.repeat(np.arange(k), NONFINITE_SIZES)
    X = rng.standard_normal((labels.size, 3)) + 3.0 * labels[:, None]
    frame = int(np.flatnonzero(labels == cluster)[NONFINITE_SIZES[cluster] // 2])
    X[frame, 1] = value
    offsets = np.concatenate([[0], np.cumsum(NONFINITE_SIZES)]).astype(np.int64)
    law = silhouette_law(X, labels, k)
    return X, labels, offsets, law, frame


BEFORE_NAN_RULE = "silhouette_before_nan_rule.npz"


def recipe_points(n, d, k):
    """The points and labels of test_gpu_silhouette.py::_recipe_case.  tests/golden/silhouette_before_nan_rule.npz holds
    what the device gave for them at commit 73e3f52, before the kernels had a NaN rule: `samples/n_d_k` and
    `score/n_d_k` from Engine.silhouette_samples (msm_silhouette_samples) at (1500, 3, 33) and (700, 256, 40), and
    `sorted_samples/1000_3_7`, `sorted_score/1000_3_7` from Engine.silhouette (msm_silhouette) on the (1000, 3, 7)
    points stably sorted by label.  Finite input must keep these bits."""
    from tests import _gen

    X, _ = _gen.gaussian_clusters(k, n // k + 1, d, seed=k)
    return np.ascontiguousarray(X[:n], np.float64), recipe_labels(n, k)


# ---- the C ABI, one thin wrapper per entry point -------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ptr


def _host(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def _hptr(a):
    return None if a is None else a.ctypes.data


def c_group(engine, d_labels, n, k, d_offsets, d_members):
    from pmarlo_amd import _lib

    return _lib.load().msm_group_by_label(engine.handle, d_labels.ptr, n, k, d_offsets.ptr, d_members.ptr)


def c_centroids(engine, d_x, n, d, ld, d_w, d_offsets, d_members, k, d_cen, d_wsum, d_flags):
    from pmarlo_amd import _lib

    return _lib.load().msm_state_centroids(engine.handle, d_x.ptr, n, d, ld, _ptr(d_w), d_offsets.ptr, d_members.ptr, k,
                                           d_cen.ptr, d_wsum.ptr, d_flags.ptr)


def c_scores(engine, d_x, n, d, ld, d_w, d_labels, d_offsets, d_members, k, d_cen, d_wsum, mode, h_offsets, h_states,
             d_scores):
    from pmarlo_amd import _lib

    ho = _host(h_offsets, np.int64)
    hs = _host(h_states, np.int32)
    return _lib.load().msm_state_scores(engine.handle, d_x.ptr, n, d, ld, _ptr(d_w), _ptr(d_labels), d_offsets.ptr,
                                        d_members.ptr, k, _ptr(d_cen), _ptr(d_wsum), mode, _hptr(ho), _hptr(hs),
                                        0 if hs is None else hs.size, d_scores.ptr)


def c_select(engine, d_x, n, d, ld, d_offsets, d_members, k, d_scores, d_mind, mode, h_states, n_reps, d_picks):
    from pmarlo_amd import _lib

    hs = _host(h_states, np.int32)
    return _lib.load().msm_state_select(engine.handle, _ptr(d_x), n, d, ld, d_offsets.ptr, d_members.ptr, k, d_scores.ptr,
                                        _ptr(d_mind), mode, _hptr(hs), hs.size, n_reps, d_picks.ptr)


def c_silhouette(engine, d_x, n, d, ld, h_offsets, k, d_samples, d_score):
    from pmarlo_amd import _lib

    ho = _host(h_offsets, np.int64)
    return _lib.load().msm_silhouette(engine.handle, d_x.ptr, n, d, ld, _hptr(ho), k, d_samples.ptr, d_score.ptr)


def c_silhouette_samples(engine, d_x, n, d, ld, d_labels, k, d_samples, d_score, max_products=0, work=None):
    """`work`: a workspace allocated by the caller (a call under graph capture may neither allocate nor wait)."""
    from pmarlo_amd import _lib

    lib = _lib.load()
    own = work is None
    if own:
        work = engine.empty((max(int(lib.msm_silhouette_workspace_bytes(n, d, k)), 1),), np.uint8)
    st = lib.msm_silhouette_samples(engine.handle, d_x.ptr, n, d, ld, d_labels.ptr, k, work.ptr, work.nbytes,
                                    int(max_products), d_samples.ptr, d_score.ptr)
    if own:
        engine.sync()   # the workspace is free on return
    return st
