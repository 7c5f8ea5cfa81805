"""The VAMP-2 loss and AdamW kernels of csrc/mlp_train.hip on every launch path and branch: the column and weight sums,
the fp64 MFMA moments, the one-workgroup solve (Jacobi, jitter ladder, triangular inverse, the small products), the
output gradients, plain and weighted, and the clip + AdamW pair -- against the fp64 law (tests/_deeptica_train_ref,
tests/_deeptica_weighted_ref) on the cases of tests/_vamp2_paths_ref.py.

Every loss call goes through the C entries: the outputs are the left block of a buffer three columns wider whose other
words are NaN, the gradients land in a buffer five columns wider filled with one NaN bit pattern, the workspace has
exactly the reported size and is followed, like the stats block, by guard words that must not change.

Yardstick: a case's `bound` in the table -- 1e-10 of the largest entry wherever two routes through the law agree
within 1e-12 (tests/test_vamp2_paths_reference.py shows that on the host), 100 x the recorded route disagreement for
the two cases that cannot.  What must not move is compared as bits.  AdamW: the bounds of test_adamw_step."""

from __future__ import annotations

import numpy as np
import pytest

from pmarlo_amd import _lib
from pmarlo_amd._lib import check, lib
from tests import _deeptica_train_ref as T
from tests import _vamp2_paths_ref as V

pytestmark = pytest.mark.gpu

FILL64 = np.uint64(0x7FF8000012345678)            # a quiet NaN with a payload: untouched words are recognisable
GUARD = 32                                        # guard words after the workspace and after the stats block
RUNS = [(name, weighted) for name in V.CASES for weighted in V.runs(name)]
ONE_PER_TILE_COUNT = ("w15", "w32", "w49", "w64")
_WORST: dict = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def filled(engine, shape):
    return engine.to_device(np.full(shape, FILL64, np.uint64).view(np.float64))


def wide(engine, Y, pad, extra_rows=0):
    """Y as the top left block of a NaN buffer `pad` columns wider and `extra_rows` rows longer."""
    m, d = Y.shape
    buf = np.full((m + extra_rows, d + pad), np.nan)
    buf[:m, :d] = Y
    return engine.to_device(buf)


def loss(engine, Y0, Yt, w, opts, *, pad=3, gpad=5, prefill=0xFF, want_grad=True, extra_rows=0):
    """msm_vamp2_loss / msm_vamp2_loss_weighted through the C entry; the engine's reading of the stats block (it
    raises as Engine.vamp2_loss does) plus `stats` (the raw block) and the gradients on the host."""
    m, d = Y0.shape
    weighted = w is not None
    sizer = lib.msm_vamp2_weighted_workspace if weighted else lib.msm_vamp2_workspace
    need = int(sizer(m, d))
    assert need == 8 * V.workspace_doubles(m, d, weighted)
    work = np.full(need // 8 + GUARD, FILL64, np.uint64)
    work[:need // 8] = np.frombuffer(bytes([prefill]) * 8, np.uint64)[0]
    wd, sd = engine.to_device(work.view(np.float64)), filled(engine, (_lib.VAMP2_STATS + GUARD,))
    y0, yt = wide(engine, Y0, pad, extra_rows), wide(engine, Yt, pad, extra_rows)
    g0, gt = filled(engine, (m, d + gpad)), filled(engine, (m, d + gpad))
    o = opts
    tail = (m, d, d + pad, float(o["eps"]), float(o["eps_abs"]), float(o["alpha"]), float(o["cond_reg"]), wd.ptr, sd.ptr,
            g0.ptr if want_grad else None, gt.ptr if want_grad else None, d + gpad)
    if weighted:
        wts = engine.to_device(np.concatenate([np.asarray(w, np.float64), np.full(extra_rows, np.nan)]))
        check(lib.msm_vamp2_loss_weighted(engine.handle, y0.ptr, yt.ptr, wts.ptr, *tail), engine.handle)
    else:
        check(lib.msm_vamp2_loss(engine.handle, y0.ptr, yt.ptr, *tail), engine.handle)
    stats, G0, Gt = sd.to_host(), g0.to_host(), gt.to_host()
    assert np.all(bits(wd.to_host())[need // 8:] == FILL64), "the workspace is larger than reported"
    assert np.all(bits(stats)[_lib.VAMP2_STATS:] == FILL64), "the stats block is larger than MSM_VAMP2_STATS"
    assert np.all(bits(G0[:, d:]) == FILL64) and np.all(bits(Gt[:, d:]) == FILL64), "gradient padding was written"
    if not want_grad:
        assert np.all(bits(G0) == FILL64) and np.all(bits(Gt) == FILL64)
    stats = stats[:_lib.VAMP2_STATS]
    res = engine._weighted_stats(stats, d) if weighted else engine._vamp2_stats(stats, d)
    res["stats"] = stats
    if want_grad:
        res["grad0"], res["grad_t"] = np.ascontiguousarray(G0[:, :d]), np.ascontiguousarray(Gt[:, :d])
    return res


def run(engine, name, weighted, **kw):
    Y0, Yt, w = V.inputs(name)
    return loss(engine, Y0, Yt, w if weighted else None, V.CASES[name]["opts"], **kw)


def written(res, d):
    """The bits of everything a call promises: the sixteen scalars, the first d of each vector of the stats block,
    and the gradients."""
    s, head, w = res["stats"], 16, _lib.MLP_MAX_OUT
    parts = [bits(s[:head])] + [bits(s[head + i * w: head + i * w + d]) for i in range(4)]
    parts += [bits(res[k]).reshape(-1) for k in ("grad0", "grad_t") if k in res]
    return np.concatenate(parts)


# ---- a. the table reaches what it claims -----------------------------------------------------------------------------
def test_the_cases_reach_every_path(engine):
    assert _lib.MLP_CHUNK == V.CHUNK and _lib.VAMP2_STATS == 272 and _lib.MLP_MAX_OUT == 64
    V.assert_every_path(_lib.MLP_CHUNK)
    for c in V.CASES.values():
        m, d = c["m"], c["d"]
        assert int(lib.msm_vamp2_workspace(m, d)) == 8 * V.workspace_doubles(m, d, False)
        assert int(lib.msm_vamp2_weighted_workspace(m, d)) == 8 * V.workspace_doubles(m, d, True)
    assert int(lib.msm_vamp2_workspace(1, 65)) == 0 and int(lib.msm_vamp2_workspace(0, 3)) == 0


def test_more_pairs_than_grid_rows_are_refused(engine):
    """The moments kernels take one chunk of 256 pairs per grid row and the device admits 65536 rows: 2^24 pairs is the
    envelope, one more is MSM_ERR_UNSUPPORTED before anything is launched (the buffers here hold four pairs)."""
    top = 65536 * _lib.MLP_CHUNK
    assert top == 1 << 24
    for sizer in (lib.msm_vamp2_workspace, lib.msm_vamp2_weighted_workspace):
        assert int(sizer(top, 1)) > 0 and int(sizer(top + 1, 1)) == 0
    y, wts = engine.to_device(np.ones((4, 1))), engine.to_device(np.ones(4))
    wd, sd, g0, gt = filled(engine, (64,)), filled(engine, (_lib.VAMP2_STATS,)), filled(engine, (4, 1)), filled(engine, (4, 1))
    tail = (top + 1, 1, 1, 1e-3, 1e-6, 0.3, 1e-4, wd.ptr, sd.ptr, g0.ptr, gt.ptr, 1)
    for st in (lib.msm_vamp2_loss(engine.handle, y.ptr, y.ptr, *tail),
               lib.msm_vamp2_loss_weighted(engine.handle, y.ptr, y.ptr, wts.ptr, *tail)):
        assert st == _lib.MSM_ERR_UNSUPPORTED
        assert f"{top + 1} frame pairs" in lib.msm_last_error(engine.handle).decode()
    engine.sync()
    for a in (wd, sd, g0, gt):
        assert np.all(bits(a.to_host()) == FILL64)
    with pytest.raises(ValueError, match="0 frame pairs"):
        check(lib.msm_vamp2_loss(engine.handle, y.ptr, y.ptr, 0, *tail[1:]), engine.handle)


# ---- b. every case against the law -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,weighted", RUNS)
def test_against_the_law(engine, name, weighted):
    c = V.CASES[name]
    want = V.law(name, weighted)
    got = run(engine, name, weighted)
    assert got["stats"][9] == 0.0 and np.all(got["stats"][13:16] == 0.0)
    expect = c["expect"] or {}
    if expect.get("zero"):                      # the trace clamp: nothing to measure a distance in
        V.assert_zero_case(got, want["metrics"])
        return
    dist = V.distances(got, want, c["compare"])
    worst = max(dist, key=dist.get)
    print(f"{name} {'weighted' if weighted else 'plain'}: |device - law| = {dist[worst]:.2e} ({worst}), bound {c['bound']:.1e}")
    key = (c["group"], "weighted" if weighted else "plain")
    _WORST[key] = max(_WORST.get(key, (0.0, "")), (dist[worst], f"{name} {worst}"))
    assert dist[worst] <= c["bound"], dist
    if c["route"] is not None:                  # where the law itself is the coarser side: the second route too
        two = V.second(name, weighted)
        two["term_scale"] = want["term_scale"]
        near = V.distances(got, two, c["compare"])
        print(f"    |device - second route| = {max(near.values()):.2e} ({max(near, key=near.get)})")
        assert max(near.values()) <= V.YARDSTICK, near
    if weighted:
        w = V.inputs(name)[2]
        assert np.all(got["grad0"][w <= 0] == 0.0) and np.all(got["grad_t"][w <= 0] == 0.0)   # no weight, no gradient
    if c["opts"]["cond_reg"] <= 0.0:
        assert got["penalty"] == 0.0 and bits(got["loss"]) == bits(-got["score"])
    if expect.get("total") == 1e-8:             # the ladder case: the constant output's eigenvalue is on the floor
        assert got["metrics"]["eig_C00_min"] == V.FLOOR and got["metrics"]["eig_Ctt_min"] == V.FLOOR
    if c["opts"]["alpha"] >= 1.0:
        assert got["metrics"]["cond_C00"] == 1.0 and got["metrics"]["cond_Ctt"] == 1.0 and got["penalty"] == 0.0


def test_report_the_largest_distances():
    for (group, kind), (dist, where) in sorted(_WORST.items()):
        print(f"largest |device - law|, {group} {kind}: {dist:.2e} at {where}")


@pytest.mark.parametrize("name", ["w16", "w56", "w64", "r770x17"])
def test_constant_weights_are_the_unweighted_loss(engine, name):
    Y0, Yt, _ = V.inputs(name)
    c = V.CASES[name]
    plain = loss(engine, Y0, Yt, None, c["opts"])
    const = loss(engine, Y0, Yt, np.full(c["m"], 0.37), c["opts"])
    plain["term_scale"] = V.law(name, False)["term_scale"]
    dist = V.distances(const, plain, "all")
    print(f"{name}: constant weights against no weights {max(dist.values()):.2e}")
    assert max(dist.values()) <= V.YARDSTICK
    assert abs(const["effective_pairs"] - c["m"]) <= V.YARDSTICK * c["m"]


@pytest.mark.parametrize("name", ["p257x16_zeros", "p770x64_zeros"])
def test_negative_weights_are_zero_weights(engine, name):
    Y0, Yt, w = V.inputs(name)
    assert np.any(w < 0.0)
    a = loss(engine, Y0, Yt, w, V.CASES[name]["opts"])
    b = loss(engine, Y0, Yt, np.clip(w, 0.0, None), V.CASES[name]["opts"])
    assert np.array_equal(written(a, Y0.shape[1]), written(b, Y0.shape[1]))


# ---- c. buffers, and equal bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", ONE_PER_TILE_COUNT)
def test_buffers_and_equal_bits(engine, name, weighted):
    d = V.CASES[name]["d"]
    base = run(engine, name, weighted)
    ref = written(base, d)
    assert np.all(np.isfinite(ref.view(np.float64)))
    # a workspace of zeros instead of 0xFF bytes: nothing stale is read
    assert np.array_equal(written(run(engine, name, weighted, prefill=0x00), d), ref)
    # eight NaN rows (and NaN weights) past the last pair
    assert np.array_equal(written(run(engine, name, weighted, extra_rows=8), d), ref)
    # packed inputs and packed gradients: the strides change nothing
    assert np.array_equal(written(run(engine, name, weighted, pad=0, gpad=0), d), ref)
    # without gradients: both buffers untouched (`loss` asserts it), the same stats
    nograd = run(engine, name, weighted, want_grad=False)
    assert "grad0" not in nograd and np.array_equal(written(nograd, d), written({"stats": base["stats"]}, d))
    # other shapes in between, weighted and not, then the same call again
    run(engine, "r770x17", not weighted)
    run(engine, "w2", weighted)
    run(engine, "r513x64", weighted)
    assert np.array_equal(written(run(engine, name, weighted), d), ref)


# ---- d. the clamps of the options ------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d", V.BRANCH_WIDTHS)
def test_options_are_clamped(engine, d, weighted):
    Y0, Yt, w = V.inputs(f"b_nocond{d}")
    w = w if weighted else None
    base = {"eps": 1e-3, "eps_abs": 1e-6, "alpha": 0.3, "cond_reg": 0.05}
    for key, given, means in (("alpha", -1.0, 0.0), ("alpha", 2.0, 1.0), ("eps_abs", -1.0, 0.0), ("cond_reg", -1.0, 0.0)):
        a, b = loss(engine, Y0, Yt, w, {**base, key: given}), loss(engine, Y0, Yt, w, {**base, key: means})
        assert np.array_equal(written(a, d), written(b, d)), (key, given)
        assert np.isfinite(a["loss"])
    moved = loss(engine, Y0, Yt, w, {**base, "alpha": 0.0})
    assert moved["loss"] != loss(engine, Y0, Yt, w, base)["loss"]                # the option acts


# ---- e. poisoned outputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d", V.BRANCH_WIDTHS)
def test_poisoned_outputs_raise_and_leave_no_trace(engine, d, weighted):
    name = f"b_nocond{d}"
    Y0, Yt, w = V.inputs(name)
    w = w if weighted else None
    ref = written(run(engine, name, weighted), d)
    for poison, which in ((np.nan, 0), (np.inf, 1), (-np.inf, 0)):
        bad = [Y0.copy(), Yt.copy()]
        bad[which][Y0.shape[0] // 2, d - 1 if which == 0 else 0] = poison
        with pytest.raises(RuntimeError, match="Cholesky decomposition failed after retries"):
            loss(engine, bad[0], bad[1], w, V.CASES[name]["opts"])
        assert np.array_equal(written(run(engine, name, weighted), d), ref)


# ---- f. clip + AdamW -------------------------------------------------------------------------------------------------------
LR = 3e-3


def adamw(engine, pd, g, md, vd, step, wd, clip):
    """msm_adamw_step through the C entry: out[0..3] = norm, clipped norm, skipped, clip coefficient."""
    out = filled(engine, (4 + GUARD,))
    check(lib.msm_adamw_step(engine.handle, pd.ptr, engine.to_device(g).ptr, md.ptr, vd.ptr, pd.size, int(step), LR, 0.9,
                             0.999, 1e-8, float(wd), float(clip) if clip is not None else 0.0, out.ptr), engine.handle)
    o = out.to_host()
    assert np.all(bits(o)[4:] == FILL64)
    return o[:4]


def adam_state(engine, n, step):
    """Parameters and moments of a run at `step`: zero moments at step 1, a history otherwise."""
    rng = np.random.default_rng(n + step)
    p = rng.normal(size=n).astype(np.float32)
    m = np.zeros(n) if step == 1 else rng.normal(size=n) * 10.0 ** rng.uniform(-6, 1, size=n)
    v = np.zeros(n) if step == 1 else 10.0 ** rng.uniform(-12, 2, size=n)
    g = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-8, 3, size=n)
    return p, m, v, g


@pytest.mark.parametrize("clip_kind", [None, "below", "equal"])
@pytest.mark.parametrize("step", [1, 10 ** 6])
@pytest.mark.parametrize("n", [1023, 1024, 1025, (1 << 20) + 3])
def test_adamw_sizes_and_steps(engine, n, step, clip_kind):
    p0, m0, v0, g = adam_state(engine, n, step)
    norm = float(np.sqrt(np.sum(g * g)))
    clip = {None: None, "below": 0.1 * norm, "equal": norm}[clip_kind]
    wd = 1e-4
    p1, m1, v1, norm_ref, norm_clipped, skipped = T.adamw(p0, g, m0, v0, step, LR, wd=wd, clip=clip)
    assert not skipped
    if step > 1:
        assert 1.0 - 0.9 ** step == 1.0 and np.sqrt(1.0 - 0.999 ** step) == 1.0      # the bias corrections are gone
    runs = []
    for _ in range(2):
        pd, md, vd = engine.to_device(p0), engine.to_device(m0), engine.to_device(v0)
        out = adamw(engine, pd, g, md, vd, step, wd, clip)
        runs.append((out, pd.to_host(), md.to_host(), vd.to_host()))
    out, p, m, v = runs[0]
    coef = norm_clipped / norm_ref
    print(f"n = {n}, step {step}, clip {clip_kind}: norm {out[0]!r} law {norm_ref!r}, coefficient {out[3]!r} law {coef!r}")
    assert out[2] == 0.0
    assert abs(out[0] - norm_ref) <= 1e-13 * norm_ref and abs(out[1] - norm_clipped) <= 1e-13 * norm_clipped
    assert abs(out[3] - coef) <= 1e-13 * coef
    if clip_kind is None:
        assert out[3] == 1.0 and out[1] == out[0]
    elif clip_kind == "equal":
        assert 1.0 - 2e-6 / norm < out[3] < 1.0                 # clip / (norm + 1e-6): just under 1
    assert np.all(np.abs(m - m1) <= 1e-13 * (0.9 * np.abs(m0) + 0.1 * np.abs(g) * coef))
    assert np.all(np.abs(v - v1) <= 1e-13 * np.abs(v1))
    assert np.all(np.abs(p.astype(np.float64) - p1.astype(np.float64)) <= T.ulp32(p1))
    assert np.any(p != p0)
    # equal inputs, equal bits
    assert np.array_equal(bits(runs[1][0]), bits(out)) and np.array_equal(runs[1][1].view(np.uint32), p.view(np.uint32))
    assert np.array_equal(bits(runs[1][2]), bits(m)) and np.array_equal(bits(runs[1][3]), bits(v))


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_adamw_edges_of_the_norm(engine, n):
    p0, m0, v0, g = adam_state(engine, n, 1)
    fresh = lambda: (engine.to_device(p0), engine.to_device(m0), engine.to_device(v0))      # noqa: E731
    # a zero gradient: only the decay moves the parameters
    for clip in (None, 1.0):
        pd, md, vd = fresh()
        out = adamw(engine, pd, np.zeros(n), md, vd, 1, 1e-2, clip)
        assert out[0] == 0.0 and out[1] == 0.0 and out[2] == 0.0 and out[3] == 1.0
        want = (p0.astype(np.float64) * (1.0 - LR * 1e-2)).astype(np.float32)
        assert np.all(np.abs(pd.to_host().astype(np.float64) - want.astype(np.float64)) <= T.ulp32(want))
        assert np.any(pd.to_host() != p0)
        assert np.all(md.to_host() == 0.0) and np.all(vd.to_host() == 0.0)
    # one entry of 1e200 (the last thread's, or the first thread's second): every entry finite, the norm is not
    for at in (n - 1, 0):
        big = g.copy()
        big[at] = 1e200
        assert np.all(np.isfinite(big))
        pd, md, vd = fresh()
        out = adamw(engine, pd, big, md, vd, 1, 1e-2, 1.0)
        assert out[2] == 1.0 and out[0] == np.inf
        assert T.adamw(p0, big, m0, v0, 1, LR, wd=1e-2, clip=1.0)[5]
        assert np.array_equal(pd.to_host().view(np.uint32), p0.view(np.uint32))
        assert np.array_equal(bits(md.to_host()), bits(m0)) and np.array_equal(bits(vd.to_host()), bits(v0))
    # gradients whose squares underflow: norm 0, the clip coefficient 1, and an update from the first moment alone
    tiny = np.where(g > 0, 1e-170, -1e-170)
    pd, md, vd = fresh()
    out = adamw(engine, pd, tiny, md, vd, 1, 1e-2, 0.5)
    p1, m1, v1, norm_ref, _, skipped = T.adamw(p0, tiny, m0, v0, 1, LR, wd=1e-2, clip=0.5)
    assert norm_ref == 0.0 and not skipped
    assert out[0] == 0.0 and out[1] == 0.0 and out[2] == 0.0 and out[3] == 1.0
    m, v = md.to_host(), vd.to_host()
    assert np.all(v == 0.0) and np.all(v1 == 0.0) and np.all(np.abs(m - m1) <= 1e-13 * np.abs(m1))
    assert np.all(np.isfinite(pd.to_host()))
    assert np.all(np.abs(pd.to_host().astype(np.float64) - p1.astype(np.float64)) <= T.ulp32(p1))
