"""The DeepTICA network kernels (csrc/mlp.hip, mlp_vjp.hip, mlp_train.hip) on every launch path, against the fp64 law
composed in tests/_mlp_paths_ref.py.

Every test that claims a path asks Engine.mlp_plan first -- the read-only view of the one host function all four
launch sites call (msm_mlp_launch_plan) -- and takes its sizes from it: a second grid-stride trip needs
16 * (grid_cap + 1) + 5 rows, where grid_cap = CUs x resident workgroups per CU is whatever this device answers.

Yardstick: fp64 kernels against an fp64 law, 1e-10 of the largest entry of each tensor, as in
tests/test_gpu_deeptica_train.py; tests/test_mlp_paths_reference.py shows two routes through the law to agree within
1e-12 at these shapes.  The one tensor without a largest entry, the bias of a linear head, is measured in the size of
its terms (P.grad_scales).  Everything that must not move -- padding, packed against strided calls, a frame among
other frames, a second call -- is compared as bits.  Strided calls and refusals go through the C entry points into
buffers filled with one NaN bit pattern."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from pmarlo_amd import _lib
from pmarlo_amd._lib import lib
from pmarlo_amd.features.deeptica.model import MLPSpec
from tests import _deeptica_train_ref as T
from tests import _mlp_paths_ref as P

pytestmark = pytest.mark.gpu

TOL = 1e-10
FILL64 = np.uint64(0x7FF8000012345678)            # quiet NaNs with a payload: untouched words are recognisable
FILL32 = np.uint32(0x7FC12345)
QNAN = np.float64(np.nan)
STRENGTH = 2.5
MAX_ROWS = 1 << 18

_SPECS: dict = {}


def spec(name):
    if name not in _SPECS:
        _SPECS[name] = MLPSpec(**P.network(P.case(name)))
    return _SPECS[name]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def filled(engine, shape, dtype=np.float64):
    if np.dtype(dtype) == np.float64:
        return engine.to_device(np.full(shape, FILL64, np.uint64).view(np.float64))
    return engine.to_device(np.full(shape, FILL32, np.uint32).view(np.float32))


def untouched(a) -> bool:
    a = np.ascontiguousarray(a)
    return bool(np.all(a.view(np.uint64) == FILL64)) if a.dtype == np.float64 else bool(np.all(a.view(np.uint32) == FILL32))


def padded(engine, X, pad):
    """X as the left block of a buffer `pad` columns wider whose other words are the fill pattern."""
    X = np.ascontiguousarray(X)
    n, w = X.shape
    fill = FILL64 if X.dtype == np.float64 else FILL32
    wide = np.full((n, w + pad), fill, fill.dtype).view(X.dtype)
    wide[:, :w] = X
    return engine.to_device(wide)


def close(got, want, scale=None) -> bool:
    """|got - want| <= 1e-10 of the largest entry of want (or of `scale`); prints the figure first."""
    want = np.asarray(want, np.float64)
    err = float(np.max(np.abs(np.asarray(got, np.float64) - want)))
    scale = float(np.max(np.abs(want))) if scale is None else scale
    print(f"    |device - law| = {err:.3e} = {err / scale if scale else 0.0:.2e} of {scale:.3e}")
    return err <= TOL * scale


def check_grads(c, got_packed, law):
    got = T.unpack(c["config"], c["widths"][0], np.asarray(got_packed))
    for key, scale in P.grad_scales(c, law).items():
        print(f"  {key}:")
        assert close(got[key], law["grads"][key], scale), key


# ---- the C entry points ----------------------------------------------------------------------------------------------
class Net:
    """The network arguments of the C entry points for a spec; the refusal cases override some of them."""

    def __init__(self, engine, sp, widths=None, n_params=None, with_scale=True):
        self.engine, self.sp = engine, sp
        self.w = np.ascontiguousarray(sp.widths if widths is None else widths, np.int32)
        self.params, self.mean, self.scale = engine._mlp_on_device(sp)
        self.n_params = self.params.size if n_params is None else n_params
        self.with_scale = with_scale

    def head(self, xd, n, ld):
        code = _lib.MSM_F32 if xd.dtype == np.float32 else _lib.MSM_F64
        return (self.engine.handle, xd.ptr, code, n, int(self.w[0]), ld, self.mean.ptr,
                self.scale.ptr if self.with_scale else None, len(self.w) - 1, self.w.ctypes.data, self.sp.activation,
                int(self.sp.ln_in), int(self.sp.ln_hidden), int(self.sp.head_activation), self.params.ptr, self.n_params)

    def flags(self):
        return len(self.w) - 1, self.w.ctypes.data, int(self.sp.ln_in), int(self.sp.ln_hidden), int(self.sp.head_activation)

    def message(self) -> str:
        return lib.msm_last_error(self.engine.handle).decode()


def c_forward(net, xd, n, ld, od, ldo):
    return lib.msm_mlp_forward(*net.head(xd, n, ld), od.ptr, ldo)


def c_vjp(net, xd, n, ld, gd, ldgo, ed, od, ldo, gxd, ldgx, wd, work_bytes=None):
    return lib.msm_mlp_vjp(*net.head(xd, n, ld), gd.ptr if gd is not None else None, ldgo, STRENGTH,
                           ed.ptr if ed is not None else None, od.ptr if od is not None else None, ldo, gxd.ptr, ldgx,
                           wd.ptr, wd.nbytes if work_bytes is None else work_bytes)


def c_loss_grad(net, xd, n, ld, itd, itaud, m, drop, sd, gd, od, ldo, wd, work_bytes=None, step=P.STEP):
    o = T.LOSS_OPTS
    drop = None if drop is None else np.ascontiguousarray(drop, np.float64)
    return lib.msm_mlp_loss_grad(*net.head(xd, n, ld), itd.ptr, itaud.ptr, m,
                                 drop.ctypes.data if drop is not None else None, P.SEED, step, o["eps"], o["eps_abs"],
                                 o["alpha"], o["cond_reg"], wd.ptr, wd.nbytes if work_bytes is None else work_bytes,
                                 sd.ptr, gd.ptr if gd is not None else None, od.ptr if od is not None else None, ldo)


def vjp_work(engine, net, n):
    return engine.empty((max(int(lib.msm_mlp_vjp_workspace(n, *net.flags())), 8) // 8,), np.float64)


def train_work(engine, net, m):
    need = int(lib.msm_mlp_train_workspace(m, *net.flags()))
    assert need > 0
    return engine.empty((need // 8,), np.float64)


def run_loss_grad(engine, name, X, it, itau, drop, pad=0, want_out=True):
    """msm_mlp_loss_grad through the C entry into filled buffers: (status, stats, grad, the whole output buffer)."""
    net = Net(engine, spec(name))
    n, F = X.shape
    m, d = len(it), int(net.w[-1])
    xd = padded(engine, X, pad)
    itd, itaud = engine.to_device(np.ascontiguousarray(it, np.int64)), engine.to_device(np.ascontiguousarray(itau, np.int64))
    sd, gd = filled(engine, (_lib.VAMP2_STATS,)), filled(engine, (net.n_params,))
    od = filled(engine, (2 * m, d + pad)) if want_out else None
    wd = train_work(engine, net, m)
    st = c_loss_grad(net, xd, n, F + pad, itd, itaud, m, drop, sd, gd, od, d + pad, wd)
    assert st == _lib.MSM_OK, net.message()
    res = st, sd.to_host(), gd.to_host(), od.to_host() if want_out else None
    del wd                                             # held until the results are on the host
    return res


# ---- a. the second grid-stride trip ----------------------------------------------------------------------------------
def second_trip_rows(engine, kernels, name) -> tuple:
    """(rows, grid) of the smallest batch that sends the first two workgroups of every kernel in `kernels` on a
    second trip and ends in a ragged group of 5: 16 * (grid_cap + 1) + 5 with the largest grid_cap among them."""
    c, sp = P.case(name), spec(name)
    caps = [engine.mlp_plan(k, sp, MAX_ROWS, c["xdtype"])["grid_cap"] for k in kernels]
    rows = 16 * (max(caps) + 1) + 5
    assert rows <= MAX_ROWS, f"{name}: a second trip needs {rows} rows"
    return rows, max(caps)


def poison(X, grid, F):
    """Three frames of first-trip groups made non-finite, at different rows j of their groups and different
    columns (a multiple of 16; the last, partial chunk of F; another): [(frame, column, value), ...].  The first two
    have a frame 16 * grid further on, which the same lanes handle one trip later."""
    spots = [(16 * 0 + 3, 16 if F > 16 else 0, np.nan), (16 * 1 + 2, F - 1, np.inf), (16 * (grid - 1) + 15, min(5, F - 1), -np.inf)]
    Xp = np.array(X)
    for t, col, value in spots:
        Xp[t, col] = value
    return Xp, spots


@pytest.mark.parametrize("name,kernel", [("edge256", "forward"), ("edge256", "vjp"), ("deep8", "forward"), ("deep8", "vjp")])
def test_second_trip_forward_and_vjp(engine, name, kernel):
    c, sp = P.case(name), spec(name)
    n, grid = second_trip_rows(engine, [kernel], name)
    plan = engine.mlp_plan(kernel, sp, n, c["xdtype"])
    print(f"{name} {kernel}: n = {n}, plan {plan}")
    assert plan["trips"] >= 2 and plan["grid"] == grid == plan["grid_cap"] and plan["n_groups"] == grid + 2
    assert (plan["lds_bytes"] > 48 * 1024) == (name == "edge256")
    assert c["xdtype"] == (np.float32 if name == "edge256" else np.float64)        # both dtype instances
    X = P.frames(name, n)
    F = X.shape[1]

    def run(frames):
        xd = engine.to_device(np.ascontiguousarray(frames))
        if kernel == "forward":
            return {"outputs": engine.mlp_forward(xd, sp).to_host()}
        res = engine.mlp_vjp(xd, sp, strength=STRENGTH)
        return {k: res[k].to_host() for k in ("outputs", "energy", "gx")}

    clean = run(X)
    energy, y, gx = P.vjp(c, X, strength=STRENGTH)
    for key, want in (("outputs", y), ("energy", energy), ("gx", gx)):
        if key in clean:
            print(f"  {key}:")
            assert close(clean[key], want), key
    # the first trip poisoned: its frames are NaN, every other frame keeps its bits
    Xp, spots = poison(X, grid, F)
    dirty = run(Xp)
    hit = np.zeros(n, bool)
    hit[[t for t, _, _ in spots]] = True
    later = [t + 16 * grid for t, _, _ in spots if t + 16 * grid < n]
    assert len(later) == 2 and not hit[later].any()
    for key in clean:
        assert np.all(np.isnan(dirty[key][hit])), key
        assert np.array_equal(bits(dirty[key][~hit]), bits(clean[key][~hit])), key
        assert np.array_equal(bits(dirty[key][later]), bits(clean[key][later])), key
    # the second trip's groups alone: a whole group, and the ragged last one of 5 rows
    for lo, hi in ((16 * grid, 16 * grid + 16), (16 * (grid + 1), n)):
        alone = run(X[lo:hi])
        assert hi - lo in (16, 5)
        for key in clean:
            assert np.array_equal(bits(alone[key]), bits(clean[key][lo:hi])), (key, lo)


def test_second_trip_training(engine):
    name = "edge256"
    c, sp = P.case(name), spec(name)
    rows, grid = second_trip_rows(engine, ["train_forward", "train_backward"], name)
    rows += rows % 2
    m = rows // 2
    for kernel in ("train_forward", "train_backward"):
        plan = engine.mlp_plan(kernel, sp, rows, c["xdtype"])
        print(f"{name} {kernel}: 2m = {rows}, plan {plan}")
        assert plan["trips"] >= 2 and plan["lds_bytes"] > 48 * 1024 and plan["param_chunks"] == -(-rows // 256)
    n = 1500
    X = P.frames(name, n)
    it, itau = P.pairs(name, m, n - 10)                 # the last ten frames are named by the slots below alone
    slots = np.concatenate([it, itau])
    # three slots of first-trip groups at different rows j, each naming a frame of its own; the first of these
    # frames is named once more, by a slot of the ragged last group
    picked = [3, 16 + 2, 16 * (grid - 1) + 15]
    slots[picked] = n - 3, n - 2, n - 1
    slots[16 * (grid + 1) + 1] = n - 3
    later = [s + 16 * grid for s in picked[:2]]         # the slots the same lanes handle one trip later
    assert max(later) < rows and 16 * (grid + 1) + 1 not in later
    it, itau = np.ascontiguousarray(slots[:m]), np.ascontiguousarray(slots[m:])
    drop = P.dropout_of(name)
    assert min(drop) > 0.0
    law = P.loss_grad(c, X, it, itau, dropout=drop)
    xd = engine.to_device(np.ascontiguousarray(X))
    kw = dict(dropout=drop, seed=P.SEED, step=P.STEP, want_outputs=True, **T.LOSS_OPTS)
    got = engine.mlp_loss_grad(xd, sp, it, itau, **kw)
    for key in ("loss", "score"):
        print(f"  {key}: device {got[key]!r} law {law[key]!r}")
        assert abs(got[key] - law[key]) <= TOL * abs(law[key])
    out = got["outputs"].to_host()
    assert close(out, law["outputs"])
    check_grads(c, got["grad"].to_host(), law)
    # two equal calls give equal bits
    again = engine.mlp_loss_grad(xd, sp, it, itau, **kw)
    assert again["loss"] == got["loss"]
    for key in ("grad", "outputs"):
        assert np.array_equal(bits(again[key].to_host()), bits(got[key].to_host())), key
    # with dropout off the outputs are those of the inference kernel on the gathered rows
    plain = engine.mlp_loss_grad(xd, sp, it, itau, want_outputs=True, want_grad=False, **T.LOSS_OPTS)["outputs"].to_host()
    fwd = engine.mlp_forward(engine.to_device(np.ascontiguousarray(X[slots])), sp).to_host()
    assert np.array_equal(bits(plain), bits(fwd))
    # frames of first-trip slots poisoned: the slots that name them are NaN, every other slot keeps its bits
    Xp = np.array(X)
    for s, col, value in zip(picked, (16, X.shape[1] - 1, 5), (np.nan, np.inf, -np.inf)):
        Xp[slots[s], col] = value
    hit = np.isin(slots, slots[picked])
    assert hit.sum() == 4 and not hit[later].any()
    _, stats, _, dirty = run_loss_grad(engine, name, Xp, it, itau, drop)
    assert np.isnan(stats[0])
    assert np.all(np.isnan(dirty[hit])) and np.array_equal(bits(dirty[~hit]), bits(out[~hit]))
    assert np.array_equal(bits(dirty[later]), bits(out[later]))


# ---- b. the chunk boundaries of the parameter gradient ---------------------------------------------------------------
CHUNKS = {128: (1, 256, 1), 129: (2, 2, 1), 256: (2, 256, 1), 257: (3, 2, 2), 300: (3, 88, 2)}   # m: chunks, tail, VAMP


@pytest.mark.parametrize("m", P.CHUNK_M)
@pytest.mark.parametrize("name", ["odd", "leaky", "deep8", "head_off"])
def test_parameter_gradient_chunks(engine, name, m):
    c, sp = P.case(name), spec(name)
    chunks, tail, vamp_chunks = CHUNKS[m]
    for kernel in ("train_forward", "train_backward"):
        plan = engine.mlp_plan(kernel, sp, 2 * m, c["xdtype"])
        assert (plan["param_chunks"], plan["vamp_chunks"]) == (chunks, vamp_chunks), plan
        assert plan["n_groups"] == -(-2 * m // 16) and plan["param_jobs"] > 0
    assert 2 * m - (chunks - 1) * _lib.MLP_CHUNK == tail
    n = m + 40
    X = P.frames(name, n)
    it, itau = P.pairs(name, m, n)
    xd = engine.to_device(np.ascontiguousarray(X))
    for drop in (None, P.dropout_of(name)):
        print(f"{name} m = {m}, dropout {drop}")
        law = P.loss_grad(c, X, it, itau, dropout=drop)
        got = engine.mlp_loss_grad(xd, sp, it, itau, dropout=drop, seed=P.SEED, step=P.STEP, **T.LOSS_OPTS)
        for key in ("loss", "score"):
            assert abs(got[key] - law[key]) <= TOL * abs(law[key]), key
        check_grads(c, got["grad"].to_host(), law)
        if drop is None:
            # the first and the last pair swapped: another order of the sums, the same law
            order = np.arange(m)
            order[[0, m - 1]] = m - 1, 0
            assert (it[order[0]], itau[order[0]]) != (it[0], itau[0])
            swapped = engine.mlp_loss_grad(xd, sp, it[order], itau[order], **T.LOSS_OPTS)
            assert abs(swapped["loss"] - got["loss"]) <= TOL * abs(got["loss"])
            check_grads(c, swapped["grad"].to_host(), {**law, "grads": T.unpack(c["config"], c["widths"][0], got["grad"].to_host())})


# ---- c. the networks at the edges of the envelope -------------------------------------------------------------------
@pytest.mark.parametrize("n", P.SIZES)
@pytest.mark.parametrize("name", list(P.NETS))
def test_envelope_forward_and_vjp(engine, name, n):
    c, sp = P.case(name), spec(name)
    X = P.frames(name, n)
    xd = engine.to_device(np.ascontiguousarray(X))
    fwd = engine.mlp_forward(xd, sp).to_host()
    for kernel in ("forward", "vjp"):
        plan = engine.mlp_plan(kernel, sp, n, c["xdtype"])
        assert plan["trips"] == 1 and plan["grid"] == plan["n_groups"] == -(-n // 16)
        assert (plan["lds_bytes"] > 48 * 1024) == (name == "edge256")
    for gout in (None, P.upstream(name, n)):
        energy, y, gx = P.vjp(c, X, gout=gout, strength=STRENGTH)
        res = engine.mlp_vjp(xd, sp, gout=None if gout is None else engine.to_device(gout), strength=STRENGTH)
        print(f"{name} n = {n}, upstream gradient {'own' if gout is None else 'given'}")
        assert close(fwd, y) and close(res["energy"].to_host(), energy) and close(res["gx"].to_host(), gx)
        assert np.array_equal(bits(res["outputs"].to_host()), bits(fwd))
    # a float32 X and its exact float64 image
    X32 = np.ascontiguousarray(X, np.float32)
    a, b = engine.to_device(X32), engine.to_device(X32.astype(np.float64))
    assert np.array_equal(bits(engine.mlp_forward(a, sp).to_host()), bits(engine.mlp_forward(b, sp).to_host()))
    ra, rb = engine.mlp_vjp(a, sp, strength=STRENGTH), engine.mlp_vjp(b, sp, strength=STRENGTH)
    for key in ("outputs", "energy", "gx"):
        assert np.array_equal(bits(ra[key].to_host()), bits(rb[key].to_host())), key
    if name == "thin":      # LayerNorm over width 1 on both sides: a function of the betas alone
        assert np.all(np.isfinite(fwd)) and np.all(bits(fwd) == bits(fwd[:1]))
    else:
        assert np.unique(fwd, axis=0).shape[0] == n


@pytest.mark.parametrize("name", ["head_off", "deep8"])
def test_envelope_training(engine, name):
    c, sp = P.case(name), spec(name)
    m, n = 40, 80
    X = P.frames(name, n)
    it, itau = P.pairs(name, m, n)
    xd = engine.to_device(np.ascontiguousarray(X))
    assert engine.mlp_plan("train_backward", sp, 2 * m, c["xdtype"])["param_chunks"] == 1
    for drop in (None, P.dropout_of(name)):
        law = P.loss_grad(c, X, it, itau, dropout=drop)
        got = engine.mlp_loss_grad(xd, sp, it, itau, dropout=drop, seed=P.SEED, step=P.STEP, want_outputs=True,
                                   **T.LOSS_OPTS)
        print(f"{name}, dropout {drop}: loss device {got['loss']!r} law {law['loss']!r}")
        assert abs(got["loss"] - law["loss"]) <= TOL * abs(law["loss"])
        assert abs(got["score"] - law["score"]) <= TOL * abs(law["score"])
        assert close(got["outputs"].to_host(), law["outputs"])
        check_grads(c, got["grad"].to_host(), law)


# ---- d. strides and untouched memory ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["head_off", "deep8"])
def test_strided_forward_and_vjp(engine, name):
    sp = spec(name)
    net = Net(engine, sp)
    n, pad = 37, 3
    X = P.frames(name, n)
    F, d = X.shape[1], int(net.w[-1])
    gout = P.upstream(name, n)
    xd, gd = padded(engine, X, pad), padded(engine, gout, pad)
    packed_x = engine.to_device(np.ascontiguousarray(X))
    fwd = engine.mlp_forward(packed_x, sp).to_host()
    ref = engine.mlp_vjp(packed_x, sp, gout=engine.to_device(gout), strength=STRENGTH)
    od = filled(engine, (n, d + pad))
    for _ in range(2):                               # a second call into the same buffers gives the same bits
        assert c_forward(net, xd, n, F + pad, od, d + pad) == _lib.MSM_OK, net.message()
        out = od.to_host()
        assert untouched(out[:, d:]) and np.array_equal(bits(out[:, :d]), bits(fwd))
    od, gxd, ed, wd = filled(engine, (n, d + pad)), filled(engine, (n, F + pad)), filled(engine, (n,)), vjp_work(engine, net, n)
    for _ in range(2):
        assert c_vjp(net, xd, n, F + pad, gd, d + pad, ed, od, d + pad, gxd, F + pad, wd) == _lib.MSM_OK, net.message()
        out, gx = od.to_host(), gxd.to_host()
        assert untouched(out[:, d:]) and untouched(gx[:, F:])
        assert np.array_equal(bits(out[:, :d]), bits(fwd)) and np.array_equal(bits(gx[:, :F]), bits(ref["gx"].to_host()))
        assert np.array_equal(bits(ed.to_host()), bits(ref["energy"].to_host()))
    # n = 0: OK, and nothing is written
    od, gxd, ed = filled(engine, (n, d + pad)), filled(engine, (n, F + pad)), filled(engine, (n,))
    assert c_forward(net, xd, 0, F + pad, od, d + pad) == _lib.MSM_OK
    assert c_vjp(net, xd, 0, F + pad, gd, d + pad, ed, od, d + pad, gxd, F + pad, wd) == _lib.MSM_OK
    assert untouched(od.to_host()) and untouched(gxd.to_host()) and untouched(ed.to_host())


@pytest.mark.parametrize("name", ["head_off", "deep8"])
def test_strided_loss_grad(engine, name):
    m, n = 40, 80
    X = P.frames(name, n)
    it, itau = P.pairs(name, m, n)
    drop = P.dropout_of(name)
    d = P.case(name)["widths"][-1]
    _, stats, grad, out = run_loss_grad(engine, name, X, it, itau, drop)
    assert not untouched(out) and np.isfinite(stats[0])
    for _ in range(2):
        _, stats_p, grad_p, out_p = run_loss_grad(engine, name, X, it, itau, drop, pad=3)
        assert untouched(out_p[:, d:]) and np.array_equal(bits(out_p[:, :d]), bits(out))
        assert np.array_equal(bits(grad_p), bits(grad)) and np.array_equal(bits(stats_p[:16]), bits(stats[:16]))
    _, stats_n, grad_n, _ = run_loss_grad(engine, name, X, it, itau, drop, pad=3, want_out=False)     # d_out = NULL
    assert np.array_equal(bits(grad_n), bits(grad)) and np.array_equal(bits(stats_n[:16]), bits(stats[:16]))
    # the wrapper's call is the same call
    got = engine.mlp_loss_grad(engine.to_device(np.ascontiguousarray(X)), spec(name), it, itau, dropout=drop,
                               seed=P.SEED, step=P.STEP, **T.LOSS_OPTS)
    assert got["loss"] == stats[0] and np.array_equal(bits(got["grad"].to_host()), bits(grad))


# ---- e. a row outside [0, n) -----------------------------------------------------------------------------------------
def test_out_of_range_rows_are_not_read(engine):
    name = "head_off"
    m, n = 40, 80
    X = P.frames(name, n)
    it, itau = P.pairs(name, m, n)
    _, stats, _, clean = run_loss_grad(engine, name, X, it, itau, None)
    assert np.isfinite(stats[0]) and stats[9] == 0.0
    for side, pair, value in ((0, 7, -1), (1, 11, n)):
        idx = [it.copy(), itau.copy()]
        idx[side][pair] = value
        st, stats, _, out = run_loss_grad(engine, name, X, idx[0], idx[1], None)
        slot = side * m + pair
        keep = np.arange(2 * m) != slot
        assert st == _lib.MSM_OK and np.isnan(stats[0])
        assert np.all(np.isnan(out[slot])) and np.array_equal(bits(out[keep]), bits(clean[keep]))
        with pytest.raises(IndexError):                  # the wrapper still refuses the same indices
            engine.mlp_loss_grad(engine.to_device(np.ascontiguousarray(X)), spec(name), idx[0], idx[1])


# ---- f. refusals launch nothing --------------------------------------------------------------------------------------
def test_refusals_launch_nothing(engine):
    name = "head_off"
    sp = spec(name)
    m, n = 40, 80
    X = P.frames(name, n)
    F, d = X.shape[1], sp.widths[-1]
    it, itau = P.pairs(name, m, n)
    xd = engine.to_device(np.ascontiguousarray(X))
    itd, itaud = engine.to_device(it), engine.to_device(itau)
    good = Net(engine, sp)
    od, gxd, ed = filled(engine, (2 * m, d)), filled(engine, (n, F)), filled(engine, (n,))
    sd, gd = filled(engine, (_lib.VAMP2_STATS,)), filled(engine, (good.n_params,))
    wv, wt = vjp_work(engine, good, n), train_work(engine, good, m)
    INV, UNS = _lib.MSM_ERR_INVALID, _lib.MSM_ERR_UNSUPPORTED

    def forward(net=good):
        return c_forward(net, xd, n, F, od, d)

    def vjp(net=good, work_bytes=None):
        return c_vjp(net, xd, n, F, None, 0, ed, od, d, gxd, F, wv, work_bytes)

    def loss(net=good, pairs=m, drop=None, work_bytes=None, step=P.STEP):
        return c_loss_grad(net, xd, n, F, itd, itaud, pairs, drop, sd, gd, od, d, wt, work_bytes, step)

    def plan(net, kernel, rows):
        out = (ctypes.c_int64 * 8)()
        return lib.msm_mlp_launch_plan(engine.handle, _lib.MLP_KERNELS[kernel], _lib.MSM_F32, rows, *net.flags(), out)

    wide, deep, many = Net(engine, sp, widths=(7, 257, 16, 3)), Net(engine, sp, widths=(7,) + (8,) * 8 + (3,)), \
        Net(engine, sp, widths=(7, 32, 16, 65))
    short = Net(engine, sp, n_params=good.n_params - 1)
    alone = Net(engine, sp, with_scale=False)
    cases = [
        ("1 frame pairs", INV, [lambda: loss(pairs=1), lambda: plan(good, "train_forward", 2)]),
        (f"{(1 << 24) + 1} frame pairs", UNS, [lambda: loss(pairs=(1 << 24) + 1),
                                               lambda: plan(good, "train_backward", 2 * ((1 << 24) + 1))]),
        ("width 257", UNS, [lambda: forward(wide), lambda: vjp(wide), lambda: loss(wide),
                            lambda: plan(wide, "forward", n), lambda: plan(wide, "train_forward", 2 * m)]),
        ("9 Linear layers", UNS, [lambda: forward(deep), lambda: vjp(deep), lambda: loss(deep),
                                  lambda: plan(deep, "vjp", n)]),
        ("65 outputs", UNS, [lambda: forward(many), lambda: vjp(many), lambda: loss(many),
                             lambda: plan(many, "train_backward", 2 * m)]),
        (f"{good.n_params - 1} parameters given", INV, [lambda: forward(short), lambda: vjp(short), lambda: loss(short)]),
        ("workspace of", INV, [lambda: vjp(work_bytes=int(lib.msm_mlp_vjp_workspace(n, *good.flags())) - 1),
                               lambda: loss(work_bytes=int(lib.msm_mlp_train_workspace(m, *good.flags())) - 1)]),
        ("dropout probability 1", INV, [lambda: loss(drop=[0.1, 1.0, 0.0])]),
        (f"step {1 << 32}", INV, [lambda: loss(step=1 << 32)]),
        ("go together", INV, [lambda: forward(alone), lambda: vjp(alone), lambda: loss(alone)]),
    ]
    assert int(lib.msm_mlp_vjp_workspace(n, *good.flags())) > 8          # head_off has a tape: one byte short is short
    for text, code, calls in cases:
        for call in calls:
            st = call()
            print(f"  {text!r}: status {st}, message {good.message()!r}")
            assert st == code and text in good.message(), (text, st, good.message())
    engine.sync()
    for buf in (od, gxd, ed, sd, gd):
        assert untouched(buf.to_host())
    # after all of it ordinary calls succeed
    assert forward() == _lib.MSM_OK and vjp() == _lib.MSM_OK and loss() == _lib.MSM_OK, good.message()
    assert plan(good, "train_forward", 2 * m) == _lib.MSM_OK
    assert np.isfinite(sd.to_host()[0]) and np.all(np.isfinite(gxd.to_host()))
