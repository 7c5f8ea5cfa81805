"""The deferred chain of Lloyd passes (msm_kmeans_lloyd_pass_deferred / msm_kmeans_assign_closing) against the ticket
chain (msm_kmeans_lloyd_pass_from + msm_kmeans_assign_packed), bit for bit after EVERY launch.

The ticket chain is the reference: tests/test_gpu_kmeans_fit.py, test_gpu_step_folds.py and test_gpu_kmeans_accum_waves.py
pin it to the C oracle.  Launch i + 1 of the deferred chain closes the iteration of launch i, so what is compared is

    after deferred launch i + 1 (a pass, or the closing assign)     after ticket pass i
        centres it wrote (centers_out)                           =      centres
        fit state (shift2, n_iter, done, ... all 8 words)        =      fit state
    after deferred pass i                                           after ticket pass i
        member sums, counts (the pass's `out` buffer), labels    =      member sums, counts, labels
    closing assign                                                  kmeans_assign under the final centres
        labels, mindist                                          =      labels, mindist

The member sums of the deferred chain rotate through three buffers and the centres through two; the tests drive the
rotation the way ShardedMSM.step does.
"""
import numpy as np
import pytest

from pmarlo_amd.dist import ShardConfig, ShardedMSM
from tests import _gen
from tests import _kmeans_ref as kr

pytestmark = pytest.mark.gpu

CLOSE_CH = 5                                  # kFilterCloseCH: the prologue close takes k d <= 5 x 1024 elements
CLOSE_LDS_CAP = 160 * 1024 - 256              # filter_lds_bytes_close


def close_lds_bytes(k: int, d: int, accum: bool) -> int:
    """filter_lds_bytes_close restated: the filter's LDS plus the fp64 centre table; 0 when it does not fit."""
    base = kr.filter_lds_bytes(k, d, accum)
    total = base + k * d * 8
    return total if base and total <= CLOSE_LDS_CAP else 0


def close_fits(k: int, d: int, accum: bool = True) -> bool:
    return 4 < d <= 10 and k * d <= 1024 * CLOSE_CH and close_lds_bytes(k, d, accum) != 0


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), f"{what}: bits differ"


class _Fit:
    """The buffers of one fit over Y [n, d] from given start centres."""

    def __init__(self, engine, Y, centres, tol2):
        self.eng, self.Y = engine, Y
        self.n, self.d = Y.shape
        self.k = k = centres.shape[0]
        d = self.d
        self.cen = [engine.empty((k, d), np.float64).fill_bytes_(0x5A) for _ in range(2)]
        self.state = engine.zeros((8,), np.float64)
        self.labels = engine.empty((self.n,), np.int32).fill_bytes_(0x5A)      # first_pass: never read
        self.acc = [engine.empty((k * d + k,), np.int64).fill_bytes_(0x5A) for _ in range(3)]
        self.rot = [(a.view((k * d,)), a.view((k,), offset_elems=k * d)) for a in self.acc]
        engine.kmeans_fit_begin(Y, k, seed=0, n_total=self.n, tol2=tol2, centers=self.cen[0], state=self.state,
                                init_centers=False, sums=self.rot[0][0], counts=self.rot[0][1])
        self.cen[0].copy_from_host(np.ascontiguousarray(centres, np.float64))
        nbytes = engine.kmeans_image_bytes(self.n, d)
        self.image = engine.kmeans_pack(Y, image=engine.empty((nbytes,), np.uint8),
                                        absmax=self.state.view((1,), offset_elems=2))


def _ticket_chain(engine, Y, centres, iters, tol2, want_mindist):
    f = _Fit(engine, Y, centres, tol2)
    trace = []
    for it in range(iters):
        engine.kmeans_lloyd_pass(Y, f.cen[0], f.state, *f.rot[0], image=f.image, prev_labels=f.labels, first_pass=it == 0)
        trace.append({"centres": f.cen[0].to_host(), "state": f.state.to_host(), "sums": f.rot[0][0].to_host(),
                      "counts": f.rot[0][1].to_host(), "labels": f.labels.to_host()})
    mind = engine.empty((f.n,), np.float64) if want_mindist else None
    engine.kmeans_assign(Y, f.cen[0], labels=f.labels, image=f.image, mindist=mind)
    final = {"labels": f.labels.to_host(), "centres": f.cen[0].to_host(), "state": f.state.to_host()}
    if want_mindist:
        final["mindist"] = mind.to_host()
    return trace, final


def _deferred_chain(engine, Y, centres, iters, tol2, want_mindist):
    """-> (per-pass trace, final), or None where the flavour does not take the shape (nothing launched)."""
    f = _Fit(engine, Y, centres, tol2)
    trace = []
    for it in range(iters):
        cin, cout = (f.cen[(it - 1) & 1], f.cen[it & 1]) if it else (f.cen[0], f.cen[0])
        ran = engine.kmeans_lloyd_pass_deferred(Y, cin, cout, f.state, f.rot[(it - 1) % 3] if it else None, f.rot[it % 3],
                                                f.rot[(it + 1) % 3], image=f.image, prev_labels=f.labels,
                                                close_pending=it > 0, first_pass=it == 0)
        if not ran:
            assert it == 0
            return None
        # the close of pass it - 1 happened in this launch; the sums / labels are this pass's own
        trace.append({"centres_prev": cout.to_host() if it else None, "state_prev": f.state.to_host() if it else None,
                      "sums": f.rot[it % 3][0].to_host(), "counts": f.rot[it % 3][1].to_host(), "labels": f.labels.to_host(),
                      "next_sums": f.acc[(it + 1) % 3].to_host()})
    mind = engine.empty((f.n,), np.float64).fill_bytes_(0x5A) if want_mindist else None
    cin, cout = f.cen[(iters - 1) & 1], f.cen[iters & 1]
    assert engine.kmeans_assign_closing(Y, cin, cout, f.state, f.rot[(iters - 1) % 3], image=f.image, labels=f.labels,
                                        close_pending=True, mindist=mind)
    final = {"labels": f.labels.to_host(), "centres": cout.to_host(), "state": f.state.to_host(),
             "caller_buffer": (iters & 1) == 0}
    if want_mindist:
        final["mindist"] = mind.to_host()
    return trace, final


def _compare_chains(engine, Y_host, centres, iters, tol2=0.0, want_mindist=False):
    Y = engine.to_device(np.ascontiguousarray(Y_host, np.float64))
    k, d = centres.shape
    assert close_fits(k, d), "the case must run the deferred flavour"
    want, wfinal = _ticket_chain(engine, Y, centres, iters, tol2, want_mindist)
    got = _deferred_chain(engine, Y, centres, iters, tol2, want_mindist)
    assert got is not None, "the deferred flavour did not take a shape its rule admits"
    got, gfinal = got
    for it in range(iters):
        for nm in ("sums", "counts", "labels"):
            _same(got[it][nm], want[it][nm], f"{nm} after pass {it + 1}")
        assert not got[it]["next_sums"].any(), f"pass {it + 1} did not clear the next launch's member sums"
        if it:
            _same(got[it]["centres_prev"], want[it - 1]["centres"], f"centres closed by launch {it + 1}")
            _same(got[it]["state_prev"], want[it - 1]["state"], f"fit state closed by launch {it + 1}")
    for nm in ("centres", "state", "labels") + (("mindist",) if want_mindist else ()):
        _same(gfinal[nm], wfinal[nm], f"{nm} after the closing assign")
    return want, wfinal, gfinal


def _start_centres(Y, k, seed):
    """k frames as start centres (with repeats when there are fewer frames than centres)."""
    rng = np.random.default_rng(seed)
    n = Y.shape[0]
    return Y[rng.choice(n, size=k, replace=n < k)].copy()


# n: fewer frames than one unit of 64; 64 units + 37 frames (several workgroups, a ragged last unit).  iters: even and odd --
# the final centres end in the caller's buffer (even) or in the second one (odd), as ShardedMSM expects
@pytest.mark.parametrize("iters", [4, 5])
@pytest.mark.parametrize("k", [3, 17, 500])
@pytest.mark.parametrize("d", [5, 10])
@pytest.mark.parametrize("n", [50, 4133])
def test_sizes(engine, n, d, k, iters):
    Y = _gen.correlated_series(n, d, seed=n + d + k).astype(np.float64)
    _, wfinal, gfinal = _compare_chains(engine, Y, _start_centres(Y, k, seed=k), iters)
    assert gfinal["caller_buffer"] == (iters % 2 == 0)
    assert wfinal["state"][6] == iters or wfinal["state"][5] == 1.0           # n_iter, unless the fit converged


def test_empty_cluster_keeps_its_coordinates(engine):
    n, d, k = 4133, 10, 17
    Y = _gen.correlated_series(n, d, seed=2).astype(np.float64)
    centres = _start_centres(Y, k, seed=4)
    centres[5] = 1.0e3 + np.arange(d)                       # far from every frame: never a member
    want, wfinal, gfinal = _compare_chains(engine, Y, centres, iters=3)
    assert all(t["counts"][5] == 0 for t in want)
    _same(gfinal["centres"][5], centres[5], "the empty centre")
    assert not np.array_equal(gfinal["centres"][4], centres[4])


def test_convergence(engine):
    d, k = 5, 4
    pts = np.array([[0.0] * d, [1.0] + [0.0] * (d - 1), [0.0, 2.0] + [0.0] * (d - 2), [3.0] * d])
    Y = np.tile(pts, (40, 1))                               # 4 distinct points, repeated
    centres = pts + 0.125                                   # pass 1 moves every centre onto its point, pass 2 moves nothing
    want, wfinal, gfinal = _compare_chains(engine, Y, centres, iters=5, tol2=0.0, want_mindist=True)
    assert [t["state"][5] for t in want] == [0.0, 1.0, 1.0, 1.0, 1.0]         # done at iteration 2
    assert wfinal["state"][6] == 2.0 == gfinal["state"][6]                    # n_iter stays there
    _same(gfinal["centres"], pts, "converged centres")
    np.testing.assert_array_equal(gfinal["mindist"], 0.0)
    # and with an even number of passes: the copies of a converged fit keep the centre rotation going
    _compare_chains(engine, Y, centres, iters=4, tol2=0.0)


@pytest.mark.parametrize("d,k", [(10, 17), (5, 500)])
def test_scan_paths(engine, d, k):
    """Frames that leave the certified pick (step 4 and the plain fp64 scan): their fp64 centre rows now come from the LDS."""
    n = 4133
    rng = np.random.default_rng(d * k)
    Y = _gen.correlated_series(n, d, seed=7).astype(np.float64)
    centres = _start_centres(Y, k, seed=1)
    centres[1] = centres[0]                                             # duplicated centres
    centres[3] = centres[2] * (1.0 + 2.0 ** -50)                        # near-ties below fp32 resolution
    Y[100] = 0.5 * (centres[0] + centres[2])                            # a frame halfway between two centres
    Y[200:264] = centres[2] + rng.normal(size=(64, d)) * 1e-9
    Y[300, d // 2] = np.nan                                             # a NaN frame: label 0, as the all-fp64 scan
    Y[400, 0] = 1e-15                                                   # below the fp16 operands' range
    Y[500, d - 1] = 1e17                                                # above the filter's scaled range guard
    want, wfinal, gfinal = _compare_chains(engine, Y, centres, iters=3, want_mindist=True)
    assert wfinal["labels"][300] == 0


def _largest_k(d: int) -> int:
    k = 1
    while close_fits(k + 1, d):
        k += 1
    return k


@pytest.mark.parametrize("d", [10, 5], ids=["d10-one-round-of-loads", "d5-lds-bytes"])
def test_lds_rule(engine, monkeypatch, capfd, d):
    """The largest k the flavour admits and that k + 1, through the MSM_KMEANS_DEBUG line of the launch that ran."""
    k = _largest_k(d)
    if d == 10:
        assert k == 512 and close_lds_bytes(513, 10, True)      # k d <= 5120 binds here, not the LDS
    else:
        assert k * d < 1024 * CLOSE_CH and not close_lds_bytes(k + 1, d, True)      # the LDS binds
    n = 900
    Y = _gen.correlated_series(n, d, seed=d).astype(np.float64)
    monkeypatch.setenv("MSM_KMEANS_DEBUG", "1")
    for kk, runs in ((k, True), (k + 1, False)):
        Yd = engine.to_device(Y)
        centres = _start_centres(Y, kk, seed=kk)
        capfd.readouterr()
        got = _deferred_chain(engine, Yd, centres, 2, 0.0, False)
        engine.sync()
        lines = kr.debug_lines(capfd.readouterr().err)
        if runs:
            assert got is not None and len(lines) == 3 and all("close=prologue" in ln for ln in lines), lines
            assert f"lds={close_lds_bytes(kk, d, True)}" in lines[0] and f"lds={close_lds_bytes(kk, d, False)}" in lines[2]
            want = _ticket_chain(engine, Yd, centres, 2, 0.0, False)
            for nm in ("centres", "state", "labels"):
                _same(got[1][nm], want[1][nm], f"{nm} at the largest k")
        else:
            assert got is None and not lines, lines            # not applicable: nothing launched
            # ... and the caller's fallback is the ticket chain, which says so
            capfd.readouterr()
            _ticket_chain(engine, Yd, centres, 1, 0.0, False)
            lines = kr.debug_lines(capfd.readouterr().err)
            assert lines and not any("close=prologue" in ln for ln in lines), lines


def test_sharded_step_end_to_end(engine, monkeypatch):
    n, F, d, k = 20_000, 16, 10, 64
    X = _gen.correlated_series(n, F, seed=5).astype(np.float32)
    outs = {}
    for iters in (3, 4):                                     # odd: the final centres come back by one device copy
        cfg = ShardConfig(n_frames=n, n_features=F, tica_dim=d, k=k, lag=2, kmeans_iters=iters, seed=1)
        for tag in ("ticket", "deferred"):
            if tag == "ticket":
                monkeypatch.setenv("MSM_KMEANS_DEFERRED_CLOSE", "0")
            else:
                monkeypatch.delenv("MSM_KMEANS_DEFERRED_CLOSE", raising=False)
            msm = ShardedMSM(engine, cfg, engine.to_device(X))
            assert msm.deferred == (tag == "deferred")
            for _ in range(2):                               # the second step starts from what the first left behind
                msm.step()
            engine.sync()
            assert msm.deferred == (tag == "deferred")       # the shape was taken
            outs[tag] = {"labels": msm.labels.to_host(), "centers": msm.buf["centers"].to_host(),
                         "counts": msm.buf["counts"].to_host(), "T": msm.T.to_host(),
                         "km_acc": msm.buf["km_acc"].to_host(), "fit_state": msm.buf["fit_state"].to_host()}
        for nm in outs["ticket"]:
            _same(outs["deferred"][nm], outs["ticket"][nm], f"{nm} ({iters} iterations)")
