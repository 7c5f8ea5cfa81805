"""Lagged covariance moments (csrc/cov.hip) on every launch path, compared exactly.

Each row of tests/_cov_ref.CASES is run through the C entry it names (plain, reversible, one-sided), with and without
assume_finite, on a wide buffer [n, ld] whose pad columns and out-of-segment frames hold 2^100, and M00, M0t, sx, sy
and T are compared with np.testing.assert_array_equal against exact_moments: the data are integers whose partial sums
all stay below 2^52, so a correct kernel is bit-equal to the reference in any summation order and no tolerance exists
anywhere in this file.  tests/test_cov_reference.py proves on the CPU that the rows reach the branches they name (tile
counts, vector / guarded loads, wave pairs, the ring at every length class, heads, tails, the blocked kernel, ...).
The same buffer then goes through msm_moments_from_lagged.  Further tests place real NaNs where each code path reads
them, run calls without a single pair, pass one segment too many, and reuse the scratch slabs of a larger launch.

Not covered: the guard on the ring's 32-bit lane offsets (ld * 4 * sizeof(T) >= 2^31 falls back to guarded loads)
needs a buffer of several gigabytes; the rule itself is checked on the CPU."""

from __future__ import annotations

import numpy as np
import pytest

from pmarlo_amd import _lib
from pmarlo_amd._lib import lib
from tests import _cov_ref as cr

pytestmark = pytest.mark.gpu

GUARD = 64                 # doubles on either side of every output
OUT_FILL = -1234.5625      # no sum of integers and halves
ENTRY = {"plain": "msm_lagged_moments", "symmetric": "msm_lagged_moments_reversible",
         "onesided": "msm_lagged_moments_onesided"}
_REF: dict = {}


@pytest.fixture(scope="module")
def n_cu(engine) -> int:
    return engine.info()["n_cu"]


def _reference(row: dict, X, shift, flavour: str, impute_nan: bool = False) -> dict:
    key = (row["name"], row["n"], row["lag"], flavour, impute_nan)
    if key not in _REF:
        _REF[key] = cr.exact_moments(X, row["segs"], row["lag"], shift, flavour, impute_nan=impute_nan)
    return _REF[key]


def _upload(engine, row: dict, X):
    """The wide buffer of a row on the device -> (allocation, pointer to frame 0).  Only [segment frames, :F] hold data."""
    n, F, ld = row["n"], row["F"], row["ld"]
    off = 0 if row["aligned"] else 1
    host = np.full(off + n * ld, cr.SENTINEL, cr.NP_DTYPE[row["dtype"]])
    frames = host[off:].reshape(n, ld)
    for a, b in cr.clip_segments(n, row["segs"]):
        if b > a:
            frames[a:b, :F] = X[a:b]
    buf = engine.to_device(host)
    return buf, buf.ptr + off * host.itemsize


def _seg_args(segs):
    if segs is None:
        return None, None, 0, ()
    starts = np.ascontiguousarray([a for a, _ in segs], np.int64)
    stops = np.ascontiguousarray([b for _, b in segs], np.int64)
    return starts.ctypes.data, stops.ctypes.data, len(segs), (starts, stops)


def _guarded(engine, size: int):
    return engine.to_device(np.full(GUARD + size + GUARD, OUT_FILL))


def _payload(blk, size: int, tag) -> np.ndarray:
    """The output between the guard bands, after checking that the bands were left alone."""
    host = blk.to_host()
    np.testing.assert_array_equal(host[:GUARD], OUT_FILL, err_msg=f"{tag}: written below the output")
    np.testing.assert_array_equal(host[GUARD + size:], OUT_FILL, err_msg=f"{tag}: written past the output")
    return host[GUARD:GUARD + size]


def _moments(engine, row: dict, ptr: int, shift_d, flavour: str, finite: int, blk=None):
    """One call of the flavour's C entry -> (status, guarded output block)."""
    F = row["F"]
    blk = blk if blk is not None else _guarded(engine, 2 * F * F + 2 * F + 1)
    p0, p1, n_seg, keep = _seg_args(row["segs"])
    st = getattr(lib, ENTRY[flavour])(engine.handle, ptr, _lib.MSM_F32 if row["dtype"] == "f32" else _lib.MSM_F64,
                                      row["n"], F, row["ld"], p0, p1, n_seg, row["lag"], shift_d.ptr, finite,
                                      blk.ptr + GUARD * 8)
    del keep
    return st, blk


def _check_moments(out: np.ndarray, ref: dict, F: int, flavour: str, tag):
    assert not np.any(out == OUT_FILL), f"{tag}: {int(np.sum(out == OUT_FILL))} elements were never written"
    M00, M0t = out[:F * F].reshape(F, F), out[F * F:2 * F * F].reshape(F, F)
    np.testing.assert_array_equal(M00, ref["M00"], err_msg=f"{tag} M00")
    np.testing.assert_array_equal(M0t, ref["M0t"], err_msg=f"{tag} M0t")
    np.testing.assert_array_equal(out[2 * F * F:2 * F * F + F], ref["sx"], err_msg=f"{tag} sx")
    np.testing.assert_array_equal(out[2 * F * F + F:2 * F * F + 2 * F], ref["sy"], err_msg=f"{tag} sy")
    assert out[-1] == ref["T"], (tag, out[-1], ref["T"])
    np.testing.assert_array_equal(M00, M00.T, err_msg=f"{tag} M00 symmetry")
    if flavour == "symmetric":
        np.testing.assert_array_equal(M0t, M0t.T, err_msg=f"{tag} M0t symmetry")


def _run_row(engine, row: dict, flavours=None, finites=(0, 1)) -> dict:
    """Every call a row asks for, checked; -> {(flavour, finite): payload}."""
    X, shift = cr.case_data(row)
    F, size = row["F"], 2 * row["F"] ** 2 + 2 * row["F"] + 1
    buf, ptr = _upload(engine, row, X)
    shift_d = engine.to_device(shift)
    outs = {}
    plain_blk = None
    for flavour in flavours or dict.fromkeys((row["flavour"], "plain")):     # the row's own entry, and the plain one
        for finite in finites:                                               # for msm_moments_from_lagged below
            tag = f"{row['name']} [{flavour}, assume_finite={finite}]"
            st, blk = _moments(engine, row, ptr, shift_d, flavour, finite)
            assert st == _lib.MSM_OK, (tag, st, lib.msm_last_error(engine.handle))
            out = _payload(blk, size, tag)
            _check_moments(out, _reference(row, X, shift, flavour), F, flavour, tag)
            outs[(flavour, finite)] = out
            if flavour == "plain" and finite == 0:
                plain_blk = blk
    if row["lag"] >= 1 and plain_blk is not None:
        tag = f"{row['name']} [moments_from_lagged]"
        sums = _guarded(engine, 3 * F)
        p0, p1, n_seg, keep = _seg_args(row["segs"])
        st = lib.msm_moments_from_lagged(engine.handle, ptr, _lib.MSM_F32 if row["dtype"] == "f32" else _lib.MSM_F64,
                                         row["n"], F, row["ld"], p0, p1, n_seg, row["lag"], shift_d.ptr,
                                         plain_blk.ptr + GUARD * 8, sums.ptr + GUARD * 8)
        del keep
        if n_seg > cr.SEG_INLINE:       # this entry counts the short segments too: it refuses, and writes nothing
            assert st == _lib.MSM_ERR_INVALID and b"at most 16 segments" in lib.msm_last_error(engine.handle), (tag, st)
            np.testing.assert_array_equal(_payload(sums, 3 * F, tag), OUT_FILL, err_msg=tag)
        else:
            assert st == _lib.MSM_OK, (tag, st, lib.msm_last_error(engine.handle))
            np.testing.assert_array_equal(_payload(sums, 3 * F, tag), cr.exact_column_sums(X, row["segs"], shift),
                                          err_msg=tag)
    del buf
    return outs


@pytest.mark.parametrize("row", cr.CASES, ids=cr.case_ids())
def test_row_is_exact(engine, n_cu, row):
    row = cr.resolve(row, n_cu)
    got = cr.reached(cr.row_path(row, n_cu), row["lag"])
    assert not cr.covers(got, row["reach"]), (n_cu, row["name"], cr.covers(got, row["reach"]))   # on THIS device too
    _run_row(engine, row)


# NaN placement: (F, ld) per kernel; one segment of 122 (two out-of-segment lanes re-read the last frame) and of 113
# frames (length 1 mod 4: three of them), lag 2.  With 32 frames per wave, frames 40, 42 and 70 lie in the rings of
# waves 1 and 2 on the vector kernels, 42 being the partner of 40.
_NAN_SHAPES = [(16, 16), (32, 34), (40, 40), (64, 64), (65, 66), (128, 128)]


def _nan_frames(n: int, lag: int) -> dict:
    return {"ring interior": [40, 70], "ring interior and its partner": [42], "first lag frames": [0, lag - 1],
            "partner only": [n - lag], "last frame": [n - 1]}


@pytest.mark.parametrize("flavour", ["plain", "symmetric"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("F,ld", _NAN_SHAPES)
def test_nan_is_imputed_wherever_it_is_read(engine, n_cu, F, ld, dtype, flavour):
    lag = 2
    for n in (122, 113):
        row = {"name": f"nan-F{F}-{dtype}-{flavour}-n{n}", "n": n, "F": F, "ld": ld, "lag": lag, "dtype": dtype,
               "aligned": True, "segs": None, "flavour": flavour, "family": "small", "seed": 77 + n + F}
        path = cr.row_path(row, n_cu)
        pieces = {q["wave"]: q for q in path["pieces"]}
        if path["vec"] and not path["blocked"]:                  # the placement is what the comment above says
            assert path["frames_per_wave"] == 32 and pieces[1]["ring"] == 8 and pieces[2]["ring"] == 8
            assert pieces[0]["head"] == 1 and pieces[3]["tail"] >= 1
        X, shift = cr.case_data(row)
        for q, (what, frames) in enumerate(_nan_frames(n, lag).items()):
            for t in frames:
                X[t, (5 * q + t) % F] = np.nan      # a column of its own ...
                X[t, F - 1] = np.nan                # ... and one that collects them all
        X[40, 0] = X[42, 0] = np.nan                # x and its partner in one column
        assert np.isnan(X).sum() >= 9
        buf, ptr = _upload(engine, row, X)
        shift_d = engine.to_device(shift)
        st, blk = _moments(engine, row, ptr, shift_d, flavour, 0)
        assert st == _lib.MSM_OK, (row["name"], st)
        out = _payload(blk, 2 * F * F + 2 * F + 1, row["name"])
        assert np.all(np.isfinite(out)), (row["name"], int(np.sum(~np.isfinite(out))))
        _check_moments(out, cr.exact_moments(X, None, lag, shift, flavour, impute_nan=True), F, flavour, row["name"])
        del buf


@pytest.mark.parametrize("F", [16, 48, 64, 100])
def test_no_pairs_gives_a_zero_block(engine, F):
    size = 2 * F * F + 2 * F + 1
    shift_d = engine.to_device(np.zeros(F))
    for flavour in cr.FLAVOURS:
        # every segment is no longer than the lag
        row = {"name": f"nopairs-F{F}", "n": 40, "F": F, "ld": F + 3, "lag": 7, "dtype": "f32", "aligned": True,
               "segs": [(0, 7), (8, 10), (12, 19), (30, 30), (33, 47)], "flavour": flavour}
        buf, ptr = _upload(engine, row, np.ones((40, F)))
        st, blk = _moments(engine, row, ptr, shift_d, flavour, 0)
        assert st == _lib.MSM_OK
        np.testing.assert_array_equal(_payload(blk, size, row["name"]), 0.0)
        # no frames at all, no buffer
        row = dict(row, n=0, segs=None, ld=F, lag=1)
        st, blk = _moments(engine, row, None, shift_d, flavour, 1)
        assert st == _lib.MSM_OK
        np.testing.assert_array_equal(_payload(blk, size, "n = 0"), 0.0)
        del buf


def test_seventeen_live_segments_are_refused(engine):
    F = 16
    segs = [(10 * i, 10 * i + 6) for i in range(17)]
    row = {"name": "seventeen", "n": 170, "F": F, "ld": F, "lag": 2, "dtype": "f64", "aligned": True, "segs": segs}
    X, shift = cr.small(170, F, 3)
    buf, ptr = _upload(engine, row, X)
    shift_d = engine.to_device(shift)
    for flavour in cr.FLAVOURS:
        st, blk = _moments(engine, row, ptr, shift_d, flavour, 0)
        assert st == _lib.MSM_ERR_UNSUPPORTED, (flavour, st)
        msg = lib.msm_last_error(engine.handle).decode()
        assert "more than 16 segments per call; accumulate over several calls" in msg, msg
        np.testing.assert_array_equal(_payload(blk, 2 * F * F + 2 * F + 1, flavour), OUT_FILL)
    # a seventeenth that is no longer than the lag does not count, and sixteen are served
    row["segs"] = segs[:16] + [(166, 168)]
    row["name"], row["flavour"], row["family"], row["seed"] = "sixteen", "plain", "small", 3
    _run_row(engine, dict(row, segs=segs[:16]), flavours=("plain",))
    st, blk = _moments(engine, row, ptr, shift_d, "plain", 0)
    assert st == _lib.MSM_OK
    _check_moments(_payload(blk, 2 * F * F + 2 * F + 1, "sixteen + short"),
                   cr.exact_moments(X, row["segs"], 2, shift), F, "plain", "sixteen + short")
    del buf


def test_scratch_slabs_of_a_larger_launch_are_not_read(engine, n_cu):
    """Largest launch, smallest, a blocked one, largest again on the one engine: each result is what it was the first
    time (and exact: _run_row compares), although the scratch still holds the slabs of the launch before."""
    by = {r["name"]: r for r in cr.CASES}
    big = cr.resolve(by["longring-F64-f64-symmetric-lag2"], n_cu)
    small = by["ring-nt1-f32-plain-n121-lag1"]
    blocked = next(r for r in cr.CASES if r["name"].startswith("blocked-F129-ld129-al-f32-"))
    assert cr.row_path(big, n_cu)["blocks"] == n_cu and cr.row_path(small, n_cu)["blocks"] == 1
    first = {}
    for row in (big, small, blocked, big, blocked, small, big):
        outs = _run_row(engine, row, flavours=(row["flavour"],), finites=(0,))
        out = outs[(row["flavour"], 0)]
        if row["name"] in first:
            np.testing.assert_array_equal(out, first[row["name"]], err_msg=row["name"])
        first.setdefault(row["name"], out)


def test_engine_methods_take_a_row_stride(engine):
    """Engine.lagged_moments / moments_from_lagged with ld=: the left block of a wider buffer, one element off an
    allocation."""
    n, F, ld, lag = 122, 32, 37, 3
    X, shift = cr.wide(n, F, 11)
    segs = [(0, 50), (50, 52), (61, 122)]
    host = np.full(1 + n * ld, cr.SENTINEL, np.float32)
    frames = host[1:].reshape(n, ld)
    for a, b in segs:
        frames[a:b, :F] = X[a:b]
    buf = engine.to_device(host)
    x = buf.view((n, F), offset_elems=1)
    shift_d = engine.to_device(shift)
    starts, stops = np.array([a for a, _ in segs]), np.array([b for _, b in segs])
    for kw, flavour in (({}, "plain"), ({"symmetric": True}, "symmetric"), ({"one_sided": True}, "onesided")):
        mom = engine.lagged_moments(x, lag, shift_d, starts=starts, stops=stops, ld=ld, **kw)
        _check_moments(mom.to_host(), cr.exact_moments(X, segs, lag, shift, flavour), F, flavour, flavour)
        if flavour == "plain":
            sums = engine.moments_from_lagged(x, lag, shift_d, mom, starts=starts, stops=stops, ld=ld)
            np.testing.assert_array_equal(sums.to_host(), cr.exact_column_sums(X, segs, shift))
    with pytest.raises(ValueError):
        engine.lagged_moments(x, lag, shift_d, starts=starts, stops=stops, ld=F - 1)
