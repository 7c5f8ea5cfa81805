"""The per-kind featurizer kernels of csrc/featurize.hip on every launch path: distances_kernel, angles_kernel,
dihedrals_kernel (modes 0, 1, 2), contacts_kernel and rg_kernel against the exact laws of tests/_featurize_ref.py
(the fp32 coordinates widened to longdouble), and their non-finite rules against the restatements of oracle/npport.py.

Yardsticks (tests/_featurize_ref.py has the definitions, tests/test_featurize_reference.py re-measures them on the
host): with u = 2^-24 the fp32 restatement of the reference's operation order stays within
    K_d = 2.59 (relative distance error / u),
    K_a = 7.17 (angle error x max(sin theta, sqrt(u)) / u),
    K_t = 5.76 (dihedral error modulo 2 pi x max(s, sqrt(u)) / u,  s = the smaller sine of the two bond angles)
of the exact law over every input generated here (4099 frames x 12 atoms x 65 records per kind, coordinates O(1) and
offset by 50 and 1000 nm, one frame in eight a nearly straight chain; and the 4081 x 257 second-trip inputs).  The device
is held to TWICE each K: the factor covers contracted multiply-adds and the device's acosf / atan2f / cosf / sinf.

Values at the edges (a zero bond, collinear and planar atoms, a contact at the cutoff) and everything that must not
move (padding, the packed against the strided call, a second call) are compared as bits.  Strided calls go through the
C entry points with ld = width + 3 and col_off = 2 into buffers filled with one NaN bit pattern."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import npport
from pmarlo_amd import _lib
from pmarlo_amd._lib import lib
from tests import _featurize_ref as R

pytestmark = pytest.mark.gpu

U = R.U
FILL = np.uint32(0x7FC12345)                      # a quiet NaN with a payload: untouched words are recognisable
KINDS = ("distance", "angle", "dihedral", "contact")
TRIG = 4.0 * 2.0 ** -23                            # fp32 cos / sin of a given fp32 angle: 4 ulp of 1, OpenCL's bound


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def width_of(kind, m, mode=0):
    return 2 * m if kind == "dihedral" and mode else m


def launch(engine, kind, xd, n, A, td, m, od, ld, col_off, mode=0, rcut=R.RCUT):
    """One C entry point; returns (status, message)."""
    h, xp, tp, op = engine.handle, xd.ptr if xd is not None else None, td.ptr if td is not None else None, \
        od.ptr if od is not None else None
    if kind == "distance":
        st = lib.msm_featurize_distances(h, xp, n, A, tp, m, op, ld, col_off)
    elif kind == "angle":
        st = lib.msm_featurize_angles(h, xp, n, A, tp, m, op, ld, col_off)
    elif kind == "dihedral":
        st = lib.msm_featurize_dihedrals(h, xp, n, A, tp, m, mode, op, ld, col_off)
    elif kind == "contact":
        st = lib.msm_featurize_contacts(h, xp, n, A, tp, m, rcut, op, ld, col_off)
    else:
        st = lib.msm_featurize_rg(h, xp, n, A, op, ld, col_off)
    return st, lib.msm_last_error(h).decode()


def run(engine, kind, xyz, table=None, mode=0, rcut=R.RCUT, pad=0, col_off=0):
    """The whole [n, ld] buffer after one call into a FILL-ed buffer: ld = width + pad."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n, A = xyz.shape[:2]
    m = 0 if table is None else len(table)
    ld = (1 if kind == "rg" else width_of(kind, m, mode)) + pad
    xd = engine.to_device(xyz)
    td = None if table is None else engine.to_device(np.ascontiguousarray(table, np.int32))
    od = engine.to_device(np.full((n, ld), FILL, np.uint32).view(np.float32))
    st, msg = launch(engine, kind, xd, n, A, td, m, od, ld, col_off, mode, rcut)
    assert st == _lib.MSM_OK, msg
    return od.to_host()


def ratio(err, bound):
    return float((np.asarray(err, R.LD) / bound).max())


# ---------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_distances_relative_to_the_exact_length(engine, regime):
    xyz, table = R.inputs("distance", regime)
    d = R.exact("distance", regime)
    full = run(engine, "distance", xyz, table)
    worst = ratio(np.abs(full.astype(R.LD) - d), R.bound_distance(d))
    print(f"distance {regime}: |err| / (2 K_d u d) = {worst:.3f}")
    assert worst <= 1.0
    for P in R.COUNTS[:-1]:
        np.testing.assert_array_equal(bits(run(engine, "distance", xyz, table[:P])), bits(full[:, :P]))


@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_angles_conditioned_by_the_sine(engine, regime):
    xyz, table = R.inputs("angle", regime)
    theta, sin = R.exact("angle", regime)
    full = run(engine, "angle", xyz, table)
    worst = ratio(np.abs(full.astype(R.LD) - theta), R.bound_conditioned(sin, 2 * R.K_A))
    print(f"angle {regime}: |err| max(sin, sqrt u) / (2 K_a u) = {worst:.3f}; entries at sin < 0.01: {(sin < 0.01).mean():.3f}")
    assert worst <= 1.0
    assert full.min() >= 0.0 and full.max() <= R.PI32
    for T in R.COUNTS[:-1]:
        np.testing.assert_array_equal(bits(run(engine, "angle", xyz, table[:T])), bits(full[:, :T]))


@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_dihedrals_conditioned_by_the_smaller_sine_every_mode(engine, regime):
    xyz, table = R.inputs("dihedral", regime)
    t, s = R.exact("dihedral", regime)
    bound = R.bound_conditioned(s, 2 * R.K_T)
    full = run(engine, "dihedral", xyz, table)
    worst = ratio(R.wrap_diff(full, t), bound)
    print(f"dihedral {regime}: |err| max(s, sqrt u) / (2 K_t u) = {worst:.3f}; entries at s < 0.01: {(s < 0.01).mean():.3f}")
    assert worst <= 1.0
    assert full.min() > -R.PI32 and full.max() <= R.PI32
    cos_t, sin_t = np.cos(t), np.sin(t)
    for Q in R.COUNTS:
        rad = full[:, :Q] if Q == R.COUNTS[-1] else run(engine, "dihedral", xyz, table[:Q])
        np.testing.assert_array_equal(bits(rad), bits(full[:, :Q]))
        inter, block = run(engine, "dihedral", xyz, table[:Q], mode=1), run(engine, "dihedral", xyz, table[:Q], mode=2)
        assert inter.shape == block.shape == (xyz.shape[0], 2 * Q)
        np.testing.assert_array_equal(bits(inter[:, 0::2]), bits(block[:, :Q]))      # the same cos, the same sin
        np.testing.assert_array_equal(bits(inter[:, 1::2]), bits(block[:, Q:]))
        worst_c = ratio(np.abs(block[:, :Q].astype(R.LD) - cos_t[:, :Q]), bound[:, :Q] + 2 * U)
        worst_s = ratio(np.abs(block[:, Q:].astype(R.LD) - sin_t[:, :Q]), bound[:, :Q] + 2 * U)
        print(f"  Q = {Q}: cos {worst_c:.3f}, sin {worst_s:.3f} of the bound + 2 u")
        assert worst_c <= 1.0 and worst_s <= 1.0


@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_contacts_equal_the_exact_indicator_outside_the_margin(engine, regime):
    xyz, table = R.inputs("contact", regime)
    d = R.exact("contact", regime)
    away = np.abs(d - R.RCUT) > 2 * R.K_D * U * R.RCUT
    assert away.mean() >= 0.95
    full = run(engine, "contact", xyz, table)
    assert set(np.unique(full)) == {0.0, 1.0}
    np.testing.assert_array_equal(full[away], (d[away] <= R.RCUT).astype(np.float32))
    for P in R.COUNTS[:-1]:
        np.testing.assert_array_equal(bits(run(engine, "contact", xyz, table[:P])), bits(full[:, :P]))


# ---------------------------------------------------------------------------------------------- exact edges
def test_zero_length_bond_is_the_floor(engine):
    xyz = np.random.default_rng(1).normal(size=(5, 4, 3)).astype(np.float32) + np.float32(50)
    xyz[:, 1] = xyz[:, 0]
    out = run(engine, "distance", xyz, [[0, 1], [1, 0], [2, 3]])
    assert (bits(out[:, :2]) == bits(R.EPS_ROOT)).all()
    assert (out[:, 2] > 0.1).all()
    assert (run(engine, "contact", xyz, [[0, 1]], rcut=1e-5) == 1.0).all()


def test_collinear_triplets_clamp_and_never_nan(engine):
    xyz, par, c = R.collinear_triplets()
    got = run(engine, "angle", xyz, [[0, 1, 2]])[:, 0]
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= R.PI32
    over = par & (c >= 1)
    under = ~par & (c <= -1)
    assert (c[over] > 1).sum() > 10 and (c[under] < -1).sum() > 10          # the quotient does round beyond +-1
    assert (bits(got[over]) == 0).all()                                      # +0.0
    assert (bits(got[under]) == bits(R.PI32)).all()
    # where the fp32 cosine lands inside (-1, 1) the answer is acos of it: off 0 or pi by O(sqrt(u)), inside the bound
    exact = np.where(par, 0.0, R.PI_LD)
    assert ratio(np.abs(got.astype(R.LD) - exact), R.bound_conditioned(0.0, 2 * R.K_A)) <= 1.0
    np.testing.assert_array_equal(bits(run(engine, "angle", xyz, [[2, 1, 0]])[:, 0]), bits(got))      # v1 and v2 swapped


def test_planar_and_collinear_dihedrals(engine):
    pl, trans, lifted = R.planar_dihedrals()
    q = [[0, 1, 2, 3]]
    rad = run(engine, "dihedral", pl, q)[:, 0]
    flat = trans & ~lifted
    assert (bits(rad[flat]) == bits(R.PI32)).all()                           # y = +0.0: +pi, bit for bit
    t, sn = R.exact_dihedral(pl, q)
    assert (rad[lifted] > -R.PI32).all() and (rad[lifted] <= R.PI32).all()   # y -> -0: still never -pi
    assert ratio(R.wrap_diff(rad[lifted], t[lifted, 0]), R.bound_conditioned(sn[lifted, 0], 2 * R.K_T)) <= 1.0
    assert (rad[lifted] > 3.14).all()
    assert (rad[~trans] == 0.0).all()
    inter, block = run(engine, "dihedral", pl, q, mode=1), run(engine, "dihedral", pl, q, mode=2)
    np.testing.assert_array_equal(bits(inter), bits(block))                  # Q = 1: the two layouts coincide
    assert (bits(inter[~trans, 0]) == bits(np.float32(1))).all() and (inter[~trans, 1] == 0.0).all()
    assert (np.abs(inter[trans, 0] + 1.0) <= TRIG).all() and (np.abs(inter[trans, 1]) <= TRIG).all()
    line = R.collinear_quads()                                               # the extractor's mask: exactly 0, (1, 0)
    assert (bits(run(engine, "dihedral", line, q)) == 0).all()
    for mode in (1, 2):
        cs = run(engine, "dihedral", line, q, mode=mode)
        assert (bits(cs[:, 0]) == bits(np.float32(1))).all() and (bits(cs[:, 1]) == 0).all()


def test_contact_at_the_threshold(engine):
    two = np.float32([[[0, 0, 0], [0.375, 0.5, 0]], [[7, 7, 7], [7.375, 7.5, 7]], [[0.375, 0.5, 0], [0, 0, 0]]])
    assert (bits(run(engine, "distance", two, [[0, 1]])) == bits(np.float32(0.625))).all()
    below = np.nextafter(np.float32(0.625), np.float32(0))
    assert (run(engine, "contact", two, [[0, 1], [1, 0]], rcut=0.625) == 1.0).all()
    assert (run(engine, "contact", two, [[0, 1], [1, 0]], rcut=float(below)) == 0.0).all()
    assert (run(engine, "contact", two, [[0, 1]], rcut=float(np.nextafter(np.float32(0.625), np.float32(1)))) == 1.0).all()


# ---------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("kind,mode,m", [("distance", 0, 7), ("angle", 0, 7), ("contact", 0, 7), ("dihedral", 0, 7),
                                         ("dihedral", 1, 1), ("dihedral", 1, 65), ("dihedral", 2, 1), ("dihedral", 2, 65),
                                         ("rg", 0, 0)])
def test_strided_call_equals_packed_and_leaves_the_padding(engine, kind, mode, m):
    xyz = R.inputs("dihedral", "o1")[0][:301]
    table = None if kind == "rg" else R.records(kind, 65)[:m]
    packed = run(engine, kind, xyz, table, mode)
    wide = run(engine, kind, xyz, table, mode, pad=3, col_off=2)
    w = packed.shape[1]
    assert wide.shape == (301, w + 3) and not (bits(packed) == FILL).any()
    np.testing.assert_array_equal(bits(wide[:, 2:2 + w]), bits(packed))
    assert (bits(wide[:, :2]) == FILL).all() and (bits(wide[:, 2 + w:]) == FILL).all()
    if kind == "dihedral" and mode:                                           # interleaved against blocked
        rad = run(engine, kind, xyz, table, 0)
        cos, sin = (packed[:, 0::2], packed[:, 1::2]) if mode == 1 else (packed[:, :m], packed[:, m:])
        other = run(engine, kind, xyz, table, 3 - mode)
        ocos, osin = (other[:, 0::2], other[:, 1::2]) if mode == 2 else (other[:, :m], other[:, m:])
        np.testing.assert_array_equal(bits(cos), bits(ocos))
        np.testing.assert_array_equal(bits(sin), bits(osin))
        # fp32 cos / sin of the device's own fp32 angle
        assert np.abs(cos - np.cos(rad.astype(np.float64))).max() <= TRIG
        assert np.abs(sin - np.sin(rad.astype(np.float64))).max() <= TRIG


def test_empty_calls_write_nothing(engine):
    xyz = R.inputs("distance", "o1")[0][:9]
    xd = engine.to_device(xyz)
    for kind in KINDS:
        td = engine.to_device(R.records(kind, 7))
        for n, m in ((0, 7), (9, 0), (0, 0)):
            for mode in ((0, 1, 2) if kind == "dihedral" else (0,)):
                od = engine.to_device(np.full((9, 20), FILL, np.uint32).view(np.float32))
                st, msg = launch(engine, kind, xd, n, 12, td, m, od, 20, 2, mode)
                assert st == _lib.MSM_OK, (kind, n, m, msg)
                assert (bits(od.to_host()) == FILL).all()
        assert launch(engine, kind, None, 0, 12, None, 0, None, 0, 0)[0] == _lib.MSM_OK      # nothing to touch: no pointer needed
    od = engine.to_device(np.full((9, 3), FILL, np.uint32).view(np.float32))
    assert launch(engine, "rg", xd, 0, 12, None, 0, od, 3, 1)[0] == _lib.MSM_OK
    assert (bits(od.to_host()) == FILL).all()


def test_refusals(engine):
    xyz = R.inputs("distance", "o1")[0][:9]
    xd = engine.to_device(xyz)
    od = engine.to_device(np.full((9, 40), FILL, np.uint32).view(np.float32))
    for kind in KINDS:
        td = engine.to_device(R.records(kind, 7))
        for mode in ((0, 1, 2) if kind == "dihedral" else (0,)):
            w = width_of(kind, 7, mode)
            for kw, word in ((dict(ld=w + 1, col_off=2), "exceed"), (dict(ld=w - 1, col_off=0), "exceed"),
                             (dict(ld=40, col_off=-1), "exceed"), (dict(A=0, ld=40, col_off=0), "A >= 1"),
                             (dict(n=-1, ld=40, col_off=0), "n >= 0"), (dict(m=-1, ld=40, col_off=0), "count >= 0")):
                a = dict(n=9, A=12, m=7)
                a.update(kw)
                st, msg = launch(engine, kind, xd, a["n"], a["A"], td, a["m"], od, a["ld"], a["col_off"], mode)
                assert st == _lib.MSM_ERR_INVALID and word in msg, (kind, mode, kw, st, msg)
            st, msg = launch(engine, kind, None, 9, 12, td, 7, od, 40, 0, mode)
            assert st == _lib.MSM_ERR_INVALID and "NULL" in msg
    td = engine.to_device(R.records("dihedral", 7))
    for mode in (3, -1):
        st, msg = launch(engine, "dihedral", xd, 9, 12, td, 7, od, 40, 0, mode)
        assert st == _lib.MSM_ERR_INVALID and "mode" in msg
    td = engine.to_device(R.records("contact", 7))
    for rcut in (0.0, -1.0, float("nan")):
        st, msg = launch(engine, "contact", xd, 9, 12, td, 7, od, 40, 0, rcut=rcut)
        assert st == _lib.MSM_ERR_INVALID and "rcut" in msg, rcut
    for kw in (dict(A=0), dict(ld=1, col_off=1), dict(col_off=-1), dict(n=-1)):
        a = dict(n=9, A=12, ld=40, col_off=0)
        a.update(kw)
        st, msg = launch(engine, "rg", xd, a["n"], a["A"], None, 0, od, a["ld"], a["col_off"])
        assert st == _lib.MSM_ERR_INVALID and "msm_featurize_rg" in msg, kw
    assert (bits(od.to_host()) == FILL).all()                                  # no refused call wrote anything


# ---------------------------------------------------------------------------------------------- second grid-stride trip
@pytest.mark.parametrize("kind", ["distance", "angle", "dihedral", "contact"])
def test_second_grid_stride_trip(engine, kind):
    """The grid is capped at 16 n_cu workgroups of 256 threads: 4081 x 257 = 1,048,817 elements are one more than a
    first trip of 1,048,576 holds (n_cu = 256), so the last rows are written by threads on their second element."""
    n, m = R.N_TRIP, R.M_TRIP
    assert n * m > engine.info()["n_cu"] * 16 * 256
    src = "distance" if kind == "contact" else kind
    xyz, table = R.inputs(src, "off50", n, m)
    rows = np.array(R.trip_rows(n))
    assert {0, n - 2, n - 1} <= set(rows.tolist()) and len(rows) >= 200
    ex = R.exact(src, "off50", n, m, tuple(rows.tolist()))
    rcut = 2.2                                                                  # about the median pair distance of the bulk
    got = run(engine, kind, xyz, table, rcut=rcut)
    assert not (bits(got) == FILL).any()
    sub = got[rows].astype(R.LD)
    if kind == "distance":
        assert ratio(np.abs(sub - ex), R.bound_distance(ex)) <= 1.0
    elif kind == "angle":
        assert ratio(np.abs(sub - ex[0]), R.bound_conditioned(ex[1], 2 * R.K_A)) <= 1.0
    elif kind == "dihedral":
        assert ratio(R.wrap_diff(sub, ex[0]), R.bound_conditioned(ex[1], 2 * R.K_T)) <= 1.0
    else:
        away = np.abs(ex - rcut) > 2 * R.K_D * U * rcut
        assert away.mean() >= 0.95 and 0.2 < (ex <= rcut).mean() < 0.8
        np.testing.assert_array_equal(got[rows][away], (ex[away] <= rcut).astype(np.float32))
    # a frame's result does not depend on where the frame stands: the tail rows alone, in a grid of one trip
    tail = run(engine, kind, xyz[n - 3:], table, rcut=rcut)
    np.testing.assert_array_equal(bits(tail), bits(got[n - 3:]))
    if kind == "dihedral":
        for mode in (1, 2):
            trig = run(engine, kind, xyz, table, mode=mode)
            np.testing.assert_array_equal(bits(trig[n - 3:]), bits(run(engine, kind, xyz[n - 3:], table, mode=mode)))
            assert not (bits(trig) == FILL).any()


def test_rg_second_trip(engine):
    """One wave per frame, 4 waves per workgroup: 16,384 frames fill the capped grid once (n_cu = 256)."""
    n = 16_385 + 64
    assert n > engine.info()["n_cu"] * 16 * 4
    xyz = np.random.default_rng(12).normal(size=(n, 3, 3)).astype(np.float32) + np.float32(50)
    got = run(engine, "rg", xyz)[:, 0]
    ex = R.exact_rg(xyz)
    assert (np.abs(got.astype(R.LD) - ex) <= np.spacing(ex.astype(np.float32))).all()
    np.testing.assert_array_equal(bits(got[-70:]), bits(run(engine, "rg", xyz[-70:])[:, 0]))


# ---------------------------------------------------------------------------------------------- Rg
@pytest.mark.parametrize("A", [1, 2, 63, 64, 65, 130, 1000])
def test_rg_within_one_ulp_of_the_exact_value(engine, A):
    """fp64 accumulation of fp32 coordinates: A 2^-53 relative, far below 2^-24; one rounding to fp32 remains."""
    for offset in (0.0, 1000.0):
        xyz = R.rg_frames(A, offset)
        got = run(engine, "rg", xyz)[:, 0]
        ex = R.exact_rg(xyz)
        if A == 1:
            assert (bits(got) == 0).all()
        else:
            ulps = np.abs(got.astype(R.LD) - ex) / np.spacing(ex.astype(np.float32))
            print(f"rg A = {A} offset {offset}: {float(ulps.max()):.3f} ulp")
            assert ulps.max() <= 1.0 and got.min() > 0.0
        np.testing.assert_array_equal(bits(engine.featurize_rg(engine.to_device(xyz)).to_host()), bits(got))


# ---------------------------------------------------------------------------------------------- non-finite coordinates
@pytest.fixture(scope="module")
def nonfinite():
    bad, clean, mask = R.nonfinite_frames()
    tables = {kind: R.records(kind, 65) for kind in KINDS}
    return bad, clean, mask, tables


@pytest.mark.parametrize("kind,mode", [("distance", 0), ("angle", 0), ("contact", 0), ("dihedral", 0), ("dihedral", 1),
                                       ("dihedral", 2)])
def test_nonfinite_coordinates_follow_the_reference(engine, nonfinite, kind, mode):
    bad, clean, mask, tables = nonfinite
    table = tables[kind]
    got, ok = run(engine, kind, bad, table, mode), run(engine, kind, clean, table, mode)
    want = R.restate(kind, bad, table, mode)
    np.testing.assert_array_equal(R.classes(got), R.classes(want))
    reads = R.reads_bad(mask, table)
    nan_read = R.reads_bad(np.isnan(bad).any(axis=2), table)
    assert reads.sum() > 100 and nan_read.sum() > 50
    if mode == 1:
        reads, nan_read = np.repeat(reads, 2, axis=1), np.repeat(nan_read, 2, axis=1)
    elif mode == 2:
        reads, nan_read = np.hstack([reads, reads]), np.hstack([nan_read, nan_read])
    # every frame and record that reads no bad atom: the bits of the same call on the clean array
    np.testing.assert_array_equal(bits(got)[~reads], bits(ok)[~reads])
    assert np.isfinite(ok).all()
    if kind in ("distance", "angle"):
        assert np.isnan(got[nan_read]).all() and not np.isfinite(got[reads]).any()
    if kind == "distance":
        lone = reads & ~nan_read
        lone[[40, 177]] = False
        assert lone.sum() > 5 and (got[lone] == np.inf).all()                   # a lone inf: +inf, whatever its sign
        both = (table == 1).any(axis=1) & (table == 4).any(axis=1)
        assert both.any() and np.isnan(got[40, both]).all()                     # inf - inf
    if kind == "contact":
        assert (bits(got[reads]) == 0).all()                                    # "no contact", +0.0
    if kind == "dihedral":
        np.testing.assert_array_equal(bits(got[reads]), bits(want[reads]))      # the reference's 0; (1, 0) in modes 1, 2
        assert (np.unique(got[reads]) == ([0.0] if mode == 0 else [0.0, 1.0])).all()


def test_nonfinite_rg_is_nan_for_the_frame_only(engine, nonfinite):
    bad, clean, mask, _tables = nonfinite
    got, ok = run(engine, "rg", bad)[:, 0], run(engine, "rg", clean)[:, 0]
    frame = mask.any(axis=1)
    assert frame.sum() == 8 and np.isnan(got[frame]).all()
    np.testing.assert_array_equal(bits(got[~frame]), bits(ok[~frame]))
    np.testing.assert_array_equal(R.classes(got), R.classes(npport.rg(bad)))
    assert np.isfinite(ok).all()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_spec_kernel_matches_the_per_kind_kernels_on_nonfinite_input(engine, nonfinite, mode):
    """No box, flags off: msm_featurize_spec goes through the same device functions, so classes agree everywhere and
    finite entries bit for bit (tests/test_gpu_pbc.py asserts the bit identity on finite data)."""
    bad, _clean, mask, tables = nonfinite
    per_kind = np.hstack([run(engine, "distance", bad, tables["distance"]), run(engine, "angle", bad, tables["angle"]),
                          run(engine, "dihedral", bad, tables["dihedral"], mode),
                          run(engine, "contact", bad, tables["contact"])])
    table = engine.feature_table(pairs=tables["distance"], triplets=tables["angle"], quads=tables["dihedral"],
                                 dihedral_mode=mode, contacts=tables["contact"], rcut=R.RCUT, periodic=False)
    assert table.width == per_kind.shape[1] and not table.any_mic
    xd = engine.to_device(bad)
    for mic in ("round", "search"):
        spec = engine.featurize_spec(xd, table, box=None, mic=mic).to_host()
        np.testing.assert_array_equal(R.classes(spec), R.classes(per_kind))
        fin = np.isfinite(per_kind)
        np.testing.assert_array_equal(bits(spec)[fin], bits(per_kind)[fin])
        assert (~fin).sum() > 200


def test_public_features_on_a_frame_with_missing_coordinates(engine, nonfinite):
    """distance_pair, distance and angle return 0.0 (their nan_to_num, S/features/builtins.py:127, 307, 346), contacts_pair
    0.0 (:271-272: NaN -> inf, then d <= rcut): the values the reference returns for the same frames."""
    from pmarlo_amd.features import get_feature
    from pmarlo_amd.io import Topology, Trajectory

    bad, clean, mask, _tables = nonfinite
    A = bad.shape[1]
    top = Topology([f"X{i}" for i in range(A)], ["UNK"] * A, np.zeros(A, dtype=int))
    tb, tc = Trajectory(bad, top), Trajectory(clean, top)
    for i, j, k in ((2, 5, 7), (1, 4, 0), (11, 3, 6), (8, 9, 2)):
        hit2, hit3 = mask[:, [i, j]].any(axis=1), mask[:, [i, j, k]].any(axis=1)
        assert hit2.any()
        with np.errstate(invalid="ignore", over="ignore"):
            ref_d = np.nan_to_num(R.restate("distance", bad, [[i, j]]).astype(float), nan=0.0, posinf=0.0, neginf=0.0)
            ref_a = np.nan_to_num(R.restate("angle", bad, [[i, j, k]]).astype(float), nan=0.0, posinf=0.0, neginf=0.0)
            ref_c = R.restate("contact", bad, [[i, j]], rcut=1.5).astype(float)
        assert (ref_d[hit2] == 0.0).all() and (ref_a[hit3] == 0.0).all() and (ref_c[hit2] == 0.0).all()
        for name, kw, hit, ref in (("distance_pair", dict(i=i, j=j), hit2, ref_d), ("distance", dict(indices=[i, j]), hit2, ref_d),
                                   ("angle", dict(indices=[i, j, k]), hit3, ref_a),
                                   ("contacts_pair", dict(i=i, j=j, rcut=1.5), hit2, ref_c)):
            got = get_feature(name).compute(tb, **kw)
            assert got.shape == (bad.shape[0], 1) and got.dtype == np.float64
            assert (got[hit] == 0.0).all() and not np.signbit(got[hit]).any(), name
            np.testing.assert_array_equal(got[hit], ref[hit])
            np.testing.assert_array_equal(got[~hit], get_feature(name).compute(tc, **kw)[~hit])
        assert 0 < get_feature("contacts_pair").compute(tb, i=i, j=j, rcut=1.5).sum() < bad.shape[0]


# ---------------------------------------------------------------------------------------------- determinism
def test_two_calls_give_equal_bytes(engine):
    for kind in KINDS:
        xyz, table = R.inputs("distance" if kind == "contact" else kind, "off50", R.N_TRIP, R.M_TRIP)
        for mode in ((0, 1, 2) if kind == "dihedral" else (0,)):
            a, b = run(engine, kind, xyz, table, mode), run(engine, kind, xyz, table, mode)
            assert a.tobytes() == b.tobytes(), (kind, mode)
    xyz = R.rg_frames(130, 1000.0, n=700)
    assert run(engine, "rg", xyz).tobytes() == run(engine, "rg", xyz).tobytes()
