"""The OPES kernels on every launch path: what must be the same bits is the same bits.

  * replay in launches of one deposit each (max_steps = 1) and in one launch;
  * the journal form of the bias on one workgroup and on the default grid, with and without tile skipping;
  * replay from records and the same run deposited on line from its CVs with fixed_sigma (the on-line launch writes
    the records it made; replaying those must rebuild the same ledger);
  * the live form (one wave per frame, the MD step) run twice, and run on n frames at once and frame by frame.
The live form adds in another order than the journal form (lanes, then a shuffle tree; 1 / sigma by division), so the
two agree within a measured bound, not bit for bit: WAVE holds 4 x the largest difference observed on an MI355X over
the eight cases below (in the measures of tests/test_gpu_opes.py), as that file's BOUNDS do for the restatement.  Shapes: T = 300 deposits (more than two
LDS tiles), N in {1, 257, 1000}, d in {1, 2, 3, 8}, periodic and not."""

from __future__ import annotations

import numpy as np
import pytest

from pmarlo_amd import _lib
from pmarlo_amd.reweight import OPESLedger
from tests import _opes_ref as O
from tests.test_gpu_opes import device_ledger, grad_scale, relative_v

pytestmark = pytest.mark.gpu

CASES = [(d, periodic) for d in O.DIMS for periodic in (False, True)]
# live form against journal form; observed: V 1.974e-15 (kT p), gradient 1.110e-15 (of max(|dV/ds|, kT p / sigma0))
WAVE = {"bias": 7.9e-15, "grad": 4.5e-15}


def _buffers(led: OPESLedger) -> dict:
    dev, T = led.device_ledger(), len(led)
    s = led.state()
    out = {"state": dev["state"].to_host()[:7], "live": dev["live"].to_host()[:s["live"]],
           "slot_version": dev["slot_version"].to_host()[:s["live"]], "journal": dev["journal"].to_host()[:T],
           "death": dev["death"].to_host()[:T], "per_deposit": dev["per_deposit"].to_host()[:T]}
    assert s["status"] == 0 and s["count"] == T
    return out


def _same(a: dict, b: dict) -> None:
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


@pytest.mark.parametrize("d,periodic", CASES)
def test_bounded_launches_give_the_bits_of_one_launch(engine, d, periodic):
    x, par, rec, run = O.case(d, periodic)
    one = device_ledger(engine, par, rec)
    assert one.state()["cursor"] == O.T_DEPOSITS
    stepwise = device_ledger(engine, par, rec, max_steps=1)
    _same(_buffers(one), _buffers(stepwise))
    # 7 does not divide 300: the last launch is a short one; and a ledger that had to grow on the way
    sevens = device_ledger(engine, par, rec, max_steps=7)
    _same(_buffers(one), _buffers(sevens))
    grown = OPESLedger(d, par.kT, barrier=O.BARRIER, periods=par.periods, sigma0=par.sigma0, capacity=64, engine=engine)
    for lo in range(0, O.T_DEPOSITS, 100):
        sl = slice(lo, lo + 100)
        grown.deposit_records(np.arange(lo, lo + 100.0), rec[sl, :d], rec[sl, d:2 * d], rec[sl, 2 * d], rec[sl, 2 * d + 1])
    assert grown.capacity == 512
    _same(_buffers(one), _buffers(grown))


@pytest.mark.parametrize("n", [1, 257, 1000])
@pytest.mark.parametrize("d,periodic", CASES)
def test_grid_and_tile_skipping_do_not_change_a_bit(engine, d, periodic, n):
    x, par, rec, run = O.case(d, periodic)
    led = device_ledger(engine, par, rec)
    cv, times = O.frames(d, periodic, n)
    V, g = led.bias(cv, times, gradient=True)
    for kw in (dict(max_workgroups=1), dict(skip=False), dict(max_workgroups=2, skip=False)):
        V2, g2 = led.bias(cv, times, gradient=True, **kw)
        np.testing.assert_array_equal(V2, V, err_msg=str(kw))
        np.testing.assert_array_equal(g2, g, err_msg=str(kw))
    np.testing.assert_array_equal(led.bias(cv, times), V)                  # value only
    np.testing.assert_array_equal(led.bias(cv, counts=led.counts(times)), V)
    # the final bias, for which tile skipping drops every tile without a living version
    Vf, gf = led.bias(cv, gradient=True)
    Vn, gn = led.bias(cv, gradient=True, skip=False, max_workgroups=1)
    np.testing.assert_array_equal(Vn, Vf)
    np.testing.assert_array_equal(gn, gf)
    plan = engine.opes_plan(n, O.T_DEPOSITS, d)
    assert plan["frames_per_workgroup"] == _lib.METAD_THREADS and plan["versions_per_tile"] == _lib.METAD_TILE
    assert plan["grid"] == -(-n // _lib.METAD_THREADS) and plan["deposit_threads"] == 64 and plan["live_grid"] == n
    assert engine.opes_plan(n, O.T_DEPOSITS, d, max_workgroups=1)["grid"] == 1
    assert plan["lds_bytes"] == _lib.METAD_TILE * (2 * d + 1) * 8 + (_lib.METAD_TILE + 4 + 2) * 4


@pytest.mark.parametrize("d,periodic", CASES)
def test_online_deposits_replay_to_the_same_bits(engine, d, periodic):
    x, par, rec, run = O.case(d, periodic)
    online = OPESLedger(d, par.kT, barrier=O.BARRIER, periods=par.periods, sigma0=par.sigma0, fixed_sigma=True,
                        capacity=O.T_DEPOSITS, engine=engine)
    made = online.deposit(engine.to_device(x), np.arange(float(O.T_DEPOSITS))).to_host()
    np.testing.assert_array_equal(made[:, :d], x)
    np.testing.assert_array_equal(made[:, d:2 * d], np.broadcast_to(par.sigma0, (O.T_DEPOSITS, d)))
    np.testing.assert_allclose(made[:, 2 * d], np.exp(made[:, 2 * d + 1]), rtol=4 * O.EPS)      # h = exp(logweight)
    replayed = device_ledger(engine, par, made)
    _same(_buffers(online), _buffers(replayed))
    # one deposit per call, from host CVs: the same ledger again
    single = OPESLedger(d, par.kT, barrier=O.BARRIER, periods=par.periods, sigma0=par.sigma0, fixed_sigma=True,
                        capacity=16, engine=engine)
    for j in range(40):
        single.deposit(x[j])
    first = device_ledger(engine, par, made[:40])
    _same(_buffers(single), _buffers(first))
    np.testing.assert_array_equal(single.times, np.arange(40.0))


@pytest.mark.parametrize("d,periodic", CASES)
def test_the_wave_path(engine, d, periodic):
    x, par, rec, run = O.case(d, periodic)
    led = device_ledger(engine, par, rec)
    cv, _times = O.frames(d, periodic, 257)
    Vj, gj = led.bias(cv, gradient=True)                   # the journal form at the final state
    Vw, gw = led.bias(cv, gradient=True, live=True)
    again = led.bias(cv, gradient=True, live=True, max_workgroups=3)
    np.testing.assert_array_equal(again[0], Vw)
    np.testing.assert_array_equal(again[1], gw)
    for f in (0, 100, 256):                                # n = 1, the MD step: the batch's bits
        v1, g1 = led.bias(cv[f], gradient=True, live=True)
        assert v1[0] == Vw[f] and (g1[0] == gw[f]).all()
        assert led.bias(cv[f], live=True)[0] == Vw[f]
    err_v = relative_v(Vw, Vj, par).max()
    err_g = (np.abs(gw - gj) / grad_scale(gj, par)).max()
    print(f"d={d} periodic={periodic}: wave against journal form: V {err_v:.3e}, gradient {err_g:.3e}")
    assert err_v <= WAVE["bias"] and err_g <= WAVE["grad"]
