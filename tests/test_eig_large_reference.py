"""The dispatch rule, the block schedule and the inputs behind tests/test_gpu_eig_large.py (CPU only): the restated
tournament visits every block pair once per sweep in disjoint rounds, the restated method converges on the cases it
is given, and numpy passes every case of the GPU file with a tenth of the tolerance to spare."""

from __future__ import annotations

import numpy as np
import pytest

from tests import _eig_large_ref as lr
from tests import _eig_ref as er
from tests.test_eig_reference import _host_tica


def test_dispatch_on_both_sides_of_both_limits():
    assert [lr.dispatch(n) for n in (0, 1, 256, 257, 2048, 2049)] == \
        ["invalid", "one_workgroup", "one_workgroup", "block_jacobi", "block_jacobi", "unsupported"]
    assert er.MAX_ORDER == lr.SMALL_MAX      # the old rule still describes everything below the switch
    assert lr.layout(257) == {"nb": 9, "npad": 288, "pairs": 5, "rounds": 9, "launches_per_sweep": 29,
                              "pivot_lds_bytes": 99840}
    assert lr.layout(288)["nb"] == 9 and lr.layout(289)["nb"] == 10 and lr.layout(289)["rounds"] == 9
    assert lr.layout(512)["pairs"] == 8 and lr.layout(2048)["launches_per_sweep"] == 2 + 3 * 63
    # the pivot kernel's matrices sit next to its JacobiShared inside a workgroup's LDS
    assert lr.layout(2048)["pivot_lds_bytes"] + er.STATIC_LDS_JACOBI <= er.LDS_PER_WORKGROUP
    # order 64, stride 65: the pivot problems take the pipelined Jacobi
    assert er.jacobi_variant(lr.PIVOT, lr.PIVOT + 1) == "pipelined"
    assert lr.scratch_bytes(2048, 5) < 200 * 2 ** 20


@pytest.mark.parametrize("n", [257, 288, 289, 320, 2048])
def test_schedule_visits_every_block_pair_once_in_disjoint_rounds(n):
    """Odd (257, 288: 9 blocks) and even (289, 320: 10; 2048: 64) block counts, ragged (257, 289) and exact last
    blocks."""
    L = lr.layout(n)
    nb = L["nb"]
    sched = lr.block_schedule(n)
    assert len(sched) == L["rounds"] == nb - 1 + (nb & 1)
    seen = set()
    for rnd in sched:
        assert len(rnd) == nb // 2                     # odd nb: one block sits out
        players = [b for pq in rnd for b in pq]
        assert len(set(players)) == len(players) and all(0 <= b < nb for b in players)
        for p, q in rnd:
            pair = (min(p, q), max(p, q))
            assert p != q and pair not in seen
            seen.add(pair)
    assert len(seen) == nb * (nb - 1) // 2
    if nb & 1:      # every block has exactly one bye per sweep
        byes = [({*range(nb)} - {b for pq in rnd for b in pq}).pop() for rnd in sched]
        assert sorted(byes) == list(range(nb))


@pytest.mark.parametrize("name", ["separated-257", "diagonal-300", "blockdiag-300", "identity-300"])
def test_restated_method_converges_and_keeps_padding_decoupled(name):
    """The numpy restatement through the shared checks: ragged last block (257 = 8 x 32 + 1, 300 = 9 x 32 + 12), a
    real eigenvalue 0 next to the zeros of the padding, rotations between blocks all skipped."""
    case = lr.separated_case(257) if name == "separated-257" else next(c for c in lr.n300_cases() if c["name"] == name)
    w, V, sweeps = lr.block_jacobi(case["A_in"])
    fig = er.check_eigh(w, V, case)
    assert sweeps < lr.SWEEP_CAP
    if name in ("diagonal-300", "identity-300"):
        assert sweeps == 0 and fig["err"] == 0.0
    if name == "blockdiag-300":
        assert sweeps == 1


def test_numpy_passes_the_eigh_checks_with_margin():
    cases = [lr.separated_case(n) for n in lr.SEPARATED_N] + list(lr.n300_cases())
    assert {c["name"].rsplit("-300", 1)[0] for c in lr.n300_cases()} == \
        {"triple", "cluster", "graded", "scaled", "lopsided", "zero", "identity", "diagonal", "blockdiag"}
    for case in cases:
        assert lr.dispatch(case["n"]) == "block_jacobi"
        w, v = np.linalg.eigh(case["A"])
        fig = er.check_eigh(w, v, case, margin=0.1 if case["tol"] > 0 else 1.0)
        assert 10 * fig["err"] <= case["tol"]
    lop = next(c for c in cases if c["name"] == "lopsided-300")
    assert not np.array_equal(lop["A_in"], lop["A_in"].T)
    blk = next(c for c in cases if c["name"] == "blockdiag-300")["A"]
    mask = np.kron(np.eye(10), np.ones((lr.B, lr.B)))[:300, :300] > 0
    assert not blk[~mask].any() and np.count_nonzero(blk[mask]) > 0.9 * mask.sum()


def test_cap_case_holds_its_bound_under_lapack():
    """n = 2048: LAPACK stays inside a tenth of n eps |w|_inf + the construction's rounding, which is itself far below
    the first term (three reflectors in float64)."""
    case = lr.cap_case()
    assert case["n"] == lr.MAX_ORDER and lr.dispatch(case["n"]) == "block_jacobi"
    assert 0 < case["construction"] < 0.05 * case["tol"]
    w, v = np.linalg.eigh(case["A"])
    fig = er.check_eigh(w, v, case, margin=0.1)
    print("cap case under LAPACK:", fig, "tol", case["tol"], "construction", case["construction"])


def test_numpy_passes_the_tica_checks_with_margin():
    cases = [lr.tica_full_case(F) for F in lr.FULL_F] + [lr.tica_deficient_case(F, r) for F, r in lr.DEFICIENT]
    cases += [c for k, c in lr.tica_300_cases().items() if k != "T-zero"]
    for case in cases:
        assert lr.dispatch(case["F"]) == "block_jacobi"
        fig = er.check_tica(_host_tica(case), case, margin=0.1)
        assert fig["err"] <= case["tol"] / 10
    c3 = lr.tica_300_cases()
    assert c3["cut"]["rank"] == 299 and c3["indefinite"]["rank"] == 299 and not c3["raw"]["kinetic_map"]
    assert c3["T-zero"]["zero"] and c3["T-zero"]["rank"] == 0
    assert [lr.tica_deficient_case(F, r)["rank"] for F, r in lr.DEFICIENT] == [200, 256]
    assert all(lr.tica_full_case(F)["scale"] is not None and lr.tica_full_case(F)["mu"].any() for F in lr.FULL_F)


def test_onesided_cases_are_finite():
    for F in lr.ONESIDED_F:
        case = er.onesided_case(F)
        er.check_onesided(case["want"].copy(), case)
        assert np.all(np.abs(case["want"]) < 1.0 + 1e-9)
