"""The path rule, the prescribed-spectrum inputs and the shared checks behind tests/test_gpu_eig_paths.py (CPU only):
the rule puts each order on the branch eig.hip's launchers pick, numpy passes every case of the GPU file with a tenth
of the tolerance to spare, and a deliberately wrong answer fails the checks."""

from __future__ import annotations

import numpy as np
import pytest

from tests import _eig_ref as er
from tests._host_engine import HostArray, HostEngine


# ---- the path rule ---------------------------------------------------------------------------------------------------
def test_tica_path_on_both_sides_of_every_boundary():
    assert [er.tica_path(F)["kernel"] for F in (1, 64, 65, 66, 69, 70, 97, 98, 256)] == \
        ["fused", "fused", "lds4", "lds2", "lds2", "lds2", "lds2", "global", "global"]
    assert er.tica_path(64)["ld"] == 65 and er.tica_path(65)["ld"] == 65 and er.tica_path(66)["ld"] == 67
    assert er.tica_path(64)["first"] == "ldl_registers" and er.tica_path(64)["tail"] == "lds"
    assert er.tica_path(65)["first"] == "cholesky_pair" and er.tica_path(65)["tail"] == "generic"
    # full rank: the tridiagonal solver runs on the fused orders only
    assert er.tica_path(64)["second"] == "tridiag" and er.tica_path(65)["second"] == "jacobi_generic"
    # rank 64 / 65 at F = 65 and F = 66: F = 65 with rank <= 64 is the one non-fused order that reaches it
    assert er.tica_path(65, 64)["second"] == "tridiag" and er.tica_path(65, 65)["second"] == "jacobi_generic"
    assert er.tica_path(66, 64)["second"] == "jacobi_pipelined" and er.tica_path(66, 65)["second"] == "jacobi_generic"
    assert er.tica_path(65, 1)["second"] == "tridiag" and er.tica_path(66, 1)["second"] == "jacobi_none"
    assert er.tica_path(66)["lds_mats"] == 2 and er.tica_path(69, 33)["lds_mats"] == 2   # no room next to TriShared
    assert er.tica_path(70, 64)["second"] == "jacobi_pipelined" and er.tica_path(70, 64)["lds_mats"] == 2
    # rank-deficient: the first eigensolve is Jacobi, pipelined for even orders 8..64
    assert er.tica_path(64, 60)["first"] == "jacobi_pipelined" and er.tica_path(63, 50)["first"] == "jacobi_generic"
    assert er.tica_path(8, 5)["first"] == "jacobi_pipelined" and er.tica_path(6, 5)["first"] == "jacobi_generic"
    assert er.tica_path(66, 64)["first"] == "jacobi_generic" and er.tica_path(9, 6)["first"] == "jacobi_generic"
    assert er.tica_path(64, 60)["second"] == "tridiag" and er.tica_path(64, 60)["second_fallback"] == "jacobi_pipelined"


def test_eigh_and_onesided_paths_on_both_sides_of_every_boundary():
    assert [er.eigh_path(n)["solver"] for n in (1, 64, 65, 94, 95, 256)] == \
        ["tridiag", "tridiag", "jacobi", "jacobi", "jacobi", "jacobi"]
    assert [er.eigh_path(n)["storage"] for n in (64, 65, 91, 92, 95, 256)] == ["lds", "lds", "lds", "global", "global",
                                                                                  "global"]
    assert er.eigh_path(8)["jacobi"] == "pipelined" and er.eigh_path(64)["jacobi"] == "pipelined"
    assert er.eigh_path(6)["jacobi"] == "generic" and er.eigh_path(33)["jacobi"] == "generic"
    assert er.eigh_path(66)["jacobi"] == "generic" and er.eigh_path(1)["jacobi"] == "none"
    assert [er.onesided_path(F)["storage"] for F in (64, 65, 66, 67, 256)] == ["lds", "lds", "global", "global", "global"]
    assert [er.onesided_path(F)["solver"] for F in (1, 64, 65, 67)] == ["tridiag", "tridiag", "jacobi", "jacobi"]


def test_case_tables_reach_every_branch():
    cs = er.all_tica_cases()
    full = [c for c in cs if c["rank"] == c["F"]]
    assert {"fused", "lds4", "lds2", "global"} == {c["path"]["kernel"] for c in full}
    assert {"ldl_registers", "cholesky_pair"} == {c["path"]["first"] for c in full}
    lack = [c for c in cs if 0 < c["rank"] < c["F"]]
    assert {"jacobi_pipelined", "jacobi_generic"} <= {c["path"]["first"] for c in lack}
    assert any(c["path"]["second"] == "tridiag" and not c["path"]["fused"] for c in lack)          # F = 65
    assert any(c["path"]["lds_mats"] == 2 for c in lack) and any(c["path"]["lds_mats"] == 0 for c in lack)
    assert any(not c["kinetic_map"] for c in cs) and any(c["scale"] is None for c in cs)
    assert any((c["lam"] < 0).any() for c in cs) and any(c["zero"] and c["T"] > 0 for c in cs)
    assert any(c["zero"] and not c["T"] > 0 for c in cs) and any(c["F"] == 1 for c in cs)
    for c in er.tica_clustered_cases():
        assert c["clustered"] and c["path"]["second"] == "tridiag"
    es = er.eigh_cases()
    assert {"tridiag", "jacobi"} == {c["path"]["solver"] for c in es}
    assert {"lds", "global"} == {c["path"]["storage"] for c in es}
    assert {91, 92, 94, 95, 255, 256} <= {c["n"] for c in es}
    assert {8, 64} <= {c["n"] for c in es if c["expect_sweeps"] == "positive" and c["path"]["jacobi"] == "pipelined"}
    assert {er.onesided_path(F)["storage"] for F in er.ONESIDED_F} == {"lds", "global"}


# ---- numpy through the shared checks, a tenth of the tolerance to spare ----------------------------------------------
def _host_tica(case):
    """tests/_host_engine.py's tica_solve (npport.tica_from_moments in the layout of the device outputs)."""
    F = case["F"]
    eng = HostEngine()
    mom = case["moments"].copy()
    mom[-1] = 0.5 if case["T"] > 0 else mom[-1]
    out = (HostArray(np.zeros(F)), HostArray(np.zeros((F, F))), HostArray(np.zeros(F)), HostArray(np.zeros(1, np.int32)))
    eng.tica_solve(HostArray(mom), F, scale=None if case["scale"] is None else HostArray(case["scale"]),
                   epsilon=case["epsilon"], kinetic_map=case["kinetic_map"], out=out)
    return out[0].a, out[1].a, out[2].a, int(out[3].a[0])


@pytest.mark.parametrize("group", ["full<=64", "full65..97", "full>=98", "deficient", "cut", "clustered", "indefinite"])
def test_numpy_passes_the_tica_checks_with_margin(group):
    sel = {"full<=64": [c for F in er.FULL_RANK_F if F <= 64 for c in er.tica_full_rank_cases(F)],
           "full65..97": [c for F in er.FULL_RANK_F if 64 < F < 98 for c in er.tica_full_rank_cases(F)],
           "full>=98": [c for F in er.FULL_RANK_F if F >= 98 for c in er.tica_full_rank_cases(F)],
           "deficient": er.tica_deficient_cases(), "cut": er.tica_cut_cases(), "clustered": er.tica_clustered_cases(),
           "indefinite": er.tica_indefinite_cases()}[group]
    for case in sel:
        fig = er.check_tica(_host_tica(case), case, margin=0.1)
        assert fig["err"] <= case["tol"] / 10


def test_zero_rank_contract_is_checked():
    for case in er.tica_zero_cases():
        F = case["F"]
        er.check_tica((np.zeros(F), np.zeros((F, F)), case["mu"] if case["T"] > 0 else np.zeros(F), 0), case)
        with pytest.raises(AssertionError):
            er.check_tica((np.zeros(F), np.zeros((F, F)), np.zeros(F), 1), case)
        W = np.zeros((F, F))
        W[0, 0] = 1e-300
        with pytest.raises(AssertionError):
            er.check_tica((np.zeros(F), W, np.zeros(F), 0), case)


def test_numpy_passes_the_eigh_checks_with_margin():
    for case in er.eigh_cases():
        w, v = np.linalg.eigh(case["A"])
        fig = er.check_eigh(w, v, case, margin=0.1 if case["tol"] > 0 else 1.0)
        assert fig["err"] == case["lapack_err"] and 10 * fig["err"] <= case["tol"]


def test_onesided_cases_are_finite_and_the_constant_column_is_clipped():
    for F in er.ONESIDED_F:
        case = er.onesided_case(F)
        er.check_onesided(case["want"].copy(), case)
        assert np.all(np.abs(case["want"]) < 1.0 + 1e-9)
    for F in (8, 70):
        case = er.onesided_case(F, 3)
        Xc = case["X"][case["idx"]] - case["X"][case["idx"]].mean(0)
        assert np.all(Xc[:, 3] == 0.0)            # exact zero row and column: the clipped eigenvalue
        assert np.sum(np.abs(case["want"]) < 1e-12) == 1
        with pytest.raises(AssertionError):
            er.check_onesided(case["want"] * (1 + 1e-7) + 1e-10, case)


# ---- a wrong answer fails ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [er.tica_full_rank_cases(16)[0], er.tica_full_rank_cases(16)[3],
                                  er.tica_deficient_cases()[2], er.tica_full_rank_cases(70)[2]],
                         ids=lambda c: c["name"])
def test_wrong_tica_answers_fail_the_checks(case):
    eig, W, mean, rank = _host_tica(case)
    er.check_tica((eig, W, mean, rank), case)
    swapped = W.copy()
    swapped[:, [1, 2]] = swapped[:, [2, 1]]
    with pytest.raises(AssertionError):
        er.check_tica((eig, swapped, mean, rank), case)
    flipped = W.copy()
    flipped[:, 1] *= -1.0
    with pytest.raises(AssertionError):
        er.check_tica((eig, flipped, mean, rank), case)
    off = eig.copy()
    off[1] += 10 * case["tol"]
    with pytest.raises(AssertionError):
        er.check_tica((off, W, mean, rank), case)
    for wrong in (rank - 1, rank + 1):
        with pytest.raises(AssertionError):
            er.check_tica((eig, W, mean, wrong), case)
    short_e, short_W = eig.copy(), W.copy()       # a consistent answer of one rank less
    short_e[rank - 1] = 0.0
    short_W[:, rank - 1] = 0.0
    with pytest.raises(AssertionError):
        er.check_tica((short_e, short_W, mean, rank - 1), case)
    if case["rank"] < case["F"]:
        dirty = W.copy()
        dirty[0, rank] = 1e-300
        with pytest.raises(AssertionError):
            er.check_tica((eig, dirty, mean, rank), case)
    with pytest.raises(AssertionError):
        er.check_tica((eig, W, mean + 1e-9, rank), case)


def test_wrong_eigh_answers_fail_the_checks():
    case = next(c for c in er.eigh_cases() if c["name"] == "separated-9")
    w, v = np.linalg.eigh(case["A"])
    er.check_eigh(w, v, case)
    bad = w.copy()
    bad[3] += 10 * case["tol"]
    with pytest.raises(AssertionError):
        er.check_eigh(bad, v, case)
    with pytest.raises(AssertionError):
        er.check_eigh(w, v[:, ::-1], case)
    with pytest.raises(AssertionError):
        er.check_eigh(w[::-1], v[:, ::-1], case)
    skew = v.copy()
    skew[:, 0] += 1e-9 * skew[:, 1]
    with pytest.raises(AssertionError):
        er.check_eigh(w, skew, case)

