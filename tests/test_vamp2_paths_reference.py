"""The cases of tests/_vamp2_paths_ref.py checked on the host: every condition the GPU tests of the VAMP-2 loss
kernels (tests/test_gpu_vamp2_paths.py) rely on is a property of the inputs and of the law, shown here without a
device.

  * ordinary cases have cond <= 64 on both regularised sides;
  * wherever a half of the penalty direction is present (cond_reg > 0, d > 2) the eigenvector it is built from is
    determined: eps l_max / (gap to the neighbouring eigenvalue) <= 1e-12.  The graded case is exempt and carries its
    own bound instead;
  * the law and the second route (longdouble moments, eigendecomposition instead of Cholesky, trace form of the score)
    agree within 1e-12 of the largest entry for loss, score, penalty, every metric and both gradients -- or, for the
    two cases that cannot, within twice the disagreement recorded beside their bound (100 x that disagreement);
  * branch cases take the branch they are named for: the ladder's final total, the trace clamp and the penalty halves
    present, by the law's own arithmetic and by the second route, against the table.

Prints cond, the sensitivity figure and the route disagreement per run."""

from __future__ import annotations

import numpy as np
import pytest

from tests import _vamp2_paths_ref as V

RUNS = [(name, weighted) for name in V.CASES for weighted in V.runs(name)]


def test_the_table_is_the_issue_s():
    at257 = {c["d"] for c in V.CASES.values() if c["m"] == 257 and c["group"] == "widths"}
    assert at257 == {1, 2, 15, 16, 17, 32, 33, 48, 49, 55, 56, 63, 64}
    for d in (1, 17, 64):
        rows = {c["m"] for c in V.CASES.values() if c["d"] == d and c["group"] in ("widths", "rows")}
        assert rows == {1, 2, 255, 256, 257, 512, 513, 770}, d
    for m in (257, 770):
        for d in (16, 56, 64):
            patterns = {c["weights"] for c in V.CASES.values() if (c["m"], c["d"], c["group"]) == (m, d, "weights")}
            assert patterns >= {"lognormal", "float32", "zeros", "first", "last"}
            assert ("chunk0" in patterns) == (m == 770)
    for kind in ("constant", "ladder", "nocond", "alpha1_"):
        assert {f"b_{kind}5", f"b_{kind}64"} <= set(V.CASES)
    assert V.CASES["b_graded64"]["d"] == 64
    for c in V.CASES.values():                  # a bound is the yardstick, or 100 x a recorded route disagreement
        assert c["bound"] == V.YARDSTICK if c["route"] is None else c["bound"] == pytest.approx(100.0 * c["route"])
        if c["m"] < c["d"] + 2 and c["inputs"] == "recipe":
            assert c["opts"]["cond_reg"] == 0.0
    w = V.inputs("p770x64_chunk0")[2]
    assert np.all(w[:V.CHUNK] == 0.0) and np.all(w[V.CHUNK:] > 0.0)
    assert np.sum(V.inputs("p770x16_zeros")[2] <= 0.0) > 770 // 3 and np.any(V.inputs("p770x16_zeros")[2] < 0.0)
    assert float(V.inputs("b_ladder64")[2].sum()) == 512.0


@pytest.mark.parametrize("name,weighted", RUNS)
def test_inputs_and_routes(name, weighted):
    c = V.CASES[name]
    law, two, sides = V.law(name, weighted), V.second(name, weighted), V.law_sides(name, weighted)
    cond = max(law["metrics"]["cond_C00"], law["metrics"]["cond_Ctt"])
    sens = max(V.sensitivity(s[3], s[2]) for s in sides)
    tag = f"{name} {'weighted' if weighted else 'plain'}"
    # the branches: the law's own arithmetic, the second route and the table agree
    for (total, clamped, halves, _, _), (total2, clamped2, halves2, _) in zip(sides, two["sides"]):
        assert total == pytest.approx(total2, rel=1e-6, abs=1e-15) and total2 in V.LADDER
        assert clamped == clamped2 and halves == halves2
        if c["expect"]:
            assert total2 == c["expect"]["total"] and clamped == c["expect"]["clamped"]
            assert halves == tuple(c["expect"]["halves"])
        else:
            assert total2 == 0.0 and not clamped
            assert halves == ((True, True) if c["opts"]["cond_reg"] > 0.0 and c["d"] > 1 else (False, False))
    if (c["expect"] or {}).get("zero"):
        print(f"{tag}: cond {cond:.1f}, covariances vanish: loss {law['loss']:.1e}, second route {two['loss']:.1e}")
        V.assert_zero_case(law, law["metrics"])
        V.assert_zero_case(two, law["metrics"])
        return
    dist = V.distances(two, law, c["compare"])
    worst = max(dist, key=dist.get)
    print(f"{tag}: cond {cond:.3e}, eps l_max / gap {sens:.1e}, route disagreement {dist[worst]:.1e} ({worst})")
    assert np.isfinite(law["loss"]) and law["score"] > 0.0
    if V.ordinary(name):
        assert cond <= V.COND_ORDINARY
    if c["route"] is None:
        assert sens <= V.SENSITIVITY
        assert dist[worst] <= V.ROUTE
    else:       # its own bound: the disagreement is the recorded one (a factor 2 for another LAPACK build)
        assert dist[worst] <= 2.0 * c["route"]
        scaled = max(s[4] for s in sides)
        print(f"    cond of the factorised matrices scaled to a unit diagonal: {scaled:.1f}")
        assert scaled <= V.COND_SCALED
    if c["compare"] == "all" and c["opts"]["alpha"] < 1.0 and c["m"] > 2:      # two pairs: a constant score
        assert np.max(np.abs(law["grad0"])) > 1e-6 * law["term_scale"]         # a gradient, not noise


def test_branch_figures():
    """What the branch cases are expected to show, on the law."""
    for d in V.BRANCH_WIDTHS:
        for weighted in (False, True):
            ladder = V.law(f"b_ladder{d}", weighted)
            assert ladder["metrics"]["eig_C00_min"] == V.FLOOR and ladder["metrics"]["eig_Ctt_min"] == V.FLOOR
            assert np.isfinite(ladder["loss"]) and ladder["penalty"] > 0.0
            nocond = V.law(f"b_nocond{d}", weighted)
            assert nocond["penalty"] == 0.0 and nocond["loss"] == -nocond["score"]
            alpha1 = V.law(f"b_alpha1_{d}", weighted)
            assert alpha1["metrics"]["cond_C00"] == 1.0 and alpha1["penalty"] == 0.0
    graded = V.law("b_graded64", False)
    assert max(graded["metrics"]["cond_C00"], graded["metrics"]["cond_Ctt"]) > 1e8


def test_the_cases_reach_every_path_on_paper():
    """V.assert_every_path at the chunk size written in the table; the GPU test repeats it with the library's."""
    V.assert_every_path(V.CHUNK)
