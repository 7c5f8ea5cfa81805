"""The exact references and the restated launch-path rule behind tests/test_gpu_spectrum_paths.py (CPU only): the
references agree with a general dense eigensolve, the generators make the spectra they promise, and the shape table
reaches every branch of msm_spectrum and both sides of each of its thresholds."""

from __future__ import annotations

import numpy as np
import scipy.linalg

from tests import _spectrum_ref as sr

PATHS = [c["path"] for c in sr.CASES]


def test_rule_thresholds_match_the_documented_edges():
    # p = 10: the last persistent single matrix is k = 557; the loop keeps W in LDS up to k = 1228
    assert sr.spectrum_path(557, 10, 1, 4)["persistent"] and not sr.spectrum_path(558, 10, 1, 4)["persistent"]
    assert sr.spectrum_path(1228, 10, 1, 4)["lds_w"] and not sr.spectrum_path(1229, 10, 1, 4)["lds_w"]
    assert sr.spectrum_path(384, 32, 1, 4)["lds_w"] and not sr.spectrum_path(385, 32, 1, 4)["lds_w"]
    assert sr.spectrum_path(544, 12, 1, 6)["G"] == 32 and sr.spectrum_path(545, 12, 1, 6)["G"] == 33
    assert sr.engine_p(500, 10) == (17, 11) and sr.engine_p(500, 3) == (10, 4) and sr.engine_p(5, 3) == (5, 4)
    assert not sr.spectrum_path(500, 16, 1, 10)["side_by_side"] and sr.spectrum_path(500, 16, 1, 9)["side_by_side"]


def test_shape_table_reaches_every_branch_and_edge():
    pers = [c for c in sr.CASES if c["path"]["persistent"]]
    loop = [c for c in sr.CASES if not c["path"]["persistent"]]
    # persistent: G = 1 and G = 32, several groups on one XCD, a ragged batch; G = 33 is the first loop
    assert {1, 32} <= {c["path"]["G"] for c in pers}
    assert any(c["path"]["per_xcd"] > 1 and c["batch"] > sr.XCDS for c in pers)
    assert any(c["path"]["G"] == 33 and c["batch"] == 1 for c in loop)
    assert any(c["orders"] for c in pers) and any(c["orders"] for c in loop)
    # batch == 8 * per_xcd (persistent) and one more (loop), for the same shape
    for c in pers:
        if c["batch"] == sr.XCDS * c["path"]["per_xcd"] and not c["orders"]:
            if any(d["k"] == c["k"] and d["p_eff"] == c["p_eff"] and d["batch"] == c["batch"] + 1 for d in loop):
                break
    else:
        raise AssertionError("no batch pair on both sides of 8 * per_xcd")
    # the loop with W in LDS for ONE matrix of 558 <= k <= 1228 (p = 10 range), and with W in global memory
    assert any(c["batch"] == 1 and c["path"]["lds_w"] and 558 <= c["k"] <= 1228 for c in loop)
    assert any(c["batch"] == 1 and not c["path"]["lds_w"] and c["k"] >= 1229 for c in loop)
    assert any(c["k"] == 2000 and not c["path"]["lds_w"] for c in loop)
    # w_bytes at 12 KB and one row more; at 96 KB and one row more (the last / first row of each side)
    wb = {(c["path"]["w_bytes"], c["p_eff"], c["path"]["persistent"]) for c in sr.CASES}
    assert any(w == sr.LDS_W_ATTR_BYTES and not ps for w, p, ps in wb)
    assert any(w == sr.LDS_W_ATTR_BYTES + 8 * p and not ps for w, p, ps in wb)
    assert any(w <= sr.LDS_W_BYTES < w + 8 * p and not ps for w, p, ps in wb)
    assert any(w - 8 * p <= sr.LDS_W_BYTES < w and not ps for w, p, ps in wb)
    # the subspace widths around each apply template, every template on both paths
    assert {8, 9, 16, 17, 24, 25, 32} <= {c["p_eff"] for c in sr.CASES}
    assert {8, 16, 24, 32} <= {c["path"]["apply"] for c in pers}
    assert {8, 16, 24, 32} <= {c["path"]["apply"] for c in loop}
    # the apply grid: 255 / 256 / 257 / 511 / 513 columns (one, one, two, two, three 256-column blocks)
    ks = {c["k"] for c in sr.CASES} | {n for c in sr.CASES if c["orders"] for n in c["orders"]}
    assert {255, 256, 257, 511, 513} <= ks
    # Ritz vectors side by side and one at a time, each checked for values somewhere
    assert {True, False} == {c["path"]["side_by_side"] for c in sr.CASES if c["n_vecs"]}
    assert {True, False} == {c["path"]["side_by_side"] for c in loop if c["n_vecs"]}
    # large k: p 10 and 32, n_its 3 and 10
    big = [c for c in sr.CASES if c["k"] >= 700]
    assert {10, 32} <= {c["p_eff"] for c in big} and {3, 10} <= {c["n_its"] for c in big}
    # ragged orders include p + 2, p (no iterations), 2 and 1
    for c in sr.CASES:
        if c["orders"]:
            assert {c["p_eff"] + 2, c["p_eff"], 2, 1} <= set(c["orders"]) and max(c["orders"]) == c["k"]
    # the generators of the table: repeated and large negative eigenvalues
    assert {"blocks", "bipartite", "identical"} == {c["gen"] for c in sr.CASES}


def _left_eig(T):
    w, vl = scipy.linalg.eig(T, left=True, right=False)
    order = np.argsort(-np.abs(w), kind="stable")
    return w[order], vl[:, order]


def test_reversible_reference_agrees_with_a_general_eigensolve():
    C = sr.block_counts(90, 4, 0.3, seed=3, chain=True, bipartite=(0,))
    T = sr.rownorm(C)
    ref = sr.reversible_reference(C, 4, lag=5.0, n_vecs=4)
    w, vl = _left_eig(T)
    assert np.max(np.abs(w.imag)) < 1e-12
    np.testing.assert_allclose(ref["ev"], w.real, atol=1e-13)
    np.testing.assert_allclose(ref["pi"] @ T, ref["pi"], atol=1e-15)
    np.testing.assert_allclose(ref["pi"].sum(), 1.0, rtol=1e-15)
    for q in range(4):
        x = ref["vecs"][q]
        np.testing.assert_allclose(x @ T, ref["ev"][q] * x, atol=1e-13)
        assert abs(abs(np.dot(x, sr.sign_fix(vl[:, q].real))) - 1.0) < 1e-12
        lead = int(np.argmax(np.abs(x)))
        assert x[lead] > 0 and abs(np.linalg.norm(x) - 1.0) < 1e-15
    # ITS: the convention of npport (top n+1 by magnitude, re-sorted by real part, first dropped, abs)
    top = w.real[:5]
    want = np.abs(np.sort(top)[::-1][1:])
    np.testing.assert_allclose(ref["its_eig"], want, rtol=1e-12)
    np.testing.assert_allclose(ref["its_ts"], -5.0 / np.log(want), rtol=1e-12)


def test_generators_make_the_spectra_they_promise():
    ev = sr.reversible_reference(sr.block_counts(120, 4, 0.006, seed=1, identical=True), 3)["ev"]
    np.testing.assert_allclose(ev[1:4], ev[1], rtol=0, atol=1e-14)        # exactly (3-fold) repeated
    assert ev[1] < 1 - 1e-3 and abs(ev[4]) < 0.5 * ev[1]
    c = next(c for c in sr.CASES if c["name"] == "persist_k257_p24_bipartite")
    ref = sr.reversible_reference(sr.case_counts(c, 257, 1), c["n_its"])
    top = ref["ev"][:c["n_its"] + 1]
    assert top.min() < -0.5                                              # a large negative eigenvalue among them
    assert not np.array_equal(np.abs(top[1:]), np.abs(np.sort(top)[::-1][1:]))   # magnitude order != real order
    np.testing.assert_array_equal(np.isnan(sr.reversible_reference(np.ones((2, 2)), 3)["its_eig"]), [False, True, True])
    assert np.all(np.isnan(sr.reversible_reference(np.ones((1, 1)), 2)["its_eig"]))


def test_debug_lines_are_checked_against_the_rule():
    ok = ("msm_spectrum: n=544 p=12 first cols=18\n"
          "msm_spectrum: persistent launch n=544 p=12 cols=17 G=32 groups=1 lds=1 -> no error\n")
    want = sr.spectrum_path(544, 12, 1, 6)
    ok = ok.replace("cols=17", f"cols={want['cols']}")
    assert sr.check_debug(ok, 1, 6)[0]["persist"]["G"] == 32
    for bad in (ok.replace("G=32", "G=31"), ok.splitlines()[0] + "\n",
                "msm_spectrum: n=545 p=12 first cols=17\n"
                "msm_spectrum: persistent launch n=545 p=12 cols=17 G=33 groups=1 lds=1 -> no error\n"):
        try:
            sr.check_debug(bad, 1, 6)
        except AssertionError:
            continue
        raise AssertionError(f"accepted: {bad!r}")
