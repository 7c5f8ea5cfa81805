"""Host side of the conformation finder: StateDetector's host-only methods and the result classes' to_dict layouts
against what the reference's own classes returned on the same inputs (tests/golden/conformations.npz / .json,
recorded by tests/golden/make_golden_conformations.py), the argument errors, and auto_detect's fallback order.
Nothing here touches the device."""
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from pmarlo_amd.conformations import (Conformation, ConformationSet, KISResult, StateDetector, TPTResult,
                                      UncertaintyResult, find_conformations)
from pmarlo_amd.conformations.finder import _calculate_state_flux, _compute_macrostate_memberships, _resolve_n_metastable

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def gold(golden):
    return golden("conformations.npz")


@pytest.fixture(scope="module")
def gold_json():
    return json.loads((GOLDEN / "conformations.json").read_text())


def assert_recorded(gold, key, call):
    if f"{key}/error" in gold.files:
        with pytest.raises(Exception) as e:
            call()
        assert type(e.value).__name__ == str(gold[f"{key}/error"])
        return
    source, sink = call()
    assert isinstance(source, np.ndarray) and isinstance(sink, np.ndarray)
    assert np.array_equal(source, gold[f"{key}/source"]) and np.array_equal(sink, gold[f"{key}/sink"])


# ---- detection on free-energy surfaces ------------------------------------------------------------------------
@pytest.mark.parametrize("n_basins", [2, 3])
@pytest.mark.parametrize("method", ["watershed", "local_minima", "threshold"])
@pytest.mark.parametrize("name", ["two_wells", "three_wells", "rugged", "flat"])
def test_detect_from_fes(gold, name, method, n_basins):
    key = f"{method}/{name}/{n_basins}"
    if name == "flat" and method == "local_minima":
        assert f"{key}/source" not in gold.files      # all points tie: nothing was recorded
        return
    fes = SimpleNamespace(F=gold[f"fes/{name}"])
    assert_recorded(gold, key, lambda: StateDetector().detect_from_fes(fes, n_basins=n_basins, method=method))


def test_detect_from_fes_errors():
    det = StateDetector()
    with pytest.raises(ValueError, match="'F' attribute"):
        det.detect_from_fes(object())
    with pytest.raises(ValueError, match="Unknown FES method"):
        det.detect_from_fes(SimpleNamespace(F=np.zeros((4, 4))), method="basin_hopping")
    with pytest.raises(ValueError, match="at least 2"):
        det.detect_from_fes(SimpleNamespace(F=np.zeros((4, 4))), n_basins=1)


# ---- the other host-only methods ----------------------------------------------------------------------------------
@pytest.mark.parametrize("top_n", [2, 3, 5])
def test_detect_from_populations(gold, top_n):
    assert_recorded(gold, f"population/{top_n}", lambda: StateDetector().detect_from_populations(gold["pi"], top_n=top_n))


def test_detect_from_populations_errors():
    with pytest.raises(ValueError, match="at least 2"):
        StateDetector().detect_from_populations(np.array([0.5, 0.5]), top_n=1)
    with pytest.raises(ValueError, match="At least two populated"):
        StateDetector().detect_from_populations(np.array([1.0]))
    source, sink = StateDetector().detect_from_populations(np.array([0.2, 0.5, 0.3]))
    assert source.tolist() == [1] and sink.tolist() == [2]


def test_classify_committor_states(gold):
    a, b, c = StateDetector().classify_committor_states(gold["committors"])
    assert np.array_equal(a, gold["classify/source"]) and np.array_equal(b, gold["classify/sink"])
    assert np.array_equal(c, gold["classify/transition"])
    assert 0 in a and 1 in b                      # the thresholds themselves belong to source and sink
    a, b, c = StateDetector((0.2, 0.6)).classify_committor_states([0.2, 0.21, 0.6, 0.59])
    assert (a.tolist(), b.tolist(), c.tolist()) == ([0], [2], [1, 3])
    with pytest.raises(ValueError, match="one-dimensional"):
        StateDetector().classify_committor_states(np.zeros((2, 2)))


@pytest.mark.parametrize("thresholds", [(0.5, 0.5), (0.6, 0.4), (-0.1, 0.9), (0.1, 1.1)])
def test_committor_thresholds_are_checked(thresholds):
    with pytest.raises(ValueError, match="committor_thresholds"):
        StateDetector(thresholds)


def test_explicit_specifications(gold):
    det = StateDetector()
    cv, dtrajs = gold["cv"], [gold["dtraj0"], gold["dtraj1"]]
    assert_recorded(gold, "cv_ranges/frames", lambda: det.from_cv_ranges(cv, "x", (-3.0, -0.8), (0.9, 3.0)))
    assert_recorded(gold, "cv_ranges/states", lambda: det.from_cv_ranges(cv, "x", (-3.0, -0.8), (0.9, 3.0), dtrajs=dtrajs))
    assert_recorded(gold, "cv_ranges/empty", lambda: det.from_cv_ranges(cv, "x", (50.0, 60.0), (0.9, 3.0)))
    assert_recorded(gold, "frame_indices", lambda: det.from_frame_indices([0, 3, 3, 30], [59, 12], dtrajs))
    assert_recorded(gold, "macrostate_labels/0_2", lambda: det.from_macrostate_labels(gold["labels"], 0, 2))
    assert_recorded(gold, "macrostate_labels/missing", lambda: det.from_macrostate_labels(gold["labels"], 0, 7))
    source, sink = det.from_state_indices([3, 1], (4,))
    assert source.tolist() == [3, 1] and sink.tolist() == [4] and source.dtype == sink.dtype == np.dtype(int)


def test_timescale_gap_argument_errors():
    det = StateDetector()
    T, pi = np.eye(3), np.full(3, 1.0 / 3.0)
    with pytest.raises(ValueError, match="two implied timescales"):
        det.detect_from_timescale_gap(T, pi, np.array([5.0]))
    with pytest.raises(ValueError, match="exceeds the number of microstates"):
        det.detect_from_timescale_gap(T, pi, np.array([5.0, 1.0]), n_states=4)
    with pytest.raises(ValueError, match="at least 2"):
        det.detect_from_timescale_gap(T, pi, np.array([5.0, 1.0]), n_states=1)


# ---- auto_detect ---------------------------------------------------------------------------------------------------
class Stubbed(StateDetector):
    """Records which methods auto_detect tries; each can be told to fail."""

    def __init__(self, fail=(), fes_states=(1, 2)):
        super().__init__()
        self.calls, self.fail, self.fes_states = [], set(fail), fes_states

    def _try(self, name, result):
        self.calls.append(name)
        if name in self.fail:
            raise RuntimeError(name)
        return result

    def detect_from_fes(self, fes, n_basins=None, method="watershed"):
        return self._try("fes", (np.array([self.fes_states[0]]), np.array([self.fes_states[1]])))

    def detect_from_timescale_gap(self, T, pi, its, n_states=None, gap_threshold=2.0):
        return self._try("timescale", (np.array([3]), np.array([4])))

    def detect_from_populations(self, pi, top_n=None):
        return self._try("population", (np.array([5]), np.array([6])))


def test_auto_detect_fallback_order():
    T, pi, fes, its = np.eye(8), np.full(8, 0.125), object(), np.array([9.0, 1.0])

    def auto(det, **kw):
        source, sink = det.auto_detect(T, pi, **kw)
        return det.calls, source.tolist(), sink.tolist()

    assert auto(Stubbed(), fes=fes, its=its) == (["fes"], [1], [2])
    assert auto(Stubbed(fail={"fes"}), fes=fes, its=its) == (["fes", "timescale"], [3], [4])
    assert auto(Stubbed(fail={"fes", "timescale"}), fes=fes, its=its) == (["fes", "timescale", "population"], [5], [6])
    assert auto(Stubbed(), its=its) == (["timescale"], [3], [4])
    assert auto(Stubbed(fail={"timescale"}), its=its) == (["timescale", "population"], [5], [6])
    assert auto(Stubbed()) == (["population"], [5], [6])
    # grid indices that are no MSM states fail the FES attempt as a whole; one out of two survives alone
    assert auto(Stubbed(fes_states=(1, 8)), fes=fes, its=its) == (["fes", "timescale"], [3], [4])
    det = Stubbed()
    det.detect_from_fes = lambda fes, n_basins=None: (np.array([1, 9]), np.array([2]))
    assert [s.tolist() for s in det.auto_detect(T, pi, fes=fes)] == [[1], [2]]
    # the population method's own error is not swallowed
    with pytest.raises(RuntimeError, match="population"):
        Stubbed(fail={"population"}).auto_detect(T, pi)


def test_auto_detect_named_methods():
    T, pi = np.eye(8), np.full(8, 0.125)
    det = Stubbed(fes_states=(1, 99))
    assert [s.tolist() for s in det.auto_detect(T, pi, fes=object(), method="fes")] == [[1], [99]]   # not validated
    assert [s.tolist() for s in Stubbed().auto_detect(T, pi, its=np.ones(2), method="timescale")] == [[3], [4]]
    assert [s.tolist() for s in Stubbed().auto_detect(T, pi, method="population")] == [[5], [6]]
    with pytest.raises(ValueError, match="FES data required"):
        Stubbed().auto_detect(T, pi, method="fes")
    with pytest.raises(ValueError, match="Implied timescales required"):
        Stubbed().auto_detect(T, pi, method="timescale")
    with pytest.raises(ValueError, match="Unknown detection method"):
        Stubbed().auto_detect(T, pi, method="pcca")
    with pytest.raises(ValueError, match="at least 2"):
        Stubbed().auto_detect(T, pi, n_states=1)
    with pytest.raises(RuntimeError, match="fes"):
        Stubbed(fail={"fes"}).auto_detect(T, pi, fes=object(), method="fes")


# ---- result classes ------------------------------------------------------------------------------------------------
def build_results(gold):
    tpt = TPTResult(
        source_states=np.array([0]), sink_states=np.array([3, 4]), forward_committor=gold["res/qp"],
        backward_committor=gold["res/qm"], flux_matrix=gold["res/gross"], net_flux=gold["res/net"], total_flux=0.125,
        rate=0.25, mfpt=4.0, pathways=[[0, 2, 4], [0, 1, 3]], pathway_fluxes=gold["res/path_fluxes"],
        bottleneck_states=np.array([2, 1, 0, 4, 3]), tpt_converged=False, pathway_iterations=17,
        pathway_max_iterations=10_000)
    kis = KISResult(kis_scores=gold["res/kis"], k_slow=2, eigenvectors=gold["res/evecs"],
                    eigenvalues=np.array([1.0, 0.9, 0.5]), ranked_states=np.argsort(gold["res/kis"])[::-1])
    unc = UncertaintyResult("rate", 0.25, 0.01, 0.23, 0.27, 40, "bootstrap")
    confs = [
        Conformation("metastable", 0, 0.5, 1.75, macrostate_id=0, frame_index=12, trajectory_index=1,
                     local_frame_index=2, committor=0.0, kis_score=0.125, flux=0.0625, structure_path="a/b.pdb",
                     metadata={"role": "source"}),
        Conformation("tse", np.int64(2), np.float64(0.125), np.float64(5.25), committor=np.float64(0.5)),
    ]
    full = ConformationSet(conformations=confs, tpt_result=tpt, kis_result=kis, uncertainty_results=[unc],
                           macrostate_labels=np.array([0, 0, 1, 1, 1]), metadata={"n_conformations": 2})
    return tpt, confs, full


def same_layout(mine, theirs):
    """Equal values AND equal key order at every level (the order is the file layout)."""
    assert json.dumps(mine) == json.dumps(theirs)


def test_to_dict_layouts(gold, gold_json):
    tpt, confs, full = build_results(gold)
    same_layout(tpt.to_dict(), gold_json["tpt"])
    same_layout(confs[0].to_dict(), gold_json["conformation"])
    same_layout(confs[1].to_dict(), gold_json["conformation_defaults"])
    same_layout(full.to_dict(), gold_json["set"])
    same_layout(ConformationSet().to_dict(), gold_json["set_empty"])
    assert full.to_json() == gold_json["set_json"]


def test_load_reads_a_file_the_reference_wrote(gold, gold_json, tmp_path):
    path = tmp_path / "nested" / "set.json"
    path.parent.mkdir()
    path.write_text(gold_json["set_json"])
    back = ConformationSet.load(path)
    same_layout(back.to_dict(), gold_json["set"])
    assert isinstance(back.tpt_result.net_flux, np.ndarray) and back.tpt_result.tpt_converged is False
    assert back.kis_result.bootstrap_std is None and back.uncertainty_results[0].mean == 0.25
    assert [c.conformation_type for c in back.conformations] == ["metastable", "tse"]
    again = tmp_path / "deeper" / "dir" / "again.json"
    back.save(again)                                   # save creates the directories
    assert again.read_text() == gold_json["set_json"]


def test_getters_and_metadata_arrays(gold):
    _, confs, full = build_results(gold)
    full.conformations.append(Conformation("transition", 1, 0.25, 3.5, metadata={"macrostate_members": np.array([0.25, 0.75]),
                                                                              "n": np.int64(3)}))
    assert full.get_metastable_states() == [confs[0]] and full.get_transition_state_ensemble() == [confs[1]]
    assert [c.state_id for c in full.get_transition_states()] == [1] and full.get_by_type("other") == []
    d = json.loads(full.to_json())                     # arrays in the metadata do not stop the serialisation
    assert d["conformations"][2]["metadata"] == {"macrostate_members": [0.25, 0.75], "n": 3}


# ---- the finder's host checks (all raise before the device is asked) ------------------------------------------------
def test_find_conformations_input_checks():
    T, pi = np.eye(3), np.full(3, 1.0 / 3.0)
    with pytest.raises(ValueError, match="must contain 'T'"):
        find_conformations({"T": T})
    for tol in (0.6, -0.01):
        with pytest.raises(ValueError, match="tse_tolerance"):
            find_conformations({"T": T, "pi": pi}, tse_tolerance=tol)
    with pytest.raises(ValueError, match=r"n_metastable \(4\) cannot exceed the number of MSM states \(3\)"):
        find_conformations({"T": T, "pi": pi}, n_metastable=4)
    with pytest.raises(ValueError, match="at least 2"):
        find_conformations({"T": T, "pi": pi}, n_metastable=1)
    assert _resolve_n_metastable(None, 5) == 2 and _resolve_n_metastable(5, 5) == 5


def test_macrostate_membership_checks():
    T = np.array([[0.9, 0.1], [0.2, 0.8]])
    pi = np.array([2.0 / 3.0, 1.0 / 3.0])
    cases = [
        (np.ones((2, 3)), pi, 2, ValueError, "must be square"),
        (T, pi, 2.0, TypeError, "must be an integer"),
        (T, pi, 0, ValueError, "at least 1"),
        (T, pi, 3, ValueError, "only 2 microstates"),
        (np.array([[np.nan, 1.0], [0.2, 0.8]]), pi, 2, ValueError, "Transition matrix contains NaN"),
        (np.array([[1.1, -0.1], [0.2, 0.8]]), pi, 2, ValueError, "negative probabilities"),
        (np.array([[0.9, 0.2], [0.2, 0.8]]), pi, 2, ValueError, "row-stochastic"),
        (T, np.array([0.5, 0.25, 0.25]), 2, ValueError, "size must match"),
        (T, np.array([np.inf, 0.0]), 2, ValueError, "Stationary distribution contains NaN"),
        (T, np.array([1.5, -0.5]), 2, ValueError, "negative probabilities"),
        (T, np.array([0.5, 0.25]), 2, ValueError, "must sum to 1"),
        (T, np.array([0.5, 0.5]), 2, ValueError, "not stationary"),
    ]
    for T_, pi_, m, exc, text in cases:
        with pytest.raises(exc, match=text):
            _compute_macrostate_memberships(T_, pi_, m)


def test_state_flux_formula():
    F = np.array([[0.0, 2.0, 1.0], [0.5, 0.0, 4.0], [0.0, 0.0, 0.0]])
    assert _calculate_state_flux(F).tolist() == [1.75, 3.25, 2.5]     # half of row sum plus column sum
