"""TPTAnalysis, find_conformations and StateDetector.detect_from_timescale_gap on the device, against the public
pieces they are made of: markov_state_model.tpt (reactive_flux, pathway_decomposition), KineticImportanceScore,
pcca_memberships, RepresentativePicker, UncertaintyQuantifier.  Equalities are exact: the finder adds no arithmetic
of its own beyond the stated formulas, which the tests restate."""
import numpy as np
import pytest

from pmarlo_amd.conformations import (ConformationSet, KineticImportanceScore, RepresentativePicker, StateDetector,
                                      TPTAnalysis, find_conformations, tpt_analysis)
from pmarlo_amd.conformations.uncertainty import AVOGADRO_PER_MOL, BOLTZMANN_J_PER_K
from pmarlo_amd.markov_state_model import tpt
from pmarlo_amd.markov_state_model.pcca import pcca_memberships
from tests import _pathways_ref as R

pytestmark = pytest.mark.gpu


# ---- TPTAnalysis ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.TABLE[:2], ids=lambda c: f"n{c[0]}")
def test_analyze_equals_the_public_tpt_functions(engine, case):
    n, n_source, n_sink, fraction, mask, _ = case
    T, pi, source, sink, _, _ = R.chain_case(n, n_source, n_sink, 1, mask)
    res = TPTAnalysis(T, pi).analyze(np.array(source[::-1] + source), np.array(sink), n_paths=5, pathway_fraction=fraction)
    flux = tpt.reactive_flux(T, pi, source, sink)
    assert res.source_states.tolist() == source and res.sink_states.tolist() == sink
    assert np.array_equal(res.forward_committor, flux.forward_committor)
    assert np.array_equal(res.backward_committor, flux.backward_committor)
    assert np.array_equal(res.flux_matrix, flux.gross_flux) and np.array_equal(res.net_flux, flux.net_flux)
    assert (res.total_flux, res.rate, res.mfpt) == (flux.total_flux, flux.rate, flux.mfpt)
    paths, caps = tpt.pathway_decomposition(T, pi, source, sink, fraction=fraction, maxiter=10_000)
    assert len(paths) > 5
    assert res.pathways == paths[:5] and np.array_equal(res.pathway_fluxes, caps[:5])
    assert res.pathway_iterations == len(paths) and res.pathway_max_iterations == 10_000 and res.tpt_converged is True
    through = 0.5 * (flux.gross_flux.sum(axis=1) + flux.gross_flux.sum(axis=0))
    assert np.array_equal(res.bottleneck_states, np.argsort(through)[::-1][:10])


def test_analyze_reports_the_iteration_ceiling(engine, monkeypatch):
    T, pi, source, sink, _, _ = R.chain_case(12, 1, 1, 1, None)
    monkeypatch.setattr(tpt_analysis, "PATHWAY_MAX_ITERATIONS", 4)
    res = TPTAnalysis(T, pi).analyze(np.array(source), np.array(sink), n_paths=9)
    paths, caps = tpt.pathway_decomposition(T, pi, source, sink, fraction=0.99, maxiter=4)
    assert res.tpt_converged is False and res.pathway_iterations == 4 == res.pathway_max_iterations
    assert res.pathways == paths and np.array_equal(res.pathway_fluxes, caps)


def test_thin_methods(engine):
    T, pi, source, sink, _, _ = R.chain_case(12, 1, 1, 1, None)
    a = TPTAnalysis(T, pi)
    flux = tpt.reactive_flux(T, pi, source, sink)
    assert np.array_equal(a.compute_committor(source, sink), flux.forward_committor)
    assert np.array_equal(a.compute_committor(source, sink, forward=False), flux.backward_committor)
    gross, net, total = a.compute_reactive_flux_direct(source, sink)
    assert np.array_equal(gross, flux.gross_flux) and np.array_equal(net, flux.net_flux) and total == flux.total_flux
    sets, cg = a.coarse_grain_flux(source, sink, [[0, 1, 2], [3, 4, 5, 6]])
    want_sets, want = tpt.coarse_grain_flux(T, pi, source, sink, [[0, 1, 2], [3, 4, 5, 6]])
    assert sets == want_sets and np.array_equal(cg.net_flux, want.net_flux)
    q = flux.forward_committor
    assert np.array_equal(a.identify_transition_state_ensemble(q, 0.2), np.where((q >= 0.3) & (q <= 0.7))[0])
    stats = a.pathway_statistics([[0, 3, 11]], np.array([0.5]))
    assert stats[0]["length"] == 3 and stats[0]["flux_fraction"] == 1.0 and stats[0]["states"] == [0, 3, 11]
    assert stats[0]["free_energies"] == [float(-np.log(pi[s])) for s in (0, 3, 11)] and a.pathway_statistics([], []) == []
    with pytest.raises(ValueError, match="must not overlap"):
        a.analyze(np.array([0, 1]), np.array([1, 2]))
    with pytest.raises(ValueError, match="must be square"):
        TPTAnalysis(np.ones((2, 3)), pi)


# ---- find_conformations on a three-well chain ----------------------------------------------------------------------
N_STATES, SOURCE, SINK = 30, [3, 4, 5], [24, 25]


@pytest.fixture(scope="module")
def three_wells():
    """Metropolis chain on a line of 30 states with wells at 4, 14.5 and 25 (barriers of 3 kT); four trajectories
    sampled on the host, each beginning with a sweep over all states so that every resample of them is connected."""
    x = np.arange(N_STATES)
    U = 1.5 * (1.0 - np.cos(2.0 * np.pi * (x - 4.0) / 10.5)) + 0.04 * np.abs(x - 14.0)
    T = np.zeros((N_STATES, N_STATES))
    for i in range(N_STATES):
        for j in (i - 1, i + 1):
            if 0 <= j < N_STATES:
                T[i, j] = 0.25 * min(1.0, np.exp(U[i] - U[j]))
        T[i, i] = 1.0 - T[i].sum()
    pi = np.exp(-U)
    pi /= pi.sum()
    rng = np.random.default_rng(5)
    cdf = np.cumsum(T, axis=1)
    sweep = np.concatenate([x, x[::-1]])
    dtrajs = []
    for start in (0, 9, 19, 29):
        walk = [start]
        for u in rng.random(1200):
            walk.append(min(int(np.searchsorted(cdf[walk[-1]], u, side="right")), N_STATES - 1))
        dtrajs.append(np.concatenate([sweep, np.arange(0, start + 1), walk]).astype(np.int64))
    n_frames = sum(len(d) for d in dtrajs)
    states = np.concatenate(dtrajs)
    features = np.stack([states + rng.normal(0.0, 0.3, n_frames), rng.normal(0.0, 1.0, n_frames)], axis=1)
    return {"T": T, "pi": pi, "dtrajs": dtrajs, "features": features}


@pytest.fixture(scope="module")
def pieces(engine, three_wells):
    """What the public pieces return on the chain, computed once."""
    T, pi = three_wells["T"], three_wells["pi"]
    flux = tpt.reactive_flux(T, pi, SOURCE, SINK)
    chi = pcca_memberships(T, 3, pi)
    order = np.lexsort((np.arange(3), -(pi @ chi)))
    return {"flux": flux, "kis": KineticImportanceScore(T, pi).compute(k_slow="auto"), "chi": chi[:, order],
            "through": 0.5 * (flux.gross_flux.sum(axis=1) + flux.gross_flux.sum(axis=0))}


@pytest.fixture(scope="module")
def found(engine, three_wells):
    return find_conformations(three_wells, source_states=np.array(SOURCE), sink_states=np.array(SINK), auto_detect=False,
                              n_metastable=3, tse_tolerance=0.2)


def test_every_field_equals_its_public_piece(three_wells, pieces, found):
    pi, q = three_wells["pi"], pieces["flux"].forward_committor
    kT = BOLTZMANN_J_PER_K * 300.0 * AVOGADRO_PER_MOL / 1000.0
    labels = np.argmax(pieces["chi"], axis=1)
    assert sorted(c.state_id for c in found.conformations) == list(range(N_STATES))
    assert np.array_equal(found.macrostate_labels, labels) and len(set(labels.tolist())) == 3
    for c in found.conformations:
        s = c.state_id
        assert c.population == float(pi[s]) and c.free_energy == -kT * np.log(float(pi[s]))
        assert c.committor == float(q[s]) and c.flux == float(pieces["through"][s])
        assert c.kis_score == float(pieces["kis"].kis_scores[s]) and c.macrostate_id == int(labels[s])
        if c.conformation_type == "metastable":
            assert c.metadata["role"] == ("source" if s in SOURCE else "sink")
            assert np.array_equal(c.metadata["macrostate_members"], pieces["chi"][s])
        else:
            assert c.metadata == {}
    # macrostate 0 is the most populated one
    weights = pi @ pieces["chi"]
    assert np.all(np.diff(weights) <= 0.0)
    assert np.array_equal(found.tpt_result.forward_committor, q) and found.tpt_result.pathway_iterations >= 1
    assert len(found.tpt_result.pathways) == min(5, found.tpt_result.pathway_iterations)
    assert found.tpt_result.pathways[0][0] in SOURCE and found.tpt_result.pathways[0][-1] in SINK
    assert np.array_equal(found.kis_result.kis_scores, pieces["kis"].kis_scores) and found.uncertainty_results == []
    assert found.metadata == {"n_conformations": N_STATES, "auto_detected": False, "temperature_K": 300.0,
                              "uncertainty_analysis": False, "n_metastable_states": 3,
                              "n_transition_state_ensemble": len(found.get_transition_state_ensemble())}


def test_types_partition_the_states(pieces, found):
    q = pieces["flux"].forward_committor
    ends = set(SOURCE) | set(SINK)
    assert [c.state_id for c in found.get_metastable_states()] == sorted(ends)
    tse = [s for s in range(N_STATES) if s not in ends and abs(float(q[s]) - 0.5) <= 0.2]
    assert [c.state_id for c in found.get_transition_state_ensemble()] == tse and len(tse) >= 1
    assert [c.state_id for c in found.get_transition_states()] == [s for s in range(N_STATES) if s not in ends | set(tse)]
    # metastable first, then the reactive states in state order
    assert [c.state_id for c in found.conformations[len(ends):]] == [s for s in range(N_STATES) if s not in ends]


def test_tse_boundary_is_inclusive(three_wells, pieces):
    q = pieces["flux"].forward_committor
    inner = [s for s in range(N_STATES) if s not in SOURCE + SINK]
    s = min(inner, key=lambda i: abs(float(q[i]) - 0.5))
    edge = abs(float(q[s]) - 0.5)
    assert 0.0 < edge < 0.5
    kw = dict(source_states=SOURCE, sink_states=SINK, auto_detect=False, compute_kis=False, find_metastable_states=False)
    data = {"T": three_wells["T"], "pi": three_wells["pi"]}
    at = find_conformations(data, tse_tolerance=edge, **kw)
    below = find_conformations(data, tse_tolerance=float(np.nextafter(edge, 0.0)), **kw)
    assert [c.state_id for c in at.get_transition_state_ensemble()] == [s]
    assert below.get_transition_state_ensemble() == [] and len(below.get_transition_states()) == len(inner)
    assert at.kis_result is None and at.get_metastable_states() == [] and at.conformations[0].kis_score is None
    assert at.conformations[0].frame_index is None            # no features, no dtrajs: no representatives


def test_argument_errors(three_wells):
    with pytest.raises(ValueError, match="must be provided when auto_detect=False"):
        find_conformations(three_wells, auto_detect=False)
    with pytest.raises(ValueError, match="must be provided when auto_detect=False"):
        find_conformations(three_wells, auto_detect=False, source_states=[1])
    with pytest.raises(ValueError, match="tse_tolerance"):
        find_conformations(three_wells, tse_tolerance=0.6)
    with pytest.raises(ValueError, match="cannot exceed"):
        find_conformations(three_wells, n_metastable=N_STATES + 1)
    bad = dict(three_wells, pi=np.full(N_STATES, 1.0 / N_STATES))
    with pytest.raises(RuntimeError, match="Failed to compute PCCA"):
        find_conformations(bad, source_states=SOURCE, sink_states=SINK, auto_detect=False)


def test_representatives(three_wells, found):
    want = {s: (g, t, l) for s, g, t, l in RepresentativePicker().pick_representatives(
        three_wells["features"], three_wells["dtrajs"], list(range(N_STATES)), n_reps=1)}
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in three_wells["dtrajs"]])])
    for c in found.conformations:
        assert (c.frame_index, c.trajectory_index, c.local_frame_index) == want[c.state_id]
        assert c.frame_index == offsets[c.trajectory_index] + c.local_frame_index
        assert three_wells["dtrajs"][c.trajectory_index][c.local_frame_index] == c.state_id and c.structure_path is None


def test_uncertainty_and_auto_detection(three_wells, pieces):
    data = dict(three_wells, its=np.array([400.0, 150.0, 6.0, 4.0]))
    res = find_conformations(data, uncertainty_analysis=True, n_bootstrap=6, n_metastable=3, k_slow=2, random_seed=3)
    assert [u.observable_name for u in res.uncertainty_results] == ["rate", "mfpt", "total_flux", "free_energies"]
    assert all(u.method == "bootstrap" and 1 <= u.n_samples <= 6 for u in res.uncertainty_results)
    assert res.uncertainty_results[3].mean.shape == (N_STATES,) and res.uncertainty_results[0].mean > 0.0
    assert res.kis_result.k_slow == 2 and 0.0 <= res.kis_result.stability_metric <= 1.0
    assert res.kis_result.bootstrap_std.shape == (N_STATES,)
    # the timescale gap picked the two most populated PCCA+ sets
    source, sink = StateDetector().detect_from_timescale_gap(data["T"], data["pi"], data["its"], n_states=3)
    assert res.tpt_result.source_states.tolist() == sorted(source.tolist())
    assert res.tpt_result.sink_states.tolist() == sorted(sink.tolist())
    assert res.metadata["auto_detected"] is True and res.metadata["uncertainty_analysis"] is True
    assert {c.state_id for c in res.get_metastable_states()} == set(source.tolist()) | set(sink.tolist())


def test_detect_from_timescale_gap(three_wells):
    T, pi = three_wells["T"], three_wells["pi"]
    source, sink = StateDetector().detect_from_timescale_gap(T, pi, np.array([400.0, 150.0, 6.0]), n_states=3)
    labels = np.argmax(pcca_memberships(T, 3), axis=1)
    pops = np.array([pi[labels == m].sum() for m in range(3)])
    first, second = np.argsort(pops)[::-1][:2]
    assert np.array_equal(source, np.where(labels == first)[0]) and np.array_equal(sink, np.where(labels == second)[0])
    assert pops[first] >= pops[second] >= pops[3 - first - second] and len(source) > 1 and len(sink) > 1
    # the wells: each set is a contiguous stretch of the line
    assert np.all(np.diff(source) == 1) and np.all(np.diff(sink) == 1)


def test_save_load_round_trip(found, tmp_path):
    path = tmp_path / "out" / "conformations.json"
    found.save(path)
    back = ConformationSet.load(path)
    assert back.to_json() == found.to_json()
    assert np.array_equal(back.tpt_result.net_flux, found.tpt_result.net_flux)
    assert back.tpt_result.pathways == found.tpt_result.pathways
    assert [c.to_dict() for c in back.conformations] == [c.to_dict() for c in found.conformations]
    assert np.array_equal(back.macrostate_labels, found.macrostate_labels) and back.metadata == found.metadata
