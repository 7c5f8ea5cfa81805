"""find_conformations: the entry point of the conformations package.

Mirrors pmarlo.conformations.finder (S/conformations/finder.py:33-680), same signature and step order: input checks,
PCCA+ macrostates, source / sink detection (StateDetector) or the given sets, TPTAnalysis.analyze, kinetic importance
scores (with their bootstrap stability when asked), classification of every microstate, representative frames,
optional structure files, bootstrap error bars, metadata.  Each step is a class of this package that already runs on
the device; this module holds the host logic between them.

Classification: the states of A and B are 'metastable' (metadata: role 'source' / 'sink' and the state's PCCA+
memberships); every other state is 'tse' when |q+ - 0.5| <= tse_tolerance and 'transition' otherwise.
free_energy = -kT ln pi in kJ/mol (inf for an empty state).

Parity: PCCA+ comes from markov_state_model.pcca.pcca_memberships where the reference calls deeptime's pcca; parity
with the reference's own memberships is unpinned as it is there."""

from __future__ import annotations

import logging
from numbers import Integral
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np

from ..markov_state_model.pcca import pcca_memberships
from .kinetic_importance import KineticImportanceScore
from .representative_picker import RepresentativePicker, TrajectoryFrameLocator
from .results import Conformation, ConformationSet, KISResult, TPTResult, UncertaintyResult
from .state_detection import StateDetector
from .tpt_analysis import TPTAnalysis
from .uncertainty import AVOGADRO_PER_MOL, BOLTZMANN_J_PER_K, UncertaintyQuantifier

__all__ = ["find_conformations"]

logger = logging.getLogger("pmarlo.conformations")


def _kT_kJ_per_mol(temperature_K: float) -> float:
    return BOLTZMANN_J_PER_K * temperature_K * AVOGADRO_PER_MOL / 1000.0


def _resolve_n_metastable(requested: Optional[int], n_states: int) -> int:
    resolved = 2 if requested is None else int(requested)
    if resolved < 2:
        raise ValueError("n_metastable must be at least 2")
    if resolved > n_states:
        raise ValueError(f"n_metastable ({resolved}) cannot exceed the number of MSM states ({n_states})")
    return resolved


def _require_probabilities(name: str, values: np.ndarray, atol: float) -> None:
    if not np.all(np.isfinite(values)):
        raise ValueError(f"{name} contains NaN or infinite values.")
    if np.any(values < -atol):
        raise ValueError(f"{name} contains negative probabilities. Minimum value: {float(np.min(values)):.3e}.")


def _require_unit_rows(what: str, row_sums: np.ndarray, atol: float, rtol: float) -> None:
    if not np.allclose(row_sums, 1.0, atol=atol, rtol=rtol):
        raise ValueError(f"{what} Maximum row-sum deviation from 1: {float(np.max(np.abs(row_sums - 1.0))):.3e}.")


def _compute_macrostate_memberships(T: np.ndarray, pi: np.ndarray, n_metastable: int, *, atol: float = 1e-8,
                                    rtol: float = 1e-7, stationary_atol: float = 1e-6) -> tuple[np.ndarray, np.ndarray]:
    """(memberships [n, n_metastable], labels [n]): PCCA+ memberships with the macrostates ordered by decreasing
    stationary weight pi @ memberships (equal weights keep the lower index first), and their argmax.  T must be a
    finite row-stochastic matrix and pi a finite distribution that it leaves stationary, within the tolerances."""
    T_arr = np.asarray(T, dtype=float)
    if T_arr.ndim != 2 or T_arr.shape[0] != T_arr.shape[1]:
        raise ValueError("Transition matrix must be square to compute macrostates.")
    n_states = T_arr.shape[0]
    if not isinstance(n_metastable, Integral):
        raise TypeError("n_metastable must be an integer.")
    n_metastable = int(n_metastable)
    if n_metastable < 1:
        raise ValueError("n_metastable must be at least 1.")
    if n_metastable > n_states:
        raise ValueError(f"Requested {n_metastable} macrostates, but only {n_states} microstates are available.")
    _require_probabilities("Transition matrix", T_arr, atol)
    _require_unit_rows("Transition matrix must be row-stochastic.", T_arr.sum(axis=1), atol, rtol)

    pi_vec = np.asarray(pi, dtype=float).reshape(-1)
    if pi_vec.shape[0] != n_states:
        raise ValueError("Stationary distribution size must match the transition matrix. "
                         f"Expected {n_states}, got {pi_vec.shape[0]}.")
    _require_probabilities("Stationary distribution", pi_vec, atol)
    pi_sum = float(pi_vec.sum())
    if not np.isclose(pi_sum, 1.0, atol=atol, rtol=rtol):
        raise ValueError(f"Stationary distribution must sum to 1. Observed sum: {pi_sum:.12g}.")
    moved = pi_vec @ T_arr
    if not np.allclose(moved, pi_vec, atol=stationary_atol, rtol=rtol):
        raise ValueError("Provided pi is not stationary for the transition matrix. "
                         f"Maximum absolute residual in pi @ T - pi: {float(np.max(np.abs(moved - pi_vec))):.3e}.")

    memberships = np.asarray(pcca_memberships(T_arr, n_metastable, pi_vec), dtype=float)
    if memberships.shape != (n_states, n_metastable):
        raise ValueError("PCCA+ returned memberships with unexpected shape. "
                         f"Expected {(n_states, n_metastable)}, got {memberships.shape}.")
    if not np.all(np.isfinite(memberships)):
        raise ValueError("PCCA+ returned NaN or infinite membership values.")
    if np.any(memberships < -atol):
        raise ValueError("PCCA+ returned negative membership probabilities. "
                         f"Minimum value: {float(np.min(memberships)):.3e}.")
    _require_unit_rows("PCCA+ memberships must sum to 1 for each microstate.", memberships.sum(axis=1), atol, rtol)

    order = np.lexsort((np.arange(n_metastable), -(pi_vec @ memberships)))
    memberships = memberships[:, order]
    return memberships, np.argmax(memberships, axis=1).astype(int)


def _calculate_state_flux(flux_matrix: np.ndarray) -> np.ndarray:
    """Reactive flux through every state: half of its inflow plus outflow."""
    return 0.5 * (np.sum(flux_matrix, axis=1) + np.sum(flux_matrix, axis=0))


def _conformation(kind: str, state_id: int, tpt_result: TPTResult, pi: np.ndarray, kT: float,
                  kis_result: Optional[KISResult], flux_by_state: np.ndarray, macrostate_labels: Optional[np.ndarray],
                  metadata: Optional[Dict[str, Any]] = None) -> Conformation:
    population = float(pi[state_id])
    macrostate_id = None
    if macrostate_labels is not None and state_id < macrostate_labels.shape[0]:
        macrostate_id = int(macrostate_labels[state_id])
    return Conformation(
        conformation_type=kind, state_id=int(state_id), population=population,
        free_energy=-kT * np.log(population) if population > 0 else np.inf,
        committor=float(tpt_result.forward_committor[state_id]),
        kis_score=float(kis_result.kis_scores[state_id]) if kis_result is not None else None,
        flux=float(flux_by_state[state_id]), macrostate_id=macrostate_id, metadata={} if metadata is None else metadata)


def _find_metastable_states(tpt_result: TPTResult, pi: np.ndarray, temperature_K: float, kis_result: Optional[KISResult],
                            flux_by_state: Optional[np.ndarray] = None, macrostate_labels: Optional[np.ndarray] = None,
                            macrostate_memberships: Optional[np.ndarray] = None) -> List[Conformation]:
    """The source and sink states, in ascending state order."""
    kT = _kT_kJ_per_mol(temperature_K)
    if flux_by_state is None:
        flux_by_state = _calculate_state_flux(tpt_result.flux_matrix)
    source_states = [int(s) for s in np.asarray(tpt_result.source_states)]
    sink_states = [int(s) for s in np.asarray(tpt_result.sink_states)]
    conformations = []
    for state_id in sorted(set(source_states + sink_states)):
        meta: Dict[str, Any] = {"role": "source" if state_id in source_states else "sink"}
        if macrostate_memberships is not None and state_id < macrostate_memberships.shape[0]:
            meta["macrostate_members"] = macrostate_memberships[state_id]
        conformations.append(_conformation("metastable", state_id, tpt_result, pi, kT, kis_result, flux_by_state,
                                           macrostate_labels, meta))
    return conformations


def _find_transition_states(tpt_result: TPTResult, pi: np.ndarray, temperature_K: float, kis_result: Optional[KISResult],
                            flux_by_state: Optional[np.ndarray] = None, macrostate_labels: Optional[np.ndarray] = None,
                            tse_tolerance: float = 0.05) -> List[Conformation]:
    """Every state outside source and sink: 'tse' within tse_tolerance of q+ = 0.5 (bound included), else
    'transition'."""
    kT = _kT_kJ_per_mol(temperature_K)
    ends = set(int(s) for s in np.asarray(tpt_result.source_states)) | set(int(s) for s in np.asarray(tpt_result.sink_states))
    if flux_by_state is None:
        flux_by_state = _calculate_state_flux(tpt_result.flux_matrix)
    conformations = []
    for state_id in range(len(pi)):
        if state_id in ends:
            continue
        is_tse = abs(float(tpt_result.forward_committor[state_id]) - 0.5) <= tse_tolerance
        conformations.append(_conformation("tse" if is_tse else "transition", state_id, tpt_result, pi, kT, kis_result,
                                           flux_by_state, macrostate_labels))
    return conformations


def _update_with_representatives(conformations: List[Conformation], representatives: List[Tuple[int, int, int, int]]) -> None:
    picked = {state_id: (frame, traj, local) for state_id, frame, traj, local in representatives}
    for conf in conformations:
        if conf.state_id in picked:
            conf.frame_index, conf.trajectory_index, conf.local_frame_index = picked[conf.state_id]


def _extract_structures(conformations: List[Conformation], trajectories: Any, output_dir: str, *,
                        topology_path: Optional[str] = None,
                        trajectory_locator: Optional[TrajectoryFrameLocator] = None) -> None:
    """One directory per conformation type, one PDB file per conformation that has a representative."""
    picker = RepresentativePicker()
    for conf_type in ("metastable", "transition", "tse"):
        of_type = [c for c in conformations if c.conformation_type == conf_type]
        representatives: List[Tuple[int, int, int, int]] = []
        for c in of_type:
            if c.frame_index is None:
                continue
            if c.trajectory_index is None or c.local_frame_index is None:
                raise ValueError(f"Representative selection missing trajectory or local frame index for state {c.state_id}")
            representatives.append((c.state_id, c.frame_index, c.trajectory_index, c.local_frame_index))
        if not representatives:
            continue
        saved = picker.extract_structures(representatives, trajectories, str(Path(output_dir) / conf_type),
                                          prefix=conf_type, topology_path=topology_path,
                                          trajectory_locator=trajectory_locator)
        for conf, path in zip(of_type, saved):
            conf.structure_path = path


def find_conformations(
    msm_data: Dict[str, Any],
    trajectories: Optional[Any] = None,
    source_states: Optional[np.ndarray] = None,
    sink_states: Optional[np.ndarray] = None,
    auto_detect: bool = True,
    auto_detect_method: str = "auto",
    find_transition_states: bool = True,
    find_metastable_states: bool = True,
    compute_kis: bool = True,
    uncertainty_analysis: bool = False,
    n_bootstrap: int = 100,
    representative_selection: str = "closest_to_centroid",
    output_dir: Optional[str] = None,
    save_structures: bool = False,
    tse_tolerance: float = 0.05,
    n_metastable: Optional[int] = None,
    temperature: float = 300.0,
    k_slow: Union[int, str] = "auto",
    n_paths: int = 5,
    lag: int = 1,
    random_seed: int = 42,
    topology_path: Optional[str] = None,
    trajectory_locator: Optional[TrajectoryFrameLocator] = None,
) -> ConformationSet:
    """Conformations of an MSM by transition path theory.

    msm_data holds 'T' and 'pi' (required), 'dtrajs' (needed for representatives and error bars), 'features'
    (needed for representatives), and optionally 'fes' and 'its' for the detection of source and sink.  With
    auto_detect=False the two sets must be given.  Returns the ConformationSet with one Conformation per state asked
    for (find_metastable_states, find_transition_states), the TPTResult, the KISResult (compute_kis), the bootstrap
    results of rate, mfpt, total flux and free energies (uncertainty_analysis with dtrajs) and the PCCA+ labels."""
    logger.info("Starting conformations finder with TPT analysis")
    if "T" not in msm_data or "pi" not in msm_data:
        raise ValueError("msm_data must contain 'T' (transition matrix) and 'pi' (stationary distribution)")
    if not (0.0 <= tse_tolerance <= 0.5):
        raise ValueError("tse_tolerance must be between 0 and 0.5 inclusive")
    T = np.asarray(msm_data["T"])
    pi = np.asarray(msm_data["pi"])
    dtrajs, features = msm_data.get("dtrajs"), msm_data.get("features")
    fes, its = msm_data.get("fes"), msm_data.get("its")
    n_metastable_resolved = _resolve_n_metastable(n_metastable, T.shape[0])

    macrostate_labels = macrostate_memberships = None
    if find_metastable_states or find_transition_states:
        try:
            macrostate_memberships, macrostate_labels = _compute_macrostate_memberships(T, pi, n_metastable_resolved)
        except Exception as exc:
            raise RuntimeError("Failed to compute PCCA+ macrostates required for conformations analysis") from exc

    # 1. source and sink
    if auto_detect:
        logger.info("Auto-detecting source and sink states")
        source_states, sink_states = StateDetector().auto_detect(T=T, pi=pi, fes=fes, its=its,
                                                                 n_states=n_metastable_resolved,
                                                                 method=auto_detect_method)
        logger.info(f"Detected {len(source_states)} source states and {len(sink_states)} sink states")
    elif source_states is None or sink_states is None:
        raise ValueError("source_states and sink_states must be provided when auto_detect=False")
    else:
        source_states, sink_states = np.asarray(source_states), np.asarray(sink_states)
        logger.info("Using provided source and sink states")

    # 2. transition path theory
    logger.info("Running Transition Path Theory analysis")
    tpt_result = TPTAnalysis(T, pi).analyze(source_states, sink_states, n_paths=n_paths)

    # 3. kinetic importance
    kis_result: Optional[KISResult] = None
    if compute_kis:
        logger.info("Computing Kinetic Importance Scores")
        kis_calc = KineticImportanceScore(T, pi)
        kis_result = kis_calc.compute(k_slow=k_slow, its=its)
        if uncertainty_analysis and dtrajs is not None:
            logger.info("Computing KIS stability")
            stability, boot_std = kis_calc.bootstrap_stability(dtrajs, n_boot=n_bootstrap // 2, top_n=10,
                                                               random_seed=random_seed, lag=lag)
            kis_result = KISResult(kis_scores=kis_result.kis_scores, k_slow=kis_result.k_slow,
                                   eigenvectors=kis_result.eigenvectors, eigenvalues=kis_result.eigenvalues,
                                   ranked_states=kis_result.ranked_states, stability_metric=stability,
                                   bootstrap_std=boot_std)

    # 4. classification
    conformations: List[Conformation] = []
    flux_by_state = _calculate_state_flux(tpt_result.flux_matrix)
    if find_metastable_states:
        logger.info("Classifying metastable states from source and sink sets")
        conformations.extend(_find_metastable_states(tpt_result, pi, temperature, kis_result, flux_by_state,
                                                     macrostate_labels, macrostate_memberships))
    if find_transition_states:
        logger.info(f"Classifying reactive (transition) states (tolerance={tse_tolerance})")
        conformations.extend(_find_transition_states(tpt_result, pi, temperature, kis_result, flux_by_state,
                                                     macrostate_labels, tse_tolerance=tse_tolerance))

    # 5. representative frames
    if features is not None and dtrajs is not None and len(conformations) > 0:
        logger.info(f"Selecting representatives using {representative_selection} method")
        representatives = RepresentativePicker().pick_representatives(
            features=features, dtrajs=dtrajs, state_ids=list(set(c.state_id for c in conformations)), n_reps=1,
            method=representative_selection)
        _update_with_representatives(conformations, representatives)

    # 6. structure files
    if save_structures and output_dir is not None:
        logger.info("Extracting representative structures")
        _extract_structures(conformations, trajectories, output_dir, topology_path=topology_path,
                            trajectory_locator=trajectory_locator)

    # 7. error bars
    uncertainty_results: List[UncertaintyResult] = []
    if uncertainty_analysis and dtrajs is not None:
        logger.info("Performing uncertainty quantification")
        quantifier = UncertaintyQuantifier(random_seed=random_seed)
        uncertainty_results.extend(quantifier.bootstrap_tpt(dtrajs, source_states, sink_states, n_boot=n_bootstrap,
                                                            lag=lag).values())
        uncertainty_results.append(quantifier.bootstrap_free_energies(dtrajs, T_K=temperature, n_boot=n_bootstrap))

    counts = {kind: sum(1 for c in conformations if c.conformation_type == kind)
              for kind in ("metastable", "transition", "tse")}
    result = ConformationSet(
        conformations=conformations, tpt_result=tpt_result, kis_result=kis_result,
        uncertainty_results=uncertainty_results, macrostate_labels=macrostate_labels,
        metadata={
            "n_conformations": len(conformations),
            "auto_detected": auto_detect,
            "temperature_K": temperature,
            "uncertainty_analysis": uncertainty_analysis,
            "n_metastable_states": n_metastable_resolved,
            "n_transition_state_ensemble": counts["tse"],
        })
    logger.info(f"Conformations finder complete: found {len(conformations)} conformations "
                f"({counts['metastable']} metastable, {counts['transition']} transition, "
                f"{counts['tse']} transition state ensemble)")
    return result
