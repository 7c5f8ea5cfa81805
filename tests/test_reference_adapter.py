"""The adapter INTEGRATION.md section 1 describes, against the reference's own registry: the engine's feature objects are
registered on ``pmarlo.features`` ("last registration wins", S/features/base.py:24-33), looked up through the
reference's ``get_feature`` and its spec parser, and a ``compute`` call dispatched that way reaches the HIP engine (which,
without a GPU, must fail loudly rather than fall back).  What the reference's registry and parser do with the engine's
names and with typical specs is recorded in tests/golden/registry.json (tests/golden/make_golden.py, golden_registry)."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "registry.json"


@pytest.fixture(scope="module")
def ref():
    return json.loads(GOLDEN.read_text())


def _engine_objects():
    from pmarlo_amd.features import builtins as gpu
    return [gpu.PhiPsiFeature(), gpu.Chi1Feature(), gpu.DistanceFeature(), gpu.AngleFeature(), gpu.DihedralFeature(),
            gpu.RadiusOfGyrationFeature(), gpu.DistancePairFeature(), gpu.ContactsPairFeature(), gpu.SASAFeature(),
            gpu.HBondsCountFeature(), gpu.SecondaryStructureFractionFeature()]


def _reference_registry(ref, objs):
    """The reference's FEATURE_REGISTRY after registering `objs`, keyed as its register_feature keyed them."""
    reg = {ref["register_keys"][obj.name]: obj for obj in objs}
    assert len(reg) == len(objs)                     # no two engine objects land on one key
    return reg


@pytest.fixture()
def engine_registry():
    from pmarlo_amd.features import base

    saved = dict(base.FEATURE_REGISTRY)
    yield base
    base.FEATURE_REGISTRY.clear()
    base.FEATURE_REGISTRY.update(saved)


def test_engine_features_register_on_the_reference_registry(ref, engine_registry):
    objs = _engine_objects()
    assert sorted(obj.name for obj in objs) == sorted(ref["register_keys"])
    reg = _reference_registry(ref, objs)
    for obj in objs:
        assert reg[ref["lookup_keys"][obj.name]] is obj
        assert reg[ref["lookup_keys"][obj.name.upper()]] is obj     # the reference's lookup is case-insensitive
        assert callable(obj.compute) and isinstance(obj.is_periodic(), np.ndarray)   # the FeatureComputer protocol
    # the engine's own registry keys, looks up and replaces as the reference's does
    for obj in objs:
        engine_registry.register_feature(obj)
    for obj in objs:
        for spelling in (obj.name, obj.name.upper()):
            assert engine_registry.get_feature(spelling) is obj
            assert engine_registry.FEATURE_REGISTRY[ref["lookup_keys"][spelling]] is obj
    assert ref["last_registration_wins"] and ref["unknown_name_raises_key_error"]
    second = type(objs[5])()
    engine_registry.register_feature(second)
    assert engine_registry.get_feature("rg") is second
    with pytest.raises(KeyError):
        engine_registry.get_feature("not_a_feature")


def test_reference_spec_parser_resolves_to_engine_objects(ref):
    """`parse_feature_spec` of the reference names the registry keys the engine's objects carry, and the keyword
    arguments it produces are the ones those objects read."""
    from pmarlo_amd.features import builtins as gpu

    reg = _reference_registry(ref, _engine_objects())
    parsed = {spec: (name, kwargs) for spec, name, kwargs in ref["parse_feature_spec"]}
    for spec, want in [("phi_psi", "phi_psi"), ("Rg", "rg"), ("dist:AtomPair(3, 17)", "distance_pair"),
                       ("contacts:Pair(1, 2)", "contacts_pair")]:
        assert parsed[spec][0].lower() == want
    assert parsed["dist:AtomPair(3, 17)"][1] == {"i": 3, "j": 17}

    class _Traj:
        n_atoms = 20

    for spec, (name, kwargs) in parsed.items():
        obj = reg[ref["lookup_keys"][name]]
        assert obj.__class__.__module__ == "pmarlo_amd.features.builtins", spec
        if isinstance(obj, gpu._PairKwFeature):
            assert obj._pair(_Traj(), kwargs) == [kwargs["i"], kwargs["j"]], spec
        elif isinstance(obj, gpu._IndexedFeature):
            assert len(kwargs["indices"]) == obj.width, spec


def test_dispatch_through_the_reference_reaches_the_engine(ref, gpu_present):
    """No GPU here: a compute call routed through the reference's registry must end in the engine's loud failure
    (device / library missing), not in a CPU result."""
    if gpu_present:
        pytest.skip("a GPU is present: covered by tests/test_gpu_api.py")
    from pmarlo_amd import _lib

    fc = _reference_registry(ref, _engine_objects())[ref["lookup_keys"]["rg"]]      # Rg

    class _Traj:            # the two attributes the engine's features read from an mdtraj-like trajectory
        def __init__(self):
            self.xyz = np.zeros((4, 3, 3), np.float32)
            self.n_frames, self.n_atoms = 4, 3
            self.topology = None

    with pytest.raises((_lib.MsmError, RuntimeError, OSError)):
        fc.compute(_Traj())
