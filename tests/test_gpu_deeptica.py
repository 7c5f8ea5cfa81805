"""DeepTICA inference on the device: msm_mlp_forward and DeepTICAModel against the fp64 restatement and the
reference's recorded outputs.

Yardstick: `ref_dev`, the distance of the reference's own fp32 evaluation from the exact law, recorded per case in
tests/golden/deeptica.json.  The device evaluates in fp64, 2^29 times finer than fp32, so it must sit within
1e-3 ref_dev of the restatement (five orders of slack for another summation order and other erf / tanh / expm1
implementations, while an indexing, padding or layout mistake is of the order of the outputs and misses by six), and
within 1.5 ref_dev of the reference's outputs themselves."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

from tests import _deeptica_ref as R

from pmarlo_amd.features.deeptica import DeepTICAModel, MLPSpec

pytestmark = pytest.mark.gpu

WHITENED = [n for n, c in R.CASES.items() if c[-1] != "none"]


@pytest.fixture(scope="module")
def gold(golden):
    return golden("deeptica.npz"), json.loads((Path(__file__).parent / "golden" / "deeptica.json").read_text())


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name):
        if name not in cache:
            c = R.case(name)
            cache[name] = DeepTICAModel.from_arrays(c["config"], c["params"], c["mean"], c["std"], c["history"])
        return cache[name]

    return get


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _raw(engine, models, name, X=None):
    X = R.case(name)["X"] if X is None else X
    return engine.mlp_forward(engine.to_device(X), models(name).spec).to_host()


@pytest.mark.parametrize("name", list(R.CASES))
def test_raw_outputs(engine, models, gold, name):
    arrays, doc = gold
    c, dev = R.case(name), doc[name]["ref_dev"]["raw"]
    got = _raw(engine, models, name)
    assert got.shape == c["raw"].shape and got.dtype == np.float64
    err_law = float(np.max(np.abs(got - c["raw"])))
    err_ref = float(np.max(np.abs(got - arrays[f"raw__{name}"])))
    print(f"{name}: |device - restatement| = {err_law:.3e} = {err_law / dev:.2e} ref_dev; "
          f"|device - reference| = {err_ref / dev:.3f} ref_dev")
    assert err_law <= 1e-3 * dev
    assert err_ref <= 1.5 * dev


@pytest.mark.parametrize("name", list(R.CASES))
def test_transform_end_to_end(engine, models, gold, name):
    """Scaler, network and whitening with the metadata absent, present and inconsistent (the last leaves the raw
    outputs); the host entry is the device entry plus one copy."""
    arrays, doc = gold
    c, dev = R.case(name), doc[name]["ref_dev"]["final"]
    model = models(name)
    got = model.transform(c["X"])
    on_device = model.transform_device(engine.to_device(c["X"])).to_host()
    assert _same_bits(got, on_device)
    err_law = float(np.max(np.abs(got - c["final"])))
    err_ref = float(np.max(np.abs(got - arrays[f"final__{name}"])))
    print(f"{name}: final |device - restatement| = {err_law:.3e} = {err_law / dev:.2e} ref_dev; "
          f"|device - reference| = {err_ref / dev:.3f} ref_dev")
    assert err_law <= 1e-3 * dev
    assert err_ref <= 1.5 * dev
    if R.CASES[name][-1] == "bad":
        assert _same_bits(got, _raw(engine, models, name))
    elif R.CASES[name][-1] == "ok":
        assert np.max(np.abs(got - c["raw"])) > 1e-3        # the whitening did happen


@pytest.mark.parametrize("name", ["wide", "odd"])
def test_frames_are_independent_bit_for_bit(engine, models, name):
    c, spec = R.case(name), models(name).spec
    n, F = c["X"].shape
    assert n == 130
    xd = engine.to_device(c["X"])
    batch = engine.mlp_forward(xd, spec).to_host()
    assert _same_bits(batch, engine.mlp_forward(xd, spec).to_host())
    alone = engine.empty((n, spec.widths[-1]), np.float64)
    for t in range(n):
        engine.mlp_forward(xd.view((1, F), offset_elems=t * F), spec, out=alone.view((1, spec.widths[-1]),
                                                                                     offset_elems=t * spec.widths[-1]))
    assert _same_bits(batch, alone.to_host())
    # and in another place of another tile: the batch without its first 7 frames
    assert _same_bits(batch[7:], engine.mlp_forward(xd.view((n - 7, F), offset_elems=7 * F), spec).to_host())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_row_stride_wider_than_the_features(engine, models, dtype):
    """Columns from F on are NaN and must not be read; float32 and its exact float64 image give the same bits."""
    c, spec = R.case("flagship"), models("flagship").spec
    n, F = c["X"].shape
    assert c["X"].dtype == np.float32
    want = _raw(engine, models, "flagship")
    wide = np.full((n, F + 3), np.nan, dtype)
    wide[:, :F] = c["X"]
    got = engine.mlp_forward(engine.to_device(wide).view((n, F)), spec, ld=F + 3).to_host()
    assert _same_bits(got, want)


@pytest.mark.parametrize("name", ["odd", "default", "one", "flagship"])
def test_a_non_finite_frame_is_nan_and_disturbs_no_other(engine, models, name):
    c = R.case(name)
    clean = _raw(engine, models, name)
    n, F = c["X"].shape
    X = np.array(c["X"])
    bad = sorted({n // 3, n - 1, min(n - 1, 16)})
    for i, t in enumerate(bad):
        X[t, (5 * i) % F] = (np.nan, np.inf, -np.inf)[i % 3]
    got = _raw(engine, models, name, X)
    assert np.isnan(got[bad]).all()
    keep = np.setdiff1d(np.arange(n), bad)
    assert _same_bits(got[keep], clean[keep])


def test_width_257_is_refused_cleanly(engine, models):
    spec = MLPSpec((257, 3), 0, False, False, True, np.zeros(257 * 3 + 3, np.float32))
    with pytest.raises(NotImplementedError, match="257"):
        engine.mlp_forward(engine.zeros((4, 257), np.float32), spec)
    spec = MLPSpec((4,) * 10, 0, False, False, True, np.zeros(9 * 20, np.float32))
    with pytest.raises(NotImplementedError, match="9"):
        engine.mlp_forward(engine.zeros((4, 4), np.float32), spec)
    spec = MLPSpec((4, 65), 0, False, False, True, np.zeros(5 * 65, np.float32))
    with pytest.raises(NotImplementedError, match="65"):
        engine.mlp_forward(engine.zeros((4, 4), np.float32), spec)
    spec = MLPSpec((4, 3), 0, False, False, True, np.zeros(14, np.float32))        # one parameter short
    with pytest.raises(ValueError):
        engine.mlp_forward(engine.zeros((4, 4), np.float32), spec)
    assert _same_bits(_raw(engine, models, "one"), _raw(engine, models, "one"))    # the engine is usable afterwards
    assert np.max(np.abs(_raw(engine, models, "one") - R.case("one")["raw"])) < 1e-12


def test_capture_replays_to_the_same_bits(engine, models):
    c, spec = R.case("flagship"), models("flagship").spec
    xd = engine.to_device(c["X"])
    want = engine.mlp_forward(xd, spec).to_host()          # also uploads the parameters, outside the capture
    out = engine.zeros(want.shape, np.float64)
    engine.graph_begin()
    try:
        engine.mlp_forward(xd, spec, out=out)
    finally:
        g = engine.graph_end()
    try:
        for _ in range(2):
            out.zero_()
            engine.graph_launch(g)
            engine.sync()
            assert _same_bits(out.to_host(), want)
    finally:
        engine.graph_destroy(g)


def test_mlp_kernels_use_no_scratch(tmp_path):
    from tests.test_code_objects import _kernel_scratch

    sizes = {name: size for name, size in _kernel_scratch(tmp_path).items() if "mlp_" in name}
    assert len(sizes) >= 2, sizes                          # the float32 and the float64 instance
    assert not any(sizes.values()), sizes
