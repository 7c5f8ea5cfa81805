"""Inference with a trained DeepTICA network on the device: mirror of pmarlo.features.deeptica.DeepTICAModel's
load / transform (S/features/deeptica/_full.py:283-387) for the network that override_core_mlp and PrePostWrapper
build (S/features/deeptica/core/model.py:72-107, 355-368).

transform(X) in evaluation mode is: Z = (X - mean_) / scale_ in fp64, rounded to fp32; an optional LayerNorm over
the inputs; Linear layers of widths [F, *hidden, n_out], each hidden one followed by an optional LayerNorm and the
activation (dropout is the identity); the activation once more on the outputs unless linear_head is set; then, when
the training history carries output_mean / output_transform, the output whitening of
analysis.project_cv.apply_output_transform.  Scaler, network and whitening passes run on the device
(msm_mlp_forward, then the projection and moment kernels); the frames never come back to the host in between.

Training is out of scope.  torch is needed to read the reference's `.pt` files and for nothing else: it is imported
inside `load` only, and `from_arrays` builds the same object from numpy arrays."""

from __future__ import annotations

import json
import re
from pathlib import Path
from typing import Any, Mapping, Sequence

import numpy as np

from ..._lib import MLP_MAX_LINEAR, MLP_MAX_OUT, MLP_MAX_WIDTH
from ...analysis import project_cv

__all__ = ["DeepTICAModel", "MLPSpec", "activation_code", "resolve_hidden_layers"]

ACT_TANH, ACT_GELU, ACT_RELU, ACT_ELU, ACT_SELU, ACT_LEAKY_RELU = range(6)
_ACTIVATIONS = {"gelu": ACT_GELU, "gaussian": ACT_GELU, "relu": ACT_RELU, "relu+": ACT_RELU, "elu": ACT_ELU,
                "selu": ACT_SELU, "leaky_relu": ACT_LEAKY_RELU, "lrelu": ACT_LEAKY_RELU}


def activation_code(name) -> int:
    """resolve_activation_module (model.py:36-50): any name it does not know is tanh."""
    return _ACTIVATIONS.get(str(name or "").strip().lower(), ACT_TANH)


def resolve_hidden_layers(config: Mapping[str, Any]) -> tuple[int, ...]:
    """model.py:248-252: no hidden layer under linear_head, (32, 16) for an empty list."""
    if bool(config.get("linear_head", False)):
        return ()
    hidden = tuple(int(h) for h in (config.get("hidden", ()) or ()))
    return hidden if hidden else (32, 16)


class MLPSpec:
    """What Engine.mlp_forward needs of a network: widths [F, ..., n_out], activation code, the three flags, the
    fp32 parameters packed in msm_mlp_forward's order, and the scaler (mean, scale; both None: identity)."""

    def __init__(self, widths: Sequence[int], activation: int, ln_in: bool, ln_hidden: bool, head_activation: bool,
                 params: np.ndarray, mean: np.ndarray | None = None, scale: np.ndarray | None = None):
        self.widths = tuple(int(w) for w in widths)
        self.activation = int(activation)
        self.ln_in, self.ln_hidden, self.head_activation = bool(ln_in), bool(ln_hidden), bool(head_activation)
        self.params = np.ascontiguousarray(params, np.float32).reshape(-1)
        self.mean = None if mean is None else np.ascontiguousarray(mean, np.float64).reshape(-1)
        self.scale = None if scale is None else np.ascontiguousarray(scale, np.float64).reshape(-1)
        self._dev = None    # (engine, parameters, mean, scale) once uploaded

    def n_params(self) -> int:
        """Number of parameters the widths and flags call for."""
        w = self.widths
        total = 2 * w[0] if self.ln_in else 0
        for i in range(len(w) - 1):
            total += w[i] * w[i + 1] + w[i + 1]
            if self.ln_hidden and i + 2 < len(w):
                total += 2 * w[i + 1]
        return total

    def check_envelope(self) -> None:
        """The limits of msm_mlp_forward, raised here without a device, naming the offending number."""
        w = self.widths
        if not 1 <= len(w) - 1 <= MLP_MAX_LINEAR:
            raise NotImplementedError(f"{len(w) - 1} Linear layers (1 to {MLP_MAX_LINEAR} are supported)")
        for i, wi in enumerate(w):
            if wi < 1:
                raise ValueError(f"width {wi} of layer {i}")
            if wi > MLP_MAX_WIDTH:
                raise NotImplementedError(f"width {wi} of layer {i} (at most {MLP_MAX_WIDTH} is supported)")
        if w[-1] > MLP_MAX_OUT:
            raise NotImplementedError(f"{w[-1]} outputs (at most {MLP_MAX_OUT} are supported)")

    def __eq__(self, other):
        if not isinstance(other, MLPSpec):
            return NotImplemented

        def same(a, b):
            return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))

        return ((self.widths, self.activation, self.ln_in, self.ln_hidden, self.head_activation)
                == (other.widths, other.activation, other.ln_in, other.ln_hidden, other.head_activation)
                and np.array_equal(self.params, other.params) and same(self.mean, other.mean)
                and same(self.scale, other.scale))

    __hash__ = None


def _walk_state_dict(params: Mapping[str, np.ndarray]):
    """The Linear / LayerNorm sequence of `inner.nn.{i}.*` in index order (activations and dropouts own indices
    but no keys): [(W, b, gamma or None, beta or None), ...].  A 2-D weight is a Linear, a 1-D weight after it its
    LayerNorm."""
    found: dict[int, dict[str, np.ndarray]] = {}
    for key, value in params.items():
        m = re.fullmatch(r"inner\.nn\.(\d+)\.(weight|bias)", key)
        if m:
            found.setdefault(int(m.group(1)), {})[m.group(2)] = np.asarray(value)
    layers: list[list] = []
    for idx in sorted(found):
        entry = found[idx]
        if "weight" not in entry or "bias" not in entry:
            raise ValueError(f"inner.nn.{idx}: {'weight' if 'weight' not in entry else 'bias'} is missing")
        W, b = entry["weight"], entry["bias"]
        if W.ndim == 2:
            if b.shape != (W.shape[0],):
                raise ValueError(f"inner.nn.{idx}: bias {b.shape} does not fit weight {W.shape}")
            layers.append([W, b, None, None])
        elif W.ndim == 1:
            if not layers or layers[-1][2] is not None:
                raise ValueError(f"inner.nn.{idx}: a LayerNorm that follows no Linear layer")
            if W.shape != layers[-1][1].shape or b.shape != W.shape:
                raise ValueError(f"inner.nn.{idx}: LayerNorm of width {W.shape} after a Linear of width {layers[-1][1].shape}")
            layers[-1][2], layers[-1][3] = W, b
        else:
            raise ValueError(f"inner.nn.{idx}.weight has {W.ndim} dimensions")
    return layers


def _build_spec(config: Mapping[str, Any], params: Mapping[str, np.ndarray], mean, scale) -> MLPSpec:
    mean = np.asarray(mean, np.float64).reshape(-1)
    scale = np.asarray(scale, np.float64).reshape(-1)
    if mean.shape != scale.shape:
        raise ValueError(f"scaler mean {mean.shape} and std {scale.shape} differ in length")
    F = int(mean.shape[0])
    n_out = int(config.get("n_out", config.get("output_dim", 2)))
    ln_in = bool(config.get("layer_norm_in", False))
    ln_hidden = bool(config.get("layer_norm_hidden", False))
    linear_head = bool(config.get("linear_head", False))
    widths = (F, *resolve_hidden_layers(config), n_out)
    MLPSpec(widths, 0, ln_in, ln_hidden, not linear_head, np.zeros(0, np.float32)).check_envelope()

    # when the bundle holds keys the network does not have, the reference loads once more with one leading `inner.`
    # stripped from every key (_full.py:373-383): a network saved inside another wrapper carries `inner.ln.*` and
    # `inner.inner.nn.{i}.*`
    known = re.compile(r"(ln|inner\.nn\.\d+)\.(weight|bias)").fullmatch
    if any(not known(k) for k in params):
        stripped = {(k[6:] if k.startswith("inner.") else k): v for k, v in params.items()}
        params = {**{k: v for k, v in params.items() if known(k)}, **{k: v for k, v in stripped.items() if known(k)}}
    layers = _walk_state_dict(params)
    found = tuple([int(layers[0][0].shape[1])] + [int(L[0].shape[0]) for L in layers]) if layers else ()
    if found != widths:
        missing = "a parameter is missing or " if len(found) < len(widths) else ""
        raise ValueError(f"{missing}the bundle's Linear layers have widths {found}, its config calls for {widths}")
    for i, L in enumerate(layers):
        if i and L[0].shape[1] != layers[i - 1][0].shape[0]:
            raise ValueError(f"Linear {i} takes {L[0].shape[1]} inputs after {layers[i - 1][0].shape[0]} outputs")
    parts: list[np.ndarray] = []
    if ln_in:
        if "ln.weight" not in params or "ln.bias" not in params:
            raise ValueError("layer_norm_in is set but ln.weight / ln.bias is missing")
        g, b = np.asarray(params["ln.weight"]), np.asarray(params["ln.bias"])
        if g.shape != (F,) or b.shape != (F,):
            raise ValueError(f"input LayerNorm of shape {g.shape} / {b.shape} for {F} features")
        parts += [g, b]
    for i, (W, b, g, beta) in enumerate(layers):
        hidden = i + 1 < len(layers)
        if (g is not None) != (ln_hidden and hidden):
            raise ValueError(f"Linear {i}: LayerNorm parameters {'missing' if g is None else 'present'} with "
                             f"layer_norm_hidden = {ln_hidden}")
        parts += [W, b] + ([g, beta] if g is not None else [])
    packed = np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in parts])
    spec = MLPSpec(widths, activation_code(config.get("activation", "gelu")), ln_in, ln_hidden, not linear_head, packed,
                   mean, scale)
    assert packed.size == spec.n_params()
    return spec


class DeepTICAModel:
    """A trained DeepTICA network with its scaler and training history, evaluated on the device."""

    def __init__(self, config: Mapping[str, Any], spec: MLPSpec, history: Mapping[str, Any] | None = None):
        self.config = dict(config)
        self.spec = spec
        self.training_history = dict(history) if isinstance(history, Mapping) else {}

    @classmethod
    def from_arrays(cls, config: Mapping[str, Any], params: Mapping[str, np.ndarray], scaler_mean, scaler_std,
                    history: Mapping[str, Any] | None = None) -> "DeepTICAModel":
        """The model from the reference's config fields (unknown keys ignored), its state_dict as numpy arrays under
        the reference's key names, and the scaler's mean_ / scale_.  A parameter the config calls for and the arrays
        lack raises ValueError (the reference loads with strict=False and would keep random initial weights)."""
        return cls(config, _build_spec(config, params, scaler_mean, scaler_std), history)

    @classmethod
    def load(cls, path) -> "DeepTICAModel":
        """Read the reference's bundle (DeepTICAModel.save, _full.py:311-352): `<path>.json` (config), `<path>.pt`
        ({"state_dict": ...}), `<path>.scaler.pt` (mean, std) and, if present, `<path>.history.json`."""
        import torch  # only to read the two .pt files

        path = Path(path)
        config = json.loads(path.with_suffix(".json").read_text(encoding="utf-8"))
        state = torch.load(path.with_suffix(".pt"), map_location="cpu", weights_only=False)["state_dict"]
        scaler = torch.load(path.with_suffix(".scaler.pt"), map_location="cpu", weights_only=False)

        def as_np(v):
            return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)

        params = {k: as_np(v) for k, v in state.items()}
        history = None
        hist_path = path.with_suffix(".history.json")
        if hist_path.exists():
            try:
                history = json.loads(hist_path.read_text(encoding="utf-8"))
            except ValueError:
                history = None
        return cls.from_arrays(config, params, as_np(scaler["mean"]), as_np(scaler["std"]),
                               history if isinstance(history, dict) else None)

    # -- evaluation ---------------------------------------------------------
    def transform_device(self, xd):
        """Collective variables [n, n_out] float64 on the device for frames xd [n, F] (float32 or float64 device
        array): network, then the output whitening when the history carries it.  Inconsistent whitening metadata
        (the ValueError / TypeError of apply_output_transform) leaves the raw outputs, as the reference does; device
        errors propagate."""
        eng = xd.engine
        if len(xd.shape) != 2 or xd.shape[1] != self.spec.widths[0]:
            raise ValueError(f"frames of shape {xd.shape} for a network of {self.spec.widths[0]} features")
        raw = eng.mlp_forward(xd, self.spec)
        hist = self.training_history
        mean, transform = hist.get("output_mean"), hist.get("output_transform")
        if mean is None or transform is None or xd.shape[0] == 0:
            return raw
        try:
            if project_cv._coerce_bool_flag(hist.get("output_transform_applied")):
                return raw
            mu, T = project_cv._output_transform_metadata(raw.shape, mean, transform)
            v, drift = project_cv.output_transform_device(eng, raw, mu, T)
        except (ValueError, TypeError):
            return raw
        m = T.shape[1]
        return eng.project(v, drift, eng.to_device(np.ones(m)), eng.to_device(np.eye(m)), m)    # v - drift

    def transform(self, X) -> np.ndarray:
        """transform_device on host frames [n, F]; float32 input is uploaded as it is, anything else as float64."""
        from ...device import get_engine

        X = np.asarray(X)
        if X.dtype != np.float32:
            X = np.asarray(X, np.float64)
        if X.ndim != 2:
            raise ValueError(f"frames must be a 2D array, got shape {X.shape}")
        if X.shape[0] == 0:
            return np.zeros((0, self.spec.widths[-1]))
        return self.transform_device(get_engine().to_device(np.ascontiguousarray(X))).to_host()
