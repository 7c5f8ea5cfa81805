"""Inference with a trained DeepTICA network on the device: mirror of pmarlo.features.deeptica.DeepTICAModel's
load / transform (S/features/deeptica/_full.py:283-387) for the network that override_core_mlp and PrePostWrapper
build (S/features/deeptica/core/model.py:72-107, 355-368).

transform(X) in evaluation mode is: Z = (X - mean_) / scale_ in fp64, rounded to fp32; an optional LayerNorm over
the inputs; Linear layers of widths [F, *hidden, n_out], each hidden one followed by an optional LayerNorm and the
activation (dropout is the identity); the activation once more on the outputs unless linear_head is set; then, when
the training history carries output_mean / output_transform, the output whitening of
analysis.project_cv.apply_output_transform.  Scaler, network and whitening passes run on the device
(msm_mlp_forward, then the projection and moment kernels); the frames never come back to the host in between.

Training lives next door (trainer.py: DeepTICACurriculumTrainer); this module gives it `initialize`, a freshly
initialised network, and `save`, which writes the bundle `load` reads.  Stated divergence of `initialize`: weights and
biases are drawn uniform in +-1/sqrt(fan_in) from numpy's generator, the distribution of torch's Linear for the
biases and (in the bound, not the stream) for the weights; the stream is not torch's, so a seed gives other numbers
than the reference's build_network.  torch is needed to read and write the reference's `.pt` files and for nothing
else: it is imported inside `load` and `save` only, and `from_arrays` builds the same object from numpy arrays."""

from __future__ import annotations

import json
import re
from pathlib import Path
from typing import Any, Mapping, Sequence

import numpy as np

from ..._lib import MLP_MAX_LINEAR, MLP_MAX_OUT, MLP_MAX_WIDTH
from ...analysis import project_cv

__all__ = ["DeepTICAModel", "MLPSpec", "activation_code", "dropout_sites", "resolve_hidden_layers", "state_dict_layout"]

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


def _hidden_dropout(spec, transitions: int) -> list[float]:
    """normalize_hidden_dropout (model.py:53-69): one probability per hidden layer, the last one repeated."""
    if transitions <= 0:
        return []
    if spec is None:
        return [0.0] * transitions
    if isinstance(spec, (int, float, str)) and not isinstance(spec, bool):
        return [float(spec)] * transitions
    values = [float(v) for v in spec] or [0.0]
    return (values + [values[-1]] * transitions)[:transitions]


def dropout_sites(config: Mapping[str, Any], n_linear: int) -> list[float]:
    """Dropout probabilities in training mode, one per Linear layer: the inputs (resolve_input_dropout,
    model.py:262-266: `dropout_input`, else `dropout`, else DeepTICAConfig's default 0; clamped at 0), then the
    hidden layers.  A probability of 1 or more raises ValueError (the reference would zero every activation)."""
    p_in = config.get("dropout_input")
    if p_in is None:
        p_in = config.get("dropout", 0.0)
    sites = [max(0.0, float(0.0 if p_in is None else p_in))]
    sites += [max(0.0, p) for p in _hidden_dropout(config.get("hidden_dropout"), n_linear - 1)]
    for i, p in enumerate(sites):
        if not p < 1.0:
            raise ValueError(f"dropout probability {p} at site {i} (0 <= p < 1)")
    return sites


def state_dict_layout(config: Mapping[str, Any], F: int) -> list[tuple[str, tuple[int, ...]]]:
    """[(key, shape), ...] of the reference network's state_dict in the packed order of the parameters.  The
    Sequential gives an index to every module, so LayerNorms, activations and dropouts with p > 0 make the Linear
    indices skip (override_core_mlp, model.py:72-107)."""
    widths = (int(F), *resolve_hidden_layers(config), int(config.get("n_out", config.get("output_dim", 2))))
    drop = _hidden_dropout(config.get("hidden_dropout"), len(widths) - 2)
    keys: list[tuple[str, tuple[int, ...]]] = []
    if bool(config.get("layer_norm_in", False)):
        keys += [("ln.weight", (widths[0],)), ("ln.bias", (widths[0],))]
    idx = 0
    for i in range(len(widths) - 1):
        keys += [(f"inner.nn.{idx}.weight", (widths[i + 1], widths[i])), (f"inner.nn.{idx}.bias", (widths[i + 1],))]
        idx += 1
        if i < len(widths) - 2:
            if bool(config.get("layer_norm_hidden", False)):
                keys += [(f"inner.nn.{idx}.weight", (widths[i + 1],)), (f"inner.nn.{idx}.bias", (widths[i + 1],))]
                idx += 1
            idx += 1 + (1 if drop[i] > 0 else 0)        # the activation, the dropout
    return keys


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

    @classmethod
    def initialize(cls, config: Mapping[str, Any], scaler_mean, scaler_std, seed: int = 0) -> "DeepTICAModel":
        """A network ready for training: Linear weights and biases uniform in +-1/sqrt(fan_in) from
        numpy.random.default_rng(seed), LayerNorms at (1, 0).  The stream is not torch's (module docstring)."""
        F = int(np.asarray(scaler_mean).reshape(-1).shape[0])
        rng = np.random.default_rng(seed)
        params: dict[str, np.ndarray] = {}
        bound = 1.0
        for key, shape in state_dict_layout(config, F):
            if len(shape) == 2:
                bound = 1.0 / np.sqrt(shape[1])
                params[key] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
            elif key.endswith("weight"):
                params[key] = np.ones(shape, np.float32)                        # LayerNorm gamma
            elif key.startswith("ln.") or params[key.replace("bias", "weight")].ndim == 1:
                params[key] = np.zeros(shape, np.float32)                       # LayerNorm beta
            else:
                params[key] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
        return cls.from_arrays(config, params, scaler_mean, scaler_std)

    def state_dict(self) -> dict[str, np.ndarray]:
        """The parameters under the reference's key names, unpacked from the spec (fp32 copies)."""
        out, off = {}, 0
        for key, shape in state_dict_layout(self.config, self.spec.widths[0]):
            size = int(np.prod(shape))
            out[key] = self.spec.params[off:off + size].reshape(shape).copy()
            off += size
        assert off == self.spec.params.size
        return out

    def save(self, path) -> None:
        """Write the bundle `load` reads (the reference's DeepTICAModel.save, _full.py:311-352): `<path>.json`,
        `<path>.pt`, `<path>.scaler.pt` and, with a non-empty history, `<path>.history.json`."""
        import torch  # only to write the two .pt files

        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.with_suffix(".json").write_text(
            json.dumps(self.config, sort_keys=True, separators=(",", ":"), allow_nan=False), encoding="utf-8")
        torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in self.state_dict().items()}},
                   path.with_suffix(".pt"))
        mean = self.spec.mean if self.spec.mean is not None else np.zeros(self.spec.widths[0])
        scale = self.spec.scale if self.spec.scale is not None else np.ones(self.spec.widths[0])
        torch.save({"mean": np.asarray(mean), "std": np.asarray(scale)}, path.with_suffix(".scaler.pt"))
        if self.training_history:
            path.with_suffix(".history.json").write_text(
                json.dumps(self.training_history, sort_keys=True, indent=2), encoding="utf-8")

    def __eq__(self, other):
        """Same config, parameters, scaler and history; config and history are compared as the JSON `save` writes
        (a tuple equals the list it is stored as, an integer key the string it becomes)."""
        if not isinstance(other, DeepTICAModel):
            return NotImplemented

        def norm(obj):
            return json.loads(json.dumps(obj, sort_keys=True))

        return (norm(self.config) == norm(other.config) and self.spec == other.spec
                and norm(self.training_history) == norm(other.training_history))

    __hash__ = None

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
