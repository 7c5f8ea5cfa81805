"""Metadynamics: a ledger of Gaussian hills on the device, its bias at any frame, and the weights that undo it.

The reference demonstrates one biased-sampling method, metadynamics: example_programs/14_muller_brown_active_bias.py
keeps an ActiveBiasLedger of hills in CV space (add_hill, potential_in_cv, force_on_xy, reproject_to,
stable_reweighting_factors), and its PLUMED validation run writes a HILLS and a COLVAR file.  Here the ledger lives on
the device (csrc/metad.hip): ``HillsLedger.bias`` is the N frames x H hills sum with its time dimension -- a frame
sees the hills deposited before it --, ``metadynamics_weights`` adds the time-dependent offset c(t) of Tiwary and
Parrinello (J. Phys. Chem. B 119, 736 (2015)) from one scan over a CV grid, and ``MetadynamicsReweighter`` writes
``dataset["frame_weights"]`` in the layout ``Reweighter.apply`` writes, where the FES, counting and weighted training
code pick them up.  ``read_hills`` / ``read_colvar`` read PLUMED's files.

Units: heights, kT and the bias share one energy unit; times share the unit of the hills' times."""

from __future__ import annotations

import re
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, Mapping, MutableMapping, Optional, Sequence

import numpy as np

from .. import _lib
from ..analysis.fes import BOLTZMANN_CONSTANT_KJ_PER_MOL
from ..device import DeviceArray, Engine, get_engine

__all__ = ["HillsLedger", "MetadWeights", "MetadynamicsReweighter", "metadynamics_weights", "read_colvar",
           "read_hills"]

DEFAULT_CUT = 6.25


# ---- PLUMED's files ------------------------------------------------------------------------------------------------
def _plumed_number(token: str) -> float:
    """A number as PLUMED writes it in a SET line: a float, or a multiple of pi ("pi", "-pi", "2pi", "0.5*pi")."""
    try:
        return float(token)
    except ValueError:
        m = re.fullmatch(r"([+-]?)(\d*\.?\d*)\*?pi", token.strip())
        if not m:
            raise ValueError(f"cannot read the number {token!r}") from None
        return (-1.0 if m.group(1) == "-" else 1.0) * (float(m.group(2)) if m.group(2) else 1.0) * np.pi


def _read_table(path):
    fields: Optional[list[str]] = None
    sets: dict[str, str] = {}
    rows: list[list[float]] = []
    for line in Path(path).read_text().splitlines():
        parts = line.split()
        if not parts:
            continue
        if parts[0] == "#!":
            if len(parts) >= 2 and parts[1] == "FIELDS":
                if fields is not None and parts[2:] != fields:
                    raise ValueError(f"{path}: the FIELDS line changes inside the file")
                fields = parts[2:]
            elif len(parts) >= 4 and parts[1] == "SET":
                sets[parts[2]] = parts[3]
            continue
        if parts[0].startswith("#"):
            continue
        if fields is None:
            raise ValueError(f"{path}: data before the '#! FIELDS' line")
        if len(parts) != len(fields):
            raise ValueError(f"{path}: a row has {len(parts)} columns, FIELDS names {len(fields)}")
        rows.append([float(p) for p in parts])
    if fields is None:
        raise ValueError(f"{path}: no '#! FIELDS' line")
    return fields, sets, np.asarray(rows, np.float64).reshape(len(rows), len(fields))


def read_colvar(path) -> Dict[str, np.ndarray]:
    """The named columns of a PLUMED COLVAR file, float64 each."""
    fields, _sets, data = _read_table(path)
    return {name: np.ascontiguousarray(data[:, i]) for i, name in enumerate(fields)}


def read_hills(path, *, engine: Engine | None = None) -> "HillsLedger":
    """A PLUMED HILLS file as a HillsLedger.  Reads the FIELDS line (time, the CVs, sigma_<cv>, height, biasf), the
    kerneltype and, for a periodic CV, its min_<cv> / max_<cv>.  ``multivariate true`` (non-diagonal hills) is
    refused.  Where biasf > 1 the file stores h gamma / (gamma - 1); the ledger holds the heights AS APPLIED
    (x (gamma - 1) / gamma) and keeps gamma as ``bias_factor``."""
    fields, sets, data = _read_table(path)
    if sets.get("multivariate", "false").lower() == "true":
        raise ValueError(f"{path}: multivariate (non-diagonal) hills are not supported")
    if len(fields) < 5 or fields[0] != "time" or fields[-2:] != ["height", "biasf"]:
        raise ValueError(f"{path}: FIELDS must read time <cvs> <sigmas> height biasf, got {fields}")
    if (len(fields) - 3) % 2:
        raise ValueError(f"{path}: FIELDS names {len(fields) - 3} CV and sigma columns, not a pair per CV")
    d = (len(fields) - 3) // 2
    names = fields[1:1 + d]
    if fields[1 + d:1 + 2 * d] != [f"sigma_{n}" for n in names]:
        raise ValueError(f"{path}: the sigma columns {fields[1 + d:1 + 2 * d]} do not match the CVs {names}")
    kernel = sets.get("kerneltype", "gaussian")
    if kernel not in _lib.METAD_KERNELS:
        raise ValueError(f"{path}: kerneltype {kernel!r} is not supported")
    periods = np.zeros(d)
    for i, n in enumerate(names):
        if f"min_{n}" in sets or f"max_{n}" in sets:
            if not (f"min_{n}" in sets and f"max_{n}" in sets):
                raise ValueError(f"{path}: {n} has only one of min_{n} / max_{n}")
            periods[i] = _plumed_number(sets[f"max_{n}"]) - _plumed_number(sets[f"min_{n}"])
            if not periods[i] > 0:
                raise ValueError(f"{path}: {n} has a period of {periods[i]}")
    biasf = data[:, -1]
    if data.shape[0] and not (biasf == biasf[0]).all():
        raise ValueError(f"{path}: biasf changes inside the file")
    gamma = float(biasf[0]) if data.shape[0] and biasf[0] > 1.0 else None
    heights = data[:, -2] * ((gamma - 1.0) / gamma) if gamma else data[:, -2].copy()
    return HillsLedger.from_arrays(data[:, 0], data[:, 1:1 + d], data[:, 1 + d:1 + 2 * d], heights, periods=periods,
                                   kernel=kernel, bias_factor=gamma, names=names, engine=engine)


# ---- the ledger ------------------------------------------------------------------------------------------------------
class HillsLedger:
    """Gaussian hills in the space of d collective variables: ``times`` [H], ``centers`` [H, d], ``sigmas`` [H, d]
    (per hill, diagonal), ``heights`` [H], ``periods`` [d] (0: not periodic), ``kernel`` ("gaussian" or
    "stretched-gaussian", PLUMED's default) and ``bias_factor`` (gamma of well-tempered metadynamics, or None).

    The records live in a device buffer with a capacity (centre, 1 / sigma, height per hill); ``add_hill`` appends one
    without waiting for the device, so a running simulation can deposit on line.  ``sigma``, ``height`` and ``kT`` are
    the defaults of ``add_hill``; with a bias factor, ``height`` is the initial height h0 of the well-tempered rule."""

    def __init__(self, n_cv: int, *, sigma=None, height: float | None = None, periods=None, kernel: str = "gaussian",
                 bias_factor: float | None = None, kT: float | None = None, cut: float = DEFAULT_CUT,
                 capacity: int = 256, names: Sequence[str] | None = None, engine: Engine | None = None) -> None:
        d = int(n_cv)
        if not 1 <= d <= _lib.METAD_MAX_D:
            raise ValueError(f"{d} collective variables, 1 to {_lib.METAD_MAX_D} are supported")
        if kernel not in _lib.METAD_KERNELS:
            raise ValueError(f"kernel must be one of {sorted(_lib.METAD_KERNELS)}, got {kernel!r}")
        if bias_factor is not None and not (np.isfinite(bias_factor) and bias_factor > 1.0):
            raise ValueError("bias_factor must be a finite number > 1 (None: no tempering)")
        if kT is not None and not (np.isfinite(kT) and kT > 0):
            raise ValueError("kT must be positive and finite")
        if not (np.isfinite(cut) and cut > 0):
            raise ValueError("cut must be positive and finite")
        per = np.zeros(d) if periods is None else np.asarray(periods, np.float64).reshape(-1)
        if per.size != d or not (np.isfinite(per).all() and (per >= 0).all()):
            raise ValueError(f"periods must be {d} finite numbers >= 0 (0: not periodic)")
        self.n_cv, self.periods, self.kernel, self.cut = d, per.copy(), kernel, float(cut)
        self.bias_factor = None if bias_factor is None else float(bias_factor)
        self.kT = None if kT is None else float(kT)
        self.sigma = None if sigma is None else self._sigma(sigma)
        self.height = None if height is None else float(height)
        self.names = list(names) if names is not None else [f"cv{i}" for i in range(d)]
        self.engine = engine
        cap = max(int(capacity), 1)
        self._n = 0
        self._times = np.zeros(cap)
        self._sig = np.zeros((cap, d))
        self._rec = np.zeros((cap, 2 * d + 1))      # the packed records as the device holds them
        self._dev: DeviceArray | None = None        # [capacity, 2 d + 1]; None: not uploaded yet
        self._device_rows: list[int] = []           # records the device wrote and the host has not read back

    @classmethod
    def from_arrays(cls, times, centers, sigmas, heights, **kw) -> "HillsLedger":
        c = np.asarray(centers, np.float64)
        c = c.reshape(c.shape[0], -1) if c.size else c.reshape(0, max(c.shape[-1] if c.ndim > 1 else 1, 1))
        H, d = c.shape
        t = np.asarray(times, np.float64).reshape(-1)
        s = np.asarray(sigmas, np.float64)
        s = np.broadcast_to(s, (H, d)) if s.ndim < 2 else s
        h = np.broadcast_to(np.asarray(heights, np.float64), (H,))
        if t.size != H or s.shape != (H, d):
            raise ValueError(f"times [{t.size}], centers {c.shape} and sigmas {s.shape} disagree")
        if H and not (np.isfinite(c).all() and np.isfinite(s).all() and (s > 0).all() and np.isfinite(h).all()
                      and np.isfinite(t).all()):
            raise ValueError("times, centers, sigmas and heights must be finite, sigmas positive")
        if H > 1 and (np.diff(t) < 0).any():
            raise ValueError("the hills' times must not decrease")
        led = cls(d, capacity=max(H, 1), **kw)
        led._n = H
        led._times[:H], led._sig[:H] = t, s
        led._rec[:H] = np.concatenate([c, 1.0 / s, h[:, None]], axis=1)
        return led

    # -- what it holds ---------------------------------------------------------
    def __len__(self) -> int:
        return self._n

    @property
    def capacity(self) -> int:
        return self._rec.shape[0]

    @property
    def times(self) -> np.ndarray:
        return self._times[:self._n].copy()

    @property
    def sigmas(self) -> np.ndarray:
        return self._sig[:self._n].copy()

    @property
    def centers(self) -> np.ndarray:
        self._read_back()
        return self._rec[:self._n, :self.n_cv].copy()

    @property
    def heights(self) -> np.ndarray:
        self._read_back()
        return self._rec[:self._n, 2 * self.n_cv].copy()

    def packed(self) -> np.ndarray:
        """The records as the device holds them: [H, 2 d + 1] = centre, 1 / sigma, height."""
        self._read_back()
        return self._rec[:self._n].copy()

    def _sigma(self, sigma) -> np.ndarray:
        s = np.broadcast_to(np.asarray(sigma, np.float64), (self.n_cv,)).copy()
        if not (np.isfinite(s).all() and (s > 0).all()):
            raise ValueError("sigma must be positive and finite")
        return s

    # -- the device copy ---------------------------------------------------------
    def _engine(self) -> Engine:
        if self.engine is None:
            self.engine = get_engine()
        return self.engine

    def _read_back(self) -> None:
        if self._device_rows:
            dev = self._dev.to_host()
            rows = np.asarray(self._device_rows)
            self._rec[rows] = dev[rows]
            self._device_rows = []

    def device_hills(self) -> DeviceArray:
        """The packed device buffer [capacity, 2 d + 1], its first len(self) records current."""
        eng = self._engine()
        if self._dev is None:
            self._dev = eng.to_device(self._rec)
        return self._dev

    def _grow(self) -> None:
        self._read_back()
        cap = 2 * self.capacity
        for name in ("_times", "_sig", "_rec"):
            old = getattr(self, name)
            new = np.zeros((cap,) + old.shape[1:])
            new[:old.shape[0]] = old
            setattr(self, name, new)
        self._dev = None                     # uploaded again, at the new capacity, on the next use

    # -- deposition ----------------------------------------------------------------
    def add_hill(self, center, sigma=None, height: float | None = None, *, time: float | None = None) -> int:
        """Appends one hill and returns its index.  `center`: d numbers, or a device array whose first d float64
        entries are the CVs (they never visit the host).  `sigma` and `height` default to the ledger's.  With
        height=None, a bias factor and the ledger's ``height`` h0 and ``kT``, the well-tempered height
        h0 exp(-V(center) / ((gamma - 1) kT)) is evaluated on the device, V being the bias of the hills so far.
        `time` defaults to the last hill's time plus the last spacing (1 for the first hills)."""
        d = self.n_cv
        sig = self._sigma(sigma) if sigma is not None else self.sigma
        if sig is None:
            raise ValueError("add_hill needs a sigma (or a ledger built with one)")
        on_device = isinstance(center, DeviceArray)
        if on_device:
            if center.dtype != np.float64 or center.size < d:
                raise ValueError(f"a device center must be float64 with at least {d} entries")
            c = np.full(d, np.nan)
        else:
            c = np.asarray(center, np.float64).reshape(-1)
            if c.size != d or not np.isfinite(c).all():
                raise ValueError(f"center must be {d} finite numbers")
        tempered = height is None and self.bias_factor is not None
        if height is None:
            if self.height is None:
                raise ValueError("add_hill needs a height (or a ledger built with one)")
            if tempered and self.kT is None:
                raise ValueError("the well-tempered height needs the ledger's kT")
            h = self.height
        else:
            h = float(height)
        if not (np.isfinite(h) and h >= 0):
            raise ValueError("height must be finite and >= 0")
        if time is None:
            n = self._n
            time = 0.0 if n == 0 else self._times[n - 1] + (self._times[n - 1] - self._times[n - 2] if n > 1 else 1.0)
        if self._n and time < self._times[self._n - 1]:
            raise ValueError("a hill cannot be deposited before the last one")
        if self._n == self.capacity:
            self._grow()
        k = self._n
        rec = np.concatenate([c, 1.0 / sig, [h]])
        self._times[k], self._sig[k] = float(time), sig
        self._rec[k] = rec
        if on_device or tempered or self._dev is not None:
            eng, dev = self._engine(), self.device_hills()
            v = None
            if tempered:
                cd = center if on_device else eng.to_device(c.reshape(1, d))
                v = eng.metad_bias(cd.view((1, d)), dev, k, periods=self.periods, kernel=self.kernel, cut=self.cut)
            eng.metad_append(dev, k, np.where(np.isnan(rec), 0.0, rec), center=center if on_device else None, v=v,
                             v_scale=-1.0 / ((self.bias_factor - 1.0) * self.kT) if tempered else 0.0)
            if on_device or tempered:
                self._device_rows.append(k)
        self._n = k + 1
        return k

    def set_centers(self, centers) -> None:
        """Replaces every centre (the same hills seen through another CV model); heights, sigmas and times stay."""
        c = np.asarray(centers, np.float64)
        if c.shape != (self._n, self.n_cv) or not np.isfinite(c).all():
            raise ValueError(f"centers must be finite with shape ({self._n}, {self.n_cv})")
        self._read_back()
        self._rec[:self._n, :self.n_cv] = c
        self._dev = None

    # -- evaluation ------------------------------------------------------------------
    def counts(self, times) -> np.ndarray:
        """Hills a frame at each of `times` sees: those deposited strictly before it (a frame at exactly a hill's time
        does not see that hill, as in PLUMED)."""
        t = np.asarray(times, np.float64).reshape(-1)
        return np.searchsorted(self._times[:self._n], t, side="left").astype(np.int32)

    def bias(self, cv, times=None, counts=None, grad: bool = False, *, max_workgroups: int = 0):
        """V(s_n, t_n) of the frames cv [n, d] (host array or float64 device array with >= d columns): the sum of the
        hills frame n sees -- counts[n] of them, or those before times[n], or all.  With grad also dV/ds [n, d].
        Host input gives host arrays, device input device arrays.  A frame with a non-finite CV is NaN."""
        if times is not None and counts is not None:
            raise ValueError("give times or counts, not both")
        eng = self._engine()
        host = not isinstance(cv, DeviceArray)
        if host:
            a = np.asarray(cv, np.float64)
            a = a.reshape(-1, self.n_cv) if a.ndim != 2 else a
            if a.shape[1] != self.n_cv:
                raise ValueError(f"cv must have {self.n_cv} columns, got {a.shape[1]}")
            if a.shape[0] == 0:
                return (np.zeros(0), np.zeros((0, self.n_cv))) if grad else np.zeros(0)
            cvd = eng.to_device(a)
        else:
            cvd = cv
        n = cvd.shape[0]
        cd = None
        if times is not None:
            counts = self.counts(times)
        if counts is not None:
            if isinstance(counts, DeviceArray):
                cd = counts
            else:
                cnt = np.asarray(counts).reshape(-1)
                if cnt.size != n:
                    raise ValueError(f"{cnt.size} times / counts for {n} frames")
                if cnt.size and (cnt.min() < 0 or cnt.max() > self._n):
                    raise ValueError(f"counts outside [0, {self._n}]")
                cd = eng.to_device(cnt, np.int32)
        out = eng.metad_bias(cvd, self.device_hills(), self._n, periods=self.periods, kernel=self.kernel, cut=self.cut,
                             counts=cd, grad=grad, max_workgroups=max_workgroups)
        if not host:
            if cd is not None and not isinstance(counts, DeviceArray):
                eng.sync()      # the uploaded counts are freed on return
            return out
        return (out[0].to_host(), out[1].to_host()) if grad else out.to_host()

    def grid(self, lo, hi, bins):
        """(lo, step, bins) of the regular grid with `bins` points per axis from lo to hi inclusive; a periodic axis
        runs over one period without the duplicate end point."""
        d = self.n_cv
        lo, hi = (np.broadcast_to(np.asarray(a, np.float64), (d,)).copy() for a in (lo, hi))
        bins = np.broadcast_to(np.asarray(bins, np.int64), (d,)).astype(np.int32)
        if d > _lib.METAD_GRID_MAX_D:
            raise ValueError(f"a grid takes at most {_lib.METAD_GRID_MAX_D} CVs, the ledger has {d}")
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all() and (bins >= 1).all()):
            raise ValueError("a grid needs finite lo < hi and bins >= 1")
        step = np.where(self.periods > 0, (hi - lo) / bins, (hi - lo) / np.maximum(bins - 1, 1))
        return lo, step, bins

    def scan(self, lo, hi, bins, checkpoints, a1: float, a2: float, *, want_grid: bool = False,
             max_workgroups: int = 0):
        """lse [M, 2] = log sum_g exp(a V_k(g)) at the checkpoints k for a = a1, a2 (Engine.metad_grid_scan), host
        arrays; with want_grid also V_H on the grid."""
        glo, step, gb = self.grid(lo, hi, bins)
        lse, vg = self._engine().metad_grid_scan(self.device_hills(), self._n, glo, step, gb, checkpoints, a1, a2,
                                                 periods=self.periods, kernel=self.kernel, cut=self.cut,
                                                 want_grid=want_grid, max_workgroups=max_workgroups)
        return (lse.to_host(), vg.to_host()) if want_grid else lse.to_host()

    def on_grid(self, lo, hi, bins) -> np.ndarray:
        """V_H, the bias of all hills, on the grid: float64 of shape `bins`."""
        return self.scan(lo, hi, bins, [self._n], 0.0, 0.0, want_grid=True)[1]

    def fes(self, lo, hi, bins) -> np.ndarray:
        """The free-energy estimate -gamma / (gamma - 1) V_H (the factor is 1 without tempering) on the grid, shifted so
        that its minimum is 0."""
        g = self.bias_factor
        F = -(g / (g - 1.0) if g else 1.0) * self.on_grid(lo, hi, bins)
        return F - F.min()


# ---- weights ---------------------------------------------------------------------------------------------------------
@dataclass
class MetadWeights:
    """weights sum to 1; log_weights = log(weights); ess is the Kish size 1 / sum w^2; c [M] is the offset at the
    checkpoints 0, rct_stride, 2 rct_stride, .. (None for method "final"); bias [n] is V(s_n, t_n)."""
    weights: np.ndarray
    log_weights: np.ndarray
    ess: float
    c: Optional[np.ndarray]
    bias: np.ndarray

    def __iter__(self):
        return iter((self.weights, self.log_weights, self.ess))


def _exponents(kT: float, bias_factor) -> tuple[float, float]:
    if bias_factor is None:
        return 1.0 / kT, 0.0
    g = float(bias_factor)
    return g / ((g - 1.0) * kT), 1.0 / ((g - 1.0) * kT)


def _unnormalised(ledger: HillsLedger, cv, times, kT: float, method: str, grid, rct_stride: int, offsets=None):
    """(log w [n] before normalising, c [M] or None, V [n]).  `offsets`: a dict that keeps c per ledger, so that frames
    given in several pieces (the splits of a dataset) pay for one grid scan per ledger, not one per piece."""
    if method not in ("tiwary", "final"):
        raise ValueError(f'method must be "tiwary" or "final", got {method!r}')
    if not (np.isfinite(kT) and kT > 0):
        raise ValueError("kT must be positive and finite")
    if int(rct_stride) < 1:
        raise ValueError("rct_stride must be >= 1")
    if method == "final":
        V = ledger.bias(cv)
        return V / kT, None, V
    if times is None:
        raise ValueError('method="tiwary" needs the frames\' times')
    if grid is None:
        raise ValueError('method="tiwary" needs grid=(lo, hi, bins) for the offset c(t)')
    counts = ledger.counts(times)
    V = ledger.bias(cv, counts=counts)
    stride = int(rct_stride)
    ck = np.arange(0, len(ledger) + 1, stride, dtype=np.int32)
    c = None if offsets is None else offsets.get(id(ledger))
    if c is None:
        a1, a2 = _exponents(kT, ledger.bias_factor)
        lse = ledger.scan(*grid, ck, a1, a2)
        c = kT * (lse[:, 0] - lse[:, 1])
        if offsets is not None:
            offsets[id(ledger)] = c
    return (V - c[counts // stride]) / kT, c, V


def _normalise(logw: np.ndarray):
    if not np.isfinite(logw).all():
        raise ValueError("a frame has a non-finite bias: its CVs are not finite")
    if logw.size == 0:
        raise ValueError("no frames")
    m = logw.max()
    lw = logw - (m + np.log(np.exp(logw - m).sum()))
    w = np.exp(lw)
    return w, lw, float(1.0 / np.sum(w * w))


def metadynamics_weights(ledger: HillsLedger, cv, times=None, kT: float = None, method: str = "tiwary", grid=None,
                         rct_stride: int = 1) -> MetadWeights:
    """Weights that turn the frames of a metadynamics run into samples of the unbiased ensemble.

    "tiwary": log w_n = (V(s_n, t_n) - c(t_n)) / kT with c_k = kT (LSE_g(a1 V_k) - LSE_g(a2 V_k)) over the CV grid
    ``grid=(lo, hi, bins)``, a1 = gamma / ((gamma - 1) kT), a2 = 1 / ((gamma - 1) kT) (without tempering 1 / kT
    and 0), c_0 = 0; c is evaluated every ``rct_stride`` hills and held between evaluations, as PLUMED's RCT_USTRIDE
    does.  "final": log w_n = V_H(s_n) / kT, the bias of all hills.  Unpacks as (weights, log_weights, ess)."""
    if kT is None:
        raise ValueError("metadynamics_weights needs kT")
    logw, c, V = _unnormalised(ledger, cv, times, float(kT), method, grid, rct_stride)
    w, lw, ess = _normalise(logw)
    return MetadWeights(w, lw, ess, c, V)


class MetadynamicsReweighter:
    """``MetadynamicsReweighter(kT=...).apply(dataset)`` writes ``dataset["frame_weights"]`` as ``Reweighter.apply``
    does: one float64 array per split, jointly normalised (summed over all splits they give 1).

    Every split of ``dataset["splits"]`` carries ``"cv"`` [N_s, d], the CV columns the hills were deposited in, and
    (method "tiwary") ``"time"`` [N_s].  The hills are the ``ledger`` given here (a HillsLedger or the path of a HILLS
    file), or a split's own ``"ledger"``.  ``kT`` in the hills' energy unit, or ``temperature_K`` (kJ / mol)."""

    def __init__(self, kT: float | None = None, *, temperature_K: float | None = None, ledger=None,
                 method: str = "tiwary", grid=None, rct_stride: int = 1) -> None:
        if (kT is None) == (temperature_K is None):
            raise ValueError("give exactly one of kT and temperature_K")
        value = float(kT) if kT is not None else BOLTZMANN_CONSTANT_KJ_PER_MOL * float(temperature_K)
        if not (np.isfinite(value) and value > 0):
            raise ValueError("kT / temperature_K must be positive and finite")
        if method not in ("tiwary", "final"):
            raise ValueError(f'method must be "tiwary" or "final", got {method!r}')
        if method == "tiwary" and grid is None:
            raise ValueError('method="tiwary" needs grid=(lo, hi, bins)')
        if int(rct_stride) < 1:
            raise ValueError("rct_stride must be >= 1")
        self.kT, self.method, self.grid, self.rct_stride = value, method, grid, int(rct_stride)
        self.ledger = self._ledger(ledger)
        self.result: Dict[str, Any] | None = None     # per split: c and bias of the latest apply()

    @staticmethod
    def _ledger(ledger):
        if ledger is None or isinstance(ledger, HillsLedger):
            return ledger
        return read_hills(ledger)

    def apply(self, dataset: MutableMapping[str, Any]) -> Dict[str, np.ndarray]:
        splits = dataset.get("splits") if isinstance(dataset, Mapping) else None
        if not isinstance(splits, Mapping) or not splits:
            raise ValueError('MetadynamicsReweighter.apply needs dataset["splits"]')
        logs, sizes, self.result = [], {}, {}
        offsets: dict = {}          # c(t) per ledger: one grid scan however many splits share the ledger
        own: dict = {}              # a split's ledger given as a path is read once per path
        for name, split in splits.items():
            if not isinstance(split, Mapping) or split.get("cv") is None:
                raise ValueError(f"split '{name}' has no \"cv\"")
            ledger = split.get("ledger")
            if ledger is not None and not isinstance(ledger, HillsLedger):
                if str(ledger) not in own:
                    own[str(ledger)] = read_hills(ledger)
                ledger = own[str(ledger)]
            if ledger is None:
                ledger = self.ledger
            if ledger is None:
                raise ValueError(f"split '{name}' has no \"ledger\" and the reweighter was built without one")
            cv = np.asarray(split["cv"], np.float64)
            cv = cv.reshape(-1, ledger.n_cv) if cv.ndim != 2 else cv
            times = split.get("time")
            if self.method == "tiwary":
                if times is None:
                    raise ValueError(f"split '{name}' has no \"time\": method=\"tiwary\" needs the frames' times")
                if np.asarray(times).size != cv.shape[0]:
                    raise ValueError(f"split '{name}': time has {np.asarray(times).size} entries, "
                                     f"cv {cv.shape[0]} rows")
            logw, c, V = _unnormalised(ledger, cv, times, self.kT, self.method, self.grid, self.rct_stride, offsets)
            logs.append(logw)
            sizes[str(name)] = logw.size
            self.result[str(name)] = {"c": c, "bias": V}
        w, _lw, ess = _normalise(np.concatenate(logs))
        self.result["ess"] = ess
        out: Dict[str, np.ndarray] = {}
        at = 0
        for name, n in sizes.items():
            out[name] = w[at:at + n].copy()
            at += n
        fw = dataset.get("frame_weights")
        if not isinstance(fw, MutableMapping):
            fw = {}
            dataset["frame_weights"] = fw
        fw.update(out)
        return out
