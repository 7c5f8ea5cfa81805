"""OPES: a ledger of compressed kernels on the device, its bias at any frame, and the weights that undo it.

OPES (Invernizzi and Parrinello, J. Phys. Chem. Lett. 11, 2731 (2020); PLUMED's OPES_METAD) builds its bias from an
on-line kernel density estimate of the sampled CV distribution: V(s) = kT (1 - 1 / gamma) log(P(s) / Z + epsilon).
The kernels are compressed as they arrive -- a new one merges into its nearest neighbour, possibly in a chain -- so
"the kernels deposited before a frame" is not a prefix of anything.  ``OPESLedger`` replays the deposit sequence on the
device (csrc/opes.hip) into a journal of kernel versions with life spans and evaluates N frames against it, each frame
against the kernels and the normalisation it actually saw; ``opes_weights`` and ``OPESReweighter`` turn that into
``dataset["frame_weights"]`` in the layout ``Reweighter.apply`` writes.  ``read_kernels`` reads PLUMED's KERNELS file.
``OPESLedger.deposit`` makes one deposit on line at CVs that may still be on the device.

The definition is this package's own ("OPES"); parity with PLUMED's numbers is not pinned.

Units: kT, the barrier and the bias share one energy unit; times share the unit of the kernels' times."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Mapping, MutableMapping, Sequence

import numpy as np

from .. import _lib
from ..analysis.fes import BOLTZMANN_CONSTANT_KJ_PER_MOL
from ..device import DeviceArray, Engine, get_engine
from .metadynamics import _normalise, _plumed_number, _read_table

__all__ = ["OPESLedger", "OPESReweighter", "OPESWeights", "opes_weights", "read_kernels"]


def read_kernels(path, kT: float, *, barrier: float | None = None, max_steps: int = 0,
                 engine: Engine | None = None) -> "OPESLedger":
    """A PLUMED KERNELS file (OPES_METAD) as an OPESLedger.  Reads the FIELDS line (time, the CVs, sigma_<cv>, height,
    logweight), the SET lines biasfactor, epsilon, kernel_cutoff, compression_threshold and, for a periodic CV, its
    min_<cv> / max_<cv>.  The file does not hold kT: it is given here, in the unit of the bias."""
    return OPESLedger.from_kernels(path, kT, barrier=barrier, max_steps=max_steps, engine=engine)


class OPESLedger:
    """The state of an OPES run in the space of d collective variables, on the device.

    ``kT``; ``barrier`` (the free-energy barrier to overcome) sets the defaults gamma = barrier / kT,
    epsilon = exp(-barrier / (kT p)) and cutoff = sqrt(2 barrier / (kT p)) with p = 1 - 1 / gamma; ``biasfactor``,
    ``epsilon``, ``cutoff`` override them (biasfactor = inf: p = 1).  ``threshold`` is the compression threshold,
    ``periods`` [d] (0: not periodic), ``sigma0`` [d] the kernel width of an on-line deposit, which shrinks with the
    effective sample size unless ``fixed_sigma``.

    ``deposit_records`` replays given deposits, ``deposit`` makes one on line; both run on the device and wait for
    nothing.  ``bias`` evaluates frames against the journal (each frame against the state it saw) or, with
    ``live=True``, against the live kernels."""

    def __init__(self, n_cv: int, kT: float, *, barrier: float | None = None, biasfactor: float | None = None,
                 epsilon: float | None = None, cutoff: float | None = None, threshold: float = 1.0, periods=None,
                 sigma0=None, fixed_sigma: bool = False, capacity: int = 256, max_steps: int = 0,
                 names: Sequence[str] | None = None, engine: Engine | None = None) -> None:
        d = int(n_cv)
        if not 1 <= d <= _lib.METAD_MAX_D:
            raise ValueError(f"{d} collective variables, 1 to {_lib.METAD_MAX_D} are supported")
        if not (np.isfinite(kT) and kT > 0):
            raise ValueError("kT must be positive and finite")
        if barrier is not None and not (np.isfinite(barrier) and barrier > 0):
            raise ValueError("barrier must be positive and finite")
        if biasfactor is None:
            if barrier is None:
                raise ValueError("give a barrier or a biasfactor")
            biasfactor = float(barrier) / float(kT)
        if not biasfactor > 1.0:
            raise ValueError("biasfactor (barrier / kT by default) must be > 1; inf gives p = 1")
        p = 1.0 if np.isinf(biasfactor) else 1.0 - 1.0 / float(biasfactor)
        if (epsilon is None or cutoff is None) and barrier is None:
            raise ValueError("without a barrier both epsilon and cutoff must be given")
        eps = float(np.exp(-float(barrier) / (float(kT) * p))) if epsilon is None else float(epsilon)
        cut = float(np.sqrt(2.0 * float(barrier) / (float(kT) * p))) if cutoff is None else float(cutoff)
        if not (np.isfinite(eps) and eps > 0):
            raise ValueError("epsilon must be positive and finite")
        if not (np.isfinite(cut) and cut > 0):
            raise ValueError("cutoff must be positive and finite")
        if not (np.isfinite(threshold) and threshold >= 0):
            raise ValueError("threshold must be finite and >= 0")
        per = np.zeros(d) if periods is None else np.asarray(periods, np.float64).reshape(-1)
        if per.size != d or not (np.isfinite(per).all() and (per >= 0).all()):
            raise ValueError(f"periods must be {d} finite numbers >= 0 (0: not periodic)")
        s0 = None
        if sigma0 is not None:
            s0 = np.broadcast_to(np.asarray(sigma0, np.float64), (d,)).copy()
            if not (np.isfinite(s0).all() and (s0 > 0).all()):
                raise ValueError("sigma0 must be positive and finite")
        if int(max_steps) < 0:
            raise ValueError("max_steps must be >= 0 (0: one launch per call)")
        self.n_cv, self.kT, self.barrier = d, float(kT), None if barrier is None else float(barrier)
        self.biasfactor, self.prefactor, self.epsilon, self.cutoff = float(biasfactor), p, eps, cut
        self.threshold, self.periods, self.sigma0 = float(threshold), per.copy(), s0
        self.fixed_sigma = bool(fixed_sigma)
        self.max_steps = int(max_steps)
        self.names = list(names) if names is not None else [f"cv{i}" for i in range(d)]
        self.engine = engine
        self._capacity = max(int(capacity), 1)
        self._dev: dict | None = None
        self._n = 0
        self._times = np.zeros(self._capacity)

    # -- construction ------------------------------------------------------------
    @classmethod
    def from_arrays(cls, times, centers, sigmas, heights, logweights, kT: float, **kw) -> "OPESLedger":
        """The ledger after replaying the deposits (time, centre, sigma, height, logweight) in order."""
        c = np.asarray(centers, np.float64)
        c = c.reshape(c.shape[0], -1) if c.size else c.reshape(0, max(c.shape[-1] if c.ndim > 1 else 1, 1))
        led = cls(c.shape[1], kT, capacity=max(c.shape[0], 1), **kw)
        led.deposit_records(times, c, sigmas, heights, logweights)
        return led

    @classmethod
    def from_kernels(cls, path, kT: float, *, barrier: float | None = None, max_steps: int = 0,
                     engine: Engine | None = None) -> "OPESLedger":
        fields, sets, data = _read_table(path)
        if len(fields) < 5 or fields[0] != "time" or fields[-2:] != ["height", "logweight"]:
            raise ValueError(f"{path}: FIELDS must read time <cvs> <sigmas> height logweight, got {fields}")
        if (len(fields) - 3) % 2:
            raise ValueError(f"{path}: FIELDS names {len(fields) - 3} CV and sigma columns, not a pair per CV")
        d = (len(fields) - 3) // 2
        names = fields[1:1 + d]
        if fields[1 + d:1 + 2 * d] != [f"sigma_{n}" for n in names]:
            raise ValueError(f"{path}: the sigma columns {fields[1 + d:1 + 2 * d]} do not match the CVs {names}")
        for key in ("biasfactor", "epsilon", "kernel_cutoff", "compression_threshold"):
            if key not in sets:
                raise ValueError(f"{path}: no '#! SET {key}' line")
        periods = np.zeros(d)
        for i, n in enumerate(names):
            if f"min_{n}" in sets or f"max_{n}" in sets:
                if not (f"min_{n}" in sets and f"max_{n}" in sets):
                    raise ValueError(f"{path}: {n} has only one of min_{n} / max_{n}")
                periods[i] = _plumed_number(sets[f"max_{n}"]) - _plumed_number(sets[f"min_{n}"])
                if not periods[i] > 0:
                    raise ValueError(f"{path}: {n} has a period of {periods[i]}")
        return cls.from_arrays(data[:, 0], data[:, 1:1 + d], data[:, 1 + d:1 + 2 * d], data[:, -2], data[:, -1], kT,
                               barrier=barrier, biasfactor=float(sets["biasfactor"]), epsilon=float(sets["epsilon"]),
                               cutoff=float(sets["kernel_cutoff"]), threshold=float(sets["compression_threshold"]),
                               periods=periods, names=names, max_steps=max_steps, engine=engine)

    # -- the device copy -----------------------------------------------------------
    def _engine(self) -> Engine:
        if self.engine is None:
            self.engine = get_engine()
        return self.engine

    def params(self, fixed_sigma: bool | None = None) -> np.ndarray:
        return Engine.opes_params(self.n_cv, self.kT, self.prefactor, self.epsilon, self.cutoff, self.threshold,
                                  self.fixed_sigma if fixed_sigma is None else fixed_sigma, self.periods,
                                  self.sigma0 if self.sigma0 is not None else np.ones(self.n_cv))

    def device_ledger(self) -> dict:
        """The device buffers (Engine.opes_state), their first len(self) versions current."""
        if self._dev is None:
            self._dev = self._engine().opes_state(self._capacity, self.n_cv)
        return self._dev

    def _reserve(self, more: int) -> None:
        need = self._n + int(more)
        if need <= self._capacity and self._dev is not None:
            return
        cap = self._capacity
        while cap < need:
            cap *= 2
        old, n = self._dev, self._n
        self._capacity = cap
        self._dev = self._engine().opes_state(cap, self.n_cv)
        times = np.zeros(cap)
        times[:n] = self._times[:n]
        self._times = times
        if old is not None:
            self._dev["state"].copy_from(old["state"])
            for key in ("live", "slot_version", "journal", "death", "per_deposit"):
                if n:       # the first n rows of each buffer are all that is current (K <= n live slots)
                    shape = (n,) + tuple(old[key].shape[1:])
                    self._dev[key].view(shape).copy_from(old[key].view(shape))

    # -- what it holds ---------------------------------------------------------------
    def __len__(self) -> int:
        return self._n

    @property
    def capacity(self) -> int:
        return self._capacity

    @property
    def times(self) -> np.ndarray:
        return self._times[:self._n].copy()

    def state(self) -> dict:
        """The scalar state, read back: count, live, W, W2, S, Z, status, cursor.  The host's own count follows the
        device's: deposits the device refused (see ``clear_status``) are dropped from ``len`` and ``times``."""
        s = self._engine().opes_read_state(self.device_ledger())
        if s["status"] and 0 <= s["count"] < self._n:
            self._n = s["count"]
        return s

    def clear_status(self) -> int:
        """After a refused deposit -- an on-line deposit at CVs that were not finite, which the host cannot see
        without waiting -- the device marks the ledger and consumes nothing more; every property raises until this is
        called.  It drops the refused deposit and all submitted after it from the host's count, clears the mark and
        returns the number of deposits the ledger holds.  Waits for the stream."""
        self.state()
        s = self._engine().opes_clear_status(self.device_ledger())
        self._n = min(self._n, s["count"])
        return self._n

    def _checked_state(self) -> dict:
        s = self.state()
        if s["status"]:
            bits = ((_lib.OPES_FULL, "the ledger is full"),
                    (_lib.OPES_BAD_RECORD, "a deposit is not finite or has no positive sigma / height"),
                    (_lib.OPES_BAD_STATE, "the state does not fit its buffers"))
            what = [name for bit, name in bits if s["status"] & bit]
            raise ValueError(f"the OPES ledger refused a deposit: {', '.join(what)} (status {s['status']}); it holds "
                             f"{s['count']} deposits and takes no more until clear_status()")
        return s

    @property
    def n_kernels(self) -> int:
        """The number of live (compressed) kernels."""
        return self._checked_state()["live"]

    @property
    def zed(self) -> float:
        """Z, the normalisation of the current state (1 before the first deposit)."""
        return self._checked_state()["Z"]

    @property
    def neff(self) -> float:
        """The effective sample size (1 + W)^2 / (1 + W2) of the current state."""
        s = self._checked_state()
        return (1.0 + s["W"]) ** 2 / (1.0 + s["W2"])

    def kernels(self) -> np.ndarray:
        """The live kernels [K, 2 d + 1] = centre, sigma, height, in slot order."""
        K = self._checked_state()["live"]
        return self.device_ledger()["live"].to_host()[:K].copy()

    def journal(self) -> dict:
        """The versions on the host: "kernels" [T, 2 d + 1], "death" [T] (T for a version that lives), "live_version"
        [K] (the version each live slot holds) and the per-deposit "W", "Z", "neff", "K" [T]."""
        s = self._checked_state()
        T, dev = self._n, self.device_ledger()
        pd = dev["per_deposit"].to_host()[:T]
        return {"kernels": dev["journal"].to_host()[:T].copy(),
                "death": np.minimum(dev["death"].to_host()[:T].astype(np.int64), T),
                "live_version": dev["slot_version"].to_host()[:s["live"]].astype(np.int64),
                "W": pd[:, 0].copy(), "Z": pd[:, 1].copy(), "neff": pd[:, 2].copy(), "K": pd[:, 3].astype(np.int64)}

    # -- deposition --------------------------------------------------------------------
    def _next_times(self, time, n: int) -> np.ndarray:
        if time is None:
            k = self._n
            last = self._times[k - 1] if k else -1.0
            gap = self._times[k - 1] - self._times[k - 2] if k > 1 else 1.0
            return last + gap * np.arange(1, n + 1)
        t = np.asarray(time, np.float64).reshape(-1)
        if t.size != n or not np.isfinite(t).all():
            raise ValueError(f"{t.size} times for {n} deposits")
        if (n > 1 and (np.diff(t) < 0).any()) or (self._n and n and t[0] < self._times[self._n - 1]):
            raise ValueError("the deposits' times must not decrease")
        return t

    def deposit_records(self, times, centers, sigmas, heights, logweights, *, max_steps: int | None = None) -> None:
        """Replays the deposits (time, centre [d], sigma [d], height, logweight), as a KERNELS file lists them."""
        d = self.n_cv
        c = np.asarray(centers, np.float64).reshape(-1, d)
        n = c.shape[0]
        s = np.asarray(sigmas, np.float64)
        s = np.broadcast_to(s, (n, d)) if s.ndim < 2 else s
        h = np.broadcast_to(np.asarray(heights, np.float64), (n,))
        lw = np.broadcast_to(np.asarray(logweights, np.float64), (n,))
        if s.shape != (n, d):
            raise ValueError(f"centers {c.shape} and sigmas {s.shape} disagree")
        if n and not (np.isfinite(c).all() and np.isfinite(s).all() and (s > 0).all() and np.isfinite(h).all()
                      and (h > 0).all() and np.isfinite(lw).all()):
            raise ValueError("centers, sigmas, heights and logweights must be finite, sigmas and heights positive")
        t = self._next_times(times, n)
        if n == 0:
            return
        self._reserve(n)
        eng = self._engine()
        rec = eng.to_device(np.ascontiguousarray(np.concatenate([c, s, h[:, None], lw[:, None]], axis=1)))
        eng.opes_deposit(self.device_ledger(), self.params(), rec,
                         max_steps=self.max_steps if max_steps is None else max_steps)
        eng.sync()          # the uploaded records are freed on return
        self._times[self._n:self._n + n] = t
        self._n += n

    def deposit(self, cv, time=None, *, records: DeviceArray | None = None, max_steps: int | None = None):
        """Deposits on line at the CVs `cv` [m, d] (m = 1: d numbers), host array or float64 device array with >= d
        columns: per row the height exp(V(s) / kT) and the width are formed on the device from the state so far.
        Returns the device array [m, 2 d + 2] of the records made (centre, sigma, height, logweight).  With device
        input and a given `records` buffer nothing is allocated, uploaded or waited for; a device row that is not
        finite is then refused on the device: it and every later deposit are dropped, ``bias`` keeps to the deposits
        made, and the next read of the state raises until ``clear_status``."""
        if self.sigma0 is None:
            raise ValueError("an on-line deposit needs the ledger's sigma0")
        d, eng = self.n_cv, self._engine()
        if isinstance(cv, DeviceArray):
            cvd = cv if len(cv.shape) == 2 else cv.view((1, cv.size))
            if cvd.dtype != np.float64 or cvd.shape[1] < d:
                raise ValueError(f"a device cv must be float64 with at least {d} columns")
        else:
            a = np.asarray(cv, np.float64).reshape(-1, d)
            if not np.isfinite(a).all():
                raise ValueError("cv must be finite")
            cvd = eng.to_device(a)
        m = cvd.shape[0]
        t = self._next_times(time, m)
        self._reserve(m)
        rec = records if records is not None else eng.empty((m, 2 * d + 2), np.float64)
        eng.opes_deposit(self.device_ledger(), self.params(), rec, m, cv=cvd,
                         max_steps=self.max_steps if max_steps is None else max_steps)
        if not isinstance(cv, DeviceArray):
            eng.sync()      # the uploaded CVs are freed on return
        self._times[self._n:self._n + m] = t
        self._n += m
        return rec

    # -- evaluation ----------------------------------------------------------------------
    def counts(self, times) -> np.ndarray:
        """Deposits a frame at each of `times` saw: those made strictly before it."""
        t = np.asarray(times, np.float64).reshape(-1)
        return np.searchsorted(self._times[:self._n], t, side="left").astype(np.int32)

    def bias(self, cv, times=None, gradient: bool = False, *, counts=None, live: bool = False, skip: bool = True,
             max_workgroups: int = 0):
        """V of the frames cv [n, d] (host array or float64 device array with >= d columns).  A frame sees the state
        after the deposits before times[n] (or after counts[n] deposits); with neither, the final state.  With
        gradient also dV/ds [n, d].  live=True evaluates against the live kernels, one wave per frame (the MD step).
        Host input gives host arrays, device input device arrays.  A frame with a non-finite CV is NaN."""
        if times is not None and counts is not None:
            raise ValueError("give times or counts, not both")
        if live and (times is not None or counts is not None):
            raise ValueError("the live kernels are the final state: no times or counts")
        eng = self._engine()
        host = not isinstance(cv, DeviceArray)
        if host:
            a = np.asarray(cv, np.float64)
            a = a.reshape(-1, self.n_cv) if a.ndim != 2 else a
            if a.shape[1] != self.n_cv:
                raise ValueError(f"cv must have {self.n_cv} columns, got {a.shape[1]}")
            if a.shape[0] == 0:
                return (np.zeros(0), np.zeros((0, self.n_cv))) if gradient else np.zeros(0)
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
        out = eng.opes_bias(cvd, self.device_ledger(), self.params(), None if live else self._n, counts=cd, live=live,
                            grad=gradient, skip=skip, max_workgroups=max_workgroups)
        if not host:
            if cd is not None and not isinstance(counts, DeviceArray):
                eng.sync()      # the uploaded counts are freed on return
            return out
        return (out[0].to_host(), out[1].to_host()) if gradient else out.to_host()


# ---- weights ---------------------------------------------------------------------------------------------------------
@dataclass
class OPESWeights:
    """weights sum to 1; log_weights = log(weights); ess is the Kish size 1 / sum w^2; bias [n] is V_t(s_t)."""
    weights: np.ndarray
    log_weights: np.ndarray
    ess: float
    bias: np.ndarray

    def __iter__(self):
        return iter((self.weights, self.log_weights, self.ess))


def opes_weights(ledger: OPESLedger, cv, times=None, kT: float | None = None) -> OPESWeights:
    """Weights that turn the frames of an OPES run into samples of the unbiased ensemble: w_n proportional to
    exp(V_t(s_n) / kT), V_t the bias the frame saw at its time (times=None: the final bias), normalised through a
    log-sum-exp.  kT defaults to the ledger's.  Unpacks as (weights, log_weights, ess)."""
    kT = ledger.kT if kT is None else float(kT)
    if not (np.isfinite(kT) and kT > 0):
        raise ValueError("kT must be positive and finite")
    V = ledger.bias(cv, times)
    w, lw, ess = _normalise(V / kT)
    return OPESWeights(w, lw, ess, V)


class OPESReweighter:
    """``OPESReweighter(kT=...).apply(dataset)`` writes ``dataset["frame_weights"]`` as ``Reweighter.apply`` does: one
    float64 array per split, jointly normalised (summed over all splits they give 1).

    Every split of ``dataset["splits"]`` carries ``"cv"`` [N_s, d], the CV columns the kernels were deposited in, and
    ``"time"`` [N_s] (without it the final bias is used).  The kernels are the ``ledger`` given here (an OPESLedger or
    the path of a KERNELS file), or a split's own ``"ledger"``.  ``kT`` in the bias's energy unit, or
    ``temperature_K`` (kJ / mol)."""

    def __init__(self, kT: float | None = None, *, temperature_K: float | None = None, ledger=None,
                 barrier: float | None = None) -> None:
        if (kT is None) == (temperature_K is None):
            raise ValueError("give exactly one of kT and temperature_K")
        value = float(kT) if kT is not None else BOLTZMANN_CONSTANT_KJ_PER_MOL * float(temperature_K)
        if not (np.isfinite(value) and value > 0):
            raise ValueError("kT / temperature_K must be positive and finite")
        self.kT, self.barrier = value, barrier
        self.ledger = self._ledger(ledger)
        self.result: Dict[str, Any] | None = None     # per split: the bias of the latest apply()

    def _ledger(self, ledger):
        if ledger is None or isinstance(ledger, OPESLedger):
            return ledger
        return read_kernels(ledger, self.kT, barrier=self.barrier)

    def apply(self, dataset: MutableMapping[str, Any]) -> Dict[str, np.ndarray]:
        splits = dataset.get("splits") if isinstance(dataset, Mapping) else None
        if not isinstance(splits, Mapping) or not splits:
            raise ValueError('OPESReweighter.apply needs dataset["splits"]')
        logs, sizes, self.result = [], {}, {}
        own: dict = {}              # a split's ledger given as a path is read once per path
        for name, split in splits.items():
            if not isinstance(split, Mapping) or split.get("cv") is None:
                raise ValueError(f"split '{name}' has no \"cv\"")
            ledger = split.get("ledger")
            if ledger is not None and not isinstance(ledger, OPESLedger):
                if str(ledger) not in own:
                    own[str(ledger)] = self._ledger(ledger)
                ledger = own[str(ledger)]
            if ledger is None:
                ledger = self.ledger
            if ledger is None:
                raise ValueError(f"split '{name}' has no \"ledger\" and the reweighter was built without one")
            cv = np.asarray(split["cv"], np.float64)
            cv = cv.reshape(-1, ledger.n_cv) if cv.ndim != 2 else cv
            times = split.get("time")
            if times is not None and np.asarray(times).size != cv.shape[0]:
                raise ValueError(f"split '{name}': time has {np.asarray(times).size} entries, cv {cv.shape[0]} rows")
            V = ledger.bias(cv, times)
            logs.append(V / self.kT)
            sizes[str(name)] = V.size
            self.result[str(name)] = {"bias": V}
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
