"""Device context and buffers: the thin host-side layer over the C ABI.

``Engine`` owns one ``msm_ctx`` (one HIP device, one stream).  ``DeviceArray``
is a typed view of hipMalloc'ed memory; arrays can also wrap foreign device
pointers (e.g. ``torch.Tensor.data_ptr()``) so collectives can run on them.
"""

from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Iterable, Sequence

import numpy as np

from . import _lib
from ._lib import check, lib

__all__ = ["Engine", "DeviceArray", "FeatureTable", "build_incidence", "get_engine", "segments_to_bounds"]


def _dtype_code(dtype: np.dtype) -> int:
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return _lib.MSM_F32
    if dtype == np.float64:
        return _lib.MSM_F64
    raise TypeError(f"feature matrices must be float32 or float64, got {dtype}")


def segments_to_bounds(
    segments: Iterable[tuple[int, int]] | None, n: int
) -> tuple[np.ndarray, np.ndarray]:
    """[(start, stop), ...] -> (starts, stops) int64, clipped like
    pmarlo.analysis.discretize._iter_segments (S/analysis/discretize.py:596-606)."""
    if segments is None:
        return np.zeros(1, np.int64), np.full(1, int(n), np.int64)
    starts, stops = [], []
    for start, stop in segments:
        a, b = max(0, int(start)), min(int(n), int(stop))
        if b > a:
            starts.append(a)
            stops.append(b)
    return np.asarray(starts, np.int64), np.asarray(stops, np.int64)


class DeviceArray:
    """A shaped, typed block of device memory."""

    __slots__ = ("engine", "ptr", "shape", "dtype", "_owned", "_base", "_alloc")

    def __init__(self, engine: "Engine", ptr: int, shape, dtype, owned: bool, alloc: int = 0):
        self.engine = engine
        self.ptr = int(ptr)
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self._owned = owned
        self._base = None
        self._alloc = int(alloc)      # bytes of the block behind an owned array (the engine's pool takes it back)

    @property
    def size(self) -> int:
        return int(np.prod(self.shape)) if self.shape else 1

    @property
    def nbytes(self) -> int:
        return self.size * self.dtype.itemsize

    def to_host(self) -> np.ndarray:
        out = np.empty(self.shape, self.dtype)
        if out.nbytes:
            check(lib.msm_memcpy_d2h(self.engine.handle, out.ctypes.data, self.ptr, out.nbytes),
                  self.engine.handle)
        return out

    def copy_from_host(self, arr: np.ndarray) -> "DeviceArray":
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        if arr.size != self.size:
            raise ValueError(f"size mismatch: device {self.shape} vs host {arr.shape}")
        if arr.nbytes:
            check(lib.msm_memcpy_h2d(self.engine.handle, self.ptr, arr.ctypes.data, arr.nbytes),
                  self.engine.handle)
        return self

    def copy_from(self, src: "DeviceArray") -> "DeviceArray":
        """Device-to-device copy of `src` (same byte count) into this array."""
        if src.nbytes != self.nbytes:
            raise ValueError(f"size mismatch: {self.nbytes} vs {src.nbytes} bytes")
        if self.nbytes:
            check(lib.msm_memcpy_d2d(self.engine.handle, self.ptr, src.ptr, self.nbytes), self.engine.handle)
        return self

    def zero_(self) -> "DeviceArray":
        check(lib.msm_memset(self.engine.handle, self.ptr, 0, self.nbytes), self.engine.handle)
        return self

    def fill_bytes_(self, byte: int) -> "DeviceArray":
        """Every byte set to `byte` (0xFF makes int32 / int64 entries -1)."""
        check(lib.msm_memset(self.engine.handle, self.ptr, int(byte) & 0xFF, self.nbytes), self.engine.handle)
        return self

    def view(self, shape, dtype=None, offset_elems: int = 0) -> "DeviceArray":
        dtype = self.dtype if dtype is None else np.dtype(dtype)
        v = DeviceArray(self.engine, self.ptr + offset_elems * self.dtype.itemsize, shape, dtype, False)
        v._base = self      # a view keeps the allocation it points into alive
        return v

    def free(self) -> None:
        if self._owned and self.ptr and self.engine.handle:
            self.engine._release(self.ptr, self._alloc)
        self.ptr = 0
        self._owned = False

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.free()
        except Exception:
            pass


class _Event:
    def __init__(self, engine: "Engine"):
        self.engine = engine
        h = C.c_void_p()
        check(lib.msm_event_create(engine.handle, C.byref(h)), engine.handle)
        self.handle = h

    def record(self) -> "_Event":
        check(lib.msm_event_record(self.engine.handle, self.handle), self.engine.handle)
        return self

    def elapsed_ms(self, stop: "_Event") -> float:
        ms = C.c_float()
        check(lib.msm_event_elapsed_ms(self.handle, stop.handle, C.byref(ms)), self.engine.handle)
        return float(ms.value)

    def __del__(self):  # pragma: no cover
        try:
            if self.handle:
                lib.msm_event_destroy(self.handle)
        except Exception:
            pass


class FeatureTable:
    """The device-resident feature list of `msm_featurize_spec` (include/msmhip.h has the record layout): `rec` int32
    [F, 8], `param` float32 [F], and what the host needs to know without reading them back.  `incidence(A)` is the
    atom -> (record, slot) incidence `msm_featurize_spec_vjp` walks, for frames of A atoms: built from the host copy
    of the records and uploaded on the first call with that A, then kept."""

    __slots__ = ("rec", "param", "width", "max_atom", "any_mic", "covers", "host_rec", "_inc")

    def __init__(self, rec: DeviceArray, param: DeviceArray, width: int, max_atom: int, any_mic: bool,
                 host_rec: np.ndarray | None = None):
        self.rec, self.param, self.width, self.max_atom, self.any_mic = rec, param, int(width), int(max_atom), any_mic
        self.host_rec = host_rec
        self._inc: dict[int, tuple[DeviceArray, DeviceArray]] = {}
        # every column in [0, width) is written by a record: the table can feed a network of `width` inputs
        self.covers = host_rec is not None and _written_columns(host_rec) == int(width)

    @property
    def n_features(self) -> int:
        return self.rec.shape[0]

    def incidence(self, n_atoms: int) -> tuple[DeviceArray, DeviceArray]:
        """(ptr int32 [A + 1], entries int32 [max(nnz, 1)]) on the device."""
        n_atoms = int(n_atoms)
        if n_atoms not in self._inc:
            if self.host_rec is None:
                raise ValueError("this FeatureTable was built without its host records: no incidence")
            ptr, inc = build_incidence(self.host_rec, n_atoms)
            eng = self.rec.engine
            self._inc[n_atoms] = (eng.to_device(ptr), eng.to_device(inc if inc.size else np.zeros(1, np.int32)))
        return self._inc[n_atoms]


def _written_columns(rec: np.ndarray) -> int:
    trig = (rec[:, 0] == _lib.FEAT_DIHEDRAL) & ((rec[:, 5] & _lib.FEAT_COSSIN) != 0)
    return int(np.unique(np.concatenate([rec[:, 6], rec[trig, 7]])).size)


def build_incidence(rec: np.ndarray, n_atoms: int) -> tuple[np.ndarray, np.ndarray]:
    """The atom -> (record, slot) incidence of a record table in CSR form: (ptr int32 [A + 1], entries int32 [nnz]);
    atom a's entries are entries[ptr[a]:ptr[a + 1]], each record * 4 + slot, in ascending order.  Contacts have no
    gradient and are not listed; neither is an atom index outside [0, A) (the forward writes NaN for its record)."""
    rec = np.asarray(rec)
    arity = np.select([rec[:, 0] == _lib.FEAT_DISTANCE, rec[:, 0] == _lib.FEAT_ANGLE, rec[:, 0] == _lib.FEAT_DIHEDRAL],
                      [2, 3, 4], 0)
    slots = np.arange(4)[None, :]
    listed = (slots < arity[:, None]) & (rec[:, 1:5] >= 0) & (rec[:, 1:5] < n_atoms)
    f, s = np.nonzero(listed)
    atom, code = rec[f, 1 + s].astype(np.int64), (4 * f + s).astype(np.int64)
    order = np.lexsort((code, atom))
    ptr = np.zeros(n_atoms + 1, np.int32)
    ptr[1:] = np.cumsum(np.bincount(atom, minlength=n_atoms))
    return ptr, code[order].astype(np.int32)


def _records(kind: int, atoms, flags, params, cols, cols2=None) -> tuple[np.ndarray, np.ndarray]:
    atoms = np.asarray(atoms, np.int64)
    m = atoms.shape[0]
    rec = np.zeros((m, 8), np.int64)
    rec[:, 0] = kind
    rec[:, 1:1 + atoms.shape[1]] = atoms
    rec[:, 5] = flags
    rec[:, 6] = cols
    if cols2 is not None:
        rec[:, 7] = cols2
    return rec, np.broadcast_to(np.asarray(params, np.float32), (m,))


def _finish_table(blocks) -> tuple[np.ndarray, np.ndarray, int]:
    """Concatenate per-kind record blocks (already in kind order, so waves rarely diverge), check atoms and columns."""
    rec = np.concatenate([b[0] for b in blocks]) if blocks else np.zeros((0, 8), np.int64)
    param = np.concatenate([b[1] for b in blocks]).astype(np.float32) if blocks else np.zeros((0,), np.float32)
    if rec.shape[0] == 0:
        raise ValueError("the feature table is empty")
    if rec[:, 1:5].min() < 0 or rec[:, 1:5].max() >= 2 ** 31:
        raise ValueError("atom indices must be non-negative int32")
    trig = (rec[:, 0] == _lib.FEAT_DIHEDRAL) & ((rec[:, 5] & _lib.FEAT_COSSIN) != 0)
    cols = np.concatenate([rec[:, 6], rec[trig, 7]])
    if cols.min() < 0 or cols.max() >= 2 ** 31 - 1:
        raise ValueError("output positions must be non-negative int32")
    if np.unique(cols).size != cols.size:
        raise ValueError("two features share an output position")
    return np.ascontiguousarray(rec, np.int32), np.ascontiguousarray(param), int(cols.max()) + 1


def _table_from_spec(spec) -> tuple[np.ndarray, np.ndarray, int]:
    if not hasattr(spec, "distance_pairs"):
        from .features.deeptica.ts_feature_extractor import canonicalize_feature_spec

        spec = canonicalize_feature_spec(spec)
    w = np.asarray(spec.feature_weights, np.float32)
    blocks = []
    for kind, atoms, pos, pbc in ((_lib.FEAT_DISTANCE, spec.distance_pairs, spec.distance_positions, spec.distance_pbc),
                                  (_lib.FEAT_ANGLE, spec.angle_triplets, spec.angle_positions, spec.angle_pbc),
                                  (_lib.FEAT_DIHEDRAL, spec.dihedral_quads, spec.dihedral_positions, spec.dihedral_pbc)):
        pos = np.asarray(pos, np.int64)
        if pos.size:
            if pos.min() < 0 or pos.max() >= w.size:
                raise ValueError(f"feature position outside [0, {w.size})")
            blocks.append(_records(kind, atoms, np.where(np.asarray(pbc, bool), _lib.FEAT_MIC, 0), w[pos], pos))
    return _finish_table(blocks)


def _table_from_indices(pairs, triplets, quads, dihedral_mode: int, contacts, rcut: float, periodic: bool):
    if dihedral_mode not in (0, 1, 2):
        raise ValueError("dihedral_mode must be 0, 1 or 2")
    flag = _lib.FEAT_MIC if periodic else 0

    def _idx(arr, width):
        return np.zeros((0, width), np.int64) if arr is None else np.asarray(arr, np.int64).reshape(-1, width)

    p, t, q, c = _idx(pairs, 2), _idx(triplets, 3), _idx(quads, 4), _idx(contacts, 2)
    P, Tn, Q = p.shape[0], t.shape[0], q.shape[0]
    blocks = []
    if P:
        blocks.append(_records(_lib.FEAT_DISTANCE, p, flag, 1.0, np.arange(P)))
    if Tn:
        blocks.append(_records(_lib.FEAT_ANGLE, t, flag, 1.0, P + np.arange(Tn)))
    if Q:
        k, base = np.arange(Q), P + Tn
        if dihedral_mode == 0:
            blocks.append(_records(_lib.FEAT_DIHEDRAL, q, flag, 1.0, base + k))
        elif dihedral_mode == 1:
            blocks.append(_records(_lib.FEAT_DIHEDRAL, q, flag | _lib.FEAT_COSSIN, 1.0, base + 2 * k, base + 2 * k + 1))
        else:
            blocks.append(_records(_lib.FEAT_DIHEDRAL, q, flag | _lib.FEAT_COSSIN, 1.0, base + k, base + Q + k))
    if c.shape[0]:
        if not rcut > 0.0:
            raise ValueError("rcut must be positive")
        base = P + Tn + (Q if dihedral_mode == 0 else 2 * Q)
        blocks.append(_records(_lib.FEAT_CONTACT, c, flag, rcut, base + np.arange(c.shape[0])))
    return _finish_table(blocks)


class Engine:
    """One HIP device + stream, and the kernels of the MSM path on it."""

    def __init__(self, device: int = 0, stream: int | None = None):
        h = C.c_void_p()
        status = lib.msm_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        if status != _lib.MSM_OK:
            raise _lib.MsmError(
                f"msm_ctx_create(device={device}) failed with status {status}: "
                "no usable HIP device (pmarlo_amd has no CPU fallback)"
            )
        self.handle = h
        self.device = int(device)
        # freed blocks wait here for the next request of their size: hipMalloc / hipFree synchronise the device and
        # cost 0.1-1 ms each, which was a third of an operator call (22 frees = 10 ms in discretize_dataset at 1 M
        # frames).  All work of an engine is ordered on its one stream, so a block can be handed out again at once.
        self._pool: dict[int, list[int]] = {}
        self._pool_bytes = 0
        self._pool_cap = int(os.environ.get("MSM_POOL_BYTES", str(16 << 30)))
        self.last_pathway_launches = 0      # launches the latest reactive_pathways call took

    # -- plumbing -----------------------------------------------------------
    @staticmethod
    def _block_size(nbytes: int) -> int:
        nbytes = max(int(nbytes), 1)
        step = 512 if nbytes < (1 << 20) else (1 << 20)
        return -(-nbytes // step) * step

    def _release(self, ptr: int, alloc: int) -> None:
        if alloc and self._pool_bytes + alloc <= self._pool_cap:
            self._pool.setdefault(alloc, []).append(ptr)
            self._pool_bytes += alloc
        else:
            lib.msm_free(self.handle, ptr)

    def empty_cache(self) -> None:
        """Give the pooled blocks back to the driver."""
        for blocks in self._pool.values():
            for ptr in blocks:
                lib.msm_free(self.handle, ptr)
        self._pool.clear()
        self._pool_bytes = 0

    def close(self) -> None:
        if self.handle:
            self.empty_cache()
            lib.msm_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        arch = C.create_string_buffer(64)
        ncu = C.c_int()
        mem = C.c_size_t()
        check(lib.msm_device_info(self.handle, arch, 64, C.byref(ncu), C.byref(mem)), self.handle)
        return {"arch": arch.value.decode(), "n_cu": int(ncu.value), "total_mem": int(mem.value)}

    def empty(self, shape, dtype) -> DeviceArray:
        dtype = np.dtype(dtype)
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        nbytes = int(np.prod(shape)) * dtype.itemsize if shape else dtype.itemsize
        size = self._block_size(nbytes)
        blocks = self._pool.get(size)
        if blocks:
            self._pool_bytes -= size
            return DeviceArray(self, blocks.pop(), shape, dtype, True, size)
        p = C.c_void_p()
        status = lib.msm_malloc(self.handle, size, C.byref(p))
        if status != _lib.MSM_OK and self._pool_bytes:
            self.empty_cache()          # out of memory with blocks parked in the pool: hand them back and try again
            status = lib.msm_malloc(self.handle, size, C.byref(p))
        check(status, self.handle)
        return DeviceArray(self, p.value, shape, dtype, True, size)

    def zeros(self, shape, dtype) -> DeviceArray:
        return self.empty(shape, dtype).zero_()

    def to_device(self, arr: np.ndarray, dtype=None) -> DeviceArray:
        arr = np.ascontiguousarray(arr, dtype=dtype)
        return self.empty(arr.shape, arr.dtype).copy_from_host(arr)

    def wrap(self, ptr: int, shape, dtype) -> DeviceArray:
        """View foreign device memory (torch tensor data_ptr, etc.)."""
        return DeviceArray(self, ptr, shape, dtype, False)

    def sync(self) -> None:
        check(lib.msm_sync(self.handle), self.handle)

    def event(self) -> _Event:
        return _Event(self)

    def graph_begin(self) -> None:
        check(lib.msm_graph_begin(self.handle), self.handle)

    def graph_end(self):
        g = C.c_void_p()
        check(lib.msm_graph_end(self.handle, C.byref(g)), self.handle)
        return g

    def graph_launch(self, g) -> None:
        check(lib.msm_graph_launch(self.handle, g), self.handle)

    def graph_destroy(self, g) -> None:
        lib.msm_graph_destroy(g)

    # -- featurizers -----------------------------------------------------------
    def featurize_rg(self, xyz: DeviceArray) -> DeviceArray:
        """Radius of gyration (unit masses) per frame: float32 [n]."""
        n, A, _ = xyz.shape
        out = self.empty((n,), np.float32)
        check(lib.msm_featurize_rg(self.handle, xyz.ptr, n, A, out.ptr, 1, 0), self.handle)
        return out

    def featurize_contacts(self, xyz: DeviceArray, pairs, rcut: float) -> DeviceArray:
        """1.0 where the pair distance is <= rcut (nm): float32 [n, P]."""
        n, A, _ = xyz.shape
        p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        if p.size and (p.min() < 0 or p.max() >= A):
            raise ValueError(f"atom index out of range [0, {A})")
        pd_ = self.to_device(p)
        out = self.empty((n, p.shape[0]), np.float32)
        check(lib.msm_featurize_contacts(self.handle, xyz.ptr, n, A, pd_.ptr, p.shape[0], float(rcut), out.ptr,
                                         p.shape[0], 0), self.handle)
        self.sync()
        return out

    def featurize_sasa(self, xyz: DeviceArray, radii, points) -> DeviceArray:
        """Shrake-Rupley accessible area per atom: float32 [n, A] (nm^2).  `radii` float32 [A] already include the
        probe radius, `points` float32 [P, 3] are the unit sphere points."""
        n, A, _ = xyz.shape
        r = self.to_device(np.ascontiguousarray(radii, np.float32).reshape(A))
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        p = self.to_device(pts)
        out = self.empty((n, A), np.float32)
        check(lib.msm_featurize_sasa(self.handle, xyz.ptr, n, A, r.ptr, p.ptr, pts.shape[0], out.ptr), self.handle)
        return out

    def hbond_presence(self, xyz: DeviceArray, triplets, dist_cutoff: float, angle_cutoff: float) -> np.ndarray:
        """Frames in which each (donor, hydrogen, acceptor) triplet meets the Baker-Hubbard criteria: int64 [Tn]."""
        n, A, _ = xyz.shape
        tr = np.ascontiguousarray(triplets, np.int32).reshape(-1, 3)
        if tr.size and (tr.min() < 0 or tr.max() >= A):
            raise ValueError(f"atom index out of range [0, {A})")
        if tr.shape[0] == 0:
            return np.zeros((0,), np.int64)
        td = self.to_device(tr)
        counts = self.empty((tr.shape[0],), np.uint64)
        check(lib.msm_hbond_presence(self.handle, xyz.ptr, n, A, td.ptr, tr.shape[0], float(dist_cutoff),
                                     float(angle_cutoff), counts.ptr), self.handle)
        return counts.to_host().astype(np.int64)

    def dssp(self, xyz: DeviceArray, backbone, chain, proline) -> np.ndarray:
        """Kabsch-Sander codes per frame and protein residue: uint8 [n, R] (0 loop, 1 H, 2 B, 3 E, 4 G, 5 I, 6 T, 7 S).
        A backbone row that holds a -1 is a residue without a full backbone: never bonded, a chain break, code 0."""
        n, A, _ = xyz.shape
        bb = np.ascontiguousarray(backbone, np.int32).reshape(-1, 4)
        R = bb.shape[0]
        if R == 0 or n == 0:
            return np.zeros((n, R), np.uint8)
        if bb.min() < -1 or bb.max() >= A:
            raise ValueError(f"atom index out of range [0, {A}) (-1: atom missing)")
        bd = self.to_device(bb)
        cd = self.to_device(np.ascontiguousarray(chain, np.int32).reshape(R))
        pd_ = self.to_device(np.ascontiguousarray(proline, np.uint8).reshape(R))
        codes = self.empty((n, R), np.uint8)
        check(lib.msm_dssp(self.handle, xyz.ptr, n, A, bd.ptr, cd.ptr, pd_.ptr, R, codes.ptr), self.handle)
        return codes.to_host()

    def featurize(self, xyz: DeviceArray, *, pairs=None, triplets=None, quads=None, dihedral_mode: int = 0,
                  out: DeviceArray | None = None) -> DeviceArray:
        """xyz float32 [n, A, 3] -> float32 [n, F]: distance columns, then angle columns, then
        dihedral columns (mode 0 radians, 1 interleaved cos/sin, 2 cos block | sin block)."""
        if xyz.dtype != np.float32 or len(xyz.shape) != 3 or xyz.shape[2] != 3:
            raise ValueError("xyz must be float32 with shape (n_frames, n_atoms, 3)")
        n, A, _ = xyz.shape

        def _idx(arr, width):
            if arr is None:
                return None, 0
            a = np.ascontiguousarray(arr, np.int32).reshape(-1, width)
            if a.size and (a.min() < 0 or a.max() >= A):
                raise ValueError(f"atom index out of range [0, {A})")
            return (self.to_device(a) if a.size else None), a.shape[0]

        dp, P = _idx(pairs, 2)
        dt, Tn = _idx(triplets, 3)
        dq, Q = _idx(quads, 4)
        width = P + Tn + (Q if dihedral_mode == 0 else 2 * Q)
        out = out if out is not None else self.empty((n, width), np.float32)
        ld = out.shape[1]
        if P:
            check(lib.msm_featurize_distances(self.handle, xyz.ptr, n, A, dp.ptr, P, out.ptr, ld, 0), self.handle)
        if Tn:
            check(lib.msm_featurize_angles(self.handle, xyz.ptr, n, A, dt.ptr, Tn, out.ptr, ld, P), self.handle)
        if Q:
            check(lib.msm_featurize_dihedrals(self.handle, xyz.ptr, n, A, dq.ptr, Q, int(dihedral_mode), out.ptr, ld,
                                              P + Tn), self.handle)
        self.sync()  # index tables are freed on return
        return out

    def featurize_distances_into(self, xyz: DeviceArray, pairs: DeviceArray, out: DeviceArray, col0: int = 0) -> DeviceArray:
        """Pair distances with a device-resident int32 [P, 2] index table into columns col0.. of `out` (float32
        [n, ld]); no upload, no sync: the form a timed step uses."""
        n, A, _ = xyz.shape
        check(lib.msm_featurize_distances(self.handle, xyz.ptr, n, A, pairs.ptr, pairs.shape[0], out.ptr, out.shape[1],
                                          int(col0)), self.handle)
        return out

    # -- periodic boundaries ---------------------------------------------------
    def box_from_cell(self, cell) -> DeviceArray:
        """Cell parameters float64 [n, 6] (a, b, c in nm, alpha, beta, gamma in degrees; host array or DeviceArray)
        -> box vectors float32 [n, 9] on the device, rows a, b, c in mdtraj's convention."""
        if not isinstance(cell, DeviceArray):
            c = np.ascontiguousarray(cell, np.float64)
            if c.ndim == 1:
                c = c[None]
            if c.ndim != 2 or c.shape[1] != 6:
                raise ValueError(f"cell must have shape (n, 6), got {c.shape}")
            cell = self.to_device(c)
        elif cell.dtype != np.float64 or len(cell.shape) != 2 or cell.shape[1] != 6:
            raise ValueError("a device cell must be float64 with shape (n, 6)")
        n = cell.shape[0]
        box = self.empty((n, 9), np.float32)
        check(lib.msm_box_from_cell(self.handle, cell.ptr, n, box.ptr), self.handle)
        return box

    def feature_table(self, spec=None, *, pairs=None, triplets=None, quads=None, dihedral_mode: int = 0,
                      contacts=None, rcut: float = 0.0, periodic: bool = True) -> FeatureTable:
        """Upload the feature table of `msm_featurize_spec`.  Either `spec` (a feature specification in any form
        `canonicalize_feature_spec` accepts, or its result: entries land at their position, scaled by their weight,
        flagged by their ``pbc``), or index tables in the column layout of `featurize` (distances, angles, dihedrals
        in `dihedral_mode`) followed by one 0/1 column per `contacts` pair at `rcut`, all flagged when `periodic`."""
        if spec is not None:
            rec, param, width = _table_from_spec(spec)
        else:
            rec, param, width = _table_from_indices(pairs, triplets, quads, int(dihedral_mode), contacts, float(rcut),
                                                    bool(periodic))
        return FeatureTable(self.to_device(rec), self.to_device(param), width, int(rec[:, 1:5].max(initial=-1)),
                            bool((rec[:, 5] & _lib.FEAT_MIC).any()), host_rec=rec)

    def _box_arg(self, box, n: int):
        """(device box or None, n_box) from None, a host (3, 3) / (n, 3, 3) / (n_box, 9) array (checked: finite,
        determinant > 0) or a device float32 [n_box, 9] / [n_box, 3, 3] array (taken as it is)."""
        if box is None:
            return None, 0
        if isinstance(box, DeviceArray):
            if box.dtype != np.float32 or box.size % 9 or len(box.shape) > 3:
                raise ValueError("a device box must be float32 with shape (n_box, 9) or (n_box, 3, 3)")
            n_box, dev = box.size // 9, box
        else:
            b = np.asarray(box, np.float64)
            if b.size == 0 or b.size % 9 or b.shape[-1] not in (3, 9) or (b.shape[-1] == 3 and b.shape[-2:] != (3, 3)):
                raise ValueError(f"box must have shape (3, 3), (n, 3, 3) or (n, 9), got {b.shape}")
            b = b.reshape(-1, 3, 3)
            if not np.isfinite(b).all():
                raise ValueError("box has non-finite entries")
            if not (np.linalg.det(b) > 0.0).all():
                raise ValueError("box vectors must have a positive determinant (singular or left-handed box)")
            n_box, dev = b.shape[0], None
        if n_box != 1 and n_box != n:
            raise ValueError(f"need one box or one per frame: got {n_box} boxes for {n} frames")
        return (dev if dev is not None else self.to_device(b.reshape(-1, 9), np.float32)), n_box

    def featurize_spec(self, xyz: DeviceArray, spec_or_table, box=None, mic: str = "round", out: DeviceArray | None = None,
                       col0: int = 0) -> DeviceArray:
        """A mixed feature list in one launch, with the minimum-image convention where an entry asks for it.
        xyz float32 [n, A, 3] -> columns col0.. of `out` (float32 [n, ld]; default a new [n, width] array).
        `spec_or_table`: a `FeatureTable` (see `feature_table`) or a specification, which is uploaded for this call.
        `box`: None (nothing wraps), one box or one per frame; `mic`: "round", the reference extractor's rule, or
        "search", mdtraj's (the shortest of the 27 neighbouring images).  With a device-resident table and box (or
        none) nothing is uploaded and nothing waits: the form a timed step uses."""
        if xyz.dtype != np.float32 or len(xyz.shape) != 3 or xyz.shape[2] != 3:
            raise ValueError("xyz must be float32 with shape (n_frames, n_atoms, 3)")
        modes = {"round": _lib.MIC_ROUND, "search": _lib.MIC_SEARCH}
        if mic not in modes:
            raise ValueError(f"mic must be 'round' or 'search', got {mic!r}")
        n, A, _ = xyz.shape
        uploaded = not isinstance(spec_or_table, FeatureTable)
        table = self.feature_table(spec_or_table) if uploaded else spec_or_table
        if table.max_atom >= A:
            raise ValueError(f"atom index {table.max_atom} out of range [0, {A})")
        dbox, n_box = self._box_arg(box, n)
        uploaded = uploaded or (dbox is not None and dbox is not box)
        if not table.any_mic:
            dbox, n_box = None, 0
        out = out if out is not None else self.empty((n, int(col0) + table.width), np.float32)
        if out.dtype != np.float32 or len(out.shape) != 2 or out.shape[0] != n:
            raise ValueError(f"out must be float32 with shape ({n}, ld)")
        if col0 < 0 or col0 + table.width > out.shape[1]:
            raise ValueError(f"output columns [{col0}, {col0 + table.width}) exceed the {out.shape[1]} columns of out")
        check(lib.msm_featurize_spec(self.handle, xyz.ptr, n, A, dbox.ptr if dbox is not None else None, n_box,
                                     table.rec.ptr, table.param.ptr, table.n_features, table.width, modes[mic],
                                     out.ptr, out.shape[1], int(col0)), self.handle)
        if uploaded:
            self.sync()  # the uploaded table / box are freed on return
        return out

    _MIC = {"round": _lib.MIC_ROUND, "search": _lib.MIC_SEARCH}

    def featurize_spec_vjp(self, xyz: DeviceArray, table: FeatureTable, gfeat: DeviceArray, box=None,
                           mic: str = "round", sign: float = 1.0, col0: int = 0,
                           out: DeviceArray | None = None) -> DeviceArray:
        """The adjoint of `featurize_spec` (msm_featurize_spec_vjp): float64 [n, A, 3] with
        out[t, a] = sign * sum_f gfeat[t, col0 + col(f)] * d feature_f / d x_a, for the table, box and `mic` the forward
        was run with.  gfeat: float64 [n, ld], ld >= col0 + table.width.  No upload beyond the table's incidence on its
        first use and a host box; no host synchronisation otherwise."""
        if xyz.dtype != np.float32 or len(xyz.shape) != 3 or xyz.shape[2] != 3:
            raise ValueError("xyz must be float32 with shape (n_frames, n_atoms, 3)")
        if mic not in self._MIC:
            raise ValueError(f"mic must be 'round' or 'search', got {mic!r}")
        if not isinstance(table, FeatureTable):
            raise TypeError("featurize_spec_vjp needs a FeatureTable (Engine.feature_table)")
        n, A, _ = xyz.shape
        if table.max_atom >= A:
            raise ValueError(f"atom index {table.max_atom} out of range [0, {A})")
        if gfeat.dtype != np.float64 or len(gfeat.shape) != 2 or gfeat.shape[0] != n:
            raise ValueError(f"gfeat must be float64 with shape ({n}, ld)")
        if col0 < 0 or col0 + table.width > gfeat.shape[1]:
            raise ValueError(f"gradient columns [{col0}, {col0 + table.width}) exceed the {gfeat.shape[1]} columns of gfeat")
        dbox, n_box = self._box_arg(box, n)
        uploaded = dbox is not None and dbox is not box
        if not table.any_mic:
            dbox, n_box = None, 0
        out = out if out is not None else self.empty((n, A, 3), np.float64)
        if out.dtype != np.float64 or out.size != n * A * 3:
            raise ValueError(f"out must be float64 with shape ({n}, {A}, 3)")
        ptr, inc = table.incidence(A)
        check(lib.msm_featurize_spec_vjp(self.handle, xyz.ptr, n, A, dbox.ptr if dbox is not None else None, n_box,
                                         table.rec.ptr, table.param.ptr, table.n_features, table.width, self._MIC[mic],
                                         gfeat.ptr, gfeat.shape[1], int(col0), ptr.ptr, inc.ptr, float(sign), out.ptr),
              self.handle)
        if uploaded:
            self.sync()  # the uploaded box is freed on return
        return out

    def _mlp_args(self, spec):
        widths = np.ascontiguousarray(spec.widths, np.int32)
        params, mean, scale = self._mlp_on_device(spec)
        flags = (int(bool(spec.ln_in)), int(bool(spec.ln_hidden)), int(bool(spec.head_activation)))
        return widths, params, mean, scale, flags

    def mlp_vjp(self, x: DeviceArray, spec, gout: DeviceArray | None = None, strength: float = 1.0, *,
                want_energy: bool = True, want_outputs: bool = True, ld: int | None = None,
                work: DeviceArray | None = None) -> dict:
        """Forward pass of the network `spec` and its vector-Jacobian product with respect to the inputs x [n, F]
        (msm_mlp_vjp): `gx` float64 [n, F] = dE/dx, where dE/dy is `gout` (float64 [n, >= n_out]) or, without it,
        2 strength y, the gradient of E = strength sum y^2.  Also `energy` [n] (that E) and `outputs` [n, n_out],
        bit-identical to `mlp_forward`, and `work`, the workspace, to hand back through ``work``."""
        n, F = x.shape
        widths, params, mean, scale, flags = self._mlp_args(spec)
        n_linear, d = len(widths) - 1, int(widths[-1])
        if gout is not None and (gout.dtype != np.float64 or len(gout.shape) != 2 or gout.shape[0] != n):
            raise ValueError(f"gout must be float64 with shape ({n}, ld)")
        need = int(lib.msm_mlp_vjp_workspace(n, n_linear, widths.ctypes.data, *flags))
        if work is None or work.nbytes < max(need, 8):
            work = self.empty((max(need, 8) // 8,), np.float64)
        energy = self.empty((n,), np.float64) if want_energy else None
        out = self.empty((n, d), np.float64) if want_outputs else None
        gx = self.empty((n, F), np.float64)
        check(lib.msm_mlp_vjp(self.handle, x.ptr, _dtype_code(x.dtype), n, F, int(F if ld is None else ld),
                              mean.ptr if mean is not None else None, scale.ptr if scale is not None else None,
                              n_linear, widths.ctypes.data, int(spec.activation), *flags, params.ptr, params.size,
                              gout.ptr if gout is not None else None, gout.shape[1] if gout is not None else 0,
                              float(strength), energy.ptr if want_energy else None,
                              out.ptr if want_outputs else None, d, gx.ptr, F, work.ptr, work.nbytes), self.handle)
        res = {"gx": gx, "work": work}
        if want_energy:
            res["energy"] = energy
        if want_outputs:
            res["outputs"] = out
        return res

    BIAS_WORK_BUDGET = 256 << 20     # bytes of workspace one msm_bias_energy_forces call may use

    def bias_energy_forces(self, xyz: DeviceArray, table: FeatureTable, spec, strength: float, box=None,
                           mic: str = "round", *, want_cv: bool = True, energy: DeviceArray | None = None,
                           cv: DeviceArray | None = None, force: DeviceArray | None = None,
                           work: DeviceArray | None = None, chunk: int | None = None) -> dict:
        """Bias energy, collective variables and forces of the frames xyz float32 [n, A, 3]
        (msm_bias_energy_forces): `energy` float64 [n] = strength sum cv^2, `cv` float64 [n, n_out] (the raw outputs
        of the network `spec`), `force` float64 [n, A, 3] = -dE/dx, all on the device.  `table`: the FeatureTable whose
        columns are the network's inputs; `box`: None, one box or one per frame (a device box is used as it is).
        The workspace of a call grows with n (features, their gradient, the network's tape: msm_bias_workspace), so n
        is cut into chunks of frames whose workspace stays under BIAS_WORK_BUDGET = 256 MiB -- about 380 000 frames
        for a 23 -> 32 -> 16 -> 3 network without LayerNorms, 210 000 with both -- each chunk three launches; `chunk` overrides the chunk length.  With device-resident
        inputs and preallocated `energy`, `cv`, `force`, `work` nothing is allocated, uploaded or waited for:
        the form an MD step, or a graph capture, uses."""
        if xyz.dtype != np.float32 or len(xyz.shape) != 3 or xyz.shape[2] != 3:
            raise ValueError("xyz must be float32 with shape (n_frames, n_atoms, 3)")
        if mic not in self._MIC:
            raise ValueError(f"mic must be 'round' or 'search', got {mic!r}")
        if not isinstance(table, FeatureTable):
            raise TypeError("bias_energy_forces needs a FeatureTable (Engine.feature_table)")
        n, A, _ = xyz.shape
        if table.max_atom >= A:
            raise RuntimeError(f"expected at least {table.max_atom + 1} atoms, received {A}")
        widths, params, mean, scale, flags = self._mlp_args(spec)
        n_linear, F, d = len(widths) - 1, int(widths[0]), int(widths[-1])
        if table.width != F or not table.covers:
            raise RuntimeError(f"feature extractor returned {table.width} features but scaler expects {F}"
                               if table.width != F else "a column of the feature table is written by no record")
        dbox, n_box = self._box_arg(box, n)
        uploaded = dbox is not None and dbox is not box
        if not table.any_mic:
            dbox, n_box = None, 0
        per_frame = int(lib.msm_bias_workspace(1, F, n_linear, widths.ctypes.data, *flags))
        if per_frame == 0:
            spec.check_envelope()
            raise NotImplementedError("the network lies outside msm_mlp_forward's envelope")
        step = max(1, int(chunk) if chunk else self.BIAS_WORK_BUDGET // (per_frame + 16))
        step = min(step, max(n, 1))
        need = int(lib.msm_bias_workspace(step, F, n_linear, widths.ctypes.data, *flags))
        if work is None or work.nbytes < need:
            work = self.empty((need // 8 + 1,), np.float64)
        energy = energy if energy is not None else self.empty((n,), np.float64)
        cv = cv if cv is not None else (self.empty((n, d), np.float64) if want_cv else None)
        force = force if force is not None else self.empty((n, A, 3), np.float64)
        if energy.dtype != np.float64 or energy.size != n or force.dtype != np.float64 or force.size != n * A * 3:
            raise ValueError(f"energy must be float64 [{n}], force float64 [{n}, {A}, 3]")
        if cv is not None and (cv.dtype != np.float64 or len(cv.shape) != 2 or cv.shape[0] != n or cv.shape[1] < d):
            raise ValueError(f"cv must be float64 with shape ({n}, >= {d})")
        ptr, inc = table.incidence(A)
        ldo = cv.shape[1] if cv is not None else d
        for t0 in range(0, n, step):
            m = min(step, n - t0)
            bptr = None if dbox is None else dbox.ptr + (0 if n_box == 1 else t0 * 36)
            check(lib.msm_bias_energy_forces(
                self.handle, xyz.ptr + t0 * A * 12, m, A, bptr, 0 if dbox is None else (1 if n_box == 1 else m),
                table.rec.ptr, table.param.ptr, table.n_features, ptr.ptr, inc.ptr, self._MIC[mic],
                mean.ptr if mean is not None else None, scale.ptr if scale is not None else None, n_linear,
                widths.ctypes.data, int(spec.activation), *flags, params.ptr, params.size, float(strength), work.ptr,
                work.nbytes, energy.ptr + t0 * 8, cv.ptr + t0 * ldo * 8 if cv is not None else None, ldo,
                force.ptr + t0 * A * 24), self.handle)
        if uploaded:
            self.sync()  # the uploaded box is freed on return
        return {"energy": energy, "cv": cv, "force": force, "work": work}

    def _superpose_args(self, xyz: DeviceArray, sel, ref):
        if xyz.dtype != np.float32 or len(xyz.shape) != 3 or xyz.shape[2] != 3:
            raise ValueError("xyz must be float32 with shape (n_frames, n_atoms, 3)")
        A = xyz.shape[1]
        s = np.ascontiguousarray(sel, np.int32).reshape(-1)
        if s.size and (s.min() < 0 or s.max() >= A):
            raise ValueError(f"atom index out of range [0, {A})")
        r = np.ascontiguousarray(ref, np.float32)
        if r.shape != (s.size, 3):
            raise ValueError(f"ref must have shape ({s.size}, 3): the reference positions of the selected atoms, "
                             f"got {r.shape}")
        # S = 0 travels on to the library, whose message names the rule; an empty upload is not possible
        return (self.to_device(s) if s.size else None), (self.to_device(r) if s.size else None), int(s.size)

    def superpose(self, xyz: DeviceArray, sel, ref, *, out: DeviceArray | None = None, want_rmsd: bool = True):
        """Rigid-body fit of every frame of xyz (float32 [n, A, 3]) onto `ref` (float32 [S, 3], the reference
        positions of the atoms `sel`): (aligned float32 [n, A, 3], rmsd float32 [n] or None).  The rotation is
        proper (det +1) and is applied to all atoms; `out` may be xyz itself (in place)."""
        sd, rd, S = self._superpose_args(xyz, sel, ref)
        n, A, _ = xyz.shape
        if out is None:
            out = self.empty((n, A, 3), np.float32)
        elif out.dtype != np.float32 or tuple(out.shape) != (n, A, 3):
            raise ValueError(f"out must be float32 with shape {(n, A, 3)}")
        rmsd = self.empty((n,), np.float32) if want_rmsd else None
        check(lib.msm_superpose(self.handle, xyz.ptr, n, A, sd.ptr if sd else None, S, rd.ptr if rd else None, out.ptr,
                                rmsd.ptr if rmsd is not None else None), self.handle)
        self.sync()  # index and reference tables are freed on return
        return out, rmsd

    def rmsd(self, xyz: DeviceArray, sel, ref) -> DeviceArray:
        """RMSD of every frame to `ref` after the optimal proper rotation, float32 [n]; reads the selected atoms
        only."""
        sd, rd, S = self._superpose_args(xyz, sel, ref)
        n, A, _ = xyz.shape
        rmsd = self.empty((n,), np.float32)
        check(lib.msm_superpose(self.handle, xyz.ptr, n, A, sd.ptr if sd else None, S, rd.ptr if rd else None, None,
                                rmsd.ptr), self.handle)
        self.sync()
        return rmsd

    # -- transition counts ----------------------------------------------------
    @staticmethod
    def _seg_ptrs(starts: np.ndarray, stops: np.ndarray):
        starts = np.ascontiguousarray(starts, np.int64)
        stops = np.ascontiguousarray(stops, np.int64)
        if starts.shape != stops.shape:
            raise ValueError("segment starts/stops differ in length")
        return starts, stops

    def count_transitions(self, labels: DeviceArray, k: int, lag: int, *, starts=None, stops=None,
                          stride: int = 1, out: DeviceArray | None = None,
                          pairs: DeviceArray | None = None) -> tuple[DeviceArray, DeviceArray]:
        n = labels.size
        if starts is None:
            starts, stops = segments_to_bounds(None, n)
        starts, stops = self._seg_ptrs(starts, stops)
        out = out if out is not None else self.empty((k, k), np.int64)
        pairs = pairs if pairs is not None else self.empty((1,), np.int64)
        check(lib.msm_count_transitions(self.handle, labels.ptr, n, starts.ctypes.data, stops.ctypes.data,
                                        len(starts), int(lag), int(stride), int(k), out.ptr, pairs.ptr),
              self.handle)
        return out, pairs

    def count_transitions_normalised(self, labels: DeviceArray, k: int, lag: int, T: DeviceArray, rowsum: DeviceArray,
                                     diag_mass: DeviceArray, *, starts=None, stops=None, stride: int = 1,
                                     out: DeviceArray | None = None, pairs: DeviceArray | None = None):
        """count_transitions + row_normalise_into with the same bits, in the counting launch itself where the dense
        two-pass counting runs (msm_count_transitions_normalised) -> (counts, pairs)."""
        n = labels.size
        if starts is None:
            starts, stops = segments_to_bounds(None, n)
        starts, stops = self._seg_ptrs(starts, stops)
        out = out if out is not None else self.empty((k, k), np.int64)
        pairs = pairs if pairs is not None else self.empty((1,), np.int64)
        check(lib.msm_count_transitions_normalised(self.handle, labels.ptr, n, starts.ctypes.data, stops.ctypes.data,
                                                   len(starts), int(lag), int(stride), int(k), out.ptr, pairs.ptr, T.ptr,
                                                   rowsum.ptr, diag_mass.ptr), self.handle)
        return out, pairs

    def count_transitions_weighted(self, labels: DeviceArray, weights: DeviceArray, k: int, lag: int, *,
                                   starts=None, stops=None, stride: int = 1,
                                   out: DeviceArray | None = None, pairs: DeviceArray | None = None):
        n = labels.size
        if weights.size != n or weights.dtype != np.float64:
            raise ValueError("weights must be float64 with one entry per label")
        if starts is None:
            starts, stops = segments_to_bounds(None, n)
        starts, stops = self._seg_ptrs(starts, stops)
        out = out if out is not None else self.empty((k, k), np.float64)
        pairs = pairs if pairs is not None else self.empty((1,), np.int64)
        check(lib.msm_count_transitions_weighted(self.handle, labels.ptr, weights.ptr, n, starts.ctypes.data,
                                                 stops.ctypes.data, len(starts), int(lag), int(stride),
                                                 int(k), out.ptr, pairs.ptr), self.handle)
        return out, pairs

    def count_transitions_lagscan(self, labels: DeviceArray, k: int, lags: Sequence[int], *, starts=None,
                                  stops=None, out: DeviceArray | None = None,
                                  pairs: DeviceArray | None = None):
        n = labels.size
        lags_arr = np.ascontiguousarray(lags, np.int32)
        if starts is None:
            starts, stops = segments_to_bounds(None, n)
        starts, stops = self._seg_ptrs(starts, stops)
        L = len(lags_arr)
        out = out if out is not None else self.empty((L, k, k), np.int64)
        pairs = pairs if pairs is not None else self.empty((L,), np.int64)
        check(lib.msm_count_transitions_lagscan(self.handle, labels.ptr, n, starts.ctypes.data,
                                                stops.ctypes.data, len(starts), lags_arr.ctypes.data, L,
                                                int(k), out.ptr, pairs.ptr), self.handle)
        return out, pairs

    def count_plan(self, k: int, total_pairs: int, weighted: bool = False) -> dict:
        """The kernels a count of `total_pairs` pair positions over k states would run on this engine now
        (msm_count_transitions_plan, include/msmhip.h): {"path": "bucket" | "privatised" | "global" | "none", ...}
        with the path's launch shape.  Launches nothing."""
        import ctypes

        out = (ctypes.c_int64 * 8)()
        check(lib.msm_count_transitions_plan(self.handle, int(k), int(total_pairs), int(bool(weighted)), out), self.handle)
        v = [int(x) for x in out]
        if v[0] == _lib.COUNT_PATH_BUCKET:
            return {"path": "bucket", "R": v[1], "buckets": v[2], "chunk": v[3], "chunks": v[4], "copies": v[5],
                    "fuses_normalisation": bool(v[6])}
        if v[0] == _lib.COUNT_PATH_PRIVATISED:
            return {"path": "privatised", "rows": v[1], "row_blocks": v[2], "chunks": v[3], "pairs_per_chunk": v[4],
                    "lds_bytes": v[5]}
        if v[0] == _lib.COUNT_PATH_GLOBAL:
            return {"path": "global", "chunks": v[3]}
        return {"path": "none"}

    def effective_counts(self, labels: DeviceArray, k: int, lag: int, *, starts=None, stops=None, average: str = "row",
                         mact: float = 1.0, blocks_per_launch: int | None = None):
        """Effective count matrix at `lag` (msm_effective_counts, include/msmhip.h) -> (Ceff f64 [k, k], statistical
        inefficiencies f64 [k, k] (0 where C = 0), sliding counts C int64 [k, k], truncation lags int32 [k, k]).
        Segments must be ascending and disjoint; every segment is one trajectory.  average: "row" (deeptime's
        estimator), "all" or "none".  blocks_per_launch: lag blocks of EFF_LAG_BLOCK lags a launch may advance a cell
        by (None: the library's default); the result does not depend on it.  The number of inefficiency launches of
        the last call is kept in `last_effective_launches`."""
        import ctypes

        modes = {"row": _lib.EFF_AVERAGE_ROW, "all": _lib.EFF_AVERAGE_ALL, "none": _lib.EFF_AVERAGE_NONE}
        if average not in modes:
            raise ValueError(f"average must be one of {sorted(modes)}, got {average!r}")
        if labels.dtype != np.int32:
            raise TypeError("labels must be int32")
        n, k = labels.size, int(k)
        if k < 1:
            raise ValueError(f"k must be >= 1 (got {k})")
        if starts is None:
            starts, stops = segments_to_bounds(None, n)
        starts, stops = self._seg_ptrs(starts, stops)
        ceff, si = self.empty((k, k), np.float64), self.empty((k, k), np.float64)
        counts, trunc = self.empty((k, k), np.int64), self.empty((k, k), np.int32)
        work = self.empty((max(int(lib.msm_effective_counts_work_bytes(n, k, len(starts))), 1),), np.uint8)
        launches = ctypes.c_int64(0)
        check(lib.msm_effective_counts(self.handle, labels.ptr, n, starts.ctypes.data, stops.ctypes.data, len(starts),
                                       int(lag), k, modes[average], float(mact),
                                       0 if blocks_per_launch is None else int(blocks_per_launch), work.ptr, work.nbytes,
                                       ceff.ptr, si.ptr, counts.ptr, trunc.ptr, ctypes.byref(launches)), self.handle)
        self.sync()  # the workspace is freed on return
        self.last_effective_launches = int(launches.value)
        return ceff, si, counts, trunc

    # -- MBAR (csrc/mbar.hip) -------------------------------------------------------------------
    @staticmethod
    def _mbar_matrix(u: DeviceArray, n: int | None, what: str) -> tuple[int, int, int]:
        if len(u.shape) != 2:
            raise ValueError(f"{what} must be a [states, ld] matrix, got shape {u.shape}")
        rows, ld = u.shape
        n = ld if n is None else int(n)
        if not 1 <= n <= ld:
            raise ValueError(f"{what}: need 1 <= n <= ld (n={n}, ld={ld})")
        return rows, n, ld

    @staticmethod
    def _mbar_raise(status: int, what: str) -> None:
        if status & _lib.MBAR_BAD_INPUT:
            raise ValueError(f"{what}: the reduced potentials hold NaN or -inf")
        if status & _lib.MBAR_BAD_FRAME:
            raise ValueError(f"{what}: a frame is forbidden (+inf) in every state, its mixture denominator is zero")

    def mbar_plan(self, K: int, N: int, dtype=np.float64, max_workgroups: int = 0) -> dict:
        """What mbar_pass would launch (msm_mbar_plan, include/msmhip.h).  Launches nothing."""
        out = (C.c_int64 * 4)()
        check(lib.msm_mbar_plan(self.handle, int(K), int(N), _dtype_code(dtype), int(max_workgroups), out), self.handle)
        return {"frames_per_trip": int(out[0]), "grid": int(out[1]), "lds_bytes": int(out[2]), "gram_tiles": int(out[3])}

    def mbar_pass(self, u: DeviceArray, f: DeviceArray, lnN: DeviceArray, *, n: int | None = None,
                  want_gram: bool = True, want_logden: bool = True, max_workgroups: int = 0, check_status: bool = True) -> dict:
        """One MBAR pass at free energies f over u [K, ld] f32 / f64 (msm_mbar_pass, include/msmhip.h); the first `n`
        columns of every row are frames (default: all ld).  Returns {"s": f64 [K], "obj": f64 [1], "G": f64 [K, K] or
        None, "logden": f64 [n] or None, "status": int}, device arrays.  NaN / -inf in u and a frame forbidden in
        every state raise ValueError (check_status=False: only reported in "status")."""
        K, n, ld = self._mbar_matrix(u, n, "u")
        if f.dtype != np.float64 or lnN.dtype != np.float64 or f.size != K or lnN.size != K:
            raise ValueError(f"f and lnN must be float64 of {K} entries")
        s, obj = self.empty((K,), np.float64), self.empty((1,), np.float64)
        G = self.empty((K, K), np.float64) if want_gram and K <= _lib.MBAR_MAX_K else None
        logden = self.empty((n,), np.float64) if want_logden else None
        status = self.zeros((1,), np.int32)
        check(lib.msm_mbar_pass(self.handle, u.ptr, _dtype_code(u.dtype), K, n, ld, f.ptr, lnN.ptr, int(bool(want_gram)),
                                int(max_workgroups), logden.ptr if logden is not None else None, s.ptr,
                                G.ptr if G is not None else None, obj.ptr, status.ptr), self.handle)
        st = int(status.to_host()[0])
        if check_status:
            self._mbar_raise(st, "mbar_pass")
        return {"s": s, "obj": obj, "G": G, "logden": logden, "status": st}

    def mbar_state_means(self, u: DeviceArray, offsets, *, n: int | None = None) -> DeviceArray:
        """Mean of row k of u over its own frames [offsets[k], offsets[k+1]) (msm_mbar_state_means) -> f64 [K]."""
        K, n, ld = self._mbar_matrix(u, n, "u")
        off = np.ascontiguousarray(offsets, np.int64)
        if off.shape != (K + 1,):
            raise ValueError(f"offsets must have {K + 1} entries")
        mean = self.empty((K,), np.float64)
        check(lib.msm_mbar_state_means(self.handle, u.ptr, _dtype_code(u.dtype), K, n, ld, off.ctypes.data, mean.ptr),
              self.handle)
        return mean

    def mbar_newton_step(self, s: DeviceArray, G: DeviceArray, Nk: DeviceArray) -> np.ndarray:
        """Solves the reduced Newton system H x = g of the MBAR objective on the device (msm_mbar_newton_system, then
        msm_solve_f64) -> x, host f64 [K - 1].  Raises RuntimeError when H is singular."""
        K = s.size
        H, g = self.empty((K - 1, K - 1), np.float64), self.empty((K - 1,), np.float64)
        check(lib.msm_mbar_newton_system(self.handle, K, s.ptr, G.ptr, Nk.ptr, H.ptr, g.ptr), self.handle)
        info = self.solve(H, g)
        if info:
            raise _lib.MsmError(f"mbar: the Newton system is singular at column {info - 1}")
        return g.to_host()

    def mbar_weights(self, ut: DeviceArray, logden: DeviceArray, *, check_status: bool = True):
        """Target-state free energies, normalised weights and Kish sample sizes from the stored log denominators
        (msm_mbar_weights, include/msmhip.h): ut [T, ld] f32 / f64, logden f64 [N], N <= ld ->
        (f_t f64 [T], w f64 [T, N], ess f64 [T]), device arrays."""
        if logden.dtype != np.float64:
            raise TypeError("logden must be float64")
        T, n, ld = self._mbar_matrix(ut, logden.size, "ut")
        ft, w, ess = self.empty((T,), np.float64), self.empty((T, n), np.float64), self.empty((T,), np.float64)
        status = self.zeros((1,), np.int32)
        check(lib.msm_mbar_weights(self.handle, ut.ptr, _dtype_code(ut.dtype), T, n, ld, logden.ptr, ft.ptr, w.ptr,
                                   ess.ptr, status.ptr), self.handle)
        if check_status:
            self._mbar_raise(int(status.to_host()[0]), "mbar_weights")
        return ft, w, ess

    def mbar_reduced_potentials(self, energy: DeviceArray, beta, bias: DeviceArray | None = None) -> DeviceArray:
        """u[k, n] = beta[k] * (energy[n] + bias[k, n]) -> f64 [K, N] (msm_mbar_reduced_potentials)."""
        beta = np.ascontiguousarray(beta, np.float64).reshape(-1)
        K, n = beta.size, energy.size
        if energy.dtype != np.float64 or (bias is not None and (bias.dtype != np.float64 or bias.shape != (K, n))):
            raise ValueError(f"energy must be float64 [N] and bias float64 [{K}, N]")
        u = self.empty((K, n), np.float64)
        check(lib.msm_mbar_reduced_potentials(self.handle, energy.ptr, bias.ptr if bias is not None else None, n,
                                              self.to_device(beta).ptr, K, n, n, u.ptr), self.handle)
        self.sync()  # beta's device copy is freed on return
        return u

    # -- TRAM (csrc/tram.hip) -------------------------------------------------------------------
    @staticmethod
    def _tram_units(offsets) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        if off.size < 2 or off[0] != 0 or (np.diff(off) <= 0).any():
            raise ValueError("offsets must start at 0 and give every Markov state at least one frame")
        per_state = -(-np.diff(off) // _lib.TRAM_SEGMENT)
        unit_ptr = np.concatenate([[0], np.cumsum(per_state)]).astype(np.int64)
        return off, unit_ptr, np.repeat(np.arange(off.size - 1, dtype=np.int32), per_state)

    def tram_tables(self, offsets) -> dict:
        """The device tables that name the work units of tram_pass for frames grouped by Markov state, state i
        owning [offsets[i], offsets[i+1]): built once per problem (msm_tram_pass, include/msmhip.h)."""
        off, unit_ptr, unit_state = self._tram_units(offsets)
        return {"m": off.size - 1, "n": int(off[-1]), "units": int(unit_ptr[-1]), "host_offsets": off,
                "offsets": self.to_device(off), "unit_ptr": self.to_device(unit_ptr),
                "unit_state": self.to_device(unit_state)}

    def tram_plan(self, K: int, offsets, max_workgroups: int = 0) -> dict:
        """What tram_pass would launch (msm_tram_plan, include/msmhip.h).  Launches nothing."""
        off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        out = (C.c_int64 * 5)()
        check(lib.msm_tram_plan(self.handle, int(K), off.size - 1, off.ctypes.data, int(max_workgroups), out), self.handle)
        return {"segment": int(out[0]), "units": int(out[1]), "grid": int(out[2]), "lds_bytes": int(out[3]),
                "rows_grid": int(out[4])}

    @staticmethod
    def _tram_km(S: DeviceArray, *tables: DeviceArray) -> tuple[int, int]:
        if S.dtype != np.float64 or len(S.shape) != 3 or S.shape[1] != S.shape[2]:
            raise ValueError(f"S must be float64 [K, m, m], got {S.dtype} {S.shape}")
        K, m = S.shape[0], S.shape[1]
        for t in tables:
            if t.dtype != np.float64 or t.shape != (K, m):
                raise ValueError(f"the per-pair tables must be float64 [{K}, {m}], got {t.dtype} {t.shape}")
        return K, m

    def tram_rows(self, S: DeviceArray, g: DeviceArray, f: DeviceArray, N: DeviceArray, col: DeviceArray,
                  mode: str) -> tuple[DeviceArray, DeviceArray]:
        """Step 1 (mode "multipliers" -> v, ln v + f) or step 2 (mode "counts" -> R, ln R + f) of a TRAM iteration
        (msm_tram_rows, include/msmhip.h), f64 [K, m] device arrays."""
        modes = {"multipliers": _lib.TRAM_ROWS_MULTIPLIERS, "counts": _lib.TRAM_ROWS_COUNTS}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)}, got {mode!r}")
        K, m = self._tram_km(S, g, f, N, col)
        out, lnout = self.empty((K, m), np.float64), self.empty((K, m), np.float64)
        check(lib.msm_tram_rows(self.handle, K, m, S.ptr, g.ptr, f.ptr, N.ptr, col.ptr, modes[mode], out.ptr, lnout.ptr),
              self.handle)
        return out, lnout

    def tram_pass(self, u: DeviceArray, tables: dict, tab: DeviceArray, *, want_logden: bool = True,
                  max_workgroups: int = 0, check_status: bool = True) -> dict:
        """Step 3 over u [K, ld] f32 / f64, frames grouped by Markov state as `tables` (tram_tables) says, at the
        table tab = ln R + f, f64 [K, m] (msm_tram_pass, include/msmhip.h).  Returns {"s": f64 [K, m], "logden": f64
        [N] or None, "status": int}.  NaN / -inf in u and a frame without a finite term raise ValueError
        (check_status=False: only reported in "status")."""
        K, n, ld = self._mbar_matrix(u, tables["n"], "u")
        m = tables["m"]
        if tab.dtype != np.float64 or tab.shape != (K, m):
            raise ValueError(f"tab must be float64 [{K}, {m}]")
        s = self.empty((K, m), np.float64)
        logden = self.empty((n,), np.float64) if want_logden else None
        status = self.zeros((1,), np.int32)
        check(lib.msm_tram_pass(self.handle, u.ptr, _dtype_code(u.dtype), K, m, n, ld, tables["offsets"].ptr,
                                tables["unit_ptr"].ptr, tables["unit_state"].ptr, tables["units"], tab.ptr,
                                int(max_workgroups), logden.ptr if logden is not None else None, s.ptr, status.ptr),
              self.handle)
        st = int(status.to_host()[0])
        if check_status:
            self._mbar_raise(st, "tram_pass")
        return {"s": s, "logden": logden, "status": st}

    def tram_update(self, N: DeviceArray, tab: DeviceArray, s: DeviceArray, v: DeviceArray,
                    f: DeviceArray) -> tuple[DeviceArray, DeviceArray]:
        """Steps 4 and 5: f is updated in place -> (g = ln v + f f64 [K, m], err f64 [1]) (msm_tram_update)."""
        K, m = f.shape
        g, err = self.empty((K, m), np.float64), self.empty((1,), np.float64)
        check(lib.msm_tram_update(self.handle, K, m, N.ptr, tab.ptr, s.ptr, v.ptr, f.ptr, g.ptr, err.ptr), self.handle)
        return g, err

    def tram_solve(self, u: DeviceArray, tables: dict, S: DeviceArray, N: DeviceArray, col: DeviceArray,
                   f: DeviceArray, v: DeviceArray, *, tol: float = 1e-10, maxiter: int = 100_000,
                   check_every: int = 16, max_workgroups: int = 0) -> dict:
        """Iterates the TRAM equations from (f, v), updated in place, until err <= tol (msm_tram_iterations,
        include/msmhip.h).  `check_every` iterations are enqueued back to back with no host synchronisation; then
        the one err word and the status word are read.  Stops at the first checked iteration with err <= tol;
        MsmError (NOCONV) at `maxiter`.  Returns {"n_iterations", "err", "logden": d_n of the last pass, f64 [N]}."""
        K, m = self._tram_km(S, N, col, f, v)
        Ku, n, ld = self._mbar_matrix(u, tables["n"], "u")
        if Ku != K or tables["m"] != m:
            raise ValueError(f"u has {Ku} rows and the tables {tables['m']} Markov states; S is [{K}, {m}, {m}]")
        check_every, maxiter = int(check_every), int(maxiter)
        if check_every < 1 or maxiter < 1:
            raise ValueError("check_every and maxiter must be >= 1")
        work = self.empty((5, K, m), np.float64)
        logden, err_d = self.empty((n,), np.float64), self.empty((1,), np.float64)
        status = self.zeros((1,), np.int32)
        it, err = 0, float("inf")
        while it < maxiter:
            block = min(check_every, maxiter - it)
            check(lib.msm_tram_iterations(self.handle, u.ptr, _dtype_code(u.dtype), K, m, n, ld, tables["offsets"].ptr,
                                          tables["unit_ptr"].ptr, tables["unit_state"].ptr, tables["units"], S.ptr,
                                          N.ptr, col.ptr, f.ptr, v.ptr, work.ptr, block, int(max_workgroups),
                                          logden.ptr, err_d.ptr, status.ptr), self.handle)
            it += block
            err = float(err_d.to_host()[0])
            self._mbar_raise(int(status.to_host()[0]), "tram_solve")
            if err <= tol:
                return {"n_iterations": it, "err": err, "logden": logden}
            if not np.isfinite(err):
                raise _lib.MsmError(f"tram: the iteration left the finite numbers after {it} iterations (err = {err})")
        raise _lib.MsmError(f"tram: err {err:.3e} > tol {tol:.1e} after {it} iterations (MSM_ERR_NOCONV)")

    def tram_transition_matrices(self, S: DeviceArray, N: DeviceArray, f: DeviceArray, v: DeviceArray,
                                 k: int | None = None) -> DeviceArray:
        """The reversible transition matrix of ensemble k, f64 [m, m], or of all of them, f64 [K, m, m], at (f, v)
        (msm_tram_transition_matrices, include/msmhip.h); rows and columns of inactive states are zero."""
        K, m = self._tram_km(S, N, f, v)
        if k is not None and not 0 <= int(k) < K:
            raise ValueError(f"k must be in [0, {K})")
        P = self.empty((K, m, m) if k is None else (m, m), np.float64)
        rowsum = self.empty((K, m), np.float64)
        check(lib.msm_tram_transition_matrices(self.handle, K, m, S.ptr, N.ptr, f.ptr, v.ptr, -1 if k is None else int(k),
                                               rowsum.ptr, P.ptr), self.handle)
        self.sync()  # the row sums are freed on return
        return P

    # -- hidden Markov models (csrc/hmm.hip) ------------------------------------------------------
    def hmm_plan(self, n: int, n_chunks: int, n_sequences: int, max_workgroups: int = 0) -> dict:
        """What an E-step would launch (msm_hmm_plan, include/msmhip.h).  Launches nothing."""
        out = (C.c_int64 * 8)()
        check(lib.msm_hmm_plan(self.handle, int(n), int(n_chunks), int(n_sequences), int(max_workgroups), out),
              self.handle)
        return {"chunk": int(out[0]), "padded_n": int(out[1]), "n_chunks": int(out[2]), "grid": int(out[3]),
                "boundary_grid": int(out[4]), "product_lds_bytes": int(out[5]), "pass_lds_bytes": int(out[6]),
                "emission_lds_bytes": int(out[7])}

    def hmm_tables(self, labels: DeviceArray, k: int, sequences, *, n: int | None = None) -> dict:
        """The device tables of an HMM fit over the first `n` entries of labels int32: `sequences` int64 [Q, 3] of
        (start, stride, length) (hmm.lag_observations builds them), the chunk tables of msm_hmm_estep, and the
        frames grouped by symbol with the (symbol, 256 member frames) units of msm_hmm_emissions.  Built once per
        fit; one read-back of the k + 1 group offsets."""
        if labels.dtype != np.int32:
            raise TypeError("labels must be int32")
        N = labels.size if n is None else int(n)
        if not 1 <= N <= labels.size:
            raise ValueError(f"n must be in [1, {labels.size}]")
        seq = np.ascontiguousarray(sequences, np.int64).reshape(-1, 3)
        if seq.shape[0] < 1 or (seq[:, 2] < 1).any():
            raise ValueError("need at least one sequence, every one with at least one observation")
        per_seq = -(-(seq[:, 2] - 1) // _lib.HMM_CHUNK)
        chunk_ptr = np.concatenate([[0], np.cumsum(per_seq)]).astype(np.int64)
        chunk_seq = np.repeat(np.arange(seq.shape[0], dtype=np.int32), per_seq)
        offsets, members = self.empty((int(k) + 1,), np.int64), self.empty((N,), np.int32)
        check(lib.msm_group_by_label(self.handle, labels.ptr, N, int(k), offsets.ptr, members.ptr), self.handle)
        per_symbol = -(-np.diff(offsets.to_host()) // 256)
        unit_ptr = np.concatenate([[0], np.cumsum(per_symbol)]).astype(np.int64)
        unit_state = np.repeat(np.arange(int(k), dtype=np.int32), per_symbol)
        return {"labels": labels, "N": N, "k": int(k), "Q": seq.shape[0], "n_chunks": int(chunk_ptr[-1]),
                "units": int(unit_ptr[-1]), "host_sequences": seq, "sequences": self.to_device(seq),
                "chunk_ptr": self.to_device(chunk_ptr), "chunk_seq": self.to_device(chunk_seq) if chunk_seq.size else None,
                "offsets": offsets, "members": members, "unit_ptr": self.to_device(unit_ptr),
                "unit_state": self.to_device(unit_state) if unit_state.size else None}

    @staticmethod
    def _hmm_model(t: dict, A: DeviceArray, B: DeviceArray, p0: DeviceArray) -> int:
        n = A.shape[0]
        for name, arr, shape in (("A", A, (n, n)), ("B", B, (n, t["k"])), ("p0", p0, (n,))):
            if arr.dtype != np.float64 or arr.shape != shape:
                raise ValueError(f"{name} must be float64 {list(shape)}, got {arr.dtype} {arr.shape}")
        return n

    def _hmm_work(self, t: dict, n: int) -> DeviceArray:
        nbytes = int(lib.msm_hmm_workspace_bytes(int(n), t["n_chunks"], t["Q"], t["units"]))
        if nbytes == 0:
            check(lib.msm_hmm_plan(self.handle, int(n), t["n_chunks"], t["Q"], 0, (C.c_int64 * 8)()), self.handle)
        return self.empty((nbytes,), np.uint8)

    @staticmethod
    def _opt(arr: DeviceArray | None):
        return arr.ptr if arr is not None else None

    def hmm_estep(self, tables: dict, A: DeviceArray, B: DeviceArray, p0: DeviceArray, *, max_workgroups: int = 0,
                  want_emissions: bool = True) -> dict:
        """One scaled forward-backward pass over every sequence (msm_hmm_estep, include/msmhip.h) and the emission
        sums (msm_hmm_emissions).  Returns device arrays "gamma" f64 [N, n], "C" f64 [n, n], "gamma0" f64 [n], "logL"
        f64 [Q], "E" f64 [n, k] (or None), and the host values "total" = sum of logL and "status" (HMM_* bits)."""
        t = tables
        n = self._hmm_model(t, A, B, p0)
        work = self._hmm_work(t, n)
        gamma = self.zeros((t["N"], n), np.float64)
        Cm, g0, logL = self.empty((n, n), np.float64), self.empty((n,), np.float64), self.empty((t["Q"],), np.float64)
        total, status = self.empty((1,), np.float64), self.zeros((1,), np.int32)
        check(lib.msm_hmm_estep(self.handle, t["labels"].ptr, t["N"], t["k"], n, t["sequences"].ptr, t["Q"],
                                t["chunk_ptr"].ptr, self._opt(t["chunk_seq"]), t["n_chunks"], A.ptr, B.ptr, p0.ptr,
                                int(max_workgroups), work.ptr, gamma.ptr, Cm.ptr, g0.ptr, logL.ptr, total.ptr,
                                status.ptr), self.handle)
        E = None
        if want_emissions:
            E = self.empty((n, t["k"]), np.float64)
            part = self.empty((max(t["units"], 1), n), np.float64)
            check(lib.msm_hmm_emissions(self.handle, gamma.ptr, t["N"], n, t["k"], t["offsets"].ptr, t["members"].ptr,
                                        t["unit_ptr"].ptr, self._opt(t["unit_state"]), t["units"], int(max_workgroups),
                                        part.ptr, E.ptr), self.handle)
        out = {"gamma": gamma, "C": Cm, "gamma0": g0, "logL": logL, "E": E, "total": float(total.to_host()[0]),
               "status": int(status.to_host()[0])}
        self.sync()  # the workspace is freed on return
        return out

    def hmm_viterbi(self, tables: dict, A: DeviceArray, B: DeviceArray, p0: DeviceArray, *,
                    max_workgroups: int = 0) -> dict:
        """The most probable hidden path of every sequence (msm_hmm_viterbi, include/msmhip.h).  Returns "path" int32
        [N] on the device, in frame order (-1: a frame in no sequence, or in one of probability 0), "logp" f64 [Q] on
        the device, and the host value "status" (HMM_* bits)."""
        t = tables
        n = self._hmm_model(t, A, B, p0)
        work = self.empty((int(lib.msm_hmm_viterbi_workspace_bytes(n, t["k"], t["n_chunks"], t["Q"])) or 1,), np.uint8)
        path, logp = self.empty((t["N"],), np.int32), self.empty((t["Q"],), np.float64)
        status = self.zeros((1,), np.int32)
        check(lib.msm_hmm_viterbi(self.handle, t["labels"].ptr, t["N"], t["k"], n, t["sequences"].ptr, t["Q"],
                                  t["chunk_ptr"].ptr, self._opt(t["chunk_seq"]), t["n_chunks"], A.ptr, B.ptr, p0.ptr,
                                  int(max_workgroups), work.ptr, path.ptr, logp.ptr, status.ptr), self.handle)
        return {"path": path, "logp": logp, "status": int(status.to_host()[0])}   # synchronises: the workspace is free

    def hmm_mstep(self, C_: DeviceArray, E: DeviceArray, gamma0: DeviceArray, n_sequences: int, A: DeviceArray,
                  B: DeviceArray, p0: DeviceArray, *, reversible: bool = True, stationary: bool = False,
                  maxerr: float = 1e-8, maxiter: int = 100_000) -> dict:
        """The M-step (msm_hmm_mstep, include/msmhip.h): A, B and p0 are updated in place.  Returns {"pi": the
        stationary vector of the new A, f64 [n] on the device, "status": HMM_* bits}."""
        n, k = E.shape
        pi, status = self.empty((n,), np.float64), self.zeros((1,), np.int32)
        check(lib.msm_hmm_mstep(self.handle, n, k, int(n_sequences), C_.ptr, E.ptr, gamma0.ptr, int(bool(reversible)),
                                int(bool(stationary)), int(maxiter), float(maxerr), A.ptr, B.ptr, p0.ptr, pi.ptr,
                                status.ptr), self.handle)
        return {"pi": pi, "status": int(status.to_host()[0])}

    def hmm_iterations(self, tables: dict, A: DeviceArray, B: DeviceArray, p0: DeviceArray, n_iterations: int, *,
                       state: dict | None = None, reversible: bool = True, stationary: bool = False,
                       maxerr: float = 1e-8, maxiter: int = 100_000, max_workgroups: int = 0) -> dict:
        """`n_iterations` EM iterations enqueued back to back (msm_hmm_iterations, include/msmhip.h); A, B and p0 are
        updated in place.  Returns the state dict (pass it back in to reuse its buffers): device arrays "pi", "gamma",
        "C", "E", "gamma0", "logL", and the host values "history" (sum of logL at the start of every iteration)
        and "status"."""
        t = tables
        n = self._hmm_model(t, A, B, p0)
        n_iterations = int(n_iterations)
        if n_iterations < 1:
            raise ValueError("n_iterations must be >= 1")
        s = state
        if s is None or s.get("n") != n or s["hist_d"].size < n_iterations:
            s = {"n": n, "work": self._hmm_work(t, n), "gamma": self.zeros((t["N"], n), np.float64),
                 "pi": self.empty((n,), np.float64), "C": self.empty((n, n), np.float64),
                 "E": self.empty((n, t["k"]), np.float64), "gamma0": self.empty((n,), np.float64),
                 "logL": self.empty((t["Q"],), np.float64), "hist_d": self.empty((n_iterations,), np.float64),
                 "status_d": self.zeros((1,), np.int32)}
        check(lib.msm_hmm_iterations(self.handle, t["labels"].ptr, t["N"], t["k"], n, t["sequences"].ptr, t["Q"],
                                     t["chunk_ptr"].ptr, self._opt(t["chunk_seq"]), t["n_chunks"], t["offsets"].ptr,
                                     t["members"].ptr, t["unit_ptr"].ptr, self._opt(t["unit_state"]), t["units"],
                                     int(bool(reversible)), int(bool(stationary)), int(maxiter), float(maxerr),
                                     n_iterations, int(max_workgroups), s["work"].ptr, A.ptr, B.ptr, p0.ptr,
                                     s["pi"].ptr, s["gamma"].ptr, s["C"].ptr, s["E"].ptr, s["gamma0"].ptr,
                                     s["logL"].ptr, s["hist_d"].ptr, s["status_d"].ptr), self.handle)
        s["history"] = s["hist_d"].to_host()[:n_iterations].copy()
        s["status"] = int(s["status_d"].to_host()[0])
        return s

    def hmm_fit(self, tables: dict, A: DeviceArray, B: DeviceArray, p0: DeviceArray, *, reversible: bool = True,
                stationary: bool = False, accuracy: float = 1e-3, maxit: int = 1000, check_every: int = 8,
                max_workgroups: int = 0) -> dict:
        """Baum-Welch from (A, B, p0), updated in place: `check_every` iterations are enqueued with no host
        synchronisation, then the likelihood history is read; stops after the first interval that holds an iteration
        whose likelihood moved by less than `accuracy`, or at `maxit`.  Returns the state of hmm_iterations with "likelihoods" (one per
        iteration run), "n_iterations" and "converged"; the parameters are those after the last iteration run, the
        arrays "gamma", "C", "E" those of its E-step."""
        check_every, maxit = max(1, int(check_every)), max(1, int(maxit))
        hist: list[float] = []
        state, converged = None, False
        while len(hist) < maxit and not converged:
            block = min(check_every, maxit - len(hist))
            state = self.hmm_iterations(tables, A, B, p0, block, state=state, reversible=reversible,
                                        stationary=stationary, max_workgroups=max_workgroups)
            for v in state["history"]:
                hist.append(float(v))
            if state["status"] & (_lib.HMM_BAD_SYMBOL | _lib.HMM_BAD_TABLE):
                raise ValueError(f"hmm_fit: the labels or the sequence tables are invalid (status {state['status']})")
            if not np.isfinite(hist[-1]):
                raise _lib.MsmError("hmm_fit: a sequence has probability 0 under the model (logL = -inf)")
            d = np.abs(np.diff(hist))
            converged = bool(d.size and (d < accuracy).any())
        state["likelihoods"] = np.asarray(hist)
        state["n_iterations"] = len(hist)
        state["converged"] = converged
        return state

    # -- metadynamics (csrc/metad.hip) -----------------------------------------------------------
    @staticmethod
    def _metad_shape(hills: DeviceArray, n_hills: int | None, periods, kernel: str, max_d: int):
        """(H, d, periods array or None, kernel code) of a packed ledger hills f64 [capacity, 2 d + 1]."""
        if hills.dtype != np.float64 or len(hills.shape) != 2 or hills.shape[1] < 3 or hills.shape[1] % 2 == 0:
            raise ValueError(f"hills must be float64 with shape (capacity, 2 d + 1), got {hills.shape} {hills.dtype}")
        d = (hills.shape[1] - 1) // 2
        if d > max_d:
            raise ValueError(f"{d} collective variables, at most {max_d} are supported here")
        H = hills.shape[0] if n_hills is None else int(n_hills)
        if not 0 <= H <= hills.shape[0]:
            raise ValueError(f"n_hills = {H} outside [0, {hills.shape[0]}]")
        if kernel not in _lib.METAD_KERNELS:
            raise ValueError(f"kernel must be one of {sorted(_lib.METAD_KERNELS)}, got {kernel!r}")
        per = None
        if periods is not None:
            per = np.ascontiguousarray(periods, np.float64).reshape(-1)
            if per.size != d or not (np.isfinite(per).all() and (per >= 0).all()):
                raise ValueError(f"periods must be {d} finite numbers >= 0 (0: not periodic)")
        return H, d, per, _lib.METAD_KERNELS[kernel]

    def metad_plan(self, n: int, n_hills: int, d: int, max_workgroups: int = 0) -> dict:
        """What metad_bias would launch (msm_metad_plan, include/msmhip.h).  Launches nothing."""
        out = (C.c_int64 * 4)()
        check(lib.msm_metad_plan(self.handle, int(n), int(n_hills), int(d), int(max_workgroups), out), self.handle)
        return {"frames_per_workgroup": int(out[0]), "hills_per_tile": int(out[1]), "grid": int(out[2]),
                "lds_bytes": int(out[3])}

    def metad_bias(self, cv: DeviceArray, hills: DeviceArray, n_hills: int | None = None, *, periods=None,
                   kernel: str = "gaussian", cut: float = 6.25, counts: DeviceArray | None = None, grad: bool = False,
                   max_workgroups: int = 0, bias: DeviceArray | None = None, grad_out: DeviceArray | None = None):
        """The hills sum at the frames cv f64 [n, ld >= d] (msm_metad_bias): `bias` f64 [n] and, with grad, its
        gradient f64 [n, d] in the CVs, device arrays.  hills f64 [capacity, 2 d + 1] (centre, 1 / sigma, height), of
        which the first `n_hills` count; frame f sums the hills 0 .. counts[f] - 1 (int32 [n]; None: all).  With
        preallocated `bias` / `grad_out` nothing is allocated, uploaded or waited for."""
        H, d, per, code = self._metad_shape(hills, n_hills, periods, kernel, _lib.METAD_MAX_D)
        if cv.dtype != np.float64 or len(cv.shape) != 2 or cv.shape[1] < d or cv.shape[0] < 1:
            raise ValueError(f"cv must be float64 with shape (n >= 1, >= {d}), got {cv.shape} {cv.dtype}")
        n, ld = cv.shape
        if counts is not None and (counts.dtype != np.int32 or counts.size != n):
            raise ValueError(f"counts must be int32 of {n} entries")
        bias = bias if bias is not None else self.empty((n,), np.float64)
        if grad and grad_out is None:
            grad_out = self.empty((n, d), np.float64)
        if bias.dtype != np.float64 or bias.size != n:
            raise ValueError(f"bias must be float64 of {n} entries")
        if grad_out is not None and (grad_out.dtype != np.float64 or len(grad_out.shape) != 2
                                     or grad_out.shape[0] != n or grad_out.shape[1] < d):
            raise ValueError(f"grad_out must be float64 with shape ({n}, >= {d})")
        check(lib.msm_metad_bias(self.handle, cv.ptr, n, ld, d, hills.ptr, H, per.ctypes.data if per is not None else None,
                                 code, float(cut), counts.ptr if counts is not None else None, int(max_workgroups),
                                 bias.ptr, grad_out.ptr if grad_out is not None else None,
                                 grad_out.shape[1] if grad_out is not None else 0), self.handle)
        return (bias, grad_out) if grad_out is not None else bias

    def metad_grid_scan(self, hills: DeviceArray, n_hills: int | None, lo, step, bins, checkpoints, a1: float,
                        a2: float, *, periods=None, kernel: str = "gaussian", cut: float = 6.25,
                        want_grid: bool = False, max_workgroups: int = 0):
        """lse f64 [M, 2] with lse[j, e] = log sum_g exp(a_e V_{k_j}(g)) over the regular grid lo + i * step of
        `bins` points per axis (msm_metad_grid_scan), V_k the sum of the first k hills; checkpoints ascending in
        [0, n_hills].  -> (lse, V_H on the grid f64 [bins] or None), device arrays.  A negative height raises
        ValueError; the call waits for the stream."""
        H, d, per, code = self._metad_shape(hills, n_hills, periods, kernel, _lib.METAD_GRID_MAX_D)
        lo, step = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (lo, step))
        bins = np.ascontiguousarray(bins, np.int32).reshape(-1)
        if lo.size != d or step.size != d or bins.size != d:
            raise ValueError(f"lo, step and bins must have {d} entries")
        ck = np.ascontiguousarray(checkpoints, np.int32).reshape(-1)
        if ck.size < 1:
            raise ValueError("metad_grid_scan needs at least one checkpoint")
        lse = self.empty((ck.size, 2), np.float64)
        vgrid = self.empty(tuple(int(b) for b in bins), np.float64) if want_grid else None
        check(lib.msm_metad_grid_scan(self.handle, hills.ptr, H, d, lo.ctypes.data, step.ctypes.data, bins.ctypes.data,
                                      per.ctypes.data if per is not None else None, code, float(cut), ck.ctypes.data,
                                      ck.size, float(a1), float(a2), int(max_workgroups), lse.ptr,
                                      vgrid.ptr if vgrid is not None else None), self.handle)
        self.sync()  # the uploaded checkpoint table is shared: the scan has read it before the next upload
        return lse, vgrid

    def metad_append(self, hills: DeviceArray, index: int, record, *, center: DeviceArray | None = None,
                     v: DeviceArray | None = None, v_scale: float = 0.0) -> None:
        """Writes hill `index` of the ledger hills f64 [capacity, 2 d + 1] (msm_metad_append): `record` = centre,
        1 / sigma, height, passed by value; `center` f64 [>= d] on the device replaces the centre, `v` f64 [1] scales
        the height by exp(v_scale * v[0]).  Nothing is staged and nothing waits."""
        _H, d, _per, _code = self._metad_shape(hills, None, None, "gaussian", _lib.METAD_MAX_D)
        rec = np.ascontiguousarray(record, np.float64).reshape(-1)
        if rec.size != 2 * d + 1:
            raise ValueError(f"a hill record has {2 * d + 1} entries, got {rec.size}")
        if center is not None and (center.dtype != np.float64 or center.size < d):
            raise ValueError(f"center must be float64 with at least {d} entries")
        if v is not None and (v.dtype != np.float64 or v.size < 1):
            raise ValueError("v must be float64 with one entry")
        check(lib.msm_metad_append(self.handle, hills.ptr, hills.shape[0], int(index), d, rec.ctypes.data,
                                   center.ptr if center is not None else None, v.ptr if v is not None else None,
                                   float(v_scale)), self.handle)

    # -- OPES (csrc/opes.hip) ------------------------------------------------------------------
    @staticmethod
    def opes_params(d: int, kT: float, prefactor: float, epsilon: float, cutoff: float, threshold: float = 1.0,
                    fixed_sigma: bool = False, periods=None, sigma0=None) -> np.ndarray:
        """The parameter vector h_par f64 [MSM_OPES_PARAMS] of msm_opes_deposit / msm_opes_bias."""
        d = int(d)
        if not 1 <= d <= _lib.METAD_MAX_D:
            raise ValueError(f"{d} collective variables, 1 to {_lib.METAD_MAX_D} are supported")
        par = np.zeros(_lib.OPES_PARAMS)
        par[:6] = float(kT), float(prefactor), float(epsilon), float(cutoff), float(threshold), float(bool(fixed_sigma))
        for name, at, given in (("periods", _lib.OPES_PAR_PERIOD, periods), ("sigma0", _lib.OPES_PAR_SIGMA0, sigma0)):
            if given is not None:
                a = np.ascontiguousarray(given, np.float64).reshape(-1)
                if a.size != d or not np.isfinite(a).all():
                    raise ValueError(f"{name} must be {d} finite numbers")
                par[at:at + d] = a
        return par

    def opes_plan(self, n: int, n_versions: int, d: int, max_workgroups: int = 0) -> dict:
        """What opes_bias and opes_deposit would launch (msm_opes_plan, include/msmhip.h).  Launches nothing."""
        out = (C.c_int64 * 6)()
        check(lib.msm_opes_plan(self.handle, int(n), int(n_versions), int(d), int(max_workgroups), out), self.handle)
        return {"frames_per_workgroup": int(out[0]), "versions_per_tile": int(out[1]), "grid": int(out[2]),
                "lds_bytes": int(out[3]), "deposit_threads": int(out[4]), "live_grid": int(out[5])}

    def opes_state(self, capacity: int, d: int) -> dict:
        """A fresh OPES ledger of `capacity` deposits on the device: the buffers msm_opes_deposit writes (state, live,
        slot_version, journal, death, per_deposit), with "capacity" and "d".  Z = 1, everything else 0."""
        cap, d = int(capacity), int(d)
        if cap < 1 or not 1 <= d <= _lib.METAD_MAX_D:
            raise ValueError(f"opes_state needs capacity >= 1 and 1 <= d <= {_lib.METAD_MAX_D}")
        state = np.zeros(_lib.OPES_STATE)
        state[_lib.OPES_STATE_Z] = 1.0
        R = 2 * d + 1
        return {"capacity": cap, "d": d, "state": self.to_device(state), "live": self.zeros((cap, R), np.float64),
                "slot_version": self.zeros((cap,), np.int32), "journal": self.zeros((cap, R), np.float64),
                "death": self.zeros((cap,), np.int32),
                "per_deposit": self.zeros((cap, _lib.OPES_PER_DEPOSIT), np.float64)}

    def opes_read_state(self, ledger: dict) -> dict:
        """The scalar state of a ledger, read back (waits for the stream): count, live, W, W2, S, Z, status, cursor."""
        s = ledger["state"].to_host()
        return {"count": int(s[_lib.OPES_STATE_COUNT]), "live": int(s[_lib.OPES_STATE_LIVE]),
                "W": float(s[_lib.OPES_STATE_W]), "W2": float(s[_lib.OPES_STATE_W2]),
                "S": float(s[_lib.OPES_STATE_SUM]), "Z": float(s[_lib.OPES_STATE_Z]),
                "status": int(s[_lib.OPES_STATE_STATUS]), "cursor": int(s[_lib.OPES_STATE_CURSOR])}

    def opes_clear_status(self, ledger: dict) -> dict:
        """Writes 0 to the status word of a ledger that refused a deposit, so that it accepts deposits again; the
        ledger is as its last accepted deposit left it.  Returns the state read (waits for the stream)."""
        s = ledger["state"].to_host()
        s[_lib.OPES_STATE_STATUS] = 0.0
        ledger["state"].copy_from_host(s)
        return self.opes_read_state(ledger)

    def opes_deposit(self, ledger: dict, params: np.ndarray, records: DeviceArray, n_records: int | None = None, *,
                     cv: DeviceArray | None = None, max_steps: int = 0) -> int:
        """Consumes the deposits records f64 [n_records, 2 d + 2] = centre, sigma, height, logweight
        (msm_opes_deposit) in ceil(n_records / max_steps) bounded launches (max_steps = 0: one launch); returns the
        number of launches.  With cv f64 [n_records, ld >= d] the deposits are made on line at those CVs and
        `records` receives what was deposited.  Nothing is uploaded or waited for; a full ledger or an unusable
        record shows in the status of opes_read_state, and while the status is not 0 every launch returns at once
        (opes_clear_status)."""
        d, cap = ledger["d"], ledger["capacity"]
        if records.dtype != np.float64 or len(records.shape) != 2 or records.shape[1] != 2 * d + 2:
            raise ValueError(f"records must be float64 with shape (n, {2 * d + 2}), got {records.shape} "
                             f"{records.dtype}")
        n = records.shape[0] if n_records is None else int(n_records)
        if not 0 <= n <= records.shape[0]:
            raise ValueError(f"n_records = {n} outside [0, {records.shape[0]}]")
        ld = 0
        if cv is not None:
            if cv.dtype != np.float64 or len(cv.shape) != 2 or cv.shape[1] < d or cv.shape[0] < n:
                raise ValueError(f"cv must be float64 with shape (>= {n}, >= {d}), got {cv.shape} {cv.dtype}")
            ld = cv.shape[1]
        par = np.ascontiguousarray(params, np.float64).reshape(-1)
        if par.size != _lib.OPES_PARAMS:
            raise ValueError(f"params must have {_lib.OPES_PARAMS} entries (Engine.opes_params)")
        steps = int(max_steps) if int(max_steps) > 0 else max(n, 1)
        if int(max_steps) < 0:
            raise ValueError("max_steps must be >= 0 (0: one launch)")
        launches = -(-n // steps)
        for i in range(launches):
            check(lib.msm_opes_deposit(self.handle, d, par.ctypes.data, ledger["state"].ptr, ledger["live"].ptr,
                                       ledger["slot_version"].ptr, ledger["journal"].ptr, ledger["death"].ptr,
                                       ledger["per_deposit"].ptr, cap, records.ptr, n,
                                       cv.ptr if cv is not None else None, ld, steps, 1 if i == 0 else 0), self.handle)
        return launches

    def opes_bias(self, cv: DeviceArray, ledger: dict, params: np.ndarray, n_versions: int | None = None, *,
                  counts: DeviceArray | None = None, live: bool = False, grad: bool = False, skip: bool = True,
                  max_workgroups: int = 0, bias: DeviceArray | None = None, grad_out: DeviceArray | None = None):
        """V at the frames cv f64 [n, ld >= d] (msm_opes_bias): `bias` f64 [n] and, with grad, dV/ds f64 [n, d], device
        arrays.  Journal form: frame f sees the state after its first counts[f] deposits of the `n_versions` in the
        journal (int32 [n]; None: all of them, the final bias).  live=True: one wave per frame against the live
        kernels with the state read on the device, the MD step.  With preallocated `bias` / `grad_out` nothing is
        allocated, uploaded or waited for."""
        d = ledger["d"]
        if cv.dtype != np.float64 or len(cv.shape) != 2 or cv.shape[1] < d or cv.shape[0] < 1:
            raise ValueError(f"cv must be float64 with shape (n >= 1, >= {d}), got {cv.shape} {cv.dtype}")
        n, ld = cv.shape
        par = np.ascontiguousarray(params, np.float64).reshape(-1)
        if par.size != _lib.OPES_PARAMS:
            raise ValueError(f"params must have {_lib.OPES_PARAMS} entries (Engine.opes_params)")
        if live:
            if counts is not None or n_versions is not None:
                raise ValueError("the live form takes neither counts nor n_versions")
            T = ledger["capacity"]
        else:
            if n_versions is None:
                raise ValueError("the journal form needs n_versions, the number of deposits made")
            T = int(n_versions)
            if not 0 <= T <= ledger["capacity"]:
                raise ValueError(f"n_versions = {T} outside [0, {ledger['capacity']}]")
        if counts is not None and (counts.dtype != np.int32 or counts.size != n):
            raise ValueError(f"counts must be int32 of {n} entries")
        bias = bias if bias is not None else self.empty((n,), np.float64)
        if grad and grad_out is None:
            grad_out = self.empty((n, d), np.float64)
        if bias.dtype != np.float64 or bias.size != n:
            raise ValueError(f"bias must be float64 of {n} entries")
        if grad_out is not None and (grad_out.dtype != np.float64 or len(grad_out.shape) != 2
                                     or grad_out.shape[0] != n or grad_out.shape[1] < d):
            raise ValueError(f"grad_out must be float64 with shape ({n}, >= {d})")
        check(lib.msm_opes_bias(self.handle, cv.ptr, n, ld, d, par.ctypes.data,
                                (ledger["live"] if live else ledger["journal"]).ptr,
                                None if live else ledger["death"].ptr, ledger["per_deposit"].ptr, T,
                                counts.ptr if counts is not None else None, ledger["state"].ptr,
                                0 if skip else _lib.OPES_NO_SKIP, int(max_workgroups), bias.ptr,
                                grad_out.ptr if grad_out is not None else None,
                                grad_out.shape[1] if grad_out is not None else 0), self.handle)
        return (bias, grad_out) if grad_out is not None else bias

    def state_counts(self, labels: DeviceArray, k: int, out: DeviceArray | None = None) -> DeviceArray:
        out = out if out is not None else self.empty((k,), np.int64)
        check(lib.msm_state_counts(self.handle, labels.ptr, labels.size, int(k), out.ptr), self.handle)
        return out

    def run_lengths(self, labels: DeviceArray, k: int):
        """Dwell-time runs of a label sequence (negative labels separate trajectories) ->
        (stats int64 [4, k] = min / max / sum / number per state, run states int32 [R], run lengths int64 [R])."""
        n = labels.size
        stats = self.empty((4, int(k)), np.int64)
        rs, rl = self.empty((max(n, 1),), np.int32), self.empty((max(n, 1),), np.int64)
        cnt = self.empty((1,), np.int64)
        check(lib.msm_run_lengths(self.handle, labels.ptr, n, int(k), stats.ptr, rs.ptr, rl.ptr, n, cnt.ptr), self.handle)
        r = int(cnt.to_host()[0])
        return stats.to_host(), rs.to_host()[:r], rl.to_host()[:r]

    # -- moments / covariance / TICA -------------------------------------------
    def column_moments(self, x: DeviceArray, ddof: int = 0, ld: int | None = None):
        """-> (mean, std, count) device arrays [F] f64 (NaN entries skipped).
        ``ld``: row stride in elements when x is a wider buffer's left block."""
        n, F = x.shape
        mean, std, cnt = (self.empty((F,), np.float64) for _ in range(3))
        check(lib.msm_column_moments(self.handle, x.ptr, _dtype_code(x.dtype), n, F, int(F if ld is None else ld),
                                     int(ddof), mean.ptr, std.ptr, cnt.ptr), self.handle)
        return mean, std, cnt

    def column_minmax(self, x: DeviceArray, ld: int | None = None):
        """(min [F], max [F] over the finite entries, int64 [2] = non-finite entries, fully finite rows).
        ``ld``: row stride in elements when x is a wider buffer's left block."""
        n, F = x.shape
        mn, mx, cnt = self.empty((F,), np.float64), self.empty((F,), np.float64), self.empty((2,), np.int64)
        check(lib.msm_column_minmax(self.handle, x.ptr, _dtype_code(x.dtype), n, F, int(F if ld is None else ld), mn.ptr,
                                    mx.ptr, cnt.ptr), self.handle)
        return mn, mx, cnt

    def column_moments_partial(self, x: DeviceArray, shift: DeviceArray | None = None,
                               sums: DeviceArray | None = None, ld: int | None = None):
        """Raw sums [cnt | S1 | S2] (3F f64) about `shift` (default: row 0) -> (sums, shift).
        ``ld``: row stride in elements when x is a wider buffer's left block."""
        n, F = x.shape
        sums = sums if sums is not None else self.empty((3 * F,), np.float64)
        shift_out = self.empty((F,), np.float64) if shift is None else None  # no allocation in steady state
        check(lib.msm_column_moments_partial(self.handle, x.ptr, _dtype_code(x.dtype), n, F, int(F if ld is None else ld),
                                             shift.ptr if shift is not None else None, sums.ptr,
                                             shift_out.ptr if shift_out is not None else None), self.handle)
        return sums, (shift_out if shift_out is not None else shift)

    def moments_finalize(self, sums: DeviceArray, shift: DeviceArray, F: int, ddof: int = 0):
        mean, std, cnt = (self.empty((F,), np.float64) for _ in range(3))
        check(lib.msm_moments_finalize(self.handle, sums.ptr, shift.ptr, F, int(ddof), mean.ptr, std.ptr,
                                       cnt.ptr), self.handle)
        return mean, std, cnt

    def standardise_params(self, sums: DeviceArray, shift: DeviceArray, F: int, n_rows: float, with_std: bool = True,
                           out=None):
        """-> (mean, scale, inv_scale) device arrays [F]: the _preprocess parameters, no host sync."""
        mean, scale, inv = out if out is not None else tuple(self.empty((F,), np.float64) for _ in range(3))
        check(lib.msm_standardise_params(self.handle, sums.ptr, shift.ptr, F, float(n_rows), int(bool(with_std)),
                                         mean.ptr, scale.ptr, inv.ptr), self.handle)
        return mean, scale, inv

    def lagged_moments(self, x: DeviceArray, lag: int, shift: DeviceArray, *, starts=None, stops=None,
                       assume_finite: bool = False, out: DeviceArray | None = None,
                       one_sided: bool = False, symmetric: bool = False, ld: int | None = None) -> DeviceArray:
        """Raw lagged moments [M00 | M0t | sx | sy | T] (2F^2+2F+1 f64): the reversible estimator's
        (M00 over X0 and Yt) or, with one_sided, M00 over X0 only.  symmetric: the M0t block holds
        (M0t + M0t') / 2 -- all a reversible TICA reads of it -- from the cheaper symmetric accumulation.
        ``ld``: row stride in elements when x is a wider buffer's left block."""
        if one_sided and symmetric:
            raise ValueError("one_sided and symmetric moments exclude each other")
        n, F = x.shape
        if starts is None:
            starts, stops = segments_to_bounds(None, n)
        starts, stops = self._seg_ptrs(starts, stops)
        out = out if out is not None else self.empty((2 * F * F + 2 * F + 1,), np.float64)
        fn = (lib.msm_lagged_moments_onesided if one_sided
              else lib.msm_lagged_moments_reversible if symmetric else lib.msm_lagged_moments)
        check(fn(self.handle, x.ptr, _dtype_code(x.dtype), n, F, int(F if ld is None else ld), starts.ctypes.data,
                 stops.ctypes.data, len(starts), int(lag), shift.ptr, int(bool(assume_finite)), out.ptr), self.handle)
        return out

    def autocorr_lagscan(self, x: DeviceArray, lags: Sequence[int], *, starts=None, stops=None,
                         var_floor: float = 1e-8, ld: int | None = None):
        """Per-segment autocorrelation of the standardised columns of x [n, F] at every lag ->
        (values f64 [n_seg, n_lag], valid columns int32 [n_seg]) device arrays (msm_autocorr_lagscan).
        Any number of segments and lags; ``ld``: row stride in elements when x is a wider buffer's left block."""
        n, F = x.shape
        lags_arr = np.ascontiguousarray(lags, np.int64).reshape(-1)
        if lags_arr.size and (lags_arr.min() < 1 or lags_arr.max() > np.iinfo(np.int32).max):
            raise ValueError("lags must be integers in [1, 2^31)")
        lags_arr = lags_arr.astype(np.int32)
        if starts is None:
            starts, stops = segments_to_bounds(None, n)
        starts, stops = self._seg_ptrs(starts, stops)
        value = self.empty((len(starts), len(lags_arr)), np.float64)
        nvalid = self.empty((len(starts),), np.int32)
        check(lib.msm_autocorr_lagscan(self.handle, x.ptr, _dtype_code(x.dtype), n, F, int(F if ld is None else ld),
                                       starts.ctypes.data, stops.ctypes.data, len(starts), lags_arr.ctypes.data,
                                       len(lags_arr), float(var_floor), value.ptr, nvalid.ptr), self.handle)
        return value, nvalid

    def hstack(self, a: DeviceArray, b: DeviceArray) -> DeviceArray:
        """[a | b] as one float64 device array [n, pa + pb]; both [n, *], float32 or float64."""
        (n, pa), (nb, pb) = a.shape, b.shape
        if n != nb:
            raise ValueError(f"hstack: row counts differ ({n} vs {nb})")
        out = self.empty((n, pa + pb), np.float64)
        check(lib.msm_hstack_f64(self.handle, a.ptr, _dtype_code(a.dtype), pa, pa, b.ptr, _dtype_code(b.dtype), pb, pb,
                                 n, out.ptr), self.handle)
        return out

    def onesided_tica_eigenvalues(self, moments: DeviceArray, F: int, clip: float = 1e-12) -> DeviceArray:
        """Descending eigenvalues of the reference's in-repo estimator from one-sided moments."""
        out = self.empty((F,), np.float64)
        check(lib.msm_onesided_tica_eigenvalues(self.handle, moments.ptr, int(F), float(clip), out.ptr), self.handle)
        return out

    def moments_from_lagged(self, x: DeviceArray, lag: int, shift: DeviceArray, moments: DeviceArray, *, starts=None,
                            stops=None, out: DeviceArray | None = None, ld: int | None = None) -> DeviceArray:
        """[cnt | S1 | S2] over all frames from lagged moments of the same shift (finite data only).
        ``ld``: row stride in elements when x is a wider buffer's left block."""
        n, F = x.shape
        if starts is None:
            starts, stops = segments_to_bounds(None, n)
        starts, stops = self._seg_ptrs(starts, stops)
        out = out if out is not None else self.empty((3 * F,), np.float64)
        check(lib.msm_moments_from_lagged(self.handle, x.ptr, _dtype_code(x.dtype), n, F, int(F if ld is None else ld),
                                          starts.ctypes.data, stops.ctypes.data, len(starts), int(lag), shift.ptr,
                                          moments.ptr, out.ptr), self.handle)
        return out

    def moments_tail(self, x: DeviceArray, lag: int, shift: DeviceArray, moments: DeviceArray, n_rows: float,
                     with_std: bool = True, *, starts=None, stops=None, sums: DeviceArray | None = None, out=None,
                     zero_slot: DeviceArray | None = None, ld: int | None = None):
        """moments_from_lagged + standardise_params in one launch, same bits -> (sums, (mean, scale, inv_scale)).
        zero_slot: one 8-byte device word the launch also clears (the max |Y| slot of a fit state, for
        project(absmax_preset=True))."""
        n, F = x.shape
        if starts is None:
            starts, stops = segments_to_bounds(None, n)
        starts, stops = self._seg_ptrs(starts, stops)
        sums = sums if sums is not None else self.empty((3 * F,), np.float64)
        mean, scale, inv = out if out is not None else tuple(self.empty((F,), np.float64) for _ in range(3))
        check(lib.msm_moments_tail(self.handle, x.ptr, _dtype_code(x.dtype), n, F, int(F if ld is None else ld),
                                   starts.ctypes.data, stops.ctypes.data, len(starts), int(lag), shift.ptr, moments.ptr,
                                   sums.ptr, float(n_rows), int(bool(with_std)), mean.ptr, scale.ptr, inv.ptr,
                                   zero_slot.ptr if zero_slot is not None else None), self.handle)
        return sums, (mean, scale, inv)

    def tica_solve(self, moments: DeviceArray, F: int, *, scale: DeviceArray | None = None,
                   epsilon: float = 1e-6, kinetic_map: bool = True, out=None, n_lead: int = 0):
        """-> (eigvals [F], coeffs [F,F], mean [F], rank int32[1]) on the device (`out`: the same four, preallocated).
        n_lead in 1 .. F-1: only the first n_lead components are wanted; they carry the bits of the full solve, the
        columns and eigenvalues after them are zero (0 or >= F: all of them)."""
        if out is not None:
            eig, W, mean, rank = out
        else:
            eig = self.empty((F,), np.float64)
            W = self.empty((F, F), np.float64)
            mean = self.empty((F,), np.float64)
            rank = self.empty((1,), np.int32)
        check(lib.msm_tica_solve_leading(self.handle, moments.ptr, scale.ptr if scale is not None else None, F,
                                         float(epsilon), int(bool(kinetic_map)), eig.ptr, W.ptr, mean.ptr, rank.ptr,
                                         int(n_lead)), self.handle)
        return eig, W, mean, rank

    def project(self, x: DeviceArray, mu: DeviceArray, inv_sigma: DeviceArray, W: DeviceArray, d: int, *,
                mean2: DeviceArray | None = None, out: DeviceArray | None = None,
                absmax: DeviceArray | None = None, assume_finite: bool = False, ld: int | None = None,
                absmax_preset: bool = False) -> DeviceArray:
        """`absmax` (one f64, e.g. slot 2 of a k-means fit state) receives max |Y| from the same pass.
        absmax_preset: an earlier call on the stream left `absmax` at zero (moments_tail's zero_slot): no clear here.
        assume_finite: X holds no NaN (column_moments' count tells); the per-element NaN test is left out.
        ``ld``: row stride in elements when x is a wider buffer's left block."""
        n, F = x.shape
        ldw = W.shape[1]
        out = out if out is not None else self.empty((n, d), np.float64)
        args = (self.handle, x.ptr, _dtype_code(x.dtype), n, F, int(F if ld is None else ld), mu.ptr, inv_sigma.ptr,
                mean2.ptr if mean2 is not None else None, W.ptr, int(d), ldw, out.ptr, out.shape[1],
                absmax.ptr if absmax is not None else None)
        if absmax_preset:
            check(lib.msm_project_preset(*args, int(bool(assume_finite))), self.handle)
        else:
            check((lib.msm_project_finite if assume_finite else lib.msm_project)(*args), self.handle)
        return out

    def _mlp_on_device(self, spec):
        """(parameters, mean, scale) of a network spec on this device: uploaded on the first call with the spec and
        kept with it."""
        dev = getattr(spec, "_dev", None)
        if dev is None or dev[0] is not self:
            params = self.to_device(np.ascontiguousarray(spec.params, np.float32).reshape(-1))
            mean = self.to_device(spec.mean, np.float64) if spec.mean is not None else None
            scale = self.to_device(spec.scale, np.float64) if spec.scale is not None else None
            dev = spec._dev = (self, params, mean, scale)
        return dev[1:]

    def mlp_forward(self, x: DeviceArray, spec, out: DeviceArray | None = None, ld: int | None = None) -> DeviceArray:
        """Outputs [n, n_out] f64 of the network `spec` describes (features.deeptica.MLPSpec: widths, activation
        code, flags, packed fp32 parameters, scaler) for the frames x [n, F], f32 or f64 (msm_mlp_forward).
        The parameters are uploaded on the first call with a spec and kept with it, so later calls, and calls under
        graph capture, launch the kernel and nothing else.  `out`: preallocated, any width >= n_out.
        ``ld``: row stride in elements when x is a wider buffer's left block."""
        n, F = x.shape
        widths = np.ascontiguousarray(spec.widths, np.int32)
        params, mean, scale = self._mlp_on_device(spec)
        out = out if out is not None else self.empty((n, int(widths[-1])), np.float64)
        check(lib.msm_mlp_forward(self.handle, x.ptr, _dtype_code(x.dtype), n, F, int(F if ld is None else ld),
                                  mean.ptr if mean is not None else None, scale.ptr if scale is not None else None,
                                  len(widths) - 1, widths.ctypes.data, int(spec.activation), int(bool(spec.ln_in)),
                                  int(bool(spec.ln_hidden)), int(bool(spec.head_activation)), params.ptr, params.size,
                                  out.ptr, out.shape[1]), self.handle)
        return out

    def mlp_plan(self, kernel: str, spec, rows: int, dtype=np.float32) -> dict:
        """The launch shape `kernel` ("forward", "vjp", "train_forward" or "train_backward") would get on this engine
        now for the network `spec` (an MLPSpec, or its widths with ln_in / ln_hidden / head_activation attributes) and
        `rows` rows -- n, or the 2m slots of a training batch -- of x in `dtype` (msm_mlp_launch_plan,
        include/msmhip.h): lds_bytes, per_cu, grid, grid_cap (= CUs x per_cu: the grid of a batch that is large
        enough), n_groups, trips, and for the training kernels param_chunks, vamp_chunks, param_jobs.  Launches
        nothing."""
        import ctypes

        if kernel not in _lib.MLP_KERNELS:
            raise ValueError(f"kernel must be one of {sorted(_lib.MLP_KERNELS)}, got {kernel!r}")
        widths = np.ascontiguousarray(spec.widths, np.int32)
        out = (ctypes.c_int64 * 8)()
        check(lib.msm_mlp_launch_plan(self.handle, _lib.MLP_KERNELS[kernel], _dtype_code(np.dtype(dtype)), int(rows),
                                      len(widths) - 1, widths.ctypes.data, int(bool(spec.ln_in)),
                                      int(bool(spec.ln_hidden)), int(bool(spec.head_activation)), out), self.handle)
        v = [int(x) for x in out]
        plan = {"lds_bytes": v[0], "per_cu": v[1], "grid": v[2], "grid_cap": self.info()["n_cu"] * v[1],
                "n_groups": v[3], "trips": v[4]}
        if kernel.startswith("train"):
            plan.update(param_chunks=v[5], vamp_chunks=v[6], param_jobs=v[7])
        return plan

    # -- DeepTICA training ------------------------------------------------------
    @staticmethod
    def _vamp2_stats(stats: np.ndarray, d: int) -> dict:
        """The stats block of msm_vamp2_loss as loss, score, penalty and the reference's ten latest_metrics."""
        if stats[9] != 0.0:
            raise RuntimeError("Cholesky decomposition failed after retries")
        head, w = 16, _lib.MLP_MAX_OUT
        vec = lambda i: stats[head + i * w: head + i * w + d].tolist()       # noqa: E731
        return {"loss": float(stats[0]), "score": float(stats[1]), "penalty": float(stats[2]),
                "metrics": {"cond_C00": float(stats[3]), "cond_Ctt": float(stats[4]), "var_z0": vec(0),
                            "var_zt": vec(1), "mean_z0": vec(2), "mean_zt": vec(3), "eig_C00_min": float(stats[5]),
                            "eig_C00_max": float(stats[6]), "eig_Ctt_min": float(stats[7]),
                            "eig_Ctt_max": float(stats[8])}}

    def _pair_weights(self, weights, m: int) -> DeviceArray:
        """Per-pair weights [m] on the device: an f64 device array as it is, a host array checked (finite, clamped
        sum positive) and uploaded."""
        if isinstance(weights, DeviceArray):
            if weights.dtype != np.float64:
                raise TypeError("pair weights on the device must be float64")
            if weights.size != m:
                raise ValueError(f"{weights.size} weights for {m} frame pairs")
            return weights
        w = np.ascontiguousarray(weights, np.float64).reshape(-1)
        if w.size != m:
            raise ValueError(f"{w.size} weights for {m} frame pairs")
        if not np.all(np.isfinite(w)):
            raise ValueError("pair weights must be finite")
        total = float(np.clip(w, 0.0, None).sum())
        if not (total > 0.0 and np.isfinite(total)):
            raise ValueError("pair weights sum to zero" if total == 0.0 else "the sum of the pair weights overflows")
        return self.to_device(w)

    def _weighted_stats(self, stats: np.ndarray, d: int) -> dict:
        """The stats block of a weighted call: the device's weight flag first, then _vamp2_stats and the two
        weight figures."""
        if stats[10] != 0.0:
            raise RuntimeError("pair weights on the device are not finite or do not sum to a positive number")
        res = self._vamp2_stats(stats, d)
        res["total_weight"], res["effective_pairs"] = float(stats[11]), float(stats[12])
        return res

    def vamp2_loss(self, z0: DeviceArray, zt: DeviceArray, *, eps: float = 1e-3, eps_abs: float = 1e-6,
                   alpha: float = 0.15, cond_reg: float = 1e-4, want_grad: bool = True, ld: int | None = None,
                   weights=None) -> dict:
        """VAMP-2 loss of the outputs z0, zt [m, n_out] f64 with uniform weights (msm_vamp2_loss): a dict of loss,
        score, penalty, `metrics` (the reference's ten latest_metrics) and, with want_grad, `grad0` / `grad_t`
        [m, n_out] f64 on the device, the derivative of the loss with respect to z0 / zt.  ``ld``: row stride of
        both inputs when they are blocks of wider buffers.  A Cholesky failure after the jitter ladder raises
        RuntimeError as the reference does.
        ``weights``: per-pair weights [m], a host array or an f64 device array (msm_vamp2_loss_weighted: negative
        weights count as 0, only ratios matter); the result then also has `total_weight` and `effective_pairs`
        (Kish).  Host weights that are not finite or whose clamped sum is 0 raise ValueError; the same found on the
        device raises RuntimeError."""
        m, d = z0.shape
        if zt.shape != z0.shape:
            raise ValueError("z0 and zt must share the same shape")
        if z0.dtype != np.float64 or zt.dtype != np.float64:
            raise TypeError("outputs must be float64")
        if m == 0:
            raise ValueError("VAMP2Loss received empty batch")
        if d > _lib.MLP_MAX_OUT:
            raise NotImplementedError(f"{d} outputs (at most {_lib.MLP_MAX_OUT} are supported)")
        wts = self._pair_weights(weights, m) if weights is not None else None
        sizer = lib.msm_vamp2_workspace if wts is None else lib.msm_vamp2_weighted_workspace
        work = self.empty((max(int(sizer(m, d)), 8) // 8,), np.float64)
        stats = self.empty((_lib.VAMP2_STATS,), np.float64)
        g0 = self.empty((m, d), np.float64) if want_grad else None
        gt = self.empty((m, d), np.float64) if want_grad else None
        tail = (m, d, int(d if ld is None else ld), float(eps), float(eps_abs), float(alpha), float(cond_reg), work.ptr,
                stats.ptr, g0.ptr if want_grad else None, gt.ptr if want_grad else None, d)
        if wts is None:
            check(lib.msm_vamp2_loss(self.handle, z0.ptr, zt.ptr, *tail), self.handle)
            res = self._vamp2_stats(stats.to_host(), d)
        else:
            check(lib.msm_vamp2_loss_weighted(self.handle, z0.ptr, zt.ptr, wts.ptr, *tail), self.handle)
            res = self._weighted_stats(stats.to_host(), d)
        if want_grad:
            res["grad0"], res["grad_t"] = g0, gt
        return res

    def _pair_indices(self, idx, n: int) -> DeviceArray:
        if isinstance(idx, DeviceArray):
            if idx.dtype != np.int64:
                raise TypeError("pair indices on the device must be int64")
            return idx
        idx = np.ascontiguousarray(idx, np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            raise IndexError(f"pair index outside [0, {n})")
        return self.to_device(idx)

    def mlp_loss_grad(self, x: DeviceArray, spec, idx_t, idx_tau, *, dropout=None, seed: int = 0, step: int = 0,
                      eps: float = 1e-3, eps_abs: float = 1e-6, alpha: float = 0.15, cond_reg: float = 1e-4,
                      want_grad: bool = True, want_outputs: bool = False, ld: int | None = None,
                      work: DeviceArray | None = None, weights=None) -> dict:
        """Loss and parameter gradient of the network `spec` on the lagged pairs (idx_t[i], idx_tau[i]) of the
        resident frames x [n, F] (msm_mlp_loss_grad).  idx_t, idx_tau: equally long integer arrays (host arrays are
        range-checked and uploaded; int64 device arrays are used as they are).  dropout: None for evaluation
        mode, else the probabilities [input, after hidden layer 0, ...] (one per Linear layer); masks are a pure
        function of (seed, step, site, slot, column), see include/msmhip.h.  Returns the dict of vamp2_loss without
        its output gradients, plus `grad` [n_params] f64 (want_grad) and `outputs` [2m, n_out] f64 (want_outputs:
        the t frames' outputs, then the tau frames'), both on the device, and `work`, the workspace the call used
        (msm_mlp_train_workspace bytes): hand it back through ``work`` and the next call of the same or a smaller
        shape allocates nothing.
        ``weights``: per-pair weights [m] as in vamp2_loss (msm_mlp_loss_grad_weighted); the result then also has
        `total_weight` and `effective_pairs`, and the workspace is msm_mlp_train_weighted_workspace bytes."""
        n, F = x.shape
        widths = np.ascontiguousarray(spec.widths, np.int32)
        spec.check_envelope()
        n_linear = len(widths) - 1
        it, itau = self._pair_indices(idx_t, n), self._pair_indices(idx_tau, n)
        m = it.size
        if itau.size != m:
            raise ValueError(f"{m} t frames and {itau.size} tau frames")
        if m < 2:
            raise ValueError(f"{m} frame pairs (at least 2 are needed)")
        drop = None
        if dropout is not None:
            drop = np.ascontiguousarray(dropout, np.float64).reshape(-1)
            if drop.size != n_linear:
                raise ValueError(f"{drop.size} dropout probabilities for {n_linear} dropout sites")
            if np.any(drop >= 1.0) or np.any(drop < 0.0) or not np.all(np.isfinite(drop)):
                raise ValueError(f"dropout probabilities {drop.tolist()} (0 <= p < 1)")
        params, mean, scale = self._mlp_on_device(spec)
        flags = (int(bool(spec.ln_in)), int(bool(spec.ln_hidden)), int(bool(spec.head_activation)))
        wts = self._pair_weights(weights, m) if weights is not None else None
        sizer = lib.msm_mlp_train_workspace if wts is None else lib.msm_mlp_train_weighted_workspace
        need = int(sizer(m, n_linear, widths.ctypes.data, *flags))
        if need == 0:
            raise NotImplementedError(f"{m} frame pairs (at most {1 << 24} are supported)")
        if work is None or work.nbytes < need:
            work = self.empty((need // 8,), np.float64)
        d = int(widths[-1])
        stats = self.empty((_lib.VAMP2_STATS,), np.float64)
        grad = self.empty((params.size,), np.float64) if want_grad else None
        out = self.empty((2 * m, d), np.float64) if want_outputs else None
        head = (self.handle, x.ptr, _dtype_code(x.dtype), n, F, int(F if ld is None else ld),
                mean.ptr if mean is not None else None, scale.ptr if scale is not None else None, n_linear,
                widths.ctypes.data, int(spec.activation), *flags, params.ptr, params.size, it.ptr, itau.ptr)
        tail = (m, drop.ctypes.data if drop is not None else None, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), float(eps),
                float(eps_abs), float(alpha), float(cond_reg), work.ptr, work.nbytes, stats.ptr,
                grad.ptr if want_grad else None, out.ptr if want_outputs else None, d)
        if wts is None:
            check(lib.msm_mlp_loss_grad(*head, *tail), self.handle)
            res = self._vamp2_stats(stats.to_host(), d)
        else:
            check(lib.msm_mlp_loss_grad_weighted(*head, wts.ptr, *tail), self.handle)
            res = self._weighted_stats(stats.to_host(), d)
        res["work"] = work
        if want_grad:
            res["grad"] = grad
        if want_outputs:
            res["outputs"] = out
        return res

    def adamw_step(self, params: DeviceArray, grad: DeviceArray, m: DeviceArray, v: DeviceArray, step: int, *,
                   lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                   clip: float | None = None) -> dict:
        """Gradient clip and one AdamW step in place (msm_adamw_step): params [n] f32, grad, m, v [n] f64, step
        counting from 1; clip None or <= 0: no clipping.  Returns grad_norm_preclip, grad_norm and `skipped`: with a
        non-finite gradient norm nothing is updated and skipped is True."""
        n = params.size
        if params.dtype != np.float32 or any(a.dtype != np.float64 for a in (grad, m, v)):
            raise TypeError("params must be float32; grad, m and v float64")
        if any(a.size != n for a in (grad, m, v)):
            raise ValueError("params, grad, m and v must have the same length")
        out = self.empty((4,), np.float64)
        check(lib.msm_adamw_step(self.handle, params.ptr, grad.ptr, m.ptr, v.ptr, n, int(step), float(lr),
                                 float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                 float(clip) if clip is not None else 0.0, out.ptr), self.handle)
        o = out.to_host()
        return {"grad_norm_preclip": float(o[0]), "grad_norm": float(o[1]), "skipped": bool(o[2] != 0.0)}

    def eigh(self, a: DeviceArray, want_vectors: bool = True):
        n = a.shape[0]
        w = self.empty((n,), np.float64)
        v = self.empty((n, n), np.float64) if want_vectors else None
        sweeps = self.empty((1,), np.int32)
        check(lib.msm_eigh(self.handle, a.ptr, n, w.ptr, v.ptr if v is not None else None, sweeps.ptr),
              self.handle)
        return w, v, sweeps

    # -- k-means --------------------------------------------------------------
    def kmeans_assign(self, x: DeviceArray, centers: DeviceArray, *, mean: DeviceArray | None = None,
                      std: DeviceArray | None = None, labels: DeviceArray | None = None,
                      mindist: DeviceArray | None = None, image: DeviceArray | None = None) -> DeviceArray:
        n, d = x.shape
        k, dc = centers.shape
        if dc != d:
            raise ValueError(f"centres have {dc} features, data has {d}")
        if centers.dtype != np.float64:
            raise TypeError("centres must be float64")
        labels = labels if labels is not None else self.empty((n,), np.int32)
        check(lib.msm_kmeans_assign_packed(self.handle, x.ptr, _dtype_code(x.dtype), n, d, d, centers.ptr, k,
                                           mean.ptr if mean is not None else None,
                                           std.ptr if std is not None else None,
                                           image.ptr if image is not None else None, labels.ptr,
                                           mindist.ptr if mindist is not None else None), self.handle)
        return labels


    FIT_STATE_FIELDS = ("scale", "inv_scale", "absmax", "shift2", "tol2", "done", "n_iter", "inertia")

    def kmeans_fit(self, x: DeviceArray, k: int, *, seed: int = 0, max_iter: int = 50, tol2: float = 0.0,
                   mean: DeviceArray | None = None, std: DeviceArray | None = None,
                   centers: DeviceArray | None = None) -> tuple[DeviceArray, DeviceArray]:
        """Lloyd k-means on one device -> (centers [k,d] f64, state [8] f64).
        Pass `centers` to start from given centres instead of the seeded stratified draw."""
        n, d = x.shape
        init = centers is None
        centers = centers if centers is not None else self.empty((k, d), np.float64)
        state = self.zeros((8,), np.float64)
        check(lib.msm_kmeans_fit(self.handle, x.ptr, _dtype_code(x.dtype), n, d, d,
                                 mean.ptr if mean is not None else None, std.ptr if std is not None else None,
                                 int(k), int(seed) & (2**64 - 1), int(init), int(max_iter), float(tol2), centers.ptr,
                                 state.ptr), self.handle)
        return centers, state

    def kmeans_init_plusplus(self, x: DeviceArray, k: int, *, seed: int = 0, mean: DeviceArray | None = None,
                             std: DeviceArray | None = None, n_total: int | None = None,
                             centers: DeviceArray | None = None, return_picked: bool = False):
        """k-means++ seeding on the device (csrc/kmeanspp.hip): centres [k, d] f64 = frames drawn with probability
        proportional to the squared distance to the nearest centre already drawn (deterministic in the data and seed)."""
        n, d = x.shape
        n_total = n if n_total is None else int(n_total)
        centers, state = self.kmeans_fit_begin(x, k, seed=seed, n_total=n_total, tol2=0.0, mean=mean, std=std,
                                               centers=centers, init_centers=False)
        picked = self.empty((k,), np.int64) if return_picked else None
        check(lib.msm_kmeans_init_plusplus(self.handle, x.ptr, _dtype_code(x.dtype), n, d, d,
                                           mean.ptr if mean is not None else None, std.ptr if std is not None else None,
                                           int(k), int(seed) & (2**64 - 1), float(n_total), centers.ptr, state.ptr,
                                           picked.ptr if picked is not None else None), self.handle)
        return (centers, picked) if return_picked else centers

    def kmeans_fit_minibatch(self, x: DeviceArray, k: int, *, seed: int = 0, batch_size: int = 100, max_iter: int = 5,
                             init: str = "kmeans++", centers: DeviceArray | None = None,
                             max_batches: int = 4096) -> tuple[DeviceArray, DeviceArray]:
        """Mini-batch k-means (Sculley; what sklearn's MiniBatchKMeans and deeptime's do with their batches): the
        frames are dealt into `nb` interleaved batches (batch b = frames b, b + nb, ...: a batch of a time series should
        not be one stretch of it), every batch is assigned to the current centres and ADDED to the running member sums,
        and the centres are the running means -- `max_iter` sweeps over all batches.  nb = ceil(n / batch_size), at
        most `max_batches` (two launches per batch).  Same kernels as the full-batch fit (msm_kmeans_accumulate /
        msm_kmeans_update through their row stride), so the sums are exact fixed point and the result is
        deterministic."""
        n, d = x.shape
        if batch_size < 1 or max_iter < 0:
            raise ValueError("batch_size must be >= 1 and max_iter >= 0")
        given = centers is not None
        # the running sums see every frame once per sweep: the fixed-point scale is sized for n * max_iter terms
        n_terms = n * max(1, int(max_iter))
        centers, state = self.kmeans_fit_begin(x, k, seed=seed, n_total=n_terms, tol2=0.0, centers=centers,
                                               init_centers=not given and init != "kmeans++")
        if not given and init == "kmeans++":
            check(lib.msm_kmeans_init_plusplus(self.handle, x.ptr, _dtype_code(x.dtype), n, d, d, None, None, int(k),
                                               int(seed) & (2**64 - 1), float(n_terms), centers.ptr, state.ptr, None),
                  self.handle)
        nb = max(1, min(int(max_batches), -(-n // int(batch_size))))
        sums, counts = self.zeros((k * d,), np.int64), self.zeros((k,), np.int64)
        item = x.dtype.itemsize
        for _ in range(int(max_iter)):
            for b in range(nb):
                rows = (n - b + nb - 1) // nb
                if rows <= 0:
                    continue
                check(lib.msm_kmeans_accumulate(self.handle, x.ptr + b * d * item, _dtype_code(x.dtype), rows, d, nb * d,
                                                centers.ptr, k, None, None, state.ptr, sums.ptr, counts.ptr), self.handle)
                check(lib.msm_kmeans_update(self.handle, sums.ptr, counts.ptr, k, d, centers.ptr, state.ptr, 0), self.handle)
        return centers, state

    def kmeans_fit_begin(self, x: DeviceArray, k: int, *, seed: int, n_total: int, tol2: float,
                         mean: DeviceArray | None = None, std: DeviceArray | None = None,
                         centers: DeviceArray | None = None, init_centers: bool = True,
                         state: DeviceArray | None = None, absmax_ready: bool = False,
                         sums: DeviceArray | None = None, counts: DeviceArray | None = None):
        """absmax_ready: slot 2 of `state` already holds max |x| (left there by project(absmax=...)).
        sums [k*d] / counts [k] (int64, both or neither): the member sums of the fit, zeroed by the same launch."""
        n, d = x.shape
        centers = centers if centers is not None else self.empty((k, d), np.float64)
        state = state if state is not None else self.zeros((8,), np.float64)
        args = (self.handle, x.ptr, _dtype_code(x.dtype), n, d, d, mean.ptr if mean is not None else None,
                std.ptr if std is not None else None, int(k), int(seed) & (2**64 - 1), int(bool(init_centers)),
                float(n_total), float(tol2), centers.ptr, state.ptr, int(bool(absmax_ready)))
        if (sums is None) != (counts is None):
            raise ValueError("kmeans_fit_begin: sums and counts must come together")
        if sums is not None:
            if sums.size != k * d or counts.size != k:
                raise ValueError("kmeans_fit_begin: sums must hold k*d and counts k entries")
            check(lib.msm_kmeans_fit_begin_clear(*args, sums.ptr, counts.ptr), self.handle)
        else:
            check(lib.msm_kmeans_fit_begin(*args), self.handle)
        return centers, state

    def kmeans_accumulate(self, x: DeviceArray, centers: DeviceArray, state: DeviceArray, sums: DeviceArray,
                          counts: DeviceArray, *, mean: DeviceArray | None = None, std: DeviceArray | None = None,
                          image: DeviceArray | None = None, prev_labels: DeviceArray | None = None,
                          first_pass: bool = False):
        """Member sums / counts of one Lloyd pass.  With `prev_labels` (int32 [n], -1 before the first pass, updated
        in place) only the frames that changed centre move their contribution: `sums` / `counts` must then persist
        between the passes (kmeans_update(clear=False)).  first_pass: the first pass of a fit -- `prev_labels` need
        not hold -1, its contents are ignored."""
        n, d = x.shape
        k = centers.shape[0]
        if prev_labels is not None:
            args = (self.handle, x.ptr, _dtype_code(x.dtype), n, d, d, centers.ptr, k,
                    mean.ptr if mean is not None else None, std.ptr if std is not None else None,
                    image.ptr if image is not None else None, state.ptr, prev_labels.ptr, sums.ptr, counts.ptr)
            if first_pass:
                check(lib.msm_kmeans_accumulate_delta_from(*args, 1), self.handle)
            else:
                check(lib.msm_kmeans_accumulate_delta(*args), self.handle)
            return
        check(lib.msm_kmeans_accumulate_packed(self.handle, x.ptr, _dtype_code(x.dtype), n, d, d, centers.ptr, k,
                                               mean.ptr if mean is not None else None,
                                               std.ptr if std is not None else None,
                                               image.ptr if image is not None else None, state.ptr, sums.ptr,
                                               counts.ptr), self.handle)

    # -- bf16 frame images of the certified filter (msm_kmeans_pack) -----------------------------------------
    def kmeans_image_bytes(self, n: int, d: int) -> int:
        out = C.c_size_t(0)
        check(lib.msm_kmeans_image_bytes(int(n), int(d), C.byref(out)), self.handle)
        return int(out.value)

    def kmeans_pack(self, x: DeviceArray, *, mean: DeviceArray | None = None, std: DeviceArray | None = None,
                    image: DeviceArray | None = None, absmax: DeviceArray | None = None) -> DeviceArray | None:
        """Frame images for repeated k-means passes over the same frames; None when d is outside the filter's range.
        absmax: one device f64 >= max |x| (e.g. slot 2 of a fit state); without it the library finds the maximum."""
        n, d = x.shape
        nbytes = self.kmeans_image_bytes(n, d)
        if nbytes == 0:
            return None
        image = image if image is not None else self.empty((nbytes,), np.uint8)
        if image.nbytes < nbytes:
            raise ValueError(f"image buffer holds {image.nbytes} bytes, {nbytes} needed")
        check(lib.msm_kmeans_pack_bounded(self.handle, x.ptr, _dtype_code(x.dtype), n, d, d,
                                          mean.ptr if mean is not None else None, std.ptr if std is not None else None,
                                          absmax.ptr if absmax is not None else None, image.ptr), self.handle)
        return image

    def kmeans_filter_scanned(self, reset: bool = False) -> int:
        """Frames that took the filter's exhaustive fp64 scan since the context was created (diagnostics)."""
        out = C.c_uint64(0)
        check(lib.msm_kmeans_filter_scanned(self.handle, C.byref(out), int(reset)), self.handle)
        return int(out.value)

    def mfma_bf16_probe(self, a_bits: np.ndarray, b_bits: np.ndarray, c: np.ndarray) -> np.ndarray:
        """D = A B + C through one v_mfma_f32_16x16x32_bf16 per tile: a_bits [t, 16, 32], b_bits [t, 32, 16] uint16
        (raw bf16 patterns), c [t, 16, 16] float32 (host arrays)."""
        return self._mfma_probe(lib.msm_mfma_bf16_probe, a_bits, b_bits, c)

    def mfma_f16_probe(self, a_bits: np.ndarray, b_bits: np.ndarray, c: np.ndarray) -> np.ndarray:
        """The same through one v_mfma_f32_16x16x32_f16 per tile (raw fp16 patterns): the hardware rule behind the
        k-means filter."""
        return self._mfma_probe(lib.msm_mfma_f16_probe, a_bits, b_bits, c)

    def _mfma_probe(self, fn, a_bits: np.ndarray, b_bits: np.ndarray, c: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(a_bits, np.uint16)
        b = np.ascontiguousarray(b_bits, np.uint16)
        cc = np.ascontiguousarray(c, np.float32)
        t = a.shape[0]
        if a.shape != (t, 16, 32) or b.shape != (t, 32, 16) or cc.shape != (t, 16, 16):
            raise ValueError("mfma probe: shapes must be [t,16,32], [t,32,16], [t,16,16]")
        out = np.empty((t, 16, 16), np.float32)
        check(fn(self.handle, a.ctypes.data, b.ctypes.data, cc.ctypes.data, out.ctypes.data, t), self.handle)
        return out

    def kmeans_lloyd_pass(self, x: DeviceArray, centers: DeviceArray, state: DeviceArray, sums: DeviceArray,
                          counts: DeviceArray, *, mean: DeviceArray | None = None, std: DeviceArray | None = None,
                          image: DeviceArray | None = None, prev_labels: DeviceArray | None = None,
                          first_pass: bool = False):
        """One Lloyd iteration on a single shard: kmeans_accumulate + kmeans_update(clear=False), in one launch where the
        filter kernel runs (msm_kmeans_lloyd_pass).  first_pass: as in kmeans_accumulate."""
        n, d = x.shape
        k = centers.shape[0]
        args = (self.handle, x.ptr, _dtype_code(x.dtype), n, d, d, centers.ptr, k,
                mean.ptr if mean is not None else None, std.ptr if std is not None else None,
                image.ptr if image is not None else None, state.ptr,
                prev_labels.ptr if prev_labels is not None else None, sums.ptr, counts.ptr)
        if first_pass:
            check(lib.msm_kmeans_lloyd_pass_from(*args, 1), self.handle)
        else:
            check(lib.msm_kmeans_lloyd_pass(*args), self.handle)

    def kmeans_lloyd_pass_deferred(self, x: DeviceArray, centers_in: DeviceArray, centers_out: DeviceArray,
                                   state: DeviceArray, acc_in, acc_out, acc_next, *, image: DeviceArray | None,
                                   prev_labels: DeviceArray, close_pending: bool, first_pass: bool = False,
                                   mean: DeviceArray | None = None, std: DeviceArray | None = None) -> bool:
        """One Lloyd pass of the deferred chain (msm_kmeans_lloyd_pass_deferred): the launch closes its predecessor's
        iteration in its prologue and ends with its own flush.  acc_* are (sums, counts) pairs: acc_in the complete sums
        of the previous pass (None on the first), acc_out zero on entry, acc_next cleared for the following launch.
        False: the flavour does not run at this shape and nothing was launched (take kmeans_lloyd_pass)."""
        n, d = x.shape
        k = centers_in.shape[0]
        applied = C.c_int32(0)
        check(lib.msm_kmeans_lloyd_pass_deferred(
            self.handle, x.ptr, _dtype_code(x.dtype), n, d, d, centers_in.ptr, centers_out.ptr, k,
            mean.ptr if mean is not None else None, std.ptr if std is not None else None,
            image.ptr if image is not None else None, state.ptr, prev_labels.ptr,
            acc_in[0].ptr if acc_in is not None else None, acc_in[1].ptr if acc_in is not None else None,
            acc_out[0].ptr, acc_out[1].ptr, acc_next[0].ptr, acc_next[1].ptr, int(close_pending), int(first_pass),
            C.byref(applied)), self.handle)
        return bool(applied.value)

    def kmeans_assign_closing(self, x: DeviceArray, centers_in: DeviceArray, centers_out: DeviceArray,
                              state: DeviceArray | None, acc_in, *, image: DeviceArray | None, labels: DeviceArray,
                              close_pending: bool, mindist: DeviceArray | None = None,
                              mean: DeviceArray | None = None, std: DeviceArray | None = None) -> bool:
        """The assignment that ends the deferred chain (msm_kmeans_assign_closing): closes the last pass's iteration in
        its prologue, leaves the final centres in centers_out.  False: not run at this shape, nothing launched."""
        n, d = x.shape
        k = centers_in.shape[0]
        applied = C.c_int32(0)
        check(lib.msm_kmeans_assign_closing(
            self.handle, x.ptr, _dtype_code(x.dtype), n, d, d, centers_in.ptr, centers_out.ptr, k,
            mean.ptr if mean is not None else None, std.ptr if std is not None else None,
            image.ptr if image is not None else None, state.ptr if state is not None else None,
            acc_in[0].ptr if acc_in is not None else None, acc_in[1].ptr if acc_in is not None else None,
            int(close_pending), labels.ptr, mindist.ptr if mindist is not None else None, C.byref(applied)), self.handle)
        return bool(applied.value)

    def kmeans_update(self, sums: DeviceArray, counts: DeviceArray, centers: DeviceArray, state: DeviceArray,
                      clear: bool = True):
        k, d = centers.shape
        check(lib.msm_kmeans_update(self.handle, sums.ptr, counts.ptr, k, d, centers.ptr, state.ptr, int(clear)),
              self.handle)

    def sum_f64(self, v: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
        out = out if out is not None else self.empty((1,), np.float64)
        check(lib.msm_sum_f64(self.handle, v.ptr, v.size, out.ptr), self.handle)
        return out


    # -- MSM estimation ---------------------------------------------------------
    def transition_matrix(self, counts: DeviceArray, *, mode: int = 0, alpha: float = 1e-3,
                          epsilon: float = 1e-12) -> dict:
        """counts [k,k] (int64 or float64) -> dict of device arrays (see msm_transition_matrix)."""
        k = counts.shape[0]
        if counts.dtype not in (np.dtype(np.int64), np.dtype(np.float64)):
            raise TypeError("counts must be int64 or float64")
        T = self.empty((k, k), np.float64)
        rowsum = self.empty((k,), np.float64)
        out = {"T": T, "rowsum": rowsum}
        if mode == 0:
            dm = self.empty((1,), np.float64)
            check(lib.msm_transition_matrix(self.handle, counts.ptr, int(counts.dtype == np.float64), k, 0, 0.0, 0.0,
                                            T.ptr, None, None, None, rowsum.ptr, dm.ptr), self.handle)
            out["diag_mass"] = dm
        else:
            active, inv = self.empty((k,), np.int32), self.empty((k,), np.int32)
            na = self.empty((1,), np.int32)
            check(lib.msm_transition_matrix(self.handle, counts.ptr, int(counts.dtype == np.float64), k, 1,
                                            float(alpha), float(epsilon), T.ptr, active.ptr, inv.ptr, na.ptr,
                                            rowsum.ptr, None), self.handle)
            out.update(active=active, inv_map=inv, n_active=na)
        return out

    def row_normalise_into(self, counts: DeviceArray, T: DeviceArray, rowsum: DeviceArray, diag_mass: DeviceArray):
        """T = counts / rowsum (zero rows stay zero), trace(T)/k: msm_transition_matrix mode 0 into given arrays."""
        k = counts.shape[0]
        check(lib.msm_transition_matrix(self.handle, counts.ptr, int(counts.dtype == np.float64), k, 0, 0.0, 0.0,
                                        T.ptr, None, None, None, rowsum.ptr, diag_mass.ptr), self.handle)

    def rcp(self, src: DeviceArray, dst: DeviceArray) -> None:
        check(lib.msm_rcp_f64(self.handle, src.ptr, src.size, dst.ptr), self.handle)

    def embed_full(self, T_active: DeviceArray, inv_map: DeviceArray, pi_active: DeviceArray | None = None):
        k = T_active.shape[0]
        T_full = self.empty((k, k), np.float64)
        pi_full = self.empty((k,), np.float64)
        check(lib.msm_embed_full(self.handle, T_active.ptr, pi_active.ptr if pi_active is not None else None,
                                 inv_map.ptr, k, T_full.ptr, pi_full.ptr), self.handle)
        return T_full, pi_full

    def silhouette(self, x_sorted: DeviceArray, offsets) -> tuple[float, DeviceArray]:
        """Mean silhouette coefficient of points sorted by cluster (cluster c = rows offsets[c]:offsets[c+1])."""
        n, d = x_sorted.shape
        off = np.ascontiguousarray(offsets, np.int64)
        samples = self.empty((n,), np.float64)
        score = self.empty((1,), np.float64)
        check(lib.msm_silhouette(self.handle, x_sorted.ptr, n, d, d, off.ctypes.data, len(off) - 1, samples.ptr, score.ptr),
              self.handle)
        return float(score.to_host()[0]), samples

    def silhouette_samples(self, x: DeviceArray, labels: DeviceArray, k: int, *,
                           max_products: int | None = None) -> tuple[float, DeviceArray]:
        """(mean silhouette coefficient, samples f64 [n] in frame order) of x f64 [n, d] under labels int32 [n] with ids
        0 .. k-1 (unused ids allowed), for any 2 <= k <= n - 1.  No launch holds more than `max_products` (i, j,
        feature) products (None: 2^36); the cut changes no bit of the result."""
        if x.dtype != np.float64 or labels.dtype != np.int32:
            raise TypeError("silhouette_samples takes float64 points and int32 labels")
        if len(x.shape) != 2 or labels.size != x.shape[0]:
            raise ValueError(f"silhouette_samples: points {x.shape} and {labels.size} labels do not match")
        n, d = x.shape
        work = self.empty((max(int(lib.msm_silhouette_workspace_bytes(n, d, int(k))), 1),), np.uint8)
        samples = self.empty((n,), np.float64)
        score = self.empty((1,), np.float64)
        check(lib.msm_silhouette_samples(self.handle, x.ptr, n, d, d, labels.ptr, int(k), work.ptr, work.nbytes,
                                         0 if max_products is None else int(max_products), samples.ptr, score.ptr),
              self.handle)
        return float(score.to_host()[0]), samples   # synchronises: the workspace is free on return

    # -- representative frames of a state -----------------------------------------------------------
    def group_by_label(self, labels: DeviceArray, k: int) -> tuple[DeviceArray, DeviceArray]:
        """(offsets int64 [k + 1], members int32 [n]): members[offsets[s]:offsets[s + 1]] are the frames with label s,
        ascending (np.where); labels outside [0, k) belong to no state."""
        n = labels.size
        offsets = self.empty((int(k) + 1,), np.int64)
        members = self.empty((n,), np.int32)
        check(lib.msm_group_by_label(self.handle, labels.ptr, n, int(k), offsets.ptr, members.ptr), self.handle)
        return offsets, members

    def state_centroids(self, x: DeviceArray, offsets: DeviceArray, members: DeviceArray,
                        weights: DeviceArray | None = None) -> tuple[DeviceArray, DeviceArray, DeviceArray]:
        """(centroid f64 [k, d], weight sum f64 [k], REP_FLAG_* bits int32 [k]) of the grouped states of x f64 [n, d]."""
        n, d = x.shape
        k = offsets.size - 1
        cen, wsum, flags = self.empty((k, d), np.float64), self.empty((k,), np.float64), self.empty((k,), np.int32)
        check(lib.msm_state_centroids(self.handle, x.ptr, n, d, d, weights.ptr if weights is not None else None, offsets.ptr,
                                      members.ptr, k, cen.ptr, wsum.ptr, flags.ptr), self.handle)
        return cen, wsum, flags

    def state_scores(self, x: DeviceArray, labels: DeviceArray, offsets: DeviceArray, members: DeviceArray,
                     h_offsets: np.ndarray, *, centroid: DeviceArray | None = None, wsum: DeviceArray | None = None,
                     weights: DeviceArray | None = None, states=None) -> DeviceArray:
        """Scores f64 laid out like `members`.  With `states` None: distance of every member to its state's centroid.
        With a list of states: the medoid score sum_j w^_j |x_i - x_j| of the members of those states (the words of
        other states are left unwritten)."""
        n, d = x.shape
        k = offsets.size - 1
        ho = np.ascontiguousarray(h_offsets, np.int64)
        scores = self.empty((n,), np.float64)
        if states is None:
            mode, hs, ns = _lib.REP_SCORE_CENTROID, None, 0
        else:
            st = np.ascontiguousarray(states, np.int32).reshape(-1)
            mode, hs, ns = _lib.REP_SCORE_MEDOID, st.ctypes.data, st.size
        check(lib.msm_state_scores(self.handle, x.ptr, n, d, d, weights.ptr if weights is not None else None, labels.ptr,
                                   offsets.ptr, members.ptr, k, centroid.ptr if centroid is not None else None,
                                   wsum.ptr if wsum is not None else None, mode, ho.ctypes.data, hs, ns, scores.ptr),
              self.handle)
        return scores

    def state_select(self, x: DeviceArray, offsets: DeviceArray, members: DeviceArray, scores: DeviceArray, states,
                     n_reps: int, *, diverse: bool = False) -> np.ndarray:
        """Picks int32 [len(states), n_reps] (frame indices, -1 past a state's size) for distinct `states`: the members
        with the smallest (score, frame), or with `diverse` the max-min walk from the member with the smallest score."""
        n, d = x.shape
        k = offsets.size - 1
        st = np.ascontiguousarray(states, np.int32).reshape(-1)
        picks = self.empty((st.size, int(n_reps)), np.int32)
        mind = self.empty((n,), np.float64) if diverse else None
        check(lib.msm_state_select(self.handle, x.ptr, n, d, d, offsets.ptr, members.ptr, k, scores.ptr,
                                   mind.ptr if diverse else None,
                                   _lib.REP_SELECT_DIVERSE if diverse else _lib.REP_SELECT_SMALLEST, st.ctypes.data, st.size,
                                   int(n_reps), picks.ptr), self.handle)
        return picks.to_host()   # synchronises: the workspace is free on return

    # -- regular-grid microstates ---------------------------------------------------------------
    def grid_cells(self, x: DeviceArray, edges: np.ndarray) -> DeviceArray:
        """Flat cell index per frame for edges [F, bins + 1] (np.digitize - 1, clipped)."""
        n, F = x.shape
        e = np.ascontiguousarray(edges, np.float64)
        if e.shape[0] != F:
            raise ValueError("edges must have one row per feature")
        flat = self.empty((n,), np.int32)
        dt = _lib.MSM_F32 if x.dtype == np.float32 else _lib.MSM_F64
        ed = self.to_device(e)
        check(lib.msm_grid_cells(self.handle, x.ptr, dt, n, F, F, ed.ptr, e.shape[1] - 1, flat.ptr), self.handle)
        self.sync()
        return flat

    def first_occurrence(self, flat: DeviceArray, n_cells: int) -> np.ndarray:
        first = self.empty((int(n_cells),), np.int64)
        check(lib.msm_first_occurrence(self.handle, flat.ptr, flat.size, int(n_cells), first.ptr), self.handle)
        return first.to_host()

    def relabel(self, flat: DeviceArray, cell_map: np.ndarray) -> DeviceArray:
        m = self.to_device(np.ascontiguousarray(cell_map, np.int32))
        labels = self.empty((flat.size,), np.int32)
        check(lib.msm_relabel(self.handle, flat.ptr, flat.size, m.ptr, m.size, labels.ptr), self.handle)
        self.sync()
        return labels

    # -- dense solves on T: committors / flux / lumping / MFPT --------------------------------
    def solve(self, A: DeviceArray, B: DeviceArray) -> int:
        """A X = B in place (A -> LU factors, B -> X); returns 0 or the 1-based singular column."""
        n = A.shape[0]
        nrhs = 1 if len(B.shape) == 1 else B.shape[1]
        info = self.empty((1,), np.int32)
        check(lib.msm_solve_f64(self.handle, n, nrhs, A.ptr, A.shape[1], B.ptr, nrhs, info.ptr), self.handle)
        return int(info.to_host()[0])

    def reactive_flux(self, T: DeviceArray, pi: DeviceArray, role: np.ndarray, want_flux: bool = True) -> dict:
        n = T.shape[0]
        rd = self.to_device(np.ascontiguousarray(role, np.int32))
        qp, qm = self.empty((n,), np.float64), self.empty((n,), np.float64)
        info = self.empty((2,), np.int32)
        gross = net = tot = None
        if want_flux:
            gross, net, tot = self.empty((n, n), np.float64), self.empty((n, n), np.float64), self.empty((4,), np.float64)
        check(lib.msm_reactive_flux(self.handle, T.ptr, n, pi.ptr, rd.ptr, n, qp.ptr, qm.ptr,
                                    gross.ptr if gross is not None else None, net.ptr if net is not None else None,
                                    tot.ptr if tot is not None else None, info.ptr), self.handle)
        return {"qplus": qp, "qminus": qm, "gross": gross, "net": net, "totals": tot, "info": info.to_host()}

    def reactive_pathways(self, net: DeviceArray, role, *, fraction: float = 0.99, maxiter: int = 10_000, keep: int = 5,
                          launch_paths: int | None = None):
        """Dominant reactive pathways through the net flux `net` f64 [n, n] on the device (reactive_flux's
        out["net"], or any finite non-negative matrix); role[i] = 0 intermediate, 1 source, 2 sink.  Returns
        (paths, caps, status): the node lists of the first `keep` paths, the capacities f64 of ALL paths found and
        one of _lib.PATHWAYS_FRACTION / PATHWAYS_NO_PATH / PATHWAYS_MAXITER (msm_reactive_pathways_* in
        include/msmhip.h has the rule).  The walk is a chain of bounded launches, at most `launch_paths` paths each
        (None: the library's default for this n); the result does not depend on that number.  last_pathway_launches
        holds the number of launches taken."""
        if len(net.shape) != 2 or net.shape[0] != net.shape[1] or net.dtype != np.float64:
            raise ValueError(f"the net flux must be a square float64 matrix, got {net.dtype} {net.shape}")
        n = net.shape[0]
        role = np.ascontiguousarray(role, np.int32).ravel()
        if role.size != n or np.any((role < 0) | (role > 2)):
            raise ValueError(f"role must hold {n} entries from {{0, 1, 2}}")
        if not np.any(role == 1) or not np.any(role == 2):
            raise ValueError("Source and sink must each contain at least one state")
        fraction, maxiter, keep = float(fraction), int(maxiter), int(keep)
        if not 0.0 < fraction <= 1.0:
            raise ValueError("fraction must be in (0, 1]")
        if maxiter < 0 or keep < 0 or (launch_paths is not None and int(launch_paths) < 1):
            raise ValueError("maxiter and keep must not be negative, launch_paths at least 1")
        work = self.empty((int(lib.msm_reactive_pathways_work_bytes(n)) // 8,), np.float64)
        caps = self.empty((max(maxiter, 1),), np.float64)
        paths, lens = self.empty((max(keep, 1), n), np.int32), self.empty((max(keep, 1),), np.int32)
        rd = self.to_device(role)
        check(lib.msm_reactive_pathways_begin(self.handle, net.ptr, n, rd.ptr, n, maxiter, keep, work.ptr, caps.ptr,
                                              paths.ptr, lens.ptr), self.handle)

        def header():
            h = work.view((32,), np.uint8).to_host()
            return int(h[16:20].view(np.int32)[0]), int(h[20:24].view(np.int32)[0]), int(h[24:28].view(np.int32)[0])

        n_paths, status, bad = header()
        if bad:
            raise ValueError("the net flux holds a negative, infinite or NaN entry")
        self.last_pathway_launches = 0
        while status == _lib.PATHWAYS_RUNNING:
            check(lib.msm_reactive_pathways_run(self.handle, work.ptr, n, fraction, maxiter, keep,
                                                0 if launch_paths is None else int(launch_paths), caps.ptr, paths.ptr,
                                                lens.ptr), self.handle)
            self.last_pathway_launches += 1
            n_paths, status, _ = header()
        kept = min(keep, n_paths)
        nodes, length = paths.to_host(), lens.to_host()
        return ([nodes[p, :length[p]].tolist() for p in range(kept)], caps.to_host()[:n_paths].copy(), status)

    def lump_macro(self, T: DeviceArray, pi: DeviceArray, macro: np.ndarray, n_macro: int):
        n = T.shape[0]
        md = self.to_device(np.ascontiguousarray(macro, np.int32))
        Tm, pm = self.empty((n_macro, n_macro), np.float64), self.empty((n_macro,), np.float64)
        check(lib.msm_lump_macro(self.handle, T.ptr, n, pi.ptr, md.ptr, n, int(n_macro), Tm.ptr, pm.ptr), self.handle)
        return Tm, pm

    def macro_mfpt(self, T: DeviceArray):
        n = T.shape[0]
        out = self.empty((n, n), np.float64)
        info = self.empty((n,), np.int32)
        check(lib.msm_macro_mfpt(self.handle, T.ptr, n, n, out.ptr, info.ptr), self.handle)
        return out, info.to_host()

    # -- trajectory bootstrap in batch ---------------------------------------------------------------
    def combine_counts(self, seg_counts: DeviceArray, mult: DeviceArray, *, seg0: int = 0, out: DeviceArray | None = None,
                       accumulate: bool = False) -> DeviceArray:
        """C_b = sum_s mult[b, seg0 + s] * seg_counts[s]: int64 [n_boot, ...] from per-trajectory counts int64
        [n_seg, ...] and the multiplicity table int32 [n_boot, >= seg0 + n_seg]; added to `out` when accumulate."""
        n_seg, n_boot, ld = seg_counts.shape[0], mult.shape[0], mult.shape[1]
        if seg_counts.dtype != np.int64 or mult.dtype != np.int32:
            raise TypeError("seg_counts must be int64 and mult int32")
        if seg0 < 0 or seg0 + n_seg > ld:
            raise ValueError("the multiplicity table has no columns for these trajectories")
        cells = seg_counts.size // n_seg
        if out is None:
            if accumulate:
                raise ValueError("accumulate needs the array to add to")
            out = self.empty((n_boot,) + tuple(seg_counts.shape[1:]), np.int64)
        for s in range(0, n_seg, _lib.COMBINE_MAX_SEG):
            m = min(_lib.COMBINE_MAX_SEG, n_seg - s)
            check(lib.msm_combine_counts(self.handle, seg_counts.ptr + 8 * s * cells, mult.ptr + 4 * (seg0 + s), ld, m,
                                         n_boot, cells, out.ptr, int(accumulate or s > 0)), self.handle)
        return out

    def row_normalise_batched(self, counts: DeviceArray, T: DeviceArray | None = None,
                              rowsum: DeviceArray | None = None) -> tuple[DeviceArray, DeviceArray]:
        """counts int64 [batch, k, k] -> T f64 [batch, k, k] = C / rowsum (zero rows stay zero), rowsum int64 [batch, k]."""
        batch, k = counts.shape[0], counts.shape[-1]
        if counts.dtype != np.int64:
            raise TypeError("counts must be int64")
        T = T if T is not None else self.empty((batch, k, k), np.float64)
        rowsum = rowsum if rowsum is not None else self.empty((batch, k), np.int64)
        check(lib.msm_row_normalise_batched(self.handle, counts.ptr, k, batch, T.ptr, rowsum.ptr), self.handle)
        return T, rowsum

    def reactive_flux_batched(self, T: DeviceArray, pi: DeviceArray, role: np.ndarray, *, want_committors: bool = True,
                              chunk_bytes: int = 1 << 30) -> dict:
        """msm_reactive_flux_batched on T [batch, n, n], pi [batch, n] and one role [n]: committors [batch, n] (or
        None), totals [batch, 4] = {F, Z, rate, mfpt} on the device, info [batch, 2] on the host.  The batch is split
        so that the solver's scratch stays within chunk_bytes (at least one sample a call); the results do not
        depend on the split."""
        batch, n = T.shape[0], T.shape[-1]
        rd = self.to_device(np.ascontiguousarray(role, np.int32))
        qp = qm = None
        if want_committors:
            qp, qm = self.empty((batch, n), np.float64), self.empty((batch, n), np.float64)
        tot = self.empty((batch, 4), np.float64)
        info = self.empty((batch, 2), np.int32)
        per_sample = int(lib.msm_reactive_flux_batched_scratch_bytes(n, 1, int(want_committors)))
        step = batch if per_sample == 0 else max(1, min(batch, int(chunk_bytes) // per_sample))
        for b in range(0, batch, step):
            m = min(step, batch - b)
            check(lib.msm_reactive_flux_batched(self.handle, T.ptr + 8 * b * n * n, n * n, n, pi.ptr + 8 * b * n, rd.ptr,
                                                n, m, qp.ptr + 8 * b * n if qp is not None else None,
                                                qm.ptr + 8 * b * n if qm is not None else None, tot.ptr + 32 * b,
                                                info.ptr + 8 * b), self.handle)
        return {"qplus": qp, "qminus": qm, "totals": tot, "info": info.to_host()}

    def bootstrap_transition_matrices(self, labels: DeviceArray, starts, stops, k: int, lag: int, mult: np.ndarray, *,
                                      chunk_bytes: int = 1 << 28) -> tuple[DeviceArray, DeviceArray]:
        """Transition matrices of trajectory resamples: T f64 [n_boot, k, k] and rowsum int64 [n_boot, k] from the
        labels of all trajectories (trajectory s = labels[starts[s]:stops[s]]) and the multiplicity table
        mult [n_boot, n_seg].  Every trajectory is counted once; a resample's counts are the integer combination.
        Neither the per-trajectory counts nor the resampled counts need fit at once: both are walked in chunks of
        at most chunk_bytes (at least one matrix), the resamples on the outside, so that with several chunks of
        both the trajectories are counted again per chunk of resamples."""
        n_boot = np.shape(mult)[0] if np.ndim(mult) == 2 else 0
        T = rowsum = None
        for b, nb, counts in self.bootstrap_counts(labels, starts, stops, k, lag, mult, chunk_bytes=chunk_bytes):
            if T is None:
                T = self.empty((n_boot, k, k), np.float64)
                rowsum = self.empty((n_boot, k), np.int64)
            self.row_normalise_batched(counts, T.view((nb, k, k), offset_elems=b * k * k),
                                       rowsum.view((nb, k), offset_elems=b * k))
        return T, rowsum

    def bootstrap_counts(self, labels: DeviceArray, starts, stops, k: int, lag: int, mult: np.ndarray, *,
                         chunk_bytes: int = 1 << 28):
        """The resampled transition counts behind bootstrap_transition_matrices, a chunk of resamples at a time:
        yields (b, nb, counts) with counts int64 [nb, k, k] the counts of samples b .. b + nb - 1.  The array is
        reused for the next chunk: consume it before advancing."""
        starts, stops = self._seg_ptrs(starts, stops)
        mult = np.ascontiguousarray(mult, np.int32)
        n_seg = len(starts)
        if mult.ndim != 2 or mult.shape[1] != n_seg or n_seg == 0 or mult.shape[0] == 0:
            raise ValueError("mult must be [n_boot, n_seg] with at least one sample and one trajectory")
        n_boot, mat = mult.shape[0], k * k * 8
        seg_step = max(1, min(n_seg, int(chunk_bytes) // mat))
        boot_step = max(1, min(n_boot, int(chunk_bytes) // mat))
        mult_d = self.to_device(mult)
        seg_counts = self.empty((seg_step, k, k), np.int64)
        counts = self.empty((boot_step, k, k), np.int64)
        counted = None                       # the chunk of trajectories seg_counts holds
        for b in range(0, n_boot, boot_step):
            nb = min(boot_step, n_boot - b)
            for s in range(0, n_seg, seg_step):
                ns = min(seg_step, n_seg - s)
                if counted != s:
                    for t in range(ns):
                        self.count_transitions(labels, k, lag, starts=starts[s + t:s + t + 1], stops=stops[s + t:s + t + 1],
                                               out=seg_counts.view((k, k), offset_elems=t * k * k))
                    counted = s
                self.combine_counts(seg_counts.view((ns, k, k)), mult_d.view((nb, n_seg), offset_elems=b * n_seg),
                                    seg0=s, out=counts.view((nb, k, k)), accumulate=s > 0)
            yield b, nb, counts.view((nb, k, k))

    # -- free-energy surfaces ---------------------------------------------------
    def weighted_stats(self, x: DeviceArray, col: int = 0, weights: DeviceArray | None = None) -> np.ndarray:
        """[sum w, sum w^2, weighted mean, weighted variance, min, max] of column `col` of x [n, d] (or of a
        1-D array); unit weights when `weights` is None."""
        if len(x.shape) == 1:
            n, stride, off = x.shape[0], 1, 0
        else:
            n, stride, off = x.shape[0], x.shape[1], int(col)
        out = self.empty((6,), np.float64)
        check(lib.msm_weighted_stats(self.handle, x.ptr + off * 8, stride, n, weights.ptr if weights is not None else None,
                                     out.ptr), self.handle)
        return out.to_host()

    def gather(self, table: DeviceArray, idx: DeviceArray) -> DeviceArray:
        """table[idx] for int32 indices (0 where the index is out of range)."""
        out = self.empty((idx.size,), np.float64)
        check(lib.msm_gather_f64(self.handle, table.ptr, table.size, idx.ptr, idx.size, out.ptr), self.handle)
        return out

    def hist2d_xy(self, x, y, xedges: np.ndarray, yedges: np.ndarray) -> DeviceArray:
        """np.histogram2d (unweighted) of two device columns on the given edges -> f64 [nx, ny].  x and y are
        (array, column) pairs for columns of 2-D arrays, or 1-D arrays."""
        def col(a):
            if isinstance(a, tuple):
                arr, c = a
                return arr.ptr + int(c) * 8, arr.shape[1], arr.shape[0]
            return a.ptr, 1, a.size
        (px, sx, n), (py, sy, _) = col(x), col(y)
        nx, ny = len(xedges) - 1, len(yedges) - 1
        xe = self.to_device(np.ascontiguousarray(xedges, np.float64))
        ye = self.to_device(np.ascontiguousarray(yedges, np.float64))
        h = self.empty((nx, ny), np.float64)
        check(lib.msm_hist2d(self.handle, px, sx, py, sy, n, None, 0.0, xe.ptr, nx, ye.ptr, ny, h.ptr), self.handle)
        return h

    def clip_or_wrap(self, x: DeviceArray, lo: float, hi: float, *, wrap: bool, col: int = 0) -> DeviceArray:
        """New 1-D array: np.clip(x, lo, hi), or ((x - lo) % (hi - lo)) + lo when wrap."""
        if len(x.shape) == 1:
            n, stride, off = x.shape[0], 1, 0
        else:
            n, stride, off = x.shape[0], x.shape[1], int(col)
        out = self.empty((n,), np.float64)
        check(lib.msm_clip_or_wrap(self.handle, x.ptr + off * 8, stride, n, float(lo), float(hi), 2 if wrap else 1,
                                   out.ptr), self.handle)
        return out

    def order_statistics(self, x: DeviceArray, ranks, col: int = 0) -> np.ndarray:
        """The ranks[q]-th smallest values (0-based) of column `col` of x [n, d] (or of a 1-D array)."""
        if len(x.shape) == 1:
            n, stride, off = x.shape[0], 1, 0
        else:
            n, stride, off = x.shape[0], x.shape[1], int(col)
        r = np.ascontiguousarray(ranks, dtype=np.int64).ravel()
        out = np.empty(r.size, dtype=np.float64)
        check(lib.msm_order_statistics(self.handle, x.ptr + off * 8, stride, n, r.ctypes.data, r.size, out.ctypes.data),
              self.handle)
        return out

    def hist2d(self, x: DeviceArray, cols, xedges: np.ndarray, yedges: np.ndarray,
               weights: DeviceArray | None = None, w_absmax: float = 0.0) -> DeviceArray:
        """np.histogram2d(x[:, cols[0]], x[:, cols[1]], bins=[xedges, yedges], weights=w) -> f64 [nx, ny]."""
        n, d = x.shape
        nx, ny = len(xedges) - 1, len(yedges) - 1
        xe, ye = self.to_device(np.ascontiguousarray(xedges, np.float64)), self.to_device(np.ascontiguousarray(yedges, np.float64))
        h = self.empty((nx, ny), np.float64)
        check(lib.msm_hist2d(self.handle, x.ptr + int(cols[0]) * 8, d, x.ptr + int(cols[1]) * 8, d, n,
                             weights.ptr if weights is not None else None, float(w_absmax), xe.ptr, nx, ye.ptr, ny, h.ptr),
              self.handle)
        return h

    def smooth_sparse_bins(self, hist: DeviceArray, min_count: float) -> tuple[DeviceArray, int]:
        nx, ny = hist.shape
        out = self.empty((nx, ny), np.float64)
        cnt = self.empty((1,), np.int32)
        check(lib.msm_smooth_sparse_bins(self.handle, hist.ptr, nx, ny, float(min_count), out.ptr, cnt.ptr), self.handle)
        return out, int(cnt.to_host()[0])

    def scale_to_total(self, v: DeviceArray, total: float) -> None:
        check(lib.msm_scale_to_total(self.handle, v.ptr, v.size, float(total)), self.handle)

    def fes_finalize(self, hist: DeviceArray, kT: float) -> tuple[DeviceArray, int]:
        F = self.empty(hist.shape, np.float64)
        st = self.empty((1,), np.int32)
        check(lib.msm_fes_finalize(self.handle, hist.ptr, hist.size, float(kT), F.ptr, st.ptr), self.handle)
        return F, int(st.to_host()[0])

    def kde2d(self, x: DeviceArray, cols, xcenters: np.ndarray, ycenters: np.ndarray, bw_x: float, bw_y: float,
              weights: DeviceArray | None, w_scale: float, periodic: int = 0) -> DeviceArray:
        """periodic: bit 0 / bit 1 wrap the x / y differences to [-pi, pi) (density on a torus)."""
        n, d = x.shape
        xc, yc = self.to_device(np.ascontiguousarray(xcenters, np.float64)), self.to_device(np.ascontiguousarray(ycenters, np.float64))
        dens = self.empty((len(xcenters), len(ycenters)), np.float64)
        check(lib.msm_kde2d(self.handle, x.ptr + int(cols[0]) * 8, d, x.ptr + int(cols[1]) * 8, d, n,
                            weights.ptr if weights is not None else None, float(w_scale), xc.ptr, len(xcenters), yc.ptr,
                            len(ycenters), float(bw_x), float(bw_y), int(periodic), dens.ptr), self.handle)
        return dens

    def gemm(self, A: DeviceArray, B: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
        """C = A . B (fp64, matrix cores; ascending-k FMA chain per element)."""
        m, k = A.shape
        k2, n = B.shape
        if k != k2:
            raise ValueError(f"gemm: inner dimensions differ ({k} vs {k2})")
        C = out if out is not None else self.empty((m, n), np.float64)
        check(lib.msm_gemm_f64(self.handle, m, n, k, A.ptr, k, B.ptr, n, C.ptr, n), self.handle)
        return C

    def ck_test(self, T1: DeviceArray, Tk: DeviceArray, factors, rowcounts: DeviceArray | None = None):
        """mse[i] = mean((T1^f_i - Tk[i])^2) and, with row counts [F, n], the multinomial noise RMS
        of Tk[i] (validation/ck_rule.py:36-63).  T1 [n, n]; Tk [F, n, n]."""
        n = T1.shape[0]
        fac = np.ascontiguousarray(factors, dtype=np.int32)
        F = int(fac.size)
        if tuple(Tk.shape) != (F, n, n):
            raise ValueError(f"ck_test: Tk must have shape ({F}, {n}, {n}), got {tuple(Tk.shape)}")
        mse = self.empty((max(F, 1),), np.float64)
        noise = self.empty((max(F, 1),), np.float64) if rowcounts is not None else None
        check(lib.msm_ck_test(self.handle, T1.ptr, n, Tk.ptr, n * n, n, n, fac.ctypes.data, F,
                              rowcounts.ptr if rowcounts is not None else None, n, mse.ptr,
                              noise.ptr if noise is not None else None), self.handle)
        return mse.to_host()[:F], (noise.to_host()[:F] if noise is not None else None)

    def matrix_power(self, T: DeviceArray, squarings: int, *, n: DeviceArray | None = None) -> DeviceArray:
        """T^(2^squarings) of one matrix [k,k] or a batch [B,k,k] (orders in `n`), msm_matrix_power."""
        B = T.shape[0] if len(T.shape) == 3 else 1
        k = T.shape[-1]
        out = self.empty(T.shape, np.float64)
        tmp = self.empty(T.shape, np.float64) if squarings > 1 else None
        check(lib.msm_matrix_power(self.handle, T.ptr, k * k, k, n.ptr if n is not None else None, k, B, int(squarings),
                                   tmp.ptr if tmp is not None else None, out.ptr), self.handle)
        return out

    def spectrum(self, T: DeviceArray, *, n: DeviceArray | None = None, n_its: int = 0, lags=None,
                 p: int | None = None, want_pi: bool = True, tol: float = 1e-9, n_iter: int = 24,
                 max_launches: int = 100, seed: int = 0, allow_unconverged: bool = False, n_vecs: int = 0,
                 n_watch: int | None = None, squarings: int | None = None) -> dict:
        """Leading Ritz values / stationary distribution / implied timescales of one matrix
        [k,k] or a batch [B,k,k] of packed row-stochastic matrices (orders in `n`, int32 [B]).
        squarings: the subspace iterations run on T^(2^squarings) (default 2 for k >= 32: a quarter of the iterations,
        the reported values are those of T itself); when a run on the power does not converge it is repeated on T."""
        if squarings is None:
            squarings = int(os.environ.get("MSM_SPEC_SQUARINGS", "2")) if T.shape[-1] >= 32 else 0
        if squarings > 0:
            # One matrix: a ramp of 6, 6, 12, 24 iterations per launch (a well-separated spectrum is done after the first
            # six on T^4: 0.69 ms at k = 200, 0.89 ms at k = 500; four sufficed at k = 500 but not at k = 200); batches: two thirds of the usual number (converged matrices are frozen between
            # launches only).  Any matrix left unconverged (or a basis T^(2^s) has made too ill-conditioned to
            # factorise: NaN) sends the whole call to the plain iteration on T below.
            B = T.shape[0] if len(T.shape) == 3 else 1
            it_pow = int(os.environ.get("MSM_SPEC_NITER", -n_iter if B == 1 else max(6, (2 * n_iter) // 3)))
            try:
                return self._spectrum(T, self.matrix_power(T, squarings, n=n), it_pow, n=n, n_its=n_its, lags=lags, p=p,
                                      want_pi=want_pi, tol=tol, max_launches=max(8, max_launches // 2), seed=seed,
                                      allow_unconverged=False, n_vecs=n_vecs, n_watch=n_watch)
            except _lib.MsmError:
                pass
        return self._spectrum(T, None, n_iter, n=n, n_its=n_its, lags=lags, p=p, want_pi=want_pi, tol=tol,
                              max_launches=max_launches, seed=seed, allow_unconverged=allow_unconverged, n_vecs=n_vecs,
                              n_watch=n_watch)

    def _spectrum(self, T: DeviceArray, Tpow: DeviceArray | None, n_iter: int, *, n, n_its, lags, p, want_pi, tol,
                  max_launches, seed, allow_unconverged, n_vecs, n_watch) -> dict:
        batched = len(T.shape) == 3
        B = T.shape[0] if batched else 1
        k = T.shape[-1]
        n_vecs = int(min(n_vecs, 32, k))
        watch = int(n_watch) if n_watch is not None else max(n_its + 1, n_vecs, 1)
        if p is None:
            p = min(32, max(watch + 6, 8))
        p = int(min(p, 32, k))
        ws_bytes = int(lib.msm_spectrum_workspace_bytes(k, p, B))
        # the solver's buffers are kept between calls of the same shape (a lag scan calls this once
        # per estimate; nine hipMallocs cost more than the solve of a small matrix); pi is returned
        # to the caller and therefore always fresh
        cache = getattr(self, "_spec_cache", None)
        key = (k, B, max(n_its, 1))
        m_its = max(n_its, 1)
        if cache is None or cache[0] != key or cache[1].size < ws_bytes:
            # the small outputs share ONE allocation [ritz B x 128 | change B | its_eig B x m | its_ts B x m | status B i32]:
            # one copy to the host at the end instead of five
            outs = self.empty((B * (129 + 2 * m_its) + (B + 1) // 2,), np.float64)
            cache = (key, self.empty((ws_bytes,), np.uint8), outs)
            self._spec_cache = cache
        _, ws, outs = cache
        o_change, o_eig, o_ts, o_status = B * 128, B * 129, B * (129 + m_its), B * (129 + 2 * m_its)
        ritz = self.wrap(outs.ptr, (B, 128), np.float64)
        change = self.wrap(outs.ptr + 8 * o_change, (B,), np.float64)
        its_eig = self.wrap(outs.ptr + 8 * o_eig, (B, m_its), np.float64)
        its_ts = self.wrap(outs.ptr + 8 * o_ts, (B, m_its), np.float64)
        status = self.wrap(outs.ptr + 8 * o_status, (B,), np.int32)
        pi = self.empty((B, k), np.float64) if want_pi else None
        vecs = self.empty((B, n_vecs, k), np.float64) if n_vecs else None
        lag_d = self.to_device(np.asarray(lags if lags is not None else np.ones(B), np.float64).reshape(B))
        launches = 0
        restart = True
        since_restart = 0
        worst = prev = float("inf")
        ramp = n_iter < 0          # negative: ramp up to |n_iter|
        n_iter_max = abs(int(n_iter))
        for launch in range(max_launches):
            n_iter = min(n_iter_max, 6 << max(0, launch - 1)) if ramp else n_iter_max
            tail = (k * k, k, n.ptr if n is not None else None, k, B, p, int(n_iter), int(restart), int(seed), watch, ws.ptr,
                    ritz.ptr, pi.ptr if pi is not None else None, k, change.ptr, status.ptr, int(n_its), lag_d.ptr,
                    its_eig.ptr, its_ts.ptr, float(tol) if B > 1 else 0.0, vecs.ptr if vecs is not None else None, n_vecs)
            if Tpow is not None:
                check(lib.msm_spectrum_powered(self.handle, T.ptr, Tpow.ptr, *tail), self.handle)
            else:
                check(lib.msm_spectrum(self.handle, T.ptr, *tail), self.handle)
            launches += 1
            restart = False
            since_restart += 1
            prev, worst = worst, float(np.max(change.to_host()))
            if os.environ.get("MSM_SPEC_TRACE") == "2":
                print(f"  launch {launches}: worst residual {worst:.3e}", file=sys.stderr)
            if worst <= tol:
                break
            if Tpow is not None and not np.isfinite(worst):
                raise _lib.MsmError("msm_spectrum: the basis broke down under the powered iteration")
            # slow convergence = the watched eigenvalues are close to lambda_{p+1}: a wider basis moves
            # that ratio down at little cost per iteration.  The decay of the worst residual between two
            # launches predicts how many more this basis needs; more than a handful -> restart with the
            # widest subspace right away (converged matrices of a batch are frozen, not re-iterated)
            if since_restart >= 2 and p < min(32, k):
                rate = worst / prev if 0.0 < prev < float("inf") else 1.0
                remaining = np.log(tol / worst) / np.log(rate) if 0.0 < rate < 1.0 else float("inf")
                if remaining > 6:
                    p = int(min(32, k))
                    ws = self.empty((int(lib.msm_spectrum_workspace_bytes(k, p, B)),), np.uint8)
                    self._spec_cache = (key, ws, outs)
                    restart, since_restart, worst = True, 0, float("inf")
        else:
            if not allow_unconverged:
                raise _lib.MsmError(
                    f"msm_spectrum: residual {worst:.3e} > {tol:.1e} after {launches} launches "
                    "(leading eigenvalues too clustered for subspace iteration)")
        host = outs.to_host()
        ch = host[o_change:o_change + B].copy()
        if os.environ.get("MSM_SPEC_TRACE"):
            print(f"msm_spectrum: B={B} k={k} p={p} powered={Tpow is not None} n_iter={n_iter} launches={launches} "
                  f"worst={worst:.2e} unconverged={int(np.sum(ch > tol))}", file=sys.stderr)
        st = host[o_status:].view(np.int32)[:B]
        if np.any(st != 0):
            raise _lib.MsmError(f"msm_spectrum: hqr did not converge (status {st.tolist()})")
        r = host[:B * 128].reshape(B, 128)
        out = {"ritz": r[:, :32] + 1j * r[:, 32:64], "p": p, "launches": launches, "residual": ch, "pi": pi, "vecs": vecs}
        if n_its:
            out["its_eig"] = host[o_eig:o_eig + B * m_its].reshape(B, m_its).copy()
            out["its_ts"] = host[o_ts:o_ts + B * m_its].reshape(B, m_its).copy()
        return out


    def sample_transition_matrices(self, counts: DeviceArray, active: DeviceArray, n_active: DeviceArray, *,
                                   alpha: float, seed: int, n_samples: int, first_sample: int = 0,
                                   out: DeviceArray | None = None) -> DeviceArray:
        """n_samples posterior draws [n_samples, k, k] (packed active blocks) of a mode-1 estimate."""
        k = counts.shape[-1]
        if out is None:
            out = self.empty((int(n_samples), k, k), np.float64)
        done = 0
        while done < n_samples:                       # grid.y limit: 65535 samples per launch
            m = min(65535, n_samples - done)
            check(lib.msm_sample_transition_matrices(
                self.handle, counts.ptr, int(counts.dtype == np.float64), k, active.ptr, n_active.ptr, float(alpha),
                int(seed) & (2 ** 64 - 1), int(first_sample + done), m, out.ptr + done * k * k * 8, k * k, k),
                self.handle)
            done += m
        return out

    def reversible_mle(self, counts: DeviceArray, *, maxerr: float = 1e-8, maxiter: int = 1_000_000) -> dict:
        """Reversible maximum-likelihood T and pi of a connected f64 count matrix [n, n]."""
        import ctypes

        n = counts.shape[0]
        T, pi = self.empty((n, n), np.float64), self.empty((n,), np.float64)
        it, err = ctypes.c_int(0), ctypes.c_double(0.0)
        check(lib.msm_reversible_mle(self.handle, counts.ptr, n, counts.shape[1], float(maxerr), int(maxiter), T.ptr, n,
                                     pi.ptr, ctypes.byref(it), ctypes.byref(err)), self.handle)
        return {"T": T, "pi": pi, "iterations": it.value, "err": err.value}

    def reversible_mle_batched(self, counts: DeviceArray, *, alpha: float = 1e-3, maxerr: float = 1e-8,
                               maxiter: int = 1_000_000, chunk_bytes: int = 1 << 30) -> dict:
        """msm_reversible_mle_batched on raw int64 counts [batch, k, k]: per matrix the active set, the reversible
        estimate of counts[active, active] + alpha and its stationary vector.  On the device: T f64 [batch, k, k]
        (the n_active x n_active block packed top-left, zeros around it: what spectrum() takes with n=n_active),
        pi f64 [batch, k], active int32 [batch, k] (-1 padding), n_active int32 [batch]; on the host: iterations
        int32 [batch] and err f64 [batch] (inf: a negative count or a NaN iterate).  Above the LDS boundary the batch
        is split so that the scratch stays within chunk_bytes; the results do not depend on the split."""
        if counts.dtype != np.int64 or len(counts.shape) != 3 or counts.shape[1] != counts.shape[2]:
            raise TypeError("counts must be int64 [batch, k, k]")
        batch, k = counts.shape[0], counts.shape[-1]
        T, pi = self.empty((batch, k, k), np.float64), self.empty((batch, k), np.float64)
        active, n_active = self.empty((batch, k), np.int32), self.empty((batch,), np.int32)
        its, err = self.empty((batch,), np.int32), self.empty((batch,), np.float64)
        per_sample = int(lib.msm_reversible_mle_batched_scratch_bytes(k, 1))
        step = batch if per_sample == 0 else max(1, min(batch, int(chunk_bytes) // per_sample))
        for b in range(0, batch, step):
            m = min(step, batch - b)
            check(lib.msm_reversible_mle_batched(self.handle, counts.ptr + 8 * b * k * k, k, m, float(alpha), float(maxerr),
                                                 int(maxiter), T.ptr + 8 * b * k * k, k * k, k, pi.ptr + 8 * b * k,
                                                 active.ptr + 4 * b * k, n_active.ptr + 4 * b, its.ptr + 4 * b,
                                                 err.ptr + 8 * b), self.handle)
        return {"T": T, "pi": pi, "active": active, "n_active": n_active, "iterations": its.to_host(),
                "err": err.to_host()}

    def kis_scores(self, vecs: DeviceArray, pi: DeviceArray, active: DeviceArray, n_active: DeviceArray,
                   k_slow: int) -> tuple[DeviceArray, np.ndarray]:
        """msm_kis_scores: scores f64 [batch, k] on the device (pi * sum of squares of the left eigenvectors
        1 .. k_slow of spectrum()'s vecs [batch, n_vecs, k], scattered through active; 0 at inactive states) and
        info int32 [batch] on the host (1: n_active <= k_slow, 2: a needed vector is a complex pair)."""
        batch, n_vecs, k = vecs.shape
        if tuple(pi.shape) != (batch, k) or tuple(active.shape) != (batch, k) or n_active.size != batch:
            raise ValueError("kis_scores: pi and active must be [batch, k] and n_active [batch]")
        if active.dtype != np.int32 or n_active.dtype != np.int32:
            raise TypeError("active and n_active must be int32")
        scores, info = self.empty((batch, k), np.float64), self.empty((batch,), np.int32)
        check(lib.msm_kis_scores(self.handle, vecs.ptr, n_vecs, k, batch, pi.ptr, active.ptr, n_active.ptr, int(k_slow),
                                 scores.ptr, info.ptr), self.handle)
        return scores, info.to_host()

    def active_counts(self, counts: DeviceArray, active: DeviceArray, n_active: DeviceArray, n: int, *,
                      alpha: float) -> DeviceArray:
        """counts[active, active] + alpha as a contiguous f64 [n, n] (n = the host copy of n_active): the regularised
        active-set counts of ensure_connected_counts, built on the device from msm_transition_matrix mode 1's outputs."""
        out = self.empty((int(n), int(n)), np.float64)
        check(lib.msm_active_counts(self.handle, counts.ptr, int(counts.dtype == np.float64), counts.shape[-1],
                                    active.ptr, n_active.ptr, float(alpha), out.ptr), self.handle)
        return out

    def sample_reversible_transition_matrices(self, counts: DeviceArray, *, seed: int, n_samples: int,
                                              n_sweeps: int | None = None, first_sample: int = 0,
                                              out: DeviceArray | None = None, want_pi: bool = False):
        """n_samples draws [n_samples, n, n] of the reversible posterior of a connected f64 count matrix [n, n]
        (prior already added), one independent chain per sample started from reversible_mle(counts), which this runs
        itself.  n_sweeps=None takes 2 * ceil(sqrt(n)) + 10 sweeps per chain: this engine's own choice (the chains start
        at the posterior mode and every off-diagonal update is a mode-fitted independence proposal, so the burn-in is
        short; tests/test_gpu_revposterior.py checks it against four times as many).  want_pi: returns (T, pi) with
        the stationary vectors [n_samples, n] of the samples.  out [n_samples, m, m] with m >= n receives the samples
        packed in the top-left n x n corners (the layout spectrum() takes with `n`)."""
        n = counts.shape[0]
        if n_sweeps is None:
            n_sweeps = 2 * int(np.ceil(np.sqrt(n))) + 10
        if out is None:
            out = self.empty((int(n_samples), n, n), np.float64)
        ldt = out.shape[-1]                           # a wider `out` takes the samples packed in its top-left corner
        stride = out.shape[-2] * ldt
        pi = self.empty((int(n_samples), n), np.float64) if want_pi else None
        mle = self.reversible_mle(counts)
        done = 0
        while done < n_samples:                       # per-launch limit, as sample_transition_matrices
            m = min(65535, n_samples - done)
            check(lib.msm_sample_reversible_transition_matrices(
                self.handle, counts.ptr, n, counts.shape[1], mle["T"].ptr, mle["pi"].ptr, int(seed) & (2 ** 64 - 1),
                int(first_sample + done), m, int(n_sweeps), out.ptr + done * stride * 8, stride, ldt,
                pi.ptr + done * n * 8 if pi is not None else None), self.handle)
            done += m
        return (out, pi) if want_pi else out

    def diff_norms(self, P: DeviceArray, Q: DeviceArray) -> np.ndarray:
        """[sum |P - Q|, sum |Q|, sum (P - Q)^2] of two f64 matrices of one shape."""
        n, m = P.shape
        out = self.empty((3,), np.float64)
        check(lib.msm_diff_norms(self.handle, P.ptr, m, Q.ptr, Q.shape[1], n, m, out.ptr), self.handle)
        return out.to_host()

    def philox4x32(self, key: int, counter) -> np.ndarray:
        import ctypes

        out = self.empty((4,), np.uint32)
        c = (ctypes.c_uint32 * 4)(*[int(v) & 0xFFFFFFFF for v in counter])
        check(lib.msm_philox4x32(self.handle, int(key) & (2 ** 64 - 1), c, out.ptr), self.handle)
        return out.to_host()


_ENGINES: dict[int, Engine] = {}


def get_engine(device: int = 0) -> Engine:
    """Process-wide engine per device (operator shims share it)."""
    eng = _ENGINES.get(device)
    if eng is None or not eng.handle:
        eng = Engine(device)
        _ENGINES[device] = eng
    return eng
