"""The volume operations of the C ABI (svr_region_*, svr_volume_*, svr_mesh_*, svr_overlay_*, svr_resample_grid_*, svr_histogram_*) for
Python: the methods that host.Device inherits from VolumeOps, and the module functions on the library's host code.

Every method that stages operands does so in one scope, `with self._staging() as s:`.  The scope uploads host operands, allocates the
outputs the caller did not give and frees all of it when the method leaves, whether it returns or raises.  One rule for results: host data
is read back with to_host (svr_memcpy_d2h waits for the stream); a device pointer is returned only after synchronize().

VolumeOps needs only lib, check, malloc, free, to_host, to_device and synchronize of self.  host.py re-exports every public name."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import abi
from .abi import cudaVolume
from .host import SvrError, _host_call, _to_vec3          # host.py defines these three before it imports this module


def region_mask_words(shape) -> int:
    """svr_region_mask_words of a [nz][ny][nx] volume."""
    nz, ny, nx = shape
    return ((nx + 31) // 32) * ny * nz


def region_mask_unpack(words: np.ndarray, shape) -> np.ndarray:
    """The bit mask of svr_region_grow (uint32 words) as a bool array [nz][ny][nx]."""
    nz, ny, nx = shape
    wx = (nx + 31) // 32
    b = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8).reshape(nz, ny, wx * 4), axis=-1, bitorder="little")
    return b[:, :, :nx].astype(bool)


def region_mask_pack(mask: np.ndarray) -> np.ndarray:
    """A bool array [nz][ny][nx] as the bit mask of the region calls: uint32 words, padding bits 0."""
    nz, ny, nx = mask.shape
    wx = (nx + 31) // 32
    padded = np.zeros((nz, ny, wx * 32), dtype=np.uint8)
    padded[:, :, :nx] = mask
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32))


# noun of an operand: (a host array that is not three-dimensional, a device pointer without shape=)
_SHAPE_ERRORS = {
    "volume": ("the volume must be [nz][ny][nx]", "a device volume needs shape=(nz, ny, nx)"),
    "mask": ("a mask must be [nz][ny][nx]", "a device mask needs shape=(nz, ny, nx)"),
    "labels": ("the labels must be [nz][ny][nx]", "device labels need shape=(nz, ny, nx)"),
}


def _shape_of(noun, operands, shape=None, like=None):
    """(nz, ny, nx) of an operand, or of the first host array among several: a host array's own shape goes over shape=, a device pointer
    needs shape= (or `like`).  like: the shape of the operand it belongs to -- the volume of a label map or the other way round."""
    for a in operands if isinstance(operands, tuple) else (operands,):
        if isinstance(a, np.ndarray):
            shape = a.shape
            break
    else:
        shape = shape if shape is not None else like
    rank, missing = _SHAPE_ERRORS[noun]
    if shape is None:
        raise ValueError(missing)
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3:
        raise ValueError(rank)
    if like is not None and shape != tuple(like):
        raise ValueError("the volume and the labels differ in shape")
    return shape


def _ptr(buf):
    return None if buf is None else C.c_void_p(buf)


def _i32x3(v):
    return None if v is None else (C.c_int32 * 3)(*[int(t) for t in v])


def _dims(shape):
    return _i32x3(shape[::-1])


def _u32s(v, n):
    return None if v is None else (C.c_uint32 * n)(*[int(t) for t in v])


def _xyz(seeds):
    xyz = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
    return xyz, xyz.ctypes.data_as(C.POINTER(C.c_int32))


def _voxels(shape) -> int:
    return int(shape[0]) * int(shape[1]) * int(shape[2])


class _Staging:
    """The temporary device memory of one volume-op call: everything alloc, upload, mask, map and out allocate is freed on exit, last
    first, whether the body returned or raised.  source / mask / map give the pointer argument of the C call; alloc / upload / out give
    the address as an int."""

    def __init__(self, dev):
        self.dev, self.owned, self.keep = dev, [], []

    def __enter__(self):
        return self

    def __exit__(self, etype, exc, tb):
        failed = None
        while self.owned:
            try:
                self.dev.free(self.owned.pop())
            except Exception as e:                            # go on freeing; an exception on its way out stays the one that is seen
                failed = failed or e
        if failed is not None and etype is None:
            raise failed

    def alloc(self, nbytes: int) -> int:
        self.owned.append(self.dev.malloc(nbytes))
        return self.owned[-1]

    def upload(self, array, floor: int = 1) -> int:
        """Any array in a buffer of at least `floor` bytes."""
        a = np.ascontiguousarray(array)
        buf = self.alloc(max(a.nbytes, floor))
        if a.nbytes:
            self.dev.to_device(buf, a)
        return buf

    def source(self, vox, shape=None, like=None):
        """The u16 source volume, a host [nz][ny][nx] array (kept alive until exit) or a device pointer with `shape`: (pointer argument,
        (nz, ny, nx), src_is_device)."""
        shape = _shape_of("volume", vox, shape, like)
        if not isinstance(vox, np.ndarray):
            return C.c_void_p(int(vox)), shape, 1
        self.keep.append(np.ascontiguousarray(vox, dtype=np.uint16))
        return self.keep[-1].ctypes.data_as(C.c_void_p), shape, 0

    def mask(self, mask, shape):
        """A bit mask of the (nz, ny, nx) = shape volume: a bool array (packed and uploaded) or a device pointer; None stays None."""
        if isinstance(mask, np.ndarray):
            return C.c_void_p(self.upload(region_mask_pack(mask.reshape(shape)), 4))
        return None if mask is None else C.c_void_p(int(mask))

    def map(self, a, shape=None, like=None):
        """A uint32 map (labels, zones, squared distances), a host [nz][ny][nx] array (uploaded) or a device pointer with `shape`:
        (pointer argument, (nz, ny, nx))."""
        shape = _shape_of("labels", a, shape, like)
        if isinstance(a, np.ndarray):
            return C.c_void_p(self.upload(np.ascontiguousarray(a, dtype=np.uint32), 4)), shape
        return C.c_void_p(int(a)), shape

    def out(self, nbytes: int, out_ptr=None, wanted: bool = True):
        """The output buffer: the caller's out_ptr, else nbytes fresh bytes, else (not wanted) None."""
        if out_ptr is not None:
            return out_ptr
        return self.alloc(nbytes) if wanted else None

    def mask_out(self, shape, out_ptr=None):
        return self.out(4 * max(region_mask_words(shape), 1), out_ptr)

    def array(self, buf, shape, dtype):
        """The array result in buf: read back when the scope owns buf (None stays None); else buf is the caller's and is returned itself,
        once the work on it is complete."""
        if buf is None or buf in self.owned:
            return None if buf is None else self.dev.to_host(buf, shape, dtype)
        self.dev.synchronize()
        return buf

    def mask_result(self, buf, shape) -> np.ndarray:
        """The bit mask in buf as a bool array [nz][ny][nx], also when buf is the caller's."""
        return region_mask_unpack(self.dev.to_host(buf, (region_mask_words(shape),), np.uint32), shape)


class VolumeOps:
    """The volume-op methods of host.Device."""

    def _staging(self) -> _Staging:
        return _Staging(self)

    def _last_ms(self, fn, n: int = 1):
        ms = [C.c_float(0.0) for _ in range(n)]
        self.check(fn(*[C.byref(t) for t in ms]))
        return float(ms[0].value) if n == 1 else tuple(float(t.value) for t in ms)

    # ---- seeded region growing (svr_region_*): pick, segment, measure, show ----
    def region_params(self, lo: int = 0, hi: int = 65535, connectivity: int = 6, box=None, max_sweeps: int = 0) -> abi.RegionParams:
        """svr_region_params_default with the window, connectivity, box ((x0, y0, z0), (x1, y1, z1), inclusive) and cap replaced."""
        p = abi.RegionParams()
        self.check(self.lib.svr_region_params_default(C.byref(p)))
        p.lo, p.hi, p.connectivity, p.max_sweeps = int(lo), int(hi), int(connectivity), int(max_sweeps)
        if box is not None:
            for a in range(3):
                p.box_min[a], p.box_max[a] = int(box[0][a]), int(box[1][a])
        return p

    def region_grow(self, vox, seeds, lo: int, hi: int, connectivity: int = 6, box=None, max_sweeps: int = 0, shape=None,
                    mask_ptr: Optional[int] = None):
        """svr_region_grow: the connected component(s) of {lo <= v <= hi} (inside `box`) around the seed voxels (x, y, z).  vox is a
        host [nz][ny][nx] u16 array, or a device pointer with shape=(nz, ny, nx).  Returns (mask, stats): the region as a bool array
        [nz][ny][nx] and the svr_region_stats.  mask_ptr: a device buffer of region_mask_words(shape) uint32 that receives the bit mask
        (else a temporary one is used)."""
        with self._staging() as s:
            src, shape, on_dev = s.source(vox, shape)
            nz, ny, nx = shape
            xyz, seeds_ptr = _xyz(seeds)
            p, st = self.region_params(lo, hi, connectivity, box, max_sweeps), abi.RegionStats()
            out = s.mask_out(shape, mask_ptr)
            self.check(self.lib.svr_region_grow(src, nx, ny, nz, on_dev, seeds_ptr, len(xyz), C.byref(p), C.c_void_p(out), C.byref(st)))
            return s.mask_result(out, shape), st

    def region_stats_of(self, vox, mask, shape=None) -> abi.RegionStats:
        """svr_region_stats_of: the statistics of any mask (a bool array [nz][ny][nx], or a device pointer to the bit mask)."""
        with self._staging() as s:
            src, shape, on_dev = s.source(vox, shape)
            nz, ny, nx = shape
            st = abi.RegionStats()
            self.check(self.lib.svr_region_stats_of(src, nx, ny, nz, on_dev, s.mask(mask, shape), C.byref(st)))
            return st

    def region_apply(self, vox, mask, mode: int = abi.REGION_KEEP, fill: int = 0, shape=None, out_ptr: Optional[int] = None):
        """svr_region_apply: the volume with the voxels outside (REGION_KEEP) or inside (REGION_REMOVE) the region set to `fill`.
        Returns a u16 array [nz][ny][nx]; with out_ptr (a device buffer of nx * ny * nz u16, which may be a device `vox` itself) the
        result stays on the device and out_ptr is returned."""
        with self._staging() as s:
            src, shape, on_dev = s.source(vox, shape)
            nz, ny, nx = shape
            buf, out = s.mask(mask, shape), s.out(2 * nx * ny * nz, out_ptr)
            self.check(self.lib.svr_region_apply(src, nx, ny, nz, on_dev, buf, int(mode), int(fill), C.c_void_p(out)))
            return s.array(out, shape, np.uint16)

    def region_measure(self, stats: abi.RegionStats, spacing=(1.0, 1.0, 1.0)) -> abi.RegionMeasurement:
        """svr_region_measure: volume, mean, standard deviation, centroid (voxel indices) and surface area from the integer statistics."""
        m = abi.RegionMeasurement()
        sp = (C.c_double * 3)(*[float(t) for t in spacing])
        self.check(self.lib.svr_region_measure(C.byref(stats), sp, C.byref(m)))
        return m

    # ---- operations on region masks (svr_region_morph / _combine / _reconstruct / _fill_holes / _detach) ----
    # masks: bool arrays [nz][ny][nx] (uploaded) or device pointers with shape=(nz, ny, nx); out_ptr: a device buffer of
    # region_mask_words(shape) uint32 that receives the bit mask (else a temporary one is used).  The result is the bool array.
    def region_morph(self, mask, op: int, element: int = 6, radius: int = 1, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_morph: MORPH_DILATE / _ERODE / _OPEN / _CLOSE of a mask by the unit element 6 / 18 / 26 applied `radius` times."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", mask, shape)
            buf, out = s.mask(mask, shape), s.mask_out(shape, out_ptr)
            self.check(self.lib.svr_region_morph(buf, nx, ny, nz, int(op), int(element), int(radius), C.c_void_p(out)))
            return s.mask_result(out, shape)

    def region_combine(self, a, b, op: int, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_combine: MASK_AND / _OR / _ANDNOT (a & ~b) / _XOR of two masks, or MASK_NOT of a (b = None).  out_ptr may be a or b."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", (a, b), shape)
            abuf, bbuf, out = s.mask(a, shape), s.mask(b, shape), s.mask_out(shape, out_ptr)
            self.check(self.lib.svr_region_combine(abuf, bbuf, nx, ny, nz, int(op), C.c_void_p(out)))
            return s.mask_result(out, shape)

    def region_reconstruct(self, marker, cand, connectivity: int = 6, max_sweeps: int = 0, shape=None, out_ptr: Optional[int] = None):
        """svr_region_reconstruct: the components of `cand` that hold a voxel of marker & cand.  Returns (mask, sweeps)."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", (marker, cand), shape)
            mbuf, cbuf, out = s.mask(marker, shape), s.mask(cand, shape), s.mask_out(shape, out_ptr)
            sweeps = C.c_uint32(0)
            self.check(self.lib.svr_region_reconstruct(mbuf, cbuf, nx, ny, nz, int(connectivity), int(max_sweeps), C.c_void_p(out), C.byref(sweeps)))
            return s.mask_result(out, shape), int(sweeps.value)

    def region_fill_holes(self, mask, background_connectivity: int = 6, max_sweeps: int = 0, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_fill_holes: the mask and every background voxel that cannot reach a face of the volume."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", mask, shape)
            buf, out = s.mask(mask, shape), s.mask_out(shape, out_ptr)
            self.check(self.lib.svr_region_fill_holes(buf, nx, ny, nz, int(background_connectivity), int(max_sweeps), C.c_void_p(out)))
            return s.mask_result(out, shape)

    def region_detach(self, mask, seeds, element: int = 6, radius: int = 1, connectivity: int = 6, max_sweeps: int = 0, shape=None,
                      out_ptr: Optional[int] = None):
        """svr_region_detach: the part of a grown region around the seed voxels (x, y, z) that survives an opening by `element` applied
        `radius` times -- what hangs on it by thinner connections is cut off.  Returns (mask, status): REGION_STATUS_OK or _EMPTY."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", mask, shape)
            xyz, seeds_ptr = _xyz(seeds)
            buf, out, status = s.mask(mask, shape), s.mask_out(shape, out_ptr), C.c_int32(0)
            self.check(self.lib.svr_region_detach(buf, nx, ny, nz, seeds_ptr, len(xyz), int(element), int(radius), int(connectivity), int(max_sweeps),
                                                  C.c_void_p(out), C.byref(status)))
            return s.mask_result(out, shape), int(status.value)

    # ---- connected components of region masks (svr_region_threshold / _label / _label_table / _select / _select_by_size) ----
    def region_threshold(self, vox, lo: int, hi: int, box=None, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_threshold: the mask {voxel in `box` : lo <= v <= hi} of a host [nz][ny][nx] u16 array or a device pointer with
        shape=(nz, ny, nx); box = ((x0, y0, z0), (x1, y1, z1)), inclusive, or None for the whole volume.  Returns the bool array."""
        with self._staging() as s:
            src, shape, on_dev = s.source(vox, shape)
            nz, ny, nx = shape
            b0, b1 = (None, None) if box is None else (_i32x3(box[0]), _i32x3(box[1]))
            out = s.mask_out(shape, out_ptr)
            self.check(self.lib.svr_region_threshold(src, nx, ny, nz, on_dev, int(lo), int(hi), b0, b1, C.c_void_p(out)))
            return s.mask_result(out, shape)

    def region_label(self, mask, connectivity: int = 6, shape=None, out_ptr: Optional[int] = None):
        """svr_region_label: the connected components of a mask (a bool array [nz][ny][nx], or a device pointer with shape=) under
        connectivity 6 / 18 / 26, numbered 1 .. K by their first voxel.  Returns (labels, K): a uint32 array [nz][ny][nx], or out_ptr
        itself when a device buffer of 4 nx ny nz bytes is given."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", mask, shape)
            buf, out, k = s.mask(mask, shape), s.out(4 * max(_voxels(shape), 1), out_ptr), C.c_uint32(0)
            self.check(self.lib.svr_region_label(buf, nx, ny, nz, int(connectivity), C.c_void_p(out), C.byref(k)))
            return s.array(out, shape, np.uint32), int(k.value)

    def region_label_table(self, labels, count: int, vox=None, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_label_table: the svr_region_component of the labels 1 .. count as a numpy structured array (COMPONENT_DTYPE),
        indexed by label - 1.  labels: a uint32 array [nz][ny][nx] or a device pointer with shape=; vox (optional, for `sum`): a host
        u16 array or a device pointer of the same shape.  out_ptr: a device buffer of 40 * count bytes that receives the table."""
        with self._staging() as s:
            lbuf, shape = s.map(labels, shape)
            nz, ny, nx = shape
            src, _, on_dev = (None, shape, 0) if vox is None else s.source(vox, like=shape)
            out = s.out(40 * max(int(count), 1), out_ptr)
            self.check(self.lib.svr_region_label_table(lbuf, src, nx, ny, nz, on_dev, int(count), C.c_void_p(out)))
            return self.to_host(out, (int(count),), COMPONENT_DTYPE)

    def region_select(self, labels, count: int, keep, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_select: the mask of the voxels whose label has a non-zero entry in keep (count + 1 entries, indexed by label; entry
        0 is ignored)."""
        with self._staging() as s:
            lbuf, shape = s.map(labels, shape)
            nz, ny, nx = shape
            k = np.ascontiguousarray(keep, dtype=np.uint8).reshape(-1)
            if len(k) != int(count) + 1:
                raise ValueError("keep must have count + 1 entries")
            kbuf, out = s.upload(k), s.mask_out(shape, out_ptr)
            self.check(self.lib.svr_region_select(lbuf, nx, ny, nz, int(count), C.c_void_p(kbuf), C.c_void_p(out)))
            return s.mask_result(out, shape)

    def region_select_by_size(self, labels, count: int, table=None, min_voxels: int = 0, largest_k: int = 0, shape=None,
                              out_ptr: Optional[int] = None):
        """svr_region_select_by_size: the components with at least min_voxels voxels among the largest_k largest (0 = no limit; ties go
        to the lower label).  table: the structured array of region_label_table, a device pointer to it, or None (it is computed).
        Returns (mask, kept)."""
        with self._staging() as s:
            lbuf, shape = s.map(labels, shape)
            nz, ny, nx = shape
            if table is None:
                tbuf = s.alloc(40 * max(int(count), 1))
                self.region_label_table(lbuf.value, count, shape=shape, out_ptr=tbuf)
            elif isinstance(table, np.ndarray):
                tbuf = s.upload(np.ascontiguousarray(table, dtype=COMPONENT_DTYPE), 40)
            else:
                tbuf = int(table)
            out, kept = s.mask_out(shape, out_ptr), C.c_uint32(0)
            self.check(self.lib.svr_region_select_by_size(lbuf, nx, ny, nz, int(count), C.c_void_p(tbuf), int(min_voxels), int(largest_k),
                                                          C.c_void_p(out), C.byref(kept)))
            return s.mask_result(out, shape), int(kept.value)

    def region_label_last_ms(self) -> float:
        return self._last_ms(self.lib.svr_region_label_last_ms)

    # ---- exact Euclidean distance maps and ball morphology (svr_region_distance / _distance_select / _ball / _distance_max / _distance_volume) ----
    def region_distance(self, mask, shape=None, weights=None, target: int = abi.DIST_TO_SET, out_ptr: Optional[int] = None):
        """svr_region_distance: the exact squared distance, under the integer weights (wx, wy, wz) (None = 1, 1, 1), of every voxel to the
        nearest set voxel (DIST_TO_SET) or to the nearest unset voxel of the volume (DIST_TO_UNSET); DIST_NONE everywhere when there is
        none.  mask: a bool array [nz][ny][nx], or a device pointer with shape=.  Returns a uint32 array [nz][ny][nx], or out_ptr itself
        when a device buffer of 4 nx ny nz bytes is given."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", mask, shape)
            buf, out = s.mask(mask, shape), s.out(4 * max(_voxels(shape), 1), out_ptr)
            self.check(self.lib.svr_region_distance(buf, nx, ny, nz, _u32s(weights, 3), int(target), C.c_void_p(out)))
            return s.array(out, shape, np.uint32)

    def region_distance_select(self, d2, lo2: int, hi2: int, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_distance_select: the mask of the voxels with lo2 <= d2 <= hi2.  d2: a uint32 array [nz][ny][nx] or a device pointer
        with shape=."""
        with self._staging() as s:
            dbuf, shape = s.map(d2, shape)
            nz, ny, nx = shape
            out = s.mask_out(shape, out_ptr)
            self.check(self.lib.svr_region_distance_select(dbuf, nx, ny, nz, int(lo2), int(hi2), C.c_void_p(out)))
            return s.mask_result(out, shape)

    def region_ball(self, mask, op: int, r2: int, weights=None, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_ball: MORPH_DILATE / _ERODE / _OPEN / _CLOSE of a mask by the ball {offset : weighted d^2 <= r2}."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", mask, shape)
            buf, out = s.mask(mask, shape), s.mask_out(shape, out_ptr)
            self.check(self.lib.svr_region_ball(buf, nx, ny, nz, int(op), _u32s(weights, 3), int(r2), C.c_void_p(out)))
            return s.mask_result(out, shape)

    def region_distance_max(self, d2, mask=None, shape=None):
        """svr_region_distance_max: (max_d2, first_index, status) over the voxels of `mask` (a bool array or a device pointer; None = all
        voxels): the largest value other than DIST_NONE and the smallest linear voxel index that attains it; status REGION_STATUS_EMPTY
        when there is no such voxel."""
        with self._staging() as s:
            dbuf, shape = s.map(d2, shape)
            nz, ny, nx = shape
            m, first, status = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
            self.check(self.lib.svr_region_distance_max(dbuf, s.mask(mask, shape), nx, ny, nz, C.byref(m), C.byref(first), C.byref(status)))
            return int(m.value), int(first.value), int(status.value)

    def region_distance_volume(self, d2, scale: int = 1, shape=None, out_ptr: Optional[int] = None):
        """svr_region_distance_volume: min(65535, isqrt(d2 scale^2)) as a u16 array [nz][ny][nx] (DIST_NONE gives 65535); with out_ptr (a
        device buffer of nx * ny * nz u16) the result stays on the device and out_ptr is returned."""
        with self._staging() as s:
            dbuf, shape = s.map(d2, shape)
            nz, ny, nx = shape
            out = s.out(2 * max(_voxels(shape), 1), out_ptr)
            self.check(self.lib.svr_region_distance_volume(dbuf, nx, ny, nz, int(scale), C.c_void_p(out)))
            return s.array(out, shape, np.uint16)

    def region_distance_last_ms(self) -> float:
        return self._last_ms(self.lib.svr_region_distance_last_ms)

    def region_distance_pass_ms(self):
        """(rows, y, z) HIP-event times of the passes of the last transform."""
        return self._last_ms(self.lib.svr_region_distance_pass_ms, 3)

    # ---- geodesic distances, influence zones and splitting (svr_region_geodesic / _seed_labels / _split / _zone_cut) ----
    def region_geodesic(self, labels, domain, shape=None, step_weights=None, max_sweeps: int = 0, want_dist: bool = True, want_zones: bool = True,
                        dist_ptr: Optional[int] = None, zones_ptr: Optional[int] = None):
        """svr_region_geodesic: (dist, zones, sweeps) inside `domain` (a bool array [nz][ny][nx], or a device pointer with shape=) from the
        voxels whose entry in `labels` (a uint32 array or a device pointer) is non-zero: the cost of the cheapest path of moves with the
        seven step weights (x, y, z, xy, xz, yz, xyz; 0 forbids a class; None = 3, 3, 3, 4, 4, 4, 5) and the smallest label that attains it.
        GEO_NONE / 0 where no marker reaches.  An output that is not wanted is None; with dist_ptr / zones_ptr (device buffers of
        4 nx ny nz bytes; zones_ptr may be the labels' own pointer) the result stays on the device and the pointer is returned."""
        with self._staging() as s:
            lbuf, shape = s.map(labels, domain.shape if isinstance(domain, np.ndarray) else shape)
            nz, ny, nx = shape
            mbuf, nbytes, sweeps = s.mask(domain, shape), 4 * max(_voxels(shape), 1), C.c_uint32(0)
            dout, zout = s.out(nbytes, dist_ptr, want_dist), s.out(nbytes, zones_ptr, want_zones)
            self.check(self.lib.svr_region_geodesic(lbuf, mbuf, nx, ny, nz, _u32s(step_weights, 7), int(max_sweeps), _ptr(dout), _ptr(zout), C.byref(sweeps)))
            return s.array(dout, shape, np.uint32), s.array(zout, shape, np.uint32), int(sweeps.value)

    def region_seed_labels(self, seeds, shape, out_ptr: Optional[int] = None):
        """svr_region_seed_labels: a zero uint32 array [nz][ny][nx] with the label i + 1 on the voxel (x, y, z) of seed i (the lowest i of
        several on a voxel).  Returns the array, or out_ptr itself when a device buffer of 4 nx ny nz bytes is given."""
        with self._staging() as s:
            nz, ny, nx = shape = tuple(int(n) for n in shape)
            xyz, seeds_ptr = _xyz(seeds)
            out = s.out(4 * max(_voxels(shape), 1), out_ptr)
            self.check(self.lib.svr_region_seed_labels(seeds_ptr, len(xyz), nx, ny, nz, C.c_void_p(out)))
            return s.array(out, shape, np.uint32)

    def region_split(self, mask, r2: int, connectivity: int = 26, dist_weights=None, step_weights=None, max_sweeps: int = 0, shape=None,
                     out_ptr: Optional[int] = None):
        """svr_region_split: erodes the mask by the ball of squared radius r2 (dist_weights as in region_ball), labels the cores under
        `connectivity` and gives every voxel of the mask to the core that is nearest inside the mask (step_weights as in
        region_geodesic; None = the chamfer weights of the connectivity).  Returns (zones, count, unreached, sweeps): a uint32 array
        [nz][ny][nx] (or out_ptr itself), the number of cores, the voxels of the mask that no core reaches, the sweeps launched."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", mask, shape)
            buf, out = s.mask(mask, shape), s.out(4 * max(_voxels(shape), 1), out_ptr)
            count, lost, sweeps = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
            self.check(self.lib.svr_region_split(buf, nx, ny, nz, _u32s(dist_weights, 3), int(r2), int(connectivity), _u32s(step_weights, 7),
                                                 int(max_sweeps), C.c_void_p(out), C.byref(count), C.byref(lost), C.byref(sweeps)))
            return s.array(out, shape, np.uint32), int(count.value), int(lost.value), int(sweeps.value)

    def region_zone_cut(self, zones, connectivity: int = 26, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_zone_cut: the mask of the voxels with a zone and no connectivity-neighbour in a smaller non-zero zone: the zones with a
        cut of one voxel between them.  zones: a uint32 array [nz][ny][nx] or a device pointer with shape=."""
        with self._staging() as s:
            zbuf, shape = s.map(zones, shape)
            nz, ny, nx = shape
            out = s.mask_out(shape, out_ptr)
            self.check(self.lib.svr_region_zone_cut(zbuf, nx, ny, nz, int(connectivity), C.c_void_p(out)))
            return s.mask_result(out, shape)

    def region_geodesic_last_ms(self) -> float:
        return self._last_ms(self.lib.svr_region_geodesic_last_ms)

    # ---- grow from seeds (svr_region_growcut / _seed_classes / _label_paint) ----
    def growcut_params(self, step_weights=None, connectivity: int = 26, gain: int = 1, shift: int = 0, max_sweeps: int = 0) -> abi.GrowcutParams:
        """svr_region_growcut_params_default of the connectivity with the weights (if given), gain, shift and cap replaced."""
        p = abi.GrowcutParams()
        self.check(self.lib.svr_region_growcut_params_default(C.byref(p), int(connectivity)))
        if step_weights is not None:
            for c in range(7):
                p.step_weights[c] = int(step_weights[c])
        p.contrast_gain, p.contrast_shift, p.max_sweeps = int(gain), int(shift), int(max_sweeps)
        return p

    def region_growcut(self, vox, labels, domain=None, shape=None, step_weights=None, connectivity: int = 26, gain: int = 1, shift: int = 0,
                       max_sweeps: int = 0, want_cost: bool = True, want_zones: bool = True, cost_ptr: Optional[int] = None,
                       zones_ptr: Optional[int] = None):
        """svr_region_growcut: (cost, zones, info).  Every voxel of `domain` (a bool array [nz][ny][nx] or a device pointer; None = the
        whole volume) gets the class of the marker (non-zero entries of `labels`, a uint32 array or a device pointer) that reaches it
        over the cheapest path, a move costing step_weights[class] + gain * (|I(u) - I(v)| >> shift) on the raw voxels of `vox` (a host
        u16 array, or a device pointer with shape=).  step_weights None = 1 on the move classes of `connectivity`.  GEO_NONE / 0 where no
        marker reaches.  An output that is not wanted is None; with cost_ptr / zones_ptr (device buffers of 4 nx ny nz bytes; zones_ptr
        may be the labels' own pointer) the result stays on the device and the pointer is returned.  info is the svr_growcut_info.  A
        failure raises SvrError with .code and .info set; for REGION_ERR_RANGE (costs reached GROWCUT_CAP) .cost and .zones hold the
        saturated solution as well."""
        with self._staging() as s:
            src, shape, on_dev = s.source(vox, shape)
            lbuf, _ = s.map(labels, like=shape)
            mbuf = s.mask(domain, shape)
            p, info = self.growcut_params(step_weights, connectivity, gain, shift, max_sweeps), abi.GrowcutInfo()
            nbytes = 4 * max(_voxels(shape), 1)
            cout, zout = s.out(nbytes, cost_ptr, want_cost), s.out(nbytes, zones_ptr, want_zones)
            rc = self.lib.svr_region_growcut(src, _dims(shape), on_dev, lbuf, mbuf, C.byref(p), _ptr(cout), _ptr(zout), C.byref(info))
            try:
                self.check(rc)
            except SvrError as e:
                e.code, e.info = int(rc), info
                if rc == abi.REGION_ERR_RANGE:
                    e.cost, e.zones = s.array(cout, shape, np.uint32), s.array(zout, shape, np.uint32)
                raise
            return s.array(cout, shape, np.uint32), s.array(zout, shape, np.uint32), info

    def region_seed_classes(self, seeds, classes, shape, out_ptr: Optional[int] = None):
        """svr_region_seed_classes: a zero uint32 array [nz][ny][nx] with classes[i] on the voxel (x, y, z) of seed i (the lowest i of
        several on a voxel).  Returns the array, or out_ptr itself when a device buffer of 4 nx ny nz bytes is given."""
        with self._staging() as s:
            shape = tuple(int(n) for n in shape)
            xyz, seeds_ptr = _xyz(seeds)
            cls = np.ascontiguousarray(classes, dtype=np.uint32).reshape(-1)
            if len(cls) != len(xyz):
                raise ValueError("one class per seed")
            out = s.out(4 * max(_voxels(shape), 1), out_ptr)
            self.check(self.lib.svr_region_seed_classes(seeds_ptr, cls.ctypes.data_as(C.POINTER(C.c_uint32)), len(xyz), _dims(shape), C.c_void_p(out)))
            return s.array(out, shape, np.uint32)

    def region_label_paint(self, labels, mask, label: int, only_unlabelled: bool = False, shape=None):
        """svr_region_label_paint: `label` on every voxel of `mask` (a bool array or a device pointer), or only where the label is still 0.
        labels: a uint32 array [nz][ny][nx] (the painted copy is returned) or a device pointer with shape= (painted in place and
        returned)."""
        with self._staging() as s:
            lbuf, shape = s.map(labels, shape)
            self.check(self.lib.svr_region_label_paint(lbuf, _dims(shape), s.mask(mask, shape), int(label), int(bool(only_unlabelled))))
            return s.array(lbuf.value, shape, np.uint32)

    def region_growcut_last_ms(self) -> float:
        return self._last_ms(self.lib.svr_region_growcut_last_ms)

    # ---- histograms of the u16 voxels (svr_volume_histogram, svr_region_label_histogram); the analysis is in the module functions ----
    def histogram_params(self, lo: int = 0, hi: int = 65535, shift: int = 0, box=None) -> abi.HistogramParams:
        """svr_histogram_params_default with the window, shift and box ((x0, y0, z0), (x1, y1, z1), inclusive) replaced."""
        return histogram_params(lo, hi, shift, box, self.lib)

    def volume_histogram(self, vox, mask=None, lo: int = 0, hi: int = 65535, shift: int = 0, box=None, shape=None,
                         out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_volume_histogram: np.uint32[bins], bins = ((hi - lo) >> shift) + 1: the voxels of `box` (inclusive, cut to the volume; None
        = all) whose mask bit is set (mask: a bool array [nz][ny][nx], a device pointer to the bit mask, or None = every voxel) and whose
        value v lies in lo .. hi, counted in bin (v - lo) >> shift.  vox is a host [nz][ny][nx] u16 array, or a device pointer with
        shape=(nz, ny, nx).  out_ptr: a device buffer of 4 * bins bytes that receives the counts."""
        with self._staging() as s:
            src, shape, on_dev = s.source(vox, shape)
            p = self.histogram_params(lo, hi, shift, box)
            bins = int(self.lib.svr_histogram_bins(C.byref(p)))
            mbuf, out = s.mask(mask, shape), s.out(4 * max(bins, 1), out_ptr)
            self.check(self.lib.svr_volume_histogram(src, _dims(shape), on_dev, mbuf, C.byref(p), C.c_void_p(out)))
            return self.to_host(out, (bins,), np.uint32)

    def region_label_histogram(self, labels, vox, count: int, lo: int = 0, hi: int = 65535, shift: int = 0, box=None, shape=None,
                               out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_label_histogram: np.uint32[count + 1, bins]; row l is the histogram of the voxels whose label is l (row 0: the
        background; labels above count are ignored).  labels: a uint32 array [nz][ny][nx] or a device pointer with shape=; vox, the
        window, shift and box as in volume_histogram.  out_ptr: a device buffer of 4 * (count + 1) * bins bytes."""
        with self._staging() as s:
            lbuf, shape = s.map(labels, shape)
            src, _, on_dev = s.source(vox, like=shape)
            p = self.histogram_params(lo, hi, shift, box)
            bins = int(self.lib.svr_histogram_bins(C.byref(p)))
            cells = (int(count) + 1) * bins
            if bins == 0 or cells > abi.HISTOGRAM_MAX_CELLS:
                cells = 0                                         # the library refuses the call: a token buffer is enough to hear it
            out = s.out(4 * max(cells, 1), out_ptr)
            self.check(self.lib.svr_region_label_histogram(lbuf, src, _dims(shape), on_dev, int(count), C.byref(p), C.c_void_p(out)))
            return self.to_host(out, (cells,), np.uint32).reshape(int(count) + 1, bins)

    def volume_histogram_last_ms(self) -> float:
        return self._last_ms(self.lib.svr_volume_histogram_last_ms)

    # ---- comparing segmentations (svr_region_surface / _overlap / _label_overlap / _distance_summary / _distance_histogram /
    #      _distance_quantile / _compare); overlap_match and compare_measure are module functions ----
    def region_surface(self, mask, element: int = 6, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_surface: the voxels of a mask (a bool array [nz][ny][nx], or a device pointer with shape=) that have a neighbour
        under the unit element 6 / 18 / 26 that is unset or lies outside the volume.  Returns the bool array."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", mask, shape)
            buf, out = s.mask(mask, shape), s.mask_out(shape, out_ptr)
            self.check(self.lib.svr_region_surface(buf, nx, ny, nz, int(element), C.c_void_p(out)))
            return s.mask_result(out, shape)

    def region_overlap(self, a, b, domain=None, shape=None):
        """svr_region_overlap: (both, a_only, b_only, neither), the voxels of `domain` (None = all) by their membership in the masks a
        and b (bool arrays [nz][ny][nx], or device pointers with shape=)."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", (a, b, domain), shape)
            abuf, bbuf, dbuf = s.mask(a, shape), s.mask(b, shape), s.mask(domain, shape)
            counts = (C.c_uint64 * 4)()
            self.check(self.lib.svr_region_overlap(abuf, bbuf, nx, ny, nz, dbuf, counts))
            return tuple(int(c) for c in counts)

    def region_label_overlap(self, a, count_a: int, b, count_b: int, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_label_overlap: np.uint32[count_a + 1, count_b + 1]; cell (la, lb) counts the voxels with label la in a and lb in b
        (uint32 arrays [nz][ny][nx], or device pointers with shape=); row 0 and column 0 are the backgrounds, labels above their count are
        not counted.  out_ptr: a device buffer of 4 * (count_a + 1) * (count_b + 1) bytes that receives the table."""
        with self._staging() as s:
            abuf, shape = s.map(a, shape)
            bbuf, _ = s.map(b, like=shape)
            ra, rb = int(count_a) + 1, int(count_b) + 1
            cells = ra * rb
            if min(ra, rb) < 2 or cells > abi.HISTOGRAM_MAX_CELLS:
                ra, rb, cells = 0, 0, 0                           # the library refuses the call: a token buffer is enough to hear it
            out = s.out(4 * max(cells, 1), out_ptr)
            self.check(self.lib.svr_region_label_overlap(abuf, int(count_a), bbuf, int(count_b), _dims(shape), C.c_void_p(out)))
            return self.to_host(out, (cells,), np.uint32).reshape(ra, rb)

    def region_distance_summary(self, d2, mask=None, tolerances2=(), shape=None) -> abi.DistanceSummary:
        """svr_region_distance_summary: the svr_distance_summary of a uint32 map (an array [nz][ny][nx] or a device pointer with shape=)
        over the voxels of `mask` (a bool array or a device pointer; None = all voxels); tolerances2: up to 8 values for `within`."""
        with self._staging() as s:
            dbuf, shape = s.map(d2, shape)
            nz, ny, nx = shape
            tol, out = [int(t) for t in tolerances2], abi.DistanceSummary()
            self.check(self.lib.svr_region_distance_summary(dbuf, s.mask(mask, shape), nx, ny, nz, _u32s(tol, len(tol)) if tol else None, len(tol),
                                                            C.byref(out)))
            return out

    def region_distance_histogram(self, d2, mask=None, lo: int = 0, hi: int = 65535, shift: int = 0, shape=None,
                                  out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_distance_histogram: np.uint32[((hi - lo) >> shift) + 1]: the values lo .. hi of a uint32 map over the voxels of
        `mask` (None = all), counted in bin (v - lo) >> shift.  out_ptr: a device buffer of 4 * bins bytes that receives the counts."""
        with self._staging() as s:
            dbuf, shape = s.map(d2, shape)
            bins = ((int(hi) - int(lo)) >> int(shift)) + 1 if 0 <= int(lo) <= int(hi) and 0 <= int(shift) <= 31 else 0
            if bins > 65536:
                bins = 0                                          # the library refuses the call: a token buffer is enough to hear it
            mbuf, out = s.mask(mask, shape), s.out(4 * max(bins, 1), out_ptr)
            self.check(self.lib.svr_region_distance_histogram(dbuf, mbuf, _dims(shape), int(lo), int(hi), int(shift), C.c_void_p(out)))
            return self.to_host(out, (bins,), np.uint32)

    def region_distance_quantile(self, d2, num: int, den: int, mask=None, shape=None):
        """svr_region_distance_quantile: the exact inverted_cdf quantile num / den of the values other than DIST_NONE of a uint32 map over
        the voxels of `mask` (None = all); None when there is no such value."""
        with self._staging() as s:
            dbuf, shape = s.map(d2, shape)
            value, status = C.c_uint32(0), C.c_int32(0)
            self.check(self.lib.svr_region_distance_quantile(dbuf, s.mask(mask, shape), _dims(shape), int(num), int(den), C.byref(value), C.byref(status)))
            return None if status.value == abi.REGION_STATUS_EMPTY else int(value.value)

    def region_compare(self, a, b, element: int = 6, weights=None, quantile=(95, 100), tolerances2=(), shape=None) -> abi.RegionComparison:
        """svr_region_compare: the svr_region_comparison of two masks (bool arrays [nz][ny][nx], or device pointers with shape=): overlap
        counts, surface sizes under `element`, and per direction the summary and the `quantile` = (num, den) of the squared distances
        between the surfaces under the integer weights (wx, wy, wz) (None = 1, 1, 1).  compare_measure turns it into Dice, Hausdorff
        and surface distances."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", (a, b), shape)
            abuf, bbuf = s.mask(a, shape), s.mask(b, shape)
            p, out = compare_params(element, weights, quantile, tolerances2, self.lib), abi.RegionComparison()
            self.check(self.lib.svr_region_compare(abuf, bbuf, nx, ny, nz, C.byref(p), C.byref(out)))
            return out

    def region_compare_last_ms(self) -> float:
        return self._last_ms(self.lib.svr_region_compare_last_ms)

    # ---- scissors (svr_stencil_polygon, svr_region_scissor_camera / _slice); scissor_project_camera / _slice, stencil_rect and
    #      scissor_params are module functions ----
    def stencil_polygon(self, contours, w: int, h: int, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_stencil_polygon: the even-odd fill of a polygon on a w x h pixel grid.  contours: a list of (n, 2) arrays of (x, y) in
        pixels (the centre of pixel (px, py) is (px + 0.5, py + 0.5)), each closed implicitly, converted to 1/256 pixel by round(256 v);
        a contour inside another is a hole.  Returns the stencil words, np.uint32[h * ceil(w / 32)]: the bit mask of a [1][h][w] volume
        (region_mask_unpack(words, (1, h, w))[0] is the image).  out_ptr: a device buffer of that many words that receives them."""
        q8, counts = _contours_q8(contours)
        w, h = _image_size(w, h)
        with self._staging() as s:
            words = region_mask_words((1, h, w))
            out = s.out(4 * words, out_ptr)
            self.check(self.lib.svr_stencil_polygon(q8.ctypes.data_as(C.POINTER(C.c_int32)), counts.ctypes.data_as(C.POINTER(C.c_uint32)), len(counts),
                                                    w, h, C.c_void_p(out)))
            return self.to_host(out, (words,), np.uint32)

    def region_scissor(self, mask, stencil, volume: cudaVolume, camera=None, slice=None, w: Optional[int] = None, h: Optional[int] = None,
                       op: int = abi.SCISSOR_SELECT, depth=(-np.inf, np.inf), shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_scissor_camera / _slice: the voxels of the [nz][ny][nx] grid of `volume` (its bbox) whose centre is seen inside
        the stencil -- through `camera` (a cudaCamera; the stencil is imageW x imageH) or through `slice` (a SliceParams on a w x h
        image), exactly one of the two -- at a depth in the closed interval `depth`, combined with `mask` by op: SCISSOR_SELECT (mask
        may be None, with shape=), _ERASE_INSIDE, _ERASE_OUTSIDE, _FILL_INSIDE.  mask: a bool array [nz][ny][nx] or a device pointer
        with shape=; stencil: a bool image [h][w], the words of stencil_polygon, or a device pointer.  out_ptr may be the mask's own
        pointer.  Returns the bool array."""
        if (camera is None) == (slice is None):
            raise ValueError("exactly one of camera and slice must be given")
        if camera is not None and (w is not None or h is not None):
            raise ValueError("w and h belong to a slice view: a camera has its imageW x imageH")
        if slice is not None and (w is None or h is None):
            raise ValueError("a slice view needs w= and h=")
        w, h = _image_size(camera.imageW if camera is not None else w, camera.imageH if camera is not None else h)
        if mask is None and int(op) != abi.SCISSOR_SELECT:
            raise ValueError("only SCISSOR_SELECT works without a mask")
        if mask is None and shape is None:
            raise ValueError("SCISSOR_SELECT without a mask needs shape=(nz, ny, nx)")
        nz, ny, nx = shape = _shape_of("mask", mask, shape) if mask is not None else _shape_of("mask", (), shape)
        sten = _stencil_words(stencil, w, h)
        p = scissor_params(op, depth)
        with self._staging() as s:
            buf = s.mask(mask, shape)
            sbuf = C.c_void_p(s.upload(sten, 4)) if isinstance(sten, np.ndarray) else C.c_void_p(int(sten))
            out = s.mask_out(shape, out_ptr)
            if camera is not None:
                rc = self.lib.svr_region_scissor_camera(buf, nx, ny, nz, C.byref(volume), C.byref(camera), sbuf, C.byref(p), C.c_void_p(out))
            else:
                rc = self.lib.svr_region_scissor_slice(buf, nx, ny, nz, C.byref(volume), C.byref(slice), w, h, sbuf, C.byref(p), C.c_void_p(out))
            self.check(rc)
            return s.mask_result(out, shape)

    def region_scissor_last_ms(self) -> float:
        return self._last_ms(self.lib.svr_region_scissor_last_ms)

    # ---- fill between slices (svr_region_slice_counts / _slice_distance / _fill_between); axis 0, 1, 2 = x, y, z ----
    def region_slice_counts(self, mask, axis: int = 2, shape=None) -> np.ndarray:
        """svr_region_slice_counts: np.uint64[n_axis], the set voxels of every slice of the axis.  mask: a bool array [nz][ny][nx], or a
        device pointer with shape=."""
        shape = _shape_of("mask", mask, shape)
        axis = _slice_axis(axis)
        with self._staging() as s:
            nz, ny, nx = shape
            counts = (C.c_uint64 * shape[2 - axis])()
            self.check(self.lib.svr_region_slice_counts(s.mask(mask, shape), nx, ny, nz, axis, counts))
            return np.array(list(counts), dtype=np.uint64)

    def region_slice_distance(self, mask, axis: int = 2, weights=None, slices=None, shape=None, out_ptr: Optional[int] = None):
        """svr_region_slice_distance: the planar maps of the listed slices of the axis (None = all, in order; any order, repeats allowed)
        under the integer weights (wx, wy, wz) (None = 1, 1, 1; the slicing axis's is not used): a uint32 array [len(slices)][nv][nu],
        u < v the in-plane axes, or out_ptr itself when a device buffer of that many uint32 is given."""
        shape = _shape_of("mask", mask, shape)
        axis = _slice_axis(axis)
        ks = None if slices is None else _slice_list("slices", slices, shape[2 - axis], increasing=False)
        if ks is not None and len(ks) == 0:
            raise ValueError("the slice list is empty")
        with self._staging() as s:
            nz, ny, nx = shape
            n = shape[2 - axis] if ks is None else len(ks)
            out_shape = (n,) + tuple(t for a, t in zip((2, 1, 0), shape) if a != axis)
            buf, out = s.mask(mask, shape), s.out(4 * max(n * (_voxels(shape) // shape[2 - axis]), 1), out_ptr)
            self.check(self.lib.svr_region_slice_distance(buf, nx, ny, nz, axis, _u32s(weights, 3), None if ks is None else ks.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          n, C.c_void_p(out)))
            return s.array(out, out_shape, np.uint32)

    def region_fill_between(self, mask, axis: int = 2, keys=None, weights=None, keep_between: bool = False, shape=None,
                            out_ptr: Optional[int] = None, gap_by_gap: bool = False):
        """svr_region_fill_between: the mask with the slices between consecutive keys of the axis filled by shape-based interpolation.
        keys: strictly increasing slice numbers (they may name empty slices), None = every slice that holds a set voxel; weights: (wx,
        wy, wz), None = 1, 1, 1; keep_between: OR the input bits of the slices between keys into the result; gap_by_gap: at most two
        planar maps at a time.  mask: a bool array [nz][ny][nx], or a device pointer with shape=; out_ptr may be the mask's own pointer.
        Returns (mask, info): the bool array and the svr_fill_between_info."""
        shape = _shape_of("mask", mask, shape)
        p = fill_between_params(axis, keys, weights, keep_between, gap_by_gap, n_axis=shape[2 - _slice_axis(axis)])
        with self._staging() as s:
            nz, ny, nx = shape
            buf, out, info = s.mask(mask, shape), s.mask_out(shape, out_ptr), abi.FillBetweenInfo()
            self.check(self.lib.svr_region_fill_between(buf, nx, ny, nz, C.byref(p), C.c_void_p(out), C.byref(info)))
            return s.mask_result(out, shape), info

    def region_fill_between_last_ms(self) -> float:
        return self._last_ms(self.lib.svr_region_fill_between_last_ms)

    def region_fill_between_pass_ms(self):
        """(counts, maps, fill) milliseconds of the last region_fill_between that had a gap"""
        return self._last_ms(self.lib.svr_region_fill_between_pass_ms, 3)

    # ---- smoothing masks and label maps (svr_region_box_count / _smooth / _label_smooth); radii = (rx, ry, rz), each 0 .. 8 ----
    def region_box_count(self, mask, radii, shape=None, out_ptr: Optional[int] = None, density: bool = False):
        """svr_region_box_count: the set voxels in the (2rx+1) x (2ry+1) x (2rz+1) window around every voxel, the border replicated: a
        u16 array [nz][ny][nx], or out_ptr itself when a device buffer of nx * ny * nz u16 is given.  mask: a bool array [nz][ny][nx], or
        a device pointer with shape=.  density: svr_region_box_density, floor(65535 count / N) instead of the count."""
        shape = _shape_of("mask", mask, shape)
        r = _radii(radii)
        with self._staging() as s:
            buf, out = s.mask(mask, shape), s.out(2 * max(_voxels(shape), 1), out_ptr)
            call = self.lib.svr_region_box_density if density else self.lib.svr_region_box_count
            self.check(call(buf, _dims(shape), r, C.c_void_p(out)))
            return s.array(out, shape, np.uint16)

    def region_smooth(self, mask, op: int, radii, iterations: int = 1, shape=None, out_ptr: Optional[int] = None):
        """svr_region_smooth: SMOOTH_MAJORITY (set iff more than half of the window is set: the binary median) or SMOOTH_BINOMIAL (the
        upper half of volume_smooth of the mask at 65535) applied `iterations` times.  Returns (mask, changed): the bool array and the
        voxels that differ from the input.  out_ptr: a device buffer of region_mask_words(shape) uint32 that is not the input."""
        shape = _shape_of("mask", mask, shape)
        r = _radii(radii)
        with self._staging() as s:
            buf, out, changed = s.mask(mask, shape), s.mask_out(shape, out_ptr), C.c_uint64(0)
            self.check(self.lib.svr_region_smooth(buf, _dims(shape), int(op), r, int(iterations), C.c_void_p(out), C.byref(changed)))
            return s.mask_result(out, shape), int(changed.value)

    def region_label_smooth(self, labels, count: int, radii, iterations: int = 1, shape=None, out_ptr: Optional[int] = None):
        """svr_region_label_smooth: the mode filter of a label map with values 0 .. count (count <= 255; larger values read as 0): every
        voxel takes the most frequent label of its window, its own where that is among the most frequent, else the smallest of them.
        Returns (labels, changed): a uint32 array [nz][ny][nx], or out_ptr itself when a device buffer of 4 nx ny nz bytes is given."""
        r = _radii(radii)
        with self._staging() as s:
            lbuf, shape = s.map(labels, shape)
            out, changed = s.out(4 * max(_voxels(shape), 1), out_ptr), C.c_uint64(0)
            self.check(self.lib.svr_region_label_smooth(lbuf, _dims(shape), int(count), r, int(iterations), C.c_void_p(out), C.byref(changed)))
            return s.array(out, shape, np.uint32), int(changed.value)

    def region_smooth_last_ms(self) -> float:
        return self._last_ms(self.lib.svr_region_smooth_last_ms)

    # ---- overlays: region masks and label maps on slices and 3D views (svr_slice_ids, svr_hit_ids, svr_overlay_ids, svr_overlay_slice) ----
    def overlay_style(self, fill_alpha: Optional[int] = None, edge_alpha: Optional[int] = None, palette=None) -> abi.OverlayStyle:
        """The library's default svr_overlay_style (fill 96, edge 255, built-in palette) with the named members replaced.  palette: up
        to abi.OVERLAY_MAX_PALETTE RGBA8 entries as uint32 (r in the low byte) or as rows (r, g, b, a); the style keeps the array alive."""
        st = abi.OverlayStyle()
        self.check(self.lib.svr_overlay_style_default(C.byref(st)))
        if fill_alpha is not None:
            st.fill_alpha = int(fill_alpha)
        if edge_alpha is not None:
            st.edge_alpha = int(edge_alpha)
        if palette is not None:
            pal = np.asarray(palette)
            if pal.ndim == 2:
                pal = np.ascontiguousarray(pal, dtype=np.uint8).view("<u4").reshape(-1)
            st._palette = np.ascontiguousarray(pal, dtype=np.uint32)
            st.palette = st._palette.ctypes.data_as(C.POINTER(C.c_uint32))
            st.palette_count = len(st._palette)
        return st

    def overlay_palette_default(self, n: int = abi.OVERLAY_DEFAULT_PALETTE) -> np.ndarray:
        out = np.zeros(int(n), dtype=np.uint32)
        self.check(self.lib.svr_overlay_palette_default(out.ctypes.data_as(C.POINTER(C.c_uint32)), int(n)))
        return out

    @staticmethod
    def _overlay_source(mask: Optional[int], labels: Optional[int]) -> abi.OverlaySource:
        return abi.OverlaySource(C.c_void_p(int(mask)) if mask else None, C.c_void_p(int(labels)) if labels else None)

    def slice_ids(self, ids: int, volume: cudaVolume, shape, w: int, h: int, params: abi.SliceParams, mask: Optional[int] = None,
                  labels: Optional[int] = None, count: int = 1, spacing: float = 0.0):
        """svr_slice_ids: the region id of every owned pixel of `count` slices into the device buffer ids (count x h x w uint32).  mask /
        labels: the device pointer of a bit mask or of a uint32 label array of the (nz, ny, nx) = shape volume; exactly one is given."""
        nz, ny, nx = (int(n) for n in shape)
        src = self._overlay_source(mask, labels)
        self.check(self.lib.svr_slice_ids(C.c_void_p(int(ids)), C.byref(volume), nx, ny, nz, int(w), int(h), C.byref(params), int(count),
                                          C.c_float(float(spacing)), C.byref(src)))

    def hit_ids(self, ids: int, hits: int, w: int, h: int, volume: cudaVolume, shape, mask: Optional[int] = None, labels: Optional[int] = None):
        """svr_hit_ids: the region id of every record of a full w x h hit map (svr_render_hits) into the device buffer ids."""
        nz, ny, nx = (int(n) for n in shape)
        src = self._overlay_source(mask, labels)
        self.check(self.lib.svr_hit_ids(C.c_void_p(int(ids)), C.c_void_p(int(hits)), int(w), int(h), C.byref(volume), nx, ny, nz, C.byref(src)))

    def overlay_ids(self, imgs: int, ids: int, w: int, h: int, count: int = 1, style: Optional[abi.OverlayStyle] = None):
        """svr_overlay_ids: tints `count` RGBA8 images of w x h in place by their id images: fill inside a part, outline at its edge."""
        st = style if style is not None else self.overlay_style()
        self.check(self.lib.svr_overlay_ids(C.c_void_p(int(imgs)), C.c_void_p(int(ids)), int(w), int(h), int(count), C.byref(st)))

    def overlay_slice(self, imgs: int, volume: cudaVolume, shape, w: int, h: int, params: abi.SliceParams, mask: Optional[int] = None,
                      labels: Optional[int] = None, style: Optional[abi.OverlayStyle] = None, count: int = 1, spacing: float = 0.0):
        """svr_overlay_slice: slice_ids followed by overlay_ids in one kernel, over the owned pixels of the slice images at imgs."""
        nz, ny, nx = (int(n) for n in shape)
        src = self._overlay_source(mask, labels)
        st = style if style is not None else self.overlay_style()
        self.check(self.lib.svr_overlay_slice(C.c_void_p(int(imgs)), C.byref(volume), nx, ny, nz, int(w), int(h), C.byref(params), int(count),
                                              C.c_float(float(spacing)), C.byref(src), C.byref(st)))

    def overlay_last_ms(self) -> float:
        return self._last_ms(self.lib.svr_overlay_last_ms)

    # ---- surface meshes by surface nets (svr_mesh_isosurface / _region / _measure / _positions) ----
    def mesh_params(self, level: Optional[int] = None, relax: int = 0) -> abi.MeshParams:
        p = abi.MeshParams()
        self.check(self.lib.svr_mesh_params_default(C.byref(p)))
        if level is not None:
            p.level = int(level)
        p.relax = int(relax)
        return p

    def _mesh_extract(self, s: _Staging, call):
        """A counting call, then an extraction call into a buffer of the counted size from the scope s.  call(vertices pointer, vertex
        capacity, triangles pointer, triangle capacity, info) runs the C function.  Returns (vertices int32 [nv, 3], triangles uint32
        [nt, 3], info)."""
        info = abi.MeshInfo()
        self.check(call(None, 0, None, 0, info))
        nv, nt = int(info.vertices), int(info.triangles)
        if nv == 0:
            return np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32), info
        buf = s.alloc(12 * (nv + max(nt, 1)))
        self.check(call(C.c_void_p(buf), nv, C.c_void_p(buf + 12 * nv), nt, info))
        return self.to_host(buf, (nv, 3), np.int32), self.to_host(buf + 12 * nv, (nt, 3), np.uint32), info

    def mesh_isosurface(self, vox, level: int, relax: int = 0, shape=None):
        """svr_mesh_isosurface: the surface-nets mesh of {v >= level} of a host [nz][ny][nx] u16 array or a device pointer with
        shape=(nz, ny, nx), after `relax` constrained relaxation steps.  Returns (vertices, triangles, info): int32 [nv, 3] in units of
        1/256 voxel on the padded grid (sample x sits at 256 (x + 1)), uint32 [nt, 3], and the svr_mesh_info."""
        with self._staging() as s:
            src, (nz, ny, nx), on_dev = s.source(vox, shape)
            p = self.mesh_params(level, relax)
            return self._mesh_extract(s, lambda v, nv, t, nt, info: self.lib.svr_mesh_isosurface(src, nx, ny, nz, on_dev, C.byref(p), v, nv, t, nt, C.byref(info)))

    def mesh_region(self, mask, relax: int = 0, shape=None):
        """svr_mesh_region: the same for a region mask (a bool array [nz][ny][nx], or a device pointer to the bit mask with shape=)."""
        with self._staging() as s:
            nz, ny, nx = shape = _shape_of("mask", mask, shape)
            buf, p = s.mask(mask, shape), self.mesh_params(None, relax)
            return self._mesh_extract(s, lambda v, nv, t, nt, info: self.lib.svr_mesh_region(buf, nx, ny, nz, C.byref(p), v, nv, t, nt, C.byref(info)))

    def mesh_measure(self, vertices, triangles, scale=(1.0 / 256, 1.0 / 256, 1.0 / 256)):
        """svr_mesh_measure of host arrays (uploaded): (volume6, area) -- the exact integer 6 * 256^3 * (enclosed volume in voxels) and the
        surface area under the per-axis scale (spacing / 256)."""
        v = np.ascontiguousarray(vertices, dtype=np.int32).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        sc = (C.c_double * 3)(*[float(x) for x in scale])
        vol, area = C.c_int64(0), C.c_double(0.0)
        with self._staging() as s:
            buf = s.alloc(max(v.nbytes, 4) + max(t.nbytes, 4))    # one buffer: the vertices, then the triangles
            tbuf = buf + max(v.nbytes, 4)
            if len(v):
                self.to_device(buf, v)
            if len(t):
                self.to_device(tbuf, t)
            self.check(self.lib.svr_mesh_measure(C.c_void_p(buf), len(v), C.c_void_p(tbuf), len(t), sc, C.byref(vol), C.byref(area)))
        return int(vol.value), float(area.value)

    def mesh_positions(self, vertices, spacing=(1.0, 1.0, 1.0), volume: Optional[cudaVolume] = None) -> np.ndarray:
        return mesh_positions(self.lib, vertices, spacing, volume)

    def mesh_last_ms(self):
        """(classify, emit, relax) HIP-event milliseconds of the last mesh call"""
        return self._last_ms(self.lib.svr_mesh_last_ms, 3)

    # ---- exact volume filters (svr_volume_*): median / min / max and binomial smoothing of the raw voxels ----
    def volume_rank(self, vox, op: int, element: int = 6, iterations: int = 1, shape=None, out_ptr: Optional[int] = None):
        """svr_volume_rank: the median (FILTER_MEDIAN), minimum (FILTER_MIN) or maximum (FILTER_MAX) of every voxel's window under the
        unit element 6 / 18 / 26 with a replicated border, applied `iterations` times.  vox is a host [nz][ny][nx] u16 array, or a device
        pointer with shape=(nz, ny, nx).  Returns a u16 array [nz][ny][nx]; with out_ptr (a device buffer of nx * ny * nz u16 that does
        not overlap a device `vox`) the result stays on the device and out_ptr is returned."""
        with self._staging() as s:
            src, shape, on_dev = s.source(vox, shape)
            nz, ny, nx = shape
            out = s.out(2 * max(_voxels(shape), 1), out_ptr)
            self.check(self.lib.svr_volume_rank(src, nx, ny, nz, on_dev, int(op), int(element), int(iterations), C.c_void_p(out)))
            return s.array(out, shape, np.uint16)

    def volume_median(self, vox, element: int = 6, iterations: int = 1, shape=None, out_ptr: Optional[int] = None):
        """volume_rank with FILTER_MEDIAN."""
        return self.volume_rank(vox, abi.FILTER_MEDIAN, element, iterations, shape, out_ptr)

    def volume_smooth(self, vox, radii, shape=None, out_ptr: Optional[int] = None):
        """svr_volume_smooth: separable binomial smoothing with the per-axis radii (rx, ry, rz), each 0 .. SMOOTH_MAX_RADIUS, one
        rounding per axis, a replicated border.  vox, the return value and out_ptr as in volume_rank."""
        with self._staging() as s:
            src, shape, on_dev = s.source(vox, shape)
            nz, ny, nx = shape
            out = s.out(2 * max(_voxels(shape), 1), out_ptr)
            self.check(self.lib.svr_volume_smooth(src, nx, ny, nz, on_dev, _u32s(radii, 3), C.c_void_p(out)))
            return s.array(out, shape, np.uint16)

    def volume_filter_last_ms(self) -> float:
        """HIP-event time of the device work of the last volume_rank / volume_smooth call."""
        return self._last_ms(self.lib.svr_volume_filter_last_ms)

    # ---- crop and resample (svr_resample_grid_* / svr_volume_resample / svr_region_resample / _label_resample / _paste / _mask_expand) ----
    def resample_grid_box(self, shape, box) -> abi.ResampleGrid:
        return resample_grid_box(shape, box, self.lib)

    def resample_grid_spacing(self, shape, src_spacing, target_spacing, box=None):
        return resample_grid_spacing(shape, src_spacing, target_spacing, box, self.lib)

    def resample_grid_dims(self, shape, out_shape, box=None) -> abi.ResampleGrid:
        return resample_grid_dims(shape, out_shape, box, self.lib)

    def resample_grid_place(self, volume: cudaVolume, shape, grid) -> cudaVolume:
        return resample_grid_place(volume, shape, grid, self.lib)

    def volume_resample(self, vox, grid, mode: int = abi.RESAMPLE_AUTO, shape=None, out_ptr: Optional[int] = None):
        """svr_volume_resample: the volume on `grid` (a ResampleGrid, or ((origin, step, count) of x, y, z)) under RESAMPLE_NEAREST /
        _LINEAR / _AREA / _AUTO.  vox is a host [nz][ny][nx] u16 array, or a device pointer with shape=(nz, ny, nx).  Returns a u16 array
        of grid.shape; with out_ptr (a device buffer of that many u16 that does not overlap a device `vox`) the result stays on the
        device and out_ptr is returned."""
        with self._staging() as s:
            src, shape, on_dev = s.source(vox, shape)
            g = resample_grid(grid)
            out = s.out(2 * max(_voxels(g.shape), 1), out_ptr)
            self.check(self.lib.svr_volume_resample(src, _dims(shape), on_dev, C.byref(g), int(mode), C.c_void_p(out)))
            return s.array(out, g.shape, np.uint16)

    def volume_crop(self, vox, box, shape=None, out_ptr: Optional[int] = None):
        """volume_resample on the grid of a box ((x0, y0, z0), (x1, y1, z1)), inclusive, cut to the volume.  Returns (result, grid)."""
        shape = vox.shape if isinstance(vox, np.ndarray) else shape
        g = self.resample_grid_box(shape, box)
        return self.volume_resample(vox, g, abi.RESAMPLE_NEAREST, shape, out_ptr), g

    def region_resample(self, mask, grid, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_resample: NEAREST on a mask (a bool array [nz][ny][nx], or a device pointer with shape=).  Returns the bool array of
        grid.shape; out_ptr: a device buffer of region_mask_words(grid.shape) uint32 that receives the bit mask."""
        with self._staging() as s:
            shape, g = _shape_of("mask", mask, shape), resample_grid(grid)
            buf, out = s.mask(mask, shape), s.mask_out(g.shape, out_ptr)
            self.check(self.lib.svr_region_resample(buf, _dims(shape), C.byref(g), C.c_void_p(out)))
            return s.mask_result(out, g.shape)

    def region_label_resample(self, labels, grid, shape=None, out_ptr: Optional[int] = None):
        """svr_region_label_resample: NEAREST on a uint32 map (labels, zones; a squared-distance map only for crops).  Returns the uint32
        array of grid.shape, or out_ptr itself when a device buffer of that many uint32 is given."""
        with self._staging() as s:
            buf, shape = s.map(labels, shape)
            g = resample_grid(grid)
            out = s.out(4 * max(_voxels(g.shape), 1), out_ptr)
            self.check(self.lib.svr_region_label_resample(buf, _dims(shape), C.byref(g), C.c_void_p(out)))
            return s.array(out, g.shape, np.uint32)

    def region_paste(self, sub, full, offset, op: int = abi.PASTE_REPLACE, sub_shape=None, full_shape=None):
        """svr_region_paste: the sub-mask put back at offset (x, y, z) of the full mask with PASTE_REPLACE, MASK_OR or MASK_ANDNOT.  Masks
        are bool arrays, or device pointers with their shapes.  A device `full` is changed in place and returned; a host `full` is left
        alone and the pasted bool array is returned."""
        with self._staging() as s:
            sub_shape, full_shape = _shape_of("mask", sub, sub_shape), _shape_of("mask", full, full_shape)
            sbuf, fbuf = s.mask(sub, sub_shape), s.mask(full, full_shape)
            self.check(self.lib.svr_region_paste(sbuf, _dims(sub_shape), fbuf, _dims(full_shape), _i32x3(offset), int(op)))
            if isinstance(full, np.ndarray):
                return s.mask_result(fbuf.value, full_shape)
            self.synchronize()
            return full

    def region_mask_expand(self, mask, value: int = 1, shape=None, out_ptr: Optional[int] = None):
        """svr_region_mask_expand: one byte per voxel, `value` (1 .. 255) inside the mask and 0 outside -- what io.mhd_write saves a mask
        from.  Returns the u8 array [nz][ny][nx], or out_ptr itself when a device buffer of nx * ny * nz bytes is given."""
        with self._staging() as s:
            shape = _shape_of("mask", mask, shape)
            buf, out = s.mask(mask, shape), s.out(max(_voxels(shape), 4), out_ptr)
            self.check(self.lib.svr_region_mask_expand(buf, _dims(shape), int(value), C.c_void_p(out)))
            return s.array(out, shape, np.uint8)

    def volume_resample_last_ms(self) -> float:
        """HIP-event time of the device work of the last volume_resample / region_resample / _label_resample / _paste / _mask_expand."""
        return self._last_ms(self.lib.svr_volume_resample_last_ms)


# svr_region_component as a numpy record (40 bytes); LABEL_SCAN_BLOCK mirrors SVR_LABEL_SCAN_BLOCK of csrc/svr_label.hip
COMPONENT_DTYPE = np.dtype([("voxels", "<u4"), ("first", "<u4"), ("bbox_min", "<i4", (3,)), ("bbox_max", "<i4", (3,)), ("sum", "<u8")])
assert COMPONENT_DTYPE.itemsize == 40
LABEL_SCAN_BLOCK = abi.LABEL_SCAN_BLOCK


def region_label_scan_levels(shape) -> int:
    """The levels of svr_region_label's renumbering scan for a [nz][ny][nx] volume: 1 while one block covers the mask words, 2 up to
    a block of blocks, and so on."""
    n, levels = region_mask_words(shape), 1
    while n > LABEL_SCAN_BLOCK:
        n, levels = (n + LABEL_SCAN_BLOCK - 1) // LABEL_SCAN_BLOCK, levels + 1
    return levels


def mesh_positions(lib, vertices, spacing=(1.0, 1.0, 1.0), volume=None) -> np.ndarray:
    """svr_mesh_positions: float32 [nv, 3] positions of mesh vertices (int32 [nv, 3], 1/256 voxel on the padded grid) -- millimetres,
    (u / 256 - 0.5) * spacing, or with `volume` (a cudaVolume) the world coordinates of the sampler's mapping.  Host code of the library:
    no device is needed."""
    lib = lib if lib is not None else abi.load()
    v = np.ascontiguousarray(vertices, dtype=np.int32).reshape(-1, 3)
    out = np.zeros((len(v), 3), dtype=np.float32)
    sp = (C.c_double * 3)(*[float(t) for t in spacing])
    _host_call(lib, "svr_mesh_positions", lib.svr_mesh_positions(v.ctypes.data_as(C.c_void_p), len(v), sp, C.byref(volume) if volume is not None else None,
                                                                 out.ctypes.data_as(C.c_void_p)))
    return out


def distance_weights(spacing, shape, lib=None):
    """svr_region_distance_weights: ((wx, wy, wz), unit) for a spacing (sx, sy, sz) and a [nz][ny][nx] shape: the integer weights of the
    squared distance in units of `unit` = min(spacing) / 2^k.  A length L is r2 = floor((L / unit)^2); a map value d2 means sqrt(d2) unit.
    Host code of the library: no device is needed."""
    lib = lib if lib is not None else abi.load()
    nz, ny, nx = (int(n) for n in shape)
    sp = (C.c_double * 3)(*[float(t) for t in spacing])
    w, unit = (C.c_uint32 * 3)(), C.c_double(0.0)
    _host_call(lib, "svr_region_distance_weights", lib.svr_region_distance_weights(sp, nx, ny, nz, w, C.byref(unit)))
    return (int(w[0]), int(w[1]), int(w[2])), float(unit.value)


def geodesic_weights(spacing, connectivity, shape, lib=None):
    """svr_region_geodesic_weights: ((w_x, w_y, w_z, w_xy, w_xz, w_yz, w_xyz), unit) for a spacing (sx, sy, sz), a connectivity 6 / 18 / 26
    and a [nz][ny][nx] shape: the Euclidean lengths of the moves in units of `unit` = min(spacing) / 2^k, rounded, 0 for the classes
    beyond the connectivity.  A geodesic map value d means about d unit.  Host code of the library: no device is needed."""
    lib = lib if lib is not None else abi.load()
    nz, ny, nx = (int(n) for n in shape)
    sp = (C.c_double * 3)(*[float(t) for t in spacing])
    w, unit = (C.c_uint32 * 7)(), C.c_double(0.0)
    _host_call(lib, "svr_region_geodesic_weights", lib.svr_region_geodesic_weights(sp, int(connectivity), nx, ny, nz, w, C.byref(unit)))
    return tuple(int(t) for t in w), float(unit.value)


def smooth_radii(spacing, sigma, lib=None):
    """svr_volume_smooth_radii: ((rx, ry, rz), (sx, sy, sz)) for a spacing and a sigma in the spacing's units: the binomial radii
    llround(2 (sigma / spacing[a])^2) and the sigma each one applies, sqrt(r / 2) spacing[a].  Host code of the library: no device is
    needed."""
    lib = lib if lib is not None else abi.load()
    sp = (C.c_double * 3)(*[float(t) for t in spacing])
    r, so = (C.c_uint32 * 3)(), (C.c_double * 3)()
    _host_call(lib, "svr_volume_smooth_radii", lib.svr_volume_smooth_radii(sp, float(sigma), r, so))
    return (int(r[0]), int(r[1]), int(r[2])), (float(so[0]), float(so[1]), float(so[2]))


def _histogram_call(lib, name, rc) -> bool:
    """Raises on an error code; returns True when the histogram was empty (SVR_HISTOGRAM_STATUS_EMPTY)."""
    return _host_call(lib, name, rc, ok=(0, abi.HISTOGRAM_STATUS_EMPTY)) == abi.HISTOGRAM_STATUS_EMPTY


def _histogram_counts(counts):
    c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    return c, c.ctypes.data_as(C.c_void_p) if len(c) else None


def histogram_params(lo: int = 0, hi: int = 65535, shift: int = 0, box=None, lib=None) -> abi.HistogramParams:
    """svr_histogram_params_default with the window, shift and box ((x0, y0, z0), (x1, y1, z1), inclusive) replaced.  The histogram
    helpers below are host code of the library: no device is needed."""
    lib = lib if lib is not None else abi.load()
    p = abi.HistogramParams()
    _histogram_call(lib, "svr_histogram_params_default", lib.svr_histogram_params_default(C.byref(p)))
    p.lo, p.hi, p.shift = int(lo), int(hi), int(shift)
    if box is not None:
        for a in range(3):
            p.box_min[a], p.box_max[a] = int(box[0][a]), int(box[1][a])
    return p


def histogram_bins(lo: int = 0, hi: int = 65535, shift: int = 0, lib=None) -> int:
    """svr_histogram_bins: ((hi - lo) >> shift) + 1, or 0 for an invalid window or shift."""
    lib = lib if lib is not None else abi.load()
    p = histogram_params(lo, hi, shift, None, lib)
    return int(lib.svr_histogram_bins(C.byref(p)))


def histogram_bin_range(bin: int, lo: int = 0, hi: int = 65535, shift: int = 0, lib=None):
    """svr_histogram_bin_range: (v_lo, v_hi), the raw values of a bin -- the window for region_threshold."""
    lib = lib if lib is not None else abi.load()
    p = histogram_params(lo, hi, shift, None, lib)
    a, b = C.c_uint32(0), C.c_uint32(0)
    _histogram_call(lib, "svr_histogram_bin_range", lib.svr_histogram_bin_range(C.byref(p), int(bin), C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def histogram_moments(counts, lib=None):
    """svr_histogram_moments: (n, sum, sum_sq) of the bin indices of a uint32 histogram; (0, 0, 0) when it is empty."""
    lib = lib if lib is not None else abi.load()
    c, ptr = _histogram_counts(counts)
    n, s, q = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _histogram_call(lib, "svr_histogram_moments", lib.svr_histogram_moments(ptr, len(c), C.byref(n), C.byref(s), C.byref(q)))
    return int(n.value), int(s.value), int(q.value)


def histogram_quantile(counts, num: int, den: int, lib=None):
    """svr_histogram_quantile: the smallest bin b with C(b) > 0 and den * C(b) >= num * N (numpy's inverted_cdf for 0 < num / den <= 1;
    num = 0: the first occupied bin); None when the histogram is empty."""
    lib = lib if lib is not None else abi.load()
    c, ptr = _histogram_counts(counts)
    b = C.c_uint32(0)
    empty = _histogram_call(lib, "svr_histogram_quantile", lib.svr_histogram_quantile(ptr, len(c), int(num), int(den), C.byref(b)))
    return None if empty else int(b.value)


def histogram_otsu(counts, classes: int = 2, lib=None):
    """svr_histogram_otsu: (thresholds, eta): the classes - 1 exact Otsu thresholds (the last bins of the lower classes; ties go to the
    lexicographically smallest tuple) and between-class / total variance; (None, 0.0) when the histogram is empty."""
    lib = lib if lib is not None else abi.load()
    c, ptr = _histogram_counts(counts)
    t, eta = (C.c_uint32 * 2)(), C.c_double(0.0)
    empty = _histogram_call(lib, "svr_histogram_otsu", lib.svr_histogram_otsu(ptr, len(c), int(classes), t, C.byref(eta)))
    if empty:
        return None, 0.0
    return tuple(int(t[k]) for k in range(int(classes) - 1)), float(eta.value)


def compare_params(element: int = 6, weights=None, quantile=(95, 100), tolerances2=(), lib=None) -> abi.CompareParams:
    """svr_compare_params_default with the element, weights (None = 1, 1, 1), quantile (num, den) and squared tolerances replaced.  The
    comparison helpers below are host code of the library: no device is needed."""
    lib = lib if lib is not None else abi.load()
    p = abi.CompareParams()
    _host_call(lib, "svr_compare_params_default", lib.svr_compare_params_default(C.byref(p)))
    p.element, p.q_num, p.q_den = int(element), int(quantile[0]), int(quantile[1])
    if weights is not None:
        for a in range(3):
            p.weights[a] = int(weights[a])
    tol = [int(t) for t in tolerances2]
    p.ntol = len(tol)                                         # (more than 8: the library refuses the call)
    for k, t in enumerate(tol[:abi.COMPARE_MAX_TOLERANCES]):
        p.tolerances2[k] = t
    return p


def overlap_match(table, lib=None):
    """svr_overlap_match: (best_b_for_a, best_a_for_b) of a label overlap table np.uint32[count_a + 1, count_b + 1]: for each label 1 ..
    count of one map the non-background label of the other with the largest Jaccard index (sizes from the row and column sums; ties go to
    the lower label), 0 where nothing overlaps.  Two uint32 arrays, indexed by label - 1."""
    lib = lib if lib is not None else abi.load()
    t = np.ascontiguousarray(table, dtype=np.uint32)
    if t.ndim != 2:
        raise ValueError("the table must be [count_a + 1][count_b + 1]")
    ca, cb = t.shape[0] - 1, t.shape[1] - 1
    best_b, best_a = np.zeros(max(ca, 1), np.uint32), np.zeros(max(cb, 1), np.uint32)
    _host_call(lib, "svr_overlap_match", lib.svr_overlap_match(t.ctypes.data_as(C.c_void_p), ca, cb, best_b.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                               best_a.ctypes.data_as(C.POINTER(C.c_uint32))))
    return best_b[:ca], best_a[:cb]


def compare_measure(comparison: abi.RegionComparison, unit: float = 1.0, lib=None) -> abi.CompareMeasurement:
    """svr_region_compare_measure: Dice, Jaccard, volume difference, directed / symmetric / quantile Hausdorff distances, ASSD, RMS and
    surface Dice (the formulas are in include/svr_abi.h) from the integers of region_compare; `unit` is the length of sqrt(d2) = 1, e.g.
    the unit of distance_weights.  NaN where a denominator is 0."""
    lib = lib if lib is not None else abi.load()
    m = abi.CompareMeasurement()
    _host_call(lib, "svr_region_compare_measure", lib.svr_region_compare_measure(C.byref(comparison), float(unit), C.byref(m)))
    return m


def _image_size(w, h):
    w, h = int(w), int(h)
    if w < 1 or h < 1 or w * h > 1 << 31:
        raise ValueError(f"an image of {w} x {h} pixels: w and h must be at least 1 and w * h at most 2^31")
    return w, h


def _contours_q8(contours):
    """(int32 (x, y) pairs in 1/256 pixel, uint32 vertex counts) of a list of (n, 2) pixel arrays; ValueError for what the library refuses"""
    if isinstance(contours, np.ndarray) and contours.ndim == 2:
        contours = [contours]
    if len(contours) == 0:
        raise ValueError("a polygon needs at least one contour")
    parts = []
    for k, c in enumerate(contours):
        a = np.asarray(c, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 3:
            raise ValueError(f"contour {k} must be an (n, 2) array of (x, y) with n >= 3")
        if not np.isfinite(a).all():
            raise ValueError(f"contour {k} holds a coordinate that is not finite")
        q = np.rint(a * 256.0)
        if np.abs(q).max() > abi.STENCIL_MAX_COORD:
            raise ValueError(f"contour {k} holds a coordinate beyond 2^23 / 256 = 32768 pixels")
        parts.append(q.astype(np.int32))
    counts = np.array([len(q) for q in parts], dtype=np.uint32)
    if int(counts.sum()) > abi.STENCIL_MAX_VERTICES:
        raise ValueError(f"more than {abi.STENCIL_MAX_VERTICES} vertices")
    return np.ascontiguousarray(np.concatenate(parts)), counts


def _stencil_words(stencil, w: int, h: int):
    """The stencil operand of a w x h image: a bool image [h][w] packed, uint32 words checked for their number, a device pointer as it is"""
    if not isinstance(stencil, np.ndarray):
        if stencil is None:
            raise ValueError("a stencil is needed")
        return int(stencil)
    if stencil.dtype == bool:
        if stencil.shape != (h, w):
            raise ValueError(f"the stencil image must be [{h}][{w}] (got {list(stencil.shape)})")
        return region_mask_pack(stencil.reshape(1, h, w))
    words = region_mask_words((1, h, w))
    if stencil.dtype != np.uint32 or stencil.shape != (words,):
        raise ValueError(f"the stencil must be a bool image [{h}][{w}] or its {words} uint32 words")
    return np.ascontiguousarray(stencil)


def scissor_params(op: int = abi.SCISSOR_SELECT, depth=(-np.inf, np.inf)) -> abi.ScissorParams:
    """svr_scissor_params with the op and the closed depth interval (lo, hi); flags 0"""
    return abi.ScissorParams(int(op), float(depth[0]), float(depth[1]), 0)


def stencil_rect(x0: int, y0: int, x1: int, y1: int, lib=None) -> np.ndarray:
    """svr_stencil_rect: the contour, a float (4, 2) array in pixels, of the inclusive pixel rectangle x0 .. x1, y0 .. y1.  Host code of the
    library, as the two projections below: no device is needed."""
    lib = lib if lib is not None else abi.load()
    q = (C.c_int32 * 8)()
    _host_call(lib, "svr_stencil_rect", lib.svr_stencil_rect(int(x0), int(y0), int(x1), int(y1), q))
    return np.array(list(q), dtype=np.float64).reshape(4, 2) / 256.0


def scissor_project_camera(camera, point, lib=None):
    """svr_scissor_project_camera: ((x, y), depth) of the pixel at which the pinhole camera sees a world point and its depth along the
    view axis; (None, depth) when it is seen at no pixel."""
    lib = lib if lib is not None else abi.load()
    xy, depth, pt = (C.c_int32 * 2)(), C.c_float(0.0), _to_vec3(point)
    rc = _host_call(lib, "svr_scissor_project_camera", lib.svr_scissor_project_camera(C.byref(camera), C.byref(pt), xy, C.byref(depth)), ok=(0, 1))
    return ((int(xy[0]), int(xy[1])) if rc == 0 else None), float(depth.value)


def scissor_project_slice(slice, w: int, h: int, point, lib=None):
    """svr_scissor_project_slice: the same through the orthographic window of slice 0 of a SliceParams on a w x h image; depth is the
    signed distance from the plane along its normal."""
    lib = lib if lib is not None else abi.load()
    xy, depth, pt = (C.c_int32 * 2)(), C.c_float(0.0), _to_vec3(point)
    rc = _host_call(lib, "svr_scissor_project_slice", lib.svr_scissor_project_slice(C.byref(slice), int(w), int(h), C.byref(pt), xy, C.byref(depth)),
                    ok=(0, 1))
    return ((int(xy[0]), int(xy[1])) if rc == 0 else None), float(depth.value)


def _radii(radii):
    r = [int(t) for t in radii]
    if len(r) != 3 or min(r) < 0:
        raise ValueError("the radii must be three integers >= 0 (rx, ry, rz)")
    return (C.c_uint32 * 3)(*r)


def region_box_size(radii, lib=None) -> int:
    """svr_region_box_size: N = (2rx+1)(2ry+1)(2rz+1), the voxels of a smoothing window; 0 for a radius above 8.  Host code of the
    library: no device is needed."""
    lib = lib if lib is not None else abi.load()
    return int(lib.svr_region_box_size(_radii(radii)))


def region_smooth_radii(spacing, size, lib=None):
    """svr_region_smooth_radii: ((rx, ry, rz), (sx, sy, sz)) for a spacing and a window size in the spacing's units: the radii of the odd
    window nearest to the size, max(0, llround((size / spacing[a] - 1) / 2)), and the size each one spans, (2 r + 1) spacing[a].  Host
    code of the library: no device is needed."""
    lib = lib if lib is not None else abi.load()
    sp = (C.c_double * 3)(*[float(t) for t in spacing])
    r, so = (C.c_uint32 * 3)(), (C.c_double * 3)()
    _host_call(lib, "svr_region_smooth_radii", lib.svr_region_smooth_radii(sp, float(size), r, so))
    return (int(r[0]), int(r[1]), int(r[2])), (float(so[0]), float(so[1]), float(so[2]))


def _slice_axis(axis) -> int:
    axis = int(axis)
    if axis not in (0, 1, 2):
        raise ValueError(f"the axis must be 0, 1 or 2 for x, y, z (got {axis})")
    return axis


def _slice_list(noun: str, values, n_axis: Optional[int], increasing: bool) -> np.ndarray:
    """Slice numbers as a contiguous int32 array; ValueError for what the library refuses about them"""
    ks = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
    if len(ks) and (ks.min() < 0 or (n_axis is not None and ks.max() >= n_axis)):
        raise ValueError(f"the {noun} must lie inside the axis" + (f", in 0 .. {n_axis - 1}" if n_axis is not None else ""))
    if increasing and len(ks) > 1 and (np.diff(ks) <= 0).any():
        raise ValueError(f"the {noun} must increase strictly")
    return ks.astype(np.int32)


def fill_between_params(axis: int = 2, keys=None, weights=None, keep_between: bool = False, gap_by_gap: bool = False,
                        n_axis: Optional[int] = None) -> abi.FillBetweenParams:
    """svr_fill_between_params of the axis, the keys (None = every non-empty slice), the weights (None = 1, 1, 1) and the flags.  The
    struct keeps the key array alive.  n_axis: the length of the axis, to check the keys against."""
    p = abi.FillBetweenParams()
    p.axis = _slice_axis(axis)
    p.flags = (abi.FILL_KEEP_BETWEEN if keep_between else 0) | (abi.FILL_GAP_BY_GAP if gap_by_gap else 0)
    if weights is not None:
        w = [int(t) for t in weights]
        if len(w) != 3 or min(w) < 1:
            raise ValueError("the weights must be three integers >= 1")
        p.weights[:] = w
    if keys is not None:
        ks = _slice_list("keys", keys, n_axis, increasing=True)
        p.nkeys = len(ks)
        p._keys = ks if len(ks) else np.zeros(1, dtype=np.int32)      # (the struct holds its address; an empty list is still a list)
        p.keys = p._keys.ctypes.data_as(C.POINTER(C.c_int32))
    return p


def resample_grid(grid) -> abi.ResampleGrid:
    """A ResampleGrid from ((origin, step, count) of x, of y, of z); a ResampleGrid is returned as it is."""
    if isinstance(grid, abi.ResampleGrid):
        return grid
    g = abi.ResampleGrid()
    for a in range(3):
        g.axis[a].origin, g.axis[a].step, g.axis[a].count = (int(t) for t in grid[a])
    return g


def _grid_box_args(shape, box):
    b0, b1 = (None, None) if box is None else (_i32x3(box[0]), _i32x3(box[1]))
    return _dims(tuple(shape)), b0, b1


def resample_grid_box(shape, box, lib=None) -> abi.ResampleGrid:
    """svr_resample_grid_box: the grid of a crop of a [nz][ny][nx] volume to box = ((x0, y0, z0), (x1, y1, z1)), inclusive, cut to the
    volume.  The grid helpers are host code of the library: no device is needed."""
    lib = lib if lib is not None else abi.load()
    dims, b0, b1 = _grid_box_args(shape, box)
    g = abi.ResampleGrid()
    _host_call(lib, "svr_resample_grid_box", lib.svr_resample_grid_box(dims, b0, b1, C.byref(g)))
    return g


def resample_grid_spacing(shape, src_spacing, target_spacing, box=None, lib=None):
    """svr_resample_grid_spacing: (grid, spacing applied) for resampling a [nz][ny][nx] volume (or a box of it) from src_spacing to
    target_spacing, both (x, y, z); a scalar target means isotropic."""
    lib = lib if lib is not None else abi.load()
    dims, b0, b1 = _grid_box_args(shape, box)
    target = [float(target_spacing)] * 3 if np.isscalar(target_spacing) else [float(t) for t in target_spacing]
    g, out = abi.ResampleGrid(), (C.c_double * 3)()
    _host_call(lib, "svr_resample_grid_spacing", lib.svr_resample_grid_spacing(dims, (C.c_double * 3)(*[float(t) for t in src_spacing]), b0, b1,
                                                                                (C.c_double * 3)(*target), C.byref(g), out))
    return g, (float(out[0]), float(out[1]), float(out[2]))


def resample_grid_dims(shape, out_shape, box=None, lib=None) -> abi.ResampleGrid:
    """svr_resample_grid_dims: the grid that maps a [nz][ny][nx] volume (or a box of it) onto out_shape = (nz', ny', nx')."""
    lib = lib if lib is not None else abi.load()
    dims, b0, b1 = _grid_box_args(shape, box)
    g = abi.ResampleGrid()
    _host_call(lib, "svr_resample_grid_dims", lib.svr_resample_grid_dims(dims, b0, b1, _dims(tuple(out_shape)), C.byref(g)))
    return g


def resample_grid_place(volume: cudaVolume, shape, grid, lib=None) -> cudaVolume:
    """svr_resample_grid_place: a copy of `volume` (the cudaVolume of the [nz][ny][nx] source) whose box and spacing are those of the
    resampled volume, where it lay inside the source's box.  tex is copied: the caller replaces it."""
    lib = lib if lib is not None else abi.load()
    dims, _, _ = _grid_box_args(shape, None)
    g, out = resample_grid(grid), cudaVolume()
    _host_call(lib, "svr_resample_grid_place", lib.svr_resample_grid_place(C.byref(volume), dims, C.byref(g), C.byref(out)))
    return out


def region_seed_from_world(lib, volume: cudaVolume, dim, point):
    """svr_region_seed_from_world: the voxel (x, y, z) whose cell contains a world point (e.g. a svr_hit position); dim = (nx, ny, nz).
    Host code of the library: no device is needed."""
    ijk = (C.c_int32 * 3)()
    pt = _to_vec3(point)
    _host_call(lib, "svr_region_seed_from_world", lib.svr_region_seed_from_world(C.byref(volume), int(dim[0]), int(dim[1]), int(dim[2]), C.byref(pt), ijk))
    return (int(ijk[0]), int(ijk[1]), int(ijk[2]))
