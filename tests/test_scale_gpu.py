"""The volume operations beyond one trip of their launch code, on the GPU through the raw C ABI on buffers the test owns: the smallest
shapes past every launch threshold (a second trip of a capped grid, a second plane of a grid split over y and z, a fourth scan level,
2^32 lanes) against the full numpy / scipy references, and two large volumes whose byte offsets pass 2^31 and 2^32 against the small
references run on cut-outs around sparse contents.  Every comparison is equality.  tests/scale_ref.py holds the shapes and the builders;
tests/test_scale_cpu.py shows that each shape is past its threshold."""
import ctypes as C

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import distance_ref as dr
from tests import filter_ref as fr
from tests import label_ref as lr
from tests import mesh_ref as mr
from tests import region_ref as rr
from tests import resample_ref as rs
from tests import scale_ref as sr
from tests.test_filter_gpu import Filt
from tests.test_filter_gpu import same as same_volume
from tests.test_label_gpu import same_table
from tests.test_mesh_gpu import check as same_mesh
from tests.test_region_gpu import same_stats
from tests.test_resample_gpu import GUARD, Rs
from tests.test_resample_gpu import same as same_array

pytestmark = pytest.mark.gpu

PATTERN = 0xA5


class Vol:
    """Raw calls on buffers the test owns, for a [nz][ny][nx] volume of any size: buffers are pre-filled with a pattern (or a given
    byte), small pieces are written and read at element offsets, and the calls return what they report."""

    def __init__(self, dev, shape):
        self.dev, self.lib, self.shape = dev, dev.lib, tuple(int(n) for n in shape)
        self.dims = (self.shape[2], self.shape[1], self.shape[0])
        self.dims3 = (C.c_int32 * 3)(*self.dims)
        self.words = host.region_mask_words(self.shape)
        self.wx = (self.shape[2] + 31) // 32
        self.n = sr.voxels(self.shape)
        self.bufs = []

    # ---- memory
    def raw(self, nbytes, fill=PATTERN):
        p = self.dev.malloc(max(int(nbytes), 4))
        self.bufs.append(p)
        self.dev.check(self.lib.svr_memset_device(C.c_void_p(p), fill, max(int(nbytes), 4)))
        return p

    def put(self, arr):
        a = np.ascontiguousarray(arr)
        p = self.raw(a.nbytes)
        self.dev.to_device(p, a)
        return p

    def poke(self, ptr, dtype, at, values):
        """values -> elements at, at + 1, ... of the `dtype` array at ptr"""
        a = np.ascontiguousarray(values, dtype=dtype).reshape(-1)
        self.dev.to_device(ptr + int(at) * a.itemsize, a)

    def peek(self, ptr, dtype, at, count):
        return self.dev.to_host(ptr + int(at) * np.dtype(dtype).itemsize, (int(count),), dtype)

    def reserve(self, *nbytes, headroom=0):
        """All the buffers of a large test at once, pattern-filled, and `headroom` bytes for what the calls allocate themselves (taken and
        given back).  Skips the test if the device has not got the memory; any other failure is one."""
        ptrs = []
        try:
            for n in nbytes:
                ptrs.append(self.dev.malloc(max(int(n), 4)))
            if headroom:
                self.dev.free(self.dev.malloc(int(headroom)))
        except host.SvrError as e:
            for p in ptrs:
                self.dev.free(p)
            if "OutOfMemory" in str(e):
                pytest.skip(f"the device has not got {(sum(nbytes) + headroom) / 2 ** 30:.1f} GiB: {e}")
            raise
        self.bufs += ptrs
        for p, n in zip(ptrs, nbytes):
            self.fill(p, PATTERN, n)
        return ptrs

    def fill(self, ptr, byte, nbytes):
        self.dev.check(self.lib.svr_memset_device(C.c_void_p(ptr), byte, max(int(nbytes), 4)))

    def write_volume(self, ptr, sparse):
        """u16: 0 everywhere, the points of a scale_ref.Sparse on top."""
        self.fill(ptr, 0, 2 * self.n)
        for at, run in sparse.x_runs():
            self.poke(ptr, np.uint16, at, run)

    def write_map(self, ptr, values):
        """uint32: 0 everywhere but at {point: value}."""
        self.fill(ptr, 0, 4 * self.n)
        for (z, y, x), v in values.items():
            self.poke(ptr, np.uint32, (z * self.shape[1] + y) * self.shape[2] + x, [v])

    def volume_of(self, sparse):
        p = self.raw(2 * self.n, 0)
        self.write_volume(p, sparse)
        return p

    def mask_of(self, points, dirty=True):
        p = self.raw(4 * self.words, 0)
        self.write_mask(p, points, dirty)
        return p

    def write_mask(self, p, points, dirty=True):
        """A device mask with exactly `points` set.  dirty: the padding bits of the words written are set as well (they are ignored)."""
        self.fill(p, 0, 4 * self.words)
        idx, w = sr.sparse_words(self.shape, points)
        pad = np.uint32(0)
        if dirty and self.shape[2] % 32:
            pad = np.uint32((0xFFFFFFFF << (self.shape[2] % 32)) & 0xFFFFFFFF)
        for i, word in zip(idx.tolist(), w.tolist()):
            last = i % self.wx == self.wx - 1
            self.poke(p, np.uint32, i, [np.uint32(word) | (pad if last else np.uint32(0))])

    def free(self, *ptrs):
        for p in ptrs:
            self.bufs.remove(p)
            self.dev.free(p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.dev.synchronize()
        for p in self.bufs:
            self.dev.free(p)
        self.bufs = []

    # ---- calls
    def ok(self, rc):
        msg = self.lib.svr_last_error().decode()
        self.lib.svr_clear_error()
        assert rc == 0, msg

    def threshold(self, vox, lo, hi, out):
        self.ok(self.lib.svr_region_threshold(C.c_void_p(vox), *self.dims, 1, lo, hi, None, None, C.c_void_p(out)))
        self.dev.synchronize()

    def grow(self, vox, seeds, lo, hi, conn, out):
        p = self.dev.region_params(lo, hi, conn)
        xyz = (C.c_int32 * (3 * len(seeds)))(*[c for s in seeds for c in s])
        st = abi.RegionStats()
        self.ok(self.lib.svr_region_grow(C.c_void_p(vox), *self.dims, 1, xyz, len(seeds), C.byref(p), C.c_void_p(out), C.byref(st)))
        return st

    def stats_of(self, vox, mask):
        st = abi.RegionStats()
        self.ok(self.lib.svr_region_stats_of(C.c_void_p(vox), *self.dims, 1, C.c_void_p(mask), C.byref(st)))
        return st

    def apply(self, vox, mask, mode, fill, out):
        self.ok(self.lib.svr_region_apply(C.c_void_p(vox), *self.dims, 1, C.c_void_p(mask), mode, fill, C.c_void_p(out)))
        self.dev.synchronize()

    def morph(self, mask, op, element, radius, out):
        self.ok(self.lib.svr_region_morph(C.c_void_p(mask), *self.dims, op, element, radius, C.c_void_p(out)))
        self.dev.synchronize()

    def fill_holes(self, mask, conn, out):
        self.ok(self.lib.svr_region_fill_holes(C.c_void_p(mask), *self.dims, conn, 0, C.c_void_p(out)))
        self.dev.synchronize()

    def label(self, mask, conn, out):
        k = C.c_uint32(0xFFFFFFFF)
        self.ok(self.lib.svr_region_label(C.c_void_p(mask), *self.dims, conn, C.c_void_p(out), C.byref(k)))
        return int(k.value)

    def table(self, labels, count, vox=None):
        out = self.raw(40 * max(count, 1))
        self.ok(self.lib.svr_region_label_table(C.c_void_p(labels), None if vox is None else C.c_void_p(vox), *self.dims, 1, count, C.c_void_p(out)))
        self.dev.synchronize()
        return out, self.dev.to_host(out, (count,), host.COMPONENT_DTYPE)

    def select(self, labels, count, keep, out):
        k = self.put(np.asarray(keep, dtype=np.uint8))
        self.ok(self.lib.svr_region_select(C.c_void_p(labels), *self.dims, count, C.c_void_p(k), C.c_void_p(out)))
        self.dev.synchronize()
        self.free(k)

    def by_size(self, labels, count, table, min_voxels, largest_k, out):
        k = C.c_uint32(0xFFFFFFFF)
        self.ok(self.lib.svr_region_select_by_size(C.c_void_p(labels), *self.dims, count, C.c_void_p(table), min_voxels, largest_k, C.c_void_p(out),
                                                   C.byref(k)))
        self.dev.synchronize()
        return int(k.value)

    def distance(self, mask, target, out, weights=None):
        w = None if weights is None else (C.c_uint32 * 3)(*weights)
        self.ok(self.lib.svr_region_distance(C.c_void_p(mask), *self.dims, w, target, C.c_void_p(out)))
        self.dev.synchronize()

    def distance_select(self, dmap, lo2, hi2, out):
        self.ok(self.lib.svr_region_distance_select(C.c_void_p(dmap), *self.dims, lo2, hi2, C.c_void_p(out)))
        self.dev.synchronize()

    def ball(self, mask, op, r2, out):
        self.ok(self.lib.svr_region_ball(C.c_void_p(mask), *self.dims, op, None, r2, C.c_void_p(out)))
        self.dev.synchronize()

    def dmax(self, dmap, mask=None):
        m, first, status = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF), C.c_int32(-1)
        self.ok(self.lib.svr_region_distance_max(C.c_void_p(dmap), None if mask is None else C.c_void_p(mask), *self.dims, C.byref(m), C.byref(first),
                                                 C.byref(status)))
        return int(m.value), int(first.value), int(status.value)

    def paint(self, labels, mask, label, only_unlabelled):
        self.ok(self.lib.svr_region_label_paint(C.c_void_p(labels), self.dims3, C.c_void_p(mask), label, only_unlabelled))
        self.dev.synchronize()

    def rank(self, vox, op, element, out):
        self.ok(self.lib.svr_volume_rank(C.c_void_p(vox), *self.dims, 1, op, element, 1, C.c_void_p(out)))
        self.dev.synchronize()

    def smooth(self, vox, radii, out):
        self.ok(self.lib.svr_volume_smooth(C.c_void_p(vox), *self.dims, 1, (C.c_uint32 * 3)(*radii), C.c_void_p(out)))
        self.dev.synchronize()

    def geodesic(self, labels, domain, weights, dist, zones):
        sweeps = C.c_uint32(0xFFFFFFFF)
        self.ok(self.lib.svr_region_geodesic(C.c_void_p(labels), C.c_void_p(domain), *self.dims, (C.c_uint32 * 7)(*weights), 0, C.c_void_p(dist),
                                             C.c_void_p(zones), C.byref(sweeps)))
        return int(sweeps.value)

    def growcut(self, vox, labels, domain, weights, gain, shift, cost, zones):
        p, info = abi.GrowcutParams(), abi.GrowcutInfo()
        p.step_weights[:] = [int(w) for w in weights]
        p.contrast_gain, p.contrast_shift, p.max_sweeps = gain, shift, 0
        self.ok(self.lib.svr_region_growcut(C.c_void_p(vox), self.dims3, 1, C.c_void_p(labels), C.c_void_p(domain), C.byref(p), C.c_void_p(cost),
                                            C.c_void_p(zones), C.byref(info)))
        return info

    def crop(self, call, src, box_lo, counts, dtype, source_is_volume=False):
        """A crop-only resample of the box at box_lo (x, y, z) with `counts` voxels an axis, into a fresh guarded buffer: the array."""
        grid = host.resample_grid(tuple((lo << 16, 65536, n) for lo, n in zip(box_lo, counts)))
        shape = tuple(counts[::-1])
        nbytes = sr.voxels(shape) * np.dtype(dtype).itemsize
        out = self.raw(nbytes + GUARD)
        if source_is_volume:
            self.ok(call(C.c_void_p(src), self.dims3, 1, C.byref(grid), abi.RESAMPLE_NEAREST, C.c_void_p(out)))
        else:
            self.ok(call(C.c_void_p(src), self.dims3, C.byref(grid), C.c_void_p(out)))
        self.dev.synchronize()
        got = self.dev.to_host(out, (nbytes + GUARD,), np.uint8)
        self.free(out)
        assert (got[nbytes:] == PATTERN).all(), "memory past the end of out was written"
        return got[:nbytes].view(dtype).reshape(shape)

    # ---- comparisons against sparse expectations
    def peek_box(self, ptr, dtype, box):
        """The dense contents of the half-open box ((z0, y0, x0), (z1, y1, x1)) of the array at ptr, row by row."""
        (z0, y0, x0), (z1, y1, x1) = box
        out = np.empty((z1 - z0, y1 - y0, x1 - x0), dtype=dtype)
        for z in range(z0, z1):
            for y in range(y0, y1):
                out[z - z0, y - y0] = self.peek(ptr, dtype, (z * self.shape[1] + y) * self.shape[2] + x0, x1 - x0)
        return out

    def same_points(self, ptr, dtype, want, what, boxes, whole, background=0):
        """The voxel array at ptr is `background` but at want = {point: value}: read back whole, or only the boxes (which hold every
        point) where the caller covers the rest through a call that reduces the whole array."""
        if whole:
            items = sorted((((z * self.shape[1] + y) * self.shape[2] + x), v) for (z, y, x), v in want.items())
            idx, vals = np.array([i for i, _ in items], dtype=np.int64), np.array([v for _, v in items], dtype=np.int64)
            return self.same_sparse(ptr, dtype, self.n, (idx, vals), what, background)
        inside = 0
        for box in boxes:
            (z0, y0, x0), (z1, y1, x1) = box
            dense = np.full((z1 - z0, y1 - y0, x1 - x0), background, dtype=dtype)
            for (z, y, x), v in want.items():
                if z0 <= z < z1 and y0 <= y < y1 and x0 <= x < x1:
                    dense[z - z0, y - y0, x - x0] = v
                    inside += 1
            got = self.peek_box(ptr, dtype, box)
            if not np.array_equal(got, dense):
                at = tuple(np.argwhere(got != dense)[0].tolist())
                raise AssertionError(f"{what}: box {box}: {int((got != dense).sum())} entries differ; first at {at}: {int(got[at])} for {int(dense[at])}")
        assert inside == len(want), f"{what}: the boxes hold {inside} of the {len(want)} expected points"

    # ---- whole-buffer comparisons against sparse expectations
    def same_sparse(self, ptr, dtype, count, want, what, background=0):
        """The `count` elements at ptr are `background` but at the indices of want = (indices ascending, values)."""
        got = self.dev.to_host(ptr, (int(count),), dtype)
        idx, vals = want
        at = np.flatnonzero(got != background)
        if not np.array_equal(at, idx) or not np.array_equal(got[idx], np.asarray(vals).astype(dtype)):
            extra, missing = np.setdiff1d(at, idx)[:4].tolist(), np.setdiff1d(idx, at)[:4].tolist()
            wrong = [int(i) for i, v in zip(idx, vals) if got[i] != v][:4]
            raise AssertionError(f"{what}: {len(at)} entries differ from the background where {len(idx)} should; set but not expected at {extra}, "
                                 f"expected but not set at {missing}, wrong values at {wrong}: {[int(got[i]) for i in wrong]}")

    def same_mask(self, ptr, points, what):
        self.same_sparse(ptr, np.uint32, self.words, sr.sparse_words(self.shape, points), what)

    def same_map(self, ptr, values, what):
        """A uint32 map that is 0 but at {point: value}."""
        items = sorted((((z * self.shape[1] + y) * self.shape[2] + x), v) for (z, y, x), v in values.items())
        self.same_sparse(ptr, np.uint32, self.n, (np.array([i for i, _ in items], dtype=np.int64), np.array([v for _, v in items], dtype=np.int64)), what)


def same_words(got, want_mask, what):
    want = rr.pack(want_mask)
    if not np.array_equal(got, want):
        diff = rr.unpack(got ^ want, want_mask.shape)
        raise AssertionError(f"{what}: {int(diff.sum())} voxels differ; first (z, y, x) {np.argwhere(diff)[:1].tolist()}; "
                             f"padding differs: {not np.array_equal(rr.pack(rr.unpack(got, want_mask.shape)), got)}")


# ================================================================================================ mid tier
# ------------------------------------------------------------------------------------------------ region: a second trip of the span loop
@pytest.mark.parametrize("vector", [8, 1], ids=["vector-8", "scalar"])
def test_region_calls_span_both_trips(hip_dev, vector):
    vox, seeds, region, stats = sr.region_case(vector)
    shape = vox.shape
    lo, hi = rr.NOISE_LO, rr.NOISE_HI
    cand = rr.candidates(vox, lo, hi)
    with Vol(hip_dev, shape) as g:
        d_vox, d_mask = g.put(vox), g.raw(4 * g.words)
        assert (d_vox % 16 == 0) and (shape[2] % 8 == 0) == (vector == 8)                   # the path: vec8_ok of svr_region.hip
        g.threshold(d_vox, lo, hi, d_mask)
        same_words(hip_dev.to_host(d_mask, (g.words,), np.uint32), cand, f"{shape} threshold")
        same_stats(g.stats_of(d_vox, d_mask), rr.cached(("scale", "cand stats", vector), lambda: rr.stats(vox, cand)), f"{shape} stats of the window")
        grown = g.raw(4 * g.words, 0xFF)
        st = g.grow(d_vox, seeds, lo, hi, 6, grown)
        same_words(hip_dev.to_host(grown, (g.words,), np.uint32), region, f"{shape} grow")
        same_stats(st, stats, f"{shape} grow")
        same_stats(g.stats_of(d_vox, grown), stats, f"{shape} stats of the region")
        out = g.raw(2 * g.n + GUARD)
        for mode in (abi.REGION_KEEP, abi.REGION_REMOVE):
            g.apply(d_vox, grown, mode, 1000, out)
            got = hip_dev.to_host(out, (2 * g.n + GUARD,), np.uint8)
            assert (got[2 * g.n:] == PATTERN).all(), "memory past the end of out was written"
            same_volume(got[:2 * g.n].view(np.uint16).reshape(shape), rr.apply(vox, region, mode, 1000), f"{shape} apply mode {mode}")
        assert np.array_equal(hip_dev.to_host(d_vox, shape, np.uint16), vox)                # the source is not written
        g.apply(d_vox, grown, abi.REGION_KEEP, 7, d_vox)                                  # in place
        same_volume(hip_dev.to_host(d_vox, shape, np.uint16), rr.apply(vox, region, rr.KEEP, 7), f"{shape} apply in place")


# ------------------------------------------------------------------------------------------------ filter: a second plane of the row grid
SMOOTH_RADII = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (8, 0, 0), (0, 8, 0), (0, 0, 8), (8, 8, 8)]


@pytest.mark.parametrize("radii", SMOOTH_RADII, ids=lambda r: "-".join(str(t) for t in r))
def test_smooth_past_one_grid_plane(hip_dev, radii):
    vol = sr.filter_volume()
    with Filt(hip_dev, sr.FILTER_SHAPE) as f:
        same_volume(f.smooth(f.put(vol), radii, f.out(), str(radii)), fr.smooth(vol, radii), f"{sr.FILTER_SHAPE} smooth {radii}")


def test_median_26_on_the_filter_shape(hip_dev):
    vol = sr.filter_volume()
    with Filt(hip_dev, sr.FILTER_SHAPE) as f:
        same_volume(f.rank(f.put(vol), abi.FILTER_MEDIAN, 26, 1, f.out(), "median 26"), fr.rank(vol, fr.MEDIAN, 26), f"{sr.FILTER_SHAPE} median 26")


# ------------------------------------------------------------------------------------------------ resample: a second plane of the row grid
RESAMPLE_MODES = {"nearest": (rs.NEAREST,), "linear": (rs.LINEAR,), "area": (rs.AREA,), "crop": (rs.NEAREST, rs.LINEAR, rs.AREA)}


@pytest.mark.parametrize("name", list(RESAMPLE_MODES))
def test_resample_past_one_grid_plane(hip_dev, name):
    grid, src = sr.resample_grid(name), sr.resample_source_shape(name)
    vol = fr.random_volume(src, 75)
    with Rs(hip_dev) as r:
        d_vol = r.put(vol)
        for mode in RESAMPLE_MODES[name]:
            want = rs.volume_resample(vol, grid, mode)
            assert want.shape == sr.RESAMPLE_OUT
            same_array(r.volume(d_vol, src, grid, mode, name), want, f"{name} mode {mode} onto {sr.RESAMPLE_OUT}")


@pytest.mark.parametrize("name", ["nearest", "crop"])
def test_resample_labels_and_masks_past_one_grid_plane(hip_dev, name):
    grid, src = sr.resample_grid(name), sr.resample_source_shape(name)
    rng = np.random.default_rng(76)
    labels = rng.integers(0, 1 << 32, size=src, dtype=np.uint64).astype(np.uint32)         # (the call moves any uint32)
    mask = rng.random(src) < 0.5
    g = host.resample_grid(grid)
    with Rs(hip_dev) as r:
        out = r.raw(4 * sr.voxels(sr.RESAMPLE_OUT) + GUARD)
        r.ok(r.lib.svr_region_label_resample(C.c_void_p(r.put(labels)), (C.c_int32 * 3)(*src[::-1]), C.byref(g), C.c_void_p(out)))
        same_array(r.fetch(out, sr.RESAMPLE_OUT, np.uint32, name), rs.nearest_any(labels, grid), f"labels {name}")
        got = r.mask_words(r.put(sr.garbage_padded(mask, 77)), src, grid, name)
        same_words(got, rs.nearest_any(mask, grid), f"mask {name}")


# ------------------------------------------------------------------------------------------------ distance_max: a second trip of the stride loop
def test_distance_max_beyond_the_first_trip(hip_dev):
    noise = sr.distance_map_noise()
    early, late, peak = sr.DISTANCE_EARLY, sr.DISTANCE_LATE, sr.DISTANCE_PEAK
    mask = np.random.default_rng(78).random(sr.DISTANCE_SHAPE) < 0.5
    mask[early] = mask[late] = True
    without_early = mask.copy()
    without_early[early] = False
    index = sr.Sparse(sr.DISTANCE_SHAPE, {}).index
    with Vol(hip_dev, sr.DISTANCE_SHAPE) as g:
        d_mask, d_without = g.put(sr.garbage_padded(mask, 79)), g.put(rr.pack(without_early))
        for name, planted in (("only late", {late: peak}), ("both", {early: peak, late: peak}), ("late is larger", {early: peak, late: peak + 1}),
                              ("neither", {})):
            m = noise.copy()
            for p, v in planted.items():
                m[p] = v
            d_map = g.put(m)
            for what, dm, hm in (("unmasked", None, None), ("masked", d_mask, mask), ("masked without the early one", d_without, without_early)):
                want = dr.dmax(m, hm)
                assert g.dmax(d_map, dm) == want, (name, what, want)
            g.free(d_map)
        # what the cases are there for, on the reference
        m = noise.copy()
        m[late] = peak
        assert dr.dmax(m)[:2] == (peak, index(late))
        m[early] = peak
        assert dr.dmax(m)[:2] == (peak, index(early)) and dr.dmax(m, without_early)[:2] == (peak, index(late))


# ------------------------------------------------------------------------------------------------ mesh: more vertices than one trip
@pytest.mark.parametrize("relax", [0, 3])
def test_mesh_with_more_vertices_than_one_trip(hip_dev, relax):
    mask = sr.mesh_mask()
    want = mr.mesh_region(mask, relax)
    assert len(want[0]) > sr.BBOX_TRIP
    with Vol(hip_dev, sr.MESH_SHAPE) as g:
        got = hip_dev.mesh_region(g.put(sr.garbage_padded(mask, 80)), relax, shape=sr.MESH_SHAPE)
    same_mesh(got, want, f"noise mask relax {relax}")
    scale = (0.7 / 256, 0.9 / 256, 1.5 / 256)
    vol6, area = hip_dev.mesh_measure(got[0], got[1], scale)
    want_area = mr.area(want[0], want[1], scale)
    assert vol6 == mr.volume6(want[0], want[1]) and abs(area - want_area) <= 1e-9 * want_area


# ------------------------------------------------------------------------------------------------ label: a fourth scan level
def narrow_words(mask, seed):
    """The words of a mask of a volume with nx = 1 (one word a voxel), the 31 padding bits of every word random."""
    junk = np.random.default_rng(seed).integers(0, 1 << 32, size=mask.size, dtype=np.uint64).astype(np.uint32)
    return (junk & np.uint32(0xFFFFFFFE)) | mask.reshape(-1).astype(np.uint32)


def same_narrow_mask(got, want_mask, what):
    if not np.array_equal(got, want_mask.reshape(-1).astype(np.uint32)):
        diff = got != want_mask.reshape(-1)
        raise AssertionError(f"{what}: {int(diff.sum())} words differ; first at {int(np.flatnonzero(diff)[0])}: {int(got[np.flatnonzero(diff)[0]])}")


def check_big_labelling(g, mask, conn, want, want_k, what, sizes=((3, 1000),)):
    """Labels, K, the table and selections by size of a mask of the label shape against `want`."""
    dev = g.dev
    d_mask, d_labels = g.put(narrow_words(mask, 81)), g.raw(4 * g.n)
    k = g.label(d_mask, conn, d_labels)
    got = dev.to_host(d_labels, g.shape, np.uint32)
    if k != want_k or not np.array_equal(got, want):
        diff = got != want
        raise AssertionError(f"{what}: K {k} (reference {want_k}); {int(diff.sum())} labels differ, first (z, y, x) {np.argwhere(diff)[:1].tolist()}")
    d_table, t = g.table(d_labels, k)
    want_t = sr.fast_table(want, want_k)
    same_table(t, want_t, what + ", table")
    out = g.raw(4 * g.words)
    for min_voxels, largest_k in sizes:
        keep = sr.fast_kept(want_t["voxels"], min_voxels, largest_k)
        kept = g.by_size(d_labels, k, d_table, min_voxels, largest_k, out)
        assert kept == int(keep.sum()), (what, min_voxels, largest_k, kept, int(keep.sum()))
        same_narrow_mask(dev.to_host(out, (g.words,), np.uint32), keep[want].astype(bool), f"{what}, by size {min_voxels} / {largest_k}")
    return want_t


@pytest.mark.parametrize("conn", [6, 26])
def test_label_through_four_scan_levels(hip_dev, conn):
    mask = rr.cached(("scale", "label mask"), sr.label_random)
    want, want_k = sr.scipy_label(mask, conn)
    assert want_k > 1 << 16
    with Vol(hip_dev, sr.LABEL_SHAPE) as g:
        t = check_big_labelling(g, mask, conn, want, want_k, f"{sr.LABEL_SHAPE} random, {conn}", sizes=((3, 1000), (0, 1), (2, 0)))
        assert int(t["voxels"].sum()) == int(mask.sum())


def test_label_every_other_voxel_has_more_than_2_to_the_23_components(hip_dev):
    mask = sr.label_checker()
    want_k = sr.label_checker_count()
    want = np.zeros(mask.shape, dtype=np.uint32)
    want[mask] = np.arange(1, want_k + 1, dtype=np.uint32)                                 # each set voxel a component, in scan order
    assert want_k > 1 << 23
    with Vol(hip_dev, sr.LABEL_SHAPE) as g:
        check_big_labelling(g, mask, 6, want, want_k, f"{sr.LABEL_SHAPE} every other voxel", sizes=((0, 5), (2, 0)))


# ------------------------------------------------------------------------------------------------ narrow rows: 2^27 words, 2^32 lanes
def narrow():
    return sr.Sparse(sr.NARROW_SHAPE, sr.narrow_points())


def test_narrow_rows_threshold(hip_dev):
    s = narrow()
    lo, hi = sr.NARROW_WINDOW
    with Vol(hip_dev, s.shape) as g:
        d_vox, out = g.volume_of(s), g.raw(4 * g.words)
        g.threshold(d_vox, lo, hi, out)
        g.same_mask(out, s.points, "threshold of the whole window")
        half = {p: v for p, v in s.points.items() if v % 2}
        g.poke(d_vox, np.uint16, 5000, [hi + 1])                                           # one voxel outside the window
        for p, v in s.points.items():
            if p not in half:
                g.poke(d_vox, np.uint16, s.index(p), [lo - 1])
        g.threshold(d_vox, lo, hi, out)
        g.same_mask(out, half, "threshold of every other point")


@pytest.mark.parametrize("conn", [6, 26])
def test_narrow_rows_label_table_and_select(hip_dev, conn):
    s = narrow()
    labelling, k = s.labels(conn)
    with Vol(hip_dev, s.shape) as g:
        d_vox, d_mask, d_labels = g.volume_of(s), g.mask_of(s.points), g.raw(4 * g.n)
        g.poke(d_mask, np.uint32, 12345, [0xFFFFFFFE])                                      # only padding bits: not a voxel
        assert g.label(d_mask, conn, d_labels) == k
        g.same_map(d_labels, labelling, f"labels, {conn}")
        d_table, t = g.table(d_labels, k, d_vox)
        want_t = s.table(labelling, k, s.points)
        same_table(t, want_t, f"table, {conn}")
        out = g.raw(4 * g.words)
        keep = np.zeros(k + 1, dtype=np.uint8)
        keep[[1, k]] = 1
        g.select(d_labels, k, keep, out)
        g.same_mask(out, [p for p, lab in labelling.items() if lab in (1, k)], f"select first and last, {conn}")
        kept_labels = lr.kept_labels(want_t["voxels"], 2, 3)
        assert g.by_size(d_labels, k, d_table, 2, 3, out) == len(kept_labels) == 3
        g.same_mask(out, [p for p, lab in labelling.items() if lab in kept_labels], f"by size, {conn}")


def test_narrow_rows_distance_select_and_max(hip_dev):
    s = narrow()
    nz, ny, _ = s.shape
    with Vol(hip_dev, s.shape) as g:
        d_mask, d_map, out = g.mask_of(s.points), g.raw(4 * g.n), g.raw(4 * g.words)
        # to the nearest unset voxel: 0 off the points, and local on them
        unset = s.apply(4, lambda m: np.where(m > 0, dr.distance_map(m > 0, (1, 1, 1), dr.TO_UNSET), 0))
        assert sorted(unset) == sorted(s.points) and set(unset.values()) == {1, 2}
        g.distance(d_mask, abi.DIST_TO_UNSET, d_map)
        g.same_map(d_map, unset, "distance to unset")
        g.distance_select(d_map, 2, 0xFFFFFFFE, out)
        g.same_mask(out, [p for p, v in unset.items() if v == 2], "select d2 >= 2")
        first = min(s.index(p) for p, v in unset.items() if v == 2)
        assert g.dmax(d_map) == (2, first, rr.OK) and g.dmax(d_map, d_mask) == (2, first, rr.OK)
        # to the nearest set voxel: every voxel has one; compared on random voxels and around the points, and through the selection
        g.distance(d_mask, abi.DIST_TO_SET, d_map)
        sites = np.array(sorted(s.points), dtype=np.int64)
        rng = np.random.default_rng(82)
        at = np.unique(np.concatenate([rng.integers(0, g.n, size=1 << 16), s.indices()[0], s.indices()[0] + 3, [0, g.n - 1, 1 << 26, (1 << 26) - 1]]))
        at = at[at < g.n]
        z, y = at // ny, at % ny
        want = ((z[:, None] - sites[None, :, 0]) ** 2 + (y[:, None] - sites[None, :, 1]) ** 2).min(axis=1)
        assert int(want.max()) <= dr.LIMIT
        got = hip_dev.to_host(d_map, (g.n,), np.uint32)
        bad = np.flatnonzero(got[at] != want)
        assert len(bad) == 0, f"distance to set: {len(bad)} of {len(at)} sampled entries differ, first at voxel {int(at[bad[0]])}: {int(got[at[bad[0]]])} for {int(want[bad[0]])}"
        del got
        g.distance_select(d_map, 0, 4, out)
        near = s.apply(4, lambda m: dr.dilate(m > 0, 4))
        g.same_mask(out, near, "select d2 <= 4")
        # the maximum of a map the test writes: at the last voxel alone, then also before it -- the lower index wins
        g.dev.check(g.lib.svr_memset_device(C.c_void_p(d_map), 0, 4 * g.n))
        g.poke(d_map, np.uint32, g.n - 1, [77])
        assert g.dmax(d_map) == (77, g.n - 1, rr.OK)
        g.poke(d_map, np.uint32, (1 << 26) + 1, [77])
        assert g.dmax(d_map) == (77, (1 << 26) + 1, rr.OK)
        assert g.dmax(d_map, d_mask) == (77, (1 << 26) + 1, rr.OK)                         # both are points
        g.poke(d_map, np.uint32, g.n - 1, [78])
        assert g.dmax(d_map, d_mask) == (78, g.n - 1, rr.OK)


def test_narrow_rows_label_paint(hip_dev):
    s = narrow()
    with Vol(hip_dev, s.shape) as g:
        d_mask, d_labels = g.mask_of(s.points), g.raw(4 * g.n, 0)
        had = {p: 5 for p in list(sorted(s.points))[::3]}
        had[(100, 100, 0)] = 9                                                             # a label off the mask stays
        for p, v in had.items():
            g.poke(d_labels, np.uint32, s.index(p), [v])
        g.paint(d_labels, d_mask, 0x80000001, 1)
        want = {p: had.get(p, 0x80000001) for p in s.points}
        want[(100, 100, 0)] = 9
        g.same_map(d_labels, want, "paint only unlabelled")
        g.paint(d_labels, d_mask, 3, 0)
        want = {p: 3 for p in s.points}
        want[(100, 100, 0)] = 9
        g.same_map(d_labels, want, "paint")


# ================================================================================================ large tier
# Byte offsets past 2^31 and 2^32.  The contents are sparse -- beacons of tests/scale_ref.py at the corners, across the planes where the
# voxel index passes 2^28, 2^29, 2^30 and 3 * 2^29, and at the last voxel -- and the expected results are the small references run on
# cut-outs.  A truncated offset writes a beacon's result at an aliased address, so the rest of every output is checked as well: masks and
# the maps of L1 are read back whole; of the 4 and 8 GiB outputs of L2 the cut-outs are read back and the rest goes through a call that
# reduces the whole array to a mask or a number (threshold, select, distance_select, the component table, distance_max).
LARGE = {"L1": sr.L1, "L2": sr.L2}
MIB = 1 << 20
tiers = pytest.mark.parametrize("tier", list(LARGE))


def beacons(shape):
    return rr.cached(("scale", "beacons", shape), lambda: sr.Sparse(shape, sr.beacon_points(shape)))


def ones(sparse, points=None):
    """The mask of the points as a Sparse of value 1."""
    return sr.Sparse(sparse.shape, {p: 1 for p in (sparse.points if points is None else points)})


@tiers
def test_large_region_calls(hip_dev, tier):
    """threshold, grow from the far corner and the origin, stats_of, apply.  Device memory: two u16 volumes, three masks and the
    candidate mask of the grow call -- 4.5 n bytes for n voxels: 2.3 GiB at L1, 9 GiB at L2."""
    shape = LARGE[tier]
    s, whole = beacons(shape), tier == "L1"
    nz, ny, nx = shape
    lo, hi = sr.BEACON_WINDOW
    labelling, _ = s.labels(6)
    seeds = [(nx - 1, ny - 1, nz - 1), (0, 0, 0)]
    seeded = {labelling[(z, y, x)] for x, y, z in seeds}
    region = {p: s.points[p] for p, lab in labelling.items() if lab in seeded}
    assert len(region) == 4 * sr.BEACON ** 3 + 2 * sr.ROD                                   # either corner, its companion and the rod between them
    boxes = s.cutouts(2)
    with Vol(hip_dev, shape) as g:
        d_vox, d_out, m_all, m_grown, m_tmp = g.reserve(2 * g.n, 2 * g.n, 4 * g.words, 4 * g.words, 4 * g.words, headroom=8 * g.words + 64 * MIB)
        g.write_volume(d_vox, s)
        g.threshold(d_vox, lo, hi, m_all)
        g.same_mask(m_all, s.points, f"{tier} threshold")
        same_stats(g.stats_of(d_vox, m_all), s.stats(), f"{tier} stats of the window")
        st = g.grow(d_vox, seeds, lo, hi, 6, m_grown)
        g.same_mask(m_grown, region, f"{tier} grow")
        same_stats(st, s.stats(region), f"{tier} grow")
        same_stats(g.stats_of(d_vox, m_grown), s.stats(region), f"{tier} stats of the region")
        for mode, fill, want in ((abi.REGION_KEEP, 0, region), (abi.REGION_REMOVE, 60000, {p: (60000 if p in region else v) for p, v in s.points.items()})):
            g.apply(d_vox, m_grown, mode, fill, d_out)
            g.threshold(d_out, 1, 65535, m_tmp)                                              # the whole output: nothing else is non-zero
            g.same_mask(m_tmp, want, f"{tier} apply mode {mode}, non-zero voxels")
            g.same_points(d_out, np.uint16, want, f"{tier} apply mode {mode}", boxes, whole)


@tiers
def test_large_morph_and_fill_holes(hip_dev, tier):
    """dilate / erode by 1 and 4, open, fill_holes of a hollow beacon.  Device memory: two masks and the call's temporaries -- below
    1 GiB."""
    from tests import morph_ref as mo

    shape = LARGE[tier]
    s = beacons(shape)
    m = ones(s, set(s.points) - {sr.hollow_centre(shape)})
    with Vol(hip_dev, shape) as g:
        src, out = g.reserve(4 * g.words, 4 * g.words, headroom=16 * g.words)
        g.write_mask(src, m.points)
        for op, element, radius in ((abi.MORPH_DILATE, 6, 1), (abi.MORPH_ERODE, 6, 1), (abi.MORPH_DILATE, 26, 4), (abi.MORPH_ERODE, 18, 4),
                                    (abi.MORPH_OPEN, 6, 1)):
            want = m.apply(radius + 2, lambda c: mo.morph(c > 0, op, element, radius))
            assert want or op == abi.MORPH_ERODE
            g.morph(src, op, element, radius, out)
            g.same_mask(out, want, f"{tier} morph op {op} element {element} radius {radius}")
        want = m.apply(3, lambda c: mo.fill_holes(c > 0, 6))
        assert set(want) == set(s.points)
        g.fill_holes(src, 6, out)
        g.same_mask(out, want, f"{tier} fill holes")


@tiers
def test_large_label_table_and_select(hip_dev, tier):
    """label (6 and 26), select of every label, the table with sums, select_by_size.  Device memory: the label map, a u16 volume, two masks
    and the call's root mask and scan -- 6.4 n bytes: 3.2 GiB at L1, 12.8 GiB at L2."""
    shape = LARGE[tier]
    s, whole = beacons(shape), tier == "L1"
    boxes = s.cutouts(2)
    with Vol(hip_dev, shape) as g:
        d_labels, d_vox, d_mask, d_out = g.reserve(4 * g.n, 2 * g.n, 4 * g.words, 4 * g.words, headroom=12 * g.words)
        g.write_volume(d_vox, s)
        g.write_mask(d_mask, s.points)
        for conn in (26, 6):
            labelling, k = s.labels(conn)
            assert g.label(d_mask, conn, d_labels) == k == sr.beacon_components(shape)
            g.same_points(d_labels, np.uint32, labelling, f"{tier} labels, {conn}", boxes, whole)
            g.select(d_labels, k, np.ones(k + 1, dtype=np.uint8), d_out)                     # the whole map: no label anywhere else
            g.same_mask(d_out, s.points, f"{tier} select every label, {conn}")
        d_table, t = g.table(d_labels, k, d_vox)
        want_t = s.table(labelling, k, s.points)
        same_table(t, want_t, f"{tier} table")
        assert int(want_t["first"].max()) > g.n - (1 << 23) and int(want_t["voxels"].sum()) == len(s.points)
        for min_voxels, largest_k in ((126, 0), (0, 2), (125, 0)):
            kept = lr.kept_labels(want_t["voxels"], min_voxels, largest_k)
            assert g.by_size(d_labels, k, d_table, min_voxels, largest_k, d_out) == len(kept)
            g.same_mask(d_out, [p for p, lab in labelling.items() if lab in kept], f"{tier} by size {min_voxels} / {largest_k}")


@tiers
def test_large_distance_ball_and_max(hip_dev, tier):
    """The maps to the nearest unset and set voxel, distance_select, ball open, distance_max.  Device memory: one map and two masks of the
    test, and the three maps and the mask that svr_region_ball allocates -- 16.4 n bytes: 8.2 GiB at L1, 32.8 GiB at L2."""
    shape = LARGE[tier]
    s, whole = beacons(shape), tier == "L1"
    m = ones(s)
    nz, ny, nx = shape
    with Vol(hip_dev, shape) as g:
        d_map, d_mask, d_out = g.reserve(4 * g.n, 4 * g.words, 4 * g.words, headroom=12 * g.n + 4 * g.words)
        g.write_mask(d_mask, s.points)
        unset = m.apply(4, lambda c: np.where(c > 0, dr.distance_map(c > 0, (1, 1, 1), dr.TO_UNSET), 0))
        assert sorted(unset) == sorted(s.points)
        g.distance(d_mask, abi.DIST_TO_UNSET, d_map)
        g.same_points(d_map, np.uint32, unset, f"{tier} distance to unset", m.cutouts(4), whole)
        g.distance_select(d_map, 1, dr.LIMIT, d_out)                                         # the whole map: 0 off the points
        g.same_mask(d_out, s.points, f"{tier} select d2 >= 1")
        top = max(unset.values())
        assert g.dmax(d_map) == (top, min(s.index(p) for p, v in unset.items() if v == top), rr.OK)
        # to the nearest set voxel: a value everywhere; single voxels, and the selection of the near ones over the whole map
        g.distance(d_mask, abi.DIST_TO_SET, d_map)
        rng = np.random.default_rng(83)
        at = np.unique(np.concatenate([rng.integers(0, g.n, size=192), [0, g.n - 1], [i + d for i in sr.plane_crossings(shape) for d in (-1, 0)]]))
        sites = np.array(sorted(s.points), dtype=np.int64)
        z, y, x = at // (ny * nx), (at // nx) % ny, at % nx
        want = ((z[:, None] - sites[None, :, 0]) ** 2 + (y[:, None] - sites[None, :, 1]) ** 2 + (x[:, None] - sites[None, :, 2]) ** 2).min(axis=1)
        got = np.array([int(g.peek(d_map, np.uint32, i, 1)[0]) for i in at.tolist()])
        assert np.array_equal(got, want), f"{tier} distance to set at voxels {at[got != want][:4].tolist()}: {got[got != want][:4].tolist()}"
        g.distance_select(d_map, 0, 9, d_out)
        g.same_mask(d_out, m.apply(5, lambda c: dr.dilate(c > 0, 9)), f"{tier} select d2 <= 9")
        g.ball(d_mask, abi.MORPH_OPEN, 1, d_out)
        g.same_mask(d_out, m.apply(4, lambda c: dr.ball(c > 0, dr.OPEN, 1)), f"{tier} ball open")
        # the maximum of a map the test writes: at the last voxel alone, then also before it -- the lower index wins
        g.fill(d_map, 0, 4 * g.n)
        g.poke(d_map, np.uint32, g.n - 1, [5])
        assert g.dmax(d_map) == (5, g.n - 1, rr.OK)
        g.poke(d_map, np.uint32, sr.plane_crossings(shape)[-1], [5])
        assert g.dmax(d_map) == (5, sr.plane_crossings(shape)[-1], rr.OK)
        assert g.dmax(d_map, d_mask) == (5, g.n - 1, rr.OK)                                 # (the plane voxel itself is off the beacons)


@tiers
def test_large_median_and_smooth(hip_dev, tier):
    """rank median 6 and smooth radius 1 on every axis.  Device memory: two u16 volumes, a mask and the temporary of the smoothing
    passes -- 6.1 n bytes: 3.1 GiB at L1, 12.3 GiB at L2."""
    shape = LARGE[tier]
    s, whole = beacons(shape), tier == "L1"
    boxes = s.cutouts(3)
    with Vol(hip_dev, shape) as g:
        d_vox, d_out, m_tmp = g.reserve(2 * g.n, 2 * g.n, 4 * g.words, headroom=2 * g.n)
        g.write_volume(d_vox, s)
        for name, call, fn in (("median 6", lambda: g.rank(d_vox, abi.FILTER_MEDIAN, 6, d_out), lambda c: fr.rank(c, fr.MEDIAN, 6)),
                               ("smooth 1 1 1", lambda: g.smooth(d_vox, (1, 1, 1), d_out), lambda c: fr.smooth(c, (1, 1, 1)))):
            want = s.apply(3, fn)
            assert len(want) > 12 * 27
            g.fill(d_out, PATTERN, 2 * g.n)
            call()
            g.threshold(d_out, 1, 65535, m_tmp)                                              # the whole output: nothing else is non-zero
            g.same_mask(m_tmp, want, f"{tier} {name}, non-zero voxels")
            g.same_points(d_out, np.uint16, want, f"{tier} {name}", boxes, whole)


@tiers
def test_large_crop_and_paste(hip_dev, tier):
    """Crops of the volume, the label map and the mask around the beacon on the plane where the voxel index passes 2^30 (2^28 at L1), and a
    mask pasted back across that plane.  Device memory: a u16 volume, a uint32 map and a mask -- 6.1 n bytes: 3.1 GiB at L1, 12.3 GiB at L2."""
    shape = LARGE[tier]
    s = beacons(shape)
    nz, ny, nx = shape
    plane = (1 << 30 if tier == "L2" else 1 << 28) // (ny * nx)
    z0, y0, x0 = next(o for o in sr.beacon_origins(shape)[8:] if o[0] == plane - 2)
    lo, counts = (x0 - 40, y0 - 30, plane - 6), (121, 90, 13)                                # x, y, z
    box = ((lo[2], lo[1], lo[0]), (lo[2] + counts[2], lo[1] + counts[1], lo[0] + counts[0]))
    labelling, _ = s.labels(6)
    marks = sr.Sparse(shape, {p: 0x80000000 + lab for p, lab in labelling.items()})
    with Vol(hip_dev, shape) as g:
        d_vox, d_labels, d_mask = g.reserve(2 * g.n, 4 * g.n, 4 * g.words, headroom=64 * MIB)
        g.write_volume(d_vox, s)
        g.write_map(d_labels, marks.points)
        g.write_mask(d_mask, s.points)
        want = s.cut(box)
        assert want[:6].any() and want[6:].any() and want.shape == counts[::-1]             # the beacon straddles the plane inside the box
        same_array(g.crop(g.lib.svr_volume_resample, d_vox, lo, counts, np.uint16, True), want, f"{tier} volume crop")
        same_array(g.crop(g.lib.svr_region_label_resample, d_labels, lo, counts, np.uint32), marks.cut(box, np.uint32), f"{tier} label crop")
        grid = host.resample_grid(tuple((o << 16, 65536, c) for o, c in zip(lo, counts)))
        sub_words = host.region_mask_words(want.shape)
        d_sub = g.raw(4 * sub_words)
        g.ok(g.lib.svr_region_resample(C.c_void_p(d_mask), g.dims3, C.byref(grid), C.c_void_p(d_sub)))
        g.dev.synchronize()
        same_words(hip_dev.to_host(d_sub, (sub_words,), np.uint32), want > 0, f"{tier} mask crop")
        # paste a random mask across the plane
        sub = np.random.default_rng(84).random((13, 40, 70)) < 0.5
        off = (x0 - 10, y0 - 5, plane - 6)
        d_sub = g.put(sr.garbage_padded(sub, 85))
        g.ok(g.lib.svr_region_paste(C.c_void_p(d_sub), (C.c_int32 * 3)(70, 40, 13), C.c_void_p(d_mask), g.dims3, (C.c_int32 * 3)(*off), abi.PASTE_REPLACE))
        g.dev.synchronize()
        want = {p for p in s.points if not (off[2] <= p[0] < off[2] + 13 and off[1] <= p[1] < off[1] + 40 and off[0] <= p[2] < off[0] + 70)}
        want |= {(int(z) + off[2], int(y) + off[1], int(x) + off[0]) for z, y, x in np.argwhere(sub)}
        assert any(p[0] < plane for p in want) and len(want) > len(s.points) - 125 + 1000
        g.same_mask(d_mask, want, f"{tier} paste")


def test_large_geodesic_and_growcut_along_a_rod(hip_dev):
    """L1 only: svr_region_geodesic and svr_region_growcut on a one-voxel rod along z through the plane where the voxel index passes 2^28
    up to the last voxel, a marker at either end.  The costs are those of the same column on its own: 3 a step, or 1 plus the contrast.
    Device memory: three uint32 maps, a u16 volume, a mask and the call's 8-byte keys -- 22 n bytes: 11 GiB."""
    from tests import geodesic_ref as gr
    from tests import growcut_ref as gc

    shape = sr.L1
    rod = sr.Sparse(shape, sr.rod_points(shape))
    cells = sorted(rod.points)
    markers = {cells[0]: 7, cells[-1]: 3}
    n_rod = len(cells)
    assert rod.index(cells[5]) >= 1 << 28 > rod.index(cells[4]) and rod.index(cells[-1]) == (1 << 29) - 1
    col_labels = np.zeros((n_rod, 1, 1), dtype=np.uint32)
    col_labels[0], col_labels[-1] = 7, 3
    col_vox = np.array([rod.points[p] for p in cells], dtype=np.uint16).reshape(n_rod, 1, 1)
    full = np.ones((n_rod, 1, 1), dtype=bool)
    want_d, want_z = gr.geodesic(col_labels, full, gr.CHAMFER)
    steps = np.minimum(np.arange(n_rod), n_rod - 1 - np.arange(n_rod))
    assert np.array_equal(want_d.reshape(-1), 3 * steps) and n_rod % 2 == 1 and want_z[n_rod // 2, 0, 0] == 3      # 3 a step; the tie goes to 3
    weights = gc.default_weights(6)
    want_c, want_cz = gc.growcut(col_vox, col_labels, full, weights, 1, 0)
    diffs = np.abs(np.diff(col_vox.reshape(-1).astype(np.int64)))
    assert np.array_equal(want_c.reshape(-1)[:50], np.concatenate(([0], np.cumsum(1 + diffs)))[:50])                # 1 plus the contrast a step
    idx = np.array([rod.index(p) for p in cells], dtype=np.int64)
    with Vol(hip_dev, shape) as g:
        d_labels, d_dist, d_zones, d_vox, d_dom = g.reserve(4 * g.n, 4 * g.n, 4 * g.n, 2 * g.n, 4 * g.words, headroom=8 * g.n + 64 * MIB)
        g.write_map(d_labels, markers)
        g.write_volume(d_vox, rod)
        g.write_mask(d_dom, rod.points)
        sweeps = g.geodesic(d_labels, d_dom, gr.CHAMFER, d_dist, d_zones)
        assert 1 <= sweeps <= hip_dev.lib.svr_region_geodesic_default_max_sweeps(*g.dims)
        g.same_sparse(d_dist, np.uint32, g.n, (idx, want_d.reshape(-1)), "geodesic dist", background=gr.NONE)
        g.same_sparse(d_zones, np.uint32, g.n, (idx, want_z.reshape(-1)), "geodesic zones")
        g.fill(d_dist, PATTERN, 4 * g.n)
        g.fill(d_zones, PATTERN, 4 * g.n)
        info = g.growcut(d_vox, d_labels, d_dom, weights, 1, 0, d_dist, d_zones)
        assert (info.unreached, info.saturated) == (0, 0) and info.sweeps >= 1
        g.same_sparse(d_dist, np.uint32, g.n, (idx, want_c.reshape(-1)), "growcut cost", background=gc.NONE)
        g.same_sparse(d_zones, np.uint32, g.n, (idx, want_cz.reshape(-1)), "growcut zones")


@pytest.mark.parametrize("relax", [0, 2])
def test_large_mesh_of_the_beacons(hip_dev, relax):
    """L1 only: svr_mesh_region of the beacons, index for index.  Device memory: the mask, the mesh and the call's words and scans over
    the padded points -- below 1 GiB."""
    shape = sr.L1
    s = beacons(shape)
    want = s.mesh(relax)
    assert all(256 * n < t < 256 * (n + 1) for t, n in zip(want[2]["bbox_max"], shape[::-1])) and max(want[2]["bbox_min"]) < 256
    with Vol(hip_dev, shape) as g:
        d_mask, = g.reserve(4 * g.words, headroom=g.n)
        g.write_mask(d_mask, s.points)
        same_mesh(hip_dev.mesh_region(d_mask, relax, shape=shape), want, f"L1 beacons relax {relax}")
