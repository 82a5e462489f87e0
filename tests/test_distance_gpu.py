"""svr_region_distance / _distance_select / _ball / _distance_max / _distance_volume on the GPU: every map, mask -- as uint32 words, padding
included -- and volume is EQUAL to the test-side reference (tests/distance_ref.py: the literal per-axis min-plus in int64).  Output
buffers are pre-filled with a pattern.  The fixtures and the conditions they meet are those of tests/test_distance_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import distance_ref as dr
from tests import morph_ref as mr
from tests import region_ref as rr
from tests.test_region_cpu import BONE

pytestmark = pytest.mark.gpu


class Dist:
    """Raw calls on buffers the test owns."""

    def __init__(self, dev, shape):
        self.dev, self.lib, self.shape = dev, dev.lib, tuple(shape)
        self.dims = (shape[2], shape[1], shape[0])
        self.words = host.region_mask_words(shape)
        self.n = int(np.prod(shape))
        self.bufs = []

    def raw(self, nbytes, prefill=0xA5):
        p = self.dev.malloc(max(nbytes, 4))
        self.bufs.append(p)
        self.dev.check(self.lib.svr_memset_device(C.c_void_p(p), prefill, max(nbytes, 4)))       # the calls overwrite whatever is there
        return p

    def put(self, arr):
        a = np.ascontiguousarray(arr)
        p = self.raw(a.nbytes)
        self.dev.to_device(p, a)
        return p

    def ok(self, rc):
        msg = self.lib.svr_last_error().decode()
        self.lib.svr_clear_error()
        assert rc == 0, msg

    @staticmethod
    def w(weights):
        return None if weights is None else (C.c_uint32 * 3)(*weights)

    def distance(self, mask_ptr, weights, target, out):
        self.ok(self.lib.svr_region_distance(C.c_void_p(mask_ptr), *self.dims, self.w(weights), target, C.c_void_p(out)))
        return self.dev.to_host(out, self.shape, np.uint32)

    def ball(self, mask_ptr, op, weights, r2, out):
        self.ok(self.lib.svr_region_ball(C.c_void_p(mask_ptr), *self.dims, op, self.w(weights), r2, C.c_void_p(out)))
        self.dev.synchronize()
        return self.dev.to_host(out, (self.words,), np.uint32)

    def morph(self, mask_ptr, op, element, out):
        self.ok(self.lib.svr_region_morph(C.c_void_p(mask_ptr), *self.dims, op, element, 1, C.c_void_p(out)))
        self.dev.synchronize()
        return self.dev.to_host(out, (self.words,), np.uint32)

    def select(self, map_ptr, lo2, hi2, out):
        self.ok(self.lib.svr_region_distance_select(C.c_void_p(map_ptr), *self.dims, lo2, hi2, C.c_void_p(out)))
        self.dev.synchronize()
        return self.dev.to_host(out, (self.words,), np.uint32)

    def dmax(self, map_ptr, mask_ptr=None):
        m, first, status = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF), C.c_int32(-1)
        self.ok(self.lib.svr_region_distance_max(C.c_void_p(map_ptr), None if mask_ptr is None else C.c_void_p(mask_ptr), *self.dims, C.byref(m),
                                                 C.byref(first), C.byref(status)))
        return int(m.value), int(first.value), int(status.value)

    def volume(self, map_ptr, scale, out):
        self.ok(self.lib.svr_region_distance_volume(C.c_void_p(map_ptr), *self.dims, scale, C.c_void_p(out)))
        self.dev.synchronize()
        return self.dev.to_host(out, self.shape, np.uint16)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.dev.free(p)
        self.bufs = []


def same_map(got, want, what):
    if not np.array_equal(got, want):
        diff = got != want
        at = tuple(np.argwhere(diff)[0].tolist())
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} entries differ; first (z, y, x) {at}: {int(got[at])} for {int(want[at])}")


def same_mask(words, want_mask, what):
    want = rr.pack(want_mask)
    if not np.array_equal(words, want):
        diff = rr.unpack(words ^ want, want_mask.shape)
        raise AssertionError(f"{what}: {int(diff.sum())} voxels differ; first (z, y, x) {np.argwhere(diff)[:1].tolist()}; "
                             f"padding differs: {not np.array_equal(rr.pack(rr.unpack(words, want_mask.shape)), words)}")


def trivial_map(full, target, shape):
    """empty / full masks: every entry 0 or SVR_DIST_NONE."""
    none = (target == dr.TO_SET) != full
    return np.full(shape, dr.NONE if none else 0, dtype=np.uint32)


# ------------------------------------------------------------------------------------------------ the map
@pytest.mark.parametrize("shape", rr.EDGE_SHAPES, ids=str)
def test_distance_shapes(hip_dev, shape):
    finite = 0
    with Dist(hip_dev, shape) as g:
        out = g.raw(4 * g.n)
        masks = [(f"density {d}", dr.random_mask(shape, d, 40 + k)) for k, d in enumerate(dr.DENSITIES)]
        for name, m in masks:
            src = g.put(rr.pack(m))
            for w in dr.WEIGHTS:
                for target in dr.TARGETS:
                    want = dr.cached_map(name, m, w, target)
                    finite += int((want != dr.NONE).any())
                    same_map(g.distance(src, w, target, out), want, (shape, name, w, target))
        for full in (False, True):
            src = g.put(rr.pack(np.full(shape, full)))
            for w in dr.WEIGHTS:
                for target in dr.TARGETS:
                    same_map(g.distance(src, w, target, out), trivial_map(full, target, shape), (shape, "full" if full else "empty", w, target))
        for c in dr.corners(shape):
            src = g.put(rr.pack(dr.single(shape, c)))
            for w in dr.WEIGHTS:
                for target in dr.TARGETS:
                    same_map(g.distance(src, w, target, out), dr.single_map(shape, c, w, target), (shape, "corner", c, w, target))
    assert finite


def test_distance_null_weights_are_ones(hip_dev):
    shape = rr.EDGE_SHAPES[0]
    m = dr.random_mask(shape, 0.3, 41)
    with Dist(hip_dev, shape) as g:
        same_map(g.distance(g.put(rr.pack(m)), None, dr.TO_SET, g.raw(4 * g.n)), dr.cached_map("density 0.3", m, (1, 1, 1), dr.TO_SET), "NULL weights")
    same_map(hip_dev.region_distance(m, weights=(1, 4, 9), target=abi.DIST_TO_UNSET), dr.cached_map("density 0.3", m, (1, 4, 9), dr.TO_UNSET), "Device.region_distance")


def test_distance_rows_and_slices_without_a_target(hip_dev):
    for name, m in dr.sparse_cases():
        with Dist(hip_dev, m.shape) as g:
            src, out = g.put(rr.pack(m)), g.raw(4 * g.n)
            for w in dr.WEIGHTS:
                assert dr.fits(w, m.shape)
                for target in dr.TARGETS:
                    same_map(g.distance(src, w, target, out), dr.cached_map(name, m, w, target), (name, w, target))


@pytest.mark.parametrize("shape", dr.LONG_SHAPES + [dr.BLOCK_SHAPE], ids=str)
def test_distance_long_axes_and_the_column_block(hip_dev, shape):
    cases = dr.long_masks(shape) + [("density 0.3", dr.random_mask(shape, 0.3, 9))]
    with Dist(hip_dev, shape) as g:
        out = g.raw(4 * g.n)
        for name, m in cases:
            src = g.put(rr.pack(m))
            for w in dr.WEIGHTS:
                assert dr.fits(w, shape)
                for target in dr.TARGETS:
                    same_map(g.distance(src, w, target, out), dr.cached_map(name, m, w, target), (shape, name, w, target))


def test_distance_deep_envelopes(hip_dev):
    shape = (64, 64, 64)
    m = dr.random_mask(shape, 0.001, 77)
    with Dist(hip_dev, shape) as g:
        src, out = g.put(rr.pack(m)), g.raw(4 * g.n)
        for w in ((1, 1, 1), (49, 49, 225)):
            want = dr.cached_map("sparse64", m, w, dr.TO_SET)
            assert want.max() > 30 * min(w)                                               # the distances are long
            same_map(g.distance(src, w, dr.TO_SET, out), want, ("sparse64", w))
        same_map(g.distance(src, (49, 49, 225), dr.TO_UNSET, out), dr.cached_map("sparse64", m, (49, 49, 225), dr.TO_UNSET), "sparse64 unset")


@pytest.mark.parametrize("nx", [33, 40])
def test_distance_ignores_input_padding(hip_dev, nx):
    shape = (5, 6, nx)
    m = dr.random_mask(shape, 0.1, 3)
    m[:, :, nx - 3:] = True                                                               # set up to the last voxel: the padding would be its nearest background
    m[2] = False
    m[2, :, :5] = True                                                                    # and rows whose last voxels are unset: the padding would be their nearest region
    dirty = mr.dirty_padding(rr.pack(m), shape)
    assert not np.array_equal(dirty, rr.pack(m))
    with Dist(hip_dev, shape) as g:
        src, out, bits = g.put(dirty), g.raw(4 * g.n), g.raw(4 * g.words)
        for target in dr.TARGETS:
            want = dr.cached_map(f"padding{nx}", m, (1, 4, 9), target)
            for _ in range(2):                                                            # and the same again
                same_map(g.distance(src, (1, 4, 9), target, out), want, ("padding", nx, target))
        for op in dr.OPS:
            same_mask(g.ball(src, op, (1, 1, 1), 2, bits), dr.ball(m, op, 2), ("padding ball", nx, op))
        same_mask(g.ball(src, dr.DILATE, None, 0, bits), m, "r2 = 0 clears the padding")


# ------------------------------------------------------------------------------------------------ balls
@pytest.mark.parametrize("shape", rr.EDGE_SHAPES, ids=str)
def test_ball_against_reference(hip_dev, shape):
    w = dr.WEIGHTS[rr.EDGE_SHAPES.index(shape) % 2]
    m = dr.random_mask(shape, 0.5, 13)
    to_set, to_unset = dr.cached_map("ball", m, w, dr.TO_SET), dr.cached_map("ball", m, w, dr.TO_UNSET)

    def want(op, r2):
        """dr.ball, with the first half taken from the two maps of `m` that every radius shares."""
        first = dr.dilate_of(to_set, r2) if op in (dr.DILATE, dr.CLOSE) else dr.erode_of(to_unset, r2)
        if op in (dr.DILATE, dr.ERODE):
            return first
        return dr.cached(("ball", shape, w, op, r2), lambda: dr.ball(first, dr.DILATE if op == dr.OPEN else dr.ERODE, r2, w))

    assert np.array_equal(want(dr.OPEN, 2), dr.ball(m, dr.OPEN, 2, w)) and np.array_equal(want(dr.ERODE, 9), dr.ball(m, dr.ERODE, 9, w))
    with Dist(hip_dev, shape) as g:
        src, out = g.put(rr.pack(m)), g.raw(4 * g.words)
        for r2 in dr.BALL_R2 + (dr.beyond(w, shape),):
            for op in dr.OPS:
                same_mask(g.ball(src, op, w, r2, out), want(op, r2), (shape, w, op, r2))
    assert np.array_equal(hip_dev.region_ball(m, abi.MORPH_CLOSE, 9, weights=w), want(dr.CLOSE, 9))


@pytest.mark.parametrize("shape", [rr.EDGE_SHAPES[0], rr.EDGE_SHAPES[5], rr.EDGE_SHAPES[12], mr.TWO_BALL_SHAPE], ids=str)
def test_ball_of_r2_1_2_3_is_the_unit_element(hip_dev, shape):
    masks = [mr.two_balls()] if shape == mr.TWO_BALL_SHAPE else [dr.random_mask(shape, d, 21) for d in (0.05, 0.6)]
    with Dist(hip_dev, shape) as g:
        a, b = g.raw(4 * g.words), g.raw(4 * g.words)
        for m in masks:
            src = g.put(rr.pack(m))
            for r2, element in ((1, 6), (2, 18), (3, 26)):
                for op in dr.OPS:
                    assert np.array_equal(g.ball(src, op, None, r2, a), g.morph(src, op, element, b)), (shape, r2, element, op)   # word for word


def test_ball_open_close_properties_and_a_large_radius(hip_dev):
    m = mr.two_balls()
    sub = lambda a, b: not (a & ~b).any()
    for r2 in (5, 16):
        opened, closed = hip_dev.region_ball(m, abi.MORPH_OPEN, r2), hip_dev.region_ball(m, abi.MORPH_CLOSE, r2)
        assert sub(opened, m) and sub(m, closed)
        assert np.array_equal(hip_dev.region_ball(opened, abi.MORPH_OPEN, r2), opened)
        assert np.array_equal(hip_dev.region_ball(closed, abi.MORPH_CLOSE, r2), closed)
    assert mr.second_ball(hip_dev.region_ball(m, abi.MORPH_OPEN, 5)) > 0 and not hip_dev.region_ball(m, abi.MORPH_OPEN, 5)[9, 9, 30:40].any()   # the bridge goes
    # far beyond SVR_MORPH_MAX_RADIUS: the cost does not depend on the radius
    shape, r2 = (300, 8, 8), 100 * 100
    assert 100 > abi.MORPH_MAX_RADIUS
    s = np.zeros(shape, dtype=bool)
    s[0], s[299, 3, 3] = True, True
    with Dist(hip_dev, shape) as g:
        src, out = g.put(rr.pack(s)), g.raw(4 * g.words)
        for op in dr.OPS:
            same_mask(g.ball(src, op, None, r2, out), dr.cached(("ball-far", op), lambda: dr.ball(s, op, r2)), ("r2 = 100^2", op))
    assert dr.ball(s, dr.DILATE, r2)[100].all() and not dr.ball(s, dr.DILATE, r2)[101, 7, 7]


# ------------------------------------------------------------------------------------------------ select, max, volume
def test_select_margins_shells_and_none(hip_dev):
    shape = rr.EDGE_SHAPES[9]
    m = dr.random_mask(shape, 0.02, 5)
    dmap = dr.cached_map("select", m, (1, 4, 9), dr.TO_SET)
    with Dist(hip_dev, shape) as g:
        src, out = g.put(dmap), g.raw(4 * g.words)
        for lo2, hi2 in ((0, 0), (0, 9), (0, 50), (5, 20), (10, 10), (1, dr.LIMIT), (0, dr.NONE)):
            want = dr.select(dmap, lo2, hi2)
            same_mask(g.select(src, lo2, hi2, out), want, (lo2, hi2))
            assert np.array_equal(hip_dev.region_distance_select(dmap, lo2, hi2), want)
        assert np.array_equal(dr.select(dmap, 0, 0), m) and 0 < dr.select(dmap, 5, 20).sum() < m.size
        none = g.put(np.full(shape, dr.NONE, dtype=np.uint32))
        same_mask(g.select(none, 0, dr.NONE, out), np.ones(shape, dtype=bool), "NONE with hi2 = 0xFFFFFFFF")
        same_mask(g.select(none, 0, dr.LIMIT, out), np.zeros(shape, dtype=bool), "NONE with hi2 = 0xFFFFFFFE")
        same_mask(g.select(none, dr.NONE, dr.NONE, out), np.ones(shape, dtype=bool), "NONE alone")


def test_distance_max(hip_dev):
    tie = dr.tie_mask()
    with Dist(hip_dev, dr.TIE_SHAPE) as g:
        src, out = g.put(rr.pack(tie)), g.raw(4 * g.n)
        dmap = g.distance(src, None, dr.TO_UNSET, out)
        assert g.dmax(out, src) == g.dmax(out) == (dr.TIE_D2, dr.TIE_INDEX, rr.OK) == dr.dmax(dmap, tie)
        second = tie.copy()
        second[2, 2, 2] = False                                                           # a mask that excludes the first of the two: the other one
        assert g.dmax(out, g.put(rr.pack(second))) == dr.dmax(dmap, second) == (dr.TIE_D2, (2 * 6 + 2) * 11 + 7, rr.OK)
        assert g.dmax(out, g.put(rr.pack(np.zeros(dr.TIE_SHAPE, dtype=bool)))) == (0, 0, rr.EMPTY)
        none = g.put(np.full(dr.TIE_SHAPE, dr.NONE, dtype=np.uint32))
        assert g.dmax(none) == g.dmax(none, src) == (0, 0, rr.EMPTY)
    shape = rr.EDGE_SHAPES[13]                                                            # more than one block, words of padding-free rows
    m = dr.random_mask(shape, 0.02, 8)
    dmap = dr.cached_map("max", m, (1, 4, 9), dr.TO_SET)
    region = dr.random_mask(shape, 0.5, 9)
    top = dr.dmax(dmap)
    region.reshape(-1)[np.flatnonzero(dmap.reshape(-1) == top[0])] = False                # the mask excludes the global maximum
    assert dr.dmax(dmap, region)[0] < top[0]
    dirty = mr.dirty_padding(rr.pack(region), shape)
    with Dist(hip_dev, shape) as g:
        src = g.put(dmap)
        assert g.dmax(src) == top and g.dmax(src, g.put(dirty)) == dr.dmax(dmap, region)
    assert hip_dev.region_distance_max(dmap, region) == dr.dmax(dmap, region) and hip_dev.region_distance_max(dmap) == top
    shape = (3, 5, 33)                                                                    # padding bits of the mask are not voxels
    dmap = np.arange(np.prod(shape), dtype=np.uint32).reshape(shape)
    with Dist(hip_dev, shape) as g:
        assert g.dmax(g.put(dmap), g.put(mr.dirty_padding(rr.pack(np.zeros(shape, dtype=bool)), shape))) == (0, 0, rr.EMPTY)


def test_distance_volume(hip_dev):
    shape = rr.EDGE_SHAPES[0]
    m = dr.random_mask(shape, 0.02, 5)
    dmap = dr.cached_map("volume", m, (49, 49, 225), dr.TO_SET).copy()
    flat = dmap.reshape(-1)
    flat[:8] = [dr.NONE, dr.LIMIT, 65535 * 65535, 65535 * 65535 - 1, 65534 * 65534, 0, 1, 2]
    with Dist(hip_dev, shape) as g:
        src, out = g.put(dmap), g.raw(2 * g.n)
        for scale in (1, 16, 65535):
            want = dr.cached(("volume", scale), lambda: dr.to_volume(dmap, scale))
            got = g.volume(src, scale, out)
            assert np.array_equal(got, want), (scale, np.argwhere(got != want)[:1].tolist())
        assert dr.to_volume(dmap, 1).reshape(-1)[:5].tolist() == [65535, 65535, 65535, 65534, 65534]
        assert (dr.to_volume(dmap, 16) == 65535).sum() < dmap.size and (dr.to_volume(dmap, 65535).reshape(-1)[5:8] == [0, 65535, 65535]).all()
    assert np.array_equal(hip_dev.region_distance_volume(dmap, 16), dr.to_volume(dmap, 16))


# ------------------------------------------------------------------------------------------------ the loop, once
def _raycast(canvas, volume):
    dev = canvas.dev
    dev.check(dev.lib.svr_memset_device(C.c_void_p(canvas.img), 0, canvas.W * canvas.H * 4))
    dev.lib.render_raycasting(C.c_void_p(canvas.img), C.byref(volume), C.byref(canvas.transferFunction), C.byref(canvas.camera),
                              C.c_float(canvas.stepSize))
    dev.check()
    dev.synchronize()
    return canvas.read_img()


def test_threshold_ball_close_measure_show(hip_dev):
    dev, lib = hip_dev, hip_dev.lib
    sc = scenes.make_scene("tiny_head")
    head = sc.vox
    cv = host.Canvas(dev, sc.width, sc.height)
    scenes.apply_to_canvas(sc, cv)
    nz, ny, nx = head.shape
    words = host.region_mask_words(head.shape)
    spacing = (0.7, 0.7, 1.5)
    w, unit = host.distance_weights(spacing, head.shape)
    assert (w, unit) == dr.weights(spacing, head.shape)[:2]
    r2 = int((2.0 / unit) ** 2)                                                           # close by 2 units of the spacing
    d_out, d_mask, d_closed, texs = dev.malloc(head.nbytes), dev.malloc(4 * words), dev.malloc(4 * words), []
    try:
        before = _raycast(cv, cv.deviceVolume)
        window = dev.region_threshold(head, BONE[0], BONE[1], out_ptr=d_mask)
        closed = dev.region_ball(d_mask, abi.MORPH_CLOSE, r2, weights=w, shape=head.shape, out_ptr=d_closed)
        want = dr.ball(window, dr.CLOSE, r2, w)
        assert np.array_equal(closed, want) and window.sum() < want.sum() < want.size
        got, ref = dev.region_stats_of(head, d_closed).as_dict(), rr.stats(head, want)
        for key in rr.STAT_INTS:
            assert got[key] == ref[key], f"{key} is {got[key]}, reference {ref[key]}"
        assert dev.region_apply(head, d_closed, abi.REGION_KEEP, 0, out_ptr=d_out) == d_out
        shown = []
        for voxels, on_device in ((C.c_void_p(d_out), 1), (np.ascontiguousarray(rr.apply(head, want, rr.KEEP, 0)), 0)):
            src = voxels if on_device else voxels.ctypes.data_as(C.c_void_p)
            tex = lib.svr_create_volume_texture(src, nx, ny, nz, on_device, abi.LAYOUT_AUTO)
            dev.check()
            texs.append(tex)
            vol = abi.cudaVolume.from_buffer_copy(cv.deviceVolume)
            vol.tex = tex
            shown.append(_raycast(cv, vol))
        assert np.array_equal(shown[0], shown[1])
        assert not np.array_equal(shown[0], before) and shown[0].any()
        assert np.array_equal(_raycast(cv, cv.deviceVolume), before)                      # the distance calls left the renderers alone
        assert dev.region_distance_last_ms() >= 0.0 and all(t >= 0.0 for t in dev.region_distance_pass_ms())
    finally:
        for t in texs:
            lib.svr_destroy_texture(t)
        for p in (d_out, d_mask, d_closed):
            dev.free(p)
        cv.close()
