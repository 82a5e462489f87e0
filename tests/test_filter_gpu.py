"""svr_volume_rank / svr_volume_smooth on the GPU: every result is EQUAL, as a u16 array, to the test-side reference
(tests/filter_ref.py: pad with the edge, stack the window, sort, take the rank; per axis an int64 binomial sum, one rounding).  Output
buffers are pre-filled with a pattern and carry a guard tail that must come back untouched.  The shapes are those at which such kernels
break: single voxels, lines and slabs thinner than any halo (and than radius 8), one more than a 128 x 8 x 8 tile on every axis with an
odd nx -- rows then start at odd u16 offsets -- and a thin box that crosses several tiles and x segments."""
import ctypes as C

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import filter_ref as fr

pytestmark = pytest.mark.gpu

# (nz, ny, nx)
SMALL = [(1, 1, 1), (2, 2, 2), (1, 1, 40), (3, 1, 33)]
TILED = [(10, 9, 131), (5, 17, 63), (2, 3, 515)]
HEAD = (48, 48, 48)
RADII = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (2, 3, 1), (8, 8, 8)]
GUARD = 64                                               # u16 past the end of `out`
PATTERN = 0xA5A5


def volumes(shape):
    """(name, volume) of the value cases: full-range random, all-65535, all-0, only {0, 65535}."""
    return [("random", fr.random_volume(shape, 31)), ("all 65535", np.full(shape, 65535, dtype=np.uint16)), ("all 0", np.zeros(shape, dtype=np.uint16)),
            ("extremes", fr.extremes_volume(shape, 32))]


class Filt:
    """Raw calls on buffers the test owns."""

    def __init__(self, dev, shape):
        self.dev, self.lib, self.shape = dev, dev.lib, tuple(shape)
        self.dims = (shape[2], shape[1], shape[0])
        self.n = int(np.prod(shape))
        self.bufs = []

    def raw(self, nbytes, prefill=0xA5):
        p = self.dev.malloc(max(nbytes, 4))
        self.bufs.append(p)
        self.dev.check(self.lib.svr_memset_device(C.c_void_p(p), prefill, max(nbytes, 4)))
        return p

    def put(self, arr):
        a = np.ascontiguousarray(arr)
        p = self.raw(a.nbytes)
        self.dev.to_device(p, a)
        return p

    def out(self):
        """A pattern-filled output buffer with its guard tail."""
        return self.raw(2 * (self.n + GUARD))

    def ok(self, rc):
        msg = self.lib.svr_last_error().decode()
        self.lib.svr_clear_error()
        assert rc == 0, msg

    def fetch(self, out, what):
        self.dev.synchronize()
        got = self.dev.to_host(out, (self.n + GUARD,), np.uint16)
        assert (got[self.n:] == PATTERN).all(), f"{what}: memory past the end of out was written"
        return got[:self.n].reshape(self.shape)

    def src(self, vox):
        """(pointer, src_is_device) of a device pointer (int) or a host array."""
        if isinstance(vox, np.ndarray):
            assert vox.dtype == np.uint16 and vox.flags.c_contiguous
            return vox.ctypes.data_as(C.c_void_p), 0
        return C.c_void_p(vox), 1

    def rank(self, vox, op, element, iterations, out, what=""):
        p, on_dev = self.src(vox)
        self.ok(self.lib.svr_volume_rank(p, *self.dims, on_dev, op, element, iterations, C.c_void_p(out)))
        return self.fetch(out, what)

    def smooth(self, vox, radii, out, what=""):
        p, on_dev = self.src(vox)
        self.ok(self.lib.svr_volume_smooth(p, *self.dims, on_dev, (C.c_uint32 * 3)(*radii), C.c_void_p(out)))
        return self.fetch(out, what)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.dev.free(p)
        self.bufs = []


def same(got, want, what):
    assert got.dtype == want.dtype == np.uint16 and got.shape == want.shape
    if not np.array_equal(got, want):
        diff = got != want
        at = tuple(np.argwhere(diff)[0].tolist())
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} voxels differ; first (z, y, x) {at}: {int(got[at])} for {int(want[at])}")


# ------------------------------------------------------------------------------------------------ rank
@pytest.mark.parametrize("shape", SMALL + TILED, ids=str)
def test_rank_every_op_and_element(hip_dev, shape):
    with Filt(hip_dev, shape) as f:
        out = f.out()
        for name, vol in volumes(shape):
            d_vol = f.put(vol)
            for op in fr.OPS:
                for element in fr.ELEMENTS:
                    what = f"{shape} {name} op {op} element {element}"
                    same(f.rank(d_vol, op, element, 1, out, what), fr.rank(vol, op, element), what)


@pytest.mark.parametrize("shape", SMALL + TILED, ids=str)
def test_rank_iterations(hip_dev, shape):
    """iterations = 2 and 5 equal the reference's, and n calls of one iteration equal one call of n."""
    vol = fr.random_volume(shape, 33)
    with Filt(hip_dev, shape) as f:
        d_vol, a, b = f.put(vol), f.out(), f.out()
        for op, element in ((fr.MEDIAN, 26), (fr.MEDIAN, 6), (fr.MIN, 18), (fr.MAX, 6)):
            for n in (2, 5):
                what = f"{shape} op {op} element {element} x {n}"
                got = f.rank(d_vol, op, element, n, a, what)
                same(got, fr.rank(vol, op, element, n), what)
                src, dst = d_vol, b
                for _ in range(n):                                                       # one at a time, ping-pong between two buffers
                    step = f.rank(src, op, element, 1, dst, what)
                    src, dst = dst, (a if dst == b else b)
                same(step, got, what + " (one at a time)")


def test_rank_on_the_heads(hip_dev):
    clean, salted = fr.heads()
    with Filt(hip_dev, HEAD) as f:
        out = f.out()
        for name, vol in (("clean", clean), ("salted", salted)):
            d_vol = f.put(vol)
            for op in fr.OPS:
                for element in fr.ELEMENTS:
                    what = f"head {name} op {op} element {element}"
                    same(f.rank(d_vol, op, element, 1, out, what), fr.cached_rank(name, op, element), what)
        same(f.rank(d_vol, fr.MEDIAN, 26, 5, out, "salted median 26 x 5"), fr.cached_rank("salted", fr.MEDIAN, 26, 5), "salted median 26 x 5")


@pytest.mark.parametrize("shape", SMALL + TILED[:1], ids=str)
def test_rank_from_a_host_source(hip_dev, shape):
    vol = fr.random_volume(shape, 34)
    with Filt(hip_dev, shape) as f:
        out = f.out()
        for op, element, n in ((fr.MEDIAN, 18, 1), (fr.MEDIAN, 26, 2), (fr.MIN, 6, 5), (fr.MAX, 26, 1)):
            what = f"{shape} host op {op} element {element} x {n}"
            same(f.rank(vol, op, element, n, out, what), fr.rank(vol, op, element, n), what)
    # and through the Python layer, which owns the output
    same(hip_dev.volume_median(vol, 26, 2), fr.rank(vol, fr.MEDIAN, 26, 2), f"{shape} volume_median")
    same(hip_dev.volume_rank(vol, abi.FILTER_MAX, 18), fr.rank(vol, fr.MAX, 18), f"{shape} volume_rank")


def test_the_source_is_not_written(hip_dev):
    shape = TILED[0]
    vol = fr.random_volume(shape, 35)
    with Filt(hip_dev, shape) as f:
        d_vol, out = f.put(vol), f.out()
        f.rank(d_vol, fr.MEDIAN, 26, 4, out)
        f.smooth(d_vol, (2, 3, 1), out)
        assert np.array_equal(hip_dev.to_host(d_vol, shape, np.uint16), vol)


# ------------------------------------------------------------------------------------------------ smoothing
@pytest.mark.parametrize("shape", SMALL + TILED, ids=str)
def test_smooth_every_radius(hip_dev, shape):
    with Filt(hip_dev, shape) as f:
        out = f.out()
        for name, vol in volumes(shape):
            d_vol = f.put(vol)
            for radii in RADII:
                what = f"{shape} {name} radii {radii}"
                same(f.smooth(d_vol, radii, out, what), fr.smooth(vol, radii), what)


def test_smooth_every_single_radius(hip_dev):
    """Radii 1 .. 8 along each axis alone: one instantiation of the kernel each."""
    shape = (19, 18, 37)
    vol = fr.random_volume(shape, 36)
    with Filt(hip_dev, shape) as f:
        d_vol, out = f.put(vol), f.out()
        for r in range(1, 9):
            for axis in range(3):
                radii = tuple(r if a == axis else 0 for a in range(3))
                same(f.smooth(d_vol, radii, out, str(radii)), fr.smooth(vol, radii), f"{shape} radii {radii}")


def test_smooth_on_the_heads(hip_dev):
    with Filt(hip_dev, HEAD) as f:
        out = f.out()
        for name, vol in zip(("clean", "salted"), fr.heads()):
            d_vol = f.put(vol)
            for radii in RADII:
                same(f.smooth(d_vol, radii, out, f"head {name} {radii}"), fr.smooth(vol, radii), f"head {name} radii {radii}")


@pytest.mark.parametrize("shape", SMALL + TILED[:1], ids=str)
def test_smooth_from_a_host_source_and_the_copy(hip_dev, shape):
    vol = fr.random_volume(shape, 37)
    with Filt(hip_dev, shape) as f:
        d_vol, out = f.put(vol), f.out()
        for radii in ((1, 0, 0), (2, 3, 1), (8, 8, 8)):
            same(f.smooth(vol, radii, out, f"host {radii}"), fr.smooth(vol, radii), f"{shape} host radii {radii}")
        same(f.smooth(d_vol, (0, 0, 0), out, "copy"), vol, f"{shape} the (0, 0, 0) copy of a device source")
        out2 = f.out()
        same(f.smooth(vol, (0, 0, 0), out2, "copy"), vol, f"{shape} the (0, 0, 0) copy of a host source")
    same(hip_dev.volume_smooth(vol, (2, 3, 1)), fr.smooth(vol, (2, 3, 1)), f"{shape} volume_smooth")


def test_out_ptr_keeps_the_result_on_the_device(hip_dev):
    shape = TILED[1]
    vol = fr.random_volume(shape, 38)
    with Filt(hip_dev, shape) as f:
        d_vol, out = f.put(vol), f.out()
        assert hip_dev.volume_median(d_vol, 18, 1, shape=shape, out_ptr=out) == out
        same(f.fetch(out, "out_ptr"), fr.rank(vol, fr.MEDIAN, 18), "volume_median out_ptr")
        assert hip_dev.volume_smooth(d_vol, (1, 1, 1), shape=shape, out_ptr=out) == out
        same(f.fetch(out, "out_ptr"), fr.smooth(vol, (1, 1, 1)), "volume_smooth out_ptr")


# ------------------------------------------------------------------------------------------------ the chain, the timer, the refusal on a live device
def test_median_then_threshold_then_label(hip_dev):
    """The bone window of the salted head has 747 parts; after one median-18 pass on the GPU it has one -- all on the device."""
    _, salted = fr.heads()
    nz, ny, nx = HEAD
    with Filt(hip_dev, HEAD) as f:
        d_vol, d_med = f.put(salted), f.out()
        d_mask, d_labels = f.raw(4 * host.region_mask_words(HEAD)), f.raw(4 * f.n)
        f.rank(d_vol, fr.MEDIAN, 18, 1, d_med)
        counts = []
        for src in (d_vol, d_med):
            f.ok(f.lib.svr_region_threshold(C.c_void_p(src), nx, ny, nz, 1, fr.BONE[0], fr.BONE[1], None, None, C.c_void_p(d_mask)))
            k = C.c_uint32(0)
            f.ok(f.lib.svr_region_label(C.c_void_p(d_mask), nx, ny, nz, 6, C.c_void_p(d_labels), C.byref(k)))
            counts.append(int(k.value))
        assert counts == [747, 1]
        mask = hip_dev.region_threshold(d_med, fr.BONE[0], fr.BONE[1], shape=HEAD)
        assert int(mask.sum()) == 5336 and int((mask ^ fr.window(fr.heads()[0])).sum()) == 270


def test_filter_last_ms(hip_dev):
    vol = fr.random_volume(TILED[0], 39)
    hip_dev.volume_median(vol, 26)
    assert 0.0 <= hip_dev.volume_filter_last_ms() < 1000.0
    hip_dev.volume_smooth(vol, (1, 1, 1))
    assert 0.0 <= hip_dev.volume_filter_last_ms() < 1000.0


def test_a_refused_call_writes_nothing(hip_dev):
    shape = SMALL[1]
    with Filt(hip_dev, shape) as f:
        d_vol, out = f.put(fr.random_volume(shape, 40)), f.out()
        for rc in (f.lib.svr_volume_rank(C.c_void_p(d_vol), *f.dims, 1, fr.MEDIAN, 7, 1, C.c_void_p(out)),
                   f.lib.svr_volume_rank(C.c_void_p(d_vol), *f.dims, 1, fr.MEDIAN, 6, 65, C.c_void_p(out)),
                   f.lib.svr_volume_smooth(C.c_void_p(d_vol), *f.dims, 1, (C.c_uint32 * 3)(9, 0, 0), C.c_void_p(out)),
                   f.lib.svr_volume_rank(C.c_void_p(d_vol), *f.dims, 1, fr.MEDIAN, 6, 1, C.c_void_p(d_vol + 2))):
            assert rc == -3
            f.lib.svr_clear_error()
        assert (hip_dev.to_host(out, (f.n + GUARD,), np.uint16) == PATTERN).all()
