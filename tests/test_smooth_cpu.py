"""Smoothing of masks and label maps without a GPU (include/svr_abi.h, "smoothing region masks and label maps"): the numpy
reference against scipy and a brute-force mode, the properties of MAJORITY, the two host calls of the library, every refusal of the
three device calls -- they stand before the device is touched -- and the Python layer on the fake device."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import morph_ref as mr
from tests import smooth_ref as sm
from tests.host_fake import FakeDevice

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()
PTR = 1 << 40            # any non-null "device pointer": a refused call does not touch it
FAR = 1 << 44            # another one, far enough not to overlap

# (nx, ny, nz), radii: the shapes of the GPU tests (tests/test_smooth_gpu.py)
CASES = [((70, 21, 19), (7, 2, 3)), ((70, 21, 19), (8, 8, 8)), ((33, 5, 1), (8, 8, 8)), ((3, 1, 4), (7, 0, 1)), ((40, 7, 6), (3, 3, 3)),
         ((9, 9, 9), (1, 1, 1)), ((64, 16, 16), (1, 0, 0)), ((64, 16, 16), (0, 1, 0)), ((64, 16, 16), (0, 0, 1)), ((40, 7, 6), (0, 0, 0))]


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    return lib


def masks(shape_xyz, seed=0):
    shape = shape_xyz[::-1]
    return [np.random.default_rng(seed + sum(shape_xyz)).random(shape) < 0.5, sm.ball_with_salt(shape, seed)]


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("shape_xyz, radii", CASES)
def test_reference_count_and_majority_are_scipy(shape_xyz, radii):
    ndi = pytest.importorskip("scipy.ndimage")
    size = tuple(2 * r + 1 for r in radii[::-1])
    for m in masks(shape_xyz):
        count = sm.box_count(m, radii)
        assert count.dtype == np.uint16 and count.max() <= sm.box_size(radii)
        assert np.array_equal(count, ndi.correlate(m.astype(np.int32), np.ones(size, np.int32), mode="nearest"))
        assert np.array_equal(sm.majority(m, radii), ndi.median_filter(m.astype(np.uint8), size=size, mode="nearest").astype(bool))


@pytest.mark.parametrize("r", [1, 2, 4])
def test_count_extremes_are_dilate_and_erode(r):
    """count >= 1 is the dilation and count == N the erosion by the cube: the replicated border agrees with both"""
    ndi = pytest.importorskip("scipy.ndimage")
    for m in masks((40, 7, 6)) + [mr.two_balls()]:
        count, cube = sm.box_count(m, (r, r, r)), np.ones((2 * r + 1,) * 3, bool)
        assert np.array_equal(count >= 1, ndi.binary_dilation(m, cube)) and np.array_equal(count >= 1, mr.dilate(m, 26, r))
        assert np.array_equal(count == (2 * r + 1) ** 3, ndi.binary_erosion(m, cube, border_value=1))
        assert np.array_equal(count == (2 * r + 1) ** 3, mr.erode(m, 26, r))


@pytest.mark.parametrize("shape_xyz, radii", CASES)
def test_majority_is_self_dual_and_keeps_its_fixed_points(shape_xyz, radii):
    shape = shape_xyz[::-1]
    for m in masks(shape_xyz):
        assert np.array_equal(sm.majority(~m, radii), ~sm.majority(m, radii))
    for fixed in (np.ones(shape, bool), np.zeros(shape, bool)):
        assert np.array_equal(sm.majority(fixed, radii), fixed)
    for axis in range(3):
        for cut in (0, shape[axis] // 2, shape[axis] - 1):
            half = np.zeros(shape, bool)
            half[tuple(slice(cut, None) if a == axis else slice(None) for a in range(3))] = True
            assert np.array_equal(sm.majority(half, radii), half), (axis, cut)
            assert np.array_equal(sm.majority(~half, radii), ~half), (axis, cut)


def test_binomial_is_the_upper_half_of_the_smoothed_mask():
    m = masks((40, 7, 6))[1]
    assert np.array_equal(sm.binomial(m, (0, 0, 0)), m)
    out, changed = sm.smooth(m, sm.BINOMIAL, (1, 1, 1), 2)
    assert np.array_equal(out, sm.binomial(sm.binomial(m, (1, 1, 1)), (1, 1, 1))) and changed == (out != m).sum()
    line = np.zeros((1, 1, 8), bool)                           # halves round up: (2 * 65535 + 2) >> 2 = 32768 keeps a lone voxel ...
    line[0, 0, 3] = True
    assert np.array_equal(sm.binomial(line, (1, 0, 0)), line)
    assert sm.binomial(~line, (1, 0, 0)).all()                # ... and fills a lone hole: not self-dual


@pytest.mark.parametrize("shape_xyz, radii, count", [((9, 9, 9), (1, 1, 1), 3), ((12, 5, 4), (3, 1, 2), 4), ((7, 6, 3), (2, 2, 2), 255),
                                                      ((3, 1, 4), (7, 0, 1), 1)])
def test_reference_mode_is_the_brute_force(shape_xyz, radii, count):
    rng = np.random.default_rng(count)
    lab = rng.integers(0, min(count, 6) + 2, shape_xyz[::-1]).astype(np.uint32)      # (holds a value above count when count < 6)
    if count == 255:
        lab *= 40
    got, changed = sm.label_smooth(lab, count, radii)
    assert np.array_equal(got, sm.mode_brute(lab, count, radii)) and changed == (got != sm.read_labels(lab, count)).sum()


def test_mode_tie_rule():
    """a checkerboard of labels 2 and 3 around a 1: 13 : 13 : 1 at the centre -> the smaller; 14 : 13 elsewhere keeps the centre's own
    only where it is the 14"""
    z, y, x = np.mgrid[:3, :3, :3]
    lab = np.where((x + y + z) % 2 == 0, 2, 3).astype(np.uint32)
    lab[1, 1, 1] = 1
    board = np.pad(lab, 3, mode="edge")
    got, _ = sm.label_smooth(board, 3, (1, 1, 1))
    assert got[4, 4, 4] == 2 and np.array_equal(got, sm.mode_brute(board, 3, (1, 1, 1)))
    two = np.array([[[1, 2, 1, 2]]], np.uint32)                 # windows at the ends: 2 : 1 by the clamp
    assert sm.label_smooth(two, 2, (1, 0, 0))[0].tolist() == [[[1, 1, 2, 2]]]


@pytest.mark.parametrize("shape_xyz, radii", CASES)
def test_mode_of_one_label_is_majority(shape_xyz, radii):
    for m in masks(shape_xyz):
        got, changed = sm.label_smooth(m.astype(np.uint32), 1, radii, 2)
        want, wchanged = sm.smooth(m, sm.MAJORITY, radii, 2)
        assert np.array_equal(got, want.astype(np.uint32)) and changed == wchanged


# ------------------------------------------------------------------------------------------------ the host calls of the library
def test_constants(lib):
    for name, value in (("SVR_SMOOTH_MAJORITY", abi.SMOOTH_MAJORITY), ("SVR_SMOOTH_BINOMIAL", abi.SMOOTH_BINOMIAL),
                        ("SVR_REGION_SMOOTH_MAX_RADIUS", abi.REGION_SMOOTH_MAX_RADIUS),
                        ("SVR_REGION_SMOOTH_MAX_ITERATIONS", abi.REGION_SMOOTH_MAX_ITERATIONS),
                        ("SVR_LABEL_SMOOTH_MAX_COUNT", abi.LABEL_SMOOTH_MAX_COUNT)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", HEADER).group(1)) == value
    assert abi.REGION_SMOOTH_MAX_RADIUS == abi.SMOOTH_MAX_RADIUS and (abi.SMOOTH_MAJORITY, abi.SMOOTH_BINOMIAL) == (sm.MAJORITY, sm.BINOMIAL)


def test_box_size(lib):
    for radii in ((0, 0, 0), (1, 1, 1), (7, 2, 3), (8, 8, 8), (0, 8, 0)):
        assert host.region_box_size(radii, lib) == sm.box_size(radii)
    assert host.region_box_size((8, 8, 8), lib) == 4913
    for radii in ((9, 0, 0), (0, 9, 0), (0, 0, 1 << 31)):
        assert host.region_box_size(radii, lib) == 0
    assert lib.svr_region_box_size(None) == 0


def test_smooth_radii(lib):
    for q, r in ((0.0, 0), (1.0, 0), (1.9, 0), (2.0, 1), (3.0, 1), (4.0, 2), (5.0, 2), (16.9, 8), (17.0, 8), (17.9, 8)):
        radii, sizes = host.region_smooth_radii((1.0, 1.0, 2.0), q, lib)
        assert radii[0] == r and sizes[0] == 2 * r + 1 and (radii, sizes) == sm.smooth_radii((1.0, 1.0, 2.0), q), q
    radii, sizes = host.region_smooth_radii((0.5, 0.5, 1.5), 3.0, lib)               # q = 6, 6, 2
    assert radii == (3, 3, 1) and sizes == (3.5, 3.5, 4.5) and (radii, sizes) == sm.smooth_radii((0.5, 0.5, 1.5), 3.0)
    r, so = (C.c_uint32 * 3)(7, 7, 7), (C.c_double * 3)(7.0, 7.0, 7.0)
    sp = lambda *v: (C.c_double * 3)(*v)                                              # noqa: E731

    def refused(rc, code):
        assert rc == code and lib.svr_last_error_code() == code and b"svr_region_smooth_radii" in lib.svr_last_error()
        assert list(r) == [7, 7, 7] and list(so) == [7.0, 7.0, 7.0]                  # nothing written
        lib.svr_clear_error()
    refused(lib.svr_region_smooth_radii(None, 1.0, r, so), -4)
    refused(lib.svr_region_smooth_radii(sp(1, 1, 1), 1.0, None, so), -4)
    for bad in ((0.0, 1, 1), (1, -1.0, 1), (1, 1, math.inf), (math.nan, 1, 1)):
        refused(lib.svr_region_smooth_radii(sp(*bad), 1.0, r, so), -3)
    for size in (-1.0, math.inf, math.nan):
        refused(lib.svr_region_smooth_radii(sp(1, 1, 1), size, r, so), -3)
    refused(lib.svr_region_smooth_radii(sp(1, 1, 1), 18.0, r, so), -3)                # (18 - 1) / 2 = 8.5 rounds to 9
    refused(lib.svr_region_smooth_radii(sp(1, 1, 0.1), 3.0, r, so), -3)
    refused(lib.svr_region_smooth_radii(sp(1, 1, 1e-300), 1e300, r, so), -3)
    assert lib.svr_region_smooth_radii(sp(1, 1, 1), 3.0, r, None) == 0 and list(r) == [1, 1, 1]


# ------------------------------------------------------------------------------------------------ the refusals of the device calls
def test_device_call_refusals(lib):
    u32, dims3 = lambda *v: (C.c_uint32 * 3)(*v), lambda *v: (C.c_int32 * 3)(*v)     # noqa: E731
    changed = C.c_uint64(77)

    def refused(name, rc, code):
        assert rc == code and lib.svr_last_error_code() == code and name.encode() in lib.svr_last_error(), (name, rc, lib.svr_last_error())
        assert changed.value == 77
        lib.svr_clear_error()

    def count(mask=PTR, dims=(4, 4, 4), radii=(1, 1, 1), out=FAR):
        return lib.svr_region_box_count(mask, None if dims is None else dims3(*dims), None if radii is None else u32(*radii), out)

    def smooth(mask=PTR, dims=(4, 4, 4), op=abi.SMOOTH_MAJORITY, radii=(1, 1, 1), iterations=1, out=FAR):
        return lib.svr_region_smooth(mask, None if dims is None else dims3(*dims), op, None if radii is None else u32(*radii), iterations, out,
                                     C.byref(changed))

    def mode(labels=PTR, dims=(4, 4, 4), n=3, radii=(1, 1, 1), iterations=1, out=FAR):
        return lib.svr_region_label_smooth(labels, None if dims is None else dims3(*dims), n, None if radii is None else u32(*radii), iterations,
                                           out, C.byref(changed))

    def density(mask=PTR, dims=(4, 4, 4), radii=(1, 1, 1), out=FAR):
        return lib.svr_region_box_density(mask, None if dims is None else dims3(*dims), None if radii is None else u32(*radii), out)

    for name, call, first in (("svr_region_box_count", count, "mask"), ("svr_region_box_density", density, "mask"), ("svr_region_smooth", smooth, "mask"),
                              ("svr_region_label_smooth", mode, "labels")):
        for kw in ({first: None}, {"dims": None}, {"radii": None}, {"out": None}):
            refused(name, call(**kw), -4)
        for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (2048, 2048, 513)):
            refused(name, call(dims=dims), -6)
        for radii in ((9, 0, 0), (0, 9, 0), (1, 1, 0xFFFFFFFF)):
            refused(name, call(radii=radii), -3)
        refused(name, call(out=PTR), -3)                          # out is the input
        refused(name, call(out=PTR + 4), -3)
    refused("svr_region_box_count", count(out=PTR - 100), -3)      # the u16 volume (128 bytes) reaches into the mask from below
    for op in (0, 3, -1):
        refused("svr_region_smooth", smooth(op=op), -3)
    for name, call in (("svr_region_smooth", smooth), ("svr_region_label_smooth", mode)):
        for iterations in (0, 17, 0xFFFFFFFF):
            refused(name, call(iterations=iterations), -3)
    refused("svr_region_smooth", smooth(op=abi.SMOOTH_BINOMIAL, radii=(0, 0, 9)), -3)
    for n in (0, 256, 0xFFFFFFFF):
        refused("svr_region_label_smooth", mode(n=n), -3)
    refused("svr_region_smooth_last_ms", lib.svr_region_smooth_last_ms(None), -4)


def test_declarations_keep_the_closed_refusal_list_closed():
    """the three calls take dims[3]: no new declaration carries `int nx, int ny, int nz` on its first line"""
    for name in ("svr_region_box_count", "svr_region_smooth", "svr_region_label_smooth"):
        assert re.search(rf"^int {name}\([^\n]*const int32_t dims\[3\]", HEADER, flags=re.M), name


# ------------------------------------------------------------------------------------------------ the Python layer on the fake device
def test_python_argument_errors():
    m, lab = np.zeros((6, 4, 5), bool), np.zeros((6, 4, 5), np.uint32)
    for fn, args in (("region_box_count", (m,)), ("region_smooth", (m, abi.SMOOTH_MAJORITY)), ("region_label_smooth", (lab, 3))):
        for radii in ((1, 1), (1, 1, -1), (1, 1, 1, 1)):
            dev = FakeDevice()
            with pytest.raises(ValueError):
                getattr(dev, fn)(*args, radii)
            assert dev.lib.calls == [] and dev.live == set() and dev.nmalloc == 0
        for bad in ((np.zeros((4, 5), bool if fn != "region_label_smooth" else np.uint32),) + args[1:], (1 << 61,) + args[1:]):
            dev = FakeDevice()
            with pytest.raises(ValueError):
                getattr(dev, fn)(*bad, (1, 1, 1))
            assert dev.lib.calls == [] and dev.live == set()


def test_fake_device_calls_and_no_leak():
    m, lab = np.zeros((6, 4, 40), bool), np.zeros((6, 4, 40), np.uint32)
    dev = FakeDevice()
    count = dev.region_box_count(m, (7, 2, 3))
    assert count.shape == m.shape and count.dtype == np.uint16 and dev.live == set()
    call = dev.lib.calls[-1]
    assert call["fn"] == "svr_region_box_count" and call["args"][1:3] == [[40, 4, 6], [7, 2, 3]]
    assert dev.region_box_count(m, (1, 1, 1), density=True).dtype == np.uint16 and dev.lib.calls[-1]["fn"] == "svr_region_box_density"
    out, changed = dev.region_smooth(m, abi.SMOOTH_BINOMIAL, (1, 0, 2), iterations=3)
    assert out.shape == m.shape and out.dtype == bool and changed == 0 and dev.live == set()
    call = dev.lib.calls[-1]
    assert call["fn"] == "svr_region_smooth" and call["args"][1:5] == [[40, 4, 6], abi.SMOOTH_BINOMIAL, [1, 0, 2], 3] and call["args"][6] == 0
    out, changed = dev.region_label_smooth(lab, 5, (1, 1, 1), 2)
    assert out.shape == lab.shape and out.dtype == np.uint32 and changed == 0 and dev.live == set()
    call = dev.lib.calls[-1]
    assert call["fn"] == "svr_region_label_smooth" and call["args"][1:5] == [[40, 4, 6], 5, [1, 1, 1], 2]
    assert dev.region_smooth_last_ms() == 0.0
    # a caller's buffers: the pointer comes back for the count and the labels, the mask is read back
    words = host.region_mask_words(m.shape)
    d_in, d_out, d_u16, d_lab = dev.malloc(4 * words), dev.malloc(4 * words), dev.malloc(2 * m.size), dev.malloc(4 * m.size)
    assert dev.region_box_count(d_in, (1, 1, 1), shape=m.shape, out_ptr=d_u16) == d_u16
    assert dev.region_smooth(d_in, abi.SMOOTH_MAJORITY, (1, 1, 1), shape=m.shape, out_ptr=d_out)[0].shape == m.shape
    assert dev.region_label_smooth(lab, 5, (1, 1, 1), out_ptr=d_lab)[0] == d_lab
    assert dev.live == {d_in, d_out, d_u16, d_lab}
    # nothing stays allocated when the library call or an allocation fails
    for fn, args in (("region_box_count", (m, (1, 1, 1))), ("region_smooth", (m, abi.SMOOTH_MAJORITY, (1, 1, 1))),
                     ("region_label_smooth", (lab, 3, (1, 1, 1)))):
        for fail in (dict(fail_call=1), dict(fail_malloc=1), dict(fail_malloc=2)):
            dev = FakeDevice()
            dev.lib.fail_call, dev.fail_malloc = fail.get("fail_call"), fail.get("fail_malloc")
            with pytest.raises(host.SvrError):
                getattr(dev, fn)(*args)
            assert dev.live == set()
