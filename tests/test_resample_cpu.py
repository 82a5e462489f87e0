"""Crop / resample without a device: the grid helpers of the library against the test-side reference (tests/resample_ref.py), the
placement of a resampled volume, every refusal of the new entry points (they answer before the device is touched), the reference's own
properties -- they keep the reference and the kernels from sharing a mistake -- and the MetaImage writer's round trips."""
import ctypes as C
import zlib

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from sunvolumerender_amd import io as sio
from tests import resample_ref as rr


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    lib.svr_clear_error()
    return lib


def i3(*v):
    return (C.c_int32 * 3)(*v)


def d3(*v):
    return (C.c_double * 3)(*v)


def refused(lib, rc, code, name):
    msg = lib.svr_last_error().decode()
    lib.svr_clear_error()
    assert rc == code, (rc, msg)
    assert name in msg, msg


# ---------------------------------------------------------------- the grid helpers against the reference
SHAPE = (43, 36, 28)                                     # (nz, ny, nx)
DIMS = (28, 36, 43)
BOXES = [None, ((3, 4, 5), (20, 30, 40)), ((-5, -1, -100), (10, 99, 7)), ((27, 35, 42), (27, 35, 42)), ((0, 0, 0), (500, 500, 500))]


@pytest.mark.parametrize("box", BOXES[1:], ids=str)
def test_grid_box_against_reference(lib, box):
    assert host.resample_grid_box(SHAPE, box, lib).as_tuples() == rr.grid_box(DIMS, *box)


@pytest.mark.parametrize("box", BOXES, ids=str)
@pytest.mark.parametrize("src,target", [((0.9, 0.9, 1.5), (0.9, 0.9, 0.9)), ((0.5, 0.5, 2.0), (1.0, 1.0, 1.0)), ((1.0, 1.0, 1.0), (2.0, 2.0, 2.0)),
                                        ((0.7, 1.3, 0.31), (0.45, 2.9, 0.33))], ids=str)
def test_grid_spacing_against_reference(lib, box, src, target):
    g, applied = host.resample_grid_spacing(SHAPE, src, target, box, lib)
    want, want_applied = rr.grid_spacing(DIMS, src, target, *(box or (None, None)))
    assert g.as_tuples() == want
    assert applied == want_applied                        # exact doubles
    assert g.shape == rr.grid_shape(want)


def test_grid_spacing_count_rounds_half_up(lib):
    # 3 voxels at step 2: 1.5 cells -> 2; 5 voxels at step 2: 2.5 -> 3; 1 voxel at step 4: 0.25 -> max(1, 0)
    for n, factor, count in [(3, 2.0, 2), (5, 2.0, 3), (1, 4.0, 1), (7, 2.0, 4), (6, 4.0, 2)]:
        g, _ = host.resample_grid_spacing((n, n, n), (1.0, 1.0, 1.0), (factor,) * 3, None, lib)
        assert g.as_tuples() == rr.grid_spacing((n, n, n), (1.0,) * 3, (factor,) * 3)[0]
        assert g.axis[0].count == count


@pytest.mark.parametrize("step,ok", [(1024.0, True), (1023.5, True), (1023.4, False), (4194304.0, True), (4194304.4, True), (4194304.5, False)])
def test_grid_spacing_step_limits(lib, step, ok):
    target = step / 65536.0                               # exact: a power of two divides
    for axis in range(3):
        t = [1.0, 1.0, 1.0]
        t[axis] = target
        g, out = abi.ResampleGrid(), d3(7.0, 7.0, 7.0)
        g.axis[0].step = 77
        rc = lib.svr_resample_grid_spacing(i3(*DIMS), d3(1.0, 1.0, 1.0), None, None, d3(*t), C.byref(g), out)
        if ok:
            assert rc == 0, lib.svr_last_error().decode()
            assert g.as_tuples() == rr.grid_spacing(DIMS, (1.0,) * 3, t)[0]
            assert g.axis[axis].step in (rr.MIN_STEP, rr.MAX_STEP)
        else:
            refused(lib, rc, -3, "svr_resample_grid_spacing")
            assert g.axis[0].step == 77 and list(out) == [7.0, 7.0, 7.0]
            with pytest.raises(rr.Refused):
                rr.grid_spacing(DIMS, (1.0,) * 3, t)


@pytest.mark.parametrize("box", BOXES, ids=str)
@pytest.mark.parametrize("out_shape", [(43, 36, 28), (21, 18, 14), (22, 18, 14), (64, 64, 64), (1, 1, 1), (5, 200, 3)], ids=str)
def test_grid_dims_against_reference(lib, box, out_shape):
    try:
        want = rr.grid_dims(DIMS, out_shape[::-1], *(box or (None, None)))
    except rr.Refused:
        with pytest.raises(host.SvrError):
            host.resample_grid_dims(SHAPE, out_shape, box, lib)
        return
    g = host.resample_grid_dims(SHAPE, out_shape, box, lib)
    assert g.as_tuples() == want and g.shape == tuple(out_shape)


def test_grid_place_maps_a_point_to_the_cell_its_source_voxel_meets(lib):
    """A point of the output box lies in source voxel i (svr_region_seed_from_world on the source volume) and in output cell j (the same
    call on the placed volume): cell j must be one that voxel i meets.  The points are centres of (voxel, cell) intersections, so
    float32 rounding cannot move them across an edge."""
    spacing = (0.9, 0.9, 1.5)
    src = host.create_device_volume(0x1234, DIMS, spacing, 3.0)
    src.densityScale, src.gradientFactor = 2.5, 0.25
    rng = np.random.default_rng(5)
    grids = [host.resample_grid_box(SHAPE, ((3, 4, 5), (20, 30, 40)), lib),
             host.resample_grid_spacing(SHAPE, spacing, 0.9, None, lib)[0],
             host.resample_grid_spacing(SHAPE, spacing, (2.0, 0.5, 1.1), ((2, 2, 2), (25, 30, 40)), lib)[0],
             host.resample_grid_dims(SHAPE, (20, 50, 28), None, lib)]
    for g in grids:
        placed = host.resample_grid_place(src, SHAPE, g, lib)
        assert placed.tex == src.tex and placed.densityScale == src.densityScale and placed.gradientFactor == src.gradientFactor
        assert placed.invMaxMagnitude == src.invMaxMagnitude
        out_dims = g.shape[::-1]
        vmin = (src.bbox.vmin.x, src.bbox.vmin.y, src.bbox.vmin.z)
        sp = (src.spacing.x, src.spacing.y, src.spacing.z)
        for a, name in enumerate("xyz"):
            origin, step, count = g.as_tuples()[a]
            assert getattr(placed.bbox.vmin, name) == np.float32(vmin[a] + origin / 65536.0 * sp[a])
            assert getattr(placed.spacing, name) == np.float32(sp[a] * step / 65536.0)
        for _ in range(200):
            point, want = [], []
            for a in range(3):
                origin, step, count = g.as_tuples()[a]
                j = int(rng.integers(0, count))
                lo, hi = max(origin + j * step, 0), min(origin + (j + 1) * step, DIMS[a] << 16)
                wide = [i for i in range(lo >> 16, ((hi - 1) >> 16) + 1) if min(hi, (i + 1) << 16) - max(lo, i << 16) >= 8192]
                i = wide[int(rng.integers(0, len(wide)))]                                    # an eighth of a voxel or more of cell j
                e =(max(lo, i << 16) + min(hi, (i + 1) << 16)) / 2.0 / 65536.0            # the centre of voxel i's part of cell j
                point.append(vmin[a] + e * sp[a])
                want.append((i, j))
            ijk = host.region_seed_from_world(lib, src, DIMS, point)
            cell = host.region_seed_from_world(lib, placed, out_dims, point)
            assert [(ijk[a], cell[a]) for a in range(3)] == want


# ---------------------------------------------------------------- refusals
FAKE, FAKE2 = C.c_void_p(0x10000), C.c_void_p(0x40000000)


def good_grid():
    return host.resample_grid(((0, 65536, 4), (0, 65536, 4), (0, 65536, 4)))


def bad_grids():
    """(grid tuples, code) for a 4 x 4 x 4 source"""
    ok = (0, 65536, 4)
    return [((ok, (0, 1023, 4), ok), -3), ((ok, ok, (0, 4194305, 4)), -3), (((0, 65536, 0), ok, ok), -3), ((ok, (4 << 16, 65536, 4), ok), -3),
            ((ok, ok, (-(4 << 16), 65536, 4)), -3), (((1 << 47, 65536, 4), ok, ok), -3), (((-(1 << 47), 4194304, 4), ok, ok), -3),
            (((0, 65536, 1 << 16), (0, 65536, 1 << 16), ok), -6), (((0, 65536, 0x80000000), ok, ok), -6)]


def test_volume_resample_refusals(lib):
    name, dims, g = "svr_volume_resample", i3(4, 4, 4), good_grid()
    call = lib.svr_volume_resample
    refused(lib, call(None, dims, 1, C.byref(g), 0, FAKE2), -4, name)
    refused(lib, call(FAKE, None, 1, C.byref(g), 0, FAKE2), -4, name)
    refused(lib, call(FAKE, dims, 1, None, 0, FAKE2), -4, name)
    refused(lib, call(FAKE, dims, 1, C.byref(g), 0, None), -4, name)
    refused(lib, call(FAKE, i3(0, 4, 4), 1, C.byref(g), 0, FAKE2), -6, name)
    refused(lib, call(FAKE, i3(4, -1, 4), 1, C.byref(g), 0, FAKE2), -6, name)
    refused(lib, call(FAKE, i3(2048, 2048, 513), 1, C.byref(g), 0, FAKE2), -6, name)
    for tuples, code in bad_grids():
        bad = host.resample_grid(tuples)
        refused(lib, call(FAKE, dims, 1, C.byref(bad), 0, FAKE2), code, name)
    for mode in (-1, 4):
        refused(lib, call(FAKE, dims, 1, C.byref(g), mode, FAKE2), -3, name)
    refused(lib, call(FAKE, dims, 1, C.byref(g), 0, FAKE), -3, name)                          # out is voxels
    refused(lib, call(FAKE, dims, 1, C.byref(g), 0, C.c_void_p(0x10000 + 126)), -3, name)     # out begins in the last voxel


@pytest.mark.parametrize("name", ["svr_region_resample", "svr_region_label_resample"])
def test_mask_and_label_resample_refusals(lib, name):
    call, dims, g = getattr(lib, name), i3(4, 4, 4), good_grid()
    refused(lib, call(None, dims, C.byref(g), FAKE2), -4, name)
    refused(lib, call(FAKE, None, C.byref(g), FAKE2), -4, name)
    refused(lib, call(FAKE, dims, None, FAKE2), -4, name)
    refused(lib, call(FAKE, dims, C.byref(g), None), -4, name)
    refused(lib, call(FAKE, i3(4, 4, 0), C.byref(g), FAKE2), -6, name)
    for tuples, code in bad_grids():
        bad = host.resample_grid(tuples)
        refused(lib, call(FAKE, dims, C.byref(bad), FAKE2), code, name)
    refused(lib, call(FAKE, dims, C.byref(g), FAKE), -3, name)
    refused(lib, call(FAKE, dims, C.byref(g), C.c_void_p(0x10000 + 60)), -3, name)            # the mask has 16 words, the map 64


def test_paste_refusals(lib):
    name, call = "svr_region_paste", lib.svr_region_paste
    sub, full, off = i3(4, 4, 4), i3(40, 8, 8), i3(1, 2, 3)
    refused(lib, call(None, sub, FAKE2, full, off, 0), -4, name)
    refused(lib, call(FAKE, None, FAKE2, full, off, 0), -4, name)
    refused(lib, call(FAKE, sub, None, full, off, 0), -4, name)
    refused(lib, call(FAKE, sub, FAKE2, None, off, 0), -4, name)
    refused(lib, call(FAKE, sub, FAKE2, full, None, 0), -4, name)
    refused(lib, call(FAKE, i3(0, 4, 4), FAKE2, full, off, 0), -6, name)
    refused(lib, call(FAKE, sub, FAKE2, i3(40, 8, -8), off, 0), -6, name)
    for bad in [(-1, 0, 0), (37, 0, 0), (0, 5, 0), (0, 0, 5), (0, 0, 2 ** 31 - 1)]:
        refused(lib, call(FAKE, sub, FAKE2, full, i3(*bad), 0), -3, name)
    for op in (-1, 1, 4, 5):                             # MASK_AND, _XOR and _NOT are not paste ops
        refused(lib, call(FAKE, sub, FAKE2, full, off, op), -3, name)
    refused(lib, call(FAKE, sub, FAKE, full, off, 0), -3, name)


def test_expand_refusals(lib):
    name, call, dims = "svr_region_mask_expand", lib.svr_region_mask_expand, i3(4, 4, 4)
    refused(lib, call(None, dims, 1, FAKE2), -4, name)
    refused(lib, call(FAKE, None, 1, FAKE2), -4, name)
    refused(lib, call(FAKE, dims, 1, None), -4, name)
    refused(lib, call(FAKE, i3(4, 0, 4), 1, FAKE2), -6, name)
    for value in (0, -1, 256):
        refused(lib, call(FAKE, dims, value, FAKE2), -3, name)
    refused(lib, call(FAKE, dims, 1, FAKE), -3, name)
    refused(lib, lib.svr_volume_resample_last_ms(None), -4, "svr_volume_resample_last_ms")


def test_grid_helper_refusals_write_nothing(lib):
    dims, lo, hi = i3(*DIMS), i3(0, 0, 0), i3(5, 5, 5)
    g = host.resample_grid(((7, 7, 7),) * 3)
    untouched = lambda: g.as_tuples() == ((7, 7, 7),) * 3
    name = "svr_resample_grid_box"
    for args in [(None, lo, hi, C.byref(g)), (dims, None, hi, C.byref(g)), (dims, lo, None, C.byref(g)), (dims, lo, hi, None)]:
        refused(lib, lib.svr_resample_grid_box(*args), -4, name)
    refused(lib, lib.svr_resample_grid_box(i3(0, 1, 1), lo, hi, C.byref(g)), -6, name)
    for b0, b1 in [((5, 0, 0), (4, 5, 5)), ((0, 36, 0), (5, 40, 5)), ((0, 0, -9), (5, 5, -1))]:
        refused(lib, lib.svr_resample_grid_box(dims, i3(*b0), i3(*b1), C.byref(g)), -3, name)
    name = "svr_resample_grid_spacing"
    one = d3(1.0, 1.0, 1.0)
    for args in [(None, one, None, None, one, C.byref(g), None), (dims, None, None, None, one, C.byref(g), None),
                 (dims, one, None, None, None, C.byref(g), None), (dims, one, None, None, one, None, None)]:
        refused(lib, lib.svr_resample_grid_spacing(*args), -4, name)
    refused(lib, lib.svr_resample_grid_spacing(i3(1, 1, -1), one, None, None, one, C.byref(g), None), -6, name)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(lib, lib.svr_resample_grid_spacing(dims, d3(1.0, bad, 1.0), None, None, one, C.byref(g), None), -3, name)
        refused(lib, lib.svr_resample_grid_spacing(dims, one, None, None, d3(1.0, 1.0, bad), C.byref(g), None), -3, name)
    refused(lib, lib.svr_resample_grid_spacing(dims, one, i3(9, 0, 0), i3(3, 5, 5), one, C.byref(g), None), -3, name)
    name = "svr_resample_grid_dims"
    for args in [(None, None, None, i3(4, 4, 4), C.byref(g)), (dims, None, None, None, C.byref(g)), (dims, None, None, i3(4, 4, 4), None)]:
        refused(lib, lib.svr_resample_grid_dims(*args), -4, name)
    refused(lib, lib.svr_resample_grid_dims(dims, None, None, i3(4, 0, 4), C.byref(g)), -6, name)
    refused(lib, lib.svr_resample_grid_dims(i3(200, 4, 4), None, None, i3(3, 4, 4), C.byref(g)), -3, name)        # step 66.7 voxels
    refused(lib, lib.svr_resample_grid_dims(i3(2, 4, 4), None, None, i3(129, 4, 4), C.byref(g)), -3, name)        # step 1016
    assert untouched()
    name = "svr_resample_grid_place"
    vol, out = abi.cudaVolume(), abi.cudaVolume()
    out.tex = 99
    ok = good_grid()
    for args in [(None, dims, C.byref(ok), C.byref(out)), (C.byref(vol), None, C.byref(ok), C.byref(out)), (C.byref(vol), dims, None, C.byref(out)),
                 (C.byref(vol), dims, C.byref(ok), None)]:
        refused(lib, lib.svr_resample_grid_place(*args), -4, name)
    refused(lib, lib.svr_resample_grid_place(C.byref(vol), i3(0, 0, 0), C.byref(ok), C.byref(out)), -6, name)
    refused(lib, lib.svr_resample_grid_place(C.byref(vol), dims, C.byref(g), C.byref(out)), -3, name)             # step 7
    assert out.tex == 99


# ---------------------------------------------------------------- the reference's own properties
def rand(shape, seed=1):
    return np.random.default_rng(seed).integers(0, 65536, size=shape, dtype=np.uint16)


STEPS = [1024, 32768, 43691, 65535, 65536, 65537, 98304, 131072, 4194304]


def test_reference_identity_and_crop_equal_slicing():
    v = rand((6, 7, 9))
    ident = ((0, 65536, 9), (0, 65536, 7), (0, 65536, 6))
    crop = ((2 << 16, 65536, 5), (1 << 16, 65536, 6), (3 << 16, 65536, 2))
    for mode in rr.MODES:
        assert np.array_equal(rr.volume_resample(v, ident, mode), v)
        assert np.array_equal(rr.volume_resample(v, crop, mode), v[3:5, 1:7, 2:7])
    assert np.array_equal(rr.volume_resample(v, rr.grid_box((9, 7, 6), (2, 1, 3), (6, 6, 4)), rr.NEAREST), v[3:5, 1:7, 2:7])
    # a crop that sticks out replicates the border
    out = rr.volume_resample(v, ((-(2 << 16), 65536, 13), (0, 65536, 7), (0, 65536, 6)), rr.LINEAR)
    assert np.array_equal(out, np.pad(v, ((0, 0), (0, 0), (2, 2)), mode="edge"))


def test_reference_area_by_an_integer_factor_is_the_rounded_block_mean():
    v = rand((8, 6, 12), 2)
    for factor in (2, 3):
        want = v
        for axis in (2, 1, 0):                           # x, y, z: one rounding per axis
            n = want.shape[axis] // factor
            blocks = np.stack([np.take(want, np.arange(n) * factor + k, axis=axis).astype(np.int64) for k in range(factor)])
            want = ((2 * blocks.sum(axis=0) + factor) // (2 * factor)).astype(np.uint16)
        grid = tuple((0, factor * 65536, v.shape[2 - a] // factor) for a in range(3))
        assert np.array_equal(rr.volume_resample(v, grid, rr.AREA), want)
    pair = rr.axis_area(v, 2, 0, 131072, 6).astype(np.int64)
    assert np.array_equal(pair, (v[:, :, 0::2].astype(np.int64) + v[:, :, 1::2] + 1) >> 1)


@pytest.mark.parametrize("step", STEPS)
def test_reference_constants_stay_and_outputs_lie_in_the_source_range(step):
    count = 7 if step > 65536 else 40
    grid = ((-70000, step, count), (12345, step, 5), (0, 65536, 2))
    for value in (0, 1, 40000, 65535):
        c = np.full((2, 5, 6), value, dtype=np.uint16)
        for mode in rr.MODES:
            assert (rr.volume_resample(c, grid, mode) == value).all()
    v = rand((2, 5, 6), 3)
    v[v < 1000] = 1000
    v[v > 60000] = 60000
    for mode in rr.MODES:
        out = rr.volume_resample(v, grid, mode)
        assert out.shape == (2, 5, count) and out.min() >= v.min() and out.max() <= v.max()


def test_reference_linear_at_f_0_copies_and_halfway_averages():
    v = rand((3, 4, 10), 4)
    # c - 32768 = origin + j step + step / 2 - 32768 a multiple of 65536: step 65536, origin a multiple of 65536
    assert np.array_equal(rr.axis_linear(v, 2, 3 << 16, 65536, 7), v[:, :, 3:10])
    # step 32768 from origin 16384: centres at 32768 + 32768 j, so t = 32768 j: f = 0 at even j, f = 1/2 at odd j
    out = rr.axis_linear(v, 2, 16384, 32768, 19)
    assert np.array_equal(out[:, :, 0::2], v)
    assert np.array_equal(out[:, :, 1::2].astype(np.int64), (v[:, :, :-1].astype(np.int64) + v[:, :, 1:] + 1) >> 1)


@pytest.mark.parametrize("step", STEPS[:-1])
def test_reference_mask_of_nearest_volume_is_nearest_mask(step):
    m = np.random.default_rng(6).integers(0, 2, size=(5, 6, 37)).astype(bool)
    grid = ((-40000, step, 50), (1 << 16, 65536, 4), (7, step, 9))
    as_volume = rr.volume_resample(m.astype(np.uint16), grid, rr.NEAREST)
    assert np.array_equal(as_volume != 0, rr.nearest_any(m, grid))


def test_reference_paste_after_crop_restores_the_mask():
    m = np.random.default_rng(7).integers(0, 2, size=(6, 7, 70)).astype(bool)
    box = ((30, 2, 1), (66, 5, 4))
    sub = rr.nearest_any(m, rr.grid_box((70, 7, 6), *box))
    assert np.array_equal(sub, m[1:5, 2:6, 30:67])
    other = ~m
    assert np.array_equal(rr.paste(m, sub, box[0], rr.PASTE_REPLACE), m)
    back = rr.paste(other, sub, box[0], rr.PASTE_REPLACE)
    assert np.array_equal(back[1:5, 2:6, 30:67], sub)
    back[1:5, 2:6, 30:67] = other[1:5, 2:6, 30:67]
    assert np.array_equal(back, other)
    assert np.array_equal(rr.paste(np.zeros_like(m), sub, box[0], rr.MASK_OR)[1:5, 2:6, 30:67], sub)
    assert not rr.paste(m, sub, box[0], rr.MASK_ANDNOT)[1:5, 2:6, 30:67].any()
    assert np.array_equal(rr.expand(sub, 255), sub.astype(np.uint8) * 255)


# ---------------------------------------------------------------- svr_mhd_write
def parse_header(path):
    keys, raw = {}, path.read_bytes()
    pos = 0
    while True:
        eol = raw.index(b"\n", pos)
        k, v = raw[pos:eol].decode().split(" = ")
        keys[k] = v
        pos = eol + 1
        if k == "ElementDataFile":
            return keys, raw[pos:]


DTYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.float32, np.float64]


@pytest.mark.parametrize("shape", [(1, 1, 1), (33, 1, 3)], ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("ext,compress", [(".mhd", False), (".mhd", True), (".mha", False), (".mha", True)])
def test_mhd_write_round_trip(lib, tmp_path, shape, dtype, ext, compress):
    rng = np.random.default_rng(8)
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        arr = rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)
    else:
        arr = rng.standard_normal(shape).astype(dtype)
    spacing, offset = (0.1, 1.0 / 3.0, 2.5e-7), (-12.3, 1e10 / 7.0, 0.0)
    path = tmp_path / ("vol" + ext)
    sio.mhd_write(str(path), arr, spacing, offset, compress, lib)
    got, got_spacing = sio.mhd_read(str(path), lib)
    assert got.dtype == arr.dtype and np.array_equal(got, arr)
    assert got_spacing == spacing
    keys, tail = parse_header(path)
    assert list(keys)[:5] == ["ObjectType", "NDims", "BinaryData", "BinaryDataByteOrderMSB", "CompressedData"]
    assert keys["ObjectType"] == "Image" and keys["NDims"] == "3" and keys["BinaryData"] == "True" and keys["BinaryDataByteOrderMSB"] == "False"
    assert keys["TransformMatrix"] == "1 0 0 0 1 0 0 0 1" and keys["CenterOfRotation"] == "0 0 0"
    assert tuple(float(t) for t in keys["ElementSpacing"].split()) == spacing          # exact doubles
    assert tuple(float(t) for t in keys["Offset"].split()) == offset
    assert [int(t) for t in keys["DimSize"].split()] == list(shape[::-1])
    assert keys["CompressedData"] == str(bool(compress)) and ("CompressedDataSize" in keys) == bool(compress)
    if ext == ".mha":
        assert keys["ElementDataFile"] == "LOCAL"
        data = tail
        assert sorted(p.name for p in tmp_path.iterdir()) == ["vol.mha"]
    else:
        assert keys["ElementDataFile"] == ("vol.zraw" if compress else "vol.raw") and tail == b""
        data = (tmp_path / keys["ElementDataFile"]).read_bytes()
    if compress:
        assert int(keys["CompressedDataSize"]) == len(data)
        data = zlib.decompress(data)
    assert data == arr.tobytes()


def test_mhd_write_refusals(lib, tmp_path):
    name, arr = "svr_mhd_write", np.zeros(8, np.uint16)
    p, e = str(tmp_path / "a.mhd").encode(), arr.ctypes.data_as(C.c_void_p)
    dim, one, zero = i3(2, 2, 2), d3(1.0, 1.0, 1.0), d3(0.0, 0.0, 0.0)
    for args in [(None, e, 3, dim, one, zero, 0), (p, None, 3, dim, one, zero, 0), (p, e, 3, None, one, zero, 0), (p, e, 3, dim, None, zero, 0),
                 (p, e, 3, dim, one, None, 0)]:
        refused(lib, lib.svr_mhd_write(*args), -4, name)
    for args in [(p, e, 8, dim, one, zero, 0), (p, e, -1, dim, one, zero, 0), (p, e, 3, i3(2, 0, 2), one, zero, 0), (p, e, 3, dim, d3(1.0, 0.0, 1.0), zero, 0),
                 (p, e, 3, dim, one, d3(0.0, float("nan"), 0.0), 0)]:
        refused(lib, lib.svr_mhd_write(*args), -3, name)
    assert list(tmp_path.iterdir()) == []
    missing = str(tmp_path / "no_such_dir" / "a.mhd").encode()
    rc = lib.svr_mhd_write(missing, e, 3, dim, one, zero, 0)
    msg = lib.svr_last_error().decode()
    lib.svr_clear_error()
    assert rc == -20 and "no_such_dir" in msg
