"""svr_volume_resample / svr_region_resample / _label_resample / _paste / _mask_expand on the GPU: every result is EQUAL to the test-side
reference (tests/resample_ref.py: per axis, int64, straight from the definitions).  Output buffers are pre-filled with a pattern and
carry a guard tail that must come back untouched.  The shapes are those of tests/test_filter_gpu.py: thinner than any tile, one more
than a tile on every axis with an odd nx -- rows then start at odd u16 offsets, which the paired stores of the y and z passes must
handle -- several x segments, and the 48^3 head."""
import ctypes as C

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import filter_ref as fr
from tests import resample_ref as rr

pytestmark = pytest.mark.gpu

# (nz, ny, nx)
SMALL = [(1, 1, 1), (2, 2, 2), (1, 1, 40), (3, 1, 33)]
TILED = [(10, 9, 131), (5, 17, 63), (2, 3, 515)]
HEAD = (48, 48, 48)
STEPS = [65536, 32768, 43691, 98304, 131072, 65535, 65537]
GUARD = 64                                               # bytes past the end of an output
PATTERN = 0xA5
MODE_NAMES = {rr.NEAREST: "nearest", rr.LINEAR: "linear", rr.AREA: "area", rr.AUTO: "auto"}


class Rs:
    """Raw calls on buffers the test owns."""

    def __init__(self, dev):
        self.dev, self.lib, self.bufs = dev, dev.lib, []

    def raw(self, nbytes):
        p = self.dev.malloc(max(nbytes, 4))
        self.bufs.append(p)
        self.dev.check(self.lib.svr_memset_device(C.c_void_p(p), PATTERN, max(nbytes, 4)))
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

    def fetch(self, out, shape, dtype, what):
        """The result and the check of its guard tail."""
        self.dev.synchronize()
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        got = self.dev.to_host(out, (nbytes + GUARD,), np.uint8)
        assert (got[nbytes:] == PATTERN).all(), f"{what}: memory past the end of out was written"
        return got[:nbytes].view(dtype).reshape(shape)

    def volume(self, vox, src_shape, grid, mode, what):
        """svr_volume_resample of a host array or a device pointer into a fresh guarded buffer."""
        g = host.resample_grid(grid)
        out = self.raw(2 * int(np.prod(g.shape)) + GUARD)
        if isinstance(vox, np.ndarray):
            p, on_dev = vox.ctypes.data_as(C.c_void_p), 0
        else:
            p, on_dev = C.c_void_p(vox), 1
        self.ok(self.lib.svr_volume_resample(p, (C.c_int32 * 3)(*src_shape[::-1]), on_dev, C.byref(g), mode, C.c_void_p(out)))
        got = self.fetch(out, g.shape, np.uint16, what)
        self.free_last()
        return got

    def mask_words(self, d_mask, src_shape, grid, what):
        """svr_region_resample: the raw output words."""
        g = host.resample_grid(grid)
        words = host.region_mask_words(g.shape)
        out = self.raw(4 * words + GUARD)
        self.ok(self.lib.svr_region_resample(C.c_void_p(d_mask), (C.c_int32 * 3)(*src_shape[::-1]), C.byref(g), C.c_void_p(out)))
        got = self.fetch(out, (words,), np.uint32, what)
        self.free_last()
        return got

    def free_last(self):
        self.dev.free(self.bufs.pop())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.dev.free(p)
        self.bufs = []


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        diff = got != want
        at = tuple(np.argwhere(diff)[0].tolist())
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} elements differ; first {at}: {int(got[at])} for {int(want[at])}")


def count_for(n, step):
    return max(1, (n * 65536 + step // 2) // step)


def uniform_grid(shape, step, origin=0):
    return tuple((origin, step, count_for(shape[2 - a], step)) for a in range(3))


def garbage_padded(mask, seed):
    """The bit mask of a bool array with random bits in the padding of every row's last word."""
    nz, ny, nx = mask.shape
    words = host.region_mask_pack(mask).reshape(nz, ny, -1).copy()
    if nx % 32:
        junk = np.random.default_rng(seed).integers(0, 1 << 32, size=(nz, ny), dtype=np.uint64).astype(np.uint32)
        words[:, :, -1] |= junk & np.uint32((0xFFFFFFFF << (nx % 32)) & 0xFFFFFFFF)
    return np.ascontiguousarray(words.reshape(-1))


# ------------------------------------------------------------------------------------------------ volumes
@pytest.mark.parametrize("shape", SMALL + TILED, ids=str)
def test_every_step_and_mode(hip_dev, shape):
    """The same step on the three axes, from the origin: 65536 is the copy, 65535 and 65537 drift by one source voxel over 65536."""
    vol = fr.random_volume(shape, 51)
    with Rs(hip_dev) as r:
        d_vol = r.put(vol)
        for step in STEPS:
            grid = uniform_grid(shape, step)
            for mode in rr.MODES:
                what = f"{shape} step {step} {MODE_NAMES[mode]}"
                same(r.volume(d_vol, shape, grid, mode, what), rr.volume_resample(vol, grid, mode), what)


@pytest.mark.parametrize("shape", SMALL[2:] + TILED[:2], ids=str)
def test_value_cases_from_host_and_device_sources(hip_dev, shape):
    grid = ((-30000, 43691, count_for(shape[2], 43691) + 2), (12345, 98304, count_for(shape[1], 98304)), (0, 131072, count_for(shape[0], 131072)))
    cases = [("random", fr.random_volume(shape, 52)), ("all 65535", np.full(shape, 65535, dtype=np.uint16)), ("all 0", np.zeros(shape, dtype=np.uint16)),
             ("extremes", fr.extremes_volume(shape, 53))]
    with Rs(hip_dev) as r:
        for name, vol in cases:
            d_vol = r.put(vol)
            for mode in rr.MODES:
                want = rr.volume_resample(vol, grid, mode)
                same(r.volume(d_vol, shape, grid, mode, name), want, f"{shape} {name} {MODE_NAMES[mode]} device source")
                same(r.volume(vol, shape, grid, mode, name), want, f"{shape} {name} {MODE_NAMES[mode]} host source")


def test_the_step_limits(hip_dev):
    with Rs(hip_dev) as r:
        shape = (1, 1, 3)
        vol = fr.random_volume(shape, 54)
        grid = ((0, 1024, 192), (0, 1024, 64), (0, 65536, 1))         # 192 outputs from 3
        for mode in rr.MODES:
            same(r.volume(vol, shape, grid, mode, "1024"), rr.volume_resample(vol, grid, mode), f"step 1024 {MODE_NAMES[mode]}")
        shape = TILED[2]
        vol = fr.random_volume(shape, 55)
        grid = ((0, 4194304, 8), (-65536, 4194304, 1), (0, 4194304, 1))  # 64 voxels a cell: 8 cells of 515, the last runs past the face
        for mode in rr.MODES:
            same(r.volume(vol, shape, grid, mode, "4194304"), rr.volume_resample(vol, grid, mode), f"step 4194304 {MODE_NAMES[mode]}")


MIXED = {
    "x crops, y and z resample": ((3 << 16, 65536, 50), (0, 43691, 20), (20000, 98304, 3)),
    "x resamples, y and z crop": ((-5000, 98304, 40), (2 << 16, 65536, 6), (1 << 16, 65536, 3)),
    "only y resamples": ((1 << 16, 65536, 62), (0, 32768, 34), (0, 65536, 5)),
    "only z resamples": ((0, 65536, 63), (0, 65536, 17), (-70000, 43691, 11)),
    "x and z": ((77, 65537, 60), (4 << 16, 65536, 9), (0, 131072, 3)),
    "a negative origin and one past the far face": ((-(3 << 16) - 17, 65536, 70), (-200000, 50000, 40), ((3 << 16) + 9, 43691, 9)),
    "crops that stick out": ((-(2 << 16), 65536, 70), (10 << 16, 65536, 12), (-(1 << 16), 65536, 7)),
    "fractional origins at step 1": ((1, 65536, 63), (65535, 65536, 17), (32768, 65536, 5)),
}


@pytest.mark.parametrize("name", list(MIXED))
def test_mixed_axes_and_origins(hip_dev, name):
    shape, grid = TILED[1], MIXED[name]
    vol = fr.random_volume(shape, 56)
    with Rs(hip_dev) as r:
        d_vol = r.put(vol)
        for mode in rr.MODES:
            same(r.volume(d_vol, shape, grid, mode, name), rr.volume_resample(vol, grid, mode), f"{name} {MODE_NAMES[mode]}")


@pytest.mark.parametrize("offset", [1, 31, 32, 33])
def test_crop_offsets_in_x(hip_dev, offset):
    shape = TILED[0]
    vol = fr.random_volume(shape, 57)
    box = ((offset, 2, 3), (offset + 90, 7, 8))
    got, g = hip_dev.volume_crop(vol, box)
    assert g.as_tuples() == rr.grid_box(shape[::-1], *box)
    same(got, np.ascontiguousarray(vol[3:9, 2:8, offset:offset + 91]), f"crop at x {offset}")
    with Rs(hip_dev) as r:
        for mode in rr.MODES:                             # a crop is exact under every mode
            same(r.volume(vol, shape, g, mode, "crop"), got, f"crop at x {offset} {MODE_NAMES[mode]}")


def test_the_head(hip_dev):
    clean, _ = fr.heads()
    iso, _ = host.resample_grid_spacing(HEAD, (0.9, 0.9, 1.5), 0.9)
    grids = {"finer": uniform_grid(HEAD, 43691), "coarser": uniform_grid(HEAD, 98304), "half": uniform_grid(HEAD, 131072), "isotropic": iso.as_tuples()}
    assert grids["isotropic"] == rr.grid_spacing(HEAD[::-1], (0.9, 0.9, 1.5), (0.9, 0.9, 0.9))[0] and grids["isotropic"][0] == (0, 65536, 48)
    with Rs(hip_dev) as r:
        d_vol = r.put(clean)
        for name, grid in grids.items():
            for mode in rr.MODES:
                same(r.volume(d_vol, HEAD, grid, mode, name), rr.volume_resample(clean, grid, mode), f"head {name} {MODE_NAMES[mode]}")
    same(hip_dev.volume_resample(clean, grids["half"], abi.RESAMPLE_AREA), rr.volume_resample(clean, grids["half"], rr.AREA), "Device.volume_resample")


def test_out_ptr_the_timer_and_a_refusal_on_a_live_device(hip_dev):
    shape = TILED[1]
    vol = fr.random_volume(shape, 58)
    grid = uniform_grid(shape, 98304)
    g = host.resample_grid(grid)
    n = int(np.prod(g.shape))
    with Rs(hip_dev) as r:
        d_vol, out = r.put(vol), r.raw(2 * n + GUARD)
        assert hip_dev.volume_resample(d_vol, grid, abi.RESAMPLE_LINEAR, shape=shape, out_ptr=out) == out
        same(r.fetch(out, g.shape, np.uint16, "out_ptr"), rr.volume_resample(vol, grid, rr.LINEAR), "out_ptr")
        assert 0.0 <= hip_dev.volume_resample_last_ms() < 1000.0
        fresh = r.raw(2 * n + GUARD)
        dims = (C.c_int32 * 3)(*shape[::-1])
        bad = host.resample_grid(((0, 1000, 4),) * 3)
        for rc in (r.lib.svr_volume_resample(C.c_void_p(d_vol), dims, 1, C.byref(g), 9, C.c_void_p(fresh)),
                   r.lib.svr_volume_resample(C.c_void_p(d_vol), dims, 1, C.byref(bad), 0, C.c_void_p(fresh)),
                   r.lib.svr_volume_resample(C.c_void_p(d_vol), dims, 1, C.byref(g), 0, C.c_void_p(d_vol + 2))):
            assert rc == -3
            r.lib.svr_clear_error()
        assert (hip_dev.to_host(fresh, (2 * n + GUARD,), np.uint8) == PATTERN).all()
        same(hip_dev.to_host(d_vol, shape, np.uint16), vol, "the source after the refusals")


# ------------------------------------------------------------------------------------------------ masks
def mask_grids(nx):
    """Crops (the funnel form where the x range lies inside the source, else the general form) and resampling grids for an nx x 5 x 4 mask;
    the output widths end mid-word except where they are 32 or 64."""
    grids = {"identity": ((0, 65536, nx), (0, 65536, 5), (0, 65536, 4)),
             "y and z clamp": ((0, 65536, nx), (-(1 << 16), 65536, 8), (2 << 16, 65536, 4)),
             "x sticks out": ((-(3 << 16), 65536, nx + 5), (1 << 16, 65536, 3), (0, 65536, 4)),
             "finer": ((-20000, 32768, 2 * nx + 3), (0, 43691, 7), (0, 65536, 4)),
             "coarser": ((0, 98304, count_for(nx, 98304)), (10000, 65537, 5), (0, 131072, 2))}
    for off in (1, 31, 32, 33):
        for width in (1, 32, 33, 64, nx - off):
            if 0 < width <= nx - off:
                grids[f"crop {off} + {width}"] = ((off << 16, 65536, width), (1 << 16, 65536, 3), (1 << 16, 65536, 2))
    return grids


@pytest.mark.parametrize("nx", [1, 31, 32, 33, 64, 65, 131])
def test_masks(hip_dev, nx):
    shape = (4, 5, nx)
    mask = np.random.default_rng(60 + nx).integers(0, 2, size=shape).astype(bool)
    with Rs(hip_dev) as r:
        d_mask = r.put(garbage_padded(mask, nx))
        for name, grid in mask_grids(nx).items():
            want = rr.nearest_any(mask, grid)
            assert np.array_equal(want, rr.volume_resample(mask.astype(np.uint16), grid, rr.NEAREST) != 0)
            same(r.mask_words(d_mask, shape, grid, name), host.region_mask_pack(want), f"nx {nx} {name} (the raw words: the padding is 0)")
    grid = mask_grids(nx)["finer"]
    assert np.array_equal(hip_dev.region_resample(mask, grid), rr.nearest_any(mask, grid))


@pytest.mark.parametrize("op", [rr.PASTE_REPLACE, rr.MASK_OR, rr.MASK_ANDNOT])
def test_paste(hip_dev, op):
    rng = np.random.default_rng(70)
    full_shape = (5, 6, 131)
    full = rng.integers(0, 2, size=full_shape).astype(bool)
    with Rs(hip_dev) as r:
        for (sx, sy, sz), off in [((37, 3, 2), (30, 2, 1)), ((1, 1, 1), (130, 5, 4)), ((32, 6, 5), (32, 0, 0)), ((33, 2, 2), (31, 1, 3)), ((131, 6, 5), (0, 0, 0)),
                                  ((5, 2, 2), (3, 1, 1)), ((70, 1, 1), (61, 0, 4)), ((64, 2, 1), (64, 4, 2))]:
            sub = rng.integers(0, 2, size=(sz, sy, sx)).astype(bool)
            d_sub = r.put(garbage_padded(sub, sx))
            words = host.region_mask_words(full_shape)
            d_full = r.raw(4 * words + GUARD)
            hip_dev.to_device(d_full, host.region_mask_pack(full))
            r.ok(r.lib.svr_region_paste(C.c_void_p(d_sub), (C.c_int32 * 3)(sx, sy, sz), C.c_void_p(d_full), (C.c_int32 * 3)(*full_shape[::-1]),
                                        (C.c_int32 * 3)(*off), op))
            what = f"op {op}: {sx} x {sy} x {sz} at {off}"
            want = rr.paste(full, sub, off, op)
            outside = np.ones(full_shape, bool)
            outside[off[2]:off[2] + sz, off[1]:off[1] + sy, off[0]:off[0] + sx] = False
            assert np.array_equal(want[outside], full[outside])
            same(r.fetch(d_full, (words,), np.uint32, what), host.region_mask_pack(want), what)
            assert np.array_equal(hip_dev.region_paste(sub, full, off, op), want)


def test_labels_of_the_head(hip_dev):
    clean, _ = fr.heads()
    labels, k = hip_dev.region_label(fr.window(clean), 6)
    assert k >= 1 and labels.dtype == np.uint32
    box = ((5, 7, 9), (40, 41, 38))
    grids = {"crop": rr.grid_box(HEAD[::-1], *box), "finer": uniform_grid(HEAD, 43691), "coarser": ((-100000, 98304, 35), (0, 65536, 48), (7, 131072, 24))}
    with Rs(hip_dev) as r:
        d_labels = r.put(labels)
        for name, grid in grids.items():
            g = host.resample_grid(grid)
            out = r.raw(4 * int(np.prod(g.shape)) + GUARD)
            r.ok(r.lib.svr_region_label_resample(C.c_void_p(d_labels), (C.c_int32 * 3)(*HEAD[::-1]), C.byref(g), C.c_void_p(out)))
            same(r.fetch(out, g.shape, np.uint32, name), rr.nearest_any(labels, grid), f"labels {name}")
    same(hip_dev.region_label_resample(labels, grids["crop"]), np.ascontiguousarray(labels[9:39, 7:42, 5:41]), "labels cropped")


@pytest.mark.parametrize("value", [1, 255])
def test_expand(hip_dev, value):
    with Rs(hip_dev) as r:
        for shape in [(1, 1, 1), (3, 1, 33), (5, 17, 63), (2, 3, 515)]:
            mask = np.random.default_rng(80).integers(0, 2, size=shape).astype(bool)
            d_mask, out = r.put(garbage_padded(mask, 81)), r.raw(int(np.prod(shape)) + GUARD)
            r.ok(r.lib.svr_region_mask_expand(C.c_void_p(d_mask), (C.c_int32 * 3)(*shape[::-1]), value, C.c_void_p(out)))
            same(r.fetch(out, shape, np.uint8, "expand"), rr.expand(mask, value), f"expand {shape} value {value}")
    assert np.array_equal(hip_dev.region_mask_expand(mask, value), rr.expand(mask, value))


# ------------------------------------------------------------------------------------------------ the chain
def test_crop_dilate_paste_equals_the_full_grid(hip_dev):
    """Threshold the head, take the region's box with a margin, crop volume and mask, dilate on the crop, paste back: the same as
    dilating on the full grid, inside the box.  The margin of 2 keeps the one-step dilation off the crop's faces wherever the crop's face
    is not the volume's own."""
    clean, _ = fr.heads()
    nz, ny, nx = HEAD
    mask = hip_dev.region_threshold(clean, *fr.BONE)
    assert np.array_equal(mask, fr.window(clean))
    st = hip_dev.region_stats_of(clean, mask)
    margin = 2
    box = (tuple(st.bbox_min[a] - margin for a in range(3)), tuple(st.bbox_max[a] + margin for a in range(3)))
    sub_vol, g = hip_dev.volume_crop(clean, box)
    (x0, y0, z0), (cx, cy, cz) = [m[0] >> 16 for m in g.as_tuples()], [m[2] for m in g.as_tuples()]
    assert (cx, cy, cz) != (nx, ny, nz), "the crop must be smaller than the volume"
    inside = (slice(z0, z0 + cz), slice(y0, y0 + cy), slice(x0, x0 + cx))
    same(sub_vol, np.ascontiguousarray(clean[inside]), "the cropped volume")
    sub_mask = hip_dev.region_resample(mask, g)
    assert np.array_equal(sub_mask, mask[inside]) and np.array_equal(sub_mask, hip_dev.region_threshold(sub_vol, *fr.BONE))
    grown = hip_dev.region_morph(sub_mask, abi.MORPH_DILATE, 6, 1)
    # the dilation does not reach a face of the crop that lies inside the volume
    for axis, (lo, n_crop, n_full) in enumerate([(z0, cz, nz), (y0, cy, ny), (x0, cx, nx)]):
        if lo > 0:
            assert not np.take(grown, 0, axis=axis).any()
        if lo + n_crop < n_full:
            assert not np.take(grown, n_crop - 1, axis=axis).any()
    pasted = hip_dev.region_paste(grown, mask, (x0, y0, z0), abi.PASTE_REPLACE)
    p = np.pad(mask, 1)
    full = p[1:-1, 1:-1, 1:-1] | p[:-2, 1:-1, 1:-1] | p[2:, 1:-1, 1:-1] | p[1:-1, :-2, 1:-1] | p[1:-1, 2:, 1:-1] | p[1:-1, 1:-1, :-2] | p[1:-1, 1:-1, 2:]
    assert np.array_equal(pasted[inside], full[inside])
    assert np.array_equal(pasted, full)                   # the box holds the whole dilated region
