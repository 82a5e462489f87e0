"""svr_region_box_count, svr_region_smooth and svr_region_label_smooth on the GPU against the numpy reference (tests/smooth_ref.py),
bit for bit: every count, every mask word and every label, padding included (output buffers hold ones before the call, input masks carry
garbage in their padding).  Random masks of density 0.5 -- where the most voxels sit next to the threshold -- and a ball with salt
noise, on the smallest shapes at which each mechanism can go wrong."""
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import morph_ref as mr
from tests import smooth_ref as sm
from tests.test_scissor_gpu import Scratch

pytestmark = pytest.mark.gpu
SOURCE = (Path(__file__).resolve().parents[1] / "sunvolumerender_amd" / "csrc" / "svr_smooth.hip").read_text()
TW, TY, TZ = (int(t) for t in re.search(r"constexpr int TW = (\d+), TY = (\d+), TZ = (\d+);", SOURCE).groups())   # a tile: words, rows, slices

# (nx, ny, nz), radii.  70 x 21 x 19: three words a row with a partial last word, windows across two word boundaries, halos wider than a
# tile in y and z; 33 x 5 x 1: one padding-heavy word, a flat volume, windows clamped on both sides at once; 3 x 1 x 4: nx below the
# radius; one pass alone on exact word multiples; (0, 0, 0): a copy
CASES = [((70, 21, 19), (7, 2, 3)), ((70, 21, 19), (8, 8, 8)), ((33, 5, 1), (8, 8, 8)), ((3, 1, 4), (7, 0, 1)), ((40, 7, 6), (3, 3, 3)),
         ((9, 9, 9), (1, 1, 1)), ((64, 16, 16), (1, 0, 0)), ((64, 16, 16), (0, 1, 0)), ((64, 16, 16), (0, 0, 1)), ((40, 7, 6), (0, 0, 0))]


def masks(shape_xyz, seed=0):
    shape = shape_xyz[::-1]
    return [np.random.default_rng(seed + sum(shape_xyz)).random(shape) < 0.5, sm.ball_with_salt(shape, seed)]


def smooth_words(dev, mask, op, radii, iterations=1):
    """(the words of the result in the caller's buffer, changed); the input has garbage in its padding, the output buffer held ones"""
    shape = mask.shape
    with Scratch(dev) as s:
        d_in, d_out = s.put(mr.dirty_padding(host.region_mask_pack(mask), shape)), s.new(4 * host.region_mask_words(shape))
        got, changed = dev.region_smooth(d_in, op, radii, iterations, shape=shape, out_ptr=d_out)
        words = dev.to_host(d_out, (host.region_mask_words(shape),), np.uint32)
    assert np.array_equal(host.region_mask_pack(got), words)
    return words, changed


@pytest.mark.parametrize("shape_xyz, radii", CASES)
def test_count_and_majority(hip_dev, shape_xyz, radii):
    dev = hip_dev
    for m in masks(shape_xyz):
        shape = m.shape
        want = sm.box_count(m, radii)
        with Scratch(dev) as s:
            d_in, d_out = s.put(mr.dirty_padding(host.region_mask_pack(m), shape)), s.new(2 * m.size)
            assert dev.region_box_count(d_in, radii, shape=shape, out_ptr=d_out) == d_out
            assert np.array_equal(dev.to_host(d_out, shape, np.uint16), want), (shape_xyz, radii)
        assert np.array_equal(dev.region_box_count(m, radii), want)                       # a host mask, the library's own buffers
        assert np.array_equal(dev.region_box_count(m, radii, density=True), want.astype(np.uint32) * 65535 // sm.box_size(radii))
        out, wchanged = sm.smooth(m, sm.MAJORITY, radii)
        words, changed = smooth_words(dev, m, abi.SMOOTH_MAJORITY, radii)
        assert np.array_equal(words, host.region_mask_pack(out)) and changed == wchanged, (shape_xyz, radii)
        got, changed = dev.region_smooth(m, abi.SMOOTH_MAJORITY, radii)
        assert np.array_equal(got, out) and changed == wchanged
        if radii == (0, 0, 0):
            assert np.array_equal(out, m) and changed == 0 and (want == m).all()
    assert dev.region_smooth_last_ms() >= 0.0


@pytest.mark.parametrize("shape_xyz, radii", [CASES[0], CASES[2], CASES[3], CASES[5]])
@pytest.mark.parametrize("iterations", [2, 16])
def test_iterations(hip_dev, shape_xyz, radii, iterations):
    dev, m = hip_dev, masks(shape_xyz, 1)[1]
    for op in (abi.SMOOTH_MAJORITY, abi.SMOOTH_BINOMIAL):
        out, wchanged = sm.smooth(m, op, radii, iterations)
        words, changed = smooth_words(dev, m, op, radii, iterations)
        assert np.array_equal(words, host.region_mask_pack(out)) and changed == wchanged, (op, shape_xyz, radii, iterations)


@pytest.mark.parametrize("r", [1, 2, 4])
def test_majority_is_the_thresholded_count_and_the_extremes_are_morphology(hip_dev, r):
    """MAJORITY against svr_region_box_count through svr_region_threshold; count >= 1 and count == N against svr_region_morph DILATE /
    ERODE with element 26, all on the GPU"""
    dev, radii, n = hip_dev, (r, r, r), (2 * r + 1) ** 3
    for m in masks((70, 21, 19)) + [mr.two_balls()]:
        shape = m.shape
        with Scratch(dev) as s:
            d_in, d_count = s.put(host.region_mask_pack(m)), s.new(2 * m.size)
            dev.region_box_count(d_in, radii, shape=shape, out_ptr=d_count)
            half = dev.region_threshold(d_count, n // 2 + 1, 65535, shape=shape)
            assert np.array_equal(dev.region_smooth(d_in, abi.SMOOTH_MAJORITY, radii, shape=shape)[0], half)
            assert np.array_equal(dev.region_threshold(d_count, 1, 65535, shape=shape), dev.region_morph(d_in, abi.MORPH_DILATE, 26, r, shape=shape))
            assert np.array_equal(dev.region_threshold(d_count, n, 65535, shape=shape), dev.region_morph(d_in, abi.MORPH_ERODE, 26, r, shape=shape))


@pytest.mark.parametrize("shape_xyz, radii", [((70, 21, 19), (1, 1, 1)), ((70, 21, 19), (8, 0, 3)), ((33, 5, 1), (0, 0, 0)), ((40, 7, 6), (3, 3, 3))])
def test_binomial(hip_dev, shape_xyz, radii):
    dev = hip_dev
    for m in masks(shape_xyz, 2):
        shape = m.shape
        out, wchanged = sm.smooth(m, sm.BINOMIAL, radii)
        words, changed = smooth_words(dev, m, abi.SMOOTH_BINOMIAL, radii)
        assert np.array_equal(words, host.region_mask_pack(out)) and changed == wchanged, (shape_xyz, radii)
        # the composition a user has without the call: paint 65535 into the region, smooth, take the upper half
        e = dev.region_apply(np.full(shape, 65535, np.uint16), m, abi.REGION_KEEP, 0)
        assert np.array_equal(dev.region_threshold(dev.volume_smooth(e, radii), 32768, 65535), out)


def label_maps(shape, count, seed):
    """random labels 0 .. count; the same with the lower half of the rows one label (tiles whose whole halo holds that label are copied,
    next to computed ones: test_mode_where_copied_and_computed_tiles_meet counts them); one label only; blocks of one label each with
    noise between 0 and 1"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    values = np.arange(count + 1) if count < 8 else np.array([0, 1, 2, 37, 128, 200, 254, 255])
    a = values[rng.integers(0, len(values), shape)].astype(np.uint32)
    b = a.copy()
    b[:, :ny // 2, :] = count
    blobs = (values[(np.add.outer(np.add.outer(np.arange(nz) // 5, np.arange(ny) // 6), np.arange(nx) // 9)) % len(values)]).astype(np.uint32)
    return [a, b, np.full(shape, count, np.uint32), blobs ^ ((rng.random(shape) < 0.1) & (blobs < 2)).astype(np.uint32)]


@pytest.mark.parametrize("count", [1, 3, 4, 255])
@pytest.mark.parametrize("shape_xyz, radii", CASES)
def test_mode(hip_dev, shape_xyz, radii, count):
    dev, shape = hip_dev, shape_xyz[::-1]
    for k, lab in enumerate(label_maps(shape, count, count + sum(shape_xyz))):
        want, wchanged = sm.label_smooth(lab, count, radii)
        with Scratch(dev) as s:
            d_out = s.new(4 * lab.size)
            got, changed = dev.region_label_smooth(lab, count, radii, out_ptr=d_out)
            assert got == d_out and np.array_equal(dev.to_host(d_out, shape, np.uint32), want) and changed == wchanged, (shape_xyz, radii, count, k)
        if count == 1:
            assert np.array_equal(want.astype(bool), dev.region_smooth(lab.astype(bool), abi.SMOOTH_MAJORITY, radii)[0])


def tile_kinds(lab, radii):
    """(copied, computed): the tiles of k_label_mode whose halo -- one word in x, ry rows, rz slices, cut to the volume -- holds one label
    only, and the others"""
    rx, ry, rz = radii
    nz, ny, nx = lab.shape
    copied = computed = 0
    for z0 in range(0, nz, TZ):
        for y0 in range(0, ny, TY):
            for w0 in range(0, (nx + 31) // 32, TW):
                halo = lab[max(z0 - rz, 0):z0 + TZ + rz, max(y0 - ry, 0):y0 + TY + ry, max(w0 - 1, 0) * 32:(w0 + TW + 1) * 32]
                one = halo.min() == halo.max()
                copied, computed = copied + one, computed + (not one)
    return int(copied), int(computed)


# (nx, ny, nz), radii, the axis that is cut (0 = x, 1 = y, 2 = z), the first index of the one-label part for which a tile's halo lies
# wholly inside it: with the part one row or slice smaller (along x: without the halo word, from x = 256) that tile's own voxels still hold
# one label, but its halo does not, and the windows of its outermost voxels reach the random labels
MEETING = [((70, 21, 19), (7, 2, 3), 1, 10), ((70, 21, 19), (7, 2, 3), 2, 11), ((300, 9, 3), (1, 1, 1), 0, 224), ((300, 9, 3), (8, 1, 1), 0, 224),
           ((40, 37, 6), (3, 8, 3), 1, 16), ((9, 9, 40), (1, 1, 8), 2, 16)]


@pytest.mark.parametrize("shape_xyz, radii, axis, edge", MEETING)
def test_mode_where_copied_and_computed_tiles_meet(hip_dev, shape_xyz, radii, axis, edge):
    """One label from `edge` to the end of an axis (or, for y and z, from the start up to `edge`), random labels elsewhere: the tiles
    whose halo lies in the one-label part are written without counting.  The same with the part cut back to the tile's own voxels: the
    tile at its border holds one label in its own voxels but not in its halo, and must count -- a halo scan that forgot the word in x,
    the ry rows or the rz slices would copy it and miss the labels that its outermost windows hold."""
    dev, shape = hip_dev, shape_xyz[::-1]
    rng = np.random.default_rng(sum(shape_xyz) + axis)
    for count in (3, 255):
        values = np.arange(count + 1) if count < 8 else np.array([0, 1, 2, 37, 128, 200, 254, 255])
        for shrink in (0, 1):
            lab = values[rng.integers(0, len(values), shape)].astype(np.uint32)
            part = [slice(None)] * 3
            part[2 - axis] = slice(32 * 2 * TW if shrink else edge, None) if axis == 0 else slice(0, edge - shrink)
            lab[tuple(part)] = count
            copied, computed = tile_kinds(lab, radii)
            assert computed > 0 and (copied > 0) == (shrink == 0), (copied, computed)
            if shrink:                                    # the border tile's own voxels hold one label; only its halo does not
                own = [slice(None)] * 3
                own[2 - axis] = slice(32 * 2 * TW, None) if axis == 0 else slice(0, (TY, TZ)[axis - 1])
                assert (lab[tuple(own)] == count).all()
            want, wchanged = sm.label_smooth(lab, count, radii)
            got, changed = dev.region_label_smooth(lab, count, radii)
            assert np.array_equal(got, want) and changed == wchanged, (shape_xyz, radii, axis, count, shrink)
            assert wchanged > 0


def test_mode_reads_a_value_above_count_as_background_and_iterates(hip_dev):
    dev = hip_dev
    rng = np.random.default_rng(9)
    lab = rng.integers(0, 7, (19, 21, 70)).astype(np.uint32)     # count 4: the values 5 and 6 are read as 0
    lab[3, 4, 5] = 0xFFFFFFFF
    for iterations in (1, 2, 16):
        want, wchanged = sm.label_smooth(lab, 4, (1, 2, 1), iterations)
        got, changed = dev.region_label_smooth(lab, 4, (1, 2, 1), iterations)
        assert np.array_equal(got, want) and changed == wchanged and got.max() <= 4, iterations


def test_mode_ties(hip_dev):
    """a checkerboard of 2 and 3 around a 1 at the centre: 13 : 13 : 1 gives the smaller label, and a voxel whose own label is among
    the most frequent keeps it"""
    dev = hip_dev
    z, y, x = np.mgrid[:3, :3, :3]
    lab = np.where((x + y + z) % 2 == 0, 2, 3).astype(np.uint32)
    lab[1, 1, 1] = 1
    board = np.pad(lab, 3, mode="edge")
    got, _ = dev.region_label_smooth(board, 3, (1, 1, 1))
    assert got[4, 4, 4] == 2 and np.array_equal(got, sm.label_smooth(board, 3, (1, 1, 1))[0])
    stripes = np.tile(np.array([1, 2], np.uint32), (4, 5, 20))    # every window along x is 1 : 2 or 2 : 1 but at the clamped ends
    for radii in ((1, 0, 0), (2, 1, 1)):
        assert np.array_equal(dev.region_label_smooth(stripes, 2, radii)[0], sm.label_smooth(stripes, 2, radii)[0])
