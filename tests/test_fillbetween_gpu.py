"""svr_region_slice_counts, svr_region_slice_distance and svr_region_fill_between on the GPU against the numpy reference
(tests/fillbetween_ref.py), word for word: every count, every map value and every mask word, padding included (output buffers hold ones
before the call, input masks carry garbage in their padding); then the 48^3 head with three slices of four taken away."""
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import fillbetween_ref as fr
from tests import morph_ref as mr
from tests.test_scissor_gpu import Scratch

pytestmark = pytest.mark.gpu
SOURCE = (Path(__file__).resolve().parents[1] / "sunvolumerender_amd" / "csrc" / "svr_fillbetween.hip").read_text()
PLANAR_CHUNK_VOXELS = 1 << int(re.search(r"constexpr size_t PLANAR_CHUNK_VOXELS = \(size_t\)1 << (\d+);", SOURCE).group(1))

# (nx, ny, nz): flat ones, rows of less than, exactly and more than one and two mask words, more than one block of lanes along x, and
# more columns (300 x 3 = 900 for axis z) than one column block of 256 covers
SHAPES = [(1, 1, 1), (5, 1, 8), (1, 6, 9), (31, 5, 7), (32, 3, 6), (33, 7, 5), (65, 4, 9), (130, 9, 12), (300, 3, 4)]
WEIGHTS = (None, (4, 1, 9))


def key_sets(n):
    """explicit keys on an axis of n slices: from the first slice to the last with steps 1, 2, 3, 7 (no gap, then gaps of every kind the
    axis has room for), the same off both ends, and two keys as far apart as the axis lets them be"""
    def walk(start, stop, steps):
        ks, k, i = [], start, 0
        while k <= stop:
            ks.append(k)
            k, i = k + steps[i % len(steps)], i + 1
        return ks
    on = walk(0, n - 1, (1, 2, 3, 7))
    if on[-1] != n - 1:
        on.append(n - 1)
    sets = [on, walk(1, n - 2, (7, 3, 2, 1)), [0, n - 1] if n > 1 else [0], []]
    return [ks for i, ks in enumerate(sets) if ks not in sets[:i]]


def keyed_mask(rng, shape, axis, keys, density, between=0.0):
    """random voxels on the key slices at `density`, and at `between` on every other slice"""
    m = rng.random(shape) < between
    p = fr.planes(m, axis)
    for k in keys:
        p[k] = rng.random(p[k].shape) < density
    return m


def fill_on_gpu(dev, mask, axis, keys, weights=None, keep=False, in_place=False, gap_by_gap=False):
    """(the words of the result, info); the input has garbage in its padding, the output buffer held ones"""
    shape = mask.shape
    with Scratch(dev) as s:
        d_in = s.put(mr.dirty_padding(host.region_mask_pack(mask), shape))
        d_out = d_in if in_place else s.new(4 * host.region_mask_words(shape))
        got, info = dev.region_fill_between(d_in, axis, keys, weights, keep, shape=shape, out_ptr=d_out, gap_by_gap=gap_by_gap)
        words = dev.to_host(d_out, (host.region_mask_words(shape),), np.uint32)
    assert np.array_equal(host.region_mask_pack(got), words)
    return words, info


def check_fill(dev, mask, axis, keys, weights=None, keep=False, **how):
    want, winfo = fr.fill_between(mask, axis, keys, weights, keep)
    words, info = fill_on_gpu(dev, mask, axis, keys, weights, keep, **how)
    what = (mask.shape, axis, keys, weights, keep, how)
    assert np.array_equal(words, host.region_mask_pack(want)), what
    for name, value in winfo.items():
        assert getattr(info, name) == value, (name, what)
    expected_launches = 0 if winfo["gaps"] == 0 else (winfo["gaps"] if how.get("gap_by_gap") else 1)
    assert info.launches == expected_launches, what
    return want, info


@pytest.mark.parametrize("shape_xyz", SHAPES)
def test_counts_and_planar_maps(hip_dev, shape_xyz):
    dev, shape = hip_dev, shape_xyz[::-1]
    rng = np.random.default_rng(sum(shape_xyz))
    for axis in range(3):
        n = shape[2 - axis]
        for density in (0.05, 0.5, 0.95):
            m = rng.random(shape) < density
            if n > 2:
                fr.planes(m, axis)[1] = density > 0.5                # a slice with no voxel of the other kind: SVR_DIST_NONE everywhere
            with Scratch(dev) as s:
                d_in = s.put(mr.dirty_padding(host.region_mask_pack(m), shape))
                assert np.array_equal(dev.region_slice_counts(d_in, axis, shape=shape), fr.slice_counts(m, axis)), (shape, axis, density)
                for w in WEIGHTS:
                    plane = m.size // n
                    d_out = s.new(4 * n * plane)
                    dev.region_slice_distance(d_in, axis, w, shape=shape, out_ptr=d_out)
                    got = dev.to_host(d_out, (n,) + fr.planes(m, axis).shape[1:], np.uint32)
                    want = fr.slice_distance(m, axis, w)
                    assert np.array_equal(got, want), (shape, axis, density, w)
            # a list: descending, with repeats
            ks = list(range(n - 1, -1, -1))[:5] + [0, n - 1, 0]
            assert np.array_equal(dev.region_slice_distance(m, axis, (4, 1, 9), slices=ks), want[ks]), (shape, axis, ks)
    assert dev.region_fill_between_last_ms() >= 0.0


def test_planar_maps_near_the_end_of_32_bits(hip_dev):
    """2000 x 2 x 2 under weights (900, 1, 1): 900 * 1999^2 = 3 596 400 900 is within a fifth of 2^32, so the separators of the column
    pass and the fill's products need their 64 bits"""
    dev, w = hip_dev, (900, 1, 1)
    m = np.zeros((2, 2, 2000), bool)
    m[0, 0, 0] = m[1, 1, 1999] = True                                 # slice z = 1 holds one voxel, at the far end of the other row
    m[0, 1, :] = True
    m[0, 1, 1234] = False
    for axis in range(3):
        got, want = dev.region_slice_distance(m, axis, w), fr.slice_distance(m, axis, w)
        assert np.array_equal(got, want), axis
    assert int(want.max()) == 900 * 1999 ** 2 + 1                     # (axis z, the last of the loop)
    long = np.zeros((9, 1, 2000), bool)                               # keys 0 and 8: (n - t)^2 A reaches 49 * 3.6e9
    long[0, 0, :3] = True
    long[8, 0, 1990:] = True
    long[8, 0, 1] = True
    want, _ = check_fill(dev, long, 2, [0, 8], w)
    assert want[1:8].any()


def test_planar_maps_past_one_chunk_of_slices(hip_dev):
    """The slices go through the passes PLANAR_CHUNK_VOXELS voxels at a time: 17 slices of 2048 x 2048 are one chunk of 16 and one of 1.
    Slices of both chunks against svr_region_distance of the slice as a volume of its own (held against numpy in tests/test_distance_gpu.py):
    for nz = 1 its TO_UNSET map on the set voxels and its TO_SET map on the others are the planar map."""
    dev, n, nz = hip_dev, 2048, 17
    plane = n * n
    assert PLANAR_CHUNK_VOXELS // plane == 16 and nz * plane > PLANAR_CHUNK_VOXELS
    rng = np.random.default_rng(11)
    m = np.zeros((nz, n, n), bool)
    for k in (0, 15, 16):
        m[k] = rng.random((n, n)) < 0.001
        m[k, 100 * (k + 1):100 * (k + 1) + 300, 50:900] = True
    with Scratch(dev) as s:
        d_out = s.new(4 * nz * plane, fill=0)
        dev.region_slice_distance(m, 2, (4, 1, 9), out_ptr=d_out)
        for k in (0, 15, 16):
            got = dev.to_host(d_out + 4 * k * plane, (n, n), np.uint32)
            one = m[k][None]
            want = np.where(one, dev.region_distance(one, weights=(4, 1, 9), target=abi.DIST_TO_UNSET), dev.region_distance(one, weights=(4, 1, 9)))[0]
            assert np.array_equal(got, want), k
        assert (dev.to_host(d_out + 4 * plane, (n, n), np.uint32) == fr.NONE).all()          # an empty slice


@pytest.mark.parametrize("shape_xyz", SHAPES)
def test_fill_between(hip_dev, shape_xyz):
    dev, shape = hip_dev, shape_xyz[::-1]
    rng = np.random.default_rng(7 + sum(shape_xyz))
    for axis in range(3):
        n = shape[2 - axis]
        sets = key_sets(n)
        for i, keys in enumerate(sets):
            density = (0.05, 0.5, 0.95)[i % 3]
            m = keyed_mask(rng, shape, axis, keys, density)
            check_fill(dev, m, axis, None, WEIGHTS[i % 2])                                    # automatic keys: the non-empty slices
            check_fill(dev, m, axis, keys, WEIGHTS[(i + 1) % 2])                              # the same, named (some may be empty at 5 %)
            dirty = keyed_mask(rng, shape, axis, keys, 0.5, between=0.3)                      # set voxels between explicit keys
            check_fill(dev, dirty, axis, keys)                                                # ... are replaced
            check_fill(dev, dirty, axis, keys, (4, 1, 9), keep=True)                          # ... or kept
            check_fill(dev, dirty, axis, keys, keep=True, in_place=True)
            check_fill(dev, dirty, axis, keys, (4, 1, 9), gap_by_gap=True, in_place=(i % 2 == 0))   # two maps at a time, one launch per gap
        # an all-set key next to an all-unset explicit key: the tie at t = n / 2 goes to unset
        if n >= 3:
            m = np.zeros(shape, bool)
            fr.planes(m, axis)[0] = True
            want, info = check_fill(dev, m, axis, [0, n - 1])
            assert info.gaps == 1 and [bool(p.all()) for p in fr.planes(want, axis)] == [2 * t < n - 1 for t in range(n)]
            check_fill(dev, ~m, axis, [0, n - 1], (4, 1, 9))
    assert dev.region_fill_between_last_ms() >= 0.0


def test_fewer_than_two_keys_copy_the_mask(hip_dev):
    dev = hip_dev
    rng = np.random.default_rng(3)
    m = rng.random((6, 5, 40)) < 0.4
    for axis in range(3):
        for keys in ([], [2], [1, 2, 3]):                                # none, one, three without a gap
            want, info = check_fill(dev, m, axis, keys)
            assert np.array_equal(want, m) and info.launches == 0 and info.voxels_out == info.voxels_in == m.sum()


def test_fill_between_on_the_head(hip_dev):
    """The bone window of the 48^3 head with every axial slice that is no multiple of 4 cleared, filled again: equal to the reference,
    and nearer to the full mask than the sparse one is (Dice by svr_region_overlap; the two values are properties of the reference,
    0.4016 and 0.9765)."""
    dev = hip_dev
    vox = scenes.make_scene("tiny_head").vox
    full = vox >= int(0.35 * 65535)
    sparse = full.copy()
    sparse[np.arange(full.shape[0]) % 4 != 0] = False
    want, winfo = fr.fill_between(sparse, 2)
    assert fr.dice(want, full) > fr.dice(sparse, full)                   # the reference first, on the CPU
    got, info = dev.region_fill_between(sparse, 2)
    assert np.array_equal(got, want)
    assert (info.keys, info.gaps, info.filled_slices, info.voxels_out) == (winfo["keys"], winfo["gaps"], winfo["filled_slices"], winfo["voxels_out"])

    def dice(a):
        both, a_only, b_only, _ = dev.region_overlap(a, full)
        return 2.0 * both / (2 * both + a_only + b_only)
    assert dice(got) == pytest.approx(fr.dice(want, full)) and dice(got) > dice(sparse)
