"""svr_volume_histogram and svr_region_label_histogram on the GPU against the numpy reference of tests/histogram_ref.py, bit for bit:
the shapes at which the flat 8-voxel chunks of the kernel straddle rows and mask words, every mask / window / shift / box path, both
sides of the kernel's LDS switches (read from the source), the contention cases (all-equal, two-valued, the head's 68 % zeros), a volume
of more chunks than one trip of the capped grid covers, the per-label table, and the consistency with svr_region_stats_of,
svr_region_threshold and svr_region_label_table."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import histogram_ref as hr
from tests import label_ref as lr
from tests import region_ref as rr

pytestmark = pytest.mark.gpu

SOURCE = (Path(__file__).resolve().parents[1] / "sunvolumerender_amd" / "csrc" / "svr_histogram.hip").read_text()
SHAPES = [(1, 1, 1), (1, 1, 33), (3, 5, 31), (2, 3, 65), (5, 4, 97), (4, 7, 130)]


def constant(name):
    m = re.search(rf"constexpr int {name} = (\d+);", SOURCE)
    assert m, name
    return int(m.group(1))


LDS_SMALL, LDS_LARGE = constant("HIST_LDS_BINS_SMALL"), constant("HIST_LDS_BINS_LARGE")
MAX_BLOCKS, THREADS = constant("HIST_MAX_BLOCKS"), constant("HIST_THREADS")
CHUNK = 8                                                                  # voxels of a lane's chunk when the arrays are aligned


def volume(shape, seed, top=65536):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, top, shape).astype(np.uint16)
    flat = v.reshape(-1)
    flat[rng.integers(0, flat.size)] = 0                                   # the extremes are present (a 1-voxel volume keeps the last)
    flat[rng.integers(0, flat.size)] = 65535
    return v


def dirty_mask_words(mask):
    """the bit mask of a bool array with every padding bit set"""
    words = host.region_mask_pack(mask).reshape(mask.shape[0], mask.shape[1], -1).copy()
    if mask.shape[2] % 32:
        words[:, :, -1] |= np.uint32((0xFFFFFFFF << (mask.shape[2] % 32)) & 0xFFFFFFFF)
    return words.reshape(-1)


@pytest.fixture(scope="module")
def head():
    return scenes.make_ct_head_volume(48)


@pytest.fixture(scope="module")
def head_hist(head):
    return hr.histogram(head)


# ---- shapes, sources, masks ----
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_from_host_and_device_with_every_mask(hip_dev, shape):
    v = volume(shape, sum(shape))
    nz, ny, nx = shape
    want = hr.histogram(v)
    assert want[0] >= 1 or v.size == 1
    assert np.array_equal(hip_dev.volume_histogram(v), want)
    n = v.size
    buf, odd = hip_dev.malloc(2 * n), hip_dev.malloc(2 * n + 16)
    mbuf = hip_dev.malloc(4 * host.region_mask_words(shape))
    try:
        hip_dev.to_device(buf, v)
        hip_dev.to_device(odd + 2, v)                                      # a source that is not 16-byte aligned: the one-voxel chunks
        assert np.array_equal(hip_dev.volume_histogram(buf, shape=shape), want)
        assert np.array_equal(hip_dev.volume_histogram(odd + 2, shape=shape), want)
        rng = np.random.default_rng(n)
        masks = {"random": rng.random(shape) < 0.4, "empty": np.zeros(shape, bool), "full": np.ones(shape, bool),
                 "one": np.zeros(shape, bool), "rows": np.zeros(shape, bool)}
        masks["one"][nz - 1, ny - 1, nx - 1] = True
        masks["rows"][:, ::2, :] = True
        for name, mask in masks.items():
            want_m = hr.histogram(v, mask, shift=4)
            assert int(want_m.sum()) == int(mask.sum())
            assert np.array_equal(hip_dev.volume_histogram(v, mask, shift=4), want_m), name
            hip_dev.to_device(mbuf, dirty_mask_words(mask))                # every padding bit set: ignored
            assert np.array_equal(hip_dev.volume_histogram(buf, mbuf, shift=4, shape=shape), want_m), name
            assert np.array_equal(hip_dev.volume_histogram(odd + 2, mbuf, shift=4, shape=shape), want_m), name
        assert not hip_dev.volume_histogram(v, masks["empty"]).any()       # the empty mask: all counts 0, not an error
    finally:
        for p in (buf, odd, mbuf):
            hip_dev.free(p)


@pytest.mark.parametrize("nx", [31, 33, 65])
def test_padding_bits_all_set_are_ignored(hip_dev, nx):
    shape = (3, 4, nx)
    v = volume(shape, nx)
    mask = np.zeros(shape, bool)                                           # an EMPTY mask whose padding bits are all 1: nothing counts
    mbuf = hip_dev.malloc(4 * host.region_mask_words(shape))
    try:
        hip_dev.to_device(mbuf, dirty_mask_words(mask))
        assert not hip_dev.volume_histogram(v, mbuf).any()
        mask[:, :, nx - 1] = True                                          # the last voxel of every row, next to the padding
        mask[1, 2, 0] = True
        hip_dev.to_device(mbuf, dirty_mask_words(mask))
        got = hip_dev.volume_histogram(v, mbuf)
        assert np.array_equal(got, hr.histogram(v, mask)) and int(got.sum()) == 3 * 4 + 1
    finally:
        hip_dev.free(mbuf)


# ---- window, shift, bins on both sides of the LDS switches ----
def test_window_and_shift(hip_dev):
    v = volume((5, 4, 97), 3)
    v[0, 0, :8] = (999, 1000, 1001, 50000, 50001, 49999, 1000, 50000)      # the window's ends and their neighbours
    for lo, hi in ((1000, 50000), (1000, 1000), (0, 0), (65535, 65535), (1, 65534), (30000, 30006)):
        for shift in (0, 3, 8, 15):
            got = hip_dev.volume_histogram(v, lo=lo, hi=hi, shift=shift)
            want = hr.histogram(v, lo=lo, hi=hi, shift=shift)
            assert len(got) == hr.bins(lo, hi, shift) and np.array_equal(got, want), (lo, hi, shift)
            assert int(got.sum()) == int(((v >= lo) & (v <= hi)).sum())   # voxels outside vanish: they are not clamped into the end bins
    small = volume((2, 3, 65), 4, top=1200)
    got = hip_dev.volume_histogram(small, lo=100, hi=1100, shift=3)        # 1001 values in 126 bins: the last bin holds one value
    assert len(got) == 126 and np.array_equal(got, hr.histogram(small, lo=100, hi=1100, shift=3))
    assert int(got[125]) == int((small == 1100).sum())


def test_bin_counts_on_both_sides_of_the_lds_switches(hip_dev):
    assert LDS_SMALL == 16384 and LDS_LARGE == 32768 and 2 * LDS_LARGE == 65536
    v = volume((6, 40, 130), 8)
    v.reshape(-1)[:12] = (16383, 16384, 16385, 32767, 32768, 32769, 65535, 65534, 0, 16384, 32768, 16383)
    tried = set()
    for bins in (LDS_SMALL - 1, LDS_SMALL, LDS_SMALL + 1, LDS_LARGE, LDS_LARGE + 1, 2 * LDS_LARGE - 1, 2 * LDS_LARGE):
        got = hip_dev.volume_histogram(v, hi=bins - 1)
        assert len(got) == bins and np.array_equal(got, hr.histogram(v, hi=bins - 1)), bins
        tried.add("small" if bins <= LDS_SMALL else "large" if bins <= LDS_LARGE else "two passes")
    assert tried == {"small", "large", "two passes"}
    # the same through a shifted window, with a mask, from the device
    mask = np.random.default_rng(1).random(v.shape) < 0.5
    for lo, hi, shift in ((1, 65535, 1), (0, 65535, 2), (3, 65535, 0)):
        assert np.array_equal(hip_dev.volume_histogram(v, mask, lo, hi, shift), hr.histogram(v, mask, lo, hi, shift))


# ---- boxes ----
def test_boxes(hip_dev):
    shape = (6, 7, 130)
    v = volume(shape, 11)
    mask = np.random.default_rng(2).random(shape) < 0.6
    boxes = [((3, 2, 1), (100, 5, 4)), ((64, 3, 2), (64, 3, 2)), ((129, 6, 5), (129, 6, 5)), ((0, 0, 0), (0, 0, 0)),
             ((-5, -5, -5), (500, 500, 500)), ((120, 0, 3), (1000, 2, 1000)), ((31, 0, 0), (32, 6, 5)), ((0, 0, 2), (129, 6, 2)),
             ((7, 1, 0), (8, 1, 5))]
    for box in boxes:
        for m in (None, mask):
            got = hip_dev.volume_histogram(v, m, shift=5, box=box)
            assert np.array_equal(got, hr.histogram(v, m, shift=5, box=box)), box
    one = hip_dev.volume_histogram(v, box=boxes[1])
    assert int(one.sum()) == 1 and one[v[2, 3, 64]] == 1
    flat = volume((5, 3, 64), 13)                                          # rows of whole mask words: the kernel's flat path and its way out
    fmask = np.random.default_rng(3).random(flat.shape) < 0.5
    for box in (None, ((0, 0, 1), (63, 2, 3)), ((0, 0, 4), (63, 2, 4)), ((0, 1, 0), (63, 2, 4)), ((1, 0, 0), (63, 2, 4)), ((0, 0, 0), (62, 2, 4))):
        for m in (None, fmask):
            assert np.array_equal(hip_dev.volume_histogram(flat, m, shift=6, box=box), hr.histogram(flat, m, shift=6, box=box)), box
    planes = volume((4, 3, 33), 14)                                        # slices that start off a chunk boundary (99 voxels each)
    for box in (((0, 0, 1), (32, 2, 2)), ((0, 0, 3), (32, 2, 3)), ((0, 0, 0), (32, 2, 0))):
        assert np.array_equal(hip_dev.volume_histogram(planes, box=box), hr.histogram(planes, box=box)), box
    odd = volume((4, 5, 31), 12)                                           # rows at odd offsets
    for box in (((1, 1, 1), (29, 3, 2)), ((30, 0, 0), (30, 4, 3)), ((0, 4, 3), (30, 4, 3))):
        assert np.array_equal(hip_dev.volume_histogram(odd, box=box), hr.histogram(odd, box=box)), box


# ---- contention and counter width ----
@pytest.mark.parametrize("value", [0, 1, 65535])
def test_all_equal_volume(hip_dev, value):
    shape = (160, 128, 128)                                                # 2.6 M voxels: above 2^16 and above 2^21
    n = shape[0] * shape[1] * shape[2]
    buf = hip_dev.malloc(2 * n)
    try:
        hip_dev.to_device(buf, np.full(shape, value, np.uint16))
        for shift in (0, 2, 8):                                            # two passes, one 16384-bin block, a small block
            got = hip_dev.volume_histogram(buf, shift=shift, shape=shape)
            assert int(got[value >> shift]) == n and int(got.sum(dtype=np.uint64)) == n, shift
        mask = np.zeros(shape, bool)
        mask[:, ::3, 5:] = True
        got = hip_dev.volume_histogram(buf, mask, shape=shape)
        assert int(got[value]) == int(mask.sum()) and np.count_nonzero(got) == 1
    finally:
        hip_dev.free(buf)


def test_all_equal_volume_beyond_16_bits_in_every_block(hip_dev):
    # every block of the capped grid meets more than 2^16 voxels of the one value, every wave more than 2^12: no counter on the way
    # (a wave's running count, a block's LDS counter, the output) may be narrower than the 32 bits the total needs
    shape = (129, 1024, 512)
    n = shape[0] * shape[1] * shape[2]
    assert n // MAX_BLOCKS > 1 << 16 and n <= 1 << 29
    buf = hip_dev.malloc(2 * n)
    try:
        hip_dev.check(hip_dev.lib.svr_memset_device(C.c_void_p(buf), 0x11, 2 * n))        # no host array of that size
        for shift in (0, 8):
            got = hip_dev.volume_histogram(buf, shift=shift, shape=shape)
            assert int(got[0x1111 >> shift]) == n and np.count_nonzero(got) == 1, shift
    finally:
        hip_dev.free(buf)


def test_two_valued_volume(hip_dev):
    shape = (40, 64, 129)
    v = np.zeros(shape, np.uint16)
    flat = v.reshape(-1)
    flat[0::2], flat[1::2] = 7, 40000                                      # alternating per voxel: no run is longer than one
    for shift in (0, 8):
        assert np.array_equal(hip_dev.volume_histogram(v, shift=shift), hr.histogram(v, shift=shift))
    flat[:] = np.repeat(np.array([7, 40000], np.uint16), flat.size // 2 + 1)[:flat.size]     # and in two halves
    assert np.array_equal(hip_dev.volume_histogram(v), hr.histogram(v))


def test_the_head(hip_dev, head, head_hist):
    assert int(head_hist[0]) * 100 // head.size == 67
    assert np.array_equal(hip_dev.volume_histogram(head), head_hist)
    assert np.array_equal(hip_dev.volume_histogram(head, shift=8), hr.histogram(head, shift=8))
    brain = (head >= 15000) & (head <= 30000)
    assert np.array_equal(hip_dev.volume_histogram(head, brain), hr.histogram(head, brain))


# ---- past one trip of the capped grid ----
def test_more_chunks_than_one_trip_of_the_grid(hip_dev):
    one_trip = MAX_BLOCKS * THREADS * CHUNK
    shape = (3, 1025, 4097)                                                # odd rows, three trips and a part of a fourth
    n = shape[0] * shape[1] * shape[2]
    assert 3 * one_trip < n <= 1 << 29
    buf = hip_dev.malloc(2 * n)
    try:
        hip_dev.check(hip_dev.lib.svr_memset_device(C.c_void_p(buf), 0, 2 * n))
        beacons = {0: 5, one_trip - 1: 6, one_trip: 7, one_trip + 1: 7, 2 * one_trip + 12345: 60000, 3 * one_trip + 1: 65535, n - 1: 9}
        for at, value in beacons.items():
            hip_dev.to_device(buf + 2 * at, np.array([value], np.uint16))
        want = np.zeros(65536, np.uint32)
        want[0] = n - len(beacons)
        for value in beacons.values():
            want[value] += 1
        assert np.array_equal(hip_dev.volume_histogram(buf, shape=shape), want)
        assert np.array_equal(hip_dev.volume_histogram(buf, shape=shape, shift=4), np.add.reduceat(want, np.arange(0, 65536, 16)))
    finally:
        hip_dev.free(buf)


# ---- per-label tables ----
def hand_labels(shape, seed, count, top):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, top + 1, shape).astype(np.uint32)
    lab[rng.random(shape) < 0.3] = 0
    flat = lab.reshape(-1)
    flat[0], flat[-1] = count + 1, 0xFFFFFFFF                              # labels above count: ignored
    return lab


@pytest.mark.parametrize("count", [0, 1, 300])
def test_label_histogram_of_hand_made_labels(hip_dev, count):
    for shape in ((3, 5, 31), (4, 7, 130)):
        v = volume(shape, 21)
        lab = hand_labels(shape, 22, count, count + 3)
        assert (lab > count).any() and (lab == 0).any()
        for lo, hi, shift in ((0, 65535, 10), (0, 65535, 8), (1000, 60000, 0 if count < 2 else 6), (0, 65535, 0 if count < 2 else 2)):
            got = hip_dev.region_label_histogram(lab, v, count, lo, hi, shift)
            want = hr.label_histogram(lab, v, count, lo, hi, shift)
            assert got.shape == (count + 1, hr.bins(lo, hi, shift)) and np.array_equal(got, want), (shape, lo, hi, shift)
        box = ((2, 1, 1), (29, 3, 2))
        assert np.array_equal(hip_dev.region_label_histogram(lab, v, count, shift=9, box=box), hr.label_histogram(lab, v, count, shift=9, box=box))


def test_label_histogram_of_the_bone_parts(hip_dev, head):
    bone = lr.threshold(head, 40000, 65535)
    labels, k = hip_dev.region_label(bone, 6)
    assert k >= 1
    table = hip_dev.region_label_table(labels, k, head)
    for shift in (8, 0) if (k + 1) * 65536 <= abi.HISTOGRAM_MAX_CELLS else (8,):
        got = hip_dev.region_label_histogram(labels, head, k, shift=shift)
        assert np.array_equal(got, hr.label_histogram(labels, head, k, shift=shift))
        assert np.array_equal(got[1:].sum(axis=1, dtype=np.uint64), table["voxels"].astype(np.uint64))       # rows sum to the parts' sizes
        assert int(got[0].sum()) == head.size - int(bone.sum())
        if shift == 0:
            sums = (got[1:].astype(np.uint64) * np.arange(65536, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
            assert np.array_equal(sums, table["sum"].astype(np.uint64))
    # the labels and voxels on the device, the table in a buffer of the caller's that held garbage
    n = head.size
    rows = k + 1
    d_lab, d_vox, d_out = hip_dev.malloc(4 * n), hip_dev.malloc(2 * n), hip_dev.malloc(4 * rows * 256)
    try:
        hip_dev.to_device(d_lab, labels)
        hip_dev.to_device(d_vox, head)
        hip_dev.check(hip_dev.lib.svr_memset_device(C.c_void_p(d_out), 0xA5, 4 * rows * 256))
        got = hip_dev.region_label_histogram(d_lab, d_vox, k, shift=8, shape=head.shape, out_ptr=d_out)
        assert np.array_equal(got, hr.label_histogram(labels, head, k, shift=8))
        assert np.array_equal(hip_dev.to_host(d_out, (rows, 256), np.uint32), got)
    finally:
        for p in (d_lab, d_vox, d_out):
            hip_dev.free(p)


def test_label_histogram_with_a_global_table(hip_dev, head):
    # more cells than the LDS passes hold (65536): the aggregated adds go to the table in global memory
    count = 40
    slabs = (np.arange(head.size, dtype=np.uint32).reshape(head.shape) // 997) % (count + 2)         # labels 0 .. count + 1 in runs
    for shift in (4, 0):
        assert (count + 1) * hr.bins(0, 65535, shift) > 2 * LDS_LARGE
        got = hip_dev.region_label_histogram(slabs, head, count, shift=shift)
        assert np.array_equal(got, hr.label_histogram(slabs, head, count, shift=shift)), shift


def test_label_histogram_cell_cap_is_refused(hip_dev):
    v = volume((2, 3, 33), 30)
    lab = np.zeros(v.shape, np.uint32)
    assert hip_dev.region_label_histogram(lab, v, 255, shift=0).shape == (256, 65536)                # exactly 2^24 cells
    with pytest.raises(host.SvrError, match="SVR_HISTOGRAM_MAX_CELLS"):
        hip_dev.region_label_histogram(lab, v, 256, shift=0)


# ---- consistency with the chain ----
def test_moments_equal_region_stats(hip_dev, head):
    for mask in ((head >= 15000) & (head <= 30000), head >= 40000, np.ones(head.shape, bool)):
        h = hip_dev.volume_histogram(head, mask)
        st = hip_dev.region_stats_of(head, mask)
        n, s, q = host.histogram_moments(h, hip_dev.lib)
        assert (n, s, q) == (int(st.voxels), int(st.sum), int(st.sum_sq))
        assert host.histogram_quantile(h, 0, 1, hip_dev.lib) == int(st.vmin) and host.histogram_quantile(h, 1, 1, hip_dev.lib) == int(st.vmax)
        want = rr.stats(head, mask)
        assert (n, s) == (want["voxels"], want["sum"])


def test_threshold_of_an_otsu_class_has_the_class_count(hip_dev, head):
    shift = 8
    h = hip_dev.volume_histogram(head, shift=shift)
    t, _eta = host.histogram_otsu(h, 3, hip_dev.lib)
    assert t == hr.otsu(h, 3)[0] == (51, 132)
    edges = (-1,) + t + (len(h) - 1,)
    total = 0
    for first, last in zip(edges[:-1], edges[1:]):
        lo = host.histogram_bin_range(first + 1, shift=shift, lib=hip_dev.lib)[0]
        hi = host.histogram_bin_range(last, shift=shift, lib=hip_dev.lib)[1]
        region = hip_dev.region_threshold(head, lo, hi)
        assert int(region.sum()) == int(h[first + 1:last + 1].sum())
        total += int(region.sum())
    assert total == head.size


def test_output_is_overwritten_and_overlap_refused(hip_dev):
    shape = (4, 7, 130)
    v = volume(shape, 40)
    n = v.size
    d_vox, d_out = hip_dev.malloc(2 * n), hip_dev.malloc(4 * 65536)
    try:
        hip_dev.to_device(d_vox, v)
        for shift in (0, 3):                                               # garbage first, twice: overwritten, not accumulated
            hip_dev.check(hip_dev.lib.svr_memset_device(C.c_void_p(d_out), 0xA5, 4 * 65536))
            bins = 65536 >> shift
            for _ in range(2):
                got = hip_dev.volume_histogram(d_vox, shift=shift, shape=shape, out_ptr=d_out)
                assert np.array_equal(got, hr.histogram(v, shift=shift))
            if bins < 65536:
                assert (hip_dev.to_host(d_out + 4 * bins, (16,), np.uint32) == 0xA5A5A5A5).all()      # nothing is written past the bins
        with pytest.raises(host.SvrError, match="overlap"):
            hip_dev.volume_histogram(d_vox, shift=8, shape=shape, out_ptr=d_vox + 2 * n - 4)
        with pytest.raises(host.SvrError, match="overlap"):
            hip_dev.volume_histogram(d_vox, shift=8, shape=shape, out_ptr=d_vox)
        assert hip_dev.volume_histogram_last_ms() >= 0.0
    finally:
        hip_dev.free(d_vox)
        hip_dev.free(d_out)
