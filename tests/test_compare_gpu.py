"""The comparison calls on the GPU against the numpy reference of tests/compare_ref.py, bit for bit: the shapes at which mask words carry
into one another, end padded or unpadded, or are a single row or column; masks with every padding bit set; both sides of the label
table's LDS switches and more work than one trip of the capped grids cover (the constants are read from the source); and
svr_region_compare on the small head, field by field against the reference and against the calls that already exist."""
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import compare_ref as cr
from tests import distance_ref as dr

pytestmark = pytest.mark.gpu

SOURCE = (Path(__file__).resolve().parents[1] / "sunvolumerender_amd" / "csrc" / "svr_compare.hip").read_text()
SHAPES = [(1, 1, 1), (1, 1, 32), (1, 1, 33), (3, 5, 31), (2, 3, 64), (2, 3, 65), (5, 4, 97), (4, 7, 130), (7, 1, 1)]
NONE = cr.NONE


def constant(name):
    m = re.search(rf"constexpr int {name} = (\d+);", SOURCE)
    assert m, name
    return int(m.group(1))


CMP_THREADS, CMP_MAX_BLOCKS, HIST_LDS_BINS = constant("CMP_THREADS"), constant("CMP_MAX_BLOCKS"), constant("CMP_HIST_LDS_BINS")
OVL_THREADS, OVL_MAX_BLOCKS = constant("OVL_THREADS"), constant("OVL_MAX_BLOCKS")
OVL_SMALL, OVL_LARGE = constant("OVL_LDS_CELLS_SMALL"), constant("OVL_LDS_CELLS_LARGE")


def masks_of(shape, seed):
    nz, ny, nx = shape
    rng = np.random.default_rng(seed)
    m = {"empty": np.zeros(shape, bool), "full": np.ones(shape, bool), "corner": np.zeros(shape, bool), "rows": np.zeros(shape, bool),
         "random 2 %": rng.random(shape) < 0.02, "random 40 %": rng.random(shape) < 0.4}
    m["corner"][nz - 1, ny - 1, nx - 1] = True
    m["rows"][:, ::2, :] = True
    return m


def dirty_mask_words(mask):
    """the bit mask of a bool array with every padding bit set"""
    words = host.region_mask_pack(mask).reshape(mask.shape[0], mask.shape[1], -1).copy()
    if mask.shape[2] % 32:
        words[:, :, -1] |= np.uint32((0xFFFFFFFF << (mask.shape[2] % 32)) & 0xFFFFFFFF)
    return words.reshape(-1)


class Buffers:
    def __init__(self, dev):
        self.dev, self.ptrs = dev, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.dev.free(p)

    def put(self, array, offset=0):
        a = np.ascontiguousarray(array)
        self.ptrs.append(self.dev.malloc(max(a.nbytes, 4) + offset))
        self.dev.to_device(self.ptrs[-1] + offset, a)
        return self.ptrs[-1] + offset

    def dirty(self, mask):
        return self.put(dirty_mask_words(mask))

    def raw(self, nbytes):
        self.ptrs.append(self.dev.malloc(nbytes))
        return self.ptrs[-1]


def random_map(shape, seed, top=1 << 32):
    """a uint32 map with SVR_DIST_NONE entries, zeros and 0xFFFFFFFE in it (a one-voxel map keeps the last)"""
    rng = np.random.default_rng(seed)
    d2 = rng.integers(0, top, shape, dtype=np.uint64).astype(np.uint32)
    flat = d2.reshape(-1)
    flat[rng.random(flat.size) < 0.1] = NONE
    flat[rng.random(flat.size) < 0.1] = 0
    for value in (NONE, 0, 0xFFFFFFFE):
        flat[rng.integers(0, flat.size)] = value
    return d2


# ---- the surface ----
@pytest.mark.parametrize("shape", SHAPES)
def test_surface_shapes_elements_and_dirty_padding(hip_dev, shape):
    words = host.region_mask_words(shape)
    with Buffers(hip_dev) as b:
        out = b.raw(4 * words)
        for name, mask in masks_of(shape, sum(shape)).items():
            src = b.dirty(mask)
            for element in (6, 18, 26):
                want = cr.surface(mask, element)
                assert np.array_equal(hip_dev.region_surface(mask, element), want), (name, element)
                hip_dev.to_device(out, np.full(words, 0xFFFFFFFF, np.uint32))
                assert np.array_equal(hip_dev.region_surface(src, element, shape=shape, out_ptr=out), want), (name, element)
                got = hip_dev.to_host(out, (words,), np.uint32)
                assert np.array_equal(got, host.region_mask_pack(want)), (name, element, "the output's padding bits are 0")
            if name == "empty":
                assert not want.any()
            if name == "full":                                    # the six faces
                faces = np.ones(shape, bool)
                faces[1:-1, 1:-1, 1:-1] = False
                assert np.array_equal(want, faces)


def test_surface_of_a_box_is_its_shell_and_differs_from_erode(hip_dev):
    box = np.zeros((9, 10, 70), bool)
    box[2:7, 3:8, 20:66] = True                                   # crosses the words 0 | 1 | 2 of a row
    shell = box.copy()
    shell[3:6, 4:7, 21:65] = False
    for element in (6, 18, 26):
        assert np.array_equal(hip_dev.region_surface(box, element), shell)
        assert np.array_equal(box & ~hip_dev.region_morph(box, abi.MORPH_ERODE, element, 1), shell)     # away from the faces the two agree
    full = np.ones((3, 4, 64), bool)
    assert not (full & ~hip_dev.region_morph(full, abi.MORPH_ERODE, 6, 1)).any()                        # ERODE keeps a full mask ...
    assert int(hip_dev.region_surface(full, 6).sum()) == 3 * 4 * 64 - 1 * 2 * 62                       # ... the surface is its faces


# ---- the overlap counts ----
@pytest.mark.parametrize("shape", SHAPES)
def test_overlap_with_and_without_a_domain(hip_dev, shape):
    ms = masks_of(shape, 7 * sum(shape))
    domain = np.random.default_rng(sum(shape)).random(shape) < 0.7
    with Buffers(hip_dev) as b:
        dev = {name: b.dirty(m) for name, m in ms.items()}
        ddom = b.dirty(domain)
        for na, nb in (("random 40 %", "rows"), ("random 2 %", "random 40 %"), ("full", "corner"), ("empty", "full"), ("rows", "rows")):
            want = cr.overlap(ms[na], ms[nb])
            assert sum(want) == ms[na].size
            assert hip_dev.region_overlap(ms[na], ms[nb]) == want, (na, nb)
            assert hip_dev.region_overlap(dev[na], dev[nb], shape=shape) == want, (na, nb)
            want_d = cr.overlap(ms[na], ms[nb], domain)
            assert sum(want_d) == int(domain.sum())
            assert hip_dev.region_overlap(ms[na], ms[nb], domain) == want_d, (na, nb)
            assert hip_dev.region_overlap(dev[na], dev[nb], ddom, shape=shape) == want_d, (na, nb)


def test_overlap_beyond_one_trip_of_the_grid(hip_dev):
    shape = (1, CMP_MAX_BLOCKS * CMP_THREADS // 2 + 5, 40)        # two words a row: one trip and a bit
    assert host.region_mask_words(shape) > CMP_MAX_BLOCKS * CMP_THREADS
    rng = np.random.default_rng(1)
    a, b = rng.random(shape) < 0.5, rng.random(shape) < 0.25
    assert hip_dev.region_overlap(a, b) == cr.overlap(a, b)


# ---- the label table ----
def label_maps(shape, count_a, count_b, seed):
    """two label maps with every label up to its count + 2 present where the map is large enough, in runs and in noise"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    a = np.repeat(rng.integers(0, count_a + 3, n // 5 + 1), 5)[:n]          # runs: equal neighbouring cells
    b = rng.integers(0, count_b + 3, n)
    b[n // 2:] = np.repeat(rng.integers(0, count_b + 3, n // 16 + 1), 8)[:n - n // 2]
    return a.astype(np.uint32).reshape(shape), b.astype(np.uint32).reshape(shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_label_table_shapes_and_alignment(hip_dev, shape):
    a, b = label_maps(shape, 3, 5, sum(shape))
    want = cr.label_overlap(a, 3, b, 5)
    assert int(want.sum()) == int(((a <= 3) & (b <= 5)).sum())
    assert a.size < 64 or (a > 3).any() and (b > 5).any()         # labels above the counts are present
    assert np.array_equal(hip_dev.region_label_overlap(a, 3, b, 5), want)
    with Buffers(hip_dev) as buf:
        odd_a, odd_b = buf.put(a, 4), buf.put(b, 8)               # not 16-byte aligned: the one-voxel chunks
        assert np.array_equal(hip_dev.region_label_overlap(odd_a, 3, odd_b, 5, shape=shape), want)
        table = buf.put(np.full(24, 77, np.uint32))               # the table is overwritten, not accumulated
        hip_dev.region_label_overlap(a, 3, b, 5, out_ptr=table)
        assert np.array_equal(hip_dev.to_host(table, (4, 6), np.uint32), want)


SWITCH_COUNTS = [(127, 127), (127, 128), (255, 255), (255, 256), (1, 20000)]


@pytest.mark.parametrize("count_a,count_b", SWITCH_COUNTS)
def test_label_table_on_both_sides_of_the_lds_switches(hip_dev, count_a, count_b):
    cells = (count_a + 1) * (count_b + 1)
    sides = {(127, 127): cells == OVL_SMALL, (127, 128): OVL_SMALL < cells <= 2 * OVL_LARGE, (255, 255): cells == 2 * OVL_LARGE,
             (255, 256): cells > 2 * OVL_LARGE, (1, 20000): OVL_LARGE < cells < 2 * OVL_LARGE}        # two passes, the second partial
    assert sides[(count_a, count_b)], "the switches moved: choose other counts"
    shape = (6, 50, 67)
    a, b = label_maps(shape, count_a, count_b, cells)
    a[0, 0, :4], b[0, 0, :4] = (0, count_a, count_a, 0), (0, count_b, 0, count_b)       # the corner cells of the table
    want = cr.label_overlap(a, count_a, b, count_b)
    assert want[count_a, count_b] >= 1 and want[0, 0] >= 1
    assert np.array_equal(hip_dev.region_label_overlap(a, count_a, b, count_b), want)
    uniform = np.full(shape, count_a, np.uint32), np.full(shape, count_b, np.uint32)     # one cell: the wave-uniform trips
    got = hip_dev.region_label_overlap(uniform[0], count_a, uniform[1], count_b)
    assert got[count_a, count_b] == a.size and int(got.sum()) == a.size


def test_label_table_beyond_one_trip_of_the_grid(hip_dev):
    n = 4 * OVL_MAX_BLOCKS * OVL_THREADS * 2 + 4 * 1000 + 3       # two trips of four-voxel chunks, a part of a third, a partial chunk
    shape = (1, 1, n)
    a, b = label_maps(shape, 9, 2, 5)
    a[0, 0, n // 3:n // 2] = 4                                    # a long uniform stretch: (cell, count) carried over trips
    b[0, 0, n // 3:n // 2] = 1
    assert np.array_equal(hip_dev.region_label_overlap(a, 9, b, 2), cr.label_overlap(a, 9, b, 2))


# ---- summary, histogram, quantile of a map over a mask ----
def check_summary(got, want, note):
    for field in cr.SUMMARY_FIELDS:
        assert cr.summary_of_struct(got)[field] == want[field], (note, field)


@pytest.mark.parametrize("shape", SHAPES)
def test_map_summary_histogram_quantile(hip_dev, shape):
    d2 = random_map(shape, 3 * sum(shape))
    small = random_map(shape, 5 * sum(shape), 300)
    tol = (0, 1, 99, 1 << 20, 1 << 31, 0xFFFFFFFE, NONE, 150)
    with Buffers(hip_dev) as b:
        dmap, dsmall = b.put(d2), b.put(small)
        for name, mask in list(masks_of(shape, sum(shape)).items()) + [("no mask", None)]:
            dmask = None if mask is None else b.dirty(mask)
            for m, ptr, label in ((d2, dmap, "wide"), (small, dsmall, "small")):
                check_summary(hip_dev.region_distance_summary(m, mask, tol), cr.summary(m, mask, tol), (name, label, "host"))
                check_summary(hip_dev.region_distance_summary(ptr, dmask, tol[:3], shape=shape), cr.summary(m, mask, tol[:3]), (name, label, "device"))
                for num, den in ((0, 1), (1, 2), (95, 100), (1, 1)):
                    assert hip_dev.region_distance_quantile(ptr, num, den, dmask, shape=shape) == cr.quantile(m, num, den, mask), (name, label, num, den)
            for lo, hi, shift in ((0, 299, 0), (3, 250, 2), (0, NONE, 16), (0, 0xFFFFFFFE, 16), (1 << 31, NONE, 31), (NONE, NONE, 0),
                                  (0, HIST_LDS_BINS - 1, 0), (0, HIST_LDS_BINS, 0), (5, 65540, 0)):
                for m, ptr in ((d2, dmap), (small, dsmall)):
                    want = cr.histogram(m, mask, lo, hi, shift)
                    assert np.array_equal(hip_dev.region_distance_histogram(ptr, dmask, lo, hi, shift, shape=shape), want), (name, lo, hi, shift)
            assert np.array_equal(hip_dev.region_distance_histogram(small, mask, 0, 299), cr.histogram(small, mask, 0, 299)), name


def test_map_without_values(hip_dev):
    shape = (2, 3, 40)
    nothing = np.full(shape, NONE, np.uint32)
    s = hip_dev.region_distance_summary(nothing, None, (5,))
    check_summary(s, cr.summary(nothing, None, (5,)), "all none")
    assert (s.voxels, s.none, s.max, s.first_max) == (0, 240, 0, 0)
    assert hip_dev.region_distance_quantile(nothing, 1, 2) is None
    assert hip_dev.region_distance_quantile(np.zeros(shape, np.uint32), 1, 2, np.zeros(shape, bool)) is None
    assert int(hip_dev.region_distance_histogram(nothing, None, 0, NONE, 16)[65535]) == 240


def test_map_beyond_one_trip_of_the_grid(hip_dev):
    """A synthetic map over more mask words than one trip of the capped grid covers: rows of one voxel, so a word is a voxel."""
    trip = CMP_MAX_BLOCKS * CMP_THREADS
    shape = (trip + 77, 2, 1)
    assert host.region_mask_words(shape) > 2 * trip
    rng = np.random.default_rng(9)
    d2 = rng.integers(0, 100000, shape).astype(np.uint32)
    d2[rng.random(shape) < 0.05] = NONE
    flat = d2.reshape(-1)
    flat[[5, flat.size - 2]] = 123456                             # the maximum twice: the first index wins, from the last trip or not
    for mask in (None, rng.random(shape) < 0.03, rng.random(shape) < 0.6):
        with Buffers(hip_dev) as b:
            dmap, dmask = b.put(d2), None if mask is None else b.dirty(mask)
            check_summary(hip_dev.region_distance_summary(dmap, dmask, (10, 50000), shape=shape), cr.summary(d2, mask, (10, 50000)), "trips")
            assert np.array_equal(hip_dev.region_distance_histogram(dmap, dmask, 0, 123456, 1, shape=shape), cr.histogram(d2, mask, 0, 123456, 1))
            assert hip_dev.region_distance_quantile(dmap, 95, 100, dmask, shape=shape) == cr.quantile(d2, 95, 100, mask)
    wide = (trip // 20 + 3, 2, 300)                               # ten words a row, the last padded: one trip and a bit
    assert host.region_mask_words(wide) > trip
    d2 = rng.integers(0, 70000, wide).astype(np.uint32)
    mask = rng.random(wide) < 0.02
    check_summary(hip_dev.region_distance_summary(d2, mask, (7,)), cr.summary(d2, mask, (7,)), "wide trips")
    assert hip_dev.region_distance_quantile(d2, 1, 2, mask) == cr.quantile(d2, 1, 2, mask)


def test_two_pass_quantile_with_a_shift(hip_dev):
    """Values beyond 65536: the first pass bins at a shift, the second resolves the chosen bin."""
    rng = np.random.default_rng(4)
    shape = (5, 6, 70)
    d2 = (rng.integers(0, 1 << 12, shape).astype(np.uint32) << 20) + rng.integers(0, 1 << 20, shape).astype(np.uint32)
    d2[0, 0, 0] = 0xFFFFFFFE
    d2[0, 0, 1:9] = NONE
    mask = rng.random(shape) < 0.5
    for num, den in ((0, 7), (1, 3), (1, 2), (95, 100), (999, 1000), (1, 1)):
        assert hip_dev.region_distance_quantile(d2, num, den, mask) == cr.quantile(d2, num, den, mask), (num, den)
        assert hip_dev.region_distance_quantile(d2, num, den) == cr.quantile(d2, num, den), (num, den)
    same = np.full(shape, 3000000000, np.uint32)                  # one value in one bin of the second pass
    assert hip_dev.region_distance_quantile(same, 1, 2) == 3000000000


# ---- svr_region_compare on the small head ----
@pytest.fixture(scope="module")
def head():
    return scenes.make_ct_head_volume(48)


@pytest.fixture(scope="module")
def brain(head):
    """(lo, hi, mask): the brain window of the phantom head (the raw window of tools/distance_time.py)"""
    lo, hi = 23593, 28835
    mask = (head >= lo) & (head <= hi)
    assert 0.02 < mask.mean() < 0.9
    return lo, hi, mask


def check_comparison(got, want, note):
    got = cr.comparison_of_struct(got)
    for field in want:
        assert got[field] == want[field], (note, field)


def test_compare_with_itself(hip_dev, brain):
    _, _, a = brain
    c = hip_dev.region_compare(a, a, tolerances2=(0,))
    check_comparison(c, cr.compare(a, a, tolerances2=(0,)), "itself")
    n, s = int(a.sum()), int(cr.surface(a).sum())
    assert list(c.overlap) == [n, 0, 0, a.size - n] and list(c.surface) == [s, s] and c.status == 0
    for d in (c.ab, c.ba):
        assert (d.voxels, d.none, d.sum, d.sum_root_q8, d.max, d.within[0]) == (s, 0, 0, 0, 0, s)
    m = host.compare_measure(c)
    assert (m.dice, m.jaccard, m.hausdorff, m.hausdorff_q, m.assd, m.rms, m.surface_dice[0]) == (1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)


def test_compare_with_the_median_filtered_window(hip_dev, head, brain):
    lo, hi, a = brain
    filtered = hip_dev.volume_median(head, 18, 1)
    b = hip_dev.region_threshold(filtered, lo, hi)
    assert (a ^ b).any() and (a & b).any()
    tol = (0, 1, 4)
    for element in (6, 26):
        c = hip_dev.region_compare(a, b, element, tolerances2=tol)
        check_comparison(c, cr.compare(a, b, element, tolerances2=tol), ("median", element))
    # the struct agrees with the calls that exist
    c = hip_dev.region_compare(a, b)
    assert c.overlap[0] + c.overlap[1] == hip_dev.region_stats_of(head, a).voxels
    assert c.overlap[0] + c.overlap[2] == hip_dev.region_stats_of(head, b).voxels
    sa, sb = hip_dev.region_surface(a), hip_dev.region_surface(b)
    assert list(c.surface) == [int(sa.sum()), int(sb.sum())]
    to_b = hip_dev.region_distance(sb)
    assert (c.ab.max, c.ab.first_max, abi.REGION_STATUS_OK) == hip_dev.region_distance_max(to_b, sa)
    assert c.quantile_ab == hip_dev.region_distance_quantile(to_b, 95, 100, sa)
    check_summary(hip_dev.region_distance_summary(to_b, sa), cr.comparison_of_struct(c)["ab"], "summary alone")
    assert hip_dev.region_compare_last_ms() > 0.0


def test_compare_with_a_shifted_copy_and_spacing_weights(hip_dev, brain):
    _, _, a = brain
    b = np.zeros_like(a)
    b[:, 2:, 1:] = a[:, :-2, :-1]                                 # moved by (1, 2, 0) in (x, y, z)
    c = hip_dev.region_compare(a, b, quantile=(1, 2), tolerances2=(1, 5))
    check_comparison(c, cr.compare(a, b, 6, (1, 1, 1), (1, 2), (1, 5)), "shifted")
    assert 0 < c.ab.max and c.status == 0
    weights, unit = host.distance_weights((1.0, 1.0, 2.0), a.shape)
    assert weights[2] == 4 * weights[0]
    cw = hip_dev.region_compare(a, b, 18, weights, tolerances2=(weights[0],))
    want = cr.compare(a, b, 18, weights, (95, 100), (weights[0],))
    check_comparison(cw, want, "weights")
    m, ref = host.compare_measure(cw, unit), cr.measure(want, unit)
    for name in ("dice", "hausdorff", "hausdorff_q", "assd", "rms"):
        assert abs(getattr(m, name) - ref[name]) <= 1e-12 * abs(ref[name]), name


def test_compare_with_an_empty_mask(hip_dev, brain):
    _, _, a = brain
    e = np.zeros_like(a)
    s = int(cr.surface(a).sum())
    c = hip_dev.region_compare(a, e, tolerances2=(9,))
    check_comparison(c, cr.compare(a, e, tolerances2=(9,)), "B empty")
    assert c.status == abi.COMPARE_B_EMPTY and (c.ab.voxels, c.ab.none, c.ba.voxels, c.ba.none) == (0, s, 0, 0)
    c = hip_dev.region_compare(e, a)
    check_comparison(c, cr.compare(e, a), "A empty")
    assert c.status == abi.COMPARE_A_EMPTY and (c.ab.none, c.ba.none) == (0, s)
    c = hip_dev.region_compare(e, e)
    check_comparison(c, cr.compare(e, e), "both empty")
    assert c.status == abi.COMPARE_A_EMPTY | abi.COMPARE_B_EMPTY and list(c.overlap) == [0, 0, 0, a.size]


@pytest.mark.parametrize("shape", SHAPES)
def test_compare_on_the_edge_shapes(hip_dev, shape):
    ms = masks_of(shape, 11 * sum(shape))
    if not dr.fits((1, 2, 3), shape):
        pytest.fail("the shapes changed: choose weights that fit")
    with Buffers(hip_dev) as b:
        for na, nb in (("random 40 %", "rows"), ("full", "corner"), ("random 2 %", "random 40 %")):
            want = cr.compare(ms[na], ms[nb], 18, (1, 2, 3), (3, 4), (2, 6))
            got = hip_dev.region_compare(b.dirty(ms[na]), b.dirty(ms[nb]), 18, (1, 2, 3), (3, 4), (2, 6), shape=shape)
            check_comparison(got, want, (na, nb))
