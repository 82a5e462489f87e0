"""svr_region_threshold / _label / _label_table / _select / _select_by_size on the GPU: every label array, table and mask -- masks as
uint32 words, padding included -- is EQUAL to the test-side reference (tests/label_ref.py: a numpy fixpoint iteration and definitions).
Output buffers are pre-filled with a pattern.  The fixtures and the conditions they meet are those of tests/test_label_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import label_ref as lr
from tests import region_ref as rr
from tests.test_label_cpu import HEAD_COUNTS, NOISE_COUNTS, NOISE_SHAPE, WINDOWS
from tests.test_region_cpu import BONE, BRAIN

pytestmark = pytest.mark.gpu


class Labels:
    """Raw calls on buffers the test owns: (return code, message, ...) back."""

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

    def mask(self, m=None):
        return self.raw(4 * self.words) if m is None else self.put(rr.pack(m))

    def read_mask(self, p):
        return self.dev.to_host(p, (self.words,), np.uint32)

    def done(self, rc):
        msg = self.lib.svr_last_error().decode()
        self.lib.svr_clear_error()
        return rc, msg

    def label(self, src, conn, out):
        k = C.c_uint32(0xFFFFFFFF)
        rc, msg = self.done(self.lib.svr_region_label(C.c_void_p(src), *self.dims, conn, C.c_void_p(out), C.byref(k)))
        assert rc == 0, msg
        return self.dev.to_host(out, self.shape, np.uint32), int(k.value)

    def table(self, labels, count, out, vox=None, on_device=1):
        src = None if vox is None else (C.c_void_p(vox) if on_device else vox.ctypes.data_as(C.c_void_p))
        rc, msg = self.done(self.lib.svr_region_label_table(C.c_void_p(labels), src, *self.dims, on_device, count, C.c_void_p(out)))
        assert rc == 0, msg
        self.dev.synchronize()
        return self.dev.to_host(out, (count,), host.COMPONENT_DTYPE)

    def select(self, labels, count, keep, out):
        rc, msg = self.done(self.lib.svr_region_select(C.c_void_p(labels), *self.dims, count, C.c_void_p(self.put(np.asarray(keep, dtype=np.uint8))),
                                                       C.c_void_p(out)))
        assert rc == 0, msg
        self.dev.synchronize()
        return self.read_mask(out)

    def by_size(self, labels, count, table, min_voxels, largest_k, out):
        k = C.c_uint32(0xFFFFFFFF)
        rc, msg = self.done(self.lib.svr_region_select_by_size(C.c_void_p(labels), *self.dims, count, C.c_void_p(table), min_voxels, largest_k,
                                                               C.c_void_p(out), C.byref(k)))
        assert rc == 0, msg
        return self.read_mask(out), int(k.value)

    def threshold(self, vox, on_device, lo, hi, box, out):
        src = C.c_void_p(vox) if on_device else vox.ctypes.data_as(C.c_void_p)
        b0 = b1 = None
        if box is not None:
            b0, b1 = (C.c_int32 * 3)(*box[0]), (C.c_int32 * 3)(*box[1])
        rc, msg = self.done(self.lib.svr_region_threshold(src, *self.dims, on_device, lo, hi, b0, b1, C.c_void_p(out)))
        assert rc == 0, msg
        self.dev.synchronize()
        return self.read_mask(out)

    def close(self):
        for p in self.bufs:
            self.dev.free(p)
        self.bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def same_mask(words, want_mask, what):
    want = rr.pack(want_mask)
    if not np.array_equal(words, want):
        diff = rr.unpack(words ^ want, want_mask.shape)
        raise AssertionError(f"{what}: {int(diff.sum())} voxels differ; first (z, y, x) {np.argwhere(diff)[:1].tolist()}; "
                             f"padding differs: {not np.array_equal(rr.pack(rr.unpack(words, want_mask.shape)), words)}")


def same_labels(got, k, want, want_k, what):
    if k != want_k or not np.array_equal(got, want):
        diff = got != want
        at = np.argwhere(diff)[:1].tolist()
        raise AssertionError(f"{what}: K {k} (reference {want_k}); {int(diff.sum())} labels differ, first (z, y, x) {at}: "
                             f"{got[tuple(at[0])] if at else None} for {want[tuple(at[0])] if at else None}")


def same_table(got, want, what):
    for f in lr.COMPONENT_FIELDS:
        if not np.array_equal(got[f], want[f]):
            bad = got[f] != want[f]
            i = int(np.flatnonzero(bad.any(axis=1) if bad.ndim > 1 else bad)[0])
            raise AssertionError(f"{what}: `{f}` of label {i + 1} is {got[f][i]}, reference {want[f][i]}")


def check_labelling(L, m, conn, what, ref=None, vox=None, d_vox=None):
    """Labels, K and the table of mask m against the reference; returns (labels, K)."""
    want, want_k = ref if ref is not None else lr.label(m, conn)
    d_labels = L.raw(4 * L.n)
    got, k = L.label(L.mask(m), conn, d_labels)
    same_labels(got, k, want, want_k, what)
    if k:
        t = L.table(d_labels, k, L.raw(40 * k), d_vox, 1)
        same_table(t, lr.table(want, want_k, vox if d_vox is not None else None), what + ", table")
        assert int(t["voxels"].sum()) == int(m.sum()) and (np.diff(t["first"].astype(np.int64)) > 0).all()
    return got, k


@pytest.fixture(scope="module")
def head():
    return scenes.make_scene("tiny_head").vox


# ------------------------------------------------------------------------------------------------ labels, K and the table
@pytest.mark.parametrize("shape", rr.EDGE_SHAPES + [lr.SCAN3_SHAPE], ids=lambda s: "x".join(str(n) for n in s[::-1]))
def test_label_shapes(hip_dev, shape):
    vox = rr.noise_volume(shape, seed=5)
    # (the shape that is there for the third level of the scan takes the case with the most components only, 12 250 under 6: its reference
    # is the slowest, and the scan does not depend on the connectivity)
    densities = lr.DENSITIES if shape != lr.SCAN3_SHAPE else (0.3,)
    masks = [(str(d), lr.random_mask(shape, d, 30 + i)) for i, d in enumerate(densities)]
    masks += [("empty", np.zeros(shape, dtype=bool)), ("full", np.ones(shape, dtype=bool))]
    with Labels(hip_dev, shape) as L:
        d_vox = L.put(vox)
        for name, m in masks:
            for conn in (lr.CONNS if shape != lr.SCAN3_SHAPE or name in ("empty", "full") else (6,)):
                ref = (m.astype(np.uint32), int(m.any())) if name in ("empty", "full") else None
                _, k = check_labelling(L, m, conn, f"{shape} density {name} conn {conn}", ref, vox, d_vox)
                assert name not in ("empty", "full") or k == (name == "full")


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_label_head_windows(hip_dev, head, name):
    m = lr.threshold(head, *WINDOWS[name])
    with Labels(hip_dev, head.shape) as L:
        d_vox = L.put(head)
        for conn in lr.CONNS:
            _, k = check_labelling(L, m, conn, f"head {name} conn {conn}", lr.labelled("head-" + name, m, conn), head, d_vox)
            assert k == HEAD_COUNTS[name][conn]


def test_label_noise_and_serpentine(hip_dev):
    vox = rr.noise_volume(NOISE_SHAPE)
    with Labels(hip_dev, NOISE_SHAPE) as L:
        d_vox = L.put(vox)
        for (lo, hi), counts in NOISE_COUNTS.items():
            m = lr.threshold(vox, lo, hi)
            for conn in lr.CONNS:
                _, k = check_labelling(L, m, conn, f"noise 0..{hi} conn {conn}", lr.labelled(f"noise-{hi}", m, conn), vox, d_vox)
                assert k == counts[conn]
    s = rr.serpentine()[0] > 0
    with Labels(hip_dev, s.shape) as L:
        for conn in lr.CONNS:
            _, k = check_labelling(L, s, conn, f"serpentine conn {conn}", (s.astype(np.uint32), 1))     # one label, the longest chains
            assert k == 1


def test_label_checkerboard(hip_dev):
    c = lr.checkerboard()
    rank = np.zeros(c.shape, dtype=np.uint32)
    rank[c] = np.arange(1, int(c.sum()) + 1, dtype=np.uint32)                            # every voxel its own component: label = rank
    with Labels(hip_dev, c.shape) as L:
        _, k = check_labelling(L, c, 6, "checkerboard conn 6", (rank, 131072))
        assert k == 131072
        for conn in (18, 26):
            check_labelling(L, c, conn, f"checkerboard conn {conn}", (c.astype(np.uint32), 1))


@pytest.mark.parametrize("pair", rr.PAIRS, ids=lambda p: p[0])
def test_label_pairs(hip_dev, pair):
    _, a, b = pair
    with Labels(hip_dev, rr.PAIR_SHAPE) as L:
        d_labels, d_mask = L.raw(4 * L.n), L.mask()
        for first, second in ((a, b), (b, a)):
            m = rr.pair_volume(first, second) > 0
            L.dev.to_device(d_mask, rr.pack(m))
            for conn in lr.CONNS:
                got, k = L.label(d_mask, conn, d_labels)
                assert k == 3 - rr.pair_expected(a, b, conn), (pair[0], conn)
                lo, hi = sorted([(p[2], p[1], p[0]) for p in (a, b)])
                want = np.zeros(rr.PAIR_SHAPE, dtype=np.uint32)
                want[lo], want[hi] = 1, k
                assert np.array_equal(got, want), (pair[0], conn)


@pytest.mark.parametrize("nx", [33, 40])
def test_label_ignores_input_padding(hip_dev, nx):
    shape = (6, 9, nx)
    m = lr.random_mask(shape, 0.4, 3)
    wx = (nx + 31) // 32
    dirty = rr.pack(m).reshape(-1, wx).copy()
    dirty[:, -1] |= np.uint32((0xFFFFFFFF << (nx % 32)) & 0xFFFFFFFF)                    # ones in every padding bit
    with Labels(hip_dev, shape) as L:
        d_labels, d_labels2 = L.raw(4 * L.n), L.raw(4 * L.n, prefill=0x5A)
        for conn in lr.CONNS:
            want, want_k = lr.label(m, conn)
            got, k = L.label(L.put(dirty.reshape(-1)), conn, d_labels)
            same_labels(got, k, want, want_k, f"padding nx {nx} conn {conn}")
            again, k2 = L.label(L.put(dirty.reshape(-1)), conn, d_labels2)               # determinism: every word, twice
            assert k2 == k and np.array_equal(again, got)


def test_label_numbers_by_first_voxel(hip_dev):
    m = lr.last_largest()
    with Labels(hip_dev, m.shape) as L:
        for conn in lr.CONNS:
            got, k = check_labelling(L, m, conn, f"last-largest conn {conn}")
            assert k == 3 and got[0, 0, 0] == 1 and got[0, 0, 40] == 2 and (got[2:5, 3:9, 20:60] == 3).all()


# ------------------------------------------------------------------------------------------------ the table
def test_table_sums_sources_and_contention(hip_dev):
    shape = NOISE_SHAPE
    vox = rr.noise_volume(shape)
    m = lr.threshold(vox, 0, 250)
    want, want_k = lr.labelled("noise-250", m, 6)
    with Labels(hip_dev, shape) as L:
        d_labels, d_vox = L.put(want), L.put(vox)
        d_table = L.raw(40 * want_k)
        same_table(L.table(d_labels, want_k, d_table), lr.table(want, want_k), "no volume")
        same_table(L.table(d_labels, want_k, d_table, d_vox, 1), lr.table(want, want_k, vox), "device volume")
        same_table(L.table(d_labels, want_k, d_table, vox, 0), lr.table(want, want_k, vox), "host volume")
        # one component that fills the volume: every run of every wave lands on one entry
        full = np.ones(shape, dtype=np.uint32)
        t = L.table(L.put(full), 1, L.raw(40), d_vox, 1)
        same_table(t, lr.table(full, 1, vox), "one component")
        assert int(t["voxels"][0]) == vox.size and int(t["sum"][0]) == int(vox.astype(np.uint64).sum())
        # labels above `count` are ignored
        same_table(L.table(d_labels, 5, L.raw(40 * 5), d_vox, 1), {k: v[:5] for k, v in lr.table(want, want_k, vox).items()}, "count 5")
        got = hip_dev.region_label_table(want, want_k, vox)
        same_table(got, lr.table(want, want_k, vox), "Device.region_label_table")


# ------------------------------------------------------------------------------------------------ selection
def test_select_and_select_by_size(hip_dev, head):
    m = lr.threshold(head, *WINDOWS["brain"])
    with Labels(hip_dev, head.shape) as L:
        out = L.mask()
        for conn in (6, 18):
            labels, count = lr.labelled("head-brain", m, conn)
            d_labels = L.put(labels)
            d_table = L.raw(40 * count)
            L.table(d_labels, count, d_table)
            none, every = np.zeros(count + 1, dtype=np.uint8), np.ones(count + 1, dtype=np.uint8)
            odd = (np.arange(count + 1) % 2).astype(np.uint8)
            even = (1 - odd).astype(np.uint8)                                            # (entry 0 set: background must not enter)
            for name, keep in (("none", none), ("all", every), ("odd", odd), ("even", even)):
                same_mask(L.select(d_labels, count, keep, out), lr.select(labels, keep), f"select {name} conn {conn}")
            same_mask(L.select(d_labels, count, odd, out) | L.select(d_labels, count, even, out), m, "complementary keeps")
            for min_voxels, largest_k in ((1, 0), (10, 0), (0, 1), (0, 3), (10, 2), (13710, 0), (0, count + 5)):
                want, want_kept = lr.select_by_size(labels, count, min_voxels, largest_k)
                got, kept = L.by_size(d_labels, count, d_table, min_voxels, largest_k, out)
                assert kept == want_kept, (conn, min_voxels, largest_k, kept, want_kept)
                same_mask(got, want, f"select_by_size min {min_voxels} k {largest_k} conn {conn}")
                if min_voxels == 13710:
                    assert kept == 0 and not got.any()
            if conn == 18:                                                               # k = 3 on the tie 20 = 20: the lower label wins
                sizes = np.bincount(labels.reshape(-1))[1:]
                tied = np.flatnonzero(sizes == 20) + 1
                got, kept = L.by_size(d_labels, count, d_table, 0, 3, out)
                g = rr.unpack(got, head.shape)
                assert kept == 3 and len(tied) >= 2 and g[labels == tied[0]].all() and not g[labels == tied[1]].any()
    # padding in out, and the Python layer
    shape = (5, 7, 33)
    mm = lr.random_mask(shape, 0.5, 9)
    labels, count = lr.label(mm, 6)
    with Labels(hip_dev, shape) as L:
        same_mask(L.select(L.put(labels), count, np.ones(count + 1, dtype=np.uint8), L.mask()), mm, "padding of select")
    assert np.array_equal(hip_dev.region_select(labels, count, np.ones(count + 1)), mm)
    got, kept = hip_dev.region_select_by_size(labels, count, min_voxels=3, largest_k=2)
    want, want_kept = lr.select_by_size(labels, count, 3, 2)
    assert kept == want_kept and np.array_equal(got, want)
    got_labels, k = hip_dev.region_label(mm, 6)
    assert k == count and np.array_equal(got_labels, labels)


# ------------------------------------------------------------------------------------------------ threshold
@pytest.mark.parametrize("shape", [(9, 10, 40), (7, 9, 33), (5, 6, 130)], ids=lambda s: "x".join(str(n) for n in s[::-1]))
def test_threshold(hip_dev, shape):
    vox = rr.noise_volume(shape, seed=3)
    nz, ny, nx = shape
    boxes = [None, ((1, 2, 1), (nx - 3, ny - 2, nz - 2)), ((-5, 0, 2), (31, 100, 2)), ((nx - 1, 0, 0), (nx + 7, ny, nz))]
    with Labels(hip_dev, shape) as L:
        d_vox, out = L.put(vox), L.mask()
        for box in boxes:
            for lo, hi in ((0, 649), (300, 300), (0, 65535)):
                want = rr.candidates(vox, lo, hi, box)
                same_mask(L.threshold(d_vox, 1, lo, hi, box, out), want, f"threshold device {shape} {lo}..{hi} box {box}")
                same_mask(L.threshold(vox, 0, lo, hi, box, out), want, f"threshold host {shape} {lo}..{hi} box {box}")
    assert np.array_equal(hip_dev.region_threshold(vox, 0, 649, boxes[1]), rr.candidates(vox, 0, 649, boxes[1]))


# ------------------------------------------------------------------------------------------------ against the existing code
def test_labels_agree_with_reconstruct(hip_dev, head):
    m = lr.threshold(head, *WINDOWS["brain"])
    for conn in lr.CONNS:
        labels, k = hip_dev.region_label(m, conn)
        t = hip_dev.region_label_table(labels, k)
        for i in range(1, 6):
            marker = np.zeros(head.shape, dtype=bool)
            marker.reshape(-1)[int(t["first"][i - 1])] = True
            got, _ = hip_dev.region_reconstruct(marker, m, conn)
            assert np.array_equal(rr.pack(got), rr.pack(labels == i)), (conn, i)


# ------------------------------------------------------------------------------------------------ the loop, once
def _raycast(canvas, volume):
    dev = canvas.dev
    dev.check(dev.lib.svr_memset_device(C.c_void_p(canvas.img), 0, canvas.W * canvas.H * 4))
    dev.lib.render_raycasting(C.c_void_p(canvas.img), C.byref(volume), C.byref(canvas.transferFunction), C.byref(canvas.camera),
                              C.c_float(canvas.stepSize))
    dev.check()
    dev.synchronize()
    return canvas.read_img()


def test_threshold_label_keep_largest_measure_show(hip_dev, head):
    dev, lib = hip_dev, hip_dev.lib
    sc = scenes.make_scene("tiny_head")
    cv = host.Canvas(dev, sc.width, sc.height)
    scenes.apply_to_canvas(sc, cv)
    nz, ny, nx = head.shape
    words = host.region_mask_words(head.shape)
    lo, hi = BRAIN[0], BONE[1]                                                           # brain and bone in one window
    d_out, d_mask, d_big, d_labels, texs = dev.malloc(head.nbytes), dev.malloc(4 * words), dev.malloc(4 * words), dev.malloc(4 * head.size), []
    try:
        before = _raycast(cv, cv.deviceVolume)
        window = dev.region_threshold(head, lo, hi, out_ptr=d_mask)
        assert np.array_equal(window, lr.threshold(head, lo, hi))
        ptr, k = dev.region_label(d_mask, 6, shape=head.shape, out_ptr=d_labels)
        want_labels, want_k = lr.label(window, 6)
        assert ptr == d_labels and k == want_k and k >= 1
        big, kept = dev.region_select_by_size(d_labels, k, largest_k=1, shape=head.shape, out_ptr=d_big)
        want, want_kept = lr.select_by_size(want_labels, want_k, 0, 1)
        assert kept == want_kept == 1 and np.array_equal(big, want) and 0 < big.sum() <= window.sum()
        got, ref = dev.region_stats_of(head, d_big).as_dict(), rr.stats(head, want)
        for key in rr.STAT_INTS:
            assert got[key] == ref[key], f"{key} is {got[key]}, reference {ref[key]}"
        assert dev.region_apply(head, d_big, abi.REGION_KEEP, 0, out_ptr=d_out) == d_out
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
        assert np.array_equal(_raycast(cv, cv.deviceVolume), before)                      # the component calls left the renderers alone
    finally:
        for t in texs:
            lib.svr_destroy_texture(t)
        for p in (d_out, d_mask, d_big, d_labels):
            dev.free(p)
        cv.close()
