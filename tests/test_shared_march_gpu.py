"""The whole-ray march that the two pixels of a pair share (csrc/svr_walk.hpp, walk_setup_shared): launches of one pixel x 64 frames per task in
the skipping traceDepth-1 queue builds without pooled walks (folding, counting, DIRECT).  A wave keeps its last march -- reference ray, interval,
result, map -- and the next task reuses it when every lane that hits the box passes the admission against it.  Scheduling only: accumulator and
image are the oracle's bit for bit in the production and the counting build, and paths, taps, Woodcock iterations and scatter events are the
oracle's.  The shapes break the pairs in every way the launcher can: odd widths and heights, ticket units and row orders that split pairs, a window
with an odd left edge, a row shard; cameras for which the admission refuses (inside the volume, thin lens, pixels too wide) and a call with two
pixels per task, where nothing is shared.

The property all of this rests on -- a march may call clear only what is empty, for every lane that is admitted to it -- is tested directly with
svr_selftest_group_march (csrc/svr_selftest.hip), which also says how many marches were shared, reused and refused, so that the cases are known
to have run both paths."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests.util import assert_bit_exact, hip_frames, oracle_frames

pytestmark = pytest.mark.gpu

COUNTERS = ("vol_taps", "woodcock_iters", "scatter_events")


@functools.lru_cache(maxsize=None)
def _scene(name, W, H, variant="default"):
    sc = scenes.make_scene(name, trace_depth=1, width=W, height=H)
    half = sc.dim[0] / 2.0
    if variant == "inside":        # tMin = 1e-6 for every ray
        cam = host.camera_setup((3.0, -2.0, 5.0), (0.0, 1.0, -4.0), (0.0, 1.0, 0.0), 60.0, 0.0, 1.0, 1.0, W, H)
        sc = dataclasses.replace(sc, name=name + "_inside", camera=cam)
    elif variant == "grazing":     # along the +x face of the box: short and missing box segments next to long ones
        cam = host.camera_setup((half * 1.02, 0.1 * half, 3.5 * half), (half * 0.9, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.0, 1.0, 1.0, W, H)
        sc = dataclasses.replace(sc, name=name + "_grazing", camera=cam)
    elif variant == "lens":        # origins differ from lane to lane: no lane is admitted to another lane's march
        sc = dataclasses.replace(sc, name=name + "_lens", apeture=0.8, focal_length=1.3)
    return sc


@functools.lru_cache(maxsize=None)
def _oracle(name, W, H, variant, nframes, window=None):
    """(accumulator, image, counters) of the oracle: computed once per shape, shared by the cases, never written to."""
    hdr, img, c = oracle_frames(_scene(name, W, H, variant), nframes, window=window)
    hdr.setflags(write=False)
    img.setflags(write=False)
    return hdr, img, c


class _options:
    """set options for a block and put back what they were"""

    def __init__(self, dev, **opts):
        self.dev, self.opts = dev, [(getattr(abi, k), v) for k, v in opts.items()]

    def __enter__(self):
        self.old = [(o, self.dev.lib.svr_get_option(o)) for o, _ in self.opts]
        for o, v in self.opts:
            self.dev.set_option(o, v)

    def __exit__(self, *exc):
        for o, v in self.old:
            self.dev.set_option(o, v)


def _check(dev, name, W, H, nframes, what, variant="default", rows=None, cols=None, oracle_window=None, opts=None, **kw):
    """production + counting build (hip_frames compares the two) against the oracle"""
    sc = _scene(name, W, H, variant)
    ref_hdr, ref_img, ref_c = _oracle(name, W, H, variant, nframes, oracle_window or kw.get("window"))
    with _options(dev, OPT_QUEUE=2, **(opts or {})):
        hdr, img, c = hip_frames(dev, sc, nframes, batch=True, **kw)
    ys = slice(*rows) if rows else slice(0, H)
    xs = slice(*cols) if cols else slice(0, W)
    assert_bit_exact(hdr[ys, xs], ref_hdr[ys, xs], what)
    assert np.array_equal(img[ys, xs], ref_img[ys, xs]), what
    n_px = (ys.stop - ys.start) * (xs.stop - xs.start)
    print(what, {k: (c[k], ref_c[k]) for k in COUNTERS}, "paths", c["paths"])
    assert c["paths"] == n_px * nframes, f"{what}: {c['paths']} paths traced, {n_px} pixels x {nframes} frames asked for"
    for k in COUNTERS:
        assert c[k] == ref_c[k], f"{what}: {k} {c[k]}, oracle {ref_c[k]}"
    return c


@pytest.mark.parametrize("unit,row_order", [(0, 0), (3, 0), (0, 1), (3, 1)])
def test_pairs_units_and_row_orders(hip_dev, unit, row_order):
    """24 x 8: whole pairs.  Tickets of three tasks and tickets that own tile rows split them: reuse is decided by the tag and the admission"""
    c = _check(hip_dev, "tiny_head", 24, 8, 64, f"tiny_head 24 x 8 x 64, unit {unit}, row order {row_order}", opts=dict(OPT_UNIT=unit, OPT_ROW_ORDER=row_order))
    assert c["scatter_events"] > 0


def test_odd_width_and_height(hip_dev):
    """17 x 5: the last pixel of a row has no partner, and with two tasks per ticket the pairs of every other row straddle two tickets"""
    c = _check(hip_dev, "tiny_head", 17, 5, 64, "tiny_head 17 x 5 x 64")
    assert c["scatter_events"] > 0


def test_window_with_odd_left_edge(hip_dev):
    c = _check(hip_dev, "tiny_head", 24, 8, 64, "window (3, 1, 20, 6)", rows=(1, 6), cols=(3, 20), window=(3, 1, 20, 6))
    assert c["scatter_events"] > 0


def test_row_shard(hip_dev):
    """rank 1 of 3 with 16-row strips on a 16 x 48 image: rows 16 .. 31, which the oracle renders as a window"""
    c = _check(hip_dev, "tiny_head", 16, 48, 64, "row shard", rows=(16, 32), shard=(16, 1, 3), oracle_window=(0, 16, 16, 32))
    assert c["scatter_events"] > 0


def test_camera_inside_the_volume(hip_dev):
    c = _check(hip_dev, "tiny_head", 24, 8, 64, "camera inside the volume", variant="inside")
    assert c["scatter_events"] > 0


def test_thin_lens(hip_dev):
    """apeture > 0: the lanes of a pixel start from different points of the lens, so none is admitted to a shared march"""
    c = _check(hip_dev, "tiny_head", 24, 8, 64, "thin lens", variant="lens")
    assert c["scatter_events"] > 0


def test_pixels_too_wide(hip_dev):
    """8 x 8 pixels on small_head: a pixel is several macro-cells wide at the far end of the box, dev * hi > 0.25"""
    c = _check(hip_dev, "small_head", 8, 8, 64, "small_head 8 x 8 x 64")
    assert c["scatter_events"] > 0


def test_two_pixels_per_task(hip_dev):
    """a 40-frame call: two pixels x 32 frame lanes per task, nothing is shared between tasks"""
    c = _check(hip_dev, "tiny_head", 24, 8, 40, "tiny_head 24 x 8 x 40")
    assert c["scatter_events"] > 0


def test_direct_form(hip_dev):
    """The DIRECT form runs only in batches of frames traced ahead of per-frame calls (tests/test_drain_shape_gpu.py): 127 canvas.paint() calls
    trace frames 63 .. 126 as one 64-frame batch of one-pixel tasks and fold all of it."""
    W, H, calls = 24, 8, 127
    sc = _scene("tiny_head", W, H)
    ref_hdr, ref_img, _ = _oracle("tiny_head", W, H, "default", calls)
    canvas = host.Canvas(hip_dev, W, H)
    try:
        scenes.apply_to_canvas(sc, canvas)
        with _options(hip_dev, OPT_QUEUE=2):
            canvas.ReStartRender()
            for _ in range(calls):
                canvas.paint()
            hip_dev.synchronize()
            assert_bit_exact(canvas.read_hdr(), ref_hdr, f"tiny_head {W} x {H}, {calls} per-frame calls, frames traced ahead")
            assert np.array_equal(canvas.read_img(), ref_img)
    finally:
        canvas.close()


def _selftest(dev, name, W, H, variant, frame0=0):
    """svr_selftest_group_march on the scene: dict of its eight sums"""
    sc = _scene(name, W, H, variant)
    canvas = host.Canvas(dev, W, H)
    try:
        scenes.apply_to_canvas(sc, canvas)
        out = np.zeros(8, dtype=np.uint64)
        dev.check(dev.lib.svr_selftest_group_march(frame0, out.ctypes.data_as(C.c_void_p)))
    finally:
        canvas.close()
    keys = ("violations", "points", "shared", "reused", "refused", "alone", "hit_lanes", "valid_maps")
    return dict(zip(keys, (int(v) for v in out)))


@pytest.mark.parametrize("size", [64, 256])
@pytest.mark.parametrize("variant", ["default", "grazing", "inside"])
@pytest.mark.parametrize("name", ["tiny_head", "small_head"])
def test_march_calls_clear_only_what_is_empty(hip_dev, name, variant, size):
    """Every lane that hits the box walks its ray in steps of 1/8 macro-cell; no point of a stretch that the returned parameter or the map calls
    clear may lie in a macro-cell that is not empty."""
    r = _selftest(hip_dev, name, size, size, variant)
    print(name, variant, size, r)
    assert r["hit_lanes"] > 0 and r["points"] > 0
    assert r["violations"] == 0
    if name == "small_head" and variant == "default" and size == 256:
        # both ways out of a matching tag ran: the kept march reused, and the kept march refused with a march for the pixel alone behind it
        assert r["reused"] > 0
        assert r["refused"] > 0


def test_no_reuse_at_wide_pixels(hip_dev):
    r = _selftest(hip_dev, "small_head", 8, 8, "default")
    print(r)
    assert r["hit_lanes"] > 0 and r["violations"] == 0
    assert r["reused"] == 0 and r["refused"] > 0


def test_render_where_every_pair_reuses(hip_dev):
    """The small images above have pixels so wide that no march is ever reused: they hold the refusals and the marches for a pixel alone.  At 256 x 256
    from inside tiny_head every ray hits the box, every pair marches once and its second pixel reuses that march (the self-test: pair marches =
    reuses = pixels / 2, nothing refused).  Four rows of that image through the tile kernel, production and counting build, against the oracle: the
    paths of the pixels that walked on a neighbour's march are the oracle's bit for bit."""
    W = H = 256
    r = _selftest(hip_dev, "tiny_head", W, H, "inside")
    print(r)
    assert r["violations"] == 0
    assert r["shared"] == W * H // 2 and r["reused"] == W * H // 2 and r["refused"] == 0 and r["alone"] == 0
    y0, y1 = 126, 130
    c = _check(hip_dev, "tiny_head", W, H, 64, f"rows {y0} .. {y1 - 1} of 256 x 256 from inside", variant="inside", rows=(y0, y1), window=(0, y0, W, y1))
    assert c["scatter_events"] > 0
