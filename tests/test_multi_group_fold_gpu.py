"""Folding launches of several groups of 64 frames (SVR_OPT_GROUP_FRAMES = 128 / 256; csrc/svr_trace_tile.hip launch_tile_t, csrc/svr_tile_tasks.hpp
fold_pending_groups, csrc/svr_api_trace.hip fold_group_frames): in the skipping traceDepth-1 queue builds without pooled walks a call of 128 frames and more is
ONE launch per 128 / 256 frames.  A ticket is a pixel pair x all its frame groups, the running mean of a pixel is replayed in frame order across its groups
(chained where they are pending together, through the accumulator where a drain falls between them), and the kept whole-ray march of a pair -- its
tag no longer names a frame group -- serves every group.  Scheduling only: image and accumulator are the oracle's bit for bit in the production and
the counting build, the counting build traces pixels x frames paths and its taps, Woodcock iterations, scatter events and shadow walks are the
oracle's.  How many launches a call made is read from the timing ring (svr_get_kernel_time), so that every case is known to have run the form it is
about: one launch per call in the new form, launches of at most 64 frames for every plan that does not have it.

The fixture of tests/conftest.py sets SVR_OPT_GROUP_FRAMES = 64 before every test, so every case here sets the option itself."""
import ctypes as C
import dataclasses
import functools
import re

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests.util import assert_bit_exact, hip_frames, oracle_frames

pytestmark = pytest.mark.gpu

COUNTERS = ("vol_taps", "woodcock_iters", "scatter_events", "shadow_walks")


@functools.lru_cache(maxsize=None)
def _scene(name, W, H, depth=1, variant="default"):
    sc = scenes.make_scene(name, trace_depth=depth, width=W, height=H)
    if variant == "inside":        # tMin = 1e-6 for every ray (tests/test_shared_march_gpu.py: every pair marches once, its second pixel reuses)
        cam = host.camera_setup((3.0, -2.0, 5.0), (0.0, 1.0, -4.0), (0.0, 1.0, 0.0), 60.0, 0.0, 1.0, 1.0, W, H)
        sc = dataclasses.replace(sc, name=name + "_inside", camera=cam)
    elif variant == "grazing":
        half = sc.dim[0] / 2.0
        cam = host.camera_setup((half * 1.02, 0.1 * half, 3.5 * half), (half * 0.9, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.0, 1.0, 1.0, W, H)
        sc = dataclasses.replace(sc, name=name + "_grazing", camera=cam)
    elif variant == "lens":
        sc = dataclasses.replace(sc, name=name + "_lens", apeture=0.8, focal_length=1.3)
    return sc


@functools.lru_cache(maxsize=None)
def _oracle(name, W, H, depth, variant, nframes, window=None):
    """(accumulator, image, counters) of the oracle: computed once per shape, shared by the cases, never written to."""
    hdr, img, c = oracle_frames(_scene(name, W, H, depth, variant), nframes, window=window)
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


def _check(dev, name, W, H, nframes, what, launches, group=256, depth=1, variant="default", rows=None, cols=None, oracle_window=None, opts=None, **kw):
    """production + counting build (hip_frames compares the two) against the oracle; `launches`: trace launches of ONE render of the call"""
    sc = _scene(name, W, H, depth, variant)
    ref_hdr, ref_img, ref_c = _oracle(name, W, H, depth, variant, nframes, oracle_window or kw.get("window"))
    with _options(dev, OPT_QUEUE=2, OPT_GROUP_FRAMES=group, OPT_TIMING=1, **(opts or {})):
        dev.check(dev.lib.svr_reset_kernel_time())
        hdr, img, c = hip_frames(dev, sc, nframes, batch=True, **kw)
        n_launch = dev.kernel_time()[1]
    ys = slice(*rows) if rows else slice(0, H)
    xs = slice(*cols) if cols else slice(0, W)
    assert_bit_exact(hdr[ys, xs], ref_hdr[ys, xs], what)
    assert np.array_equal(img[ys, xs], ref_img[ys, xs]), what
    n_px = (ys.stop - ys.start) * (xs.stop - xs.start)
    print(what, {k: (c[k], ref_c[k]) for k in COUNTERS}, "paths", c["paths"], "launches", n_launch)
    assert c["paths"] == n_px * nframes, f"{what}: {c['paths']} paths traced, {n_px} pixels x {nframes} frames asked for"
    for k in COUNTERS:
        assert c[k] == ref_c[k], f"{what}: {k} {c[k]}, oracle {ref_c[k]}"
    assert n_launch == 2 * launches, f"{what}: {n_launch} trace launches in the two renders, {launches} each expected"
    return c


@pytest.mark.parametrize("nframes", [128, 192])
def test_one_launch_from_frame_0(hip_dev, nframes):
    """(1) tiny_head 24 x 8: two and three groups (three does not divide the 64 tasks of a drain)"""
    c = _check(hip_dev, "tiny_head", 24, 8, nframes, f"tiny_head 24 x 8 x {nframes}", launches=1)
    assert c["shadow_walks"] > 0


def _many_tasks_shape(dev, groups):
    """width x height with at least 1.25 x 64 tasks (pixels x groups) for every wave of a launch at one block per CU"""
    num_cus = int(re.search(r"CUs=(\d+)", dev.info()).group(1))
    waves = num_cus * 4 // 16 * 16
    W = 320
    H = -(-(5 * 64 * waves // 4) // (W * groups))
    assert W * H * groups >= 1.25 * 64 * waves
    return W, H


def test_pixel_straddles_a_drain(hip_dev):
    """(1) 192 frames with more than 64 tasks per wave.  By construction: at one block per CU the launch has num_cus x 4 waves, and the shape gives
    them 80 tasks each on average, so by pigeonhole some wave takes more than 64.  Its tickets are 2 pixels x 3 groups = 6 tasks and it drains when 64
    are pending (or earlier, when its records run out): 64 = 10 x 6 + 4, so the drain falls behind group 0 of a ticket's second pixel, whose groups 1
    and 2 are folded by the next drain from the accumulator that the first one wrote."""
    W, H = _many_tasks_shape(hip_dev, 3)
    c = _check(hip_dev, "tiny_head", W, H, 192, f"tiny_head {W} x {H} x 192, 1 block per CU", launches=1, opts=dict(OPT_BLOCKS_PER_CU=1))
    assert c["shadow_walks"] > 0


@pytest.mark.parametrize("shape", ["small", "many_tasks"])
def test_continue_an_accumulator(hip_dev, shape):
    """(2) 64 frames, then 128 frames with frameNo = 64: group 0 of the second call reads the accumulator, nothing is cleared"""
    W, H = (24, 8) if shape == "small" else _many_tasks_shape(hip_dev, 2)
    sc = _scene("tiny_head", W, H)
    calls = (64, 128)
    ref_hdr, ref_img, ref_c = _oracle("tiny_head", W, H, 1, "default", sum(calls))
    canvas = host.Canvas(hip_dev, W, H)
    try:
        scenes.apply_to_canvas(sc, canvas)
        with _options(hip_dev, OPT_QUEUE=2, OPT_GROUP_FRAMES=256, OPT_TIMING=1, OPT_BLOCKS_PER_CU=1):
            for count in (0, 1):
                hip_dev.set_option(abi.OPT_COUNT, count)
                hip_dev.reset_counters()
                hip_dev.check(hip_dev.lib.svr_reset_kernel_time())
                canvas.ReStartRender()
                for n in calls:
                    canvas.paint_frames(n)
                hip_dev.synchronize()
                assert hip_dev.kernel_time()[1] == 2
                assert_bit_exact(canvas.read_hdr(), ref_hdr, f"calls of {calls} frames, count {count}")
                assert np.array_equal(canvas.read_img(), ref_img)
            c = hip_dev.counters()
        print({k: (c[k], ref_c[k]) for k in COUNTERS}, "paths", c["paths"])
        assert c["paths"] == W * H * sum(calls)
        for k in COUNTERS:
            assert c[k] == ref_c[k], f"{k} {c[k]}, oracle {ref_c[k]}"
    finally:
        hip_dev.set_option(abi.OPT_COUNT, 0)
        canvas.close()


@pytest.mark.parametrize("nframes,group,launches", [(200, 256, 2), (130, 256, 2), (200, 128, 3)])
def test_remainders(hip_dev, nframes, group, launches):
    """(3) 200 = 192 + 8 (a folding launch of 8 frames), 130 = 128 + 2 (the scratch slots), and 200 = 128 + 64 + 8 at 128 frames per launch"""
    _check(hip_dev, "tiny_head", 24, 8, nframes, f"tiny_head 24 x 8 x {nframes}, {group} frames per launch", launches=launches, group=group)


@pytest.mark.parametrize("unit", [1, 3, 5])
def test_ticket_units_that_would_split_a_pixel(hip_dev, unit):
    """(4) tickets of 1, 3 and 5 tasks are no multiple of the two groups of a 128-frame launch: a pixel's groups would go to different waves, which
    cannot fold them in order, so the call is two launches of 64 frames and the result does not change"""
    _check(hip_dev, "tiny_head", 24, 8, 128, f"tiny_head 24 x 8 x 128, unit {unit}", launches=2, opts=dict(OPT_UNIT=unit))


@pytest.mark.parametrize("unit", [2, 6])
def test_ticket_units_of_whole_pixels(hip_dev, unit):
    """(4) one pixel and three pixels per ticket: pairs are split between waves, every pixel keeps its groups"""
    _check(hip_dev, "tiny_head", 24, 8, 128, f"tiny_head 24 x 8 x 128, unit {unit}", launches=1, opts=dict(OPT_UNIT=unit))


def test_odd_width_and_height(hip_dev):
    """(5)"""
    _check(hip_dev, "tiny_head", 17, 5, 128, "tiny_head 17 x 5 x 128", launches=1)


def test_window_with_odd_left_edge(hip_dev):
    """(5)"""
    _check(hip_dev, "tiny_head", 24, 8, 128, "window (3, 1, 20, 6)", launches=1, rows=(1, 6), cols=(3, 20), window=(3, 1, 20, 6))


def test_row_shard(hip_dev):
    """(5) rank 1 of 3 with 16-row strips on a 16 x 48 image: rows 16 .. 31, which the oracle renders as a window"""
    _check(hip_dev, "tiny_head", 16, 48, 128, "row shard", launches=1, rows=(16, 32), shard=(16, 1, 3), oracle_window=(0, 16, 16, 32))


def test_nan_guard(hip_dev):
    """(6) the guarded loop of the chained fold: no sample is a NaN here, so the oracle's bits"""
    assert np.isfinite(_oracle("tiny_head", 24, 8, 1, "default", 128)[0]).all()
    _check(hip_dev, "tiny_head", 24, 8, 128, "tiny_head 24 x 8 x 128, NaN guard", launches=1, opts=dict(OPT_NAN_GUARD=1))


def test_render_where_every_pair_reuses(hip_dev):
    """(7) four rows of 256 x 256 from inside tiny_head, where every pair's second pixel walks on its neighbour's march
    (tests/test_shared_march_gpu.py): here the march of a pair serves its four tasks"""
    W = H = 256
    y0, y1 = 126, 130
    c = _check(hip_dev, "tiny_head", W, H, 128, f"rows {y0} .. {y1 - 1} of 256 x 256 from inside, 128 frames", launches=1, variant="inside",
               rows=(y0, y1), window=(0, y0, W, y1))
    assert c["scatter_events"] > 0


@pytest.mark.parametrize("case", ["small", "inside"])
def test_64_frames_per_launch_gives_the_same_bits(hip_dev, case):
    """(8) the same inputs as two launches of 64 frames"""
    if case == "small":
        _check(hip_dev, "tiny_head", 24, 8, 128, "tiny_head 24 x 8 x 128, 64 frames per launch", launches=2, group=64)
    else:
        _check(hip_dev, "tiny_head", 256, 256, 128, "rows 126 .. 129 of 256 x 256 from inside, 64 frames per launch", launches=2, group=64, variant="inside",
               rows=(126, 130), window=(0, 126, 256, 130))


def test_thin_lens_keeps_64_frames_per_launch(hip_dev):
    """(9) no shared march under a thin lens: not the form"""
    _check(hip_dev, "tiny_head", 24, 8, 128, "thin lens, 128 frames", launches=2, variant="lens")


def test_depth_2_keeps_64_frames_per_launch(hip_dev):
    """(9) deeper paths drain 32 tasks and fold with fold_pending"""
    _check(hip_dev, "tiny_head", 24, 8, 128, "depth 2, 128 frames", launches=2, depth=2)


def test_row_order_keeps_64_frames_per_launch(hip_dev):
    """(9) tickets that own tile rows are single tasks"""
    _check(hip_dev, "tiny_head", 24, 8, 128, "row order, 128 frames", launches=2, opts=dict(OPT_ROW_ORDER=1))


def test_adaptive_call_keeps_64_frames_per_launch(hip_dev):
    """(9) an adaptive call with a target below every tile's error is a uniform render of max_frames = 256 frames, traced between checkpoints at 8, 16,
    32, 64 and 128 frames over tile lists: its launches keep at most 64 frames (7 of them at least), and the result is the oracle's"""
    W, H = 24, 8
    sc = _scene("tiny_head", W, H)
    ref_hdr, _, _ = _oracle("tiny_head", W, H, 1, "default", 256)
    canvas = host.Canvas(hip_dev, W, H)
    try:
        scenes.apply_to_canvas(sc, canvas)
        with _options(hip_dev, OPT_QUEUE=2, OPT_GROUP_FRAMES=256, OPT_TIMING=1):
            hip_dev.check(hip_dev.lib.svr_reset_kernel_time())
            canvas.ReStartRender()
            res = canvas.paint_adaptive(1e-9, 0, 256, sync=True)
            n_launch = hip_dev.kernel_time()[1]
        print(res.frames_max, res.checkpoints, "launches", n_launch)
        assert res.frames_max == res.frames_min == 256
        assert n_launch >= 7
        assert_bit_exact(canvas.read_hdr(), ref_hdr, "adaptive call, target 1e-9, 256 frames")
    finally:
        canvas.close()


def _selftest(dev, name, W, H, variant, frame0):
    """svr_selftest_group_march on the scene, the wave's lanes = frames frame0 .. frame0 + 63: dict of its eight sums"""
    sc = _scene(name, W, H, 1, variant)
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
def test_march_calls_clear_only_what_is_empty_in_later_groups(hip_dev, name, variant, size):
    """The property the shared march rests on, for the frame lanes of groups 1 .. 3 (frames 64 .. 255): whatever group's lanes are admitted to a march
    along the pair's un-jittered reference ray, no point of a stretch that the returned parameter or the map calls clear lies in a macro-cell that
    is not empty.  (The tag names the pair alone; that a lane may use a march is the admission's word, which this runs for every lane.)"""
    for frame0 in (64, 128, 192):
        r = _selftest(hip_dev, name, size, size, variant, frame0)
        print(name, variant, size, frame0, r)
        assert r["hit_lanes"] > 0 and r["points"] > 0
        assert r["violations"] == 0
