"""The first iteration of a shadow walk run in place by the traceDepth-1 queue builds of the tile kernel (svr_trace_tile.hip / svr_lanes.hpp,
SVR_SHADOW_FIRST): after the shading, a hit lane sets its shadow walk up, runs its first Woodcock iteration on its own generator and either
settles the estimate where it stands (the walk collided, left the box, or had nothing to do) or queues the walk as a resumable record that the
lane machine continues.  Scheduling only: accumulator and image are the oracle's bit for bit in the production and the counting build, the
counting build traces pixels x frames paths, and its taps, iterations, scatter events and shadow walks are the oracle's.

tiny_head at 24 x 8 x 64 frames has 873 shadow walks (oracle): 649 collide in their first iteration, 32 in the second, 6 later, 185 escape, and 123
have a BSDF value of exactly zero -- every branch runs, and a wrong generator or ray parameter in a resumed record changes an escape or a
collision and with it a pixel.  The other shapes: two pixels per task with dead frame lanes, a launch in which most waves get no task, the
non-folding (DIRECT) form, a window, a row shard (strips are multiples of 8 rows, so the shard is the 16 x 48 one of test_task_loop_gpu.py),
one light without an environment behind a steep transfer function, the pooled and the deeper build (which keep their code), and calls of
13, 61 and 64 frames onto one accumulator (records resumed with frame0 > 0)."""
import functools

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests.util import assert_bit_exact, hip_frames, oracle_frames

pytestmark = pytest.mark.gpu

COUNTERS = ("vol_taps", "woodcock_iters", "scatter_events", "shadow_walks")


@functools.lru_cache(maxsize=None)
def _scene(name, W, H, depth):
    return scenes.make_scene(name, trace_depth=depth, width=W, height=H)


@functools.lru_cache(maxsize=None)
def _oracle(name, W, H, depth, nframes, window=None):
    """(accumulator, image, counters) of the oracle: computed once per shape, shared by the cases, never written to."""
    hdr, img, c = oracle_frames(_scene(name, W, H, depth), nframes, window=window)
    hdr.setflags(write=False)
    img.setflags(write=False)
    return hdr, img, c


def _check(dev, name, W, H, depth, nframes, what, rows=None, cols=None, oracle_window=None, **kw):
    """production + counting build (hip_frames compares the two) against the oracle.  oracle_window: the part of the image the oracle renders
    when the launch is cut out another way (a row shard): its counters are then those of the launch's own pixels."""
    sc = _scene(name, W, H, depth)
    ref_hdr, ref_img, ref_c = _oracle(name, W, H, depth, nframes, oracle_window or kw.get("window"))
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


# 24 x 8 x 64: every outcome of the first iteration; 17 x 5 x 40: two pixels per task, 24 dead frame lanes -- hit lanes of two pixels settle and
# push in one task; 8 x 8 x 64: most waves get no task, the queue is drained with a handful of records
@pytest.mark.parametrize("W,H,nframes", [(24, 8, 64), (17, 5, 40), (8, 8, 64)])
def test_first_iteration_in_place(hip_dev, W, H, nframes):
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    c = _check(hip_dev, "tiny_head", W, H, 1, nframes, f"tiny_head {W} x {H}, {nframes} frames")
    assert c["shadow_walks"] > 0


def test_non_folding_launch(hip_dev):
    """The DIRECT form: a path settled in place writes its scratch slot itself."""
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    hip_dev.set_option(abi.OPT_FOLD, 0)
    _check(hip_dev, "tiny_head", 24, 8, 1, 40, "24 x 8, 40 frames, not folding")


def test_window(hip_dev):
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    _check(hip_dev, "tiny_head", 24, 8, 1, 64, "window of 24 x 8", rows=(1, 6), cols=(3, 20), window=(3, 1, 20, 6))


def test_row_shard(hip_dev):
    """rank 1 of 3 with 16-row strips on a 16 x 48 image: rows 16 .. 31, which the oracle renders as a window (x0, y0, x1, y1) so that its
    counters are those of the shard's pixels"""
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    c = _check(hip_dev, "tiny_head", 16, 48, 1, 64, "row shard", rows=(16, 32), shard=(16, 1, 3), oracle_window=(0, 16, 16, 32))
    assert c["shadow_walks"] > 0


def test_one_light_steep_transfer_function(hip_dev):
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    c = _check(hip_dev, "tiny_bone", 24, 8, 1, 64, "tiny_bone 24 x 8, 64 frames")
    assert c["shadow_walks"] > 0


def test_pooled_build_unchanged(hip_dev):
    hip_dev.set_option(abi.OPT_POOL, 2)
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    _check(hip_dev, "tiny_head_noisy", 24, 8, 1, 64, "tiny_head_noisy 24 x 8, pooled primary walks")


def test_deeper_build_unchanged(hip_dev):
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    _check(hip_dev, "tiny_head", 24, 8, 3, 64, "tiny_head 24 x 8, depth 3")


def test_calls_onto_one_accumulator(hip_dev):
    """13, 61 and 64 frames: the second and third call resume their records with frame0 > 0."""
    W, H = 24, 8
    sc = _scene("tiny_head", W, H, 1)
    calls = (13, 61, 64)
    ref_hdr, ref_img, ref_c = _oracle("tiny_head", W, H, 1, sum(calls))
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    canvas = host.Canvas(hip_dev, W, H)
    try:
        scenes.apply_to_canvas(sc, canvas)
        for count in (0, 1):
            hip_dev.set_option(abi.OPT_COUNT, count)
            hip_dev.reset_counters()
            canvas.ReStartRender()
            for n in calls:
                canvas.paint_frames(n)
            hip_dev.synchronize()
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
