"""Tasks per drain and record capacity as properties of a build of the tile kernel (svr_kernels.hpp DrainShape, svr_trace_tile.hip): the skipping
traceDepth-1 queue builds without pooled walks (folding, DIRECT) pend 64 tasks before they drain their records and fold -- three full passes of
the fold for 64 one-pixel tasks -- and run two iterations of a shadow walk in place (svr_lanes.hpp, SVR_SHADOW_FIRST = 2); every other queue build
and the local-majorant pools keep 32 tasks, in the front of slices that are allocated for the largest form.  Scheduling only: accumulator and
image are the oracle's bit for bit in the production and the counting build, the counting build traces pixels x frames paths, and its taps,
iterations, scatter events and shadow walks are the oracle's.

A wave pends more than 64 tasks only when the launch has more than 64 tasks per wave: with SVR_OPT_BLOCKS_PER_CU = 1 the launcher starts at most
num_cus x 4 / 16 blocks of 16 waves, and an image of at least 1.25 x 64 x waves pixels in one 64-frame call (one pixel per task) gives, by
pigeonhole, some wave a full drain of 64 tasks and then a partial one.  The DIRECT form runs only in batches of frames traced ahead of
per-frame calls, so its case makes such calls at that shape until a 64-frame batch is traced and consumed.  The small shapes put the fold's
item counts around its pass boundaries (21 tasks x 3 channels = 63 items, 22 -> 66, 43 -> 129, 64 -> 192), in windows through the head -- on a
tiny image most waves get one task, so these mostly check the windows themselves -- and two pixels per task with dead frame lanes."""
import functools
import re

import numpy as np
import pytest

from oracle import binding
from sunvolumerender_amd import abi, host, scenes
from tests.util import ORACLE_THREADS, assert_bit_exact, hip_frames, oracle_frames

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


def _check(dev, name, W, H, depth, nframes, what, rows=None, cols=None, ref=None, **kw):
    """production + counting build (hip_frames compares the two) against the oracle (ref: its result where the caller has it already)"""
    sc = _scene(name, W, H, depth)
    ref_hdr, ref_img, ref_c = ref or _oracle(name, W, H, depth, nframes, kw.get("window"))
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


def _many_tasks_shape(dev):
    """width x height with at least 1.25 x 64 tasks for every wave of a launch at one block per CU: 320 x 256 on 256 CUs"""
    num_cus = int(re.search(r"CUs=(\d+)", dev.info()).group(1))
    waves = num_cus * 4 // 16 * 16
    W = 320
    H = -(-(5 * 64 * waves // 4) // W)
    assert W * H >= 1.25 * 64 * waves
    return W, H


AHEAD_CALLS = 127      # per-frame calls after which the first 64-frame batch traced ahead (frames 63 .. 126) is folded whole


@functools.lru_cache(maxsize=None)
def _oracle_many_tasks(W, H):
    """The oracle on small_head at the many-tasks shape after 64 and after AHEAD_CALLS frames, {frames: (accumulator, image, counters)}: ONE
    progressive run (most of the time of this file), shared by the cases at that shape and never written to."""
    o = binding.OracleScene(_scene("small_head", W, H, 1))
    hdr = o.new_hdr()
    img = np.zeros((o.H, o.W, 4), dtype=np.uint8)
    total, out = None, {}
    for f in range(AHEAD_CALLS):
        c = o.render_pathtracer(hdr, f, img=img, nthreads=ORACLE_THREADS)
        total = c if total is None else {k: total[k] + c[k] for k in c}
        if f + 1 in (64, AHEAD_CALLS):
            snap = (hdr.copy(), img.copy(), dict(total))
            snap[0].setflags(write=False)
            snap[1].setflags(write=False)
            out[f + 1] = snap
    return out


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


def test_wave_pends_more_than_64_tasks(hip_dev):
    """(1) a full 64-task drain with a three-pass fold, then a partial one, in some wave"""
    W, H = _many_tasks_shape(hip_dev)
    with _options(hip_dev, OPT_QUEUE=2, OPT_BLOCKS_PER_CU=1):
        c = _check(hip_dev, "small_head", W, H, 1, 64, f"small_head {W} x {H}, 64 frames, 1 block per CU", ref=_oracle_many_tasks(W, H)[64])
    assert c["shadow_walks"] > 0


@pytest.mark.parametrize("n", [21, 22, 43, 64])
def test_fold_items_around_pass_boundaries(hip_dev, n):
    """(2) windows of n pixels in one row, 64 frames: n one-pixel tasks, 3 n fold items.  The head covers columns 29 .. 33 of rows 1 .. 5 of this
    image; the windows are centred in row 3, so every one of them holds those pixels and their shadow walks."""
    W, H, row = 64, 8, 3
    x0 = (W - n) // 2
    with _options(hip_dev, OPT_QUEUE=2, OPT_BLOCKS_PER_CU=1):
        c = _check(hip_dev, "tiny_head", W, H, 1, 64, f"window of {n} pixels in row {row} from column {x0}", rows=(row, row + 1), cols=(x0, x0 + n),
                   window=(x0, row, x0 + n, row + 1))
    assert c["shadow_walks"] > 0


def test_two_pixels_per_task_dead_frame_lanes(hip_dev):
    """(2) 17 x 5 x 40 frames"""
    with _options(hip_dev, OPT_QUEUE=2, OPT_BLOCKS_PER_CU=1):
        c = _check(hip_dev, "tiny_head", 17, 5, 1, 40, "tiny_head 17 x 5, 40 frames")
    assert c["shadow_walks"] > 0


def test_direct_form_many_tasks(hip_dev):
    """(3) the DIRECT form at the shape of (1).  Only frames traced AHEAD of per-frame calls run it (svr_api_trace.hip, render_ahead: batches of
    16 frames and more, production build), so the calls are canvas.paint(): the batches are 1, 2, 4, 8 (straight-line), 16, 32 (DIRECT, four
    and two pixels per task, 20 and 40 tasks per wave), then 64 frames from frame 63 and from frame 127 (DIRECT,
    one pixel per task, 80 tasks per wave on average: full drains of 64 tasks, their records popped into the scratch slots, then partial
    ones).  AHEAD_CALLS = 127 calls fold every frame of the first 64-frame batch into the accumulator."""
    W, H = _many_tasks_shape(hip_dev)
    calls = AHEAD_CALLS
    sc = _scene("small_head", W, H, 1)
    ref_hdr, ref_img, ref_c = _oracle_many_tasks(W, H)[calls]
    assert ref_c["shadow_walks"] > 0
    canvas = host.Canvas(hip_dev, W, H)
    try:
        scenes.apply_to_canvas(sc, canvas)
        with _options(hip_dev, OPT_QUEUE=2, OPT_BLOCKS_PER_CU=1):
            canvas.ReStartRender()
            for _ in range(calls):
                canvas.paint()
            hip_dev.synchronize()
            assert_bit_exact(canvas.read_hdr(), ref_hdr, f"small_head {W} x {H}, {calls} per-frame calls, frames traced ahead, 1 block per CU")
            assert np.array_equal(canvas.read_img(), ref_img)
    finally:
        canvas.close()


def test_non_folding_launch_many_tasks(hip_dev):
    """(3) SVR_OPT_FOLD = 0 at the shape of (1): a 64-frame call that does not fold is two straight-line launches of 32 frames through the
    scratch slots -- no queue build runs; this holds the host path beside the queue allocation, the test above holds the DIRECT form"""
    W, H = _many_tasks_shape(hip_dev)
    with _options(hip_dev, OPT_QUEUE=2, OPT_BLOCKS_PER_CU=1, OPT_FOLD=0):
        _check(hip_dev, "small_head", W, H, 1, 64, f"small_head {W} x {H}, 64 frames, not folding", ref=_oracle_many_tasks(W, H)[64])


def test_calls_onto_one_accumulator(hip_dev):
    """(3) 13, 61 and 64 frames at 24 x 8: four pixels per task, then one; the later calls fold onto frame0 > 0"""
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


def test_deeper_build_keeps_32_tasks(hip_dev):
    """(4) depth 3"""
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    _check(hip_dev, "tiny_head", 24, 8, 3, 64, "tiny_head 24 x 8 x 64, depth 3")


def test_pooled_build_keeps_32_tasks(hip_dev):
    """(4) pooled primary walks"""
    hip_dev.set_option(abi.OPT_POOL, 2)
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    _check(hip_dev, "tiny_head_noisy", 24, 8, 1, 64, "tiny_head_noisy 24 x 8 x 64, pooled primary walks")


def test_build_without_skipping_keeps_32_tasks(hip_dev):
    """(4) SVR_OPT_EMPTY_SKIP = 0"""
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    _check(hip_dev, "tiny_head", 24, 8, 1, 64, "tiny_head 24 x 8 x 64, no empty-space skipping", empty_skip=False)


def test_local_majorant_pools_share_the_allocation(hip_dev):
    """(5) the record pool of the local-majorant kernel (21 tasks per batch, several full batches and a partial one per wave) in the rows and
    queue slices that are now allocated for 64 tasks, against its own straight-line form"""
    dev = hip_dev
    sc = scenes.make_scene("small_head", trace_depth=1)
    canvas = host.Canvas(dev, sc.width, sc.height)
    try:
        scenes.apply_to_canvas(sc, canvas)
        with _options(dev, OPT_BLOCKS_PER_CU=1, OPT_LM_TUNE=1 | (16 << 8) | (16 << 16) | (21 << 24)):

            def run(mode):
                dev.set_option(abi.OPT_LOCAL_MAJORANT, mode)
                canvas.ReStartRender()
                canvas.paint_frames(64, sync=True)
                return canvas.read_hdr(), canvas.read_img()

            ref, ref_img = run(2)
            hdr, img = run(1)
        assert ref.max() > 0
        assert_bit_exact(hdr, ref, "small_head depth 1, 21 tasks per batch, 1 block per CU: pools vs straight-line paths")
        assert np.array_equal(img, ref_img)
    finally:
        dev.set_option(abi.OPT_LOCAL_MAJORANT, 0)
        canvas.close()
