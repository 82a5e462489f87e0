"""The task loop of the persistent tile kernel (svr_trace_tile.hip: sharded tickets, pending tasks, the fold of a pixel's frames,
svr_tile_tasks.hpp) at the smallest shapes where it can go wrong.  Every unit of a launch must be traced exactly once and every pixel's
frames folded in order -- the accumulator is the oracle's bit for bit, in the production and the counting build, and the counting build's
`paths` is pixels x frames exactly: fewer tasks than waves, counters with unequal numbers of units, partial tiles, both ticket orders,
several tasks per ticket, windows, row shards, tile lists, every build of the kernel that shares the loop, and frame counts around the
fold's load chunk (FOLD_CHUNK = 8 samples loaded together, the rest one by one) on accumulators that already hold frames."""
import functools

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests.adaptive_ref import pixel_frames
from tests.util import assert_bit_exact, hip_frames, oracle_frames

pytestmark = pytest.mark.gpu

OPT_UNIT = 101          # svr_set_option key: tasks per ticket of the tile kernel (svr_api.hip; 0 = one)


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


def _check(dev, name, W, H, depth, nframes, what, rows=None, cols=None, **kw):
    """production + counting build (hip_frames compares the two) against the oracle: accumulator, walk counters, paths == pixels x frames"""
    sc = _scene(name, W, H, depth)
    ref_hdr, ref_img, ref_c = _oracle(name, W, H, depth, nframes, kw.get("window"))
    hdr, img, c = hip_frames(dev, sc, nframes, batch=True, **kw)
    ys = slice(*rows) if rows else slice(0, H)
    xs = slice(*cols) if cols else slice(0, W)
    assert_bit_exact(hdr[ys, xs], ref_hdr[ys, xs], what)
    n_px = (ys.stop - ys.start) * (xs.stop - xs.start)
    assert c["paths"] == n_px * nframes, f"{what}: {c['paths']} paths traced, {n_px} pixels x {nframes} frames asked for"
    if rows is None:
        assert np.array_equal(img[ys, xs], ref_img[ys, xs]), what
        assert c["vol_taps"] == ref_c["vol_taps"] and c["woodcock_iters"] == ref_c["woodcock_iters"] and c["scatter_events"] == ref_c["scatter_events"], what
    return c


# 8 x 8: 64 tasks of one pixel x 64 frames, most waves never get one; 24 x 8 and 17 x 5: the eight counters hold unequal numbers of units,
# 17 x 5 x 40 frames: two pixels per task, the last tile of a row and the last row are partial, 24 dead frame lanes
SHAPES = [(8, 8, 64), (24, 8, 64), (17, 5, 64), (17, 5, 40), (8, 8, 40)]


@pytest.mark.parametrize("queue", [0, 2], ids=["straight", "queue"])
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("W,H,nframes", SHAPES)
def test_every_unit_once(hip_dev, W, H, nframes, depth, queue):
    """The straight-line, QUEUE and DEPTH1 builds, folding launches."""
    hip_dev.set_option(abi.OPT_QUEUE, queue)
    _check(hip_dev, "tiny_head", W, H, depth, nframes, f"{W} x {H}, {nframes} frames, depth {depth}, queue {queue}")


@pytest.mark.parametrize("nan_guard", [0, 1])
@pytest.mark.parametrize("queue", [0, 2], ids=["straight", "queue"])
def test_fold_in_chunks_and_remainders(hip_dev, queue, nan_guard):
    """Folding launches of 13 (one chunk + 5), 61 (seven chunks + 5), 8 (one chunk), 9 and 64 frames onto one accumulator (frame0 > 0 from the
    second on): the running mean after 155 frames is the oracle's.  One and two pixels per task (64- and 13-frame launches), rows in LDS
    (straight-line build) and in global memory (QUEUE build); the NaN guard changes nothing where no sample is a NaN."""
    W, H = 17, 5
    sc = _scene("tiny_head", W, H, 1)
    calls = (13, 61, 8, 9, 64)
    ref_hdr, ref_img, _ = _oracle("tiny_head", W, H, 1, sum(calls))
    assert np.isfinite(ref_hdr).all()
    hip_dev.set_option(abi.OPT_QUEUE, queue)
    hip_dev.set_option(abi.OPT_NAN_GUARD, nan_guard)
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
            assert_bit_exact(canvas.read_hdr(), ref_hdr, f"calls of {calls} frames, queue {queue}, nan guard {nan_guard}, count {count}")
            assert np.array_equal(canvas.read_img(), ref_img)
        assert hip_dev.counters()["paths"] == W * H * sum(calls)
    finally:
        hip_dev.set_option(abi.OPT_COUNT, 0)
        canvas.close()


@pytest.mark.parametrize("W,H", [(24, 8), (17, 5)])
def test_non_folding_launch(hip_dev, W, H):
    """40 frames through the scratch slots + k_resolve: frame groups of 32 and 8, tasks of two pixels."""
    hip_dev.set_option(abi.OPT_FOLD, 0)
    _check(hip_dev, "tiny_head", W, H, 1, 40, f"{W} x {H}, 40 frames, not folding")


@pytest.mark.parametrize("row_order,unit", [(0, 0), (1, 0), (0, 3), (1, 3)])
@pytest.mark.parametrize("queue", [0, 2], ids=["straight", "queue"])
@pytest.mark.parametrize("W,H", [(24, 8), (17, 5)])
def test_ticket_orders_and_unit(hip_dev, W, H, queue, row_order, unit):
    try:
        hip_dev.set_option(abi.OPT_ROW_ORDER, row_order)
        hip_dev.set_option(OPT_UNIT, unit)
        hip_dev.set_option(abi.OPT_QUEUE, queue)
        _check(hip_dev, "tiny_head", W, H, 1, 64, f"{W} x {H}, row order {row_order}, {unit} tasks per ticket, queue {queue}")
    finally:
        hip_dev.set_option(abi.OPT_ROW_ORDER, 0)
        hip_dev.set_option(OPT_UNIT, 0)


@pytest.mark.parametrize("row_order", [0, 1])
def test_window(hip_dev, row_order):
    try:
        hip_dev.set_option(abi.OPT_ROW_ORDER, row_order)
        hip_dev.set_option(abi.OPT_QUEUE, 2)
        _check(hip_dev, "tiny_head", 24, 8, 1, 64, f"window, row order {row_order}", rows=(1, 6), cols=(3, 20), window=(3, 1, 20, 6))
    finally:
        hip_dev.set_option(abi.OPT_ROW_ORDER, 0)


@pytest.mark.parametrize("row_order", [0, 1])
def test_row_shard(hip_dev, row_order):
    """rank 1 of 3 with 16-row strips on a 16 x 48 image: rows 16 .. 31"""
    try:
        hip_dev.set_option(abi.OPT_ROW_ORDER, row_order)
        hip_dev.set_option(abi.OPT_QUEUE, 2)
        _check(hip_dev, "tiny_head", 16, 48, 1, 64, f"row shard, row order {row_order}", rows=(16, 32), shard=(16, 1, 3))
    finally:
        hip_dev.set_option(abi.OPT_ROW_ORDER, 0)


def test_pooled_primary_walks(hip_dev):
    hip_dev.set_option(abi.OPT_POOL, 2)
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    for W, H in ((24, 8), (17, 5)):
        _check(hip_dev, "tiny_head_noisy", W, H, 1, 64, f"pooled primary walks, {W} x {H}")


def test_frames_traced_ahead(hip_dev):
    """DIRECT builds: 70 per-frame calls, the frames traced ahead of the calls (batches 1, 2, 4 ... 32) into scratch slots."""
    W, H = 24, 8
    sc = _scene("tiny_head", W, H, 1)
    ref_hdr, ref_img, _ = _oracle("tiny_head", W, H, 1, 70)
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    canvas = host.Canvas(hip_dev, W, H)
    try:
        scenes.apply_to_canvas(sc, canvas)
        for _ in range(70):
            canvas.paint()
        hip_dev.synchronize()
        assert_bit_exact(canvas.read_hdr(), ref_hdr, "70 per-frame calls, frames traced ahead")
        assert np.array_equal(canvas.read_img(), ref_img)
    finally:
        canvas.close()


def _adaptive(dev, sc, target, count, rmse=False):
    cv = host.Canvas(dev, sc.width, sc.height)
    try:
        scenes.apply_to_canvas(sc, cv)
        cv.ReStartRender()
        dev.set_option(abi.OPT_COUNT, 1 if count else 0)
        dev.synchronize()
        dev.reset_counters()
        res = cv.paint_adaptive(target, 0, 1024)
        dev.synchronize()
        return res, cv.adaptive_tiles()[1 if rmse else 0].copy(), cv.read_hdr(), dev.counters()
    finally:
        dev.set_option(abi.OPT_COUNT, 0)
        cv.close()


def test_tile_list_with_one_and_three_tiles(hip_dev):
    """One adaptive call on 3 x 2 tiles (40 x 24 pixels: the right column and the lower row are partial, so no two tiles hold the same part
    of the head) whose launches run over tile lists of 3 tiles and of 1 tile: every tile is the uniform render of its own frame count (the
    oracle's), and the counting build traces exactly the call's samples.  The target is searched between the tiles' own noise estimates;
    the tile frame counts say how many tiles each launch of the call had."""
    W, H = 40, 24
    sc = _scene("tiny_head", W, H, 1)
    hip_dev.set_option(abi.OPT_QUEUE, 2)
    est = _adaptive(hip_dev, sc, 1e-9, False, rmse=True)[1].ravel()
    est = np.sort(est[np.isfinite(est) & (est > 0)])
    # an estimate falls like 1 / sqrt(frames): targets from below the smallest final estimate (1024 frames) up to the largest one at 4 frames
    found = None
    for t in np.geomspace(est[0] * 0.9, est[-1] * 18.0, 96):
        res, frames, hdr, _ = _adaptive(hip_dev, sc, float(t), False)
        active = {int((frames > c).sum()) for c in (4, 8, 16, 32, 64, 128, 256, 512)}
        if {1, 3} <= active:
            found = (float(t), res, frames, hdr)
            break
    assert found is not None, "no target gives launches with 3 and with 1 active tiles"
    t, res, frames, hdr = found
    print("target", t, "tile frames", frames.tolist())
    for n in np.unique(frames).tolist():
        ref = _oracle("tiny_head", W, H, 1, int(n))[0]
        sel = np.kron(frames == n, np.ones((16, 16), bool))[:H, :W]
        assert_bit_exact(hdr[sel], ref[sel], f"tiles with {n} frames")
    res_c, frames_c, hdr_c, cnt = _adaptive(hip_dev, sc, t, True)
    assert np.array_equal(frames_c, frames)
    assert_bit_exact(hdr_c, hdr, "counting build vs production build")
    assert cnt["paths"] == res_c.pixel_frames == res.pixel_frames == pixel_frames(frames, 0, H, W)


@pytest.mark.parametrize("queue", [0, 2], ids=["straight", "queue"])
def test_group_map_with_gaps(hip_dev, queue):
    """tiny_bone: the rays cross the skull twice with transparent space in between, so the primary walks leave an occupied stretch and ask
    the group's map for the next one, from every round of the map (1 pixel x 64 frames per task: shared whole-ray tests)."""
    hip_dev.set_option(abi.OPT_QUEUE, queue)
    _check(hip_dev, "tiny_bone", 32, 32, 1, 64, f"tiny_bone, queue {queue}")
