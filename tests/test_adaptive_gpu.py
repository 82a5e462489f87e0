"""Adaptive sampling (svr_render_pathtracer_adaptive, svr_get_adaptive_tiles) on the GPU: every pixel equals the uniform render of its tile's
frame count bit for bit (through every kernel the call can reach), frozen tiles are not traced, the freeze decisions replay from the estimates
of uniform renders (tests/adaptive_ref.py), the degenerate targets, errors that change nothing, and the quality of frozen tiles against a
4096-frame reference."""
import ctypes as C
import dataclasses
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import binding
from sunvolumerender_amd import abi, host, scenes
from tests.adaptive_ref import pixel_frames, replay, schedule
from tests.noise_ref import estimate_ref, measured_error, tile_sums
from tests.util import ORACLE_THREADS, assert_bit_exact, bits

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CAP = 128          # max_frames of the bit-exactness cases: checkpoints 8 .. 128, tile counts 16, 32, 64, 128


@pytest.fixture(autouse=True)
def _reset(hip_dev):
    yield
    hip_dev.lib.svr_clear_error()
    hip_dev.set_option(abi.OPT_NOISE_ESTIMATE, 0)
    hip_dev.lib.svr_clear_error()


def _canvas(dev, sc):
    cv = host.Canvas(dev, sc.width, sc.height)
    scenes.apply_to_canvas(sc, cv)
    return cv


def _options(dev, opts):
    for k, v in opts.items():
        dev.set_option(k, v)


def _uniform(dev, sc, counts, opts=None):
    """{n: accumulator} of one uniform render at the frame counts `counts` (ascending)."""
    cv = _canvas(dev, sc)
    try:
        _options(dev, opts or {})
        cv.ReStartRender()
        out, cur = {}, 0
        for n in counts:
            if n > cur:
                cv.paint_frames(n - cur)
                cur = n
            dev.synchronize()
            out[n] = cv.read_hdr()
        return out
    finally:
        cv.close()


def _adaptive(dev, sc, target, f0=0, min_frames=0, max_frames=CAP, opts=None, count=False):
    """(result, frames map, rmse map, accumulator, image, frameNo after the call, image re-tone-mapped from the accumulator, counters)"""
    cv = _canvas(dev, sc)
    try:
        _options(dev, opts or {})
        cv.ReStartRender()
        if f0:
            cv.paint_frames(f0)
        if count:
            dev.set_option(abi.OPT_COUNT, 1)
        dev.synchronize()
        dev.reset_counters()
        res = cv.paint_adaptive(target, min_frames, max_frames)
        dev.synchronize()
        cnt = dev.counters()
        frames, rmse = cv.adaptive_tiles()
        hdr, img = cv.read_hdr(), cv.read_img()
        frame_no = cv.renderParams.frameNo
        dev.check(dev.lib.svr_hdr_to_ldr(C.c_void_p(cv.img), C.byref(cv.renderParams)))
        dev.synchronize()
        return res, frames, rmse, hdr, img, frame_no, cv.read_img(), cnt
    finally:
        dev.set_option(abi.OPT_COUNT, 0)
        cv.close()


def _estimates(sc, uni):
    """estimate(m, n) for adaptive_ref.replay from uniform accumulators: (tile RMSE, counted pixels per tile)."""
    def est(m, n):
        ref = estimate_ref(uni[m], m, uni[n], n, sc.exposure)
        fin = np.isfinite(uni[m]).all(-1) & np.isfinite(uni[n]).all(-1)
        return ref["tiles"], np.rint(tile_sums(fin.astype(np.float64), sc.height, sc.width)).astype(np.int64)
    return est


def _pick_target(sc, uni, f0, cap, shape):
    """The target, between two estimated tile values, with the most distinct tile frame counts, then the widest margin to every estimate."""
    pts = schedule(f0, cap)
    est = _estimates(sc, uni)
    vals = np.unique(np.concatenate([est(m, n)[0].ravel() for m, n in zip(pts, pts[1:])]))
    vals = vals[np.isfinite(vals) & (vals > 0)]
    best = None
    for lo, hi in zip(vals, vals[1:]):
        t = float(np.sqrt(lo * hi))
        r = replay(f0, 0, cap, t, est, shape)
        key = (len(np.unique(r["frames"])), min(t / lo, hi / t))
        if best is None or key > best[0]:
            best = (key, t)
    return best[1]


def _tiles_equal(hdr, ref, frames, count, what):
    """the pixels of the tiles holding `count` frames: bit-identical in hdr and ref"""
    H, W = hdr.shape[:2]
    sel = np.kron(frames == count, np.ones((16, 16), bool))[:H, :W]
    assert sel.any()
    bad = (bits(hdr) != bits(ref)).any(-1) & sel
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels of the {count}-frame tiles differ from the uniform render"


def _near_target(est, pts, target, shape):
    """tiles whose estimate lies within 1e-4 relative of the target at some checkpoint (float32 vs float64 may decide them either way)"""
    near = np.zeros(shape, bool)
    for m, n in zip(pts, pts[1:]):
        r = est(m, n)[0]
        with np.errstate(invalid="ignore"):
            near |= np.abs(r / target - 1.0) <= 1e-4
    return near


def sun_map(w=128, h=64, sun=2000.0, sky=0.1):
    img = np.full((h, w, 4), sky, dtype=np.float32)
    img[..., 2] *= 1.5
    img[10:14, 20:24, :3] = np.array([sun, 0.9 * sun, 0.7 * sun], dtype=np.float32)
    img[..., 3] = 1.0
    return np.ascontiguousarray(img)


CASES = [
    ("tiny_head", 1, {}, 0),
    ("tiny_head", 3, {}, 0),
    ("tiny_head_noisy", 1, {}, 0),                                   # media without exactly transparent space: pooled primary walks
    ("tiny_bone", 1, {}, 0),
    ("tiny_head", 1, {abi.OPT_FOLD: 0}, 0),                           # scratch slots + k_resolve
    ("tiny_head", 3, {abi.OPT_SPLIT: 1}, 0),                          # the retired SVR_OPT_SPLIT: changes nothing
    ("tiny_head", 2, {abi.OPT_LOCAL_MAJORANT: 1}, 0),                 # local-majorant pools (against their own uniform render)
    ("tiny_head_env", 3, {abi.OPT_ENV_NEE: 1}, 0),                    # env-map importance sampling (against its own uniform render)
    ("tiny_head", 1, {}, 8),                                          # f0 > 0: on from a uniform 8-frame accumulator
]


@pytest.mark.parametrize("name,depth,opts,f0", CASES, ids=[f"{n}-d{d}-{'-'.join(str(k) for k in o) or 'default'}-f{f}" for n, d, o, f in CASES])
def test_bit_exact_and_decisions(hip_dev, name, depth, opts, f0):
    if name == "tiny_head_env":
        sc = dataclasses.replace(scenes.make_scene("tiny_head", trace_depth=depth), env_map=sun_map(), env_intensity=1.0, env_on_escape=True)
    else:
        sc = scenes.make_scene(name, trace_depth=depth)
    H, W = sc.height, sc.width
    shape = (-(-H // 16), -(-W // 16))
    pts = schedule(f0, CAP)
    uni = _uniform(hip_dev, sc, sorted(set(([f0] if f0 else []) + pts + [f0 + CAP])), opts)
    target = _pick_target(sc, uni, f0, CAP, shape)
    res, frames, rmse, hdr, img, frame_no, img_again, _ = _adaptive(hip_dev, sc, target, f0=f0, opts=opts)
    what = f"{name} depth {depth} {opts} f0 {f0} target {target:.6g}"
    counts = sorted(np.unique(frames).tolist())
    print(what, "tile counts", {c: int((frames == c).sum()) for c in counts}, "checkpoints", res.checkpoints)
    assert len(counts) >= 3, (what, counts)
    # 1. every tile equals the uniform render of its frame count, bit for bit
    for c in counts:
        _tiles_equal(hdr, uni[c], frames, c, what)
    if name == "tiny_head" and depth == 1 and not opts and f0 == 0:
        o = binding.OracleScene(sc)
        ora = o.new_hdr()
        for f in range(max(counts)):
            o.render_pathtracer(ora, f, nthreads=ORACLE_THREADS)
            if f + 1 in counts:
                _tiles_equal(hdr, ora, frames, f + 1, what + " (oracle)")
    assert np.array_equal(img, img_again), "the image is not the tone map of the final accumulator"
    # the result fields
    assert (res.tiles_x, res.tiles_y) == (shape[1], shape[0])
    assert res.frames_max == frames.max() == frame_no and res.frames_min == frames.min()
    assert res.pixel_frames == pixel_frames(frames, f0, H, W)
    # 3. the freeze decisions and the final estimates, replayed from the uniform renders
    est = _estimates(sc, uni)
    ref = replay(f0, 0, CAP, target, est, shape)
    near = _near_target(est, pts, target, shape)
    assert not near.all()
    assert np.array_equal(frames[~near], ref["frames"][~near]), (what, frames, ref["frames"])
    if not near.any():
        assert res.checkpoints == ref["checkpoints"] and res.tiles_active == int(ref["active"].sum())
        assert np.array_equal(np.isnan(rmse), np.isnan(ref["tile_rmse"]))
        fin = ~np.isnan(rmse)
        # (1e-4 relative; tiles of near-black background estimate ~1e-5 from float32 tone curves of tiny values, which differ from float64 by
        # up to 2e-9 absolute: atol 1e-6 = 1/4000 of a code value)
        np.testing.assert_allclose(rmse[fin], ref["tile_rmse"][fin], rtol=1e-4, atol=1e-6)
        assert res.pixels == ref["pixels"]
        assert abs(res.sse / ref["sse"] - 1) <= 1e-4 and abs(res.rmse / ref["rmse"] - 1) <= 1e-4, (res.sse, ref["sse"], res.rmse, ref["rmse"])
        assert abs(res.tile_max / ref["tile_max"] - 1) <= 1e-4
    if name == "tiny_head" and depth == 1 and not opts and f0 == 0:
        # 2. frozen tiles are not traced: the path counter of the counting build is the call's sample count
        res_c, frames_c, _, hdr_c, _, _, _, cnt = _adaptive(hip_dev, sc, target, count=True)
        assert np.array_equal(frames_c, frames)
        assert_bit_exact(hdr_c, hdr, "counting build vs production build")
        assert cnt["paths"] == res_c.pixel_frames == res.pixel_frames
        assert res.pixel_frames < H * W * (res.frames_max - f0)


def test_degenerate_targets(hip_dev):
    sc = scenes.make_scene("tiny_head")
    H, W = sc.height, sc.width
    # a target below every tile's error: a uniform render of max_frames, bit for bit
    res, frames, _, hdr, _, frame_no, _, _ = _adaptive(hip_dev, sc, 1e-9, max_frames=40)
    assert (frames == 40).all() and res.frames_max == res.frames_min == frame_no == 40
    assert res.tiles_active == frames.size and res.checkpoints == 3 and res.pixel_frames == 40 * H * W
    assert_bit_exact(hdr, _uniform(hip_dev, sc, [40])[40], "target 1e-9 vs paint_frames(40)")
    # the same from a uniform 8-frame accumulator
    res, frames, _, hdr, _, frame_no, _, _ = _adaptive(hip_dev, sc, 1e-9, f0=8, max_frames=40)
    assert (frames == 48).all() and frame_no == 48 and res.pixel_frames == 40 * H * W
    assert_bit_exact(hdr, _uniform(hip_dev, sc, [48])[48], "f0 8, target 1e-9 vs paint_frames(48)")
    # a huge target: everything freezes at the earliest checkpoint that allows it
    res, frames, _, _, _, frame_no, _, _ = _adaptive(hip_dev, sc, 1e9, max_frames=4096)
    assert (frames == 16).all() and res.frames_max == frame_no == 16 and res.tiles_active == 0 and res.checkpoints == 2
    res, frames, _, hdr, _, frame_no, _, _ = _adaptive(hip_dev, sc, 1e9, min_frames=64, max_frames=4096)
    assert (frames == 64).all() and res.frames_max == frame_no == 64 and res.tiles_active == 0 and res.checkpoints == 4
    assert_bit_exact(hdr, _uniform(hip_dev, sc, [64])[64], "min_frames 64 vs paint_frames(64)")


def test_get_adaptive_tiles_before_any_call():
    """a fresh process: svr_get_adaptive_tiles fails before the first adaptive call"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from sunvolumerender_amd import abi\n"
            "lib = abi.load()\n"
            "lib.svr_set_error_mode(0)\n"
            "assert lib.svr_init(0) == 0\n"
            "rc = lib.svr_get_adaptive_tiles(None, None)\n"
            "print('rc', rc, lib.svr_last_error().decode())\n"
            "lib.svr_shutdown()\n"
            "sys.exit(0 if rc != 0 else 3)\n") % str(ROOT)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert res.returncode == 0, res.stdout + res.stderr
    assert "before any" in res.stdout


def test_errors_change_nothing(hip_dev):
    sc = scenes.make_scene("tiny_head")
    cv = _canvas(hip_dev, sc)
    lib = hip_dev.lib
    W, H = sc.width, sc.height
    try:
        cv.ReStartRender()
        cv.paint_frames(8)
        hip_dev.synchronize()
        before, img_before = cv.read_hdr(), cv.read_img()
        rp = cv.renderParams
        out = abi.AdaptiveResult()

        def refused(target=0.01, min_frames=0, max_frames=64, what=""):
            rc = lib.svr_render_pathtracer_adaptive(C.c_void_p(cv.img), C.byref(rp), C.c_float(target), min_frames, max_frames, C.byref(out))
            assert rc == -6, (what, rc)
            assert lib.svr_last_error_code() != 0
            lib.svr_clear_error()
            hip_dev.synchronize()
            assert rp.frameNo == 8, what
            assert np.array_equal(bits(cv.read_hdr()), bits(before)), f"{what}: the accumulator changed"
            assert np.array_equal(cv.read_img(), img_before), f"{what}: the image changed"

        hip_dev.check(lib.svr_set_row_shard(16, 0, 2))
        refused(what="row shard")
        hip_dev.check(lib.svr_set_row_shard(0, 0, 1))
        hip_dev.check(lib.svr_set_render_window(0, 0, W // 2, H))
        refused(what="window")
        hip_dev.check(lib.svr_set_render_window(0, 0, -1, -1))
        for k in (abi.KERNEL_PIXEL, abi.KERNEL_ULOOP, abi.KERNEL_WAVEFRONT):
            hip_dev.set_option(abi.OPT_KERNEL, k)
            refused(what=f"kernel {k}")
        hip_dev.set_option(abi.OPT_KERNEL, abi.KERNEL_AUTO)
        for t in (0.0, -0.01, float("nan"), float("inf")):
            refused(target=t, what=f"target {t}")
        refused(max_frames=0, what="max_frames 0")
        refused(max_frames=0xFFFFFFFF - 7, what="f0 + max_frames = 2^32")
        # still usable: from f0 = 8 the snapshot is at 9, the estimates at 18 and 36, so a huge target freezes every tile at 36
        res = cv.paint_adaptive(1e9, 0, 64)
        assert res.frames_max == res.frames_min == rp.frameNo == 36
    finally:
        cv.close()


def test_tile_maps_and_estimator_state_afterwards(hip_dev):
    sc = scenes.make_scene("tiny_head")
    cv = _canvas(hip_dev, sc)
    lib = hip_dev.lib
    try:
        cv.ReStartRender()
        res = cv.paint_adaptive(1e9, 0, 4096)
        assert res.frames_max == 16
        n = res.tiles_x * res.tiles_y
        small = hip_dev.malloc(4 * (n - 1))
        try:
            assert lib.svr_get_adaptive_tiles(C.c_void_p(small), None) != 0
            lib.svr_clear_error()
            assert lib.svr_get_adaptive_tiles(None, C.c_void_p(small)) != 0
            lib.svr_clear_error()
        finally:
            hip_dev.free(small)
        hip_dev.check(lib.svr_get_adaptive_tiles(None, None))
        frames, rmse = cv.adaptive_tiles()
        assert (frames == 16).all() and rmse.shape == frames.shape
        # the estimator follows no render afterwards: a plain call starts a new one (snapshot first, no estimate yet)
        cv.SetNoiseEstimate(True)
        assert cv.noise_estimate().frames == 0
        cv.paint_frames(8)
        assert cv.noise_estimate().frames == 0
        cv.paint_frames(24)
        est = cv.noise_estimate()
        assert (est.frames, est.frames_ref) == (48, 24)
        # and a restarted render is the uniform render
        cv.ReStartRender()
        cv.paint_frames(32)
        hip_dev.synchronize()
        assert_bit_exact(cv.read_hdr(), _uniform(hip_dev, sc, [32])[32], "plain render after an adaptive call")
    finally:
        cv.close()


def test_quality_of_frozen_tiles(hip_dev):
    """small_head, depth 1, T = 0.02: the 95th percentile of the measured tile RMSE of the frozen tiles (against a 4096-frame uniform render)
    is <= 2 T."""
    sc = scenes.make_scene("small_head", trace_depth=1)
    T = 0.02
    ref = _uniform(hip_dev, sc, [4096])[4096]
    res, frames, rmse, hdr, _, _, _, _ = _adaptive(hip_dev, sc, T, max_frames=4096)
    e2, ok = measured_error(hdr, ref, sc.exposure)
    meas = np.sqrt(tile_sums(e2, sc.height, sc.width) / np.maximum(tile_sums(ok.astype(np.float64), sc.height, sc.width), 1))
    frozen = frames < 4096 if res.tiles_active else np.ones(frames.shape, bool)
    p95 = float(np.percentile(meas[frozen], 95))
    print(f"small_head depth 1 T {T}: {int(frozen.sum())} of {frames.size} tiles frozen, counts "
          f"{ {int(c): int((frames == c).sum()) for c in np.unique(frames)} }, measured tile RMSE of frozen tiles p50 "
          f"{float(np.percentile(meas[frozen], 50)):.5f} p95 {p95:.5f} max {float(meas[frozen].max()):.5f}; predicted tile max {res.tile_max:.5f}; "
          f"samples {res.pixel_frames} = {res.pixel_frames / (sc.width * sc.height * 4096):.3f} of uniform 4096")
    assert frozen.any()
    assert p95 <= 2 * T
