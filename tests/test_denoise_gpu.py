"""Denoised preview (SVR_OPT_DENOISE_PREVIEW, svr_render_guides, svr_denoise_to_ldr / svr_denoise_hdr) on the GPU: the guides
against a restatement from the oracle's primitives, the filter against a numpy restatement, exact pass-through, an untouched
accumulator, an actual reduction of noise, the guide cache, and the documented inert cases."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding
from sunvolumerender_amd import abi, host, scenes
from tests.denoise_ref import atrous_ref, guide_step, guides_ref, pixel_scale
from tests.util import ORACLE_THREADS, assert_bit_exact

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _reset_denoise(hip_dev):
    """conftest.py resets only the options it lists: put the preview and its parameters back after every test."""
    yield
    hip_dev.lib.svr_clear_error()
    hip_dev.set_option(abi.OPT_DENOISE_PREVIEW, 0)
    hip_dev.set_denoise_params()
    hip_dev.lib.svr_clear_error()


def _canvas(dev, sc):
    cv = host.Canvas(dev, sc.width, sc.height)
    scenes.apply_to_canvas(sc, cv)
    return cv


def _ldr(dev, cv, hdr_ptr, params=None):
    img = dev.malloc(cv.W * cv.H * 4)
    try:
        dev.denoise_to_ldr(img, hdr_ptr, cv.W, cv.H, params)
        return dev.to_host(img, (cv.H, cv.W, 4), np.uint8)
    finally:
        dev.free(img)


def _dn_hdr(dev, cv, hdr_ptr, params=None):
    out = dev.malloc(cv.W * cv.H * 12)
    try:
        dev.denoise_hdr(out, hdr_ptr, cv.W, cv.H, params)
        return dev.to_host(out, (cv.H, cv.W, 3), np.float32)
    finally:
        dev.free(out)


def _tonemap_frame(dev, hdr, w, h):
    buf, img = dev.malloc(w * h * 12), dev.malloc(w * h * 4)
    try:
        dev.to_device(buf, np.ascontiguousarray(hdr, dtype=np.float32))
        dev.check(dev.lib.svr_hdr_to_ldr_frame(C.c_void_p(img), C.c_void_p(buf), w, h))
        return dev.to_host(img, (h, w, 4), np.uint8)
    finally:
        dev.free(buf)
        dev.free(img)


# ---------------------------------------------------------------------------------------------------------------------
# 1. guides against the restatement from the oracle's primitives
# ---------------------------------------------------------------------------------------------------------------------
GUIDE_SCENES = [
    ("tiny_head", {}),
    ("tiny_bone", {}),
    ("tiny", {}),
    ("tiny_head", {"clip": ((-0.6, 0.9), (-1.0, 0.5), (-0.8, 1.0))}),
    ("tiny_head", {"density_scale": 0.45}),
]


@pytest.mark.parametrize("name,over", GUIDE_SCENES, ids=["tiny_head", "tiny_bone", "tiny", "tiny_head_clip", "tiny_head_ds"])
def test_guides_match_cpu_restatement(hip_dev, name, over):
    sc = scenes.make_scene(name, **over)
    ora = binding.OracleScene(sc)
    lib = binding.load()
    cv = _canvas(hip_dev, sc)
    try:
        got = {}
        for skip in (1, 0):
            hip_dev.set_option(abi.OPT_EMPTY_SKIP, skip)
            got[skip] = cv.read_guides()
        hip_dev.set_option(abi.OPT_EMPTY_SKIP, 1)
        vol = cv.deviceVolume
        h = guide_step((vol.bbox.invSize.x, vol.bbox.invSize.y, vol.bbox.invSize.z), sc.dim)
    finally:
        cv.close()
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), "guides differ with and without empty-space skipping"
    g = got[1]
    stride = 3
    n_hit = 0
    for y in range(0, sc.height, stride):
        for x in range((y // stride) % stride, sc.width, stride):
            ref = guides_ref(lib, ora.ptr, x, y, h)
            gp = g[y, x]
            if ref[7] == 0:
                assert np.array_equal(gp, ref), (x, y, gp, ref)
                continue
            n_hit += 1
            assert gp[7] != 0, (x, y, gp, ref)
            np.testing.assert_allclose(gp[[3, 4, 5, 6, 7]], ref[[3, 4, 5, 6, 7]], rtol=1e-5, atol=1e-7, err_msg=f"pixel {(x, y)}")
            np.testing.assert_allclose(gp[0:3], ref[0:3], rtol=0, atol=1e-4, err_msg=f"normal of pixel {(x, y)}")
    assert n_hit > 20


# ---------------------------------------------------------------------------------------------------------------------
# 2. the filter against the numpy restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,params", [("tiny_head", {}), ("tiny_bone", {"sigma_color": 0.5, "passes": 3})])
def test_filter_matches_numpy(hip_dev, name, params):
    sc = scenes.make_scene(name)
    cv = _canvas(hip_dev, sc)
    try:
        for _ in range(2):
            cv.paint()
        hip_dev.synchronize()
        hdr = cv.read_hdr()
        guides = cv.read_guides()
        p = hip_dev.denoise_params(**params)
        out = _dn_hdr(hip_dev, cv, int(cv.renderParams.hdrBuffer), p)
        img = _ldr(hip_dev, cv, int(cv.renderParams.hdrBuffer), p)
        ps = pixel_scale(cv.camera.tanFovxOverTwo, cv.H)
    finally:
        cv.close()
    ref = atrous_ref(hdr, guides, pix_scale=ps, **{k: getattr(p, k) for k in ("passes", "sigma_depth", "sigma_normal", "sigma_albedo",
                                                                               "sigma_opacity", "sigma_color")})
    fin = np.isfinite(ref)
    assert fin.mean() > 0.999
    np.testing.assert_allclose(out[fin], ref[fin], rtol=1e-5, atol=1e-6 * float(np.abs(ref[fin]).max()))
    # RGBA8: at most 1 code, in at most 0.1 % of the pixels -- against the library's own tone map (k_tonemap) of the numpy result
    ref8 = _tonemap_frame(hip_dev, np.where(fin, ref, 0.0).astype(np.float32), sc.width, sc.height)
    d = np.abs(img[..., :3].astype(np.int32) - ref8[..., :3].astype(np.int32))
    d = np.where(fin, d, 0)
    assert d.max() <= 1 and (d.max(axis=-1) > 0).mean() <= 1e-3, (d.max(), (d.max(axis=-1) > 0).mean())


# ---------------------------------------------------------------------------------------------------------------------
# 3. pass-through is exact;  4. the accumulator is untouched;  7. inert where documented
# ---------------------------------------------------------------------------------------------------------------------
def _run(dev, sc, nframes, preview, frame_ahead=1, batches=None, snap=(1, 4, 8, 16), setup=None):
    """render_pathtracer (or svr_render_pathtracer_frames in `batches`) with the preview at `preview` frames; hdr and img after
    each frame count in `snap`."""
    cv = _canvas(dev, sc)
    try:
        dev.set_option(abi.OPT_FRAME_AHEAD, frame_ahead)
        cv.SetDenoisePreview(preview)
        if setup:
            setup(cv)
        cv.ReStartRender()
        dev.check(dev.lib.svr_memset_device(C.c_void_p(cv.img), 0, cv.W * cv.H * 4))
        out = {}
        done = 0
        for n in (batches or [1] * nframes):
            if batches:
                cv.paint_frames(n)
            else:
                cv.paint()
            done += n
            if done in snap:
                dev.synchronize()
                out[done] = (cv.read_hdr(), cv.read_img())
        return out, cv.read_guides()
    finally:
        dev.set_option(abi.OPT_FRAME_AHEAD, 1)
        dev.lib.svr_set_row_shard(0, 0, 1)
        dev.lib.svr_set_render_window(0, 0, -1, -1)
        dev.set_option(abi.OPT_SKIP_TONEMAP, 0)
        cv.close()


def _oracle_snapshots(sc, snap):
    o = binding.OracleScene(sc)
    hdr = o.new_hdr()
    out = {}
    for f in range(max(snap)):
        o.render_pathtracer(hdr, f, nthreads=ORACLE_THREADS)
        if f + 1 in snap:
            out[f + 1] = hdr.copy()
    return out


@pytest.mark.parametrize("depth", [1, 3])
def test_accumulator_untouched_and_pass_through(hip_dev, depth):
    sc = scenes.make_scene("tiny_head", trace_depth=depth)
    ora = _oracle_snapshots(sc, (1, 4, 8, 16))
    for fa in (0, 1):
        off, _ = _run(hip_dev, sc, 16, 0, frame_ahead=fa)
        on, guides = _run(hip_dev, sc, 16, 8, frame_ahead=fa)
        bg = guides[..., 7] == 0
        assert bg.any() and (~bg).any()
        for n in (1, 4, 8, 16):
            assert_bit_exact(on[n][0], off[n][0], f"hdr after {n} frames, preview on vs off (frame ahead {fa})")
            assert_bit_exact(on[n][0], ora[n], f"hdr after {n} frames vs oracle (frame ahead {fa})")
            assert np.array_equal(on[n][1][bg], off[n][1][bg]), f"O == 0 pixels differ after {n} frames"
        assert not np.array_equal(on[4][1], off[4][1]), "the preview changed nothing"
        assert np.array_equal(on[16][1], off[16][1]), "frames past the preview are not the ordinary tone map"
    # svr_render_pathtracer_frames: 1 + 3 + 4 frames shown denoised, then 8 more in one launch
    off, _ = _run(hip_dev, sc, 16, 0, batches=[1, 3, 4, 8], snap=(1, 4, 8, 16))
    on, guides = _run(hip_dev, sc, 16, 8, batches=[1, 3, 4, 8], snap=(1, 4, 8, 16))
    bg = guides[..., 7] == 0
    for n in (1, 4, 8, 16):
        assert_bit_exact(on[n][0], off[n][0], f"batched hdr after {n} frames")
        assert_bit_exact(on[n][0], ora[n], f"batched hdr after {n} frames vs oracle")
        assert np.array_equal(on[n][1][bg], off[n][1][bg])
    assert not np.array_equal(on[8][1], off[8][1])
    assert np.array_equal(on[16][1], off[16][1])


@pytest.mark.parametrize("mode", ["shard", "window", "skip_tonemap"])
def test_inert_where_documented(hip_dev, mode):
    sc = scenes.make_scene("tiny_head")

    def setup(cv):
        if mode == "shard":
            hip_dev.check(hip_dev.lib.svr_set_row_shard(8, 0, 2))
        elif mode == "window":
            hip_dev.check(hip_dev.lib.svr_set_render_window(8, 4, 70, 60))
        else:
            hip_dev.set_option(abi.OPT_SKIP_TONEMAP, 1)

    off, _ = _run(hip_dev, sc, 4, 0, snap=(1, 4), setup=setup)
    on, _ = _run(hip_dev, sc, 4, 8, snap=(1, 4), setup=setup)
    for n in (1, 4):
        assert_bit_exact(on[n][0], off[n][0], f"{mode}: hdr")
        assert np.array_equal(on[n][1], off[n][1]), f"{mode}: image differs with the preview on"


# ---------------------------------------------------------------------------------------------------------------------
# 5. it actually denoises
# ---------------------------------------------------------------------------------------------------------------------
def _tm(hdr, exposure):
    return np.clip(1.0 - np.exp(-np.asarray(hdr, np.float64) * 16.0 * exposure), 0, None) ** 2.2


@pytest.mark.parametrize("name,depth", [("small_head", 1), ("small_head", 3), ("c2", 1)])
def test_denoise_reduces_error(hip_dev, name, depth):
    sc = scenes.make_scene(name, trace_depth=depth)
    cv = _canvas(hip_dev, sc)
    try:
        cv.ReStartRender()
        for _ in range(64):
            cv.paint_frames(64)
        hip_dev.synchronize()
        ref = cv.read_hdr().astype(np.float64)
        guides = cv.read_guides()
        fg = guides[..., 7] > 0
        lines = []
        for spp in (1, 4):
            cv.ReStartRender()
            cv.paint_frames(spp)
            hip_dev.synchronize()
            raw = cv.read_hdr().astype(np.float64)
            den = _dn_hdr(hip_dev, cv, int(cv.renderParams.hdrBuffer)).astype(np.float64)
            ok = np.isfinite(raw).all(-1) & np.isfinite(den).all(-1) & np.isfinite(ref).all(-1)
            e_raw = np.sqrt(np.mean((_tm(raw[ok], sc.exposure) - _tm(ref[ok], sc.exposure)) ** 2))
            e_den = np.sqrt(np.mean((_tm(den[ok], sc.exposure) - _tm(ref[ok], sc.exposure)) ** 2))
            h_raw = np.sqrt(np.mean((raw[ok] - ref[ok]) ** 2))
            h_den = np.sqrt(np.mean((den[ok] - ref[ok]) ** 2))
            m = fg & ok
            lum = np.array([0.2126, 0.7152, 0.0722])
            mean_ref, mean_den = float((ref[m] @ lum).mean()), float((den[m] @ lum).mean())
            lines.append(f"{name} depth {depth} {spp} spp: RMSE(tone-mapped) raw {e_raw:.5f} denoised {e_den:.5f} ratio {e_den / e_raw:.3f}; "
                         f"RMSE(hdr) ratio {h_den / h_raw:.3f}; mean lum O>0 ref {mean_ref:.5f} denoised {mean_den:.5f} "
                         f"({100 * (mean_den / mean_ref - 1):+.2f} %)")
            print(lines[-1])
            assert e_den <= 0.6 * e_raw, lines[-1]
            assert abs(mean_den / mean_ref - 1.0) <= 0.02, lines[-1]
    finally:
        cv.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the guide cache invalidates on what the guides depend on, and only on that
# ---------------------------------------------------------------------------------------------------------------------
def test_guide_cache(hip_dev):
    sc = scenes.make_scene("tiny_head")
    cv = _canvas(hip_dev, sc)
    try:
        def fresh():
            # a forced recomputation: the skipping mode is part of the key (and does not change the result)
            hip_dev.set_option(abi.OPT_EMPTY_SKIP, 0)
            g = cv.read_guides()
            hip_dev.set_option(abi.OPT_EMPTY_SKIP, 1)
            return g

        g0 = cv.read_guides()
        b = hip_dev.guide_builds()
        assert np.array_equal(cv.read_guides(), g0) and hip_dev.guide_builds() == b, "unchanged scene: recomputed"

        def changed(what, fn):
            before = cv.read_guides()
            fn()
            b0 = hip_dev.guide_builds()
            g = cv.read_guides()
            assert hip_dev.guide_builds() == b0 + 1, f"{what}: guides not recomputed"
            assert not np.array_equal(g, before), f"{what}: guides unchanged"
            assert np.array_equal(g.view(np.uint32), fresh().view(np.uint32)), f"{what}: cached guides differ from a fresh computation"

        cam = host.camera_setup((5.0, 3.0, cv.eyeDist), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), cv.fov, 0.0, 1.0, 1.0, cv.W, cv.H)
        changed("setup_camera", lambda: cv.SetCamera(cam))
        tf = np.array(sc.tf_rgba, dtype=np.float32, copy=True)
        tf[:, 0:3] = tf[:, 2::-1]
        tf[:, 3] *= 0.5
        changed("svr_update_tf_texture", lambda: hip_dev.check(hip_dev.lib.svr_update_tf_texture(
            C.c_uint64(cv.transferFunction.tex), tf.ctypes.data_as(C.c_void_p), tf.shape[0], 0)))
        changed("densityScale", lambda: cv.SetDensityScale(0.6))
        changed("clip planes", lambda: cv.SetClipPlane((-0.5, 1.0), (-1.0, 1.0), (-1.0, 0.7)))

        g1 = cv.read_guides()
        b1 = hip_dev.guide_builds()
        cv.SetAreaLights([scenes.default_light(sc.dim, sc.spacing)])
        cv.SetEnvLightBackground((0.2, 0.3, 0.4))
        cv.SetEnvLightMapTable(scenes.synthetic_env_map(64, 32))
        cv.SetEnvLightIntensity(2.0)
        assert np.array_equal(cv.read_guides(), g1)
        assert hip_dev.guide_builds() == b1, "a light / environment change recomputed the guides"
    finally:
        cv.close()


def test_preview_image_is_the_denoised_tone_map(hip_dev):
    """What render_pathtracer shows in preview frames is svr_denoise_to_ldr of its accumulator."""
    sc = scenes.make_scene("tiny_head")
    cv = _canvas(hip_dev, sc)
    try:
        hip_dev.set_denoise_params(sigma_albedo=0.3, passes=4)
        cv.SetDenoisePreview(4)
        for _ in range(3):
            cv.paint()
        hip_dev.synchronize()
        shown = cv.read_img()
        assert np.array_equal(shown, _ldr(hip_dev, cv, int(cv.renderParams.hdrBuffer)))
        assert hip_dev.get_denoise_params().passes == 4
    finally:
        cv.close()


def test_bad_arguments(hip_dev):
    with pytest.raises(host.SvrError):
        hip_dev.set_denoise_params(passes=0)
    with pytest.raises(host.SvrError):
        hip_dev.set_denoise_params(sigma_depth=-1.0)
    with pytest.raises(host.SvrError):
        hip_dev.set_option(abi.OPT_DENOISE_PREVIEW, -1)
    sc = scenes.make_scene("tiny")
    cv = _canvas(hip_dev, sc)
    try:
        with pytest.raises(host.SvrError):
            hip_dev.denoise_to_ldr(cv.img, int(cv.renderParams.hdrBuffer), cv.W + 1, cv.H)
    finally:
        cv.close()
