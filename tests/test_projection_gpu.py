"""svr_render_projection on the GPU: every image is IDENTICAL (RGBA8, tolerance 0) to the test-side reference
(tests/projection_ref.py), which implements the contract of include/svr_abi.h literally on the CPU oracle's primitives and
skips nothing."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import projection_ref as pr

pytestmark = pytest.mark.gpu

# raycast_steps / vol_taps / vol_taps_executed of tiny_head with skipping on, per view, macro shift and mode, recorded from the kernels before
# k_project and k_hits were put on one march (svr_march.hpp): sums of per-ray integers, so they are deterministic
SKIP_COUNTS = json.loads((Path(__file__).parent / "golden" / "viewer_skip_counts.json").read_text())
COUNTERS = ("raycast_steps", "vol_taps", "vol_taps_executed")

MODES = ((pr.MIP, "mip"), (pr.MEAN, "mean"), (pr.ISO, "iso"))
FILL = 0xAB                                          # images start as this byte: untouched pixels keep it
# ISO levels per volume: skin-like / bone-like for the head phantoms (air 0, soft tissue ~0.2-0.3, bone up to 0.72)
LEVELS = {"tiny_head": (0.15, 0.5), "tiny_bone": (0.15, 0.5), "tiny_head_noisy": (0.15, 0.5), "tiny": (0.3, 0.7)}
WINDOW = (0.05, 0.6)                                 # grey window of MIP / MEAN in the tests


class Rig:
    """A canvas with a scene applied; renders projections into an image pre-filled with FILL."""

    def __init__(self, dev, scene, layout=abi.LAYOUT_AUTO, step=None):
        self.dev, self.sc = dev, scene
        self.canvas = host.Canvas(dev, scene.width, scene.height)
        scenes.apply_to_canvas(scene, self.canvas, layout)
        if step is not None:
            self.canvas.stepSize = float(step)

    def render(self, mode, iso=0.5, window=WINDOW, color_tf=False, skip=1, count=False, shard=None, win=None):
        dev, cv = self.dev, self.canvas
        dev.check(dev.lib.svr_memset_device(C.c_void_p(cv.img), FILL, cv.W * cv.H * 4))
        dev.set_option(abi.OPT_EMPTY_SKIP, skip)
        dev.set_option(abi.OPT_COUNT, 1 if count else 0)
        if shard is not None:
            dev.check(dev.lib.svr_set_row_shard(*shard))
        if win is not None:
            dev.check(dev.lib.svr_set_render_window(*win))
        dev.reset_counters()
        try:
            cv.paint_projection(mode, iso=iso, window=window, color_tf=color_tf, sync=True)
            return cv.read_img(), dev.counters()
        finally:
            dev.lib.svr_set_row_shard(0, 0, 1)
            dev.lib.svr_set_render_window(0, 0, -1, -1)
            dev.set_option(abi.OPT_EMPTY_SKIP, 1)
            dev.set_option(abi.OPT_COUNT, 0)

    def close(self):
        self.canvas.close()


def same(img, ref, what):
    if not np.array_equal(img, ref):
        d = np.argwhere((img != ref).any(axis=-1))
        y, x = d[0]
        raise AssertionError(f"{what}: {len(d)} of {img.shape[0] * img.shape[1]} pixels differ; first at x={x} y={y}: "
                             f"got {img[y, x].tolist()}, reference {ref[y, x].tolist()}")


def check_all_modes(rig, R, levels, what, colours=(False, True), **kw):
    """The three modes (ISO at every level) x colours of `rig` against the reference R; returns the reference ISO infos."""
    step = rig.canvas.stepSize
    infos = []
    for mode, mname in MODES:
        for iso in (levels if mode == pr.ISO else (0.5,)):
            for col in colours:
                ref, _, info = R.image(mode, step, iso=iso, window=WINDOW, color_tf=col)
                img, _ = rig.render(mode, iso=iso, color_tf=col, **kw)
                same(img, ref, f"{what}, {mname}, iso {iso}, {'TF colour' if col else 'grey / white'}")
                if mode == pr.ISO and not col:
                    infos.append(info)
    return infos


# ------------------------------------------------------------------------------------------------ scenes x modes x colours
@pytest.mark.parametrize("name", ["tiny_head", "tiny_bone", "tiny_head_noisy", "tiny"])
def test_modes_scenes_colours(hip_dev, name):
    sc = scenes.make_scene(name)
    R = pr.reference(name, lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        infos = check_all_modes(rig, R, LEVELS[name], name)
        for lvl, ns in zip(LEVELS[name], infos):
            assert (ns >= 0).any() and (ns == -1).any(), f"{name}: level {lvl} must give surface and no-surface pixels"
        grey, _, _ = R.image(pr.MIP, sc.step_size(), window=WINDOW)
        tf, _, _ = R.image(pr.MIP, sc.step_size(), window=WINDOW, color_tf=True)
        assert not np.array_equal(grey, tf) and len(np.unique(grey[..., 0])) > 8
    finally:
        rig.close()


@pytest.mark.parametrize("layout", [abi.LAYOUT_LINEAR, abi.LAYOUT_BRICK, abi.LAYOUT_PAIR, abi.LAYOUT_CELL])
def test_layouts(hip_dev, layout):
    sc = scenes.make_scene("tiny_head")
    R = pr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc, layout=layout)
    try:
        check_all_modes(rig, R, (0.15,), f"layout {layout}", colours=(False,))
    finally:
        rig.close()


@pytest.mark.parametrize("shift", [0, 2])
def test_skip_on_off_and_counters(hip_dev, shift):
    """SVR_OPT_EMPTY_SKIP 1 and 0 give the same images and the reference's counts; with skipping on fewer fetches are issued
    (the air of tiny_head is exactly 0, so skippable samples exist in every mode)."""
    hip_dev.set_option(abi.OPT_MACRO_SHIFT_MIN, shift)
    sc = scenes.make_scene("tiny_head")
    R = pr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        for mode, mname in MODES:
            ref, rc, _ = R.image(mode, sc.step_size(), iso=0.15, window=WINDOW)
            for skip in (1, 0):
                img, c = rig.render(mode, iso=0.15, skip=skip, count=True)
                same(img, ref, f"{mname}, skip {skip}, counting build")
                img2, _ = rig.render(mode, iso=0.15, skip=skip, count=False)
                same(img2, ref, f"{mname}, skip {skip}")
                print(f"shift {shift} {mname} skip {skip}: steps {c['raycast_steps']} taps {c['vol_taps']} executed {c['vol_taps_executed']}")
                assert c["raycast_steps"] == rc["raycast_steps"] and c["vol_taps"] == rc["vol_taps"], (mname, skip, c, rc)
                if skip:
                    assert c["vol_taps_executed"] < c["vol_taps"], (mname, c)
                else:
                    assert c["vol_taps_executed"] == c["vol_taps"], (mname, c)
    finally:
        rig.close()


def skip_counts(dev, shift):
    """{mode name: {counter: value}} of tiny_head at 96 x 80, macro shift `shift`, skipping on: MIP, MEAN and ISO 0.15."""
    dev.set_option(abi.OPT_MACRO_SHIFT_MIN, shift)
    rig = Rig(dev, scenes.make_scene("tiny_head"))
    try:
        return {mname: {k: int(c[k]) for k in COUNTERS} for mode, mname in MODES for c in [rig.render(mode, iso=0.15, skip=1, count=True)[1]]}
    finally:
        rig.close()


@pytest.mark.parametrize("shift", [0, 2])
def test_skip_counts_are_the_recorded_ones(hip_dev, shift):
    """The skipping itself, not only its result: the verdict kept per macro-cell and the leaps pass exactly the samples they passed when
    the counts were recorded (test_skip_on_off_and_counters only asks for fewer fetches than without skipping)."""
    got = skip_counts(hip_dev, shift)
    print(f"shift {shift}: {got}")
    assert got == SKIP_COUNTS["projection"][f"shift{shift}"]


# ------------------------------------------------------------------------------------------------ geometry
def test_clip_planes_inside_the_volume(hip_dev):
    sc = scenes.make_scene("tiny_head", clip=((-0.5, 0.6), (-1.0, 1.0), (-0.7, 0.4)))
    R = pr.reference("tiny_head_clip", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        infos = check_all_modes(rig, R, (0.15, 0.5), "clip planes")
        assert all((ns == 0).any() for ns in infos), "the clip planes must cut tissue: cap pixels (n* = 0) in the reference"
        assert any((ns > 0).any() for ns in infos)
    finally:
        rig.close()


def _crop_scene():
    """An anisotropic, non-cubic crop of the head phantom: 40 x 56 x 48 voxels, spacing 1 / 0.8 / 1.3."""
    base = scenes.make_scene("tiny_head", n=64)
    vox = np.ascontiguousarray(base.vox[8:56, 4:60, 12:52])
    assert vox.shape == (48, 56, 40)
    spacing = (1.0, 0.8, 1.3)
    return scenes.make_scene("tiny_head", n=64, vox=vox, spacing=spacing, max_magnitude=scenes.max_gradient_magnitude(vox, spacing),
                             width=64, height=56)


def test_anisotropic_noncubic_crop(hip_dev):
    R = pr.reference("crop", _crop_scene)
    rig = Rig(hip_dev, R.scene)
    try:
        infos = check_all_modes(rig, R, (0.15, 0.5), "anisotropic crop")
        assert any((ns == 0).any() for ns in infos), "the crop cuts through tissue: cap pixels"
    finally:
        rig.close()


def test_camera_inside_the_volume(hip_dev):
    cam = host.camera_setup((3.0, 2.0, 5.0), (0.0, -4.0, -30.0), (0.0, 1.0, 0.0), 60.0, 0.0, 1.0, 1.0, 64, 48)
    sc = scenes.make_scene("tiny_head", camera=cam, width=64, height=48)
    R = pr.reference("inside", lambda: sc)
    rays = R.rays(sc.step_size())
    assert all(r is not None and r.ts[0] < 0 for row in rays for r in row), "every ray starts behind the eye, inside the box"
    rig = Rig(hip_dev, sc)
    try:
        check_all_modes(rig, R, (0.15, 0.5), "camera inside")
    finally:
        rig.close()


def _long_scene():
    """40 x 40 x 600 voxels: the macro grid (cells of 2 voxels) has 300 cells along z."""
    base = scenes.make_scene("tiny_head")
    slab = base.vox[:, 4:44, 4:44]
    vox = np.ascontiguousarray(np.concatenate([slab] * 13, axis=0)[:600])
    assert vox.shape == (600, 40, 40)
    cam = host.camera_setup((260.0, 90.0, 420.0), (0.0, 0.0, 60.0), (0.0, 1.0, 0.0), 75.0, 0.0, 1.0, 1.0, 40, 32)
    return scenes.make_scene("tiny_head", vox=vox, max_magnitude=scenes.max_gradient_magnitude(vox), camera=cam, width=40, height=32)


def test_elongated_volume_macro_grid_above_64(hip_dev):
    hip_dev.set_option(abi.OPT_MACRO_SHIFT_MIN, 0)
    R = pr.reference("long", _long_scene)
    rig = Rig(hip_dev, R.scene)
    try:
        infos = check_all_modes(rig, R, (0.15, 0.5), "40 x 40 x 600")
        assert all((ns >= 0).any() and (ns < 0).any() for ns in infos)
    finally:
        rig.close()


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("step", [0.3, None, 10.0])
def test_step_sizes(hip_dev, step, shift):
    """Below a voxel, the default (the voxel's bounding-sphere radius), and above a macro-cell (h = 5 voxels; cells of 1 and 4)."""
    hip_dev.set_option(abi.OPT_MACRO_SHIFT_MIN, shift)
    sc = scenes.make_scene("tiny_head", width=48, height=40)
    R = pr.reference("tiny_head_48x40", lambda: sc)
    rig = Rig(hip_dev, sc, step=step)
    try:
        check_all_modes(rig, R, (0.15, 0.5), f"step {step}, macro shift {shift}", colours=(False,))
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------ shard, window, refusals, state
def test_row_shard_and_window(hip_dev):
    sc = scenes.make_scene("tiny_head")
    R = pr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        for mode, mname in MODES:
            ref, _, _ = R.image(mode, sc.step_size(), iso=0.15, window=WINDOW)
            parts = [rig.render(mode, iso=0.15, shard=(8, rank, 2))[0] for rank in (0, 1)]
            rows = np.arange(sc.height)
            for rank, img in enumerate(parts):
                own = (rows // 8) % 2 == rank
                same(img[own], ref[own], f"{mname}, rank {rank}: owned rows")
                assert np.all(img[~own] == FILL), f"{mname}, rank {rank}: rows of the other rank were written"
            x0, y0, x1, y1 = 21, 13, 70, 59
            img, _ = rig.render(mode, iso=0.15, win=(x0, y0, x1, y1))
            same(img[y0:y1, x0:x1], ref[y0:y1, x0:x1], f"{mname}: window")
            outside = np.ones(img.shape[:2], dtype=bool)
            outside[y0:y1, x0:x1] = False
            assert np.all(img[outside] == FILL), f"{mname}: pixels outside the window were written"
    finally:
        rig.close()


def test_refused_arguments_leave_the_image_alone(hip_dev):
    sc = scenes.make_scene("tiny")
    rig = Rig(hip_dev, sc)
    cv, lib = rig.canvas, hip_dev.lib
    try:
        hip_dev.check(lib.svr_memset_device(C.c_void_p(cv.img), FILL, cv.W * cv.H * 4))
        nan, inf = float("nan"), float("inf")
        P = abi.ProjectionParams

        def call(p=None, step=None, vol=None, img=True, null=None):
            args = [C.c_void_p(cv.img if img else 0), C.byref(vol if vol is not None else cv.deviceVolume), C.byref(cv.transferFunction),
                    C.byref(cv.camera), C.c_float(cv.stepSize if step is None else step), C.byref(p) if p is not None else None]
            if null is not None:
                args[null] = None
            rc = lib.svr_render_projection(*args)
            hip_dev.synchronize() if rc == 0 else None
            lib.svr_clear_error()
            return rc

        good = P(abi.PROJ_MIP, 0, 0.5, 0.0, 1.0)
        bad_vol = type(cv.deviceVolume).from_buffer_copy(cv.deviceVolume)
        bad_vol.densityScale = -1.0
        nan_vol = type(cv.deviceVolume).from_buffer_copy(cv.deviceVolume)
        nan_vol.densityScale = nan
        refused = {
            "null img": dict(p=good, img=False), "null volume": dict(p=good, null=1), "null tf": dict(p=good, null=2),
            "null camera": dict(p=good, null=3), "null params": dict(p=None),
            "mode 0": dict(p=P(0, 0, 0.5, 0.0, 1.0)), "mode 4": dict(p=P(4, 0, 0.5, 0.0, 1.0)), "flag 2": dict(p=P(abi.PROJ_ISO, 2, 0.5, 0.0, 1.0)),
            "step 0": dict(p=good, step=0.0), "step < 0": dict(p=good, step=-1.0), "step nan": dict(p=good, step=nan), "step inf": dict(p=good, step=inf),
            "iso nan": dict(p=P(abi.PROJ_ISO, 0, nan, 0.0, 1.0)), "iso inf": dict(p=P(abi.PROJ_ISO, 0, inf, 0.0, 1.0)),
            "window nan": dict(p=P(abi.PROJ_MIP, 0, 0.5, nan, 1.0)), "window inf": dict(p=P(abi.PROJ_MIP, 0, 0.5, 0.0, inf)),
            "window empty": dict(p=P(abi.PROJ_MIP, 0, 0.5, 0.5, 0.5)), "window reversed": dict(p=P(abi.PROJ_MEAN, 0, 0.5, 1.0, 0.0)),
            "densityScale < 0": dict(p=good, vol=bad_vol), "densityScale nan": dict(p=good, vol=nan_vol),
        }
        for what, kw in refused.items():
            assert call(**kw) != 0, f"{what} was accepted"
            assert np.all(cv.read_img() == FILL), f"{what}: the image was written"
        assert call(p=good) == 0
        assert not np.all(cv.read_img() == FILL)
    finally:
        rig.close()


def test_projection_leaves_no_state_behind(hip_dev):
    """render_raycasting and a path-traced frame are the same before and after projection calls."""
    sc = scenes.make_scene("tiny_head")
    rig = Rig(hip_dev, sc)
    cv = rig.canvas

    def snapshot():
        cv.SetRenderMode(host.Canvas.RENDER_MODE_RAYCASTING)
        cv.paint(sync=True)
        rc = cv.read_img()
        cv.SetRenderMode(host.Canvas.RENDER_MODE_PATHTRACER)
        cv.paint(sync=True)
        return rc, cv.read_hdr(), cv.read_img()

    try:
        before = snapshot()
        for mode, _ in MODES:
            rig.render(mode, iso=0.15, color_tf=True)
            rig.render(mode, iso=0.5, skip=0)
        after = snapshot()
        assert np.array_equal(before[0], after[0]), "render_raycasting changed"
        assert np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32)), "the path-traced frame changed"
        assert np.array_equal(before[2], after[2])
        assert before[0].any() and before[1].any()
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------ full size
@pytest.mark.parametrize("name", ["c3", "c3n"])
def test_full_size_window(hip_dev, name):
    """A 64 x 8 window through the middle of the 512^3 head at 1024^2, three modes, against the reference."""
    win = (480, 500, 544, 508)
    R = pr.reference(name + "_win", lambda: scenes.make_scene(name), window=win)
    sc = R.scene
    rig = Rig(hip_dev, sc)
    try:
        x0, y0, x1, y1 = win
        for mode, mname in MODES:
            for col in (False, True):
                ref, rc, info = R.image(mode, sc.step_size(), iso=0.15, window=WINDOW, color_tf=col)
                img, c = rig.render(mode, iso=0.15, color_tf=col, win=win, count=True)
                same(img[y0:y1, x0:x1], ref[y0:y1, x0:x1], f"{name}, {mname}, TF colour {col}")
                assert c["raycast_steps"] == rc["raycast_steps"] and c["vol_taps"] == rc["vol_taps"], (name, mname, c, rc)
                img, _ = rig.render(mode, iso=0.15, color_tf=col, win=win, skip=0)
                same(img[y0:y1, x0:x1], ref[y0:y1, x0:x1], f"{name}, {mname}, TF colour {col}, skipping off")
            if mode == pr.ISO:
                assert (info[y0:y1, x0:x1] > 0).any()
    finally:
        rig.close()
