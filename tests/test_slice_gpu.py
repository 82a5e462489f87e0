"""svr_render_slice / svr_render_slice_stack on the GPU: every image is IDENTICAL (RGBA8, tolerance 0, every pixel) to the test-side
reference (tests/slice_ref.py), which implements the contract of include/svr_abi.h literally on the CPU oracle's primitives and
skips nothing."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import slice_ref as sr

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MODES = ((None, "plane"), (sr.MIP, "slab mip"), (sr.MINIP, "slab minip"), (sr.MEAN, "slab mean"))
FILL = 0xAB                                          # images start as this byte: untouched pixels keep it
WINDOW = (0.05, 0.6)                                 # grey window in the tests


class Rig:
    """A canvas with a scene applied; renders slices into an image pre-filled with FILL."""

    def __init__(self, dev, scene, layout=abi.LAYOUT_AUTO):
        self.dev, self.sc = dev, scene
        self.canvas = host.Canvas(dev, scene.width, scene.height)
        scenes.apply_to_canvas(scene, self.canvas, layout)
        self.W, self.H = scene.width, scene.height

    def render(self, p, skip=1, count=False, shard=None, win=None):
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
            cv.paint_slice(p, sync=True)
            return cv.read_img(), dev.counters()
        finally:
            dev.lib.svr_set_row_shard(0, 0, 1)
            dev.lib.svr_set_render_window(0, 0, -1, -1)
            dev.set_option(abi.OPT_EMPTY_SKIP, 1)
            dev.set_option(abi.OPT_COUNT, 0)

    def stack(self, p, count, spacing, win=None):
        dev, cv = self.dev, self.canvas
        n = cv.W * cv.H * 4
        buf = dev.malloc(count * n)
        try:
            dev.check(dev.lib.svr_memset_device(C.c_void_p(buf), FILL, count * n))
            if win is not None:
                dev.check(dev.lib.svr_set_render_window(*win))
            cv.paint_slice_stack(buf, p, count, spacing, sync=True)
            return dev.to_host(buf, (count, cv.H, cv.W, 4), np.uint8)
        finally:
            dev.lib.svr_set_render_window(0, 0, -1, -1)
            dev.free(buf)

    def close(self):
        self.canvas.close()


def same(img, ref, what):
    if not np.array_equal(img, ref):
        d = np.argwhere((img != ref).any(axis=-1))
        y, x = d[0]
        raise AssertionError(f"{what}: {len(d)} of {img.shape[0] * img.shape[1]} pixels differ; first at x={x} y={y}: "
                             f"got {img[y, x].tolist()}, reference {ref[y, x].tolist()}")


def with_(p, thickness=None, step=None, mode=None, window=WINDOW, color_tf=False):
    q = abi.SliceParams.from_buffer_copy(p)
    if thickness is not None:
        q.thickness = thickness
    if step is not None:
        q.step = step
    if mode is not None:
        q.mode = mode
    q.window_lo, q.window_hi = window
    q.flags = abi.SLICE_COLOR_TF if color_tf else 0
    return q


def planes(rig, voxel):
    """(name, params) of the three axis planes (through tissue, off the voxel lattice) and two oblique planes: a 30 degree tilt about x,
    and a general one with irrational components.  The oblique images are partly outside the box."""
    out = []
    for axis, pos in ((0, 0.43), (1, 0.55), (2, 0.38)):
        out.append((f"axis {axis}", rig.canvas.slice_params_axis(axis, pos)))
    ext = max(d * s for d, s in zip(rig.sc.dim, rig.sc.spacing))
    px = 1.5 * ext / rig.W
    c30, s30 = float(np.cos(np.pi / 6)), float(np.sin(np.pi / 6))
    p = abi.SliceParams()
    rig.dev.lib.svr_slice_params_default(C.byref(p))
    p.center = abi.vec3(0.3 * voxel, -0.7 * voxel, 1.1 * voxel)
    p.u, p.v = abi.vec3(px, 0.0, 0.0), abi.vec3(0.0, -px * c30, px * s30)
    out.append(("tilt 30", p))
    q = abi.SliceParams.from_buffer_copy(p)
    a, b = np.array([np.sqrt(2.0), 1.0 / np.pi, -np.sqrt(3.0) / 2]), np.array([np.e / 7, -np.sqrt(5.0), 0.37])
    a /= np.linalg.norm(a)
    b -= a * np.dot(a, b)
    b /= np.linalg.norm(b)
    q.u, q.v = abi.vec3(*(px * 0.9 * a)), abi.vec3(*(px * 0.9 * b))
    q.center = abi.vec3(-2.1 * voxel, 1.3 * voxel, 0.45 * voxel)
    out.append(("general", q))
    return out


def check_modes(rig, R, p, what, thickness, step, colours=(False, True), **kw):
    """plane, slab MIP, MinIP, MEAN x colours of the plane p against the reference; returns the reference values M per mode."""
    Ms = {}
    for mode, mname in MODES:
        for col in colours:
            q = with_(p, thickness=0.0 if mode is None else thickness, step=step, mode=mode if mode is not None else sr.MIP, color_tf=col)
            ref, _, M = R.image(q, rig.W, rig.H)
            img, _ = rig.render(q, **kw)
            same(img, ref, f"{what}, {mname}, {'TF colour' if col else 'grey'}")
            Ms[mname] = M
    return Ms


# ------------------------------------------------------------------------------------------------ scenes x planes x modes x colours
@pytest.mark.parametrize("name", ["tiny_head", "tiny_bone", "tiny_head_noisy", "tiny"])
def test_axes_modes_scenes_colours(hip_dev, name):
    sc = scenes.make_scene(name)
    R = sr.reference(name, lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        for pname, p in planes(rig, 1.0)[:3]:
            Ms = check_modes(rig, R, p, f"{name}, {pname}", thickness=5.0, step=0.8)
            hit = ~np.isnan(Ms["plane"])
            assert hit.any() and len(np.unique(Ms["plane"][hit])) > 8, f"{name}, {pname}: the plane must cut the object"
            assert (Ms["slab mip"][hit] > Ms["slab minip"][hit]).any()
        p = with_(planes(rig, 1.0)[2][1])
        grey, _, _ = R.image(p, rig.W, rig.H)
        tf, _, _ = R.image(with_(p, color_tf=True), rig.W, rig.H)
        assert not np.array_equal(grey, tf) and len(np.unique(grey[..., 0])) > 8
    finally:
        rig.close()


def test_oblique_planes(hip_dev):
    sc = scenes.make_scene("tiny_head")
    R = sr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        for pname, p in planes(rig, 1.0)[3:]:
            Ms = check_modes(rig, R, p, pname, thickness=7.0, step=0.9)
            hit = ~np.isnan(Ms["slab mip"])
            assert hit.any() and (~hit).any(), f"{pname}: the image must lie partly outside the box"
            assert (~np.isnan(Ms["plane"]) != hit).any(), f"{pname}: slab pixels whose centre plane misses the box"
    finally:
        rig.close()


@pytest.mark.parametrize("layout", [abi.LAYOUT_LINEAR, abi.LAYOUT_BRICK, abi.LAYOUT_PAIR, abi.LAYOUT_CELL])
def test_layouts(hip_dev, layout):
    sc = scenes.make_scene("tiny_head")
    R = sr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc, layout=layout)
    try:
        for pname, p in (planes(rig, 1.0)[0], planes(rig, 1.0)[4]):
            check_modes(rig, R, p, f"layout {layout}, {pname}", thickness=5.0, step=0.8, colours=(False,))
    finally:
        rig.close()


@pytest.mark.parametrize("shift", [0, 2])
def test_skip_on_off_and_counters(hip_dev, shift):
    """SVR_OPT_EMPTY_SKIP 1 and 0 give the same images and the reference's counts; with skipping on, slab MIP issues fewer fetches
    than it counts (the air of tiny_head is exactly 0, and a maximum once found skips darker macro-cells)."""
    hip_dev.set_option(abi.OPT_MACRO_SHIFT_MIN, shift)
    sc = scenes.make_scene("tiny_head")
    R = sr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        for pname, p in (planes(rig, 1.0)[2], planes(rig, 1.0)[3]):
            for mode, mname in MODES:
                q = with_(p, thickness=0.0 if mode is None else 6.0, step=0.7, mode=mode if mode is not None else sr.MEAN)
                ref, rc, _ = R.image(q, rig.W, rig.H)
                for skip in (1, 0):
                    img, c = rig.render(q, skip=skip, count=True)
                    same(img, ref, f"{pname}, {mname}, skip {skip}, counting")
                    img2, _ = rig.render(q, skip=skip, count=False)
                    same(img2, ref, f"{pname}, {mname}, skip {skip}")
                    print(f"shift {shift} {pname} {mname} skip {skip}: steps {c['raycast_steps']} taps {c['vol_taps']} executed {c['vol_taps_executed']}")
                    assert c["raycast_steps"] == rc["raycast_steps"] and c["vol_taps"] == rc["vol_taps"], (mname, skip, c, rc)
                    assert c["vol_taps_executed"] <= c["vol_taps"]
                    if skip and mode == sr.MIP:
                        assert c["vol_taps_executed"] < c["vol_taps"], (mname, c)
                    if not skip:
                        assert c["vol_taps_executed"] == c["vol_taps"], (mname, c)
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------ geometry
def test_clip_members_inside_the_volume(hip_dev):
    sc = scenes.make_scene("tiny_head", clip=((-0.5, 0.6), (-1.0, 1.0), (-0.7, 0.4)))
    R = sr.reference("tiny_head_clip", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        full = sr.reference("tiny_head", lambda: scenes.make_scene("tiny_head"))
        for pname, p in planes(rig, 1.0):
            Ms = check_modes(rig, R, p, f"clip, {pname}", thickness=5.0, step=0.8, colours=(False,))
            if pname in ("tilt 30", "general"):
                unclipped = full.image(with_(p), rig.W, rig.H)[2]
                assert (np.isnan(Ms["plane"]) & ~np.isnan(unclipped)).any(), "the clip members must cut pixels off the plane"
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
    R = sr.reference("crop", _crop_scene)
    rig = Rig(hip_dev, R.scene)
    try:
        for pname, p in planes(rig, 1.0):
            Ms = check_modes(rig, R, p, f"anisotropic crop, {pname}", thickness=5.0, step=0.8)
            assert (~np.isnan(Ms["plane"])).any()
    finally:
        rig.close()


def _long_scene():
    """40 x 40 x 600 voxels: the macro grid (cells of 2 voxels) has 300 cells along z."""
    base = scenes.make_scene("tiny_head")
    slab = base.vox[:, 4:44, 4:44]
    vox = np.ascontiguousarray(np.concatenate([slab] * 13, axis=0)[:600])
    assert vox.shape == (600, 40, 40)
    return scenes.make_scene("tiny_head", vox=vox, max_magnitude=scenes.max_gradient_magnitude(vox), width=40, height=120)


def test_elongated_volume_macro_grid_above_64(hip_dev):
    hip_dev.set_option(abi.OPT_MACRO_SHIFT_MIN, 0)
    R = sr.reference("long", _long_scene)
    rig = Rig(hip_dev, R.scene)
    try:
        for pname, p in (planes(rig, 1.0)[0], planes(rig, 1.0)[1], planes(rig, 1.0)[4]):
            Ms = check_modes(rig, R, p, f"40 x 40 x 600, {pname}", thickness=9.0, step=1.1, colours=(False,))
            assert (~np.isnan(Ms["plane"])).any()
    finally:
        rig.close()


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("step", [0.3, 1.0, 10.0, 25.0])
def test_step_sizes(hip_dev, step, shift):
    """0.3 x, 1 x and 10 x the voxel edge in a slab of 20 voxels, and a step larger than the thickness (K = 1)."""
    hip_dev.set_option(abi.OPT_MACRO_SHIFT_MIN, shift)
    sc = scenes.make_scene("tiny_head", width=48, height=40)
    R = sr.reference("tiny_head_48x40", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        assert sr.sample_count(20.0, step) == {0.3: 67, 1.0: 21, 10.0: 3, 25.0: 1}[step]
        for pname, p in (planes(rig, 1.0)[1], planes(rig, 1.0)[3]):
            check_modes(rig, R, p, f"step {step}, macro shift {shift}, {pname}", thickness=20.0, step=step, colours=(False,))
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------ stack, shard, window, refusals, state
def test_stack_equals_single_calls(hip_dev):
    sc = scenes.make_scene("tiny_head")
    R = sr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc)
    f32 = np.float32
    try:
        for pname, p in (planes(rig, 1.0)[2], planes(rig, 1.0)[4]):
            q = with_(p, thickness=4.0, step=0.8, mode=sr.MEAN)
            spacing = 2.3
            imgs = rig.stack(q, 5, spacing)
            n = sr.normal(q.u, q.v)
            for k in range(5):
                ref, _, _ = R.image(q, rig.W, rig.H, k=k, spacing=spacing)
                same(imgs[k], ref, f"{pname}: slice {k} of the stack against the reference")
                one = abi.SliceParams.from_buffer_copy(q)
                if k:
                    off = f32(spacing) * f32(k)                   # the header's center_k, in float32
                    c = sr.vec(q.center)
                    one.center = abi.vec3(*(float(c[a] + n[a] * off) for a in range(3)))
                img, _ = rig.render(one)
                assert img.tobytes() == imgs[k].tobytes(), f"{pname}: slice {k} of the stack differs from the single call"
            assert not np.array_equal(imgs[0], imgs[4])
            x0, y0, x1, y1 = 21, 13, 70, 59
            part = rig.stack(q, 5, spacing, win=(x0, y0, x1, y1))
            outside = np.ones(part.shape[1:3], dtype=bool)
            outside[y0:y1, x0:x1] = False
            for k in range(5):
                same(part[k][y0:y1, x0:x1], imgs[k][y0:y1, x0:x1], f"{pname}: slice {k}, window")
                assert np.all(part[k][outside] == FILL), f"{pname}: slice {k}: pixels outside the window were written"
    finally:
        rig.close()


def test_row_shard_and_window(hip_dev):
    sc = scenes.make_scene("tiny_head")
    R = sr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        rows = np.arange(sc.height)
        for mode, mname in MODES:
            p = with_(planes(rig, 1.0)[4][1], thickness=0.0 if mode is None else 5.0, step=0.8, mode=mode if mode is not None else sr.MIP)
            ref, _, _ = R.image(p, rig.W, rig.H)
            for world in (2, 3):
                whole = np.full_like(ref, FILL)
                for rank in range(world):
                    img, _ = rig.render(p, shard=(8, rank, world))
                    own = (rows // 8) % world == rank
                    assert np.all(img[~own] == FILL), f"{mname}, rank {rank} of {world}: rows of another rank were written"
                    whole[own] = img[own]
                same(whole, ref, f"{mname}: {world} ranks' strips assembled")
            x0, y0, x1, y1 = 21, 13, 70, 59
            img, _ = rig.render(p, win=(x0, y0, x1, y1))
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
        base = with_(cv.slice_params_axis(2, 0.5), thickness=3.0, step=0.5, mode=sr.MIP, window=(0.0, 1.0))

        def P(**kw):
            q = abi.SliceParams.from_buffer_copy(base)
            for k, v in kw.items():
                setattr(q, k, abi.vec3(*v) if k in ("center", "u", "v") else v)
            return q

        def call(p=None, vol=None, img=True, null=None, w=None, h=None, count=None, spacing=0.0):
            args = [C.c_void_p(cv.img if img else 0), C.byref(vol if vol is not None else cv.deviceVolume), C.byref(cv.transferFunction),
                    cv.W if w is None else w, cv.H if h is None else h, C.byref(p) if p is not None else None]
            if null is not None:
                args[null] = None
            if count is None:
                rc = lib.svr_render_slice(*args)
            else:
                rc = lib.svr_render_slice_stack(*args, count, C.c_float(spacing))
            assert (rc != 0) == (lib.svr_last_error_code() != 0)
            hip_dev.synchronize() if rc == 0 else None
            lib.svr_clear_error()
            return rc

        bad_vol = type(cv.deviceVolume).from_buffer_copy(cv.deviceVolume)
        bad_vol.densityScale = -1.0
        nan_vol = type(cv.deviceVolume).from_buffer_copy(cv.deviceVolume)
        nan_vol.densityScale = nan
        refused = {
            "null img": dict(p=base, img=False), "null volume": dict(p=base, null=1), "null tf": dict(p=base, null=2), "null params": dict(p=None),
            "w 0": dict(p=base, w=0), "h 0": dict(p=base, h=0),
            "center nan": dict(p=P(center=(0.0, nan, 0.0))), "u inf": dict(p=P(u=(inf, 0.0, 0.0))), "v nan": dict(p=P(v=(0.0, 0.0, nan))),
            "thickness nan": dict(p=P(thickness=nan)), "thickness inf": dict(p=P(thickness=inf)), "step nan": dict(p=P(step=nan)),
            "step inf": dict(p=P(step=inf)), "step nan on a plane": dict(p=P(thickness=0.0, step=nan)),
            "u x v = 0 (parallel)": dict(p=P(u=(1.0, 0.0, 0.0), v=(-2.0, 0.0, 0.0))), "u = 0": dict(p=P(u=(0.0, 0.0, 0.0))),
            "thickness < 0": dict(p=P(thickness=-1.0)), "step 0": dict(p=P(step=0.0)), "step < 0": dict(p=P(step=-0.5)),
            "mode 0": dict(p=P(mode=0)), "mode 4": dict(p=P(mode=4)), "flag 2": dict(p=P(flags=2)),
            "window nan": dict(p=P(window_lo=nan)), "window inf": dict(p=P(window_hi=inf)), "window empty": dict(p=P(window_lo=0.5, window_hi=0.5)),
            "window reversed": dict(p=P(window_lo=1.0, window_hi=0.0)),
            "densityScale < 0": dict(p=base, vol=bad_vol), "densityScale nan": dict(p=base, vol=nan_vol),
            "count 0": dict(p=base, count=0), "spacing nan": dict(p=base, count=1, spacing=nan),
            "K above the cap": dict(p=P(thickness=4096.0, step=1.0)), "K far above the cap": dict(p=P(thickness=1e30, step=1e-30)),
        }
        for what, kw in refused.items():
            assert call(**kw) != 0, f"{what} was accepted"
            assert np.all(cv.read_img() == FILL), f"{what}: the image was written"
        # at the cap, a plane that ignores mode, and the plain call are accepted
        assert call(p=P(thickness=4095.0, step=1.0)) == 0
        assert call(p=P(thickness=0.0, mode=77, step=0.0)) == 0
        hip_dev.check(lib.svr_memset_device(C.c_void_p(cv.img), FILL, cv.W * cv.H * 4))
        assert call(p=base) == 0
        assert not np.all(cv.read_img() == FILL)
    finally:
        rig.close()


def test_refused_argument_in_fatal_error_mode():
    """Under svr_set_error_mode(1) a refused argument is reported and ends the process before anything is launched (the library's
    checkCudaErrors behaviour): a fresh process, which must die with the message and never reach the line after the call."""
    code = ("import sys, ctypes as C; sys.path.insert(0, %r)\n"
            "from sunvolumerender_amd import abi, host, scenes\n"
            "dev = host.Device(0, fatal_errors=False)\n"
            "sc = scenes.make_scene('tiny')\n"
            "cv = host.Canvas(dev, sc.width, sc.height)\n"
            "scenes.apply_to_canvas(sc, cv, 0)\n"
            "p = cv.slice_params_axis(2, 0.5)\n"
            "cv.paint_slice(p, sync=True)\n"
            "print('accepted', flush=True)\n"
            "dev.lib.svr_set_error_mode(1)\n"
            "p.window_hi = p.window_lo\n"
            "rc = dev.lib.svr_render_slice(C.c_void_p(cv.img), C.byref(cv.deviceVolume), C.byref(cv.transferFunction), cv.W, cv.H, C.byref(p))\n"
            "print('returned', rc, flush=True)\n") % str(ROOT)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert "accepted" in res.stdout and "returned" not in res.stdout, res.stdout + res.stderr
    assert res.returncode == 1 and "svr_render_slice: the window must be finite" in res.stderr, (res.returncode, res.stderr)


def test_slices_leave_no_state_behind(hip_dev):
    """render_raycasting, a projection and a path-traced frame are the same before and after slice calls."""
    sc = scenes.make_scene("tiny_head")
    rig = Rig(hip_dev, sc)
    cv = rig.canvas

    def snapshot():
        cv.SetRenderMode(host.Canvas.RENDER_MODE_RAYCASTING)
        cv.paint(sync=True)
        rc = cv.read_img()
        cv.paint_projection(abi.PROJ_MIP, sync=True)
        pj = cv.read_img()
        cv.SetRenderMode(host.Canvas.RENDER_MODE_PATHTRACER)
        cv.paint(sync=True)
        return rc, pj, cv.read_hdr(), cv.read_img()

    try:
        before = snapshot()
        for pname, p in planes(rig, 1.0):
            for mode, _ in MODES:
                rig.render(with_(p, thickness=0.0 if mode is None else 5.0, step=0.8, mode=mode or sr.MIP, color_tf=True))
                rig.render(with_(p, thickness=0.0 if mode is None else 5.0, step=0.8, mode=mode or sr.MIP), skip=0)
        rig.stack(with_(planes(rig, 1.0)[0][1]), 3, 1.5)
        after = snapshot()
        assert np.array_equal(before[0], after[0]), "render_raycasting changed"
        assert np.array_equal(before[1], after[1]), "svr_render_projection changed"
        assert np.array_equal(before[2].view(np.uint32), after[2].view(np.uint32)), "the path-traced frame changed"
        assert np.array_equal(before[3], after[3])
        assert before[0].any() and before[1].any() and before[2].any()
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------ full size
@pytest.mark.parametrize("name", ["c3", "c3n"])
def test_full_size_window(hip_dev, name):
    """A 64 x 8 window of an oblique 16-sample slab MIP through the 512^3 head at 1024^2 against the reference."""
    win = (480, 500, 544, 508)
    sc = scenes.make_scene(name)
    R = sr.reference(name, lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        x0, y0, x1, y1 = win
        p = with_(planes(rig, 1.0)[4][1], thickness=12.0, step=0.8, mode=sr.MIP)
        assert sr.sample_count(p.thickness, p.step) == 16
        for col in (False, True):
            q = with_(p, color_tf=col)
            ref, rc, M = R.image(q, rig.W, rig.H, window=win)
            assert len(np.unique(M[y0:y1, x0:x1])) > 16
            img, c = rig.render(q, win=win, count=True)
            same(img[y0:y1, x0:x1], ref[y0:y1, x0:x1], f"{name}, TF colour {col}")
            assert c["raycast_steps"] == rc["raycast_steps"] == 16 * 64 * 8 and c["vol_taps"] == rc["vol_taps"], (name, c, rc)
            img, _ = rig.render(q, win=win, skip=0)
            same(img[y0:y1, x0:x1], ref[y0:y1, x0:x1], f"{name}, TF colour {col}, skipping off")
    finally:
        rig.close()
