"""svr_render_hits and svr_pick on the GPU: every record of every pixel is IDENTICAL, bit for bit (the 40 bytes viewed as uint32), to
the test-side reference (tests/hit_ref.py), which implements the contract of include/svr_abi.h literally on the CPU oracle's
primitives and skips nothing.  Scenes and sizes are those of tests/test_projection_gpu.py (the references are shared with it)."""
import ctypes as C

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import hit_ref as hr
from tests.test_projection_gpu import COUNTERS, LEVELS, SKIP_COUNTS, _crop_scene, _long_scene

pytestmark = pytest.mark.gpu

MODES = ((hr.OPACITY, "opacity"), (hr.ISO, "iso"), (hr.MAX, "max"))
ALPHAS = (0.0, 0.5, 0.95)
FILL = 0xAB                                          # the records start as this byte: untouched entries keep it
FILL_WORD = 0xABABABAB


def words(rec):
    """svr_hit records as uint32 words, (..., 10)."""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(rec.shape + (10,))


class Rig:
    """A canvas with a scene applied, and a device buffer of W x H records pre-filled with FILL."""

    def __init__(self, dev, scene, layout=abi.LAYOUT_AUTO, step=None):
        self.dev, self.sc = dev, scene
        self.canvas = host.Canvas(dev, scene.width, scene.height)
        scenes.apply_to_canvas(scene, self.canvas, layout)
        if step is not None:
            self.canvas.stepSize = float(step)
        self.n = scene.width * scene.height
        self.buf = dev.malloc(self.n * 40)

    def fill(self):
        self.dev.check(self.dev.lib.svr_memset_device(C.c_void_p(self.buf), FILL, self.n * 40))

    def read(self, n=None):
        cv = self.canvas
        return self.dev.to_host(self.buf, (cv.H, cv.W) if n is None else (n,), hr.HIT_DTYPE)

    def raw(self, fn, *lead, p, step=None, vol=None, null=None):
        """fn(hits, *lead, volume, tf, camera, step, params) with the canvas's scene; returns the status, error cleared."""
        cv = self.canvas
        args = [C.c_void_p(self.buf), *lead, C.byref(vol if vol is not None else cv.deviceVolume), C.byref(cv.transferFunction),
                C.byref(cv.camera), C.c_float(cv.stepSize if step is None else step), C.byref(p) if p is not None else None]
        if null is not None:
            args[null] = None
        rc = fn(*args)
        if rc == 0:
            self.dev.synchronize()
        self.dev.lib.svr_clear_error()
        return rc

    def hits(self, mode, alpha=0.5, iso=0.5, skip=1, count=False, shard=None, win=None):
        dev = self.dev
        self.fill()
        dev.set_option(abi.OPT_EMPTY_SKIP, skip)
        dev.set_option(abi.OPT_COUNT, 1 if count else 0)
        if shard is not None:
            dev.check(dev.lib.svr_set_row_shard(*shard))
        if win is not None:
            dev.check(dev.lib.svr_set_render_window(*win))
        dev.reset_counters()
        try:
            assert self.raw(dev.lib.svr_render_hits, p=abi.HitParams(mode, alpha, iso)) == 0
            return self.read(), dev.counters()
        finally:
            dev.lib.svr_set_row_shard(0, 0, 1)
            dev.lib.svr_set_render_window(0, 0, -1, -1)
            dev.set_option(abi.OPT_EMPTY_SKIP, 1)
            dev.set_option(abi.OPT_COUNT, 0)

    def pick(self, pixels, mode, alpha=0.5, iso=0.5):
        xy = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1, 2)
        self.fill()
        rc = self.raw(self.dev.lib.svr_pick, xy.ctypes.data_as(C.POINTER(C.c_uint32)), len(xy), p=abi.HitParams(mode, alpha, iso))
        return rc, self.read(len(xy))

    def close(self):
        self.dev.free(self.buf)
        self.canvas.close()


def same(got, ref, what):
    g, r = words(got), words(ref)
    if not np.array_equal(g, r):
        d = np.argwhere((g != r).any(axis=-1))
        i = tuple(d[0])
        raise AssertionError(f"{what}: {len(d)} of {got.size} records differ; first at {i[::-1]}: got {got[i]}, reference {ref[i]}")


def cases(levels, alphas=ALPHAS):
    return [(hr.OPACITY, "opacity", a, 0.5) for a in alphas] + [(hr.ISO, "iso", 0.5, i) for i in levels] + [(hr.MAX, "max", 0.5, 0.5)]


def check_all_modes(rig, H, levels, what, alphas=ALPHAS, **kw):
    """Every mode at every level of `rig` against the reference H; returns the reference maps."""
    refs = []
    for mode, mname, alpha, iso in cases(levels, alphas):
        ref, _ = H.hit_map(mode, rig.canvas.stepSize, alpha=alpha, iso=iso)
        got, _ = rig.hits(mode, alpha=alpha, iso=iso, **kw)
        same(got, ref, f"{what}, {mname}, alpha {alpha}, iso {iso}")
        refs.append(ref)
    return refs


# ------------------------------------------------------------------------------------------------ scenes x modes, layouts, skipping
@pytest.mark.parametrize("name", ["tiny_head", "tiny_bone", "tiny_head_noisy", "tiny"])
def test_modes_scenes(hip_dev, name):
    sc = scenes.make_scene(name)
    H = hr.reference(name, lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        refs = check_all_modes(rig, H, LEVELS[name], name)
        for ref in refs:
            assert (ref["status"] == hr.MISS).any() and (ref["status"] == hr.FOUND).any()
        if name != "tiny_head_noisy":                # (noisy air: every ray through the box finds some opacity and a maximum)
            assert all((ref["status"] == hr.NONE).any() for ref in refs)
    finally:
        rig.close()


@pytest.mark.parametrize("layout", [abi.LAYOUT_LINEAR, abi.LAYOUT_BRICK, abi.LAYOUT_PAIR, abi.LAYOUT_CELL])
def test_layouts(hip_dev, layout):
    sc = scenes.make_scene("tiny_head")
    H = hr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc, layout=layout)
    try:
        check_all_modes(rig, H, (0.15,), f"layout {layout}", alphas=(0.5,))
    finally:
        rig.close()


@pytest.mark.parametrize("shift", [0, 2])
def test_skip_on_off_and_counters(hip_dev, shift):
    """SVR_OPT_EMPTY_SKIP 1 and 0 give the same maps and the reference's counts; with skipping on fewer fetches are issued (the air
    of tiny_head is exactly 0 and exactly transparent, so skippable samples exist in every mode)."""
    hip_dev.set_option(abi.OPT_MACRO_SHIFT_MIN, shift)
    sc = scenes.make_scene("tiny_head")
    H = hr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        for mode, mname, alpha, iso in cases((0.15,), alphas=(0.5,)):
            ref, rc = H.hit_map(mode, sc.step_size(), alpha=alpha, iso=iso)
            executed = {}
            for skip in (1, 0):
                got, c = rig.hits(mode, alpha=alpha, iso=iso, skip=skip, count=True)
                same(got, ref, f"{mname}, skip {skip}, counting build")
                got2, _ = rig.hits(mode, alpha=alpha, iso=iso, skip=skip, count=False)
                same(got2, ref, f"{mname}, skip {skip}")
                print(f"shift {shift} {mname} skip {skip}: steps {c['raycast_steps']} taps {c['vol_taps']} executed {c['vol_taps_executed']}")
                assert c["raycast_steps"] == rc["raycast_steps"] and c["vol_taps"] == rc["vol_taps"], (mname, skip, c, rc)
                executed[skip] = c["vol_taps_executed"]
            assert executed[0] == rc["vol_taps"] and executed[1] < executed[0], (mname, executed)
    finally:
        rig.close()


def skip_counts(dev, shift):
    """{mode name: {counter: value}} of tiny_head at 96 x 80, macro shift `shift`, skipping on: OPACITY 0.5, ISO 0.15 and MAX."""
    dev.set_option(abi.OPT_MACRO_SHIFT_MIN, shift)
    rig = Rig(dev, scenes.make_scene("tiny_head"))
    try:
        return {mname: {k: int(c[k]) for k in COUNTERS}
                for mode, mname, alpha, iso in cases((0.15,), alphas=(0.5,)) for c in [rig.hits(mode, alpha=alpha, iso=iso, skip=1, count=True)[1]]}
    finally:
        rig.close()


@pytest.mark.parametrize("shift", [0, 2])
def test_skip_counts_are_the_recorded_ones(hip_dev, shift):
    """As in tests/test_projection_gpu.py: the samples passed by the kept verdicts and the leaps are exactly the recorded ones."""
    got = skip_counts(hip_dev, shift)
    print(f"shift {shift}: {got}")
    assert got == SKIP_COUNTS["hits"][f"shift{shift}"]


# ------------------------------------------------------------------------------------------------ geometry
def test_clip_planes_inside_the_volume(hip_dev):
    sc = scenes.make_scene("tiny_head", clip=((-0.5, 0.6), (-1.0, 1.0), (-0.7, 0.4)))
    H = hr.reference("tiny_head_clip", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        refs = check_all_modes(rig, H, (0.15, 0.5), "clip planes", alphas=(0.0, 0.5))
        caps = [((r["status"] == hr.FOUND) & (r["sample"] == 0)).any() for r in refs]
        assert caps[0] and caps[2] and caps[3], "the clip planes must cut tissue: hits at sample 0 for alpha 0 and both iso levels"
    finally:
        rig.close()


def test_anisotropic_noncubic_crop(hip_dev):
    H = hr.reference("crop", _crop_scene)
    rig = Rig(hip_dev, H.R.scene)
    try:
        refs = check_all_modes(rig, H, (0.15, 0.5), "anisotropic crop", alphas=(0.5,))
        assert any(((r["status"] == hr.FOUND) & (r["sample"] == 0)).any() for r in refs), "the crop cuts through tissue"
    finally:
        rig.close()


def test_camera_inside_the_volume(hip_dev):
    cam = host.camera_setup((3.0, 2.0, 5.0), (0.0, -4.0, -30.0), (0.0, 1.0, 0.0), 60.0, 0.0, 1.0, 1.0, 64, 48)
    sc = scenes.make_scene("tiny_head", camera=cam, width=64, height=48)
    H = hr.reference("inside", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        refs = check_all_modes(rig, H, (0.15, 0.5), "camera inside", alphas=(0.5,))
        assert not any((r["status"] == hr.MISS).any() for r in refs)
        assert any((r["t"][r["status"] == hr.FOUND] < 0).any() for r in refs), "hits behind the eye: a negative t with status FOUND"
    finally:
        rig.close()


def test_elongated_volume_macro_grid_above_64(hip_dev):
    hip_dev.set_option(abi.OPT_MACRO_SHIFT_MIN, 0)
    H = hr.reference("long", _long_scene)
    rig = Rig(hip_dev, H.R.scene)
    try:
        refs = check_all_modes(rig, H, (0.15, 0.5), "40 x 40 x 600", alphas=(0.5,))
        assert all((r["status"] == hr.FOUND).any() and (r["status"] != hr.FOUND).any() for r in refs)
        # OPACITY shares the ray caster's mask: its set-up used to fail on a half-resolution grid above 32 cells per axis (150 here)
        cv = rig.canvas
        cv.SetRenderMode(host.Canvas.RENDER_MODE_RAYCASTING)
        cv.paint(sync=True)
        ref_rc, _ = H.R.o.render_raycasting()
        assert np.array_equal(cv.read_img(), ref_rc) and ref_rc.any(), "render_raycasting of the elongated volume"
    finally:
        rig.close()


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("step", [0.3, None, 10.0])
def test_step_sizes(hip_dev, step, shift):
    """Below a voxel, the default (the voxel's bounding-sphere radius), and above a macro-cell (h = 5 voxels; cells of 1 and 4)."""
    hip_dev.set_option(abi.OPT_MACRO_SHIFT_MIN, shift)
    sc = scenes.make_scene("tiny_head", width=48, height=40)
    H = hr.reference("tiny_head_48x40", lambda: sc)
    rig = Rig(hip_dev, sc, step=step)
    try:
        check_all_modes(rig, H, (0.15, 0.5), f"step {step}, macro shift {shift}", alphas=(0.0, 0.95))
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------ shard, window, picks
def test_row_shard_and_window(hip_dev):
    sc = scenes.make_scene("tiny_head")
    H = hr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc)
    try:
        for mode, mname, alpha, iso in cases((0.15,), alphas=(0.5,)):
            ref, _ = H.hit_map(mode, sc.step_size(), alpha=alpha, iso=iso)
            parts = [rig.hits(mode, alpha=alpha, iso=iso, shard=(8, rank, 2))[0] for rank in (0, 1)]
            rows = np.arange(sc.height)
            for rank, got in enumerate(parts):
                own = (rows // 8) % 2 == rank
                same(got[own], ref[own], f"{mname}, rank {rank}: owned rows")
                assert np.all(words(got[~own]) == FILL_WORD), f"{mname}, rank {rank}: rows of the other rank were written"
            x0, y0, x1, y1 = 21, 13, 70, 59
            got, _ = rig.hits(mode, alpha=alpha, iso=iso, win=(x0, y0, x1, y1))
            same(got[y0:y1, x0:x1], ref[y0:y1, x0:x1], f"{mname}: window")
            outside = np.ones(got.shape, dtype=bool)
            outside[y0:y1, x0:x1] = False
            assert np.all(words(got[outside]) == FILL_WORD), f"{mname}: records outside the window were written"
    finally:
        rig.close()


def test_pick_equals_the_map(hip_dev):
    """n = 1, n = 4096 with duplicates, and pixels outside the window and shard in force: entry i is record (x_i, y_i) of the full map,
    and nothing behind the n records is written."""
    sc = scenes.make_scene("tiny_head")
    H = hr.reference("tiny_head", lambda: sc)
    rig = Rig(hip_dev, sc)
    rng = np.random.default_rng(11)
    try:
        many = np.stack([rng.integers(0, sc.width, abi.PICK_MAX), rng.integers(0, sc.height, abi.PICK_MAX)], axis=1)
        many[:64] = many[64:128]                                     # duplicates
        many[-1] = (sc.width - 1, sc.height - 1)
        assert rig.n > abi.PICK_MAX
        for mode, mname, alpha, iso in cases((0.15,), alphas=(0.5,)):
            ref, _ = H.hit_map(mode, sc.step_size(), alpha=alpha, iso=iso)
            full, _ = rig.hits(mode, alpha=alpha, iso=iso)
            same(full, ref, mname)
            for px in ([(40, 37)], [(0, 0)], many, many[:65]):
                px = np.asarray(px)
                rc, got = rig.pick(px, mode, alpha=alpha, iso=iso)
                assert rc == 0
                same(got, ref[px[:, 1], px[:, 0]], f"{mname}: pick of {len(px)}")
                rest = words(rig.read().reshape(-1)[len(px):])
                assert np.all(rest == FILL_WORD), f"{mname}: a pick of {len(px)} wrote behind its records"
            # a pick is a query: the window and the shard in force do not matter
            hip_dev.check(hip_dev.lib.svr_set_render_window(10, 10, 20, 20))
            rc, got = rig.pick(many[:100], mode, alpha=alpha, iso=iso)
            hip_dev.lib.svr_set_render_window(0, 0, -1, -1)
            assert rc == 0
            same(got, ref[many[:100, 1], many[:100, 0]], f"{mname}: pick under a window")
            hip_dev.check(hip_dev.lib.svr_set_row_shard(8, 1, 2))
            rc, got = rig.pick(many[:100], mode, alpha=alpha, iso=iso)
            hip_dev.lib.svr_set_row_shard(0, 0, 1)
            assert rc == 0
            same(got, ref[many[:100, 1], many[:100, 0]], f"{mname}: pick under a row shard")
        # the Python layer
        got = rig.canvas.pick(many[:10], abi.HIT_ISO, iso=0.15)
        same(got, H.hit_map(hr.ISO, sc.step_size(), iso=0.15)[0][many[:10, 1], many[:10, 0]], "Canvas.pick")
        same(rig.canvas.hit_map(abi.HIT_MAX), H.hit_map(hr.MAX, sc.step_size())[0], "Canvas.hit_map")
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------ refusals, state, the projection
def test_refused_arguments_leave_the_buffer_alone(hip_dev):
    sc = scenes.make_scene("tiny")
    rig = Rig(hip_dev, sc)
    cv, lib = rig.canvas, hip_dev.lib
    try:
        rig.fill()
        nan, inf = float("nan"), float("inf")
        P = abi.HitParams
        good = P(abi.HIT_OPACITY, 0.5, 0.5)
        bad_vol = type(cv.deviceVolume).from_buffer_copy(cv.deviceVolume)
        bad_vol.densityScale = -1.0
        nan_vol = type(cv.deviceVolume).from_buffer_copy(cv.deviceVolume)
        nan_vol.densityScale = nan
        common = {
            "null volume": dict(p=good, null=-5), "null tf": dict(p=good, null=-4), "null camera": dict(p=good, null=-3), "null params": dict(p=None),
            "null hits": dict(p=good, null=0),
            "mode 0": dict(p=P(0, 0.5, 0.5)), "mode 4": dict(p=P(4, 0.5, 0.5)),
            "step 0": dict(p=good, step=0.0), "step < 0": dict(p=good, step=-1.0), "step nan": dict(p=good, step=nan), "step inf": dict(p=good, step=inf),
            "iso nan": dict(p=P(abi.HIT_ISO, 0.5, nan)), "iso inf": dict(p=P(abi.HIT_ISO, 0.5, inf)),
            "alpha < 0": dict(p=P(abi.HIT_OPACITY, -0.01, 0.5)), "alpha > 0.95": dict(p=P(abi.HIT_OPACITY, 0.96, 0.5)),
            "alpha nan": dict(p=P(abi.HIT_OPACITY, nan, 0.5)), "alpha inf": dict(p=P(abi.HIT_MAX, inf, 0.5)),
            "densityScale < 0": dict(p=good, vol=bad_vol), "densityScale nan": dict(p=good, vol=nan_vol),
        }
        xy = np.array([[3, 4], [5, 6], [63, 63]], dtype=np.uint32)
        ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        for what, kw in common.items():
            assert rig.raw(lib.svr_render_hits, **kw) != 0, f"svr_render_hits: {what} was accepted"
            assert rig.raw(lib.svr_pick, ptr(xy), len(xy), **kw) != 0, f"svr_pick: {what} was accepted"
            assert np.all(words(rig.read()) == FILL_WORD), f"{what}: the buffer was written"
        big = np.zeros((abi.PICK_MAX + 1, 2), dtype=np.uint32)
        picks = {
            "null list": (None, 3), "n 0": (ptr(xy), 0), "n > SVR_PICK_MAX": (ptr(big), len(big)),
            "x outside": (ptr(np.array([[3, 4], [64, 6]], dtype=np.uint32)), 2), "y outside": (ptr(np.array([[3, 64]], dtype=np.uint32)), 1),
        }
        for what, (lst, n) in picks.items():
            assert rig.raw(lib.svr_pick, lst, n, p=good) != 0, f"svr_pick: {what} was accepted"
            assert np.all(words(rig.read()) == FILL_WORD), f"svr_pick, {what}: the buffer was written"
        assert rig.raw(lib.svr_pick, ptr(xy), len(xy), p=good) == 0
        got = words(rig.read().reshape(-1))
        assert not np.all(got[:3] == FILL_WORD) and np.all(got[3:] == FILL_WORD)
        assert rig.raw(lib.svr_render_hits, p=P(abi.HIT_OPACITY, 0.95, 0.5)) == 0
        assert not (words(rig.read()) == FILL_WORD).all(axis=-1).any()
    finally:
        rig.close()


def test_hits_leave_no_state_behind_and_match_the_iso_projection(hip_dev):
    """render_raycasting and svr_render_projection images are the same before and after hit calls, and the ISO FOUND pixels are the
    pixels with alpha 255 of the ISO projection."""
    sc = scenes.make_scene("tiny_head")
    rig = Rig(hip_dev, sc)
    cv = rig.canvas

    def snapshot():
        cv.SetRenderMode(host.Canvas.RENDER_MODE_RAYCASTING)
        cv.paint(sync=True)
        out = [cv.read_img()]
        for mode in (abi.PROJ_MIP, abi.PROJ_ISO):
            cv.paint_projection(mode, iso=0.15, sync=True)
            out.append(cv.read_img())
        return out

    try:
        before = snapshot()
        maps = {}
        for mode, mname, alpha, iso in cases((0.15,), alphas=(0.0, 0.95)):
            maps[mname] = rig.hits(mode, alpha=alpha, iso=iso)[0]
            rig.hits(mode, alpha=alpha, iso=iso, skip=0)
            rig.pick([(5, 5), (48, 40)], mode, alpha=alpha, iso=iso)
        after = snapshot()
        for what, b, a in zip(("render_raycasting", "the MIP projection", "the ISO projection"), before, after):
            assert np.array_equal(b, a), f"{what} changed"
            assert b.any()
        assert np.array_equal(maps["iso"]["status"] == hr.FOUND, before[2][..., 3] == 255)
        assert np.array_equal(maps["iso"]["status"] != hr.FOUND, before[2][..., 3] == 0)
    finally:
        rig.close()
