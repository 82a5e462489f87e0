"""The device-built skipping tables (csrc/svr_accel.hip), read back with svr_selftest_accel exactly as the kernels read them, against
their numpy restatement (tests/accel_ref.py, anchored on the oracle by tests/test_accel_cpu.py): EVERY entry of EVERY table, for
equality -- the min/max tables (normal, fine, wide), the packed half-resolution distances, the deep-empty and `empty` bits, the bound
classes with their thresholds, the census, the fine `empty` bits, the sub-cell occupancy bytes and the bound byte table.  An
over-conservative entry (which no image can show) fails here like a non-conservative one.  (The reference's distance field counts the
non-empty cells of clipped cubes with a summed-volume table; the all-pairs brute force anchors it, and the device's separable
construction, on small grids only: tests/test_accel_cpu.py.)

Then the flat and line-like volumes, whose grid is limited by the half-resolution tables: their tables, and their renders against the
oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding
from sunvolumerender_amd import abi, host, scenes
from tests import accel_ref as ar
from tests import hit_ref as hr
from tests.util import assert_bit_exact, hip_frames, oracle_frames

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ reading the tables back
def read_tables(dev):
    """{name: array} of the current scene's tables + "info" (svr_selftest_accel)."""
    lib = dev.lib
    info = (C.c_int32 * 16)()
    dev.check(lib.svr_selftest_accel(0, None, 0, info))
    i = list(info)
    shift, g, hg, fg = i[0], tuple(i[1:4]), tuple(i[4:7]), tuple(i[7:10])
    n, hn, fn = g[0] * g[1] * g[2], hg[0] * hg[1] * hg[2], fg[0] * fg[1] * fg[2]
    out = {"info": dict(shift=shift, grid=g, hgrid=hg, fgrid=fg if fn else None, mask_words=i[10], dist_words=i[11], bnd8_built=bool(i[12] & 1),
                        bnd8_in_use=bool(i[12] & 2), sub8_built=bool(i[13]), accel_words=i[14], bnd8_bytes=i[15])}

    def get(table, shape, dtype):
        a = np.zeros(shape, dtype=dtype)
        dev.check(lib.svr_selftest_accel(table, a.ctypes.data_as(C.c_void_p), a.nbytes, info))
        return a

    out["mm"] = get(1, (g[2], g[1], g[0], 2), np.uint16)
    out["mm_wide"] = get(3, (hg[2], hg[1], hg[0], 2), np.uint16)
    out["accel"] = get(4, (i[14],), np.uint32)
    if fn:
        out["mm_fine"] = get(2, (fg[2], fg[1], fg[0], 2), np.uint16)
        out["fine_empty"] = get(5, (ar.ceil_div(fn, 32),), np.uint32)
    if i[13]:
        out["sub8"] = get(6, (g[2], g[1], g[0]), np.uint8)
    if i[12] & 1:
        out["bnd8"] = get(7, (i[15],), np.uint8)
    return out


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape}, reference {ref.shape}"
    if not np.array_equal(got, ref):
        d = np.argwhere(got != ref)
        i = tuple(d[0])
        raise AssertionError(f"{what}: {len(d)} of {got.size} entries differ; first at {i}: device {got[i]!r}, reference {ref[i]!r}")


def compare(got, T: ar.AccelTables, what):
    """every table of `got` (read_tables) against the reference T"""
    vt, info = T.vt, got["info"]
    assert (info["shift"], info["grid"], info["hgrid"], info["fgrid"]) == (vt.shift, vt.grid, vt.hgrid, vt.fgrid), (what, info)
    assert (info["mask_words"], info["dist_words"], info["accel_words"], info["bnd8_bytes"]) == (T.mask_words, T.dist_words, ar.ACCEL_WORDS, ar.BOUND8_BYTES), (what, info)
    assert info["dist_words"] <= ar.DIST_WORDS_MAX and info["mask_words"] <= ar.MASK_WORDS_MAX
    _same(got["mm"], vt.mm, f"{what}: mm")
    _same(got["mm_wide"], vt.mm_wide, f"{what}: mm_wide")
    for region, (off, ref) in T.accel_regions().items():
        _same(got["accel"][off:off + len(ref)], ref, f"{what}: accel buffer, {region}")
    assert ("mm_fine" in got) == (vt.fgrid is not None) == info["sub8_built"], what
    if vt.fgrid is not None:
        _same(got["mm_fine"], vt.mm_fine, f"{what}: mm_fine")
        _same(got["fine_empty"], ar.pack_bits(T.fine_empty), f"{what}: fine `empty` bits")
        _same(got["sub8"], T.sub8, f"{what}: sub8")
    assert ("bnd8" in got) == (T.bnd8 is not None), f"{what}: bound byte table built: {'bnd8' in got}"
    if T.bnd8 is not None:
        _same(got["bnd8"], T.bnd8, f"{what}: bound8")


class TableRig:
    """A canvas holding one of accel_ref's volumes, its texture created under the volume's SVR_OPT_MACRO_SHIFT_MIN."""

    def __init__(self, dev, name):
        self.dev, self.name = dev, name
        self.vox, self.vt = ar.named_volume(name)
        self.canvas = host.Canvas(dev, 16, 12)
        tf, mo, _ = ar.transfer_functions()["default"]
        self.canvas.SetTransferFunctionTable(tf, mo)
        dev.set_option(abi.OPT_MACRO_SHIFT_MIN, ar.VOLUMES[name][1])
        try:
            self.canvas.LoadVolume(self.vox, (1.0, 1.0, 1.0), 1.0)
        finally:
            dev.set_option(abi.OPT_MACRO_SHIFT_MIN, 0)

    def set_tf(self, tf, max_opacity, density_scale):
        self.canvas.SetTransferFunctionTable(tf, max_opacity)
        self.canvas.SetDensityScale(density_scale)

    def check(self, tf, max_opacity, density_scale, what):
        T = ar.accel_tables(self.vt, tf, density_scale, max_opacity)
        compare(read_tables(self.dev), T, f"{self.name}, {what}")
        return T

    def close(self):
        self.canvas.close()


# ------------------------------------------------------------------------------------------------ small volumes x transfer functions
@pytest.mark.parametrize("name", ar.SMALL_VOLUMES)
def test_tables_equal_reference(hip_dev, name):
    """37 x 21 x 10 at SVR_OPT_MACRO_SHIFT_MIN 0..3 (odd grids, children beyond the end, cells of 1 to 8 voxels), 40 x 8 x 8 (one
    voxel: the distance cap and the grid's ends), 64^3 at shift 1 (the largest half-resolution grid with a byte table), each under the
    default, all-transparent, all-opaque and hazy tables, densityScale 1 and 37.5, a table with an entry that is not a number, and a
    negative densityScale (the API accepts both: class 15 / byte 255 where no bound exists)."""
    rig = TableRig(hip_dev, name)
    try:
        for tf_name, (tf, mo, ds) in ar.transfer_functions().items():
            rig.set_tf(tf, mo, ds)
            T = rig.check(tf, mo, ds, tf_name)
            if tf_name == "default":
                assert T.empty.any() and not T.empty.all() and T.bnd8 is not None
    finally:
        rig.close()


def test_tables_follow_a_transfer_function_edit(hip_dev):
    """svr_update_tf_texture on the live table: the tables read back next are those of the NEW table (and of the old one again after
    it is restored) -- in place, without a new texture or another setup call."""
    rig = TableRig(hip_dev, "37x21x10_s1")
    tfs = ar.transfer_functions()
    try:
        tf0, mo, ds = tfs["default"]
        first = rig.check(tf0, mo, ds, "before the edit")
        for edit in ("hazy", "transparent", "default"):
            tf = np.ascontiguousarray(tfs[edit][0], dtype=np.float32)
            hip_dev.check(hip_dev.lib.svr_update_tf_texture(C.c_uint64(rig.canvas.transferFunction.tex), tf.ctypes.data_as(C.c_void_p), tf.shape[0], 0))
            T = rig.check(tf, mo, ds, f"after the edit to {edit}")
            assert (edit == "default") == np.array_equal(T.hcls, first.hcls)
    finally:
        rig.close()


def test_read_back_hook_arguments(hip_dev):
    """svr_selftest_accel: a wrong size, a table the scene does not have, a bad table number and a scene without acceleration data are
    errors, and nothing is written."""
    rig = TableRig(hip_dev, "40x8x8_s0")                                   # shift 0: no fine level
    lib = hip_dev.lib
    info = (C.c_int32 * 16)()
    buf = np.full(40 * 8 * 8 * 2, 0xABCD, dtype=np.uint16)
    try:
        assert lib.svr_selftest_accel(1, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 2, info) == -4
        assert lib.svr_selftest_accel(2, buf.ctypes.data_as(C.c_void_p), buf.nbytes, info) == -3
        assert lib.svr_selftest_accel(8, buf.ctypes.data_as(C.c_void_p), buf.nbytes, info) == -4
        assert lib.svr_selftest_accel(1, None, buf.nbytes, info) == -4
        lib.svr_clear_error()
        hip_dev.set_option(abi.OPT_EMPTY_SKIP, 0)
        assert lib.svr_selftest_accel(0, None, 0, info) == -3
        lib.svr_clear_error()
        hip_dev.set_option(abi.OPT_EMPTY_SKIP, 1)
        assert np.all(buf == 0xABCD)
        lib.svr_clear_error()
        assert lib.svr_selftest_accel(1, buf.ctypes.data_as(C.c_void_p), buf.nbytes, info) == 0 and list(info)[:4] == [0, 40, 8, 8]
    finally:
        lib.svr_clear_error()
        hip_dev.set_option(abi.OPT_EMPTY_SKIP, 1)
        rig.close()


# ------------------------------------------------------------------------------------------------ flat and line-like volumes
# (spacing, eye direction): the thin axes are stretched so that the volume fills a 64 x 48 image from an oblique eye
FLAT_VIEWS = {
    "flat_512x512x1": ((1.0, 1.0, 96.0), (0.55, 0.45, 0.70)),
    "flat_1x400x330": ((96.0, 1.0, 1.0), (0.70, 0.40, 0.59)),
    "line_65538x1x1": ((1.0 / 256.0, 64.0, 64.0), (0.45, 0.50, 0.74)),
}
_FLAT_SCENES: dict = {}


def flat_scene(name):
    if name not in _FLAT_SCENES:
        vox, _ = ar.named_volume(name)
        spacing, eye_dir = FLAT_VIEWS[name]
        tf, mo, ds = ar.transfer_functions()["default"]
        dim = (vox.shape[2], vox.shape[1], vox.shape[0])
        size = host.volume_size(dim, spacing)
        dist = 1.15 * host.zoom_to_extent_eye_dist(size, 45.0)
        d = np.asarray(eye_dir, dtype=np.float64)
        eye = tuple(float(v) for v in d / np.linalg.norm(d) * dist)
        cam = host.camera_setup(eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.0, 1.0, 1.0, 64, 48)
        R = host.bounding_sphere_radius(dim, spacing)
        lights = [host.place_area_light(55.0, 35.0, 1.5 * R + 1.0, 0.5 * R, (1.0, 1.0, 1.0), 600.0)]
        _FLAT_SCENES[name] = scenes.Scene(name=name, vox=vox, spacing=spacing, max_magnitude=scenes.max_gradient_magnitude(vox, spacing), tf_rgba=tf,
                                          max_opacity=mo, width=64, height=48, lights=lights, env_map=scenes.synthetic_env_map(64, 32),
                                          env_on_escape=True, trace_depth=2, density_scale=ds, camera=cam)
    return _FLAT_SCENES[name]


@pytest.mark.parametrize("name", ar.FLAT_VOLUMES)
def test_flat_volume_tables(hip_dev, name):
    """512 x 512 x 1, 1 x 400 x 330 and 65538 x 1 x 1: the grid rule gives them one more shift than 64^3 cells alone would, every table
    fits its capacity and equals the reference, and the half-resolution grid is too long for the byte table, which is not built (the
    lane machine then takes the bound class of the exact cell, as ensure_mask documents)."""
    rig = TableRig(hip_dev, name)
    tfs = ar.transfer_functions()
    try:
        for tf_name in ("default", "hazy"):
            tf, mo, ds = tfs[tf_name]
            rig.set_tf(tf, mo, ds)
            T = rig.check(tf, mo, ds, tf_name)
            info = read_tables(hip_dev)["info"]
            assert T.bnd8 is None and not info["bnd8_built"] and not info["bnd8_in_use"]
            assert max(info["hgrid"]) > ar.BOUND8_DIM - 2 and info["shift"] == 1
    finally:
        rig.close()


@pytest.mark.parametrize("name", ar.FLAT_VOLUMES)
def test_flat_volume_renders(hip_dev, name):
    """The same volumes rendered at 64 x 48 against the oracle: the path tracer as 3 per-frame calls and as one 16-frame launch,
    with skipping on and off (bit for bit, and the counters test_degenerate_scenes compares), render_raycasting, svr_render_hits
    in OPACITY mode against tests/hit_ref.py, and under SVR_OPT_LOCAL_MAJORANT the pool form against the straight-line form."""
    sc = flat_scene(name)
    dev = hip_dev
    for frames, batch in ((3, False), (16, True)):
        ref_hdr, ref_img, ref_c = oracle_frames(sc, frames)
        assert ref_c["scatter_events"] > 0 and ref_hdr.max() > 0
        res = {}
        for skip in (True, False):
            hdr, img, c = hip_frames(dev, sc, frames, batch=batch, empty_skip=skip)
            assert_bit_exact(hdr, ref_hdr, f"{name}, {frames} frames, batch={batch}, skipping {'on' if skip else 'off'}")
            assert np.array_equal(img, ref_img)
            assert c["vol_taps"] == ref_c["vol_taps"] and c["woodcock_iters"] == ref_c["woodcock_iters"]
            res[skip] = (hdr, img, c)
        assert_bit_exact(res[True][0], res[False][0], f"{name}: skipping on vs off")
        assert np.array_equal(res[True][1], res[False][1])
        assert all(res[True][2][k] == res[False][2][k] for k in ("paths", "vol_taps", "woodcock_iters", "scatter_events", "shadow_walks"))
    canvas = host.Canvas(dev, sc.width, sc.height)
    buf = dev.malloc(sc.width * sc.height * 40)
    try:
        scenes.apply_to_canvas(sc, canvas)
        # the ray caster
        ref_rc, _ = binding.OracleScene(sc).render_raycasting()
        canvas.SetRenderMode(host.Canvas.RENDER_MODE_RAYCASTING)
        canvas.paint(sync=True)
        assert np.array_equal(canvas.read_img(), ref_rc) and ref_rc[..., :3].any()
        canvas.SetRenderMode(host.Canvas.RENDER_MODE_PATHTRACER)
        # the hit map
        H = hr.reference("accel_" + name, lambda: sc)
        ref_hits, _ = H.hit_map(hr.OPACITY, canvas.stepSize, alpha=0.5)
        dev.check(dev.lib.svr_memset_device(C.c_void_p(buf), 0xAB, sc.width * sc.height * 40))
        dev.check(dev.lib.svr_render_hits(C.c_void_p(buf), C.byref(canvas.deviceVolume), C.byref(canvas.transferFunction), C.byref(canvas.camera),
                                          C.c_float(canvas.stepSize), C.byref(abi.HitParams(abi.HIT_OPACITY, 0.5, 0.5))))
        dev.synchronize()
        hits = dev.to_host(buf, (sc.height, sc.width), hr.HIT_DTYPE)
        _same(hits.view(np.uint32).reshape(sc.height, sc.width, 10), ref_hits.view(np.uint32).reshape(sc.height, sc.width, 10), f"{name}: hit records")
        assert (ref_hits["status"] == hr.FOUND).any() and (ref_hits["status"] == hr.MISS).any()
        # local majorants: pool form (1) against the straight-line form (2)
        imgs = []
        for mode in (1, 2):
            dev.set_option(abi.OPT_LOCAL_MAJORANT, mode)
            canvas.ReStartRender()
            canvas.paint_frames(16, sync=True)
            imgs.append((canvas.read_hdr(), canvas.read_img()))
        assert_bit_exact(imgs[0][0], imgs[1][0], f"{name}: pool vs straight-line local-majorant paths")
        assert np.array_equal(imgs[0][1], imgs[1][1]) and imgs[0][0].max() > 0
        # ... and the mode was in effect (the library renders with the default kernel where it cannot be): another estimator of the same
        # image, so other bits than the default mode's 16-frame launch above
        assert not np.array_equal(imgs[0][0].view(np.uint32), res[True][0].view(np.uint32)), f"{name}: SVR_OPT_LOCAL_MAJORANT changed nothing"
    finally:
        dev.set_option(abi.OPT_LOCAL_MAJORANT, 0)
        dev.free(buf)
        canvas.close()
