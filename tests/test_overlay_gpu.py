"""svr_slice_ids, svr_hit_ids, svr_overlay_ids and svr_overlay_slice on the GPU, through the raw ABI: every id image and every tinted image
is IDENTICAL (tolerance 0, every pixel) to the numpy reference (tests/overlay_ref.py).  Every output buffer starts as a pattern, so a pixel
the call must not touch shows.  The fixtures are those whose conditions tests/test_overlay_cpu.py asserts on the reference alone."""
import ctypes as C

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import overlay_ref as ov

pytestmark = pytest.mark.gpu

FILL = 0xCD
FILL_WORD = 0xCDCDCDCD
SHARD = (8, 8)                                   # strip rows, world: an 8-way row shard
STYLES = (("custom palette", dict(fill_alpha=96, edge_alpha=255, palette=ov.CUSTOM_PALETTE)),
          ("default palette", dict()),
          ("outlines only", dict(fill_alpha=0)),
          ("edge = fill", dict(fill_alpha=140, edge_alpha=140)),
          ("both 0", dict(fill_alpha=0, edge_alpha=0)))


class Rig:
    """A canvas of w x h with the scene of a source applied, the source on the device, and buffers for `slices` images."""

    def __init__(self, dev, source_name, w, h, slices=ov.STACK[0]):
        self.dev, self.lib, self.name, self.W, self.H, self.slices = dev, dev.lib, source_name, w, h, slices
        sname = ov.scene_of(source_name)
        self.sc, self.R, self.src = ov.scene(sname), ov.reference(sname), ov.source(source_name)
        self.canvas = host.Canvas(dev, w, h)
        scenes.apply_to_canvas(scenes.make_scene("tiny_head", vox=self.sc.vox, width=w, height=h), self.canvas)
        self.vol = self.canvas.deviceVolume
        self.shape = self.src.shape
        self.bufs = []
        self.d_src = self.upload_source()
        self.d_ids = self.alloc(4 * w * h * slices)
        self.d_img = self.alloc(4 * w * h * slices)
        self.d_img2 = self.alloc(4 * w * h * slices)

    def alloc(self, nbytes):
        self.bufs.append(self.dev.malloc(nbytes))
        return self.bufs[-1]

    def upload_source(self):
        if self.src.dtype == bool:
            nz, ny, nx = self.shape
            words = host.region_mask_pack(self.src).reshape(nz, ny, -1)
            if nx % 32:
                words[:, :, -1] |= np.uint32((0xFFFFFFFF << (nx % 32)) & 0xFFFFFFFF)      # the padding bits are set: they must be ignored
            arr = np.ascontiguousarray(words.reshape(-1))
        else:
            arr = np.ascontiguousarray(self.src, dtype=np.uint32)
        buf = self.alloc(arr.nbytes)
        self.dev.to_device(buf, arr)
        return buf

    def source(self):
        return abi.OverlaySource(self.d_src, None) if self.src.dtype == bool else abi.OverlaySource(None, self.d_src)

    def fill(self, buf, slices):
        self.dev.check(self.lib.svr_memset_device(C.c_void_p(buf), FILL, 4 * self.W * self.H * slices))

    def framed(self, call, shard=None, win=None):
        """the return code of call() under a shard / window, which are reset afterwards"""
        if shard is not None:
            self.dev.check(self.lib.svr_set_row_shard(*shard))
        if win is not None:
            self.dev.check(self.lib.svr_set_render_window(*win))
        try:
            rc = call()
            self.dev.synchronize()
            return rc
        finally:
            self.lib.svr_set_row_shard(0, 0, 1)
            self.lib.svr_set_render_window(0, 0, -1, -1)

    def slice_ids(self, p, count=1, spacing=0.0, **frame):
        self.fill(self.d_ids, count)
        src = self.source()
        rc = self.framed(lambda: self.lib.svr_slice_ids(C.c_void_p(self.d_ids), C.byref(self.vol), *self.shape[::-1], self.W, self.H, C.byref(p),
                                                        count, C.c_float(spacing), C.byref(src)), **frame)
        self.dev.check(rc)
        return self.dev.to_host(self.d_ids, (count, self.H, self.W), np.uint32)

    def render(self, buf, p, count=1, spacing=0.0):
        """the slices of p, grey, into buf: the images the overlays are laid over"""
        q = abi.SliceParams.from_buffer_copy(p)
        q.window_lo, q.window_hi, q.mode = 0.05, 0.6, abi.SLAB_MEAN
        self.dev.check(self.lib.svr_render_slice_stack(C.c_void_p(buf), C.byref(self.vol), C.byref(self.canvas.transferFunction), self.W, self.H,
                                                       C.byref(q), count, C.c_float(spacing)))
        self.dev.synchronize()
        return self.dev.to_host(buf, (count, self.H, self.W, 4), np.uint8)

    def overlay_ids(self, buf, ids, style, count=1, **frame):
        """svr_overlay_ids of the id images `ids` (host) over the images in buf"""
        self.dev.to_device(self.d_ids, np.ascontiguousarray(ids, dtype=np.uint32))
        rc = self.framed(lambda: self.lib.svr_overlay_ids(C.c_void_p(buf), C.c_void_p(self.d_ids), self.W, self.H, count, C.byref(style)), **frame)
        self.dev.check(rc)
        return self.dev.to_host(buf, (count, self.H, self.W, 4), np.uint8)

    def overlay_slice(self, buf, p, style, count=1, spacing=0.0, **frame):
        src = self.source()
        rc = self.framed(lambda: self.lib.svr_overlay_slice(C.c_void_p(buf), C.byref(self.vol), *self.shape[::-1], self.W, self.H, C.byref(p), count,
                                                            C.c_float(spacing), C.byref(src), C.byref(style)), **frame)
        self.dev.check(rc)
        return self.dev.to_host(buf, (count, self.H, self.W, 4), np.uint8)

    def ref_ids(self, p, count=1, spacing=0.0):
        return np.stack([ov.slice_ids(self.R, p, self.W, self.H, self.src, k, spacing)[0] for k in range(count)])

    def close(self):
        for b in self.bufs:
            self.dev.free(b)
        self.canvas.close()


def same(got, ref, what):
    if not np.array_equal(got, ref):
        diff = got != ref
        if diff.ndim == 4:
            diff = diff.any(axis=-1)
        d = np.argwhere(diff)
        k, y, x = d[0]
        raise AssertionError(f"{what}: {len(d)} of {diff.size} pixels differ; first at slice {k} x={x} y={y}: got {got[k, y, x].tolist()}, "
                             f"reference {ref[k, y, x].tolist()}")


def style_of(dev, **kw):
    """(svr_overlay_style, its palette as uint32 for the reference)"""
    st = dev.overlay_style(**kw)
    pal = kw["palette"] if "palette" in kw else dev.overlay_palette_default()
    return st, pal


def ref_blend(img, ids, st, pal):
    return ov.blend(img, ids, pal, st.fill_alpha, st.edge_alpha)


@pytest.fixture(scope="module", params=[(s, wh) for s in ov.SOURCES for wh in ov.IMAGES], ids=lambda sp: f"{sp[0]}-{sp[1][0]}x{sp[1][1]}")
def rig(hip_dev, request):
    name, (w, h) = request.param
    r = Rig(hip_dev, name, w, h)
    yield r
    r.close()


# ------------------------------------------------------------------------------------------------ the sources come from the device calls
def test_sources_are_what_the_region_calls_give(hip_dev):
    labels, K = hip_dev.region_label(ov.noisy_mask(), 6)
    assert np.array_equal(labels, ov.source("labels6")) and K > 100 and (np.bincount(labels.ravel())[1:] == 1).any()
    zones, count, _, _ = hip_dev.region_split(ov.necked_mask(), ov.SPLIT_R2, 26)
    assert np.array_equal(zones, ov.source("zones")) and count == 8
    patched = ov.source("patched")
    assert patched.max() == 0xFFFFFFFF and ((patched > abi.OVERLAY_MAX_PALETTE) & (patched < 0xFFFFFFFF)).any()


# ------------------------------------------------------------------------------------------------ svr_slice_ids
def test_slice_ids_planes_and_slabs(rig):
    for what, p in ov.cases(rig.name, rig.W, rig.H):
        same(rig.slice_ids(p), rig.ref_ids(p), what)


def test_slice_ids_stack_window_shard(rig):
    count, spacing = ov.STACK
    win = ov.window_of(rig.W, rig.H)
    pattern = np.full((count, rig.H, rig.W), FILL_WORD, dtype=np.uint32)
    for what, p in ov.cases(rig.name, rig.W, rig.H)[5::2]:                       # axis 2 as a slab, the oblique planes as plane and slab
        ref = rig.ref_ids(p, count, spacing)
        assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2]), what
        same(rig.slice_ids(p, count, spacing), ref, f"{what}, stack")
        same(rig.slice_ids(p, count, spacing, win=win), ov.cut_out(ref, pattern, win, channels=False), f"{what}, stack, window {win}")
        for rank in range(SHARD[1]):
            rows = ov.shard_rows(rig.H, SHARD[0], rank, SHARD[1])
            want = np.where(rows[None, :, None], ref[:1], pattern[:1])
            same(rig.slice_ids(p, shard=(SHARD[0], rank, SHARD[1])), want, f"{what}, shard {rank} of {SHARD[1]}")


def test_slice_ids_device_side_refusal_leaves_the_buffer(rig):
    p = ov.slab(ov.planes(ov.scene_of(rig.name), rig.W, rig.H)[0][1])
    p.step = p.thickness / 5000.0                                                  # more than SVR_SLICE_MAX_SAMPLES
    rig.fill(rig.d_ids, 1)
    src = rig.source()
    rc = rig.lib.svr_slice_ids(C.c_void_p(rig.d_ids), C.byref(rig.vol), *rig.shape[::-1], rig.W, rig.H, C.byref(p), 1, C.c_float(0.0), C.byref(src))
    msg = rig.lib.svr_last_error().decode()
    rig.lib.svr_clear_error()
    assert rc == -3 and "svr_slice_ids" in msg and "samples" in msg, (rc, msg)
    rig.dev.synchronize()
    assert np.all(rig.dev.to_host(rig.d_ids, (rig.H, rig.W), np.uint32) == FILL_WORD)


# ------------------------------------------------------------------------------------------------ svr_overlay_ids
def test_overlay_ids_styles(rig):
    dev = rig.dev
    for what, p in ov.cases(rig.name, rig.W, rig.H)[4:8]:                        # axis 2 and tilt 30, plane and slab
        ids = rig.ref_ids(p)
        base = rig.render(rig.d_img2, p)
        for sname, kw in STYLES:
            st, pal = style_of(dev, **kw)
            dev.to_device(rig.d_img, base)
            got = rig.overlay_ids(rig.d_img, ids, st)
            ref = ref_blend(base, ids, st, pal)
            same(got, ref, f"{what}, {sname}")
            assert np.array_equal(got[ids == 0], base[ids == 0]) and np.array_equal(got[..., 3], base[..., 3])
            if sname == "both 0":
                assert np.array_equal(got, base)
            else:
                assert not np.array_equal(got, base), f"{what}, {sname}: the overlay shows nothing"


# ------------------------------------------------------------------------------------------------ svr_overlay_slice
def test_overlay_slice_equals_reference_and_two_calls(rig):
    dev = rig.dev
    count, spacing = ov.STACK
    win = ov.window_of(rig.W, rig.H)
    for i, (what, p) in enumerate(ov.cases(rig.name, rig.W, rig.H)):
        sname, kw = STYLES[i % 4]
        st, pal = style_of(dev, **kw)
        n = count if i in (5, 8) else 1                                           # axis 2 as a slab and the general plane also as stacks
        sp = spacing if n > 1 else 0.0
        ids = rig.ref_ids(p, n, sp)
        base = rig.render(rig.d_img2, p, n, sp)
        dev.to_device(rig.d_img, base)
        full = rig.overlay_slice(rig.d_img, p, st, n, sp)
        same(full, ref_blend(base, ids, st, pal), f"{what} x {n}, {sname}: fused against the reference")
        dev.to_device(rig.d_img, base)
        same(full, rig.overlay_ids(rig.d_img, rig.slice_ids(p, n, sp), st, n), f"{what} x {n}, {sname}: fused against the two calls")
        if i % 2 == 0 and n == 1:
            continue
        # windowed and sharded: the cut-out of the full overlay, edges judged from the true ids beyond the border
        dev.to_device(rig.d_img, base)
        same(rig.overlay_slice(rig.d_img, p, st, n, sp, win=win), ov.cut_out(full, base, win), f"{what} x {n}, {sname}: window {win}")
        for rank in (0, 3, SHARD[1] - 1):
            rows = ov.shard_rows(rig.H, SHARD[0], rank, SHARD[1])
            dev.to_device(rig.d_img, base)
            got = rig.overlay_slice(rig.d_img, p, st, n, sp, shard=(SHARD[0], rank, SHARD[1]))
            same(got, np.where(rows[None, :, None, None], full, base), f"{what} x {n}, {sname}: shard {rank} of {SHARD[1]}")


def test_long_stack_takes_several_tasks_per_ticket(hip_dev):
    """From 4 tickets per wave of the full grid on, a ticket grants more than one (slice, tile) task: 63 tiles x 1117 slices are 70371 tasks,
    8797 per ticket shard (odd: the last grant of a shard is cut short), against 8 x 4 waves per compute unit."""
    import re
    w, h, count, spacing = 72, 56, 1117, 0.012
    cus = int(re.search(r"CUs=(\d+)", hip_dev.info()).group(1))
    tasks = ((w + 7) // 8) * ((h + 7) // 8) * count
    assert tasks // (4 * 32 * cus) >= 2 and ((tasks + 7) // 8) % 2 == 1, "the stack must be long enough for this device"
    rig = Rig(hip_dev, "labels6", w, h, slices=count)
    try:
        p = ov.planes("head", w, h)[3][1]                                              # tilt 30
        ids = rig.ref_ids(p, count, spacing)
        assert len(np.unique(ids)) > 50 and (ids[0] != 0).any() and (ids[-1] != 0).any() and not np.array_equal(ids[0], ids[-1])
        same(rig.slice_ids(p, count, spacing), ids, "long stack: svr_slice_ids")
        st, pal = style_of(hip_dev)
        base = np.random.default_rng(3).integers(0, 256, (count, h, w, 4), dtype=np.uint8)
        hip_dev.to_device(rig.d_img, base)
        same(rig.overlay_slice(rig.d_img, p, st, count, spacing), ref_blend(base, ids, st, pal), "long stack: svr_overlay_slice")
    finally:
        rig.close()


def test_canvas_paint_slice_overlay_and_paint_overlay(hip_dev):
    """the Python Canvas layer: host arrays are uploaded (a bool mask as the bit mask), device pointers are taken as they are"""
    w, h = ov.IMAGES[0]
    count, spacing = ov.STACK
    rig = Rig(hip_dev, "octants", w, h)
    cv = rig.canvas
    try:
        st, pal = style_of(hip_dev, palette=ov.CUSTOM_PALETTE)
        p = ov.slab(ov.planes("head", w, h)[4][1])
        for kw, src in ((dict(labels=rig.src), rig.src), (dict(labels=rig.d_src), rig.src), (dict(mask=ov.source("head mask")), ov.source("head mask"))):
            cv.paint_slice(p, sync=True)
            base = cv.read_img()
            cv.paint_slice_overlay(p, style=st, sync=True, **kw)
            ids = ov.slice_ids(rig.R, p, w, h, src)[0]
            same(cv.read_img()[None], ref_blend(base, ids, st, pal)[None], f"paint_slice_overlay({list(kw)[0]})")
        base = rig.render(rig.d_img, p, count, spacing)
        cv.paint_slice_overlay(p, labels=rig.d_src, style=st, count=count, spacing=spacing, imgs=rig.d_img, sync=True)
        same(hip_dev.to_host(rig.d_img, (count, h, w, 4), np.uint8), ref_blend(base, rig.ref_ids(p, count, spacing), st, pal), "paint_slice_overlay, stack")
        with pytest.raises(host.SvrError):
            cv.paint_slice_overlay(p)
        cv.SetRenderMode(cv.RENDER_MODE_RAYCASTING)
        cv.paint(sync=True)
        base = cv.read_img()
        hits = cv.hit_map(abi.HIT_OPACITY, alpha=0.5)
        cv.paint_overlay(labels=rig.src, style=st, mode=abi.HIT_OPACITY, alpha=0.5)
        ids = ov.hit_ids(rig.R.vol, rig.src, hits)
        assert len(np.unique(ids)) >= 4
        same(cv.read_img()[None], ref_blend(base, ids, st, pal)[None], "paint_overlay")
    finally:
        rig.close()


def test_overlay_last_ms(rig):
    what, p = ov.cases(rig.name, rig.W, rig.H)[1]
    rig.slice_ids(p)
    assert 0.0 < rig.dev.overlay_last_ms() < 1000.0


# ------------------------------------------------------------------------------------------------ 3D: hit map -> ids -> overlay
@pytest.mark.parametrize("source_name", ov.HIT_SOURCES)
def test_hit_ids_and_overlay_on_the_ray_caster(hip_dev, source_name):
    w, h = ov.IMAGES[0]
    rig = Rig(hip_dev, source_name, w, h, slices=1)
    dev, cv = rig.dev, rig.canvas
    d_hits = rig.alloc(w * h * host.HIT_DTYPE.itemsize)
    try:
        cv.SetRenderMode(cv.RENDER_MODE_RAYCASTING)
        cv.paint(sync=True)
        base = cv.read_img()[None]
        st, pal = style_of(dev, palette=ov.CUSTOM_PALETTE)
        for mode, alpha, iso, mname in ov.HIT_MODES:
            hp = abi.HitParams(mode, alpha, iso)
            dev.check(dev.lib.svr_render_hits(C.c_void_p(d_hits), C.byref(rig.vol), C.byref(cv.transferFunction), C.byref(cv.camera),
                                              C.c_float(cv.stepSize), C.byref(hp)))
            rig.fill(rig.d_ids, 1)
            src = rig.source()
            # a shard in force must not matter: svr_hit_ids and svr_overlay_ids are whole-image post-processes
            rc = rig.framed(lambda: dev.lib.svr_hit_ids(C.c_void_p(rig.d_ids), C.c_void_p(d_hits), w, h, C.byref(rig.vol), *rig.shape[::-1], C.byref(src)),
                            shard=(8, 1, 2))
            dev.check(rc)
            hits = dev.to_host(d_hits, (h, w), host.HIT_DTYPE)
            ids = ov.hit_ids(rig.R.vol, rig.src, hits)[None]
            found = hits["status"] == abi.HIT_STATUS_FOUND
            assert found.any() and (~found).any() and (ids[0][found] != 0).any(), mname
            same(dev.to_host(rig.d_ids, (1, h, w), np.uint32), ids, f"{source_name}, {mname}: svr_hit_ids")
            dev.to_device(rig.d_img, base)
            got = rig.overlay_ids(rig.d_img, ids, st, win=(3, 3, 9, 9))          # (nor a window)
            same(got, ref_blend(base, ids, st, pal), f"{source_name}, {mname}: svr_overlay_ids over render_raycasting")
            assert np.array_equal(got[0][~found], base[0][~found]), f"{mname}: MISS and NONE pixels must stay"
    finally:
        rig.close()
