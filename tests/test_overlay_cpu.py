"""The overlay calls without a GPU: the reference (tests/overlay_ref.py) against hand-made values, the ABI, the defaults, the refusals (all
decided before the device is touched), and the conditions on the fixtures of tests/test_overlay_gpu.py, asserted on the reference alone so
that no GPU test can pass vacuously."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import hit_ref as hr
from tests import overlay_ref as ov

HEADER = (Path(__file__).resolve().parents[1] / "include" / "svr_abi.h").read_text()
DEFAULT_RGB = [(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
               (70, 240, 240), (240, 50, 230), (210, 245, 60), (250, 190, 212), (0, 0, 128), (170, 110, 40)]


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    lib.svr_clear_error()
    return lib


# ------------------------------------------------------------------------------------------------ the reference by hand
def test_blend_by_hand():
    # one pixel, id 1, no neighbours: an edge-free fill.  a = (A * e.a + 127) / 255; c = (in * (255 - a) + e.c * a + 127) / 255
    def one(inp, colour, A, ea=255):
        img = np.array([[[inp, inp, inp, 77]]], dtype=np.uint8)
        pal = np.array([colour | (colour << 8) | (colour << 16) | (ea << 24)], dtype=np.uint32)
        out = ov.blend(img, np.array([[1]], dtype=np.uint32), pal, A, A)
        assert out[0, 0, 3] == 77 and out[0, 0, 0] == out[0, 0, 1] == out[0, 0, 2]
        return int(out[0, 0, 0])

    for inp in (0, 255, 100):
        assert one(inp, 255, 0) == inp and one(inp, 0, 0) == inp                      # a = 0: not written
        assert one(inp, 255, 255) == 255 and one(inp, 0, 255) == 0                    # a = 255: the colour
    assert one(0, 255, 1) == 1 and one(255, 0, 1) == 254 and one(255, 255, 1) == 255 and one(0, 0, 1) == 0
    assert one(0, 255, 128) == 128 and one(255, 0, 128) == 127 and one(100, 200, 128) == (100 * 127 + 200 * 128 + 127) // 255 == 150
    assert one(0, 255, 255, ea=128) == 128 and one(0, 255, 128, ea=128) == (128 * 128 + 127) // 255 == 64
    assert one(9, 255, 1, ea=127) == 9                                                # a = (127 + 127) / 255 = 0
    assert one(9, 255, 1, ea=128) == (9 * 254 + 255 + 127) // 255 == 10               # a = 1
    # ids pick entry (k - 1) mod count; an entry of alpha 0 hides its labels; id 0 is never written
    img = np.full((1, 6, 4), 50, dtype=np.uint8)
    ids = np.array([[0, 1, 2, 3, 6, 0xFFFFFFFF]], dtype=np.uint32)
    pal = np.array([0xFF0000FF, 0x0000FF00, 0xFFFF0000, 0xFF646464, 0xFF000000], dtype=np.uint32)
    out = ov.blend(img, ids, pal, 255, 255)
    assert out[0, :, :3].tolist() == [[50, 50, 50], [255, 0, 0], [50, 50, 50], [0, 0, 255], [255, 0, 0], [0, 0, 0]]    # 0xFFFFFFFF - 1 = 4 mod 5
    assert (out[..., 3] == 50).all()


def test_edges_by_hand():
    ids = np.array([[1, 1, 1, 0, 0],
                    [1, 1, 1, 0, 2],
                    [1, 1, 1, 0, 2],
                    [3, 3, 1, 0, 0],
                    [3, 3, 1, 1, 1]], dtype=np.uint32)
    want = np.array([[0, 0, 1, 0, 0],
                     [0, 0, 1, 0, 1],
                     [1, 1, 1, 0, 1],
                     [1, 1, 1, 0, 0],
                     [0, 1, 1, 1, 1]], dtype=bool)
    assert np.array_equal(ov.edges(ids), want)
    assert not ov.edges(np.full((3, 4), 7, dtype=np.uint32)).any()                    # the image border is no edge
    stack = np.stack([np.full((2, 2), 1, dtype=np.uint32), np.full((2, 2), 2, dtype=np.uint32)])
    assert not ov.edges(stack).any()                                                  # nor is the next slice


def test_point_mapping_is_that_of_seed_from_world(lib):
    R = ov.reference("crop")
    vol, (nz, ny, nx) = R.vol, ov.scene("crop").vox.shape
    rng = np.random.default_rng(11)
    lo = np.array([vol.bbox.vmin.x, vol.bbox.vmin.y, vol.bbox.vmin.z], dtype=np.float32)
    hi = np.array([vol.bbox.vmax.x, vol.bbox.vmax.y, vol.bbox.vmax.z], dtype=np.float32)
    P = (lo + (hi - lo) * rng.uniform(-0.05, 1.05, (4000, 3))).astype(np.float32)
    P[:300] = np.where(rng.random((300, 3)) < 0.5, hi, P[:300])                       # the far faces, edges and corner
    P[300:400] = np.where(rng.random((100, 3)) < 0.5, lo, P[300:400])
    lattice = (lo + (hi - lo) * (rng.integers(0, [nx + 1, ny + 1, nz + 1], (600, 3)) / np.array([nx, ny, nz]))).astype(np.float32)
    P[400:1000] = lattice                                                             # on the voxel borders
    P[1000] = (np.nan, 0.0, 0.0)
    index = np.arange(1, nx * ny * nz + 1, dtype=np.uint32).reshape(nz, ny, nx)       # id = linear index + 1
    ids = ov.voxel_ids(vol, index, P)
    ijk = (C.c_int32 * 3)()
    inside = 0
    for p, k in zip(P, ids):
        pt = abi.vec3(*[float(c) for c in p])
        rc = lib.svr_region_seed_from_world(C.byref(vol), nx, ny, nz, C.byref(pt), ijk)
        lib.svr_clear_error()
        if rc != 0:
            assert rc == -3 and k == 0, (p, k)
        else:
            assert k == (ijk[2] * ny + ijk[1]) * nx + ijk[0] + 1, (p, k, list(ijk))
            inside += 1
    assert 1000 < inside < 3900 and (ids[:300] != 0).any() and ids[1000] == 0
    far = ov.voxel_ids(vol, index, hi[None])
    assert far[0] == nx * ny * nz                                                     # the far corner belongs to the last voxel


# ------------------------------------------------------------------------------------------------ symbols, defaults
def test_symbols_structs_and_constants(lib):
    names = ["svr_overlay_style_default", "svr_overlay_palette_default", "svr_slice_ids", "svr_hit_ids", "svr_overlay_ids", "svr_overlay_slice",
             "svr_overlay_last_ms"]
    raw = C.CDLL(str(abi.library_path()))
    for n in names:
        assert n in abi.PROTOTYPES and hasattr(raw, n), n
        assert re.search(rf"\b{n}\s*\(", HEADER), n
    for method in ("slice_ids", "hit_ids", "overlay_ids", "overlay_slice", "overlay_last_ms", "overlay_style"):
        assert callable(getattr(host.Device, method))
    for method in ("paint_slice_overlay", "paint_overlay"):
        assert callable(getattr(host.Canvas, method))
    assert abi.OVERLAY_MAX_PALETTE == int(re.search(r"#define\s+SVR_OVERLAY_MAX_PALETTE\s+(\d+)", HEADER).group(1)) == 256
    assert abi.OVERLAY_DEFAULT_PALETTE == int(re.search(r"#define\s+SVR_OVERLAY_DEFAULT_PALETTE\s+(\d+)", HEADER).group(1)) >= 12
    S, T = abi.OverlaySource, abi.OverlayStyle
    assert C.sizeof(S) == 16 and S.labels_device.offset == 8
    assert C.sizeof(T) == 24 and (T.fill_alpha.offset, T.edge_alpha.offset, T.palette_count.offset, T.flags.offset, T.palette.offset) == (0, 4, 8, 12, 16)


def test_defaults(lib):
    st = abi.OverlayStyle(1, 2, 3, 4, C.cast(8, C.POINTER(C.c_uint32)))
    assert lib.svr_overlay_style_default(C.byref(st)) == 0                            # plain host code: no GPU needed
    assert (st.fill_alpha, st.edge_alpha, st.palette_count, st.flags, bool(st.palette)) == (96, 255, 0, 0, False)
    n = abi.OVERLAY_DEFAULT_PALETTE
    pal = np.zeros(n + 1, dtype=np.uint32)
    ptr = pal.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.svr_overlay_palette_default(ptr, n) == 0 and pal[n] == 0
    rgba = ov.unpack_palette(pal[:n])
    assert rgba[:12, :3].tolist() == [list(c) for c in DEFAULT_RGB] and (rgba[:, 3] == 255).all()
    for c in DEFAULT_RGB:
        assert re.search(rf"\({c[0]}, {c[1]}, {c[2]}\)", HEADER), c                  # the values are written in the header
    d = np.abs(rgba[:, None, :3] - rgba[None, :, :3]).sum(axis=-1) + 1000 * np.eye(n, dtype=np.int64)
    assert d.min() >= 100                                                             # visibly distinct: every pair differs by 100 of 765 summed over the channels
    first = np.zeros(3, dtype=np.uint32)
    assert lib.svr_overlay_palette_default(first.ctypes.data_as(C.POINTER(C.c_uint32)), 3) == 0 and np.array_equal(first, pal[:3])
    ms = C.c_float(-1.0)
    assert lib.svr_overlay_last_ms(C.byref(ms)) == 0 and ms.value >= 0.0             # (0 when no overlay call has run in this process)
    for call, want in ((lambda: lib.svr_overlay_style_default(None), -4), (lambda: lib.svr_overlay_palette_default(None, 3), -4),
                       (lambda: lib.svr_overlay_palette_default(ptr, n + 1), -3), (lambda: lib.svr_overlay_last_ms(None), -4)):
        assert call() == want and lib.svr_last_error()
        lib.svr_clear_error()


# ------------------------------------------------------------------------------------------------ refusals: before the device is touched
FAKE = 0x1000                                                                         # a "device pointer" that no refused call may look at


class Args:
    """the arguments of the four device calls with valid defaults; a refusal test replaces one"""

    def __init__(self, lib):
        self.lib = lib
        self.vol = ov.reference("crop").vol
        self.p = host.slice_params_axis(lib, self.vol, 2, 0.5, 32, 24)
        self.pal = np.arange(1, 6, dtype=np.uint32)
        self.keep = []

    def source(self, mask=FAKE, labels=None):
        s = abi.OverlaySource(mask, labels)
        self.keep.append(s)
        return C.byref(s)

    def style(self, fill=96, edge=255, count=5, flags=0, palette=True):
        ptr = self.pal.ctypes.data_as(C.POINTER(C.c_uint32)) if palette else None
        s = abi.OverlayStyle(fill, edge, count, flags, ptr)
        self.keep.append(s)
        return C.byref(s)

    def params(self, **kw):
        q = abi.SliceParams.from_buffer_copy(self.p)
        for k, v in kw.items():
            setattr(q, k, v)
        self.keep.append(q)
        return C.byref(q)

    def call(self, name, **kw):
        a = dict(out=FAKE, vol=C.byref(self.vol), dims=(37, 21, 13), w=32, h=24, p=self.params(), count=1, spacing=0.0, source=self.source(),
                 style=self.style(), hits=FAKE, ids=FAKE)
        a.update(kw)
        sp = C.c_float(a["spacing"])
        if name == "svr_slice_ids":
            return self.lib.svr_slice_ids(a["out"], a["vol"], *a["dims"], a["w"], a["h"], a["p"], a["count"], sp, a["source"])
        if name == "svr_overlay_slice":
            return self.lib.svr_overlay_slice(a["out"], a["vol"], *a["dims"], a["w"], a["h"], a["p"], a["count"], sp, a["source"], a["style"])
        if name == "svr_hit_ids":
            return self.lib.svr_hit_ids(a["out"], a["hits"], a["w"], a["h"], a["vol"], *a["dims"], a["source"])
        return self.lib.svr_overlay_ids(a["out"], a["ids"], a["w"], a["h"], a["count"], a["style"])


SLICE_CALLS = ("svr_slice_ids", "svr_overlay_slice")
SOURCE_CALLS = SLICE_CALLS + ("svr_hit_ids",)
STYLE_CALLS = ("svr_overlay_slice", "svr_overlay_ids")
ALL_CALLS = SOURCE_CALLS + ("svr_overlay_ids",)


def test_refusals(lib):
    A = Args(lib)
    inf, nan = float("inf"), float("nan")
    cases = []                                                                        # (calls, code, what, arguments)
    cases += [(ALL_CALLS, -4, "null output", dict(out=None))]
    cases += [(SOURCE_CALLS, -4, "null volume", dict(vol=None)), (SOURCE_CALLS, -4, "null source", dict(source=None))]
    cases += [(SLICE_CALLS, -4, "null params", dict(p=None)), (STYLE_CALLS, -4, "null style", dict(style=None))]
    cases += [(("svr_hit_ids",), -4, "null hits", dict(hits=None)), (("svr_overlay_ids",), -4, "null ids", dict(ids=None))]
    for dims in ((0, 21, 13), (37, -1, 13), (37, 21, 0), (2048, 2048, 1024)):
        cases += [(SOURCE_CALLS, -6, f"dimensions {dims}", dict(dims=dims))]
    cases += [(SOURCE_CALLS, -3, "both sources", dict(source=A.source(FAKE, FAKE))), (SOURCE_CALLS, -3, "no source", dict(source=A.source(None, None)))]
    cases += [(STYLE_CALLS, -3, "fill_alpha 256", dict(style=A.style(fill=256))), (STYLE_CALLS, -3, "edge_alpha 256", dict(style=A.style(edge=256))),
              (STYLE_CALLS, -3, "flags", dict(style=A.style(flags=1))), (STYLE_CALLS, -3, "palette_count 257", dict(style=A.style(count=257))),
              (STYLE_CALLS, -3, "a count without a palette", dict(style=A.style(count=5, palette=False))),
              (STYLE_CALLS, -3, "a palette without a count", dict(style=A.style(count=0)))]
    cases += [(ALL_CALLS, -3, "w = 0", dict(w=0)), (ALL_CALLS, -3, "h = 0", dict(h=0))]
    cases += [(SLICE_CALLS + ("svr_overlay_ids",), -3, "count = 0", dict(count=0))]
    # what svr_render_slice_stack refuses about center, u, v, thickness, step, count and spacing
    v3 = abi.vec3
    cases += [(SLICE_CALLS, -3, what, dict(p=A.params(**kw))) for what, kw in (
        ("center NaN", dict(center=v3(nan, 0, 0))), ("u infinite", dict(u=v3(inf, 0, 0))), ("v NaN", dict(v=v3(0, nan, 0))),
        ("thickness NaN", dict(thickness=nan)), ("step infinite", dict(step=inf)), ("thickness < 0", dict(thickness=-1.0)),
        ("a slab with step 0", dict(thickness=2.0, step=0.0)), ("a slab with step < 0", dict(thickness=2.0, step=-1.0)),
        ("too many samples", dict(thickness=4096.0, step=1.0)), ("u parallel to v", dict(u=v3(1, 0, 0), v=v3(2, 0, 0))),
        ("u = 0", dict(u=v3(0, 0, 0))))]
    cases += [(SLICE_CALLS, -3, "spacing NaN", dict(spacing=nan)), (SLICE_CALLS, -3, "2^32 tile tasks", dict(w=1 << 17, h=1 << 17, count=1 << 4))]
    bad_vol = abi.cudaVolume.from_buffer_copy(A.vol)
    bad_vol.bbox.invSize.y = nan
    cases += [(SOURCE_CALLS, -3, "a non-finite bbox", dict(vol=C.byref(bad_vol)))]
    n = 0
    for calls, code, what, kw in cases:
        for name in calls:
            rc = A.call(name, **kw)
            msg = lib.svr_last_error().decode()
            assert rc == code == lib.svr_last_error_code() and name in msg, (name, what, rc, msg)
            if code == -6:                                                            # the text of the volume ops' shared dimension check
                d = kw["dims"]
                want = (f"{name}: bad dimensions {d[0]} x {d[1]} x {d[2]}" if min(d) <= 0 else
                        f"{name}: {d[0]} x {d[1]} x {d[2]} is more than 2^31 voxels")
                assert msg == want, (msg, want)
            lib.svr_clear_error()
            n += 1
    assert n == sum(len(c[0]) for c in cases) > 80


def test_mode_window_and_colour_flag_are_not_looked_at(lib):
    """...so a refusal that follows them in svr_render_slice_stack's order is still reached: the params are accepted up to the last check"""
    A = Args(lib)
    for kw in (dict(mode=77), dict(window_lo=1.0, window_hi=0.0), dict(window_lo=float("nan")), dict(flags=abi.SLICE_COLOR_TF)):
        rc = A.call("svr_slice_ids", p=A.params(**kw), w=1 << 17, h=1 << 17, count=1 << 4)
        msg = lib.svr_last_error().decode()
        lib.svr_clear_error()
        assert rc == -3 and "tile tasks" in msg, (kw, msg)


# ------------------------------------------------------------------------------------------------ the fixtures of the GPU tests
@pytest.mark.parametrize("source_name", ov.SOURCES)
@pytest.mark.parametrize("size", ov.IMAGES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_slice_fixture_conditions(source_name, size):
    w, h = size
    R, src = ov.reference(ov.scene_of(source_name)), ov.source(source_name)
    win = ov.window_of(w, h)
    assert win[0] % 2 == win[1] % 2 == 1 and 0 < win[0] < win[2] < w and 0 < win[1] < win[3] < h
    seam8 = seam16 = border = False
    for what, p in ov.cases(source_name, w, h):
        is_slab = p.thickness > 0
        assert ov.sr.sample_count(p.thickness, p.step) == (9 if is_slab else 1), what
        ids, counting, centre = ov.slice_ids(R, p, w, h, src, want_centre=True)
        distinct = np.unique(ids)
        if src.dtype == bool:
            assert distinct.tolist() == [0, 1], what
        else:
            assert len(distinct[distinct != 0]) >= 3, what
        e = ov.edges(ids)
        assert e.any() and ((ids != 0) & ~e).any(), f"{what}: edge and non-edge pixels"
        assert (counting == 0).any() and (counting > 0).any(), f"{what}: a pixel without a counting sample"
        if is_slab:
            assert (ids != centre).any(), f"{what}: a slab pixel whose id is not its centre plane's"
        seam8 |= ov.seam(ids, 8)
        seam16 |= ov.seam(ids, 16)
        border |= ov.crosses_window(ids, win)
    assert seam8 and seam16, "an id boundary on a seam of 8 and of 16 pixels, in x and in y"
    assert border, "an id boundary on the border of the render window"
    if source_name == "patched":
        assert src.max() == 0xFFFFFFFF and ((src > abi.OVERLAY_MAX_PALETTE) & (src < 0xFFFFFFFF)).any()
    pads = (-src.shape[2]) % 32
    assert pads in (16, 27)                                                           # padding bits per mask row: 48 -> 16, 37 -> 27


def test_stack_slices_differ():
    count, spacing = ov.STACK
    for source_name in ov.SOURCES:
        for w, h in ov.IMAGES:
            R, src = ov.reference(ov.scene_of(source_name)), ov.source(source_name)
            for what, p in ov.cases(source_name, w, h)[5::2]:
                ids = [ov.slice_ids(R, p, w, h, src, k, spacing)[0] for k in range(count)]
                assert not np.array_equal(ids[0], ids[1]) and not np.array_equal(ids[1], ids[2]), what


@pytest.mark.parametrize("source_name", ov.HIT_SOURCES)
def test_hit_fixture_conditions(source_name):
    sc, src = ov.scene("head"), ov.source(source_name)
    H = hr.reference("tiny_head", lambda: sc)
    for mode, alpha, iso, mname in ov.HIT_MODES:
        hits, _ = H.hit_map(mode, sc.step_size(), alpha, iso)
        ids = ov.hit_ids(ov.reference("head").vol, src, hits)
        status = hits["status"]
        assert all((status == s).any() for s in (abi.HIT_STATUS_MISS, abi.HIT_STATUS_NONE, abi.HIT_STATUS_FOUND)), mname
        assert (ids[status != abi.HIT_STATUS_FOUND] == 0).all()
        distinct = np.unique(ids[ids != 0])
        assert len(distinct) == 1 if src.dtype == bool else len(distinct) >= 3, (mname, distinct)
        e = ov.edges(ids)
        assert e.any() and ((ids != 0) & ~e).any(), mname
