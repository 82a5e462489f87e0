"""The scissor calls without a GPU (include/svr_abi.h, "scissors"): every refusal, the two host projections against the
numpy reference bit for bit, the round trip pixel -> ray or plane point -> pixel, the voxel centres against svr_region_seed_from_world,
and the argument checks of the Python layer on the fake device."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import scissor_ref as sr
from tests.host_fake import FakeDevice

f32 = np.float32
ROOT = Path(__file__).resolve().parents[1]
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    return lib


def volume_of(dim, spacing):
    return host.create_device_volume(0, dim, spacing, 1.0)


def cameras(dim=(48, 48, 48), spacing=(1.0, 1.0, 1.0), W=64, H=48):
    """three cameras: the default one on +z (axis-aligned frame), an oblique one outside the box, one inside the box.  The projection
    takes the frame to be orthonormal; camera_setup leaves u and v shorter than 1 when `up` is not perpendicular to the view direction,
    so they are normalised here."""
    eye = host.zoom_to_extent_eye_dist(host.volume_size(dim, spacing), 45.0)
    cams = [host.camera_setup((0.0, 0.0, eye), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.0, 1.0, 1.0, W, H),
            host.camera_setup((70.0, -40.0, 55.0), (2.0, 1.0, -3.0), (0.0, 0.0, 1.0), 35.0, 0.0, 1.0, 1.0, W, H),
            host.camera_setup((3.0, 2.0, 5.0), (0.0, -4.0, -30.0), (0.0, 1.0, 0.0), 60.0, 0.0, 1.0, 1.0, W, H)]
    for cam in cams:
        cam.u, cam.v = host._to_vec3(host._normalize(cam.u.tuple())), host._to_vec3(host._normalize(cam.v.tuple()))
    return cams


def oblique_slice(W, H, pixel=0.8):
    """a slice whose u and v are perpendicular up to float32 rounding, on no axis"""
    th, ph = 0.6, 0.4
    p = abi.SliceParams()
    p.center = abi.vec3(1.5, -2.25, 0.75)
    p.u = abi.vec3(pixel * math.cos(th), pixel * math.sin(th), 0.0)
    p.v = abi.vec3(-pixel * math.sin(th) * math.cos(ph), pixel * math.cos(th) * math.cos(ph), pixel * math.sin(ph))
    p.thickness, p.step, p.mode, p.flags, p.window_lo, p.window_hi = 0.0, 1.0, abi.SLAB_MIP, 0, 0.0, 1.0
    return p


def slices(lib, vol, W=64, H=48):
    """axial, coronal, oblique"""
    return [host.slice_params_axis(lib, vol, 2, 0.4, W, H), host.slice_params_axis(lib, vol, 1, 0.55, W, H), oblique_slice(W, H)]


def lib_project(lib, view, points, w=None, h=None):
    """(seen, x, y, depth) of the library's host projection for float32 points [n][3]"""
    n = len(points)
    seen, x, y, depth = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float32)
    xy, d, pt = (C.c_int32 * 2)(), C.c_float(0.0), abi.vec3()
    for i in range(n):
        pt.x, pt.y, pt.z = float(points[i, 0]), float(points[i, 1]), float(points[i, 2])
        if w is None:
            rc = lib.svr_scissor_project_camera(C.byref(view), C.byref(pt), xy, C.byref(d))
        else:
            rc = lib.svr_scissor_project_slice(C.byref(view), w, h, C.byref(pt), xy, C.byref(d))
        assert rc in (0, 1), (rc, lib.svr_last_error())
        assert (rc == 1) == (xy[0] == -1 and xy[1] == -1)
        seen[i], x[i], y[i], depth[i] = rc == 0, xy[0], xy[1], d.value
    return seen, x, y, depth


def same_projection(got, want, what):
    for g, w_, name in zip(got[:3], want[:3], ("seen", "x", "y")):
        assert np.array_equal(g, w_), (what, name, np.nonzero(g != w_)[0][:5])
    assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32)), (what, "depth")


# ------------------------------------------------------------------------------------------------ layouts and defaults
def test_struct_size_and_defaults(lib):
    assert C.sizeof(abi.ScissorParams) == 16
    p = abi.ScissorParams(7, 1.0, 2.0, 9)
    assert lib.svr_scissor_params_default(C.byref(p)) == 0
    assert (p.op, p.depth_lo, p.depth_hi, p.flags) == (abi.SCISSOR_SELECT, -INF, INF, 0)
    q = host.scissor_params(abi.SCISSOR_FILL_INSIDE, (-1.5, 2.5))
    assert (q.op, q.depth_lo, q.depth_hi, q.flags) == (3, -1.5, 2.5, 0)


def test_header_constants_are_the_python_ones():
    header = (ROOT / "include" / "svr_abi.h").read_text()
    for name, value in (("SVR_STENCIL_MAX_VERTICES", abi.STENCIL_MAX_VERTICES), ("SVR_STENCIL_MAX_COORD", abi.STENCIL_MAX_COORD),
                        ("SVR_SCISSOR_SELECT", abi.SCISSOR_SELECT), ("SVR_SCISSOR_ERASE_INSIDE", abi.SCISSOR_ERASE_INSIDE),
                        ("SVR_SCISSOR_ERASE_OUTSIDE", abi.SCISSOR_ERASE_OUTSIDE), ("SVR_SCISSOR_FILL_INSIDE", abi.SCISSOR_FILL_INSIDE)):
        m = re.search(rf"^#define {name}\s+(\d+)", header, flags=re.M)
        assert m and int(m.group(1)) == value, name


def test_the_edge_chunk_is_a_named_constant():
    src = (ROOT / "sunvolumerender_amd" / "csrc" / "svr_scissor.hip").read_text()
    m = re.search(r"constexpr int STENCIL_EDGE_CHUNK = (\d+);", src)
    assert m and 1 < int(m.group(1)) < abi.STENCIL_MAX_VERTICES      # so that a polygon can have more edges than a chunk


def test_stencil_rect(lib):
    assert np.array_equal(host.stencil_rect(3, 5, 3, 5, lib), [[3, 5], [4, 5], [4, 6], [3, 6]])
    r = host.stencil_rect(-2, 0, 9, 4, lib)
    assert np.array_equal(r, [[-2, 0], [10, 0], [10, 5], [-2, 5]])
    inside = sr.fill([r], 12, 7)
    want = np.zeros((7, 12), bool)
    want[0:5, 0:10] = True
    assert np.array_equal(inside, want)


# ------------------------------------------------------------------------------------------------ the reference's fill
def test_reference_fill_half_open_rule_and_tiling():
    # a rectangle whose sides pass through pixel centres: the half-open rule gives each centre on a side to exactly one side
    rect = np.array([[1.5, 1.5], [5.5, 1.5], [5.5, 4.5], [1.5, 4.5]])
    img = sr.fill([rect], 8, 6)
    assert img.sum() == 4 * 3 and img[1:4, 1:5].all()
    # two polygons that share an edge through pixel centres tile their union
    a = np.array([[0.5, 0.5], [4.5, 0.5], [2.5, 6.5], [0.5, 6.5]])
    b = np.array([[4.5, 0.5], [7.5, 0.5], [7.5, 6.5], [2.5, 6.5]])
    u = np.array([[0.5, 0.5], [7.5, 0.5], [7.5, 6.5], [0.5, 6.5]])
    fa, fb, fu = sr.fill([a], 9, 8), sr.fill([b], 9, 8), sr.fill([u], 9, 8)
    assert not (fa & fb).any() and np.array_equal(fa | fb, fu) and fa.any() and fb.any()
    # a hole
    outer, inner = np.array([[1, 1], [9, 1], [9, 9], [1, 9]]), np.array([[3, 3], [6, 3], [6, 6], [3, 6]])
    img = sr.fill([outer, inner], 10, 10)
    assert img[1:9, 1:9].sum() == 64 - 9 and not img[3:6, 3:6].any()


# ------------------------------------------------------------------------------------------------ refusals
class Buffers:
    """host buffers standing in for device memory: the refused calls never read them"""

    def __init__(self):
        self.keep = []

    def __call__(self, nbytes=256):
        self.keep.append((C.c_uint8 * nbytes)())
        return C.cast(self.keep[-1], C.c_void_p)


def refuse(lib, name, *args):
    lib.svr_clear_error()
    rc = getattr(lib, name)(*args)
    text = lib.svr_last_error().decode()
    assert lib.svr_last_error_code() == rc
    lib.svr_clear_error()
    return rc, text


def _verts(*xy):
    return (C.c_int32 * len(xy))(*xy)


def _counts(*n):
    return (C.c_uint32 * len(n))(*n)


TRI = (0, 0, 2560, 0, 0, 2560)
BIG = 1 << 23


def polygon_refusals():
    buf = Buffers()
    out = buf()
    ok = (_verts(*TRI), _counts(3), 1, 16, 16, out)

    def with_(**kw):
        names = ("v", "c", "n", "w", "h", "out")
        a = dict(zip(names, ok))
        a.update(kw)
        return tuple(a[k] for k in names)
    many = _verts(*([0, 0, 256, 0, 0, 256] * 1366))          # 4098 vertices in 1366 triangles
    return buf, [
        (with_(v=None), -4, "null"), (with_(c=None), -4, "null"), (with_(out=None), -4, "null"),
        (with_(n=0), -3, "ncontours"), (with_(w=0), -3, "image size"), (with_(h=0), -3, "image size"),
        (with_(w=1 << 16, h=(1 << 15) + 1), -3, "2^31"),
        (with_(c=_counts(2)), -3, "at least 3"),
        (with_(v=_verts(*(TRI + TRI)), c=_counts(3, 2), n=2), -3, "contour 1"),
        (with_(v=many, c=_counts(*([3] * 1366)), n=1366), -3, "4096"),
        (with_(v=_verts(0, 0, BIG + 1, 0, 0, 256)), -3, "2^23"),
        (with_(v=_verts(0, 0, 256, -BIG - 1, 0, 256)), -3, "2^23"),
    ]


_POLY_BUF, POLY = polygon_refusals()


@pytest.mark.parametrize("k", range(len(POLY)))
def test_polygon_refusals(lib, k):
    args, code, word = POLY[k]
    rc, text = refuse(lib, "svr_stencil_polygon", *args)
    assert rc == code and "svr_stencil_polygon" in text and word in text, (rc, text)


def test_rect_and_default_refusals(lib):
    q = (C.c_int32 * 8)()
    for args, code, word in (((0, 0, 1, 1, None), -4, "null"), ((2, 0, 1, 5, q), -3, "inverted"), ((0, 3, 1, 2, q), -3, "inverted"),
                             ((0, 0, 32768, 1, q), -3, "2^23"), ((-32769, 0, 1, 1, q), -3, "2^23")):
        rc, text = refuse(lib, "svr_stencil_rect", *args)
        assert rc == code and "svr_stencil_rect" in text and word in text, (rc, text)
    assert lib.svr_stencil_rect(-32768, -32768, 32767, 32767, q) == 0        # the corners at the limit itself are taken
    rc, text = refuse(lib, "svr_scissor_params_default", None)
    assert rc == -4 and "svr_scissor_params_default" in text
    rc, text = refuse(lib, "svr_region_scissor_last_ms", None)
    assert rc == -4 and "svr_region_scissor_last_ms" in text


def _camera(**kw):
    cam = cameras()[1]
    cam = abi.cudaCamera.from_buffer_copy(cam)
    for k, v in kw.items():
        if k in ("pos", "u", "v", "w"):
            setattr(cam, k, abi.vec3(*v))
        else:
            setattr(cam, k, v)
    return cam


def _slice(**kw):
    p = abi.SliceParams.from_buffer_copy(oblique_slice(64, 48))
    for k, v in kw.items():
        setattr(p, k, abi.vec3(*v))
    return p


NAN = float("nan")
BAD_CAMERAS = [(dict(imageW=0), "image size"), (dict(imageH=0), "image size"), (dict(imageW=1 << 16, imageH=(1 << 15) + 1), "2^31"),
               (dict(pos=(NAN, 0, 0)), "finite"), (dict(u=(0, INF, 0)), "finite"), (dict(v=(0, 0, NAN)), "finite"), (dict(w=(-INF, 0, 0)), "finite"),
               (dict(tanFovxOverTwo=0.0), "tanFovxOverTwo"), (dict(tanFovxOverTwo=-1.0), "tanFovxOverTwo"), (dict(tanFovxOverTwo=INF), "tanFovxOverTwo"),
               (dict(tanFovxOverTwo=NAN), "tanFovxOverTwo"), (dict(aspectRatio=0.0), "aspectRatio"), (dict(aspectRatio=NAN), "aspectRatio"),
               (dict(aspectRatio=INF), "aspectRatio")]
BAD_SLICES = [(dict(center=(NAN, 0, 0)), 64, 48, "finite"), (dict(u=(INF, 0, 0)), 64, 48, "finite"), (dict(v=(0, NAN, 0)), 64, 48, "finite"),
              (dict(u=(0, 0, 0)), 64, 48, "cross"), (dict(u=(1, 2, 3), v=(2, 4, 6)), 64, 48, "cross"), (dict(u=(1e-30, 0, 0), v=(0, 1e-30, 0)), 64, 48, "cross"),
              (dict(), 0, 48, "image size"), (dict(), 64, 0, "image size"), (dict(), 1 << 16, (1 << 15) + 1, "2^31")]


@pytest.mark.parametrize("k", range(len(BAD_CAMERAS)))
def test_camera_refusals_of_the_projection_and_the_prism(lib, k):
    kw, word = BAD_CAMERAS[k]
    cam, pt, xy, d = _camera(**kw), abi.vec3(0, 0, 0), (C.c_int32 * 2)(), C.c_float()
    rc, text = refuse(lib, "svr_scissor_project_camera", C.byref(cam), C.byref(pt), xy, C.byref(d))
    assert rc == -3 and "svr_scissor_project_camera" in text and word in text, (rc, text)
    buf = Buffers()
    vol, p = volume_of((5, 4, 3), (1, 1, 1)), host.scissor_params()
    rc, text = refuse(lib, "svr_region_scissor_camera", buf(), 5, 4, 3, C.byref(vol), C.byref(cam), buf(), C.byref(p), buf())
    assert rc == -3 and "svr_region_scissor_camera" in text and word in text, (rc, text)


@pytest.mark.parametrize("k", range(len(BAD_SLICES)))
def test_slice_refusals_of_the_projection_and_the_prism(lib, k):
    kw, w, h, word = BAD_SLICES[k]
    sl, pt, xy, d = _slice(**kw), abi.vec3(0, 0, 0), (C.c_int32 * 2)(), C.c_float()
    rc, text = refuse(lib, "svr_scissor_project_slice", C.byref(sl), w, h, C.byref(pt), xy, C.byref(d))
    assert rc == -3 and "svr_scissor_project_slice" in text and word in text, (rc, text)
    buf = Buffers()
    vol, p = volume_of((5, 4, 3), (1, 1, 1)), host.scissor_params()
    rc, text = refuse(lib, "svr_region_scissor_slice", buf(), 5, 4, 3, C.byref(vol), C.byref(sl), w, h, buf(), C.byref(p), buf())
    assert rc == -3 and "svr_region_scissor_slice" in text and word in text, (rc, text)


def test_projection_null_refusals(lib):
    cam, sl, pt, xy, d = _camera(), _slice(), abi.vec3(0, 0, 0), (C.c_int32 * 2)(), C.c_float()
    ok = [C.byref(cam), C.byref(pt), xy, C.byref(d)]
    for i in range(4):
        args = list(ok)
        args[i] = None
        rc, text = refuse(lib, "svr_scissor_project_camera", *args)
        assert rc == -4 and "svr_scissor_project_camera" in text
    ok = [C.byref(sl), 64, 48, C.byref(pt), xy, C.byref(d)]
    for i in (0, 3, 4, 5):
        args = list(ok)
        args[i] = None
        rc, text = refuse(lib, "svr_scissor_project_slice", *args)
        assert rc == -4 and "svr_scissor_project_slice" in text


@pytest.mark.parametrize("call", ["svr_region_scissor_camera", "svr_region_scissor_slice"])
def test_prism_refusals(lib, call):
    buf = Buffers()
    vol, cam, sl = volume_of((5, 4, 3), (1, 1, 1)), _camera(), _slice()
    base = dict(in_=buf(), dims=(5, 4, 3), vol=C.byref(vol), stencil=buf(), p=host.scissor_params(abi.SCISSOR_ERASE_INSIDE), out=buf())

    def run(**kw):
        a = dict(base)
        a.update(kw)
        p = a["p"]
        view = (C.byref(cam),) if call.endswith("camera") else (C.byref(sl), 64, 48)
        if "view" in kw:
            view = (None,) + view[1:]
        rc, text = refuse(lib, call, a["in_"], *a["dims"], a["vol"], *view, a["stencil"], None if p is None else C.byref(p), a["out"])
        assert call in text, text
        return rc, text

    for kw in (dict(in_=None), dict(vol=None), dict(view=None), dict(stencil=None), dict(p=None), dict(out=None)):
        assert run(**kw)[0] == -4, kw
    # in may be NULL with SELECT: the call gets past the null check (to the dimensions, here)
    assert run(in_=None, p=host.scissor_params(abi.SCISSOR_SELECT), dims=(0, 4, 3))[0] == -6
    for dims in ((0, 4, 3), (5, -1, 3), (5, 4, 0), (2048, 2048, 513)):
        assert run(dims=dims)[0] == -6, dims
    for p, word in ((abi.ScissorParams(4, -INF, INF, 0), "op"), (abi.ScissorParams(-1, -INF, INF, 0), "op"), (abi.ScissorParams(0, -INF, INF, 1), "flags"),
                    (abi.ScissorParams(0, NAN, INF, 0), "depth"), (abi.ScissorParams(0, 0.0, NAN, 0), "depth"), (abi.ScissorParams(0, 2.0, 1.0, 0), "depth")):
        rc, text = run(p=p)
        assert rc == -3 and word in text, (rc, text)
    for member in ("vmin", "vmax"):
        for bad in (NAN, INF):
            v = volume_of((5, 4, 3), (1, 1, 1))
            setattr(v.bbox, member, abi.vec3(0.0, bad, 0.0))
            rc, text = run(vol=C.byref(v))
            assert rc == -3 and "bbox" in text, (rc, text)
    # equal depth bounds are an interval
    rc, text = run(p=abi.ScissorParams(0, 1.0, 1.0, 0), dims=(0, 1, 1))
    assert rc == -6


# ------------------------------------------------------------------------------------------------ the projections, bit for bit
def world_points(rng, n, extent=60.0):
    return (rng.uniform(-extent, extent, (n, 3))).astype(np.float32)


def test_project_camera_is_the_reference(lib):
    rng = np.random.default_rng(21)
    for k, cam in enumerate(cameras()):
        pos, u, v = (np.array(t.tuple(), np.float32) for t in (cam.pos, cam.u, cam.v))
        special = np.stack([pos, pos + u * f32(1.5) - v * f32(2.0), pos + u, pos * f32(1.0000001)])     # at the pinhole and beside it
        pts = np.concatenate([world_points(rng, 3000), special.astype(np.float32)])
        want = sr.project_camera(cam, pts)
        got = lib_project(lib, cam, pts)
        same_projection(got, want, f"camera {k}")
        seen, _, _, depth = want
        assert seen.any() and (~seen & (depth > 0)).any(), "points in front that are off the image"
        assert (depth < 0).any() and not seen[depth <= 0].any(), "points behind the pinhole"
        assert not seen[len(pts) - 4], "c = 0 at the pinhole itself"
        if k == 0:                                            # the axis-aligned frame: c is exactly 0 beside the pinhole
            assert want[3][len(pts) - 3] == 0 and not seen[len(pts) - 3]


def test_project_slice_is_the_reference(lib):
    rng = np.random.default_rng(22)
    vol = volume_of((48, 40, 30), (1.0, 1.2, 2.0))
    for k, sl in enumerate(slices(lib, vol)):
        pts = world_points(rng, 3000, 40.0)
        want = sr.project_slice(sl, 64, 48, pts)
        got = lib_project(lib, sl, pts, 64, 48)
        same_projection(got, want, f"slice {k}")
        assert want[0].any() and (~want[0]).any() and (want[3] < 0).any() and (want[3] > 0).any()
    # the python wrappers say the same
    xy, depth = host.scissor_project_slice(sl, 64, 48, pts[0], lib)
    assert (xy is not None) == bool(want[0][0]) and f32(depth) == want[3][0]
    cam = cameras()[0]
    xy, depth = host.scissor_project_camera(cam, (0.0, 0.0, 0.0), lib)
    assert xy is not None and abs(xy[0] - 32) <= 1 and abs(xy[1] - 24) <= 1 and depth > 0
    assert host.scissor_project_camera(cam, cam.pos.tuple(), lib)[0] is None


@pytest.mark.parametrize("size", [(64, 48), (333, 77)])
def test_camera_round_trip(lib, size):
    """the point at three ray parameters on the centre ray of every pixel projects to that pixel: no exception"""
    W, H = size
    ys, xs = np.mgrid[0:H, 0:W]
    for cam in cameras(W=W, H=H)[:2]:
        for t in (0.37, 5.1, 123.4):
            pts = sr.camera_ray_point(cam, xs.ravel(), ys.ravel(), t)
            seen, x, y, depth = lib_project(lib, cam, pts)
            assert seen.all() and np.array_equal(x, xs.ravel()) and np.array_equal(y, ys.ravel()), (size, t, int((~seen).sum()))
            assert (depth > 0).all()
            ref = sr.project_camera(cam, pts)
            assert ref[0].all() and np.array_equal(ref[1], x) and np.array_equal(ref[2], y)


@pytest.mark.parametrize("size", [(64, 48), (333, 77)])
def test_slice_round_trip(lib, size):
    W, H = size
    vol = volume_of((48, 40, 30), (1.0, 1.2, 2.0))
    ys, xs = np.mgrid[0:H, 0:W]
    for sl in slices(lib, vol, W, H):
        for off in (0.0, 1.75, -3.5):
            pts = sr.slice_plane_point(sl, W, H, xs.ravel(), ys.ravel(), off)
            seen, x, y, depth = lib_project(lib, sl, pts, W, H)
            assert seen.all() and np.array_equal(x, xs.ravel()) and np.array_equal(y, ys.ravel()), (size, off)
            assert np.abs(depth - f32(off)).max() < 1e-4


@pytest.mark.parametrize("dim,spacing", [((5, 4, 97), (0.7, 1.3, 2.1)), ((7, 1, 1), (1.5, 0.4, 3.0))])
def test_voxel_centres_map_back_to_their_voxel(lib, dim, spacing):
    vol = volume_of(dim, spacing)
    nx, ny, nz = dim
    P = sr.voxel_centres((nz, ny, nx), vol)
    assert P.dtype == np.float32
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                assert host.region_seed_from_world(lib, vol, dim, P[k, j, i]) == (i, j, k)


# ------------------------------------------------------------------------------------------------ the Python layer on the fake device
TRI_PX = np.array([[1.0, 1.0], [9.0, 2.0], [4.0, 8.0]])


def raises_before_any_call(fn, *args, **kw):
    dev = FakeDevice()
    with pytest.raises(ValueError):
        getattr(dev, fn)(*args, **kw)
    assert dev.lib.calls == [] and dev.live == set() and dev.nmalloc == 0


def test_stencil_polygon_argument_errors():
    for contours in ([], [TRI_PX[:2]], [np.zeros((3, 3))], [np.zeros(6)], [TRI_PX, np.array([[0, 0], [1, NAN], [2, 2.0]])],
                     [np.array([[0, 0], [32768.01, 0], [0, 5.0]])], [np.zeros((4097, 2))], [np.zeros((2049, 2)), np.zeros((2048, 2))]):
        raises_before_any_call("stencil_polygon", contours, 16, 16)
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 16, (1 << 15) + 1)):
        raises_before_any_call("stencil_polygon", [TRI_PX], w, h)


def test_region_scissor_argument_errors():
    vol, cam, sl = volume_of((5, 4, 3), (1, 1, 1)), cameras(W=16, H=8)[0], oblique_slice(16, 8)
    m, st = np.zeros((3, 4, 5), bool), np.zeros((8, 16), bool)
    E = raises_before_any_call
    E("region_scissor", m, st, vol)                                              # no view
    E("region_scissor", m, st, vol, camera=cam, slice=sl, w=16, h=8)             # two views
    E("region_scissor", m, st, vol, camera=cam, w=16, h=8)                       # w, h with a camera
    E("region_scissor", m, st, vol, slice=sl)                                    # a slice without w, h
    E("region_scissor", m, st, vol, slice=sl, w=16)
    E("region_scissor", m, st, vol, slice=sl, w=0, h=8)
    E("region_scissor", None, st, vol, camera=cam, op=abi.SCISSOR_ERASE_INSIDE, shape=(3, 4, 5))   # only SELECT works without a mask
    E("region_scissor", None, st, vol, camera=cam)                               # no mask and no shape
    E("region_scissor", np.zeros((4, 5), bool), st, vol, camera=cam)             # a mask that is no volume
    E("region_scissor", m, np.zeros((8, 15), bool), vol, camera=cam)             # a stencil of another image
    E("region_scissor", m, np.zeros(9, np.uint32), vol, camera=cam)              # the wrong number of words
    E("region_scissor", m, np.zeros(8, np.int32), vol, camera=cam)
    E("region_scissor", m, None, vol, camera=cam)


def test_fake_device_calls_and_no_leak():
    vol, cam, sl = volume_of((5, 4, 3), (1, 1, 1)), cameras(W=40, H=8)[0], oblique_slice(40, 8)
    m, st = np.zeros((3, 4, 5), bool), np.zeros((8, 40), bool)
    dev = FakeDevice()
    words = dev.stencil_polygon([TRI_PX, TRI_PX + 1], 40, 8)
    assert words.shape == (16,) and words.dtype == np.uint32 and dev.live == set()
    call = dev.lib.calls[-1]
    assert call["fn"] == "svr_stencil_polygon" and call["args"][2:5] == [2, 40, 8]
    out = dev.region_scissor(m, st, vol, camera=cam, op=abi.SCISSOR_ERASE_OUTSIDE, depth=(1.0, 2.0))
    assert out.shape == m.shape and dev.live == set()
    call = dev.lib.calls[-1]
    assert call["fn"] == "svr_region_scissor_camera" and call["args"][1:4] == [5, 4, 3]
    assert call["args"][7] == {"op": 2, "depth_lo": 1.0, "depth_hi": 2.0, "flags": 0}
    dev.region_scissor(None, words, vol, slice=sl, w=40, h=8, shape=(3, 4, 5))
    call = dev.lib.calls[-1]
    assert call["fn"] == "svr_region_scissor_slice" and call["args"][0] is None and call["args"][6:8] == [40, 8] and dev.live == set()
    assert dev.region_scissor_last_ms() == 0.0
    # nothing stays allocated when the library call or an allocation fails
    for fail in (dict(fail_call=1), dict(fail_malloc=1), dict(fail_malloc=2), dict(fail_malloc=3)):
        dev = FakeDevice()
        dev.lib.fail_call, dev.fail_malloc = fail.get("fail_call"), fail.get("fail_malloc")
        with pytest.raises(host.SvrError):
            dev.region_scissor(m, st, vol, camera=cam, op=abi.SCISSOR_FILL_INSIDE)
        assert dev.live == set()
