"""svr_stencil_polygon and svr_region_scissor_camera / _slice on the GPU against the numpy reference (tests/scissor_ref.py), bit for bit:
every stencil word and every mask word, padding included; then the scissors together with the hit maps, the hit ids and the bone window
of the 48^3 head."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import morph_ref as mr
from tests import overlay_ref as ov
from tests import scissor_ref as sr
from tests.test_scissor_cpu import oblique_slice, volume_of

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = Path(__file__).resolve().parents[1]
CHUNK = int(re.search(r"constexpr int STENCIL_EDGE_CHUNK = (\d+);", (ROOT / "sunvolumerender_amd" / "csrc" / "svr_scissor.hip").read_text()).group(1))
OPS = (abi.SCISSOR_SELECT, abi.SCISSOR_ERASE_INSIDE, abi.SCISSOR_ERASE_OUTSIDE, abi.SCISSOR_FILL_INSIDE)


class Scratch:
    """device buffers that are freed when the test leaves"""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            self.dev.free(b)

    def new(self, nbytes, fill=0xFF):
        self.bufs.append(self.dev.malloc(max(int(nbytes), 4)))
        self.dev.to_device(self.bufs[-1], np.full(max(int(nbytes), 4), fill, np.uint8))
        return self.bufs[-1]

    def put(self, array):
        a = np.ascontiguousarray(array)
        self.bufs.append(self.dev.malloc(max(a.nbytes, 4)))
        self.dev.to_device(self.bufs[-1], a)
        return self.bufs[-1]


# ------------------------------------------------------------------------------------------------ the stencil
def star(cx, cy, r, points=5):
    """a star drawn in one stroke: its sides cross one another"""
    k = np.arange(points) * 2 % points if points % 2 else np.arange(points)
    a = 2.0 * math.pi * k / points + 0.3
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=-1)


def ring(cx, cy, n, r0=50.0, r1=10.0, lobes=7):
    a = 2.0 * math.pi * np.arange(n) / n
    r = r0 + r1 * np.sin(lobes * a)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=-1)


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def polygons(w, h):
    return {
        "triangle": [np.array([[0.3, 0.2], [0.9 * w + 0.1, 0.35 * h], [0.4 * w, 1.1 * h]])],
        "rectangle on pixel centres": [rect(0.5, 0.5, w - 0.5, h - 0.5)],
        "star": [star(0.5 * w, 0.5 * h, 0.6 * max(w, h))],
        "hole": [rect(0.2, 0.2, w - 0.2, h - 0.2), rect(0.25 * w + 0.1, 0.25 * h + 0.1, 0.75 * w, 0.75 * h)],
        "outside": [np.array([[w + 5.0, 1.0], [w + 40.0, 2.0], [w + 8.0, h + 9.0]])],
        "covering": [rect(-10.0, -10.0, w + 10.0, h + 10.0)],
    }


def check_stencil(dev, contours, w, h, what):
    """the words of the GPU against the reference's, into a buffer that held ones: the padding must come out 0"""
    want = sr.fill(contours, w, h)
    with Scratch(dev) as s:
        out = s.new(4 * host.region_mask_words((1, h, w)))
        got = dev.stencil_polygon(contours, w, h, out_ptr=out)
    assert got.dtype == np.uint32 and np.array_equal(got, sr.stencil_words(want)), (what, w, h)
    return want


@pytest.mark.parametrize("size", [(1, 1), (31, 1), (32, 3), (33, 5), (65, 4), (130, 7), (257, 129)])
def test_stencil_polygons(hip_dev, size):
    w, h = size
    filled = {name: check_stencil(hip_dev, contours, w, h, name) for name, contours in polygons(w, h).items()}
    assert filled["covering"].all() and not filled["outside"].any()
    if w >= 31:
        assert filled["triangle"].any() and not filled["triangle"].all()
    if w >= 32 and h >= 3:
        centres = filled["rectangle on pixel centres"]                          # the half-open rule: the sides at x = 0.5 and y = 0.5 belong
        assert centres[0, 0] and centres[:-1, :-1].all() and not centres[-1].any() and not centres[:, -1].any()      # to it, the other two do not
    if w >= 65:
        assert filled["hole"][0, 1] and not filled["hole"][h // 2, w // 2]


def test_stencil_limits(hip_dev):
    w, h = 130, 7
    big = 32768.0                                                                # 2^23 / 256
    tri = check_stencil(hip_dev, [np.array([[-big, -big], [big, -big], [big, big]])], w, h, "vertices at +-2^23")
    assert tri.any() and not tri.all() and tri[0, -1] and not tri[-1, 0]
    for n in (CHUNK, CHUNK + 1, abi.STENCIL_MAX_VERTICES):
        img = check_stencil(hip_dev, [ring(128.3, 64.6, n)], 257, 129, f"{n} edges")
        assert img.any() and not img.all()
    # two contours of CHUNK vertices: the second chunk holds a whole contour
    check_stencil(hip_dev, [ring(100.0, 60.0, CHUNK), ring(100.0, 60.0, CHUNK, 20.0, 5.0)], 257, 129, "two chunks")


def test_polygons_that_share_an_edge_tile_their_union(hip_dev):
    w, h = 65, 40
    a = np.array([[0.5, 0.5], [40.5, 0.5], [20.5, 36.5], [0.5, 36.5]])
    b = np.array([[40.5, 0.5], [60.5, 0.5], [60.5, 36.5], [20.5, 36.5]])
    u = np.array([[0.5, 0.5], [60.5, 0.5], [60.5, 36.5], [0.5, 36.5]])
    wa, wb, wu = (hip_dev.stencil_polygon([p], w, h) for p in (a, b, u))
    assert not (wa & wb).any() and np.array_equal(wa | wb, wu) and wa.any() and wb.any()
    # the set operations of the region calls work on stencils: nx = w, ny = h, nz = 1
    ia, ib = (sr.stencil_image(t, w, h)[0] for t in (wa, wb))
    both = hip_dev.region_combine(ia[None], ib[None], abi.MASK_OR)
    assert np.array_equal(both[0], sr.stencil_image(wu, w, h)[0])


def test_dilating_a_stencil_is_the_brush(hip_dev):
    w, h = 70, 33
    with Scratch(hip_dev) as s:
        st = s.new(4 * host.region_mask_words((1, h, w)))
        hip_dev.stencil_polygon([star(30.0, 15.0, 14.0)], w, h, out_ptr=st)
        line = sr.fill([star(30.0, 15.0, 14.0)], w, h)
        for element, radius in ((6, 1), (18, 2), (26, 3)):
            got = hip_dev.region_morph(st, abi.MORPH_DILATE, element, radius, shape=(1, h, w))
            assert np.array_equal(got, mr.dilate(line[None], element, radius)), (element, radius)
        stats = hip_dev.region_stats_of(np.zeros((1, h, w), np.uint16), st, shape=(1, h, w))
        assert stats.voxels == line.sum()


# ------------------------------------------------------------------------------------------------ the prism
SPACING = (0.7, 1.3, 2.1)


def unit(v):
    return host._normalize(np.asarray(v, dtype=np.float32))


def camera_at(pos, target, up, fov, W, H):
    cam = host.camera_setup(pos, target, up, fov, 0.0, 1.0, 1.0, W, H)
    cam.u, cam.v = host._to_vec3(unit(cam.u.tuple())), host._to_vec3(unit(cam.v.tuple()))     # the projection takes the frame to be orthonormal
    return cam


def views(lib, vol, ext):
    """(name, kwargs of the view) for two cameras -- outside the box, and inside it so that voxels lie behind the pinhole -- and three slices"""
    R = 0.5 * float(np.sqrt((ext * ext).sum()))
    d = unit((0.5, 0.35, 0.8)) * f32(2.2 * R + 1.0)
    outside = camera_at(tuple(d), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 40, 24)
    inside = camera_at(tuple(ext * np.array([0.1, 0.15, -0.1], np.float32)), tuple(ext * np.array([0.5, -0.4, -0.5], np.float32)), (0.0, 0.0, 1.0), 70.0, 33, 20)
    ob = oblique_slice(40, 24, float(ext.max()) / 20.0)
    ob.center = abi.vec3(*(ext * np.array([0.1, 0.05, -0.1], np.float32)))
    return [("camera outside", dict(camera=outside), 40, 24), ("camera inside", dict(camera=inside), 33, 20),
            ("axial", dict(slice=host.slice_params_axis(lib, vol, 2, 0.4, 40, 24), w=40, h=24), 40, 24),
            ("coronal", dict(slice=host.slice_params_axis(lib, vol, 1, 0.55, 33, 20), w=33, h=20), 33, 20),
            ("oblique", dict(slice=ob, w=40, h=24), 40, 24)]


def ref_view(kw):
    return {k: v for k, v in kw.items() if k in ("camera", "slice")}


def input_masks(shape):
    rng = np.random.default_rng(hash(shape) & 0xFFFF)
    return [("empty", np.zeros(shape, bool)), ("full", np.ones(shape, bool)), ("2 %", rng.random(shape) < 0.02), ("40 %", rng.random(shape) < 0.4)]


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 33), (3, 5, 31), (2, 3, 65), (4, 7, 130), (7, 1, 1)])
def test_prism_against_the_reference(hip_dev, shape):
    dev = hip_dev
    nz, ny, nx = shape
    vol = volume_of((nx, ny, nz), SPACING)
    ext = host.volume_size((nx, ny, nz), SPACING)
    words = host.region_mask_words(shape)
    ever_in, ever_out = False, False
    for name, kw, w, h in views(dev.lib, vol, ext):
        image = sr.fill([star(0.45 * w, 0.5 * h, 0.55 * h)], w, h)
        seen, _, _, depth = sr.view_of_voxels(shape, vol, w=w, h=h, **ref_view(kw))
        with Scratch(dev) as s:
            d_st, d_ones = s.put(sr.stencil_words(image)), s.put(sr.stencil_words(np.ones((h, w), bool)))
            d_in, d_out = s.new(4 * words), s.new(4 * words)

            def run(mask_ptr, stencil_ptr, op, depth_=(-np.inf, np.inf), out=None):
                dev.region_scissor(mask_ptr, stencil_ptr, vol, op=op, depth=depth_, shape=shape, out_ptr=d_out if out is None else out, **kw)
                return dev.to_host(d_out if out is None else out, (words,), np.uint32)

            def same(got, want, *what):
                assert np.array_equal(got, host.region_mask_pack(want)), (shape, name) + what

            # a stencil that is all ones gives the voxels the image sees; SELECT reads no input mask
            same(run(None, d_ones, abi.SCISSOR_SELECT), seen, "all ones")
            pr = sr.prism(shape, vol, image, **ref_view(kw))
            same(run(None, d_st, abi.SCISSOR_SELECT), pr, "select")
            ever_in, ever_out = ever_in or bool(pr.any()), ever_out or bool((seen & ~pr).any())
            for mname, m in input_masks(shape):
                clean = host.region_mask_pack(m)
                for dirty in (False, True):
                    dev.to_device(d_in, mr.dirty_padding(clean, shape) if dirty else clean)
                    for op in OPS:
                        same(run(d_in, d_st, op), sr.apply(op, m, pr), mname, dirty, op)
            # out aliasing in
            m = input_masks(shape)[3][1]
            for op in OPS:
                dev.to_device(d_in, mr.dirty_padding(host.region_mask_pack(m), shape))
                same(run(d_in, d_st, op, out=d_in), sr.apply(op, m, pr), "in place", op)
            # depth bounds whose closed ends are the float depths of two voxels the image sees
            if seen.any():
                ds = np.sort(depth[seen])
                lo, hi = float(ds[len(ds) // 3]), float(ds[(2 * len(ds)) // 3])
                for bounds in ((lo, hi), (lo, lo), (hi, np.inf), (-np.inf, lo)):
                    want = sr.prism(shape, vol, np.ones((h, w), bool), depth=bounds, **ref_view(kw))
                    assert want[seen & (depth == f32(bounds[0]))].all() and want[seen & (depth == f32(bounds[1]))].all()      # the ends are inside
                    same(run(None, d_ones, abi.SCISSOR_SELECT, bounds), want, "depth", bounds)
                    same(run(d_in, d_ones, abi.SCISSOR_ERASE_INSIDE, bounds), sr.apply(abi.SCISSOR_ERASE_INSIDE, sr.apply(OPS[-1], m, pr), want), "depth erase", bounds)
        if name == "camera inside" and nx * ny * nz > 30:
            assert (depth <= 0).any() and not seen[depth <= 0].any(), "voxels behind the pinhole"
    if nx * ny * nz > 30:
        assert ever_in and ever_out, "the stencil must cut the volume"
    assert dev.region_scissor_last_ms() >= 0.0


# ------------------------------------------------------------------------------------------------ with what exists
@pytest.fixture(scope="module")
def head(hip_dev):
    """the 48^3 head on a canvas, its ISO hit map at the bone level and the bone window's mask"""
    sc = scenes.make_scene("tiny_head")
    canvas = host.Canvas(hip_dev, sc.width, sc.height)
    scenes.apply_to_canvas(sc, canvas)
    hits = canvas.hit_map(abi.HIT_ISO, iso=0.5)
    bone = hip_dev.region_threshold(sc.vox, int(0.35 * 65535), 65535)
    return sc, canvas, hits, bone


def test_hits_project_to_their_own_pixel(hip_dev, head):
    sc, canvas, hits, _ = head
    found = hits["status"] == abi.HIT_STATUS_FOUND
    assert found.sum() > 500
    ys, xs = np.nonzero(found)
    for x, y, p in zip(xs, ys, hits["position"][found]):
        xy, depth = host.scissor_project_camera(canvas.camera, p, hip_dev.lib)
        assert xy == (x, y) and depth > 0, (x, y, xy)


def hit_ids_of(dev, canvas, mask, hits, shape):
    with Scratch(dev) as s:
        d_hits, d_ids = s.put(hits), s.new(4 * hits.size)
        with dev._staging() as st:
            dev.hit_ids(d_ids, d_hits, canvas.W, canvas.H, canvas.deviceVolume, shape, st.mask(mask, shape).value)
            return dev.to_host(d_ids, hits.shape, np.uint32)


def test_erase_inside_a_rectangle_removes_what_the_picture_shows_there(hip_dev, head):
    """ERASE_INSIDE of the bone window's mask with a rectangle that cuts through the head: svr_hit_ids of the result.

    The id image of the result is the reference's, pixel for pixel.  It is 0 at every pixel of the rectangle that lies MARGIN pixels or
    more inside it.  On the rectangle's outermost pixels it need not be: the prism is defined by the voxel CENTRES, and the centre of the
    voxel that holds a pixel's hit point may be seen at the neighbouring pixel, outside the rectangle (a voxel is wider than a pixel
    here).  The CPU references give 872 pixels of this rectangle with an id before, and 5 after, all in its outermost row or column:
    (37, 25), (38, 25), (56, 25), (57, 25), (60, 37).  MARGIN comes from the geometry, not from these: half a voxel's diagonal over the
    width of a pixel at the nearest voxel."""
    dev = hip_dev
    sc, canvas, hits, bone = head
    shape, cam, vol = sc.vox.shape, canvas.camera, canvas.deviceVolume
    X0, Y0, X1, Y1 = 30, 25, 60, 55
    words = dev.stencil_polygon([host.stencil_rect(X0, Y0, X1, Y1, dev.lib)], canvas.W, canvas.H)
    image = sr.stencil_image(words, canvas.W, canvas.H)[0]
    assert image.sum() == (X1 - X0 + 1) * (Y1 - Y0 + 1) and image[Y0:Y1 + 1, X0:X1 + 1].all()
    before = hit_ids_of(dev, canvas, bone, hits, shape)
    assert np.array_equal(before, ov.hit_ids(vol, bone, hits)) and (before[Y0:Y1 + 1, X0:X1 + 1] != 0).sum() > 500
    cut = dev.region_scissor(bone, words, vol, camera=cam, op=abi.SCISSOR_ERASE_INSIDE)
    pr = sr.prism(shape, vol, image, camera=cam)
    assert np.array_equal(cut, bone & ~pr) and (bone & pr).any()
    after = hit_ids_of(dev, canvas, cut, hits, shape)
    assert np.array_equal(after, ov.hit_ids(vol, cut, hits))
    assert np.array_equal(after[~image], before[~image] * (after[~image] != 0)) and (after[~image] != 0).sum() > 50     # only removed, and much is left
    _, _, _, depth = sr.view_of_voxels(shape, vol, camera=cam)
    pixel = 2.0 * float(depth.min()) * cam.tanFovxOverTwo * cam.aspectRatio / (canvas.W - 1)      # the width of a pixel at the nearest voxel
    margin = math.ceil(sc.step_size() / pixel)                                                    # (step_size: half a voxel's diagonal)
    assert 1 <= margin <= 3
    inner = after[Y0 + margin:Y1 + 1 - margin, X0 + margin:X1 + 1 - margin]
    assert inner.size > 400 and not inner.any()
    assert (after[Y0:Y1 + 1, X0:X1 + 1] != 0).sum() <= 2 * margin * (X1 - X0 + Y1 - Y0 + 2)


def test_erase_then_fill_restores(hip_dev, head):
    dev = hip_dev
    sc, canvas, _, bone = head
    shape, cam, vol = sc.vox.shape, canvas.camera, canvas.deviceVolume
    words = dev.stencil_polygon([star(48.0, 40.0, 30.0)], canvas.W, canvas.H)
    n = host.region_mask_words(shape)
    with Scratch(dev) as s:
        d = s.put(host.region_mask_pack(bone))
        erased = dev.region_scissor(d, words, vol, camera=cam, op=abi.SCISSOR_ERASE_INSIDE, shape=shape, out_ptr=d)
        assert erased.sum() < bone.sum()
        filled = dev.region_scissor(d, words, vol, camera=cam, op=abi.SCISSOR_FILL_INSIDE, shape=shape, out_ptr=d)
        assert (filled & ~bone).any(), "the prism holds voxels outside the bone window"
        back = dev.region_combine(d, bone, abi.MASK_AND, shape=shape)
        assert np.array_equal(back, bone)
        assert dev.to_host(d, (n,), np.uint32).dtype == np.uint32
    # the same through a slice: a slab of thickness 4 around the axial plane z = 0 holds the four planes of voxels with centres at +-0.5, +-1.5
    sl = canvas.slice_params_axis(2, 0.5)
    t = 4.0 * sc.spacing[2]
    painted = dev.region_scissor(bone, words, vol, slice=sl, w=canvas.W, h=canvas.H, op=abi.SCISSOR_FILL_INSIDE, depth=(-0.5 * t, 0.5 * t))
    pr = sr.prism(shape, vol, sr.stencil_image(words, canvas.W, canvas.H)[0], slice=sl, depth=(-0.5 * t, 0.5 * t))
    assert np.array_equal(painted, bone | pr) and list(np.nonzero(pr.any(axis=(1, 2)))[0]) == [22, 23, 24, 25]
