"""Test-side reference of the scissor calls (include/svr_abi.h, "scissors"), numpy only and literal.  The fill works in
int64 integers; the projection in np.float32 operations in exactly the order the header names, nothing in float64 (the dtypes are
asserted); the prism is evaluated per voxel, each from its own centre."""
import numpy as np

f32 = np.float32
SELECT, ERASE_INSIDE, ERASE_OUTSIDE, FILL_INSIDE = 0, 1, 2, 3


def _f(*arrays):
    for a in arrays:
        assert a.dtype == np.float32, a.dtype
    return arrays[0] if len(arrays) == 1 else arrays


def _v3(v):
    return np.array([v.x, v.y, v.z], dtype=np.float32)


# ---------------------------------------------------------------------------------------------- the fill
def q8(contour):
    """(n, 2) pixel coordinates as int64 in 1/256 pixel: round(256 v)"""
    return np.rint(np.asarray(contour, dtype=np.float64) * 256.0).astype(np.int64)


def fill(contours, w, h):
    """bool [h][w]: the even-odd fill of the contours ((n, 2) arrays in pixels) under the half-open crossing rule"""
    out = np.zeros((h, w), dtype=bool)
    cx = (256 * np.arange(w, dtype=np.int64) + 128)[None, :]
    cy = 256 * np.arange(h, dtype=np.int64) + 128
    for c in contours:
        q = q8(c)
        for i in range(len(q)):
            (ax, ay), (bx, by) = (int(t) for t in q[i]), (int(t) for t in q[(i + 1) % len(q)])
            rows = np.nonzero((ay > cy) != (by > cy))[0]
            if len(rows) == 0:
                continue
            cross = np.int64(bx - ax) * (cy[rows] - ay)[:, None] - np.int64(by - ay) * (cx - ax)
            assert cross.dtype == np.int64
            out[rows] ^= (cross > 0) if by > ay else (cross < 0)
    return out


def stencil_words(image):
    """the stencil words of a bool image [h][w]: the bit mask of a w x h x 1 volume"""
    h, w = image.shape
    wx = (w + 31) // 32
    padded = np.zeros((h, wx * 32), dtype=np.uint8)
    padded[:, :w] = image
    return np.packbits(padded, axis=-1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def stencil_image(words, w, h):
    wx = (w + 31) // 32
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8).reshape(h, wx * 4), axis=-1, bitorder="little")
    return bits[:, :w].astype(bool), bits[:, w:].astype(bool)        # the image, the padding


# ---------------------------------------------------------------------------------------------- the projection
def _dot(d, q):
    return _f((d[..., 0] * q[0] + d[..., 1] * q[1]) + d[..., 2] * q[2])


def _pixel(s, r, W, H):
    _f(s, r)
    seen = (s >= f32(0)) & (s < f32(W)) & (r >= f32(0)) & (r < f32(H))
    x = np.where(seen, np.floor(np.where(seen, s, f32(0))), -1).astype(np.int64)
    y = np.where(seen, np.floor(np.where(seen, r, f32(0))), -1).astype(np.int64)
    return seen, x, y


def project_camera(cam, P):
    """(seen, x, y, depth) of world points P[..., 3] (float32) through a cudaCamera"""
    P = _f(np.asarray(P))
    pos, u, v, w = _v3(cam.pos), _v3(cam.u), _v3(cam.v), _v3(cam.w)
    tan, aspect = f32(cam.tanFovxOverTwo), f32(cam.aspectRatio)
    wm1, hm1 = f32(cam.imageW) - f32(1), f32(cam.imageH) - f32(1)
    with np.errstate(all="ignore"):
        d = _f(P - pos)
        a, b, c = _dot(d, u), _dot(d, v), _f(-_dot(d, w))
        front = c > f32(0)
        s = _f(((a / (c * (aspect * tan)) + f32(1)) * f32(0.5)) * wm1)
        r = _f(((b / (c * tan) + f32(1)) * f32(0.5)) * hm1)
        seen, x, y = _pixel(s, r, cam.imageW, cam.imageH)
    seen = seen & front
    return seen, np.where(seen, x, -1), np.where(seen, y, -1), c


def slice_normal(p):
    u, v = _v3(p.u), _v3(p.v)
    cr = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], dtype=np.float32)
    inv = f32(1) / np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2], dtype=np.float32)
    return _f(cr * inv)


def project_slice(p, W, H, P):
    """(seen, x, y, depth) of world points P[..., 3] (float32) through slice 0 of a SliceParams on a W x H image"""
    P = _f(np.asarray(P))
    center, u, v, n = _v3(p.center), _v3(p.u), _v3(p.v), slice_normal(p)
    uu, vv = _dot(u, u), _dot(v, v)
    with np.errstate(all="ignore"):
        d = _f(P - center)
        a, b = _f(_dot(d, u) / uu), _f(_dot(d, v) / vv)
        s, r = _f(a + f32(0.5) * f32(W)), _f(b + f32(0.5) * f32(H))
        seen, x, y = _pixel(s, r, W, H)
        depth = _dot(d, n)
    return seen, x, y, depth


def camera_ray_point(cam, x, y, t):
    """the point at parameter t on the pinhole centre ray of pixel (x, y): float32, the operations of the projection section"""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    wm1, hm1 = f32(cam.imageW) - f32(1), f32(cam.imageH) - f32(1)
    tan, aspect = f32(cam.tanFovxOverTwo), f32(cam.aspectRatio)
    nx = (f32(2) * ((x + f32(0.5)) / wm1) - f32(1)) * aspect * tan
    ny = (f32(2) * ((y + f32(0.5)) / hm1) - f32(1)) * tan
    u, v, w, pos = _v3(cam.u), _v3(cam.v), _v3(cam.w), _v3(cam.pos)
    d = (u * nx[..., None] + v * ny[..., None]) - w
    inv = f32(1) / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], dtype=np.float32)
    d = d * inv[..., None]
    return _f(pos + d * f32(t))


def slice_plane_point(p, W, H, x, y, off=0.0):
    """PLANE POINT of pixel (x, y) of slice 0, moved by `off` along the normal"""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    a = (x + f32(0.5)) - f32(0.5) * f32(W)
    b = (y + f32(0.5)) - f32(0.5) * f32(H)
    c = (_v3(p.center) + _v3(p.u) * a[..., None]) + _v3(p.v) * b[..., None]
    return _f(c + slice_normal(p) * f32(off))


# ---------------------------------------------------------------------------------------------- the prism
def voxel_centres(shape, volume):
    """float32 [nz][ny][nx][3]: VOXEL CENTRE of the header, on the unclipped box"""
    nz, ny, nx = shape
    vmin, vmax = _v3(volume.bbox.vmin), _v3(volume.bbox.vmax)
    axes = []
    for a, n in enumerate((nx, ny, nz)):
        tc = _f((np.arange(n, dtype=np.float32) + f32(0.5)) / f32(n))
        axes.append(_f(vmin[a] + (vmax[a] - vmin[a]) * tc))
    P = np.empty((nz, ny, nx, 3), dtype=np.float32)
    P[..., 0] = axes[0][None, None, :]
    P[..., 1] = axes[1][None, :, None]
    P[..., 2] = axes[2][:, None, None]
    return P


def view_of_voxels(shape, volume, camera=None, slice=None, w=None, h=None):
    """(seen, x, y, depth) of every voxel centre"""
    P = voxel_centres(shape, volume)
    return project_camera(camera, P) if camera is not None else project_slice(slice, w, h, P)


def prism(shape, volume, stencil, camera=None, slice=None, depth=(-np.inf, np.inf)):
    """bool [nz][ny][nx]: the voxels whose centre is seen at a set pixel of the bool image `stencil` at a depth in the closed interval"""
    h, w = stencil.shape
    seen, x, y, dep = view_of_voxels(shape, volume, camera, slice, w, h)
    _f(dep)
    lo, hi = f32(depth[0]), f32(depth[1])
    with np.errstate(invalid="ignore"):
        ok = seen & (lo <= dep) & (dep <= hi)
    return ok & stencil[np.where(ok, y, 0), np.where(ok, x, 0)]


def apply(op, mask, pr):
    if op == SELECT:
        return pr.copy()
    return {ERASE_INSIDE: mask & ~pr, ERASE_OUTSIDE: mask & pr, FILL_INSIDE: mask | pr}[op]
