"""Test-side reference of svr_render_slice / svr_render_slice_stack: the numeric contract in include/svr_abi.h ("slice views")
implemented literally on top of the CPU oracle's primitives -- the sampler (svo_volume_intensity) and the transfer-function
look-up (svo_tex1d).  float32 throughout: every geometric operation is one numpy float32 array operation (add, subtract,
multiply, divide and sqrt are correctly rounded, and numpy never contracts), in the order the header names.  It skips nothing:
every counting sample is fetched.

The samples of a slice do not depend on the slab mode or the colour, so they are computed once per geometry and kept."""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import binding

f32 = np.float32
MIP, MINIP, MEAN = 1, 2, 3
MAX_SAMPLES = 4096
ZERO, ONE, HALF = f32(0), f32(1), f32(0.5)


def vec(v):
    """a svr_vec3 / 3-sequence as three float32 scalars"""
    if hasattr(v, "x"):
        return (f32(v.x), f32(v.y), f32(v.z))
    return (f32(v[0]), f32(v[1]), f32(v[2]))


def normal(u, v):
    """n = normalize(cross(u, v)) as the header defines it; None if the cross product has no length."""
    u, v = vec(u), vec(v)
    with np.errstate(all="ignore"):
        cr = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        len2 = (cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]
        if not (len2 > 0):
            return None
        inv = ONE / np.sqrt(len2)
        n = (cr[0] * inv, cr[1] * inv, cr[2] * inv)
    if not all(np.isfinite(c) for c in n):
        return None
    return n


def box(vol):
    """(lo, hi) of the box volume.Intersect clips to: per axis min / max of bbox.vmin * (-clip.x) and bbox.vmax * clip.y."""
    lo, hi = [], []
    for a, clip in zip("xyz", (vol.x_clip, vol.y_clip, vol.z_clip)):
        e0 = f32(getattr(vol.bbox.vmin, a)) * (-f32(clip.x))
        e1 = f32(getattr(vol.bbox.vmax, a)) * f32(clip.y)
        lo.append(min(e0, e1)); hi.append(max(e0, e1))
    return lo, hi


def sample_count(thickness, step):
    """K of the header; the caller has checked the arguments."""
    if f32(thickness) == 0:
        return 1
    return int(np.floor(f32(thickness) / f32(step))) + 1


def to_u8(v):
    """k_raycast's conversion on an array: truncation, clamped to [0, 255], NaN -> 0."""
    v = np.asarray(v, dtype=np.float32)
    out = np.zeros(v.shape, dtype=np.uint8)
    pos = v > 0
    out[pos] = np.minimum(v[pos], f32(255)).astype(np.int64).astype(np.uint8)
    return out


class Samples:
    """inside[K, wh, ww] (bool) and I[K, wh, ww] (float32, 0 where not inside) of the window's pixels of one slice."""
    __slots__ = ("inside", "I")


class Reference:
    def __init__(self, scene):
        self.scene = scene
        self.o = binding.OracleScene(scene)
        self.lib, self.ptr = self.o.lib, self.o.ptr
        self.vol = self.o.s.vol
        self._p = (C.c_float * 3)()
        self._c = (C.c_float * 4)()
        self._samples = {}

    def intensity(self, p) -> f32:
        q = self._p
        q[0], q[1], q[2] = p
        return f32(self.lib.svo_volume_intensity(self.ptr, q))

    def tf_rgb(self, x):
        self.lib.svo_tex1d(self.ptr, C.c_float(float(x)), self._c)
        return (f32(self._c[0]), f32(self._c[1]), f32(self._c[2]))

    # ---- geometry and samples ----
    def points(self, p, w, h, k=0, spacing=0.0, window=None):
        """(P[K, wh, ww, 3] float32, inside[K, wh, ww]) of the pixels of `window` (default: all) of slice k: the header's FRAME,
        SLICE, PLANE POINT, SLAB SAMPLES and BOX."""
        x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
        n = normal(p.u, p.v)
        assert n is not None
        center, u, v = vec(p.center), vec(p.u), vec(p.v)
        with np.errstate(all="ignore"):
            if k != 0:
                off = f32(spacing) * f32(k)
                center = tuple(center[a] + n[a] * off for a in range(3))
            a = (np.arange(x0, x1, dtype=np.float32) + HALF) - HALF * f32(w)
            b = (np.arange(y0, y1, dtype=np.float32) + HALF) - HALF * f32(h)
            K = sample_count(p.thickness, p.step)
            if f32(p.thickness) == 0:
                d = np.zeros(1, dtype=np.float32)
            else:
                d = (np.arange(K, dtype=np.float32) * f32(p.step)) - (HALF * f32(p.thickness))
            assert a.dtype == b.dtype == d.dtype == np.float32
            lo, hi = box(self.vol)
            P = np.empty((K, y1 - y0, x1 - x0, 3), dtype=np.float32)
            inside = np.ones((K, y1 - y0, x1 - x0), dtype=bool)
            for ax in range(3):
                c = (center[ax] + u[ax] * a)[None, :] + (v[ax] * b)[:, None]             # (center + u * a) + v * b
                pj = c[None, :, :] + (n[ax] * d)[:, None, None]                            # c + n * d_j
                assert c.dtype == np.float32 and pj.dtype == np.float32
                P[..., ax] = pj
                inside &= (pj >= lo[ax]) & (pj <= hi[ax])
        return P, inside

    def samples(self, p, w, h, k=0, spacing=0.0, window=None) -> Samples:
        key = (bytes(p)[:44], w, h, k, float(f32(spacing)), window)           # center, u, v, thickness, step: the geometry
        if key in self._samples:
            return self._samples[key]
        P, inside = self.points(p, w, h, k, spacing, window)
        I = np.zeros(inside.shape, dtype=np.float32)
        q, fetch, ptr = self._p, self.lib.svo_volume_intensity, self.ptr
        vals = []
        for x, y, z in P[inside].tolist():
            q[0], q[1], q[2] = x, y, z
            vals.append(fetch(ptr, q))
        I[inside] = np.array(vals, dtype=np.float32)
        s = Samples()
        s.inside, s.I = inside, I
        self._samples[key] = s
        return s

    # ---- the pixel value and its colour ----
    @staticmethod
    def value(s: Samples, thickness, mode):
        """(M[h, w] float32 -- NaN where nothing counts --, N[h, w])"""
        inside, I = s.inside, s.I
        N = inside.sum(axis=0)
        hit = N > 0
        with np.errstate(all="ignore"):
            if f32(thickness) == 0:
                M = I[0].copy()
            elif mode == MIP:
                M = np.where(inside, I, ZERO).max(axis=0)
                M = np.maximum(M, ZERO)
            elif mode == MINIP:
                M = np.where(inside, I, f32(np.inf)).min(axis=0)
            elif mode == MEAN:
                S = np.zeros(N.shape, dtype=np.float32)
                for j in range(inside.shape[0]):                     # in sample order
                    S = np.where(inside[j], S + I[j], S)
                assert S.dtype == np.float32
                M = S / np.maximum(N, 1).astype(np.float32)
            else:
                raise ValueError(mode)
        M = M.astype(np.float32)
        M[~hit] = np.nan
        return M, N

    def colour(self, M, N, window=(0.0, 1.0), color_tf=False):
        h, w = M.shape
        img = np.zeros((h, w, 4), dtype=np.uint8)
        hit = N > 0
        k255 = f32(255)
        with np.errstate(all="ignore"):
            if color_tf:
                rgb = np.zeros((h, w, 3), dtype=np.float32)
                for y, x in np.argwhere(hit):
                    rgb[y, x] = self.tf_rgb(M[y, x])
                rgb = np.minimum(np.maximum(rgb, ZERO), ONE)
            else:
                lo, hi = f32(window[0]), f32(window[1])
                g = (M - lo) / (hi - lo)
                g = np.minimum(np.maximum(g, ZERO), ONE)
                rgb = np.stack([g, g, g], axis=-1)
            assert rgb.dtype == np.float32
            u8 = to_u8(rgb * k255)
        img[..., :3] = u8
        img[..., 3] = 255
        img[~hit] = 0
        return img

    def image(self, p, w, h, k=0, spacing=0.0, window=None):
        """(RGBA8 image, {"raycast_steps", "vol_taps"}, M) of slice k of a stack (k = 0: svr_render_slice).  window = (x0, y0, x1, y1):
        only these pixels are computed (the rest of the image stays 0, of M NaN)."""
        s = self.samples(p, w, h, k, spacing, window)
        Mw, N = self.value(s, p.thickness, p.mode)
        x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
        img = np.zeros((h, w, 4), dtype=np.uint8)
        M = np.full((h, w), np.nan, dtype=np.float32)
        img[y0:y1, x0:x1] = self.colour(Mw, N, (p.window_lo, p.window_hi), bool(p.flags & 1))
        M[y0:y1, x0:x1] = Mw
        n = int(N.sum())
        return img, {"raycast_steps": n, "vol_taps": n}, M


_CACHE: dict = {}


def reference(key, scene_factory) -> Reference:
    """The cached Reference of a named test scene (scene_factory() builds the Scene on first use)."""
    if key not in _CACHE:
        _CACHE[key] = Reference(scene_factory())
    return _CACHE[key]
