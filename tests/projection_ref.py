"""Test-side reference of svr_render_projection: a plain Python loop per pixel that implements the numeric contract in
include/svr_abi.h ("projection modes of the ray caster") literally on top of the CPU oracle's primitives -- the pinhole ray,
the box interval, the sampler, the gradient, the transfer-function look-up and powf.  float32 throughout (numpy's float32 add,
multiply, divide and sqrt are correctly rounded, and numpy never contracts).  It skips nothing: every sample is fetched.

The samples of a ray do not depend on the mode, so they are computed once per (scene, step) and kept in a module-level cache;
so are the images.  About 10^6 ctypes calls per tiny scene."""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import binding

f32 = np.float32
MIP, MEAN, ISO = 1, 2, 3
ZERO, ONE, HALF = f32(0), f32(1), f32(0.5)


def to_u8(v) -> int:
    """k_raycast's conversion: truncation, clamped to [0, 255], NaN -> 0."""
    if not (v > 0):
        return 0
    if v >= 255:
        return 255
    return int(v)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize(a):
    s = ONE / np.sqrt(_dot(a, a))
    return (a[0] * s, a[1] * s, a[2] * s)


class Ray:
    __slots__ = ("orig", "dir", "ts", "Is")


class Reference:
    def __init__(self, scene, window=None):
        """window = (x0, y0, x1, y1): only these pixels are computed (the rest of the image stays 0); None = the whole frame."""
        self.scene = scene
        self.window = window if window is not None else (0, 0, scene.width, scene.height)
        self.o = binding.OracleScene(scene)
        self.lib = self.o.lib
        self.ptr = self.o.ptr
        self.W, self.H = scene.width, scene.height
        cam = scene.resolved_camera()
        self.cam = (f32(cam.pos.x), f32(cam.pos.y), f32(cam.pos.z))
        self._p = (C.c_float * 3)()
        self._g = (C.c_float * 3)()
        self._c = (C.c_float * 4)()
        self._rays = {}
        self._images = {}

    # ---- primitives ----
    def intensity(self, p) -> f32:
        q = self._p
        q[0], q[1], q[2] = p
        return f32(self.lib.svo_volume_intensity(self.ptr, q))

    def gradient(self, p):
        q, g = self._p, self._g
        q[0], q[1], q[2] = p
        self.lib.svo_volume_gradient(self.ptr, q, g)
        return (f32(g[0]), f32(g[1]), f32(g[2]))

    def tf_rgb(self, x):
        self.lib.svo_tex1d(self.ptr, C.c_float(float(x)), self._c)
        return (f32(self._c[0]), f32(self._c[1]), f32(self._c[2]))

    @staticmethod
    def point(ray, t):
        o, d = ray.orig, ray.dir
        return (o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t)

    # ---- the ray and its samples: t_0 = tNear, t_{n+1} = fl(t_n + h), while t_n <= tFar ----
    def rays(self, step):
        key = float(f32(step))
        if key in self._rays:
            return self._rays[key]
        lib, ptr = self.lib, self.ptr
        orig, dirv = (C.c_float * 3)(), (C.c_float * 3)()
        tn, tf = C.c_float(), C.c_float()
        h = f32(step) * HALF
        q = self._p
        fetch = lib.svo_volume_intensity
        out = []
        x0, y0, x1, y1 = self.window
        for y in range(self.H):
            row = []
            for x in range(self.W):
                if not (x0 <= x < x1 and y0 <= y < y1):
                    row.append(None)
                    continue
                lib.svo_camera_ray_pinhole(ptr, x, y, orig, dirv)
                if not lib.svo_volume_intersect(ptr, orig, dirv, C.byref(tn), C.byref(tf)):
                    row.append(None)
                    continue
                r = Ray()
                r.orig = (f32(orig[0]), f32(orig[1]), f32(orig[2]))
                r.dir = (f32(dirv[0]), f32(dirv[1]), f32(dirv[2]))
                t, tFar = f32(tn.value), f32(tf.value)
                ts = []
                while t <= tFar:
                    ts.append(t)
                    t = t + h
                r.ts = np.array(ts, dtype=np.float32)
                # p(t) = orig + dir * t, one multiply and one add per component (elementwise float32, as the scalars would be)
                P = np.stack([r.orig[a] + r.dir[a] * r.ts for a in range(3)], axis=1)
                assert P.dtype == np.float32
                Is = []
                for a, b, c in P.tolist():
                    q[0], q[1], q[2] = a, b, c
                    Is.append(fetch(ptr, q))
                r.Is = np.array(Is, dtype=np.float32)
                row.append(r)
            out.append(row)
        self._rays[key] = out
        return out

    # ---- the three modes, per pixel ----
    def mip(self, ray) -> f32:
        M = ZERO
        for I in ray.Is:
            if I > M:
                M = I
        return M

    def mean(self, ray) -> f32:
        S = ZERO
        for I in ray.Is:
            S = S + I
        return S / f32(len(ray.Is))

    def iso_search(self, ray, iso):
        """(n*, lo, hi, I(hi)) or None; lo is None when n* = 0 (no bisection)."""
        iso = f32(iso)
        ns = None
        for n, I in enumerate(ray.Is):
            if I >= iso:
                ns = n
                break
        if ns is None:
            return None
        hi, I_hi = ray.ts[ns], ray.Is[ns]
        if ns == 0:
            return ns, None, hi, I_hi
        lo = ray.ts[ns - 1]
        for _ in range(8):
            mid = HALF * (lo + hi)
            Im = self.intensity(self.point(ray, mid))
            if Im >= iso:
                hi, I_hi = mid, Im
            else:
                lo = mid
        return ns, lo, hi, I_hi

    def shade(self, ray, hi, base):
        """The ray caster's head-light term with opacity 1 at p(hi)."""
        p = self.point(ray, hi)
        g = self.gradient(p)
        gm = np.sqrt(_dot(g, g))
        cosTerm, spec = ONE, ZERO
        if float(gm) > 1e-3:
            normal = _normalize(g)
            lightDir = _normalize((self.cam[0] - p[0], self.cam[1] - p[1], self.cam[2] - p[2]))
            cosTerm = np.abs(_dot(normal, lightDir))
            spec = f32(self.lib.svo_powf(C.c_float(float(cosTerm)), C.c_float(30.0)))
        a = ONE
        out = []
        for c in base:
            v = c * a * cosTerm * f32(0.8) + a * spec * f32(0.2)
            out.append(v if v < ONE else ONE)      # fminf(v, 1)
        return out

    def image(self, mode, step, iso=0.5, window=(0.0, 1.0), color_tf=False):
        """(RGBA8 image, {"raycast_steps", "vol_taps"}, info) of the whole frame.  info: per-pixel n* (-2 miss, -1 no crossing) for
        ISO, the projected value M for MIP / MEAN."""
        key = (mode, float(f32(step)), float(f32(iso)), float(f32(window[0])), float(f32(window[1])), bool(color_tf))
        if key in self._images:
            return self._images[key]
        rays = self.rays(step)
        img = np.zeros((self.H, self.W, 4), dtype=np.uint8)
        info = np.full((self.H, self.W), -2 if mode == ISO else np.nan, dtype=np.int64 if mode == ISO else np.float32)
        steps = taps = 0
        lo, hi = f32(window[0]), f32(window[1])
        k255 = f32(255)
        with np.errstate(all="ignore"):
            for y in range(self.H):
                for x in range(self.W):
                    ray = rays[y][x]
                    if ray is None:
                        continue                                  # miss: (0, 0, 0, 0)
                    if mode == ISO:
                        r = self.iso_search(ray, iso)
                        if r is None:
                            steps += len(ray.Is); taps += len(ray.Is)
                            info[y, x] = -1
                            continue
                        ns, blo, bhi, I_hi = r
                        info[y, x] = ns
                        steps += ns + 1
                        taps += ns + 1 + (8 if ns > 0 else 0) + 6
                        base = self.tf_rgb(I_hi) if color_tf else (ONE, ONE, ONE)
                        rgb = self.shade(ray, bhi, base)
                    else:
                        M = self.mip(ray) if mode == MIP else self.mean(ray)
                        info[y, x] = M
                        steps += len(ray.Is); taps += len(ray.Is)
                        if color_tf:
                            rgb = [min(max(c, ZERO), ONE) for c in self.tf_rgb(M)]
                        else:
                            g = (M - lo) / (hi - lo)
                            g = min(max(g, ZERO), ONE)
                            rgb = [g, g, g]
                    img[y, x] = (to_u8(rgb[0] * k255), to_u8(rgb[1] * k255), to_u8(rgb[2] * k255), 255)
        res = (img, {"raycast_steps": steps, "vol_taps": taps}, info)
        self._images[key] = res
        return res


_CACHE: dict = {}


def reference(key, scene_factory, window=None) -> Reference:
    """The cached Reference of a named test scene (scene_factory() builds the Scene on first use)."""
    if key not in _CACHE:
        _CACHE[key] = Reference(scene_factory(), window)
    return _CACHE[key]
