"""Test-side reference of svr_render_hits / svr_pick: a plain Python loop per pixel that implements the numeric contract in
include/svr_abi.h ("hit maps and picks") literally, on top of tests/projection_ref.py's Reference -- its rays and samples, its
isosurface search, the oracle's sampler, gradient and transfer-function look-up.  float32 throughout (numpy scalars; numpy never
contracts).  It skips nothing: every sample is looked at.

The maps are kept per (mode, step, alpha, iso) on the HitReference, and the HitReference per projection Reference."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import projection_ref as pr

f32 = np.float32
OPACITY, ISO, MAX = 1, 2, 3
MISS, NONE, FOUND = 0, 1, 2
ZERO, ONE = f32(0), f32(1)

# svr_hit: 4-byte members only, 40 bytes
HIT_DTYPE = np.dtype([("status", np.int32), ("sample", np.int32), ("t", np.float32), ("value", np.float32),
                      ("position", np.float32, 3), ("normal", np.float32, 3)])
assert HIT_DTYPE.itemsize == 40


class HitReference:
    def __init__(self, R: pr.Reference):
        self.R = R
        self._maps = {}
        self._alphas = {}

    def tf_alpha(self, x) -> f32:
        """The alpha channel of the ray caster's transfer-function look-up."""
        R = self.R
        R.lib.svo_tex1d(R.ptr, C.c_float(float(x)), R._c)
        return f32(R._c[3])

    def alphas(self, key, ray):
        """a_n of every sample of a ray (they do not depend on the level: computed once per ray and step)."""
        if key not in self._alphas:
            self._alphas[key] = [self.tf_alpha(I) for I in ray.Is]
        return self._alphas[key]

    def normal(self, p):
        g = self.R.gradient(p)
        gm = np.sqrt(pr._dot(g, g))
        if float(gm) > 1e-3:
            return pr._normalize(g)
        return (ZERO, ZERO, ZERO)

    def hit(self, ray, key, mode, alpha, iso):
        """(status, sample, t, value, samples looked at, bisected) of one ray that intersects the box."""
        N = len(ray.Is)
        if mode == OPACITY:
            level, A = f32(alpha), ZERO
            for n, a in enumerate(self.alphas(key, ray)):
                A = A + (ONE - A) * a
                if A > level:
                    return FOUND, n, ray.ts[n], ray.Is[n], n + 1, False
            return NONE, N, ZERO, ZERO, N, False
        if mode == ISO:
            r = self.R.iso_search(ray, iso)
            if r is None:
                return NONE, N, ZERO, ZERO, N, False
            ns, _, hi, I_hi = r
            return FOUND, ns, hi, I_hi, ns + 1, ns > 0
        assert mode == MAX
        M, at = ZERO, None
        for n, I in enumerate(ray.Is):
            if I > M:
                M, at = I, n
        if at is None:
            return NONE, N, ZERO, ZERO, N, False
        return FOUND, at, ray.ts[at], M, N, False

    def hit_map(self, mode, step, alpha=0.5, iso=0.5):
        """((H, W) HIT_DTYPE records, {"raycast_steps", "vol_taps"}).  Pixels outside the Reference's window read as MISS."""
        k = (mode, float(f32(step)), float(f32(alpha)), float(f32(iso)))
        if k in self._maps:
            return self._maps[k]
        R = self.R
        rays = R.rays(step)
        out = np.zeros((R.H, R.W), dtype=HIT_DTYPE)
        steps = taps = 0
        with np.errstate(all="ignore"):
            for y in range(R.H):
                for x in range(R.W):
                    ray = rays[y][x]
                    if ray is None:
                        continue
                    status, sample, t, value, looked, bisected = self.hit(ray, (k[1], y, x), mode, alpha, iso)
                    rec = out[y, x]
                    rec["status"], rec["sample"] = status, sample
                    steps += looked
                    taps += looked + (8 if bisected else 0)
                    if status == FOUND:
                        p = R.point(ray, f32(t))
                        rec["t"], rec["value"] = t, value
                        rec["position"] = p
                        rec["normal"] = self.normal(p)
                        taps += 6
        res = (out, {"raycast_steps": steps, "vol_taps": taps})
        self._maps[k] = res
        return res


_CACHE: dict = {}


def reference(key, scene_factory, window=None) -> HitReference:
    """The cached HitReference of a named test scene, on the projection reference of the same name (shared with its tests)."""
    if key not in _CACHE:
        _CACHE[key] = HitReference(pr.reference(key, scene_factory, window))
    return _CACHE[key]
