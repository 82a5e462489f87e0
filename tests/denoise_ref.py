"""Restatements of the denoised preview (include/svr_abi.h, svr_denoise_params) for the tests.

atrous_ref: the edge-avoiding a-trous filter in numpy (float64), written from the formulas of the header.
guides_ref: the guide march of one pixel restated from the oracle's exported primitives (float32, same operation order as the kernel).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

B3 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
f32 = np.float32


def lum(c):
    return (np.float32(0.2126) * c[..., 0] + np.float32(0.7152) * c[..., 1]) + np.float32(0.0722) * c[..., 2]


def pixel_scale(tan_fovx_over_two: float, height: int) -> float:
    """Pixel footprint per unit of depth: 2 tan(fovx / 2) / (H - 1), in float32 like the library."""
    return float(f32(f32(2.0) * f32(tan_fovx_over_two)) / f32(max(height - 1, 1)))


def atrous_ref(hdr, guides, passes=5, sigma_depth=1.0, sigma_normal=32.0, sigma_albedo=0.2, sigma_opacity=0.2, sigma_color=0.0,
               pix_scale=1.0):
    """hdr (H, W, 3), guides (H, W, 8) = N.xyz, D, A.rgb, O.  Returns the remodulated HDR result (H, W, 3), float64."""
    hdr = np.asarray(hdr, dtype=np.float64)
    g = np.asarray(guides, dtype=np.float64)
    H, W, _ = hdr.shape
    N, D, A, O = g[..., 0:3], g[..., 3], g[..., 4:7], g[..., 7]
    Am = np.maximum(A, 1e-3)
    valid = O != 0
    c = hdr / Am
    for k in range(passes):
        step = 1 << k
        lp = lum(c)
        with np.errstate(divide="ignore", invalid="ignore"):
            kd = 1.0 / (sigma_depth * step * (D * pix_scale)) if sigma_depth > 0 else np.zeros_like(D)
        ka = 1.0 / (sigma_albedo * sigma_albedo) if sigma_albedo > 0 else 0.0
        ko = 1.0 / sigma_opacity if sigma_opacity > 0 else 0.0
        kc = 1.0 / (sigma_color * sigma_color * 2.0 ** -k) if sigma_color > 0 else 0.0
        sw = np.zeros((H, W))
        acc = np.zeros((H, W, 3))
        ys, xs = np.mgrid[0:H, 0:W]
        for j in range(-2, 3):
            for i in range(-2, 3):
                hk = B3[j + 2] * B3[i + 2]
                qy, qx = ys + j * step, xs + i * step
                inb = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                cq = c[qyc, qxc]
                if i == 0 and j == 0:
                    w = np.full((H, W), hk)
                else:
                    ex = np.abs(D - D[qyc, qxc]) * kd + np.sum((A - A[qyc, qxc]) ** 2, axis=-1) * ka + np.abs(O - O[qyc, qxc]) * ko
                    if kc:
                        ex = ex + (lp - lum(cq)) ** 2 * kc
                    with np.errstate(over="ignore", invalid="ignore"):
                        w = hk * np.exp(-ex)
                        if sigma_normal > 0:
                            nd = np.sum(N * N[qyc, qxc], axis=-1)
                            w = np.where(nd > 0, w * np.power(np.maximum(nd, 0.0), sigma_normal), 0.0)
                    ok = inb & (O[qyc, qxc] != 0) & np.all(np.isfinite(cq), axis=-1) & (w > 0)
                    w = np.where(ok, w, 0.0)
                sw += w
                acc += w[..., None] * np.where(w[..., None] > 0, cq, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(valid[..., None], acc / sw[..., None], c)
    return np.where(valid[..., None], c * Am, hdr)


def guide_step(inv_size, dims) -> float:
    e = min(1.0 / (float(f32(s)) * float(n)) for s, n in zip(inv_size, dims))
    return float(f32(0.5 * e))


def guides_ref(lib, scene_ptr, x, y, h):
    """The guides of pixel (x, y): (N.xyz, D, A.rgb, O) as float32, from the oracle's primitives."""
    o = (C.c_float * 3)()
    d = (C.c_float * 3)()
    lib.svo_camera_ray_pinhole(C.c_void_p(scene_ptr), x, y, o, d)
    tn, tf = C.c_float(0), C.c_float(0)
    O, Ds, T = f32(0), f32(0), f32(1)
    As = np.zeros(3, dtype=np.float32)
    Ns = np.zeros(3, dtype=np.float32)
    h = f32(h)
    if lib.svo_volume_intersect(C.c_void_p(scene_ptr), o, d, C.byref(tn), C.byref(tf)):
        tMin = f32(1e-6) if f32(tn.value) < 0 else f32(tn.value)
        tMax = f32(tf.value)
        ov = np.array(o[:], dtype=np.float32)
        dv = np.array(d[:], dtype=np.float32)
        p = (C.c_float * 3)()
        rgba = (C.c_float * 4)()
        gr = (C.c_float * 3)()
        i = 0
        while True:
            t = f32(tMin + f32(f32(i) * h))
            i += 1
            if not (t <= tMax):
                break
            pv = (ov + (dv * t).astype(np.float32)).astype(np.float32)
            p[0], p[1], p[2] = float(pv[0]), float(pv[1]), float(pv[2])
            xi = lib.svo_volume_intensity(C.c_void_p(scene_ptr), p)
            lib.svo_tex1d(C.c_void_p(scene_ptr), xi, rgba)
            sigma = f32(rgba[3])
            if sigma == 0:
                continue
            e = f32(lib.svo_expf(float(f32(-sigma * h))))
            w = f32(T * f32(f32(1) - e))
            T = f32(T * e)
            if w > 0:
                lib.svo_volume_gradient(C.c_void_p(scene_ptr), p, gr)
                O = f32(O + w)
                Ds = f32(Ds + f32(w * t))
                As = (As + (np.array(rgba[:3], dtype=np.float32) * w).astype(np.float32)).astype(np.float32)
                Ns = (Ns + (np.array(gr[:], dtype=np.float32) * w).astype(np.float32)).astype(np.float32)
            if T < f32(2.0 ** -10):
                break
    if O == 0:
        return np.array([0, 0, 0, -1, 1, 1, 1, 0], dtype=np.float32)
    n2 = f32(f32(f32(Ns[0] * Ns[0]) + f32(Ns[1] * Ns[1])) + f32(Ns[2] * Ns[2]))
    N = (Ns * f32(f32(1) / np.sqrt(n2, dtype=np.float32))).astype(np.float32) if n2 > 0 else np.zeros(3, dtype=np.float32)
    return np.array([N[0], N[1], N[2], Ds / O, As[0] / O, As[1] / O, As[2] / O, O], dtype=np.float32)
