"""Host side of the reference's render API, above the C ABI.

The reference's host code is C++ (Qt `Canvas`, gui/canvas.{h,cpp}); this module mirrors the
parts of it that drive the render path -- same names, argument meaning and call protocol --
so tests and the benchmark read like the reference's own host code:

  cudaCamera.Setup            core/cuda_camera.h:35-63      -> camera_setup / camera_setup_uvw
  cudaBBox.Set                core/geometry/cuda_bbox.h:25-31 -> bbox_set
  cudaVolume.Set/...          core/cuda_volume.h:18-37      -> volume_set
  VolumeReader::CreateDeviceVolume  core/VolumeReader.cpp:174-201
  Canvas (LoadVolume, setters, paintGL, ReStartRender)  gui/canvas.cpp:8-117, gui/canvas.h:43-175

All arithmetic that the reference does in `float` is done in numpy float32 here.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np

from . import abi
from .abi import (RenderParams, cudaAreaLight, cudaBBox, cudaCamera, cudaDisk, cudaEnvironmentLight,
                  cudaTransferFunction, cudaVolume, vec2, vec3)

f32 = np.float32


def _v(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float32).reshape(3)


def _to_vec3(a) -> vec3:
    a = _v(a)
    return vec3(a[0], a[1], a[2])


def _dot(a, b) -> np.float32:
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def _normalize(a) -> np.ndarray:
    a = _v(a)
    s = f32(1.0) / np.sqrt(_dot(a, a), dtype=np.float32)
    return (a * s).astype(np.float32)


def _cross(x, y) -> np.ndarray:
    x, y = _v(x), _v(y)
    return np.array([f32(x[1] * y[2]) - f32(y[1] * x[2]),
                     f32(x[2] * y[0]) - f32(y[2] * x[0]),
                     f32(x[0] * y[1]) - f32(y[0] * x[1])], dtype=np.float32)


def _tan_fov_over_two(fovx: float) -> float:
    # cuda_camera.h:44: tanf(fovx * 0.5f * M_PI / 180.f) -- float * double / float -> double -> tanf(float)
    arg = f32(float(f32(fovx) * f32(0.5)) * math.pi / 180.0)
    return float(np.tan(arg, dtype=np.float32))


def camera_setup(pos, target, up, fovx=45.0, apeture=0.0, focalLength=1.0, exposure=1.0,
                 imageW=640, imageH=640) -> cudaCamera:
    """cudaCamera::Setup(pos, target, up, ...), core/cuda_camera.h:50-63."""
    pos, target, up = _v(pos), _v(target), _v(up)
    w = _normalize(pos - target)
    u = _cross(up, w)
    v = _cross(w, u)
    return camera_setup_uvw(pos, u, v, w, fovx, apeture, focalLength, exposure, imageW, imageH)


def camera_setup_uvw(pos, u, v, w, fovx=45.0, apeture=0.0, focalLength=1.0, exposure=1.0,
                     imageW=640, imageH=640) -> cudaCamera:
    """cudaCamera::Setup(pos, u, v, w, ...), core/cuda_camera.h:35-48."""
    cam = cudaCamera()
    cam.pos, cam.u, cam.v, cam.w = _to_vec3(pos), _to_vec3(u), _to_vec3(v), _to_vec3(w)
    cam.imageW, cam.imageH = int(imageW), int(imageH)
    cam.aspectRatio = float(f32(imageW) / f32(imageH))
    cam.tanFovxOverTwo = _tan_fov_over_two(fovx)
    cam.exposure, cam.focalLength, cam.apeture = float(exposure), float(focalLength), float(apeture)
    return cam


def zoom_to_extent_eye_dist(volume_size, fov=45.0) -> float:
    """Canvas::ZoomToExtent, gui/canvas.cpp:191-197."""
    e = _v(volume_size)
    max_span = f32(max(e[0], e[1], e[2])) * f32(1.5)
    half = f32(math.radians(float(f32(fov) * f32(0.5))))
    return float(max_span / f32(f32(2.0) * np.tan(half, dtype=np.float32)))


def bbox_set(vmin, vmax) -> cudaBBox:
    """cudaBBox::Set, core/geometry/cuda_bbox.h:25-31."""
    vmin, vmax = _v(vmin), _v(vmax)
    b = cudaBBox()
    b.vmin, b.vmax = _to_vec3(vmin), _to_vec3(vmax)
    b.invSize = _to_vec3(f32(1.0) / (vmax - vmin))
    return b


def volume_size(dim, spacing) -> np.ndarray:
    """VolumeReader::GetVolumeSize, core/VolumeReader.cpp:187-190 (dim is (nx, ny, nz))."""
    return (np.asarray(dim, dtype=np.float32) * _v(spacing)).astype(np.float32)


def bounding_sphere_radius(dim, spacing) -> float:
    """VolumeReader::GetBoundingSphereRadius, core/VolumeReader.cpp:192-196."""
    s = volume_size(dim, spacing)
    return float(np.sqrt(_dot(s, s), dtype=np.float32) * f32(0.5))


def element_bounding_sphere_radius(spacing) -> float:
    """VolumeReader::GetElementBoundingSphereRadius (the ray caster's stepSize), VolumeReader.cpp:198-201."""
    s = _v(spacing)
    return float(np.sqrt(_dot(s, s), dtype=np.float32) * f32(0.5))


def create_device_volume(tex_handle: int, dim, spacing, max_magnitude: float) -> cudaVolume:
    """VolumeReader::CreateDeviceVolume, core/VolumeReader.cpp:174-185 (+ Canvas::LoadVolume defaults,
    gui/canvas.cpp:30-32 and gui/canvas.cpp:19)."""
    ext = volume_size(dim, spacing)
    vmax = ext - ext * f32(0.5)
    vmin = -vmax
    vol = cudaVolume()
    vol.bbox = bbox_set(vmin, vmax)
    sp = _v(spacing)
    vol.spacing = _to_vec3(sp)
    vol.invSpacing = _to_vec3(f32(1.0) / sp)
    vol.tex = int(tex_handle)
    vol.invMaxMagnitude = float(f32(1.0) / f32(max_magnitude))
    vol.x_clip, vol.y_clip, vol.z_clip = vec2(-1.0, 1.0), vec2(-1.0, 1.0), vec2(-1.0, 1.0)
    vol.densityScale = 1.0
    vol.gradientFactor = 0.5
    return vol


def make_area_light(center, normal, radius=10.0, color=(1.0, 1.0, 1.0), intensity=500.0) -> cudaAreaLight:
    """cudaAreaLight::Set(cudaDisk(center, normal, radius), color, intensity), cuda_arealight.h:18-23."""
    l = cudaAreaLight()
    l.disk = cudaDisk(float(radius), _to_vec3(center), _to_vec3(normal))
    l.color = _to_vec3(color)
    l.intensity = float(intensity)
    return l


def place_area_light(latitude_deg: float, longitude_deg: float, distance: float, radius=10.0,
                     color=(1.0, 1.0, 1.0), intensity=500.0) -> cudaAreaLight:
    """Light placement of MainWindow (gui/mainwindow.cpp:229-238, 338-361): start at (0, distance, 0),
    rotate by latitude about X and by longitude about Z (sic), aim at the origin."""
    pos = np.array([0.0, distance, 0.0], dtype=np.float32)
    lat, lon = math.radians(latitude_deg), math.radians(longitude_deg)
    cz, sz = f32(math.cos(lon)), f32(math.sin(lon))
    p1 = np.array([cz * pos[0] - sz * pos[1], sz * pos[0] + cz * pos[1], pos[2]], dtype=np.float32)
    cx, sx = f32(math.cos(lat)), f32(math.sin(lat))
    p2 = np.array([p1[0], cx * p1[1] - sx * p1[2], sx * p1[1] + cx * p1[2]], dtype=np.float32)
    return make_area_light(p2, _normalize(-p2), radius, color, intensity)


def env_light_constant(radiance=(1.0, 1.0, 1.0), intensity=0.5) -> cudaEnvironmentLight:
    """Lights::SetEnvionmentLight(radiance) + SetEnvironmentLightIntensity, gui/canvas.cpp:11-12."""
    e = cudaEnvironmentLight()
    e.tex = 0
    e.defaultRadiance = _to_vec3(radiance)
    e.intensity = float(intensity)
    e.offset = vec2(0.0, 0.0)
    return e


class SvrError(RuntimeError):
    pass


class Device:
    """Thin RAII-style wrapper over the svr_* helper entry points (non-fatal error mode)."""

    def __init__(self, device: int = 0, fatal_errors: bool = False):
        self.lib = abi.load()
        self.lib.svr_set_error_mode(1 if fatal_errors else 0)
        self.check(self.lib.svr_init(int(device)))

    def check(self, rc=0):
        code = self.lib.svr_last_error_code()
        if rc != 0 or code != 0:
            msg = self.lib.svr_last_error().decode("utf-8", "replace")
            self.lib.svr_clear_error()
            raise SvrError(f"libsvr_hip error {code}: {msg}")

    def info(self) -> str:
        return self.lib.svr_device_info().decode()

    def malloc(self, nbytes: int) -> int:
        p = self.lib.svr_device_malloc(int(nbytes))
        self.check()
        if not p:
            raise SvrError("svr_device_malloc returned null")
        return int(p)

    def free(self, ptr: int):
        self.check(self.lib.svr_device_free(C.c_void_p(ptr)))

    def to_host(self, ptr: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        self.check(self.lib.svr_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes))
        return out

    def to_device(self, ptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self.check(self.lib.svr_memcpy_h2d(C.c_void_p(ptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def synchronize(self):
        self.check(self.lib.svr_device_synchronize())

    def set_option(self, key: int, value: int):
        self.check(self.lib.svr_set_option(int(key), int(value)))

    def get_option(self, key: int) -> int:
        return int(self.lib.svr_get_option(int(key)))

    def counters(self) -> dict:
        c = abi.Counters()
        self.check(self.lib.svr_get_counters(C.byref(c)))
        return c.as_dict()

    def reset_counters(self):
        self.check(self.lib.svr_reset_counters())

    def kernel_time(self):
        ms, n = C.c_double(0.0), C.c_uint64(0)
        self.check(self.lib.svr_get_kernel_time(C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    # ---- denoised preview (SVR_OPT_DENOISE_PREVIEW, svr_denoise_to_ldr) ----
    def denoise_params(self, **overrides) -> abi.DenoiseParams:
        """The library's default svr_denoise_params with the named fields replaced."""
        p = abi.DenoiseParams()
        self.check(self.lib.svr_denoise_params_default(C.byref(p)))
        for k, v in overrides.items():
            if k not in dict(abi.DenoiseParams._fields_):
                raise AttributeError(k)
            setattr(p, k, v)
        return p

    def set_denoise_params(self, params: Optional[abi.DenoiseParams] = None, **overrides):
        """svr_set_denoise_params(params or the defaults with `overrides`)."""
        p = params if params is not None else self.denoise_params(**overrides)
        self.check(self.lib.svr_set_denoise_params(C.byref(p)))

    def get_denoise_params(self) -> abi.DenoiseParams:
        p = abi.DenoiseParams()
        self.check(self.lib.svr_get_denoise_params(C.byref(p)))
        return p

    def denoise_to_ldr(self, img_ptr: int, hdr_ptr: int, width: int, height: int, params: Optional[abi.DenoiseParams] = None):
        """svr_denoise_to_ldr: the whole width x height accumulator at hdr_ptr, denoised with the current scene's guides and tone-mapped
        into img_ptr (device pointers).  params None = the current parameters."""
        self.check(self.lib.svr_denoise_to_ldr(C.c_void_p(img_ptr), C.c_void_p(hdr_ptr), int(width), int(height),
                                               C.byref(params) if params is not None else None))

    def denoise_hdr(self, out_ptr: int, hdr_ptr: int, width: int, height: int, params: Optional[abi.DenoiseParams] = None):
        """svr_denoise_hdr: the same filter, HDR result (packed float3) into out_ptr."""
        self.check(self.lib.svr_denoise_hdr(C.c_void_p(out_ptr), C.c_void_p(hdr_ptr), int(width), int(height),
                                            C.byref(params) if params is not None else None))

    def guide_builds(self) -> int:
        return int(self.lib.svr_guide_builds())

    # ---- noise estimate (SVR_OPT_NOISE_ESTIMATE, svr_estimate_noise) ----
    def estimate_noise(self, hdr_m_ptr: int, m: int, hdr_n_ptr: int, n: int, width: int, height: int,
                       tile_ptr: Optional[int] = None) -> abi.NoiseEstimate:
        """svr_estimate_noise: the predicted tone-mapped error of the whole width x height accumulator A(n) at hdr_n_ptr, from A(m) at
        hdr_m_ptr (device pointers, 0 < m < n).  tile_ptr (device, ceil(W/16) x ceil(H/16) floats) receives the tile map if given."""
        est = abi.NoiseEstimate()
        self.check(self.lib.svr_estimate_noise(C.c_void_p(hdr_m_ptr), int(m), C.c_void_p(hdr_n_ptr), int(n), int(width), int(height),
                                               C.c_void_p(tile_ptr) if tile_ptr else None, C.byref(est)))
        return est

    def noise_estimate(self, tile_ptr: Optional[int] = None) -> abi.NoiseEstimate:
        """svr_get_noise_estimate: the latest estimate of the render being followed (frames == 0: none yet)."""
        est = abi.NoiseEstimate()
        self.check(self.lib.svr_get_noise_estimate(C.byref(est), C.c_void_p(tile_ptr) if tile_ptr else None))
        return est

    # ---- seeded region growing (svr_region_*): pick, segment, measure, show ----
    def _region_source(self, vox, shape):
        """(pointer argument, (nz, ny, nx), src_is_device, keep-alive) of a host u16 array or a device pointer with `shape`."""
        if isinstance(vox, np.ndarray):
            a = np.ascontiguousarray(vox, dtype=np.uint16)
            if a.ndim != 3:
                raise ValueError("the volume must be [nz][ny][nx]")
            return a.ctypes.data_as(C.c_void_p), a.shape, 0, a
        if shape is None:
            raise ValueError("a device volume needs shape=(nz, ny, nx)")
        return C.c_void_p(int(vox)), tuple(int(n) for n in shape), 1, None

    def region_params(self, lo: int = 0, hi: int = 65535, connectivity: int = 6, box=None, max_sweeps: int = 0) -> abi.RegionParams:
        """svr_region_params_default with the window, connectivity, box ((x0, y0, z0), (x1, y1, z1), inclusive) and cap replaced."""
        p = abi.RegionParams()
        self.check(self.lib.svr_region_params_default(C.byref(p)))
        p.lo, p.hi, p.connectivity, p.max_sweeps = int(lo), int(hi), int(connectivity), int(max_sweeps)
        if box is not None:
            for a in range(3):
                p.box_min[a], p.box_max[a] = int(box[0][a]), int(box[1][a])
        return p

    def region_grow(self, vox, seeds, lo: int, hi: int, connectivity: int = 6, box=None, max_sweeps: int = 0, shape=None,
                    mask_ptr: Optional[int] = None):
        """svr_region_grow: the connected component(s) of {lo <= v <= hi} (inside `box`) around the seed voxels (x, y, z).  vox is a
        host [nz][ny][nx] u16 array, or a device pointer with shape=(nz, ny, nx).  Returns (mask, stats): the region as a bool array
        [nz][ny][nx] and the svr_region_stats.  mask_ptr: a device buffer of region_mask_words(shape) uint32 that receives the bit mask
        (else a temporary one is used)."""
        src, (nz, ny, nx), on_dev, _keep = self._region_source(vox, shape)
        xyz = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
        p = self.region_params(lo, hi, connectivity, box, max_sweeps)
        words = region_mask_words((nz, ny, nx))
        buf = mask_ptr if mask_ptr is not None else self.malloc(4 * max(words, 1))
        st = abi.RegionStats()
        try:
            self.check(self.lib.svr_region_grow(src, nx, ny, nz, on_dev, xyz.ctypes.data_as(C.POINTER(C.c_int32)), len(xyz), C.byref(p),
                                                C.c_void_p(buf), C.byref(st)))
            mask = region_mask_unpack(self.to_host(buf, (words,), np.uint32), (nz, ny, nx))
        finally:
            if mask_ptr is None:
                self.free(buf)
        return mask, st

    def region_stats_of(self, vox, mask, shape=None) -> abi.RegionStats:
        """svr_region_stats_of: the statistics of any mask (a bool array [nz][ny][nx], or a device pointer to the bit mask)."""
        src, (nz, ny, nx), on_dev, _keep = self._region_source(vox, shape)
        buf, owned = self._region_mask(mask, (nz, ny, nx))
        st = abi.RegionStats()
        try:
            self.check(self.lib.svr_region_stats_of(src, nx, ny, nz, on_dev, C.c_void_p(buf), C.byref(st)))
        finally:
            if owned:
                self.free(buf)
        return st

    def region_apply(self, vox, mask, mode: int = abi.REGION_KEEP, fill: int = 0, shape=None, out_ptr: Optional[int] = None):
        """svr_region_apply: the volume with the voxels outside (REGION_KEEP) or inside (REGION_REMOVE) the region set to `fill`.
        Returns a u16 array [nz][ny][nx]; with out_ptr (a device buffer of nx * ny * nz u16, which may be a device `vox` itself) the
        result stays on the device and out_ptr is returned."""
        src, (nz, ny, nx), on_dev, _keep = self._region_source(vox, shape)
        buf, owned = self._region_mask(mask, (nz, ny, nx))
        out = out_ptr if out_ptr is not None else self.malloc(2 * nx * ny * nz)
        try:
            self.check(self.lib.svr_region_apply(src, nx, ny, nz, on_dev, C.c_void_p(buf), int(mode), int(fill), C.c_void_p(out)))
            if out_ptr is not None:
                self.synchronize()
                return out_ptr
            return self.to_host(out, (nz, ny, nx), np.uint16)
        finally:
            if owned:
                self.free(buf)
            if out_ptr is None:
                self.free(out)

    def _region_mask(self, mask, shape):
        """(device pointer, owned) of a bool array (uploaded as the bit mask) or of a device pointer."""
        if isinstance(mask, np.ndarray):
            words = region_mask_pack(mask.reshape(shape))
            buf = self.malloc(4 * max(len(words), 1))
            self.to_device(buf, words)
            return buf, True
        return int(mask), False

    # ---- operations on region masks (svr_region_morph / _combine / _reconstruct / _fill_holes / _detach) ----
    def _mask_call(self, masks, shape, out_ptr, call):
        """Runs call(device pointers of `masks` (None stays None), shape, out) and returns the result mask as a bool array [nz][ny][nx].
        masks: bool arrays [nz][ny][nx] (uploaded) or device pointers with shape=(nz, ny, nx); out_ptr: a device buffer of
        region_mask_words(shape) uint32 that receives the bit mask (else a temporary one is used)."""
        arrays = [m for m in masks if isinstance(m, np.ndarray)]
        if arrays:
            shape = arrays[0].shape
        if shape is None:
            raise ValueError("device masks need shape=(nz, ny, nx)")
        shape = tuple(int(n) for n in shape)
        if len(shape) != 3:
            raise ValueError("a mask must be [nz][ny][nx]")
        bufs = [None if m is None else self._region_mask(m, shape) for m in masks]
        words = region_mask_words(shape)
        out = out_ptr if out_ptr is not None else self.malloc(4 * max(words, 1))
        try:
            extra = call([None if b is None else C.c_void_p(b[0]) for b in bufs], shape, C.c_void_p(out))
            mask = region_mask_unpack(self.to_host(out, (words,), np.uint32), shape)
        finally:
            for b in bufs:
                if b is not None and b[1]:
                    self.free(b[0])
            if out_ptr is None:
                self.free(out)
        return mask if extra is None else (mask, extra)

    def region_morph(self, mask, op: int, element: int = 6, radius: int = 1, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_morph: MORPH_DILATE / _ERODE / _OPEN / _CLOSE of a mask by the unit element 6 / 18 / 26 applied `radius` times."""
        def call(p, s, out):
            self.check(self.lib.svr_region_morph(p[0], s[2], s[1], s[0], int(op), int(element), int(radius), out))
        return self._mask_call([mask], shape, out_ptr, call)

    def region_combine(self, a, b, op: int, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_combine: MASK_AND / _OR / _ANDNOT (a & ~b) / _XOR of two masks, or MASK_NOT of a (b = None).  out_ptr may be a or b."""
        def call(p, s, out):
            self.check(self.lib.svr_region_combine(p[0], p[1], s[2], s[1], s[0], int(op), out))
        return self._mask_call([a, b], shape, out_ptr, call)

    def region_reconstruct(self, marker, cand, connectivity: int = 6, max_sweeps: int = 0, shape=None, out_ptr: Optional[int] = None):
        """svr_region_reconstruct: the components of `cand` that hold a voxel of marker & cand.  Returns (mask, sweeps)."""
        def call(p, s, out):
            sweeps = C.c_uint32(0)
            self.check(self.lib.svr_region_reconstruct(p[0], p[1], s[2], s[1], s[0], int(connectivity), int(max_sweeps), out, C.byref(sweeps)))
            return int(sweeps.value)
        return self._mask_call([marker, cand], shape, out_ptr, call)

    def region_fill_holes(self, mask, background_connectivity: int = 6, max_sweeps: int = 0, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_fill_holes: the mask and every background voxel that cannot reach a face of the volume."""
        def call(p, s, out):
            self.check(self.lib.svr_region_fill_holes(p[0], s[2], s[1], s[0], int(background_connectivity), int(max_sweeps), out))
        return self._mask_call([mask], shape, out_ptr, call)

    def region_detach(self, mask, seeds, element: int = 6, radius: int = 1, connectivity: int = 6, max_sweeps: int = 0, shape=None,
                      out_ptr: Optional[int] = None):
        """svr_region_detach: the part of a grown region around the seed voxels (x, y, z) that survives an opening by `element` applied
        `radius` times -- what hangs on it by thinner connections is cut off.  Returns (mask, status): REGION_STATUS_OK or _EMPTY."""
        xyz = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)

        def call(p, s, out):
            status = C.c_int32(0)
            self.check(self.lib.svr_region_detach(p[0], s[2], s[1], s[0], xyz.ctypes.data_as(C.POINTER(C.c_int32)), len(xyz), int(element),
                                                  int(radius), int(connectivity), int(max_sweeps), out, C.byref(status)))
            return int(status.value)
        return self._mask_call([mask], shape, out_ptr, call)

    # ---- connected components of region masks (svr_region_threshold / _label / _label_table / _select / _select_by_size) ----
    def region_threshold(self, vox, lo: int, hi: int, box=None, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_threshold: the mask {voxel in `box` : lo <= v <= hi} of a host [nz][ny][nx] u16 array or a device pointer with
        shape=(nz, ny, nx); box = ((x0, y0, z0), (x1, y1, z1)), inclusive, or None for the whole volume.  Returns the bool array."""
        src, (nz, ny, nx), on_dev, _keep = self._region_source(vox, shape)
        b0 = b1 = None
        if box is not None:
            b0, b1 = (C.c_int32 * 3)(*[int(t) for t in box[0]]), (C.c_int32 * 3)(*[int(t) for t in box[1]])

        def call(p, s, out):
            self.check(self.lib.svr_region_threshold(src, nx, ny, nz, on_dev, int(lo), int(hi), b0, b1, out))
        return self._mask_call([], (nz, ny, nx), out_ptr, call)

    def _region_labels(self, labels, shape):
        """(device pointer, (nz, ny, nx), owned) of a uint32 label array [nz][ny][nx] (uploaded) or of a device pointer with `shape`."""
        if isinstance(labels, np.ndarray):
            a = np.ascontiguousarray(labels, dtype=np.uint32)
            if a.ndim != 3:
                raise ValueError("the labels must be [nz][ny][nx]")
            buf = self.malloc(max(a.nbytes, 4))
            self.to_device(buf, a)
            return buf, a.shape, True
        if shape is None:
            raise ValueError("device labels need shape=(nz, ny, nx)")
        return int(labels), tuple(int(n) for n in shape), False

    def region_label(self, mask, connectivity: int = 6, shape=None, out_ptr: Optional[int] = None):
        """svr_region_label: the connected components of a mask (a bool array [nz][ny][nx], or a device pointer with shape=) under
        connectivity 6 / 18 / 26, numbered 1 .. K by their first voxel.  Returns (labels, K): a uint32 array [nz][ny][nx], or out_ptr
        itself when a device buffer of 4 nx ny nz bytes is given."""
        if isinstance(mask, np.ndarray):
            shape = mask.shape
        if shape is None:
            raise ValueError("a device mask needs shape=(nz, ny, nx)")
        nz, ny, nx = (int(n) for n in shape)
        buf, owned = self._region_mask(mask, (nz, ny, nx))
        out = out_ptr if out_ptr is not None else self.malloc(4 * max(nx * ny * nz, 1))
        k = C.c_uint32(0)
        try:
            self.check(self.lib.svr_region_label(C.c_void_p(buf), nx, ny, nz, int(connectivity), C.c_void_p(out), C.byref(k)))
            if out_ptr is not None:
                return out_ptr, int(k.value)
            return self.to_host(out, (nz, ny, nx), np.uint32), int(k.value)
        finally:
            if owned:
                self.free(buf)
            if out_ptr is None:
                self.free(out)

    def region_label_table(self, labels, count: int, vox=None, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_label_table: the svr_region_component of the labels 1 .. count as a numpy structured array (COMPONENT_DTYPE),
        indexed by label - 1.  labels: a uint32 array [nz][ny][nx] or a device pointer with shape=; vox (optional, for `sum`): a host
        u16 array or a device pointer of the same shape.  out_ptr: a device buffer of 40 * count bytes that receives the table."""
        lbuf, (nz, ny, nx), lowned = self._region_labels(labels, shape)
        src, on_dev = None, 0
        if vox is not None:
            src, vshape, on_dev, _keep = self._region_source(vox, (nz, ny, nx))
            if tuple(vshape) != (nz, ny, nx):
                raise ValueError("the volume and the labels differ in shape")
        out = out_ptr if out_ptr is not None else self.malloc(40 * max(int(count), 1))
        try:
            self.check(self.lib.svr_region_label_table(C.c_void_p(lbuf), src, nx, ny, nz, on_dev, int(count), C.c_void_p(out)))
            self.synchronize()
            return self.to_host(out, (int(count),), COMPONENT_DTYPE)
        finally:
            if lowned:
                self.free(lbuf)
            if out_ptr is None:
                self.free(out)

    def region_select(self, labels, count: int, keep, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_select: the mask of the voxels whose label has a non-zero entry in keep (count + 1 entries, indexed by label; entry
        0 is ignored)."""
        lbuf, lshape, lowned = self._region_labels(labels, shape)
        k = np.ascontiguousarray(keep, dtype=np.uint8).reshape(-1)
        if len(k) != int(count) + 1:
            raise ValueError("keep must have count + 1 entries")
        kbuf = self.malloc(len(k))
        self.to_device(kbuf, k)

        def call(p, s, out):
            self.check(self.lib.svr_region_select(C.c_void_p(lbuf), s[2], s[1], s[0], int(count), C.c_void_p(kbuf), out))
        try:
            return self._mask_call([], lshape, out_ptr, call)
        finally:
            self.free(kbuf)
            if lowned:
                self.free(lbuf)

    def region_select_by_size(self, labels, count: int, table=None, min_voxels: int = 0, largest_k: int = 0, shape=None,
                              out_ptr: Optional[int] = None):
        """svr_region_select_by_size: the components with at least min_voxels voxels among the largest_k largest (0 = no limit; ties go
        to the lower label).  table: the structured array of region_label_table, a device pointer to it, or None (it is computed).
        Returns (mask, kept)."""
        lbuf, lshape, lowned = self._region_labels(labels, shape)
        tbuf, towned = None, True
        try:
            if table is None:
                tbuf = self.malloc(40 * max(int(count), 1))
                self.region_label_table(lbuf, count, shape=lshape, out_ptr=tbuf)
            elif isinstance(table, np.ndarray):
                t = np.ascontiguousarray(table, dtype=COMPONENT_DTYPE)
                tbuf = self.malloc(max(t.nbytes, 40))
                self.to_device(tbuf, t)
            else:
                tbuf, towned = int(table), False

            def call(p, s, out):
                kept = C.c_uint32(0)
                self.check(self.lib.svr_region_select_by_size(C.c_void_p(lbuf), s[2], s[1], s[0], int(count), C.c_void_p(tbuf), int(min_voxels),
                                                              int(largest_k), out, C.byref(kept)))
                return int(kept.value)
            return self._mask_call([], lshape, out_ptr, call)
        finally:
            if towned and tbuf is not None:
                self.free(tbuf)
            if lowned:
                self.free(lbuf)

    def region_label_last_ms(self) -> float:
        ms = C.c_float(0.0)
        self.check(self.lib.svr_region_label_last_ms(C.byref(ms)))
        return float(ms.value)

    # ---- exact Euclidean distance maps and ball morphology (svr_region_distance / _distance_select / _ball / _distance_max / _distance_volume) ----
    @staticmethod
    def _weights(weights):
        return None if weights is None else (C.c_uint32 * 3)(*[int(t) for t in weights])

    def _region_map(self, d2, shape):
        """(device pointer, (nz, ny, nx), owned) of a uint32 map [nz][ny][nx] (uploaded) or of a device pointer with `shape`."""
        return self._region_labels(d2, shape)

    def region_distance(self, mask, shape=None, weights=None, target: int = abi.DIST_TO_SET, out_ptr: Optional[int] = None):
        """svr_region_distance: the exact squared distance, under the integer weights (wx, wy, wz) (None = 1, 1, 1), of every voxel to the
        nearest set voxel (DIST_TO_SET) or to the nearest unset voxel of the volume (DIST_TO_UNSET); DIST_NONE everywhere when there is
        none.  mask: a bool array [nz][ny][nx], or a device pointer with shape=.  Returns a uint32 array [nz][ny][nx], or out_ptr itself
        when a device buffer of 4 nx ny nz bytes is given."""
        if isinstance(mask, np.ndarray):
            shape = mask.shape
        if shape is None:
            raise ValueError("a device mask needs shape=(nz, ny, nx)")
        nz, ny, nx = (int(n) for n in shape)
        buf, owned = self._region_mask(mask, (nz, ny, nx))
        out = out_ptr if out_ptr is not None else self.malloc(4 * max(nx * ny * nz, 1))
        try:
            self.check(self.lib.svr_region_distance(C.c_void_p(buf), nx, ny, nz, self._weights(weights), int(target), C.c_void_p(out)))
            if out_ptr is not None:
                return out_ptr
            return self.to_host(out, (nz, ny, nx), np.uint32)
        finally:
            if owned:
                self.free(buf)
            if out_ptr is None:
                self.free(out)

    def region_distance_select(self, d2, lo2: int, hi2: int, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_distance_select: the mask of the voxels with lo2 <= d2 <= hi2.  d2: a uint32 array [nz][ny][nx] or a device pointer
        with shape=."""
        dbuf, dshape, downed = self._region_map(d2, shape)

        def call(p, s, out):
            self.check(self.lib.svr_region_distance_select(C.c_void_p(dbuf), s[2], s[1], s[0], int(lo2), int(hi2), out))
        try:
            return self._mask_call([], dshape, out_ptr, call)
        finally:
            if downed:
                self.free(dbuf)

    def region_ball(self, mask, op: int, r2: int, weights=None, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_ball: MORPH_DILATE / _ERODE / _OPEN / _CLOSE of a mask by the ball {offset : weighted d^2 <= r2}."""
        def call(p, s, out):
            self.check(self.lib.svr_region_ball(p[0], s[2], s[1], s[0], int(op), self._weights(weights), int(r2), out))
        return self._mask_call([mask], shape, out_ptr, call)

    def region_distance_max(self, d2, mask=None, shape=None):
        """svr_region_distance_max: (max_d2, first_index, status) over the voxels of `mask` (a bool array or a device pointer; None = all
        voxels): the largest value other than DIST_NONE and the smallest linear voxel index that attains it; status REGION_STATUS_EMPTY
        when there is no such voxel."""
        dbuf, (nz, ny, nx), downed = self._region_map(d2, shape)
        mbuf, mowned = (None, False) if mask is None else self._region_mask(mask, (nz, ny, nx))
        m, first, status = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        try:
            self.check(self.lib.svr_region_distance_max(C.c_void_p(dbuf), C.c_void_p(mbuf) if mbuf is not None else None, nx, ny, nz, C.byref(m),
                                                        C.byref(first), C.byref(status)))
        finally:
            if downed:
                self.free(dbuf)
            if mowned:
                self.free(mbuf)
        return int(m.value), int(first.value), int(status.value)

    def region_distance_volume(self, d2, scale: int = 1, shape=None, out_ptr: Optional[int] = None):
        """svr_region_distance_volume: min(65535, isqrt(d2 scale^2)) as a u16 array [nz][ny][nx] (DIST_NONE gives 65535); with out_ptr (a
        device buffer of nx * ny * nz u16) the result stays on the device and out_ptr is returned."""
        dbuf, (nz, ny, nx), downed = self._region_map(d2, shape)
        out = out_ptr if out_ptr is not None else self.malloc(2 * max(nx * ny * nz, 1))
        try:
            self.check(self.lib.svr_region_distance_volume(C.c_void_p(dbuf), nx, ny, nz, int(scale), C.c_void_p(out)))
            self.synchronize()
            if out_ptr is not None:
                return out_ptr
            return self.to_host(out, (nz, ny, nx), np.uint16)
        finally:
            if downed:
                self.free(dbuf)
            if out_ptr is None:
                self.free(out)

    def region_distance_last_ms(self) -> float:
        ms = C.c_float(0.0)
        self.check(self.lib.svr_region_distance_last_ms(C.byref(ms)))
        return float(ms.value)

    def region_distance_pass_ms(self):
        """(rows, y, z) HIP-event times of the passes of the last transform."""
        ms = [C.c_float(0.0) for _ in range(3)]
        self.check(self.lib.svr_region_distance_pass_ms(*[C.byref(t) for t in ms]))
        return tuple(float(t.value) for t in ms)

    # ---- geodesic distances, influence zones and splitting (svr_region_geodesic / _seed_labels / _split / _zone_cut) ----
    @staticmethod
    def _step_weights(weights):
        return None if weights is None else (C.c_uint32 * 7)(*[int(t) for t in weights])

    def region_geodesic(self, labels, domain, shape=None, step_weights=None, max_sweeps: int = 0, want_dist: bool = True, want_zones: bool = True,
                        dist_ptr: Optional[int] = None, zones_ptr: Optional[int] = None):
        """svr_region_geodesic: (dist, zones, sweeps) inside `domain` (a bool array [nz][ny][nx], or a device pointer with shape=) from the
        voxels whose entry in `labels` (a uint32 array or a device pointer) is non-zero: the cost of the cheapest path of moves with the
        seven step weights (x, y, z, xy, xz, yz, xyz; 0 forbids a class; None = 3, 3, 3, 4, 4, 4, 5) and the smallest label that attains it.
        GEO_NONE / 0 where no marker reaches.  An output that is not wanted is None; with dist_ptr / zones_ptr (device buffers of
        4 nx ny nz bytes; zones_ptr may be the labels' own pointer) the result stays on the device and the pointer is returned."""
        lbuf, (nz, ny, nx), lowned = self._region_labels(labels, domain.shape if isinstance(domain, np.ndarray) else shape)
        mbuf, mowned = self._region_mask(domain, (nz, ny, nx))
        nbytes = 4 * max(nx * ny * nz, 1)
        dout = dist_ptr if dist_ptr is not None else (self.malloc(nbytes) if want_dist else None)
        zout = zones_ptr if zones_ptr is not None else (self.malloc(nbytes) if want_zones else None)
        sweeps = C.c_uint32(0)
        try:
            self.check(self.lib.svr_region_geodesic(C.c_void_p(lbuf), C.c_void_p(mbuf), nx, ny, nz, self._step_weights(step_weights), int(max_sweeps),
                                                    None if dout is None else C.c_void_p(dout), None if zout is None else C.c_void_p(zout),
                                                    C.byref(sweeps)))
            dist = dist_ptr if dist_ptr is not None else (self.to_host(dout, (nz, ny, nx), np.uint32) if dout is not None else None)
            zones = zones_ptr if zones_ptr is not None else (self.to_host(zout, (nz, ny, nx), np.uint32) if zout is not None else None)
            return dist, zones, int(sweeps.value)
        finally:
            if lowned:
                self.free(lbuf)
            if mowned:
                self.free(mbuf)
            if dist_ptr is None and dout is not None:
                self.free(dout)
            if zones_ptr is None and zout is not None:
                self.free(zout)

    def region_seed_labels(self, seeds, shape, out_ptr: Optional[int] = None):
        """svr_region_seed_labels: a zero uint32 array [nz][ny][nx] with the label i + 1 on the voxel (x, y, z) of seed i (the lowest i of
        several on a voxel).  Returns the array, or out_ptr itself when a device buffer of 4 nx ny nz bytes is given."""
        nz, ny, nx = (int(n) for n in shape)
        xyz = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
        out = out_ptr if out_ptr is not None else self.malloc(4 * max(nx * ny * nz, 1))
        try:
            self.check(self.lib.svr_region_seed_labels(xyz.ctypes.data_as(C.POINTER(C.c_int32)), len(xyz), nx, ny, nz, C.c_void_p(out)))
            self.synchronize()
            if out_ptr is not None:
                return out_ptr
            return self.to_host(out, (nz, ny, nx), np.uint32)
        finally:
            if out_ptr is None:
                self.free(out)

    def region_split(self, mask, r2: int, connectivity: int = 26, dist_weights=None, step_weights=None, max_sweeps: int = 0, shape=None,
                     out_ptr: Optional[int] = None):
        """svr_region_split: erodes the mask by the ball of squared radius r2 (dist_weights as in region_ball), labels the cores under
        `connectivity` and gives every voxel of the mask to the core that is nearest inside the mask (step_weights as in
        region_geodesic; None = the chamfer weights of the connectivity).  Returns (zones, count, unreached, sweeps): a uint32 array
        [nz][ny][nx] (or out_ptr itself), the number of cores, the voxels of the mask that no core reaches, the sweeps launched."""
        if isinstance(mask, np.ndarray):
            shape = mask.shape
        if shape is None:
            raise ValueError("a device mask needs shape=(nz, ny, nx)")
        nz, ny, nx = (int(n) for n in shape)
        buf, owned = self._region_mask(mask, (nz, ny, nx))
        out = out_ptr if out_ptr is not None else self.malloc(4 * max(nx * ny * nz, 1))
        count, lost, sweeps = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        try:
            self.check(self.lib.svr_region_split(C.c_void_p(buf), nx, ny, nz, self._weights(dist_weights), int(r2), int(connectivity),
                                                 self._step_weights(step_weights), int(max_sweeps), C.c_void_p(out), C.byref(count), C.byref(lost),
                                                 C.byref(sweeps)))
            zones = out_ptr if out_ptr is not None else self.to_host(out, (nz, ny, nx), np.uint32)
            return zones, int(count.value), int(lost.value), int(sweeps.value)
        finally:
            if owned:
                self.free(buf)
            if out_ptr is None:
                self.free(out)

    def region_zone_cut(self, zones, connectivity: int = 26, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_zone_cut: the mask of the voxels with a zone and no connectivity-neighbour in a smaller non-zero zone: the zones with a
        cut of one voxel between them.  zones: a uint32 array [nz][ny][nx] or a device pointer with shape=."""
        zbuf, zshape, zowned = self._region_labels(zones, shape)

        def call(p, s, out):
            self.check(self.lib.svr_region_zone_cut(C.c_void_p(zbuf), s[2], s[1], s[0], int(connectivity), out))
        try:
            return self._mask_call([], zshape, out_ptr, call)
        finally:
            if zowned:
                self.free(zbuf)

    def region_geodesic_last_ms(self) -> float:
        ms = C.c_float(0.0)
        self.check(self.lib.svr_region_geodesic_last_ms(C.byref(ms)))
        return float(ms.value)

    # ---- grow from seeds (svr_region_growcut / _seed_classes / _label_paint) ----
    def growcut_params(self, step_weights=None, connectivity: int = 26, gain: int = 1, shift: int = 0, max_sweeps: int = 0) -> abi.GrowcutParams:
        """svr_region_growcut_params_default of the connectivity with the weights (if given), gain, shift and cap replaced."""
        p = abi.GrowcutParams()
        self.check(self.lib.svr_region_growcut_params_default(C.byref(p), int(connectivity)))
        if step_weights is not None:
            for c in range(7):
                p.step_weights[c] = int(step_weights[c])
        p.contrast_gain, p.contrast_shift, p.max_sweeps = int(gain), int(shift), int(max_sweeps)
        return p

    def region_growcut(self, vox, labels, domain=None, shape=None, step_weights=None, connectivity: int = 26, gain: int = 1, shift: int = 0,
                       max_sweeps: int = 0, want_cost: bool = True, want_zones: bool = True, cost_ptr: Optional[int] = None,
                       zones_ptr: Optional[int] = None):
        """svr_region_growcut: (cost, zones, info).  Every voxel of `domain` (a bool array [nz][ny][nx] or a device pointer; None = the
        whole volume) gets the class of the marker (non-zero entries of `labels`, a uint32 array or a device pointer) that reaches it
        over the cheapest path, a move costing step_weights[class] + gain * (|I(u) - I(v)| >> shift) on the raw voxels of `vox` (a host
        u16 array, or a device pointer with shape=).  step_weights None = 1 on the move classes of `connectivity`.  GEO_NONE / 0 where no
        marker reaches.  An output that is not wanted is None; with cost_ptr / zones_ptr (device buffers of 4 nx ny nz bytes; zones_ptr
        may be the labels' own pointer) the result stays on the device and the pointer is returned.  info is the svr_growcut_info.  A
        failure raises SvrError with .code and .info set; for REGION_ERR_RANGE (costs reached GROWCUT_CAP) .cost and .zones hold the
        saturated solution as well."""
        src, (nz, ny, nx), on_dev, _keep = self._region_source(vox, shape)
        lbuf, lshape, lowned = self._region_labels(labels, (nz, ny, nx))
        if tuple(lshape) != (nz, ny, nx):
            raise ValueError("the volume and the labels differ in shape")
        mbuf, mowned = (None, False) if domain is None else self._region_mask(domain, (nz, ny, nx))
        p = self.growcut_params(step_weights, connectivity, gain, shift, max_sweeps)
        dims = (C.c_int32 * 3)(nx, ny, nz)
        nbytes = 4 * max(nx * ny * nz, 1)
        cout = cost_ptr if cost_ptr is not None else (self.malloc(nbytes) if want_cost else None)
        zout = zones_ptr if zones_ptr is not None else (self.malloc(nbytes) if want_zones else None)
        info = abi.GrowcutInfo()

        def results():
            cost = cost_ptr if cost_ptr is not None else (self.to_host(cout, (nz, ny, nx), np.uint32) if cout is not None else None)
            zones = zones_ptr if zones_ptr is not None else (self.to_host(zout, (nz, ny, nx), np.uint32) if zout is not None else None)
            return cost, zones
        try:
            rc = self.lib.svr_region_growcut(src, dims, on_dev, C.c_void_p(lbuf), None if mbuf is None else C.c_void_p(mbuf), C.byref(p),
                                             None if cout is None else C.c_void_p(cout), None if zout is None else C.c_void_p(zout), C.byref(info))
            try:
                self.check(rc)
            except SvrError as e:
                e.code, e.info = int(rc), info
                if rc == abi.REGION_ERR_RANGE:
                    e.cost, e.zones = results()
                raise
            return results() + (info,)
        finally:
            if lowned:
                self.free(lbuf)
            if mowned:
                self.free(mbuf)
            if cost_ptr is None and cout is not None:
                self.free(cout)
            if zones_ptr is None and zout is not None:
                self.free(zout)

    def region_seed_classes(self, seeds, classes, shape, out_ptr: Optional[int] = None):
        """svr_region_seed_classes: a zero uint32 array [nz][ny][nx] with classes[i] on the voxel (x, y, z) of seed i (the lowest i of
        several on a voxel).  Returns the array, or out_ptr itself when a device buffer of 4 nx ny nz bytes is given."""
        nz, ny, nx = (int(n) for n in shape)
        xyz = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
        cls = np.ascontiguousarray(classes, dtype=np.uint32).reshape(-1)
        if len(cls) != len(xyz):
            raise ValueError("one class per seed")
        out = out_ptr if out_ptr is not None else self.malloc(4 * max(nx * ny * nz, 1))
        try:
            self.check(self.lib.svr_region_seed_classes(xyz.ctypes.data_as(C.POINTER(C.c_int32)), cls.ctypes.data_as(C.POINTER(C.c_uint32)), len(xyz),
                                                        (C.c_int32 * 3)(nx, ny, nz), C.c_void_p(out)))
            self.synchronize()
            if out_ptr is not None:
                return out_ptr
            return self.to_host(out, (nz, ny, nx), np.uint32)
        finally:
            if out_ptr is None:
                self.free(out)

    def region_label_paint(self, labels, mask, label: int, only_unlabelled: bool = False, shape=None):
        """svr_region_label_paint: `label` on every voxel of `mask` (a bool array or a device pointer), or only where the label is still 0.
        labels: a uint32 array [nz][ny][nx] (the painted copy is returned) or a device pointer with shape= (painted in place and
        returned)."""
        lbuf, (nz, ny, nx), lowned = self._region_labels(labels, shape)
        mbuf, mowned = self._region_mask(mask, (nz, ny, nx))
        try:
            self.check(self.lib.svr_region_label_paint(C.c_void_p(lbuf), (C.c_int32 * 3)(nx, ny, nz), C.c_void_p(mbuf), int(label), int(bool(only_unlabelled))))
            self.synchronize()
            return self.to_host(lbuf, (nz, ny, nx), np.uint32) if lowned else lbuf
        finally:
            if lowned:
                self.free(lbuf)
            if mowned:
                self.free(mbuf)

    def region_growcut_last_ms(self) -> float:
        ms = C.c_float(0.0)
        self.check(self.lib.svr_region_growcut_last_ms(C.byref(ms)))
        return float(ms.value)

    # ---- histograms of the u16 voxels (svr_volume_histogram, svr_region_label_histogram); the analysis is in the module functions ----
    def histogram_params(self, lo: int = 0, hi: int = 65535, shift: int = 0, box=None) -> abi.HistogramParams:
        """svr_histogram_params_default with the window, shift and box ((x0, y0, z0), (x1, y1, z1), inclusive) replaced."""
        return histogram_params(lo, hi, shift, box, self.lib)

    def _histogram_out(self, cells, out_ptr, call):
        out = out_ptr if out_ptr is not None else self.malloc(4 * max(cells, 1))
        try:
            call(C.c_void_p(out))
            self.synchronize()
            return self.to_host(out, (cells,), np.uint32)
        finally:
            if out_ptr is None:
                self.free(out)

    def volume_histogram(self, vox, mask=None, lo: int = 0, hi: int = 65535, shift: int = 0, box=None, shape=None,
                         out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_volume_histogram: np.uint32[bins], bins = ((hi - lo) >> shift) + 1: the voxels of `box` (inclusive, cut to the volume; None
        = all) whose mask bit is set (mask: a bool array [nz][ny][nx], a device pointer to the bit mask, or None = every voxel) and whose
        value v lies in lo .. hi, counted in bin (v - lo) >> shift.  vox is a host [nz][ny][nx] u16 array, or a device pointer with
        shape=(nz, ny, nx).  out_ptr: a device buffer of 4 * bins bytes that receives the counts."""
        src, (nz, ny, nx), on_dev, _keep = self._region_source(vox, shape)
        p = self.histogram_params(lo, hi, shift, box)
        bins = int(self.lib.svr_histogram_bins(C.byref(p)))
        mbuf, mowned = (None, False) if mask is None else self._region_mask(mask, (nz, ny, nx))
        dims = (C.c_int32 * 3)(nx, ny, nz)
        try:
            return self._histogram_out(bins, out_ptr, lambda out: self.check(self.lib.svr_volume_histogram(
                src, dims, on_dev, None if mbuf is None else C.c_void_p(mbuf), C.byref(p), out)))
        finally:
            if mowned:
                self.free(mbuf)

    def region_label_histogram(self, labels, vox, count: int, lo: int = 0, hi: int = 65535, shift: int = 0, box=None, shape=None,
                               out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_label_histogram: np.uint32[count + 1, bins]; row l is the histogram of the voxels whose label is l (row 0: the
        background; labels above count are ignored).  labels: a uint32 array [nz][ny][nx] or a device pointer with shape=; vox, the
        window, shift and box as in volume_histogram.  out_ptr: a device buffer of 4 * (count + 1) * bins bytes."""
        lbuf, (nz, ny, nx), lowned = self._region_labels(labels, shape)
        try:
            src, vshape, on_dev, _keep = self._region_source(vox, (nz, ny, nx))
            if tuple(vshape) != (nz, ny, nx):
                raise ValueError("the volume and the labels differ in shape")
            p = self.histogram_params(lo, hi, shift, box)
            bins = int(self.lib.svr_histogram_bins(C.byref(p)))
            dims = (C.c_int32 * 3)(nx, ny, nz)
            cells = (int(count) + 1) * bins
            if bins == 0 or cells > abi.HISTOGRAM_MAX_CELLS:
                cells = 0                                         # the library refuses the call: a token buffer is enough to hear it
            return self._histogram_out(cells, out_ptr, lambda out: self.check(self.lib.svr_region_label_histogram(
                C.c_void_p(lbuf), src, dims, on_dev, int(count), C.byref(p), out))).reshape(int(count) + 1, bins)
        finally:
            if lowned:
                self.free(lbuf)

    def volume_histogram_last_ms(self) -> float:
        ms = C.c_float(0.0)
        self.check(self.lib.svr_volume_histogram_last_ms(C.byref(ms)))
        return float(ms.value)

    # ---- overlays: region masks and label maps on slices and 3D views (svr_slice_ids, svr_hit_ids, svr_overlay_ids, svr_overlay_slice) ----
    def overlay_style(self, fill_alpha: Optional[int] = None, edge_alpha: Optional[int] = None, palette=None) -> abi.OverlayStyle:
        """The library's default svr_overlay_style (fill 96, edge 255, built-in palette) with the named members replaced.  palette: up
        to abi.OVERLAY_MAX_PALETTE RGBA8 entries as uint32 (r in the low byte) or as rows (r, g, b, a); the style keeps the array alive."""
        st = abi.OverlayStyle()
        self.check(self.lib.svr_overlay_style_default(C.byref(st)))
        if fill_alpha is not None:
            st.fill_alpha = int(fill_alpha)
        if edge_alpha is not None:
            st.edge_alpha = int(edge_alpha)
        if palette is not None:
            pal = np.asarray(palette)
            if pal.ndim == 2:
                pal = np.ascontiguousarray(pal, dtype=np.uint8).view("<u4").reshape(-1)
            st._palette = np.ascontiguousarray(pal, dtype=np.uint32)
            st.palette = st._palette.ctypes.data_as(C.POINTER(C.c_uint32))
            st.palette_count = len(st._palette)
        return st

    def overlay_palette_default(self, n: int = abi.OVERLAY_DEFAULT_PALETTE) -> np.ndarray:
        out = np.zeros(int(n), dtype=np.uint32)
        self.check(self.lib.svr_overlay_palette_default(out.ctypes.data_as(C.POINTER(C.c_uint32)), int(n)))
        return out

    @staticmethod
    def _overlay_source(mask: Optional[int], labels: Optional[int]) -> abi.OverlaySource:
        return abi.OverlaySource(C.c_void_p(int(mask)) if mask else None, C.c_void_p(int(labels)) if labels else None)

    def slice_ids(self, ids: int, volume: cudaVolume, shape, w: int, h: int, params: abi.SliceParams, mask: Optional[int] = None,
                  labels: Optional[int] = None, count: int = 1, spacing: float = 0.0):
        """svr_slice_ids: the region id of every owned pixel of `count` slices into the device buffer ids (count x h x w uint32).  mask /
        labels: the device pointer of a bit mask or of a uint32 label array of the (nz, ny, nx) = shape volume; exactly one is given."""
        nz, ny, nx = (int(n) for n in shape)
        src = self._overlay_source(mask, labels)
        self.check(self.lib.svr_slice_ids(C.c_void_p(int(ids)), C.byref(volume), nx, ny, nz, int(w), int(h), C.byref(params), int(count),
                                          C.c_float(float(spacing)), C.byref(src)))

    def hit_ids(self, ids: int, hits: int, w: int, h: int, volume: cudaVolume, shape, mask: Optional[int] = None, labels: Optional[int] = None):
        """svr_hit_ids: the region id of every record of a full w x h hit map (svr_render_hits) into the device buffer ids."""
        nz, ny, nx = (int(n) for n in shape)
        src = self._overlay_source(mask, labels)
        self.check(self.lib.svr_hit_ids(C.c_void_p(int(ids)), C.c_void_p(int(hits)), int(w), int(h), C.byref(volume), nx, ny, nz, C.byref(src)))

    def overlay_ids(self, imgs: int, ids: int, w: int, h: int, count: int = 1, style: Optional[abi.OverlayStyle] = None):
        """svr_overlay_ids: tints `count` RGBA8 images of w x h in place by their id images: fill inside a part, outline at its edge."""
        st = style if style is not None else self.overlay_style()
        self.check(self.lib.svr_overlay_ids(C.c_void_p(int(imgs)), C.c_void_p(int(ids)), int(w), int(h), int(count), C.byref(st)))

    def overlay_slice(self, imgs: int, volume: cudaVolume, shape, w: int, h: int, params: abi.SliceParams, mask: Optional[int] = None,
                      labels: Optional[int] = None, style: Optional[abi.OverlayStyle] = None, count: int = 1, spacing: float = 0.0):
        """svr_overlay_slice: slice_ids followed by overlay_ids in one kernel, over the owned pixels of the slice images at imgs."""
        nz, ny, nx = (int(n) for n in shape)
        src = self._overlay_source(mask, labels)
        st = style if style is not None else self.overlay_style()
        self.check(self.lib.svr_overlay_slice(C.c_void_p(int(imgs)), C.byref(volume), nx, ny, nz, int(w), int(h), C.byref(params), int(count),
                                              C.c_float(float(spacing)), C.byref(src), C.byref(st)))

    def overlay_last_ms(self) -> float:
        ms = C.c_float(0.0)
        self.check(self.lib.svr_overlay_last_ms(C.byref(ms)))
        return float(ms.value)

    # ---- surface meshes by surface nets (svr_mesh_isosurface / _region / _measure / _positions) ----
    def mesh_params(self, level: Optional[int] = None, relax: int = 0) -> abi.MeshParams:
        p = abi.MeshParams()
        self.check(self.lib.svr_mesh_params_default(C.byref(p)))
        if level is not None:
            p.level = int(level)
        p.relax = int(relax)
        return p

    def _mesh_extract(self, call):
        """A counting call, then an extraction call into buffers of the counted size.  call(vertices pointer, vertex capacity, triangles
        pointer, triangle capacity, info) runs the C function.  Returns (vertices int32 [nv, 3], triangles uint32 [nt, 3], info)."""
        info = abi.MeshInfo()
        self.check(call(None, 0, None, 0, info))
        nv, nt = int(info.vertices), int(info.triangles)
        if nv == 0:
            return np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32), info
        buf = self.malloc(12 * (nv + max(nt, 1)))
        try:
            self.check(call(C.c_void_p(buf), nv, C.c_void_p(buf + 12 * nv), nt, info))
            return self.to_host(buf, (nv, 3), np.int32), self.to_host(buf + 12 * nv, (nt, 3), np.uint32), info
        finally:
            self.free(buf)

    def mesh_isosurface(self, vox, level: int, relax: int = 0, shape=None):
        """svr_mesh_isosurface: the surface-nets mesh of {v >= level} of a host [nz][ny][nx] u16 array or a device pointer with
        shape=(nz, ny, nx), after `relax` constrained relaxation steps.  Returns (vertices, triangles, info): int32 [nv, 3] in units of
        1/256 voxel on the padded grid (sample x sits at 256 (x + 1)), uint32 [nt, 3], and the svr_mesh_info."""
        src, (nz, ny, nx), on_dev, _keep = self._region_source(vox, shape)
        p = self.mesh_params(level, relax)
        return self._mesh_extract(lambda v, nv, t, nt, info: self.lib.svr_mesh_isosurface(src, nx, ny, nz, on_dev, C.byref(p), v, nv, t, nt, C.byref(info)))

    def mesh_region(self, mask, relax: int = 0, shape=None):
        """svr_mesh_region: the same for a region mask (a bool array [nz][ny][nx], or a device pointer to the bit mask with shape=)."""
        if isinstance(mask, np.ndarray):
            shape = mask.shape
        if shape is None:
            raise ValueError("a device mask needs shape=(nz, ny, nx)")
        nz, ny, nx = (int(n) for n in shape)
        buf, owned = self._region_mask(mask, (nz, ny, nx))
        p = self.mesh_params(None, relax)
        try:
            return self._mesh_extract(lambda v, nv, t, nt, info: self.lib.svr_mesh_region(C.c_void_p(buf), nx, ny, nz, C.byref(p), v, nv, t, nt, C.byref(info)))
        finally:
            if owned:
                self.free(buf)

    def mesh_measure(self, vertices, triangles, scale=(1.0 / 256, 1.0 / 256, 1.0 / 256)):
        """svr_mesh_measure of host arrays (uploaded): (volume6, area) -- the exact integer 6 * 256^3 * (enclosed volume in voxels) and the
        surface area under the per-axis scale (spacing / 256)."""
        v = np.ascontiguousarray(vertices, dtype=np.int32).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        s = (C.c_double * 3)(*[float(x) for x in scale])
        vol, area = C.c_int64(0), C.c_double(0.0)
        buf = self.malloc(max(v.nbytes, 4) + max(t.nbytes, 4))
        try:
            if len(v):
                self.to_device(buf, v)
            if len(t):
                self.to_device(buf + max(v.nbytes, 4), t)
            self.check(self.lib.svr_mesh_measure(C.c_void_p(buf), len(v), C.c_void_p(buf + max(v.nbytes, 4)), len(t), s, C.byref(vol), C.byref(area)))
        finally:
            self.free(buf)
        return int(vol.value), float(area.value)

    def mesh_positions(self, vertices, spacing=(1.0, 1.0, 1.0), volume: Optional[cudaVolume] = None) -> np.ndarray:
        return mesh_positions(self.lib, vertices, spacing, volume)

    def mesh_last_ms(self):
        """(classify, emit, relax) HIP-event milliseconds of the last mesh call"""
        ms = [C.c_float(0.0) for _ in range(3)]
        self.check(self.lib.svr_mesh_last_ms(*[C.byref(m) for m in ms]))
        return tuple(float(m.value) for m in ms)

    # ---- exact volume filters (svr_volume_*): median / min / max and binomial smoothing of the raw voxels ----
    def volume_rank(self, vox, op: int, element: int = 6, iterations: int = 1, shape=None, out_ptr: Optional[int] = None):
        """svr_volume_rank: the median (FILTER_MEDIAN), minimum (FILTER_MIN) or maximum (FILTER_MAX) of every voxel's window under the
        unit element 6 / 18 / 26 with a replicated border, applied `iterations` times.  vox is a host [nz][ny][nx] u16 array, or a device
        pointer with shape=(nz, ny, nx).  Returns a u16 array [nz][ny][nx]; with out_ptr (a device buffer of nx * ny * nz u16 that does
        not overlap a device `vox`) the result stays on the device and out_ptr is returned."""
        src, (nz, ny, nx), on_dev, _keep = self._region_source(vox, shape)
        return self._volume_filter((nz, ny, nx), out_ptr, lambda out: self.lib.svr_volume_rank(
            src, nx, ny, nz, on_dev, int(op), int(element), int(iterations), C.c_void_p(out)))

    def volume_median(self, vox, element: int = 6, iterations: int = 1, shape=None, out_ptr: Optional[int] = None):
        """volume_rank with FILTER_MEDIAN."""
        return self.volume_rank(vox, abi.FILTER_MEDIAN, element, iterations, shape, out_ptr)

    def volume_smooth(self, vox, radii, shape=None, out_ptr: Optional[int] = None):
        """svr_volume_smooth: separable binomial smoothing with the per-axis radii (rx, ry, rz), each 0 .. SMOOTH_MAX_RADIUS, one
        rounding per axis, a replicated border.  vox, the return value and out_ptr as in volume_rank."""
        src, (nz, ny, nx), on_dev, _keep = self._region_source(vox, shape)
        r = (C.c_uint32 * 3)(*[int(t) for t in radii])
        return self._volume_filter((nz, ny, nx), out_ptr, lambda out: self.lib.svr_volume_smooth(src, nx, ny, nz, on_dev, r, C.c_void_p(out)))

    def _volume_filter(self, shape, out_ptr, call):
        nz, ny, nx = shape
        out = out_ptr if out_ptr is not None else self.malloc(2 * max(nx * ny * nz, 1))
        try:
            self.check(call(out))
            self.synchronize()
            if out_ptr is not None:
                return out_ptr
            return self.to_host(out, (nz, ny, nx), np.uint16)
        finally:
            if out_ptr is None:
                self.free(out)

    def volume_filter_last_ms(self) -> float:
        """HIP-event time of the device work of the last volume_rank / volume_smooth call."""
        ms = C.c_float(0.0)
        self.check(self.lib.svr_volume_filter_last_ms(C.byref(ms)))
        return float(ms.value)

    # ---- crop and resample (svr_resample_grid_* / svr_volume_resample / svr_region_resample / _label_resample / _paste / _mask_expand) ----
    def resample_grid_box(self, shape, box) -> abi.ResampleGrid:
        return resample_grid_box(shape, box, self.lib)

    def resample_grid_spacing(self, shape, src_spacing, target_spacing, box=None):
        return resample_grid_spacing(shape, src_spacing, target_spacing, box, self.lib)

    def resample_grid_dims(self, shape, out_shape, box=None) -> abi.ResampleGrid:
        return resample_grid_dims(shape, out_shape, box, self.lib)

    def resample_grid_place(self, volume: cudaVolume, shape, grid) -> cudaVolume:
        return resample_grid_place(volume, shape, grid, self.lib)

    def volume_resample(self, vox, grid, mode: int = abi.RESAMPLE_AUTO, shape=None, out_ptr: Optional[int] = None):
        """svr_volume_resample: the volume on `grid` (a ResampleGrid, or ((origin, step, count) of x, y, z)) under RESAMPLE_NEAREST /
        _LINEAR / _AREA / _AUTO.  vox is a host [nz][ny][nx] u16 array, or a device pointer with shape=(nz, ny, nx).  Returns a u16 array
        of grid.shape; with out_ptr (a device buffer of that many u16 that does not overlap a device `vox`) the result stays on the
        device and out_ptr is returned."""
        src, (nz, ny, nx), on_dev, _keep = self._region_source(vox, shape)
        g, dims = resample_grid(grid), (C.c_int32 * 3)(nx, ny, nz)
        return self._volume_filter(g.shape, out_ptr, lambda out: self.lib.svr_volume_resample(src, dims, on_dev, C.byref(g), int(mode), C.c_void_p(out)))

    def volume_crop(self, vox, box, shape=None, out_ptr: Optional[int] = None):
        """volume_resample on the grid of a box ((x0, y0, z0), (x1, y1, z1)), inclusive, cut to the volume.  Returns (result, grid)."""
        shape = vox.shape if isinstance(vox, np.ndarray) else shape
        g = self.resample_grid_box(shape, box)
        return self.volume_resample(vox, g, abi.RESAMPLE_NEAREST, shape, out_ptr), g

    def region_resample(self, mask, grid, shape=None, out_ptr: Optional[int] = None) -> np.ndarray:
        """svr_region_resample: NEAREST on a mask (a bool array [nz][ny][nx], or a device pointer with shape=).  Returns the bool array of
        grid.shape; out_ptr: a device buffer of region_mask_words(grid.shape) uint32 that receives the bit mask."""
        if isinstance(mask, np.ndarray):
            shape = mask.shape
        if shape is None:
            raise ValueError("a device mask needs shape=(nz, ny, nx)")
        nz, ny, nx = (int(n) for n in shape)
        g, dims = resample_grid(grid), (C.c_int32 * 3)(nx, ny, nz)
        buf, owned = self._region_mask(mask, (nz, ny, nx))
        words = region_mask_words(g.shape)
        out = out_ptr if out_ptr is not None else self.malloc(4 * max(words, 1))
        try:
            self.check(self.lib.svr_region_resample(C.c_void_p(buf), dims, C.byref(g), C.c_void_p(out)))
            return region_mask_unpack(self.to_host(out, (words,), np.uint32), g.shape)
        finally:
            if owned:
                self.free(buf)
            if out_ptr is None:
                self.free(out)

    def region_label_resample(self, labels, grid, shape=None, out_ptr: Optional[int] = None):
        """svr_region_label_resample: NEAREST on a uint32 map (labels, zones; a squared-distance map only for crops).  Returns the uint32
        array of grid.shape, or out_ptr itself when a device buffer of that many uint32 is given."""
        buf, (nz, ny, nx), owned = self._region_labels(labels, shape)
        g, dims = resample_grid(grid), (C.c_int32 * 3)(nx, ny, nz)
        out = out_ptr if out_ptr is not None else self.malloc(4 * max(int(np.prod(g.shape)), 1))
        try:
            self.check(self.lib.svr_region_label_resample(C.c_void_p(buf), dims, C.byref(g), C.c_void_p(out)))
            if out_ptr is not None:
                self.synchronize()
                return out_ptr
            return self.to_host(out, g.shape, np.uint32)
        finally:
            if owned:
                self.free(buf)
            if out_ptr is None:
                self.free(out)

    def region_paste(self, sub, full, offset, op: int = abi.PASTE_REPLACE, sub_shape=None, full_shape=None):
        """svr_region_paste: the sub-mask put back at offset (x, y, z) of the full mask with PASTE_REPLACE, MASK_OR or MASK_ANDNOT.  Masks
        are bool arrays, or device pointers with their shapes.  A device `full` is changed in place and returned; a host `full` is left
        alone and the pasted bool array is returned."""
        sub_shape = sub.shape if isinstance(sub, np.ndarray) else tuple(int(n) for n in sub_shape)
        full_shape = full.shape if isinstance(full, np.ndarray) else tuple(int(n) for n in full_shape)
        sbuf, sowned = self._region_mask(sub, sub_shape)
        fbuf, fowned = self._region_mask(full, full_shape)
        try:
            self.check(self.lib.svr_region_paste(C.c_void_p(sbuf), (C.c_int32 * 3)(*sub_shape[::-1]), C.c_void_p(fbuf), (C.c_int32 * 3)(*full_shape[::-1]),
                                                 (C.c_int32 * 3)(*[int(t) for t in offset]), int(op)))
            if not fowned:
                self.synchronize()
                return full
            return region_mask_unpack(self.to_host(fbuf, (region_mask_words(full_shape),), np.uint32), full_shape)
        finally:
            if sowned:
                self.free(sbuf)
            if fowned:
                self.free(fbuf)

    def region_mask_expand(self, mask, value: int = 1, shape=None, out_ptr: Optional[int] = None):
        """svr_region_mask_expand: one byte per voxel, `value` (1 .. 255) inside the mask and 0 outside -- what io.mhd_write saves a mask
        from.  Returns the u8 array [nz][ny][nx], or out_ptr itself when a device buffer of nx * ny * nz bytes is given."""
        if isinstance(mask, np.ndarray):
            shape = mask.shape
        if shape is None:
            raise ValueError("a device mask needs shape=(nz, ny, nx)")
        nz, ny, nx = (int(n) for n in shape)
        buf, owned = self._region_mask(mask, (nz, ny, nx))
        out = out_ptr if out_ptr is not None else self.malloc(max(nx * ny * nz, 4))
        try:
            self.check(self.lib.svr_region_mask_expand(C.c_void_p(buf), (C.c_int32 * 3)(nx, ny, nz), int(value), C.c_void_p(out)))
            if out_ptr is not None:
                self.synchronize()
                return out_ptr
            return self.to_host(out, (nz, ny, nx), np.uint8)
        finally:
            if owned:
                self.free(buf)
            if out_ptr is None:
                self.free(out)

    def volume_resample_last_ms(self) -> float:
        """HIP-event time of the device work of the last volume_resample / region_resample / _label_resample / _paste / _mask_expand."""
        ms = C.c_float(0.0)
        self.check(self.lib.svr_volume_resample_last_ms(C.byref(ms)))
        return float(ms.value)

    def region_measure(self, stats: abi.RegionStats, spacing=(1.0, 1.0, 1.0)) -> abi.RegionMeasurement:
        """svr_region_measure: volume, mean, standard deviation, centroid (voxel indices) and surface area from the integer statistics."""
        m = abi.RegionMeasurement()
        sp = (C.c_double * 3)(*[float(t) for t in spacing])
        self.check(self.lib.svr_region_measure(C.byref(stats), sp, C.byref(m)))
        return m


# svr_region_component as a numpy record (40 bytes); LABEL_SCAN_BLOCK mirrors SVR_LABEL_SCAN_BLOCK of csrc/svr_label.hip
COMPONENT_DTYPE = np.dtype([("voxels", "<u4"), ("first", "<u4"), ("bbox_min", "<i4", (3,)), ("bbox_max", "<i4", (3,)), ("sum", "<u8")])
assert COMPONENT_DTYPE.itemsize == 40
LABEL_SCAN_BLOCK = abi.LABEL_SCAN_BLOCK


def region_label_scan_levels(shape) -> int:
    """The levels of svr_region_label's renumbering scan for a [nz][ny][nx] volume: 1 while one block covers the mask words, 2 up to
    a block of blocks, and so on."""
    n, levels = region_mask_words(shape), 1
    while n > LABEL_SCAN_BLOCK:
        n, levels = (n + LABEL_SCAN_BLOCK - 1) // LABEL_SCAN_BLOCK, levels + 1
    return levels


def mesh_positions(lib, vertices, spacing=(1.0, 1.0, 1.0), volume=None) -> np.ndarray:
    """svr_mesh_positions: float32 [nv, 3] positions of mesh vertices (int32 [nv, 3], 1/256 voxel on the padded grid) -- millimetres,
    (u / 256 - 0.5) * spacing, or with `volume` (a cudaVolume) the world coordinates of the sampler's mapping.  Host code of the library:
    no device is needed."""
    lib = lib if lib is not None else abi.load()
    v = np.ascontiguousarray(vertices, dtype=np.int32).reshape(-1, 3)
    out = np.zeros((len(v), 3), dtype=np.float32)
    sp = (C.c_double * 3)(*[float(t) for t in spacing])
    rc = lib.svr_mesh_positions(v.ctypes.data_as(C.c_void_p), len(v), sp, C.byref(volume) if volume is not None else None, out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        msg = lib.svr_last_error().decode()
        lib.svr_clear_error()
        raise SvrError(f"svr_mesh_positions failed ({rc}): {msg}")
    return out


def distance_weights(spacing, shape, lib=None):
    """svr_region_distance_weights: ((wx, wy, wz), unit) for a spacing (sx, sy, sz) and a [nz][ny][nx] shape: the integer weights of the
    squared distance in units of `unit` = min(spacing) / 2^k.  A length L is r2 = floor((L / unit)^2); a map value d2 means sqrt(d2) unit.
    Host code of the library: no device is needed."""
    lib = lib if lib is not None else abi.load()
    nz, ny, nx = (int(n) for n in shape)
    sp = (C.c_double * 3)(*[float(t) for t in spacing])
    w, unit = (C.c_uint32 * 3)(), C.c_double(0.0)
    rc = lib.svr_region_distance_weights(sp, nx, ny, nz, w, C.byref(unit))
    if rc != 0:
        msg = lib.svr_last_error().decode()
        lib.svr_clear_error()
        raise SvrError(f"svr_region_distance_weights failed ({rc}): {msg}")
    return (int(w[0]), int(w[1]), int(w[2])), float(unit.value)


def geodesic_weights(spacing, connectivity, shape, lib=None):
    """svr_region_geodesic_weights: ((w_x, w_y, w_z, w_xy, w_xz, w_yz, w_xyz), unit) for a spacing (sx, sy, sz), a connectivity 6 / 18 / 26
    and a [nz][ny][nx] shape: the Euclidean lengths of the moves in units of `unit` = min(spacing) / 2^k, rounded, 0 for the classes
    beyond the connectivity.  A geodesic map value d means about d unit.  Host code of the library: no device is needed."""
    lib = lib if lib is not None else abi.load()
    nz, ny, nx = (int(n) for n in shape)
    sp = (C.c_double * 3)(*[float(t) for t in spacing])
    w, unit = (C.c_uint32 * 7)(), C.c_double(0.0)
    rc = lib.svr_region_geodesic_weights(sp, int(connectivity), nx, ny, nz, w, C.byref(unit))
    if rc != 0:
        msg = lib.svr_last_error().decode()
        lib.svr_clear_error()
        raise SvrError(f"svr_region_geodesic_weights failed ({rc}): {msg}")
    return tuple(int(t) for t in w), float(unit.value)


def smooth_radii(spacing, sigma, lib=None):
    """svr_volume_smooth_radii: ((rx, ry, rz), (sx, sy, sz)) for a spacing and a sigma in the spacing's units: the binomial radii
    llround(2 (sigma / spacing[a])^2) and the sigma each one applies, sqrt(r / 2) spacing[a].  Host code of the library: no device is
    needed."""
    lib = lib if lib is not None else abi.load()
    sp = (C.c_double * 3)(*[float(t) for t in spacing])
    r, so = (C.c_uint32 * 3)(), (C.c_double * 3)()
    rc = lib.svr_volume_smooth_radii(sp, float(sigma), r, so)
    if rc != 0:
        msg = lib.svr_last_error().decode()
        lib.svr_clear_error()
        raise SvrError(f"svr_volume_smooth_radii failed ({rc}): {msg}")
    return (int(r[0]), int(r[1]), int(r[2])), (float(so[0]), float(so[1]), float(so[2]))


def _histogram_call(lib, name, rc):
    """Raises on an error code; returns True when the histogram was empty (SVR_HISTOGRAM_STATUS_EMPTY)."""
    if rc not in (0, abi.HISTOGRAM_STATUS_EMPTY):
        msg = lib.svr_last_error().decode("utf-8", "replace")
        lib.svr_clear_error()
        raise SvrError(f"{name} failed ({rc}): {msg}")
    return rc == abi.HISTOGRAM_STATUS_EMPTY


def _histogram_counts(counts):
    c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    return c, c.ctypes.data_as(C.c_void_p) if len(c) else None


def histogram_params(lo: int = 0, hi: int = 65535, shift: int = 0, box=None, lib=None) -> abi.HistogramParams:
    """svr_histogram_params_default with the window, shift and box ((x0, y0, z0), (x1, y1, z1), inclusive) replaced.  The histogram
    helpers below are host code of the library: no device is needed."""
    lib = lib if lib is not None else abi.load()
    p = abi.HistogramParams()
    _histogram_call(lib, "svr_histogram_params_default", lib.svr_histogram_params_default(C.byref(p)))
    p.lo, p.hi, p.shift = int(lo), int(hi), int(shift)
    if box is not None:
        for a in range(3):
            p.box_min[a], p.box_max[a] = int(box[0][a]), int(box[1][a])
    return p


def histogram_bins(lo: int = 0, hi: int = 65535, shift: int = 0, lib=None) -> int:
    """svr_histogram_bins: ((hi - lo) >> shift) + 1, or 0 for an invalid window or shift."""
    lib = lib if lib is not None else abi.load()
    p = histogram_params(lo, hi, shift, None, lib)
    return int(lib.svr_histogram_bins(C.byref(p)))


def histogram_bin_range(bin: int, lo: int = 0, hi: int = 65535, shift: int = 0, lib=None):
    """svr_histogram_bin_range: (v_lo, v_hi), the raw values of a bin -- the window for region_threshold."""
    lib = lib if lib is not None else abi.load()
    p = histogram_params(lo, hi, shift, None, lib)
    a, b = C.c_uint32(0), C.c_uint32(0)
    _histogram_call(lib, "svr_histogram_bin_range", lib.svr_histogram_bin_range(C.byref(p), int(bin), C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def histogram_moments(counts, lib=None):
    """svr_histogram_moments: (n, sum, sum_sq) of the bin indices of a uint32 histogram; (0, 0, 0) when it is empty."""
    lib = lib if lib is not None else abi.load()
    c, ptr = _histogram_counts(counts)
    n, s, q = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _histogram_call(lib, "svr_histogram_moments", lib.svr_histogram_moments(ptr, len(c), C.byref(n), C.byref(s), C.byref(q)))
    return int(n.value), int(s.value), int(q.value)


def histogram_quantile(counts, num: int, den: int, lib=None):
    """svr_histogram_quantile: the smallest bin b with C(b) > 0 and den * C(b) >= num * N (numpy's inverted_cdf for 0 < num / den <= 1;
    num = 0: the first occupied bin); None when the histogram is empty."""
    lib = lib if lib is not None else abi.load()
    c, ptr = _histogram_counts(counts)
    b = C.c_uint32(0)
    empty = _histogram_call(lib, "svr_histogram_quantile", lib.svr_histogram_quantile(ptr, len(c), int(num), int(den), C.byref(b)))
    return None if empty else int(b.value)


def histogram_otsu(counts, classes: int = 2, lib=None):
    """svr_histogram_otsu: (thresholds, eta): the classes - 1 exact Otsu thresholds (the last bins of the lower classes; ties go to the
    lexicographically smallest tuple) and between-class / total variance; (None, 0.0) when the histogram is empty."""
    lib = lib if lib is not None else abi.load()
    c, ptr = _histogram_counts(counts)
    t, eta = (C.c_uint32 * 2)(), C.c_double(0.0)
    empty = _histogram_call(lib, "svr_histogram_otsu", lib.svr_histogram_otsu(ptr, len(c), int(classes), t, C.byref(eta)))
    if empty:
        return None, 0.0
    return tuple(int(t[k]) for k in range(int(classes) - 1)), float(eta.value)


def resample_grid(grid) -> abi.ResampleGrid:
    """A ResampleGrid from ((origin, step, count) of x, of y, of z); a ResampleGrid is returned as it is."""
    if isinstance(grid, abi.ResampleGrid):
        return grid
    g = abi.ResampleGrid()
    for a in range(3):
        g.axis[a].origin, g.axis[a].step, g.axis[a].count = (int(t) for t in grid[a])
    return g


def _grid_call(lib, name, rc):
    if rc != 0:
        msg = lib.svr_last_error().decode("utf-8", "replace")
        lib.svr_clear_error()
        raise SvrError(f"{name} failed ({rc}): {msg}")


def _grid_box_args(shape, box):
    nz, ny, nx = (int(n) for n in shape)
    b0 = b1 = None
    if box is not None:
        b0, b1 = (C.c_int32 * 3)(*[int(t) for t in box[0]]), (C.c_int32 * 3)(*[int(t) for t in box[1]])
    return (C.c_int32 * 3)(nx, ny, nz), b0, b1


def resample_grid_box(shape, box, lib=None) -> abi.ResampleGrid:
    """svr_resample_grid_box: the grid of a crop of a [nz][ny][nx] volume to box = ((x0, y0, z0), (x1, y1, z1)), inclusive, cut to the
    volume.  The grid helpers are host code of the library: no device is needed."""
    lib = lib if lib is not None else abi.load()
    dims, b0, b1 = _grid_box_args(shape, box)
    g = abi.ResampleGrid()
    _grid_call(lib, "svr_resample_grid_box", lib.svr_resample_grid_box(dims, b0, b1, C.byref(g)))
    return g


def resample_grid_spacing(shape, src_spacing, target_spacing, box=None, lib=None):
    """svr_resample_grid_spacing: (grid, spacing applied) for resampling a [nz][ny][nx] volume (or a box of it) from src_spacing to
    target_spacing, both (x, y, z); a scalar target means isotropic."""
    lib = lib if lib is not None else abi.load()
    dims, b0, b1 = _grid_box_args(shape, box)
    target = [float(target_spacing)] * 3 if np.isscalar(target_spacing) else [float(t) for t in target_spacing]
    g, out = abi.ResampleGrid(), (C.c_double * 3)()
    _grid_call(lib, "svr_resample_grid_spacing", lib.svr_resample_grid_spacing(dims, (C.c_double * 3)(*[float(t) for t in src_spacing]), b0, b1,
                                                                                (C.c_double * 3)(*target), C.byref(g), out))
    return g, (float(out[0]), float(out[1]), float(out[2]))


def resample_grid_dims(shape, out_shape, box=None, lib=None) -> abi.ResampleGrid:
    """svr_resample_grid_dims: the grid that maps a [nz][ny][nx] volume (or a box of it) onto out_shape = (nz', ny', nx')."""
    lib = lib if lib is not None else abi.load()
    dims, b0, b1 = _grid_box_args(shape, box)
    g = abi.ResampleGrid()
    _grid_call(lib, "svr_resample_grid_dims", lib.svr_resample_grid_dims(dims, b0, b1, (C.c_int32 * 3)(*[int(n) for n in out_shape][::-1]), C.byref(g)))
    return g


def resample_grid_place(volume: cudaVolume, shape, grid, lib=None) -> cudaVolume:
    """svr_resample_grid_place: a copy of `volume` (the cudaVolume of the [nz][ny][nx] source) whose box and spacing are those of the
    resampled volume, where it lay inside the source's box.  tex is copied: the caller replaces it."""
    lib = lib if lib is not None else abi.load()
    dims, _, _ = _grid_box_args(shape, None)
    g, out = resample_grid(grid), cudaVolume()
    _grid_call(lib, "svr_resample_grid_place", lib.svr_resample_grid_place(C.byref(volume), dims, C.byref(g), C.byref(out)))
    return out


def region_mask_words(shape) -> int:
    """svr_region_mask_words of a [nz][ny][nx] volume."""
    nz, ny, nx = shape
    return ((nx + 31) // 32) * ny * nz


def region_mask_unpack(words: np.ndarray, shape) -> np.ndarray:
    """The bit mask of svr_region_grow (uint32 words) as a bool array [nz][ny][nx]."""
    nz, ny, nx = shape
    wx = (nx + 31) // 32
    b = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8).reshape(nz, ny, wx * 4), axis=-1, bitorder="little")
    return b[:, :, :nx].astype(bool)


def region_mask_pack(mask: np.ndarray) -> np.ndarray:
    """A bool array [nz][ny][nx] as the bit mask of the region calls: uint32 words, padding bits 0."""
    nz, ny, nx = mask.shape
    wx = (nx + 31) // 32
    padded = np.zeros((nz, ny, wx * 32), dtype=np.uint8)
    padded[:, :, :nx] = mask
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32))


def region_seed_from_world(lib, volume: cudaVolume, dim, point):
    """svr_region_seed_from_world: the voxel (x, y, z) whose cell contains a world point (e.g. a svr_hit position); dim = (nx, ny, nz).
    Host code of the library: no device is needed."""
    ijk = (C.c_int32 * 3)()
    pt = _to_vec3(point)
    if lib.svr_region_seed_from_world(C.byref(volume), int(dim[0]), int(dim[1]), int(dim[2]), C.byref(pt), ijk) != 0:
        msg = lib.svr_last_error().decode("utf-8", "replace")
        lib.svr_clear_error()
        raise SvrError(msg)
    return (int(ijk[0]), int(ijk[1]), int(ijk[2]))


def slice_params_axis(lib, volume: cudaVolume, axis: int, position: float, w: int, h: int) -> abi.SliceParams:
    """svr_slice_params_axis: the plane perpendicular to world axis 0 / 1 / 2 at `position` in [0, 1] across the clipped box of
    `volume`, fitted to w x h pixels.  Host code of the library: no device is needed."""
    p = abi.SliceParams()
    if lib.svr_slice_params_axis(C.byref(p), C.byref(volume), int(axis), C.c_float(float(position)), int(w), int(h)) != 0:
        msg = lib.svr_last_error().decode("utf-8", "replace")
        lib.svr_clear_error()
        raise SvrError(f"svr_slice_params_axis: {msg}")
    return p


def slice_params_through(lib, volume: cudaVolume, axis: int, point, w: int, h: int) -> abi.SliceParams:
    """svr_slice_params_through: the axis plane of slice_params_axis through the world point `point` (a picked position).  Host code
    of the library: no device is needed."""
    p = abi.SliceParams()
    q = _to_vec3(point)
    if lib.svr_slice_params_through(C.byref(p), C.byref(volume), int(axis), C.byref(q), int(w), int(h)) != 0:
        msg = lib.svr_last_error().decode("utf-8", "replace")
        lib.svr_clear_error()
        raise SvrError(f"svr_slice_params_through: {msg}")
    return p


# numpy view of svr_hit records (40 bytes, 4-byte members)
HIT_DTYPE = np.dtype([("status", np.int32), ("sample", np.int32), ("t", np.float32), ("value", np.float32),
                      ("position", np.float32, 3), ("normal", np.float32, 3)])
assert HIT_DTYPE.itemsize == C.sizeof(abi.Hit)


def _slice_params(params, thickness, step, mode, window, color_tf) -> abi.SliceParams:
    p = abi.SliceParams.from_buffer_copy(params)
    if thickness is not None:
        p.thickness = float(thickness)
    if step is not None:
        p.step = float(step)
    if mode is not None:
        p.mode = int(mode)
    if window is not None:
        p.window_lo, p.window_hi = float(window[0]), float(window[1])
    if color_tf is not None:
        p.flags = (p.flags & ~abi.SLICE_COLOR_TF) | (abi.SLICE_COLOR_TF if color_tf else 0)
    return p


class Canvas:
    """Headless replay of the reference's Qt `Canvas` render protocol (gui/canvas.{h,cpp}).

    Owns RenderParams / cudaCamera / cudaVolume / cudaTransferFunction / lights exactly like the
    widget does; every setter re-uploads through the matching setup_* and restarts the progressive
    render (frameNo = 0, gui/canvas.h:43-47); paint() is paintGL's render branch
    (gui/canvas.cpp:90-116): render_*, then frameNo++.
    """

    RENDER_MODE_PATHTRACER, RENDER_MODE_RAYCASTING = 0, 1

    def __init__(self, dev: Device, width: int, height: int, img_ptr: Optional[int] = None,
                 hdr_ptr: Optional[int] = None):
        self.dev, self.lib = dev, dev.lib
        self.W, self.H = int(width), int(height)
        # Canvas::Canvas, gui/canvas.cpp:8-20
        self.env = env_light_constant((1.0, 1.0, 1.0), 0.5)
        self.lib.setup_env_lights(C.byref(self.env)); dev.check()
        self.renderParams = RenderParams(1, 0, None)
        self._own_hdr = hdr_ptr is None
        if hdr_ptr is None:
            dev.check(self.lib.svr_render_params_setup_hdr(C.byref(self.renderParams), self.W, self.H))
        else:
            self.renderParams.hdrBuffer = C.c_void_p(hdr_ptr)
        self._own_img = img_ptr is None
        self.img = dev.malloc(self.W * self.H * 4) if img_ptr is None else int(img_ptr)
        self.renderParams.traceDepth = 1
        self.deviceVolume = cudaVolume()
        self.deviceVolume.gradientFactor = 0.5
        self.transferFunction = cudaTransferFunction()
        self.camera = cudaCamera()
        self.areaLights: list = []
        self.renderMode = self.RENDER_MODE_PATHTRACER
        self.stepSize = 1.0
        self.fov, self.apeture, self.focalLength, self.exposure = 45.0, 0.0, 1.0, 1.0
        self.ready = False
        self._textures: list = []

    # ---- gui/canvas.h:43-47 ----
    def ReStartRender(self):
        self.renderParams.frameNo = 0

    # ---- Canvas::LoadVolume, gui/canvas.cpp:27-41 (the file reader is replaced by an array) ----
    def LoadVolume(self, voxels: np.ndarray, spacing, max_magnitude: float, layout: int = abi.LAYOUT_AUTO):
        vox = np.ascontiguousarray(voxels, dtype=np.uint16)
        nz, ny, nx = vox.shape
        h = self.lib.svr_create_volume_texture(vox.ctypes.data_as(C.c_void_p), nx, ny, nz, 0, int(layout))
        self.dev.check()
        old = getattr(self, "_volume_tex", 0)
        if old and old in self._textures:                      # a second LoadVolume replaces the texture: free the old one now
            self._textures.remove(old)
            self.lib.svr_destroy_texture(old)
        self._volume_tex = h
        self._textures.append(h)
        gf = self.deviceVolume.gradientFactor
        self.deviceVolume = create_device_volume(h, (nx, ny, nz), spacing, max_magnitude)
        self.deviceVolume.gradientFactor = gf
        self.lib.setup_volume(C.byref(self.deviceVolume)); self.dev.check()
        self.stepSize = element_bounding_sphere_radius(spacing)
        self.volumeSize = volume_size((nx, ny, nz), spacing)
        self.volumeDim = (nx, ny, nz)
        self.boundingSphereRadius = bounding_sphere_radius((nx, ny, nz), spacing)
        eye = zoom_to_extent_eye_dist(self.volumeSize, self.fov)
        self.eyeDist = eye
        self.camera = camera_setup((0.0, 0.0, eye), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), self.fov, self.apeture,
                                   self.focalLength, self.exposure, self.W, self.H)
        self.lib.setup_camera(C.byref(self.camera)); self.dev.check()
        self.ready = True
        self.ReStartRender()

    def LoadVolumeFile(self, filename: str, layout: int = abi.LAYOUT_AUTO):
        """Canvas::LoadVolume(filename), gui/canvas.cpp:27-41, with the reference's reader replaced by
        io.VolumeReader (MetaImage parse on the host, preprocessing on the GPU)."""
        from .io import VolumeReader
        if getattr(self, "volumeReader", None) is not None:
            self.volumeReader.ClearDevice()
        self.volumeReader = VolumeReader(self.dev, layout)
        self.volumeReader.Read(filename)
        self.volumeReader.CreateDeviceVolume(self.deviceVolume)
        self.deviceVolume.x_clip, self.deviceVolume.y_clip, self.deviceVolume.z_clip = vec2(-1, 1), vec2(-1, 1), vec2(-1, 1)
        self.deviceVolume.densityScale = 1.0
        self.lib.setup_volume(C.byref(self.deviceVolume)); self.dev.check()
        self.stepSize = self.volumeReader.GetElementBoundingSphereRadius()
        self.volumeSize = self.volumeReader.GetVolumeSize()
        self.volumeDim = tuple(int(d) for d in self.volumeReader.dim)
        self.boundingSphereRadius = self.volumeReader.GetBoundingSphereRadius()
        self.eyeDist = zoom_to_extent_eye_dist(self.volumeSize, self.fov)
        self.camera = camera_setup((0.0, 0.0, self.eyeDist), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), self.fov, self.apeture,
                                   self.focalLength, self.exposure, self.W, self.H)
        self.lib.setup_camera(C.byref(self.camera)); self.dev.check()
        self.ready = True
        self.ReStartRender()

    def SetEnvLightMap(self, filename: str):
        """gui/canvas.h:104-109: Lights::SetEnvironmentLight(filename) + setup_env_lights.  Like the reference's
        cudaEnvironmentLight::Set(tex), this resets the intensity to 1 and the offset to 0."""
        old = int(self.env.tex)
        self.dev.check(self.lib.svr_load_env_map(str(filename).encode(), C.byref(self.env)))
        self._textures.append(int(self.env.tex))
        if old in self._textures:
            self._textures.remove(old)
            self.lib.svr_destroy_texture(old)
        self.lib.setup_env_lights(C.byref(self.env)); self.dev.check()
        self.ReStartRender()

    def SaveFrame(self, filename: str = "0.tga"):
        """The frame dump of gui/canvas.cpp:97-104 (stbi_write_tga of the RGBA8 image)."""
        from .io import save_tga
        save_tga(self.dev, filename, self.read_img())

    def SetCamera(self, cam: cudaCamera):
        self.camera = cam
        self.lib.setup_camera(C.byref(self.camera)); self.dev.check()
        self.ReStartRender()

    # ---- gui/canvas.h:49-54 + TransferFunction ctor, gui/transferfunction.cpp:17-44 ----
    def SetTransferFunctionTable(self, rgba: np.ndarray, maxOpacity: float):
        t = np.ascontiguousarray(rgba, dtype=np.float32).reshape(-1, 4)
        h = self.lib.svr_create_tf_texture(t.ctypes.data_as(C.c_void_p), t.shape[0], 0)
        self.dev.check()
        old = getattr(self, "_tf_tex", 0)
        self._tf_tex = h
        self._textures.append(h)
        self.SetTransferFunction(h, maxOpacity)
        if old and old in self._textures:                      # replaced: free the previous table
            self._textures.remove(old)
            self.lib.svr_destroy_texture(old)

    def SetTransferFunction(self, tex: int, maxOpacity: float):
        self.transferFunction.tex = int(tex)
        self.transferFunction.maxOpacity = float(maxOpacity)
        self.lib.setup_transferfunction(C.byref(self.transferFunction)); self.dev.check()
        self.ReStartRender()

    # ---- gui/canvas.h:56-175 ----
    def SetDensityScale(self, s: float):
        self.deviceVolume.densityScale = float(s)
        self.lib.setup_volume(C.byref(self.deviceVolume)); self.dev.check()
        self.ReStartRender()

    def SetGradientFactor(self, g: float):
        self.deviceVolume.gradientFactor = float(g)
        self.lib.setup_volume(C.byref(self.deviceVolume)); self.dev.check()
        self.ReStartRender()

    def SetScatterTimes(self, val: int):
        self.renderParams.traceDepth = int(val)
        self.ReStartRender()

    def SetRenderMode(self, mode: int):
        self.renderMode = mode
        self.ReStartRender()

    def SetClipPlane(self, x_clip, y_clip, z_clip):
        self.deviceVolume.x_clip = vec2(*x_clip)
        self.deviceVolume.y_clip = vec2(*y_clip)
        self.deviceVolume.z_clip = vec2(*z_clip)
        self.lib.setup_volume(C.byref(self.deviceVolume)); self.dev.check()
        self.ReStartRender()

    def SetEnvLightBackground(self, color):
        self.env.tex = 0
        self.env.defaultRadiance = _to_vec3(color)
        self.lib.setup_env_lights(C.byref(self.env)); self.dev.check()
        self.ReStartRender()

    def SetEnvLightMapTable(self, rgba: np.ndarray):
        t = np.ascontiguousarray(rgba, dtype=np.float32)
        h, w = t.shape[0], t.shape[1]
        tex = self.lib.svr_create_env_texture(t.ctypes.data_as(C.c_void_p), w, h, 0)
        self.dev.check()
        self._textures.append(tex)
        self.env.tex = tex
        self.lib.setup_env_lights(C.byref(self.env)); self.dev.check()
        self.ReStartRender()

    def SetEnvLightIntensity(self, intensity: float):
        self.env.intensity = float(intensity)
        self.lib.setup_env_lights(C.byref(self.env)); self.dev.check()
        self.ReStartRender()

    def SetEnvLightOffset(self, offset):
        self.env.offset = vec2(*offset)
        self.lib.setup_env_lights(C.byref(self.env)); self.dev.check()
        self.ReStartRender()

    def SetAreaLights(self, lights: Sequence[cudaAreaLight]):
        self.areaLights = list(lights)
        n = len(self.areaLights)
        arr = (cudaAreaLight * max(n, 1))(*self.areaLights)
        self.lib.setup_area_lights(arr, n); self.dev.check()
        self.ReStartRender()

    def SetExposure(self, exposure: float):
        self.exposure = float(exposure)
        self.camera.exposure = float(exposure)
        self.lib.setup_camera(C.byref(self.camera)); self.dev.check()
        self.ReStartRender()

    # ---- Canvas::paintGL render branch, gui/canvas.cpp:90-116 ----
    def paint(self, sync: bool = False):
        if not self.ready:
            return
        if self.renderMode == self.RENDER_MODE_RAYCASTING:
            self.lib.render_raycasting(C.c_void_p(self.img), C.byref(self.deviceVolume), C.byref(self.transferFunction),
                                       C.byref(self.camera), C.c_float(self.stepSize))
        else:
            self.lib.render_pathtracer(C.c_void_p(self.img), C.byref(self.renderParams))
        self.dev.check()
        if sync:
            self.dev.synchronize()
        self.renderParams.frameNo += 1

    def paint_frames(self, nframes: int, sync: bool = False):
        """Extension: nframes progressive frames in one launch (svr_render_pathtracer_frames)."""
        self.dev.check(self.lib.svr_render_pathtracer_frames(C.c_void_p(self.img), C.byref(self.renderParams), int(nframes)))
        if sync:
            self.dev.synchronize()
        self.renderParams.frameNo += int(nframes)

    # ---- extension: projection modes of the ray caster (svr_render_projection) ----
    def paint_projection(self, mode: int, iso: float = 0.5, window=(0.0, 1.0), color_tf: bool = False, sync: bool = False):
        """One maximum-intensity (abi.PROJ_MIP), mean-intensity (abi.PROJ_MEAN) or isosurface (abi.PROJ_ISO) image of the canvas's
        volume, transfer function and camera at its step size into the canvas image.  Stateless: the render mode, the accumulator and
        frameNo are untouched.  window = the grey mapping (lo, hi) of MIP / MEAN; color_tf: colours from the transfer function."""
        p = abi.ProjectionParams(int(mode), abi.PROJ_COLOR_TF if color_tf else 0, float(iso), float(window[0]), float(window[1]))
        self.dev.check(self.lib.svr_render_projection(C.c_void_p(self.img), C.byref(self.deviceVolume), C.byref(self.transferFunction),
                                                      C.byref(self.camera), C.c_float(self.stepSize), C.byref(p)))
        if sync:
            self.dev.synchronize()

    # ---- extension: slice views (svr_render_slice, svr_render_slice_stack) ----
    def slice_params_axis(self, axis: int, position: float, w: Optional[int] = None, h: Optional[int] = None) -> abi.SliceParams:
        """svr_slice_params for the plane perpendicular to world axis 0 / 1 / 2 at `position` in [0, 1] across the clipped box of the
        canvas's volume, fitted to w x h pixels (default: the canvas)."""
        return slice_params_axis(self.lib, self.deviceVolume, axis, position, self.W if w is None else w, self.H if h is None else h)

    def slice_params_through(self, axis: int, point, w: Optional[int] = None, h: Optional[int] = None) -> abi.SliceParams:
        """svr_slice_params for the plane perpendicular to world axis 0 / 1 / 2 through the world point `point` (for instance the
        position of a pick), fitted to w x h pixels (default: the canvas)."""
        return slice_params_through(self.lib, self.deviceVolume, axis, point, self.W if w is None else w, self.H if h is None else h)

    def paint_slice(self, params: abi.SliceParams, thickness: Optional[float] = None, step: Optional[float] = None, mode: Optional[int] = None,
                    window=None, color_tf: Optional[bool] = None, sync: bool = False):
        """One slice of the canvas's volume into the canvas image: the plane (or slab) of `params`, with the named members replaced.
        Stateless: the render mode, the accumulator and frameNo are untouched."""
        p = _slice_params(params, thickness, step, mode, window, color_tf)
        self.dev.check(self.lib.svr_render_slice(C.c_void_p(self.img), C.byref(self.deviceVolume), C.byref(self.transferFunction),
                                                 self.W, self.H, C.byref(p)))
        if sync:
            self.dev.synchronize()

    def paint_slice_stack(self, imgs: int, params: abi.SliceParams, count: int, spacing: float, thickness: Optional[float] = None,
                          step: Optional[float] = None, mode: Optional[int] = None, window=None, color_tf: Optional[bool] = None,
                          sync: bool = False):
        """`count` parallel slices, `spacing` apart along the plane's normal, in one launch into the device buffer `imgs`
        (count x H x W x 4 bytes; Device.malloc)."""
        p = _slice_params(params, thickness, step, mode, window, color_tf)
        self.dev.check(self.lib.svr_render_slice_stack(C.c_void_p(int(imgs)), C.byref(self.deviceVolume), C.byref(self.transferFunction),
                                                       self.W, self.H, C.byref(p), int(count), C.c_float(float(spacing))))
        if sync:
            self.dev.synchronize()

    # ---- extension: hit maps and picks (svr_render_hits, svr_pick) ----
    def hit_map(self, mode: int = abi.HIT_OPACITY, alpha: float = 0.5, iso: float = 0.5) -> np.ndarray:
        """Where every pixel's ray meets what the picture shows: an (H, W) array of HIT_DTYPE records (status, sample, t, value,
        position, normal) for abi.HIT_OPACITY (the ray caster's opacity exceeds alpha), abi.HIT_ISO (the isosurface point
        paint_projection shades) or abi.HIT_MAX (the sample of the MIP value).  Stateless; synchronises.  Records outside a row shard
        or render window in force are zero."""
        p = abi.HitParams(int(mode), float(alpha), float(iso))
        nbytes = self.W * self.H * HIT_DTYPE.itemsize
        buf = self.dev.malloc(nbytes)
        try:
            self.dev.check(self.lib.svr_memset_device(C.c_void_p(buf), 0, nbytes))
            self.dev.check(self.lib.svr_render_hits(C.c_void_p(buf), C.byref(self.deviceVolume), C.byref(self.transferFunction),
                                                    C.byref(self.camera), C.c_float(self.stepSize), C.byref(p)))
            self.dev.synchronize()
            return self.dev.to_host(buf, (self.H, self.W), HIT_DTYPE)
        finally:
            self.dev.free(buf)

    def pick(self, pixels, mode: int = abi.HIT_OPACITY, alpha: float = 0.5, iso: float = 0.5) -> np.ndarray:
        """The hit records of the listed pixels ((x, y) pairs, at most abi.PICK_MAX), in list order, in one launch: each is the record
        hit_map has at that pixel.  A query: a row shard or render window in force does not matter.  Stateless; synchronises."""
        xy = np.ascontiguousarray(np.asarray(pixels, dtype=np.int64).reshape(-1, 2))
        if len(xy) and (xy.min() < 0 or xy.max() > 0xffffffff):
            raise SvrError("pick: pixel coordinates must be non-negative")
        xy = xy.astype(np.uint32)
        n = len(xy)
        p = abi.HitParams(int(mode), float(alpha), float(iso))
        buf = self.dev.malloc(max(n, 1) * HIT_DTYPE.itemsize)
        try:
            self.dev.check(self.lib.svr_pick(C.c_void_p(buf), xy.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(self.deviceVolume),
                                             C.byref(self.transferFunction), C.byref(self.camera), C.c_float(self.stepSize), C.byref(p)))
            self.dev.synchronize()
            return self.dev.to_host(buf, (n,), HIT_DTYPE)
        finally:
            self.dev.free(buf)

    # ---- extension: overlays of region masks and label maps (svr_overlay_slice; svr_render_hits + svr_hit_ids + svr_overlay_ids) ----
    def _overlay_region(self, mask, labels):
        """(mask pointer, labels pointer, owned buffer or None, (nz, ny, nx)) of a bool mask / uint32 label array [nz][ny][nx] (uploaded)
        or of a device pointer to either; exactly one of the two is given."""
        if (mask is None) == (labels is None):
            raise SvrError("an overlay needs a mask or a label array, not both")
        if not self.ready:
            raise SvrError("an overlay needs a loaded volume")
        nx, ny, nz = self.volumeDim
        shape = (nz, ny, nx)
        if mask is not None:
            buf, owned = self.dev._region_mask(mask, shape)
            return buf, None, buf if owned else None, shape
        buf, lshape, owned = self.dev._region_labels(labels, shape)
        if tuple(lshape) != shape:
            if owned:
                self.dev.free(buf)
            raise SvrError(f"the labels are {tuple(lshape)}, the volume is {shape}")
        return None, buf, buf if owned else None, shape

    def paint_slice_overlay(self, params: abi.SliceParams, mask=None, labels=None, style: Optional[abi.OverlayStyle] = None, count: int = 1,
                            spacing: float = 0.0, imgs: Optional[int] = None, sync: bool = False):
        """Tints the slice (or, with imgs and count, the stack) that paint_slice / paint_slice_stack drew with the same params by a region:
        mask (a bool array [nz][ny][nx] or the device pointer of a bit mask) or labels (a uint32 array or device pointer).  Every part
        gets the colour of its id, filled with style.fill_alpha and outlined with style.edge_alpha."""
        m, l, owned, shape = self._overlay_region(mask, labels)
        try:
            self.dev.overlay_slice(self.img if imgs is None else imgs, self.deviceVolume, shape, self.W, self.H, params, m, l, style, count, spacing)
            if sync or owned is not None:
                self.dev.synchronize()
        finally:
            if owned is not None:
                self.dev.free(owned)

    def paint_overlay(self, mask=None, labels=None, style: Optional[abi.OverlayStyle] = None, mode: int = abi.HIT_OPACITY, alpha: float = 0.5,
                      iso: float = 0.5, sync: bool = False):
        """Tints the 3D picture in the canvas image (paint with the ray caster, or paint_projection) by a region: every pixel whose ray
        meets what the picture shows (the hit map of `mode`, alpha, iso; see hit_map) inside a part gets that part's colour.  Pixels
        outside a row shard or render window in force have no hit record and stay as they are.  Synchronises."""
        m, l, owned, shape = self._overlay_region(mask, labels)
        p = abi.HitParams(int(mode), float(alpha), float(iso))
        n = self.W * self.H
        buf = self.dev.malloc(n * (HIT_DTYPE.itemsize + 4))
        ids = buf + n * HIT_DTYPE.itemsize
        try:
            self.dev.check(self.lib.svr_memset_device(C.c_void_p(buf), 0, n * HIT_DTYPE.itemsize))
            self.dev.check(self.lib.svr_render_hits(C.c_void_p(buf), C.byref(self.deviceVolume), C.byref(self.transferFunction),
                                                    C.byref(self.camera), C.c_float(self.stepSize), C.byref(p)))
            self.dev.hit_ids(ids, buf, self.W, self.H, self.deviceVolume, shape, m, l)
            self.dev.overlay_ids(self.img, ids, self.W, self.H, 1, style)
            self.dev.synchronize()
        finally:
            self.dev.free(buf)
            if owned is not None:
                self.dev.free(owned)

    # ---- extension: surface meshes of regions and isosurfaces (svr_mesh_*; io.write_stl / write_ply) ----
    def _set_surface(self, mesh):
        self.surfaceVertices, self.surfaceTriangles, self.surfaceInfo = mesh
        return self.surfaceInfo

    def ExtractRegionSurface(self, mask, relax: int = 0) -> abi.MeshInfo:
        """The surface of a region of the loaded volume (a bool array [nz][ny][nx] or the device pointer of its bit mask) after `relax`
        relaxation steps; the canvas keeps the mesh for SaveSurface / SurfaceMeasure.  Returns the svr_mesh_info."""
        if not self.ready:
            raise SvrError("a surface needs a loaded volume")
        nx, ny, nz = self.volumeDim
        return self._set_surface(self.dev.mesh_region(mask, relax, shape=(nz, ny, nx)))

    def ExtractIsoSurface(self, vox, level: int, relax: int = 0) -> abi.MeshInfo:
        """The isosurface {v >= level} of the raw u16 voxels of the loaded volume (a host array [nz][ny][nx] or a device pointer)."""
        if not self.ready:
            raise SvrError("a surface needs a loaded volume")
        nx, ny, nz = self.volumeDim
        return self._set_surface(self.dev.mesh_isosurface(vox, level, relax, shape=(nz, ny, nx)))

    def SaveSurface(self, filename: str):
        """Writes the extracted surface in world coordinates: binary STL, or binary PLY for a name that ends in .ply."""
        from .io import write_ply, write_stl
        if getattr(self, "surfaceInfo", None) is None:
            raise SvrError("SaveSurface before ExtractRegionSurface / ExtractIsoSurface")
        xyz = mesh_positions(self.lib, self.surfaceVertices, volume=self.deviceVolume)
        (write_ply if str(filename).lower().endswith(".ply") else write_stl)(self.dev, filename, xyz, self.surfaceTriangles)

    def SurfaceMeasure(self):
        """(volume, area) of the extracted surface in the volume's units (mm^3, mm^2): the enclosed volume is exact up to its last rounding."""
        if getattr(self, "surfaceInfo", None) is None:
            raise SvrError("SurfaceMeasure before ExtractRegionSurface / ExtractIsoSurface")
        sp = [float(self.deviceVolume.spacing.x), float(self.deviceVolume.spacing.y), float(self.deviceVolume.spacing.z)]
        vol6, area = self.dev.mesh_measure(self.surfaceVertices, self.surfaceTriangles, [t / 256.0 for t in sp])
        return vol6 / (6.0 * 256.0 ** 3) * sp[0] * sp[1] * sp[2], area

    # ---- extension: denoised preview of the first frames after a restart ----
    def SetDenoisePreview(self, frames: int, params: Optional[abi.DenoiseParams] = None):
        """SVR_OPT_DENOISE_PREVIEW = frames (0 = off): the image of a frame with at most `frames` samples per pixel is the
        edge-aware denoised tone map; params (svr_denoise_params) replace the current filter parameters if given."""
        if params is not None:
            self.dev.set_denoise_params(params)
        self.dev.set_option(abi.OPT_DENOISE_PREVIEW, int(frames))

    # ---- extension: noise estimate and render-until-converged ----
    def SetNoiseEstimate(self, on: bool):
        """SVR_OPT_NOISE_ESTIMATE: follow the render and estimate its remaining noise at 8, 16, 32 ... frames (read with noise_estimate)."""
        self.dev.set_option(abi.OPT_NOISE_ESTIMATE, 1 if on else 0)

    def noise_estimate(self, tiles: bool = False):
        """The latest estimate of this canvas's render (abi.NoiseEstimate; frames == 0: none yet); tiles=True: (estimate, (tiles_y, tiles_x)
        float32 tile RMSE map).  The library keeps one estimate per process, of the render it last followed: an estimate whose tile grid is
        not this canvas's belongs to another canvas and reads as none."""
        tx, ty = (self.W + 15) // 16, (self.H + 15) // 16
        est = self.dev.noise_estimate()
        if est.frames and (est.tiles_x, est.tiles_y) != (tx, ty):
            est = abi.NoiseEstimate()
        if not tiles:
            return est
        if not est.frames:
            return est, np.full((ty, tx), np.nan, np.float32)
        buf = self.dev.malloc(tx * ty * 4)
        try:
            est = self.dev.noise_estimate(buf)          # (the same estimate: nothing rendered in between)
            return est, self.dev.to_host(buf, (ty, tx), np.float32)
        finally:
            self.dev.free(buf)

    def paint_until(self, target: float, tile_target: float = 0.0, max_frames: int = 4096, sync: bool = False) -> int:
        """Extension: render until the predicted image RMSE is <= target (and the largest tile RMSE <= tile_target; 0 = unchecked) or
        max_frames frames were traced (svr_render_pathtracer_until).  Advances renderParams.frameNo like paint_frames; returns the frames
        traced."""
        done = C.c_uint32(0)
        rc = self.lib.svr_render_pathtracer_until(C.c_void_p(self.img), C.byref(self.renderParams), C.c_float(target), C.c_float(tile_target),
                                                  int(max_frames), C.byref(done))
        self.dev.check(rc)
        if sync:
            self.dev.synchronize()
        return int(done.value)

    # ---- extension: adaptive sampling ----
    def paint_adaptive(self, tile_target: float, min_frames: int = 0, max_frames: int = 4096, sync: bool = False) -> abi.AdaptiveResult:
        """Extension: render on from renderParams.frameNo, freezing each 16 x 16 tile once its predicted RMSE was <= tile_target at two
        consecutive estimates (and it holds >= min_frames frames), until no tile is active or after max_frames frames
        (svr_render_pathtracer_adaptive).  Advances renderParams.frameNo by frames_max - f0.  Frozen tiles hold fewer frames: restart
        the render (frameNo 0) before painting on."""
        res = abi.AdaptiveResult()
        rc = self.lib.svr_render_pathtracer_adaptive(C.c_void_p(self.img), C.byref(self.renderParams), C.c_float(tile_target),
                                                     int(min_frames), int(max_frames), C.byref(res))
        self.dev.check(rc)
        if sync:
            self.dev.synchronize()
        return res

    def adaptive_tiles(self):
        """(frames[ty, tx] uint32, rmse[ty, tx] float32): the tile frame counts and final tile RMSE of the last adaptive call
        (svr_get_adaptive_tiles; the maps of this canvas's size)."""
        tx, ty = (self.W + 15) // 16, (self.H + 15) // 16
        fbuf = self.dev.malloc(tx * ty * 4)
        rbuf = self.dev.malloc(tx * ty * 4)
        try:
            self.dev.check(self.lib.svr_get_adaptive_tiles(C.c_void_p(fbuf), C.c_void_p(rbuf)))
            return self.dev.to_host(fbuf, (ty, tx), np.uint32), self.dev.to_host(rbuf, (ty, tx), np.float32)
        finally:
            self.dev.free(fbuf)
            self.dev.free(rbuf)

    def read_guides(self) -> np.ndarray:
        """The guide buffer of the current scene (svr_render_guides): (H, W, 8) float32 = N.xyz, D, A.rgb, O."""
        buf = self.dev.malloc(self.W * self.H * 32)
        try:
            self.dev.check(self.lib.svr_render_guides(C.c_void_p(buf)))
            return self.dev.to_host(buf, (self.H, self.W, 8), np.float32)
        finally:
            self.dev.free(buf)

    def read_hdr(self) -> np.ndarray:
        return self.dev.to_host(int(self.renderParams.hdrBuffer), (self.H, self.W, 3), np.float32)

    def read_img(self) -> np.ndarray:
        return self.dev.to_host(self.img, (self.H, self.W, 4), np.uint8)

    def close(self):
        self.dev.synchronize()
        for h in self._textures:
            self.lib.svr_destroy_texture(h)
        self._textures.clear()
        if getattr(self, "volumeReader", None) is not None:
            self.volumeReader.ClearDevice()
            self.volumeReader = None
        if self._own_hdr:
            self.lib.svr_render_params_clear(C.byref(self.renderParams))
        if self._own_img and self.img:
            self.lib.svr_device_free(C.c_void_p(self.img))
            self.img = 0
        self.lib.svr_clear_error()
