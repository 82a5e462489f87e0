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

The volume operations (regions, masks, labels, distances, filters, meshes, resampling, histograms, overlays) are in volume_ops.py:
Device inherits their methods from volume_ops.VolumeOps, and their module functions are names of this module as well.
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


def _host_call(lib, name, rc, ok=(0,)):
    """The return value of a call into the library's host code, or SvrError with the library's message for a value outside `ok`."""
    if rc not in ok:
        msg = lib.svr_last_error().decode("utf-8", "replace")
        lib.svr_clear_error()
        raise SvrError(f"{name} failed ({rc}): {msg}")
    return rc


# The volume operations live in volume_ops.py, which takes SvrError, _host_call and _to_vec3 from here: the import follows them.  Every
# public name of it stays a name of this module.
from .volume_ops import (COMPONENT_DTYPE, LABEL_SCAN_BLOCK, VolumeOps as _VolumeOps, compare_measure, compare_params, distance_weights,  # noqa: E402,F401
                         geodesic_weights, histogram_bin_range, histogram_bins, histogram_moments, histogram_otsu, histogram_params,
                         histogram_quantile, mesh_positions, overlap_match, region_label_scan_levels, region_mask_pack,
                         region_mask_unpack, region_mask_words, region_seed_from_world,
                         scissor_params, scissor_project_camera, scissor_project_slice, stencil_rect, fill_between_params,
                         region_box_size, region_smooth_radii,
                         resample_grid, resample_grid_box, resample_grid_dims, resample_grid_place, resample_grid_spacing, smooth_radii)


class Device(_VolumeOps):
    """Thin RAII-style wrapper over the svr_* helper entry points (non-fatal error mode); the volume operations are volume_ops.VolumeOps."""

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


def slice_params_axis(lib, volume: cudaVolume, axis: int, position: float, w: int, h: int) -> abi.SliceParams:
    """svr_slice_params_axis: the plane perpendicular to world axis 0 / 1 / 2 at `position` in [0, 1] across the clipped box of
    `volume`, fitted to w x h pixels.  Host code of the library: no device is needed."""
    p = abi.SliceParams()
    _host_call(lib, "svr_slice_params_axis", lib.svr_slice_params_axis(C.byref(p), C.byref(volume), int(axis), C.c_float(float(position)), int(w), int(h)))
    return p


def slice_params_through(lib, volume: cudaVolume, axis: int, point, w: int, h: int) -> abi.SliceParams:
    """svr_slice_params_through: the axis plane of slice_params_axis through the world point `point` (a picked position).  Host code
    of the library: no device is needed."""
    p = abi.SliceParams()
    q = _to_vec3(point)
    _host_call(lib, "svr_slice_params_through", lib.svr_slice_params_through(C.byref(p), C.byref(volume), int(axis), C.byref(q), int(w), int(h)))
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
    def _overlay_region(self, s, mask, labels):
        """(mask pointer, labels pointer, (nz, ny, nx)) of a bool mask / uint32 label array [nz][ny][nx] (uploaded in the staging scope
        s) or of a device pointer to either; exactly one of the two is given."""
        if (mask is None) == (labels is None):
            raise SvrError("an overlay needs a mask or a label array, not both")
        if not self.ready:
            raise SvrError("an overlay needs a loaded volume")
        nx, ny, nz = self.volumeDim
        shape = (nz, ny, nx)
        if mask is not None:
            return s.mask(mask, shape).value, None, shape
        buf, lshape = s.map(labels, shape)
        if lshape != shape:
            raise SvrError(f"the labels are {lshape}, the volume is {shape}")
        return None, buf.value, shape

    def paint_slice_overlay(self, params: abi.SliceParams, mask=None, labels=None, style: Optional[abi.OverlayStyle] = None, count: int = 1,
                            spacing: float = 0.0, imgs: Optional[int] = None, sync: bool = False):
        """Tints the slice (or, with imgs and count, the stack) that paint_slice / paint_slice_stack drew with the same params by a region:
        mask (a bool array [nz][ny][nx] or the device pointer of a bit mask) or labels (a uint32 array or device pointer).  Every part
        gets the colour of its id, filled with style.fill_alpha and outlined with style.edge_alpha."""
        with self.dev._staging() as s:
            m, l, shape = self._overlay_region(s, mask, labels)
            self.dev.overlay_slice(self.img if imgs is None else imgs, self.deviceVolume, shape, self.W, self.H, params, m, l, style, count, spacing)
            if sync or s.owned:                               # an uploaded region is freed on exit: the kernel is done with it first
                self.dev.synchronize()

    def paint_overlay(self, mask=None, labels=None, style: Optional[abi.OverlayStyle] = None, mode: int = abi.HIT_OPACITY, alpha: float = 0.5,
                      iso: float = 0.5, sync: bool = False):
        """Tints the 3D picture in the canvas image (paint with the ray caster, or paint_projection) by a region: every pixel whose ray
        meets what the picture shows (the hit map of `mode`, alpha, iso; see hit_map) inside a part gets that part's colour.  Pixels
        outside a row shard or render window in force have no hit record and stay as they are.  Synchronises."""
        with self.dev._staging() as s:
            m, l, shape = self._overlay_region(s, mask, labels)
            p = abi.HitParams(int(mode), float(alpha), float(iso))
            n = self.W * self.H
            buf = s.alloc(n * (HIT_DTYPE.itemsize + 4))
            ids = buf + n * HIT_DTYPE.itemsize
            self.dev.check(self.lib.svr_memset_device(C.c_void_p(buf), 0, n * HIT_DTYPE.itemsize))
            self.dev.check(self.lib.svr_render_hits(C.c_void_p(buf), C.byref(self.deviceVolume), C.byref(self.transferFunction),
                                                    C.byref(self.camera), C.c_float(self.stepSize), C.byref(p)))
            self.dev.hit_ids(ids, buf, self.W, self.H, self.deviceVolume, shape, m, l)
            self.dev.overlay_ids(self.img, ids, self.W, self.H, 1, style)
            self.dev.synchronize()

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
