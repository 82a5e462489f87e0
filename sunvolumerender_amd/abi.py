"""ctypes binding of libsvr_hip.so -- exactly the C ABI declared in include/svr_abi.h.

There is no fallback: if the library has not been built, `load()` raises.  Nothing in
this module (or anywhere in the package) imports or links the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

from ._build import LIB_PATH

# ---------------------------------------------------------------------------
# POD layouts of the reference host API; names follow the reference
# ---------------------------------------------------------------------------


class vec2(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]

    def __init__(self, x=0.0, y=0.0):
        super().__init__(float(x), float(y))

    def tuple(self):
        return (self.x, self.y)


class vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def __init__(self, x=0.0, y=0.0, z=0.0):
        super().__init__(float(x), float(y), float(z))

    def tuple(self):
        return (self.x, self.y, self.z)


class cudaBBox(C.Structure):  # core/geometry/cuda_bbox.h:66-69
    _fields_ = [("vmin", vec3), ("vmax", vec3), ("invSize", vec3)]


class cudaVolume(C.Structure):  # core/cuda_volume.h:111-121
    _fields_ = [
        ("bbox", cudaBBox),
        ("_pad0", C.c_uint32),
        ("tex", C.c_uint64),
        ("densityScale", C.c_float),
        ("invMaxMagnitude", C.c_float),
        ("gradientFactor", C.c_float),
        ("spacing", vec3),
        ("invSpacing", vec3),
        ("x_clip", vec2),
        ("y_clip", vec2),
        ("z_clip", vec2),
        ("_pad1", C.c_uint32),
    ]


class cudaTransferFunction(C.Structure):  # core/cuda_transfer_function.h:57-59
    _fields_ = [("tex", C.c_uint64), ("maxOpacity", C.c_float), ("_pad", C.c_uint32)]


class cudaCamera(C.Structure):  # core/cuda_camera.h:98-106
    _fields_ = [
        ("imageW", C.c_uint32),
        ("imageH", C.c_uint32),
        ("exposure", C.c_float),
        ("apeture", C.c_float),
        ("focalLength", C.c_float),
        ("aspectRatio", C.c_float),
        ("tanFovxOverTwo", C.c_float),
        ("pos", vec3),
        ("u", vec3),
        ("v", vec3),
        ("w", vec3),
    ]


class cudaDisk(C.Structure):  # core/geometry/cuda_disk.h:58-61
    _fields_ = [("radius", C.c_float), ("center", vec3), ("normal", vec3)]


class cudaAreaLight(C.Structure):  # core/lights/cuda_arealight.h:68-71
    _fields_ = [("disk", cudaDisk), ("color", vec3), ("intensity", C.c_float)]


class cudaEnvironmentLight(C.Structure):  # core/lights/cuda_environment_light.h:74-78
    _fields_ = [("tex", C.c_uint64), ("defaultRadiance", vec3), ("intensity", C.c_float), ("offset", vec2)]


class RenderParams(C.Structure):  # core/render_parameters.h:34-37
    _fields_ = [("traceDepth", C.c_uint32), ("frameNo", C.c_uint32), ("hdrBuffer", C.c_void_p)]


class Counters(C.Structure):  # svr_counters
    _fields_ = [
        ("paths", C.c_uint64),
        ("vol_taps", C.c_uint64),
        ("woodcock_iters", C.c_uint64),
        ("scatter_events", C.c_uint64),
        ("shadow_walks", C.c_uint64),
        ("raycast_steps", C.c_uint64),
        ("loop_iters", C.c_uint64),
        ("vol_taps_executed", C.c_uint64),
        ("walks_ray_skipped", C.c_uint64),
        ("iters_ray_skipped", C.c_uint64),
        ("iters_prefix_skipped", C.c_uint64),
        ("taps_bound_culled", C.c_uint64),
    ]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ }


class DenoiseParams(C.Structure):  # svr_denoise_params
    _fields_ = [
        ("passes", C.c_int32),
        ("sigma_depth", C.c_float),
        ("sigma_normal", C.c_float),
        ("sigma_albedo", C.c_float),
        ("sigma_opacity", C.c_float),
        ("sigma_color", C.c_float),
        ("step", C.c_float),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


svr_denoise_params = DenoiseParams


class NoiseEstimate(C.Structure):  # svr_noise_estimate
    _fields_ = [
        ("frames", C.c_uint32),
        ("frames_ref", C.c_uint32),
        ("rmse", C.c_float),
        ("tile_max", C.c_float),
        ("tiles_x", C.c_uint32),
        ("tiles_y", C.c_uint32),
        ("pixels", C.c_uint64),
        ("nonfinite", C.c_uint64),
        ("sse", C.c_double),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


svr_noise_estimate = NoiseEstimate


class AdaptiveResult(C.Structure):  # svr_adaptive_result
    _fields_ = [
        ("frames_max", C.c_uint32),
        ("frames_min", C.c_uint32),
        ("tiles_x", C.c_uint32),
        ("tiles_y", C.c_uint32),
        ("tiles_active", C.c_uint32),
        ("checkpoints", C.c_uint32),
        ("pixel_frames", C.c_uint64),
        ("pixels", C.c_uint64),
        ("nonfinite", C.c_uint64),
        ("sse", C.c_double),
        ("rmse", C.c_float),
        ("tile_max", C.c_float),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


svr_adaptive_result = AdaptiveResult


class ProjectionParams(C.Structure):  # svr_projection_params
    _fields_ = [
        ("mode", C.c_int32),
        ("flags", C.c_uint32),
        ("iso", C.c_float),
        ("window_lo", C.c_float),
        ("window_hi", C.c_float),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


svr_projection_params = ProjectionParams
PROJ_MIP, PROJ_MEAN, PROJ_ISO = 1, 2, 3
PROJ_COLOR_TF = 1


class SliceParams(C.Structure):  # svr_slice_params
    _fields_ = [
        ("center", vec3),
        ("u", vec3),
        ("v", vec3),
        ("thickness", C.c_float),
        ("step", C.c_float),
        ("mode", C.c_int32),
        ("flags", C.c_uint32),
        ("window_lo", C.c_float),
        ("window_hi", C.c_float),
    ]

    def as_dict(self):
        return {n: ((getattr(self, n).x, getattr(self, n).y, getattr(self, n).z) if t is vec3 else getattr(self, n)) for n, t in self._fields_}


svr_slice_params = SliceParams
SLAB_MIP, SLAB_MINIP, SLAB_MEAN = 1, 2, 3
SLICE_COLOR_TF = 1
SLICE_MAX_SAMPLES = 4096


class Hit(C.Structure):  # svr_hit
    _fields_ = [
        ("status", C.c_int32),
        ("sample", C.c_int32),
        ("t", C.c_float),
        ("value", C.c_float),
        ("position", vec3),
        ("normal", vec3),
    ]


class HitParams(C.Structure):  # svr_hit_params
    _fields_ = [("mode", C.c_int32), ("alpha", C.c_float), ("iso", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


svr_hit, svr_hit_params = Hit, HitParams
HIT_OPACITY, HIT_ISO, HIT_MAX = 1, 2, 3
HIT_STATUS_MISS, HIT_STATUS_NONE, HIT_STATUS_FOUND = 0, 1, 2
PICK_MAX = 4096


class RegionParams(C.Structure):  # svr_region_params
    _fields_ = [
        ("lo", C.c_uint32),
        ("hi", C.c_uint32),
        ("connectivity", C.c_int32),
        ("box_min", C.c_int32 * 3),
        ("box_max", C.c_int32 * 3),
        ("max_sweeps", C.c_uint32),
    ]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n.startswith("box") else getattr(self, n)) for n, _ in self._fields_}


class RegionStats(C.Structure):  # svr_region_stats
    _fields_ = [(n, C.c_uint64) for n in ("voxels", "sum", "sum_sq", "sum_x", "sum_y", "sum_z", "faces_x", "faces_y", "faces_z")] + [
        ("vmin", C.c_uint32),
        ("vmax", C.c_uint32),
        ("bbox_min", C.c_int32 * 3),
        ("bbox_max", C.c_int32 * 3),
        ("sweeps", C.c_uint32),
        ("status", C.c_int32),
    ]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n.startswith("bbox") else int(getattr(self, n))) for n, _ in self._fields_}


class RegionMeasurement(C.Structure):  # svr_region_measurement
    _fields_ = [("volume", C.c_double), ("mean", C.c_double), ("stddev", C.c_double), ("centroid", C.c_double * 3),
                ("surface_area", C.c_double)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n == "centroid" else getattr(self, n)) for n, _ in self._fields_}


class RegionComponent(C.Structure):  # svr_region_component
    _fields_ = [("voxels", C.c_uint32), ("first", C.c_uint32), ("bbox_min", C.c_int32 * 3), ("bbox_max", C.c_int32 * 3), ("sum", C.c_uint64)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n.startswith("bbox") else int(getattr(self, n))) for n, _ in self._fields_}


svr_region_params, svr_region_stats, svr_region_measurement = RegionParams, RegionStats, RegionMeasurement
svr_region_component = RegionComponent
REGION_ERR_LABEL = -10
LABEL_SCAN_BLOCK = 256      # SVR_LABEL_SCAN_BLOCK of csrc/svr_label.hip: the words one block of a level of the renumbering scan covers
REGION_MAX_SEEDS = 64
REGION_KEEP, REGION_REMOVE = 1, 2
REGION_STATUS_OK, REGION_STATUS_EMPTY = 0, 1
REGION_ERR_SWEEPS = -9
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE = 1, 2, 3, 4
MORPH_MAX_RADIUS = 32
MASK_AND, MASK_OR, MASK_ANDNOT, MASK_XOR, MASK_NOT = 1, 2, 3, 4, 5
DIST_NONE = 0xFFFFFFFF
DIST_TO_SET, DIST_TO_UNSET = 1, 2
DISTANCE_COLUMN_BLOCK = 256  # SVR_DISTANCE_COLUMN_BLOCK of csrc/svr_distance.hip: the columns of a column pass that one block covers
FILTER_MEDIAN, FILTER_MIN, FILTER_MAX = 1, 2, 3
FILTER_MAX_ITERATIONS = 64
SMOOTH_MAX_RADIUS = 8
GEO_NONE = 0xFFFFFFFF
GEO_TILE = (32, 8, 8)     # the relaxation tile of csrc/svr_geodesic.hip in voxels (x, y, z)


class GrowcutParams(C.Structure):  # svr_growcut_params
    _fields_ = [("step_weights", C.c_uint32 * 7), ("contrast_gain", C.c_uint32), ("contrast_shift", C.c_uint32), ("max_sweeps", C.c_uint32)]


class GrowcutInfo(C.Structure):  # svr_growcut_info
    _fields_ = [("sweeps", C.c_uint32), ("unreached", C.c_uint64), ("saturated", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


svr_growcut_params, svr_growcut_info = GrowcutParams, GrowcutInfo
GROWCUT_CAP = 0xFFFFFFFE
REGION_ERR_RANGE = -12


class HistogramParams(C.Structure):  # svr_histogram_params
    _fields_ = [("lo", C.c_uint32), ("hi", C.c_uint32), ("shift", C.c_uint32), ("box_min", C.c_int32 * 3), ("box_max", C.c_int32 * 3)]


svr_histogram_params = HistogramParams
HISTOGRAM_MAX_CELLS = 1 << 24
HISTOGRAM_STATUS_EMPTY = 1


class DistanceSummary(C.Structure):  # svr_distance_summary
    _fields_ = [("voxels", C.c_uint64), ("none", C.c_uint64), ("sum", C.c_uint64), ("sum_root_q8", C.c_uint64), ("max", C.c_uint32),
                ("first_max", C.c_uint32), ("within", C.c_uint32 * 8)]


class CompareParams(C.Structure):  # svr_compare_params
    _fields_ = [("element", C.c_int32), ("weights", C.c_uint32 * 3), ("q_num", C.c_uint32), ("q_den", C.c_uint32), ("ntol", C.c_uint32),
                ("tolerances2", C.c_uint32 * 8)]


class RegionComparison(C.Structure):  # svr_region_comparison
    _fields_ = [("overlap", C.c_uint64 * 4), ("surface", C.c_uint64 * 2), ("ab", DistanceSummary), ("ba", DistanceSummary),
                ("quantile_ab", C.c_uint32), ("quantile_ba", C.c_uint32), ("ntol", C.c_uint32), ("status", C.c_int32)]


class CompareMeasurement(C.Structure):  # svr_compare_measurement
    _fields_ = [(n, C.c_double) for n in ("dice", "jaccard", "volume_difference", "hausdorff_ab", "hausdorff_ba", "hausdorff",
                                          "hausdorff_q_ab", "hausdorff_q_ba", "hausdorff_q", "assd", "rms")] + [("surface_dice", C.c_double * 8)]


svr_distance_summary, svr_compare_params, svr_region_comparison, svr_compare_measurement = DistanceSummary, CompareParams, RegionComparison, CompareMeasurement
OVERLAP_BOTH, OVERLAP_A_ONLY, OVERLAP_B_ONLY, OVERLAP_NEITHER = 0, 1, 2, 3
COMPARE_MAX_TOLERANCES = 8
COMPARE_A_EMPTY, COMPARE_B_EMPTY = 1, 2


class ScissorParams(C.Structure):  # svr_scissor_params
    _fields_ = [("op", C.c_int32), ("depth_lo", C.c_float), ("depth_hi", C.c_float), ("flags", C.c_uint32)]


svr_scissor_params = ScissorParams
SCISSOR_SELECT, SCISSOR_ERASE_INSIDE, SCISSOR_ERASE_OUTSIDE, SCISSOR_FILL_INSIDE = 0, 1, 2, 3
STENCIL_MAX_VERTICES = 4096
STENCIL_MAX_COORD = 1 << 23


class FillBetweenParams(C.Structure):  # svr_fill_between_params
    _fields_ = [("axis", C.c_int32), ("flags", C.c_uint32), ("weights", C.c_uint32 * 3), ("nkeys", C.c_int32), ("keys", C.POINTER(C.c_int32))]


class FillBetweenInfo(C.Structure):  # svr_fill_between_info
    _fields_ = [("axis", C.c_int32), ("keys", C.c_uint32), ("gaps", C.c_uint32), ("filled_slices", C.c_uint32), ("first_key", C.c_int32),
                ("last_key", C.c_int32), ("launches", C.c_uint32), ("reserved", C.c_uint32), ("voxels_in", C.c_uint64), ("voxels_out", C.c_uint64),
                ("workspace_bytes", C.c_uint64)]


svr_fill_between_params, svr_fill_between_info = FillBetweenParams, FillBetweenInfo
FILL_KEEP_BETWEEN, FILL_GAP_BY_GAP = 1, 2
FILL_MAP_BUDGET_BYTES = 1 << 30
SMOOTH_MAJORITY, SMOOTH_BINOMIAL = 1, 2
REGION_SMOOTH_MAX_RADIUS, REGION_SMOOTH_MAX_ITERATIONS, LABEL_SMOOTH_MAX_COUNT = 8, 16, 255


class OverlaySource(C.Structure):  # svr_overlay_source: exactly one device pointer is set
    _fields_ = [("mask_device", C.c_void_p), ("labels_device", C.c_void_p)]


class OverlayStyle(C.Structure):  # svr_overlay_style
    _fields_ = [
        ("fill_alpha", C.c_uint32),
        ("edge_alpha", C.c_uint32),
        ("palette_count", C.c_uint32),
        ("flags", C.c_uint32),
        ("palette", C.POINTER(C.c_uint32)),   # HOST array of palette_count RGBA8 entries; NULL with 0: the built-in table
    ]


svr_overlay_source, svr_overlay_style = OverlaySource, OverlayStyle
OVERLAY_MAX_PALETTE = 256
OVERLAY_DEFAULT_PALETTE = 12


class MeshParams(C.Structure):  # svr_mesh_params
    _fields_ = [("level", C.c_uint32), ("relax", C.c_uint32)]


class MeshInfo(C.Structure):  # svr_mesh_info
    _fields_ = [("vertices", C.c_uint64), ("quads", C.c_uint64), ("triangles", C.c_uint64), ("bbox_min", C.c_int32 * 3), ("bbox_max", C.c_int32 * 3),
                ("status", C.c_int32), ("_pad", C.c_uint32)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n.startswith("bbox") else int(getattr(self, n))) for n, _ in self._fields_ if n != "_pad"}


svr_mesh_params, svr_mesh_info = MeshParams, MeshInfo
MESH_MAX_RELAX = 64
MESH_MAX_DIM = 8388606
MESH_ERR_CAPACITY = -11


class AxisMap(C.Structure):  # svr_axis_map: Q16 source edge coordinates
    _fields_ = [("origin", C.c_int64), ("step", C.c_uint32), ("count", C.c_uint32)]


class ResampleGrid(C.Structure):  # svr_resample_grid: x, y, z
    _fields_ = [("axis", AxisMap * 3)]

    def as_tuples(self):
        """((origin, step, count) of x, of y, of z)"""
        return tuple((int(m.origin), int(m.step), int(m.count)) for m in self.axis)

    @property
    def shape(self):
        """(nz, ny, nx) of the output"""
        return (int(self.axis[2].count), int(self.axis[1].count), int(self.axis[0].count))


svr_axis_map, svr_resample_grid = AxisMap, ResampleGrid
RESAMPLE_NEAREST, RESAMPLE_LINEAR, RESAMPLE_AREA, RESAMPLE_AUTO = 0, 1, 2, 3
RESAMPLE_MIN_STEP, RESAMPLE_MAX_STEP = 1024, 4194304
PASTE_REPLACE = 0


EXPECTED_SIZES = {
    vec3: 12,
    cudaBBox: 36,
    cudaVolume: 112,
    cudaTransferFunction: 16,
    cudaCamera: 76,
    cudaDisk: 28,
    cudaAreaLight: 44,
    cudaEnvironmentLight: 32,
    RenderParams: 16,
    Counters: 96,
    DenoiseParams: 28,
    NoiseEstimate: 48,
    AdaptiveResult: 64,
    ProjectionParams: 20,
    SliceParams: 60,
    Hit: 40,
    HitParams: 12,
    RegionParams: 40,
    RegionStats: 112,
    RegionMeasurement: 56,
    RegionComponent: 40,
    OverlaySource: 16,
    OverlayStyle: 24,
    MeshParams: 8,
    MeshInfo: 56,
    AxisMap: 16,
    ResampleGrid: 48,
}
for _t, _n in EXPECTED_SIZES.items():
    assert C.sizeof(_t) == _n, (_t, C.sizeof(_t), _n)

MAX_LIGHT_SOURCES = 8
TF_TABLE_SIZE = 1024

LAYOUT_AUTO, LAYOUT_LINEAR, LAYOUT_BRICK, LAYOUT_PAIR, LAYOUT_CELL = 0, 1, 2, 3, 4
OPT_ENV_ON_ESCAPE, OPT_KERNEL, OPT_COUNT, OPT_TIMING, OPT_SKIP_TONEMAP, OPT_BLOCKS_PER_CU = 1, 2, 3, 4, 5, 6
OPT_PIPELINE, OPT_REFILL_MIN_IDLE, OPT_EMPTY_SKIP, OPT_RAY_SKIP, OPT_FRAMES_PER_WAVE_LOG2 = 7, 8, 9, 10, 11
OPT_RAYCAST_LANES_LOG2 = 12
OPT_FRAME_AHEAD = 13
OPT_FAST_MATH = 14
OPT_BOUND_CULL = 15
OPT_FOLD = 17
OPT_QUEUE = 18
OPT_PARK_END = 19
OPT_FINE_MASK = 20
OPT_ROW_ORDER = 21
OPT_GROUP_FRAMES = 22
OPT_LOCAL_MAJORANT = 23
OPT_LIGHT_CULL = 24
OPT_LM_TUNE = 25
OPT_LM_SUBCELLS = 26
OPT_PARK_CHEAP = 27
OPT_PINHOLE_FAST = 28
OPT_POOL = 29
OPT_TRIPS = 30
OPT_NAN_GUARD = 31
OPT_MACRO_SHIFT_MIN = 32
OPT_SPLIT = 33
OPT_ENV_NEE = 34
OPT_FAST_BOUND = 35
OPT_DENOISE_PREVIEW = 36
OPT_NOISE_ESTIMATE = 37
OPT_UNIT = 101                         # tasks per ticket of the tile kernel (0: the launcher's choice); placement only
KERNEL_AUTO, KERNEL_PIXEL, KERNEL_TILE, KERNEL_ULOOP, KERNEL_WAVEFRONT = 0, 1, 2, 3, 4

ELEM_I8, ELEM_U8, ELEM_I16, ELEM_U16, ELEM_I32, ELEM_U32, ELEM_F32, ELEM_F64 = range(8)


class MhdHeader(C.Structure):          # svr_mhd_header, include/svr_io.h
    _fields_ = [
        ("ndims", C.c_int32), ("dim", C.c_int32 * 3), ("spacing", C.c_double * 3),
        ("elem_type", C.c_int32), ("elem_size", C.c_int32), ("channels", C.c_int32), ("msb", C.c_int32),
        ("compressed", C.c_int32), ("compressed_size", C.c_int64), ("header_size", C.c_int64),
        ("data_offset", C.c_int64), ("data_file", C.c_char * 1024),
    ]


class VolumeInfo(C.Structure):         # svr_volume_info, include/svr_io.h
    _fields_ = [
        ("dim", C.c_int32 * 3), ("spacing", C.c_float * 3), ("range", C.c_double * 2),
        ("maxMagnitude", C.c_float), ("hist_bins", C.c_uint32),
    ]


# every symbol include/svr_abi.h and include/svr_io.h declare: name -> (restype, argtypes)
_P = C.POINTER
PROTOTYPES = {
    # (A) the reference's entry points
    "render_pathtracer": (None, [C.c_void_p, _P(RenderParams)]),
    "setup_volume": (None, [_P(cudaVolume)]),
    "setup_transferfunction": (None, [_P(cudaTransferFunction)]),
    "setup_camera": (None, [_P(cudaCamera)]),
    "setup_env_lights": (None, [_P(cudaEnvironmentLight)]),
    "setup_area_lights": (None, [_P(cudaAreaLight), C.c_uint32]),
    "render_raycasting": (None, [C.c_void_p, _P(cudaVolume), _P(cudaTransferFunction), _P(cudaCamera), C.c_float]),
    # (B) helpers
    "svr_init": (C.c_int, [C.c_int]),
    "svr_shutdown": (None, []),
    "svr_set_stream": (C.c_int, [C.c_void_p]),
    "svr_device_synchronize": (C.c_int, []),
    "svr_set_error_mode": (None, [C.c_int]),
    "svr_last_error": (C.c_char_p, []),
    "svr_last_error_code": (C.c_int, []),
    "svr_clear_error": (None, []),
    "svr_create_volume_texture": (C.c_uint64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "svr_create_tf_texture": (C.c_uint64, [C.c_void_p, C.c_int, C.c_int]),
    "svr_update_tf_texture": (C.c_int, [C.c_uint64, C.c_void_p, C.c_int, C.c_int]),
    "svr_create_env_texture": (C.c_uint64, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "svr_destroy_texture": (C.c_int, [C.c_uint64]),
    "svr_render_params_setup_hdr": (C.c_int, [_P(RenderParams), C.c_uint32, C.c_uint32]),
    "svr_render_params_clear": (C.c_int, [_P(RenderParams)]),
    "svr_device_malloc": (C.c_void_p, [C.c_size_t]),
    "svr_device_free": (C.c_int, [C.c_void_p]),
    "svr_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "svr_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "svr_memset_device": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t]),
    "svr_strip_rows_owned": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "svr_strip_row_to_y": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "svr_pack_strips": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "svr_unpack_strips": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "svr_assemble_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "svr_set_row_shard": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "svr_set_render_window": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "svr_set_option": (C.c_int, [C.c_int, C.c_int]),
    "svr_get_option": (C.c_int, [C.c_int]),
    "svr_render_pathtracer_frames": (C.c_int, [C.c_void_p, _P(RenderParams), C.c_uint32]),
    "svr_hdr_to_ldr": (C.c_int, [C.c_void_p, _P(RenderParams)]),
    "svr_hdr_to_ldr_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "svr_selftest_chain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "svr_selftest_math": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "svr_selftest_bound8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "svr_selftest_group_march": (C.c_int, [C.c_uint32, C.c_void_p]),
    "svr_macro_grid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_int)]),
    "svr_selftest_accel": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, _P(C.c_int32)]),
    "svr_denoise_params_default": (C.c_int, [_P(DenoiseParams)]),
    "svr_set_denoise_params": (C.c_int, [_P(DenoiseParams)]),
    "svr_get_denoise_params": (C.c_int, [_P(DenoiseParams)]),
    "svr_render_guides": (C.c_int, [C.c_void_p]),
    "svr_denoise_to_ldr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, _P(DenoiseParams)]),
    "svr_denoise_hdr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, _P(DenoiseParams)]),
    "svr_guide_builds": (C.c_uint64, []),
    "svr_get_noise_estimate": (C.c_int, [_P(NoiseEstimate), C.c_void_p]),
    "svr_estimate_noise": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _P(NoiseEstimate)]),
    "svr_render_pathtracer_until": (C.c_int, [C.c_void_p, _P(RenderParams), C.c_float, C.c_float, C.c_uint32, _P(C.c_uint32)]),
    "svr_render_pathtracer_adaptive": (C.c_int, [C.c_void_p, _P(RenderParams), C.c_float, C.c_uint32, C.c_uint32, _P(AdaptiveResult)]),
    "svr_get_adaptive_tiles": (C.c_int, [C.c_void_p, C.c_void_p]),
    "svr_projection_params_default": (C.c_int, [_P(ProjectionParams)]),
    "svr_render_projection": (C.c_int, [C.c_void_p, _P(cudaVolume), _P(cudaTransferFunction), _P(cudaCamera), C.c_float, _P(ProjectionParams)]),
    "svr_slice_params_default": (C.c_int, [_P(SliceParams)]),
    "svr_slice_params_axis": (C.c_int, [_P(SliceParams), _P(cudaVolume), C.c_int, C.c_float, C.c_uint32, C.c_uint32]),
    "svr_render_slice": (C.c_int, [C.c_void_p, _P(cudaVolume), _P(cudaTransferFunction), C.c_uint32, C.c_uint32, _P(SliceParams)]),
    "svr_render_slice_stack": (C.c_int, [C.c_void_p, _P(cudaVolume), _P(cudaTransferFunction), C.c_uint32, C.c_uint32, _P(SliceParams),
                                         C.c_uint32, C.c_float]),
    "svr_slice_params_through": (C.c_int, [_P(SliceParams), _P(cudaVolume), C.c_int, _P(vec3), C.c_uint32, C.c_uint32]),
    "svr_hit_params_default": (C.c_int, [_P(HitParams)]),
    "svr_render_hits": (C.c_int, [C.c_void_p, _P(cudaVolume), _P(cudaTransferFunction), _P(cudaCamera), C.c_float, _P(HitParams)]),
    "svr_pick": (C.c_int, [C.c_void_p, _P(C.c_uint32), C.c_uint32, _P(cudaVolume), _P(cudaTransferFunction), _P(cudaCamera), C.c_float,
                           _P(HitParams)]),
    "svr_region_params_default": (C.c_int, [_P(RegionParams)]),
    "svr_region_mask_words": (C.c_uint64, [C.c_int, C.c_int, C.c_int]),
    "svr_region_default_max_sweeps": (C.c_uint32, [C.c_int, C.c_int, C.c_int]),
    "svr_region_grow": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_int32), C.c_uint32, _P(RegionParams), C.c_void_p,
                                  _P(RegionStats)]),
    "svr_region_stats_of": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, _P(RegionStats)]),
    "svr_region_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]),
    "svr_region_seed_from_world": (C.c_int, [_P(cudaVolume), C.c_int, C.c_int, C.c_int, _P(vec3), _P(C.c_int32)]),
    "svr_region_measure": (C.c_int, [_P(RegionStats), _P(C.c_double), _P(RegionMeasurement)]),
    "svr_region_last_ms": (C.c_int, [_P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "svr_region_morph": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]),
    "svr_region_combine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "svr_region_reconstruct": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, _P(C.c_uint32)]),
    "svr_region_fill_holes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]),
    "svr_region_detach": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _P(C.c_int32), C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint32,
                                    C.c_void_p, _P(C.c_int32)]),
    "svr_region_mask_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_region_threshold": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, _P(C.c_int32), _P(C.c_int32),
                                       C.c_void_p]),
    "svr_region_label": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, _P(C.c_uint32)]),
    "svr_region_label_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]),
    "svr_region_select": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]),
    "svr_region_select_by_size": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                            _P(C.c_uint32)]),
    "svr_region_label_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_region_distance": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _P(C.c_uint32), C.c_int, C.c_void_p]),
    "svr_region_distance_select": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]),
    "svr_region_ball": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_uint32), C.c_uint32, C.c_void_p]),
    "svr_region_distance_max": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_int32)]),
    "svr_region_distance_volume": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]),
    "svr_region_distance_weights": (C.c_int, [_P(C.c_double), C.c_int, C.c_int, C.c_int, _P(C.c_uint32), _P(C.c_double)]),
    "svr_region_distance_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_region_distance_pass_ms": (C.c_int, [_P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "svr_volume_rank": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]),
    "svr_volume_smooth": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_uint32), C.c_void_p]),
    "svr_volume_smooth_radii": (C.c_int, [_P(C.c_double), C.c_double, _P(C.c_uint32), _P(C.c_double)]),
    "svr_volume_filter_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_region_geodesic_default_max_sweeps": (C.c_uint32, [C.c_int, C.c_int, C.c_int]),
    "svr_region_geodesic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(C.c_uint32), C.c_uint32, C.c_void_p, C.c_void_p, _P(C.c_uint32)]),
    "svr_region_seed_labels": (C.c_int, [_P(C.c_int32), C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "svr_region_geodesic_weights": (C.c_int, [_P(C.c_double), C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_uint32), _P(C.c_double)]),
    "svr_region_split": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _P(C.c_uint32), C.c_uint32, C.c_int, _P(C.c_uint32), C.c_uint32, C.c_void_p,
                                   _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32)]),
    "svr_region_zone_cut": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "svr_region_geodesic_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_region_growcut_params_default": (C.c_int, [_P(GrowcutParams), C.c_int]),
    "svr_region_growcut": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p, C.c_void_p, _P(GrowcutParams), C.c_void_p, C.c_void_p, _P(GrowcutInfo)]),
    "svr_region_seed_classes": (C.c_int, [_P(C.c_int32), _P(C.c_uint32), C.c_uint32, _P(C.c_int32), C.c_void_p]),
    "svr_region_label_paint": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_void_p, C.c_uint32, C.c_int]),
    "svr_region_growcut_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_histogram_params_default": (C.c_int, [_P(HistogramParams)]),
    "svr_histogram_bins": (C.c_uint32, [_P(HistogramParams)]),
    "svr_histogram_bin_range": (C.c_int, [_P(HistogramParams), C.c_uint32, _P(C.c_uint32), _P(C.c_uint32)]),
    "svr_volume_histogram": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p, _P(HistogramParams), C.c_void_p]),
    "svr_region_label_histogram": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), C.c_int, C.c_uint32, _P(HistogramParams), C.c_void_p]),
    "svr_volume_histogram_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_histogram_moments": (C.c_int, [C.c_void_p, C.c_uint32, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "svr_histogram_quantile": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _P(C.c_uint32)]),
    "svr_histogram_otsu": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _P(C.c_uint32), _P(C.c_double)]),
    "svr_region_surface": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "svr_region_overlap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, _P(C.c_uint64)]),
    "svr_region_label_overlap": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, _P(C.c_int32), C.c_void_p]),
    "svr_overlap_match": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _P(C.c_uint32), _P(C.c_uint32)]),
    "svr_region_distance_summary": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(C.c_uint32), C.c_uint32, _P(DistanceSummary)]),
    "svr_region_distance_histogram": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "svr_region_distance_quantile": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32), C.c_uint32, C.c_uint32, _P(C.c_uint32), _P(C.c_int32)]),
    "svr_compare_params_default": (C.c_int, [_P(CompareParams)]),
    "svr_region_compare": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(CompareParams), _P(RegionComparison)]),
    "svr_region_compare_measure": (C.c_int, [_P(RegionComparison), C.c_double, _P(CompareMeasurement)]),
    "svr_region_compare_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_scissor_params_default": (C.c_int, [_P(ScissorParams)]),
    "svr_stencil_rect": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(C.c_int32)]),
    "svr_stencil_polygon": (C.c_int, [_P(C.c_int32), _P(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "svr_scissor_project_camera": (C.c_int, [_P(cudaCamera), _P(vec3), _P(C.c_int32), _P(C.c_float)]),
    "svr_scissor_project_slice": (C.c_int, [_P(SliceParams), C.c_uint32, C.c_uint32, _P(vec3), _P(C.c_int32), _P(C.c_float)]),
    "svr_region_scissor_camera": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _P(cudaVolume), _P(cudaCamera), C.c_void_p, _P(ScissorParams),
                                            C.c_void_p]),
    "svr_region_scissor_slice": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _P(cudaVolume), _P(SliceParams), C.c_uint32, C.c_uint32,
                                           C.c_void_p, _P(ScissorParams), C.c_void_p]),
    "svr_region_scissor_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_fill_between_params_default": (C.c_int, [_P(FillBetweenParams)]),
    "svr_region_slice_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_uint64)]),
    "svr_region_slice_distance": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_uint32), _P(C.c_int32), C.c_int, C.c_void_p]),
    "svr_region_fill_between": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _P(FillBetweenParams), C.c_void_p, _P(FillBetweenInfo)]),
    "svr_region_fill_between_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_region_fill_between_pass_ms": (C.c_int, [_P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "svr_region_box_size": (C.c_uint32, [_P(C.c_uint32)]),
    "svr_region_smooth_radii": (C.c_int, [_P(C.c_double), C.c_double, _P(C.c_uint32), _P(C.c_double)]),
    "svr_region_box_count": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_uint32), C.c_void_p]),
    "svr_region_box_density": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_uint32), C.c_void_p]),
    "svr_region_smooth": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, _P(C.c_uint32), C.c_uint32, C.c_void_p, _P(C.c_uint64)]),
    "svr_region_label_smooth": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_uint32, _P(C.c_uint32), C.c_uint32, C.c_void_p, _P(C.c_uint64)]),
    "svr_region_smooth_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_overlay_style_default": (C.c_int, [_P(OverlayStyle)]),
    "svr_overlay_palette_default": (C.c_int, [_P(C.c_uint32), C.c_uint32]),
    "svr_slice_ids": (C.c_int, [C.c_void_p, _P(cudaVolume), C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, _P(SliceParams), C.c_uint32,
                                C.c_float, _P(OverlaySource)]),
    "svr_hit_ids": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, _P(cudaVolume), C.c_int, C.c_int, C.c_int, _P(OverlaySource)]),
    "svr_overlay_ids": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _P(OverlayStyle)]),
    "svr_overlay_slice": (C.c_int, [C.c_void_p, _P(cudaVolume), C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, _P(SliceParams), C.c_uint32,
                                    C.c_float, _P(OverlaySource), _P(OverlayStyle)]),
    "svr_overlay_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_mesh_params_default": (C.c_int, [_P(MeshParams)]),
    "svr_mesh_isosurface": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _P(MeshParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                      _P(MeshInfo)]),
    "svr_mesh_region": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _P(MeshParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _P(MeshInfo)]),
    "svr_mesh_measure": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _P(C.c_double), _P(C.c_int64), _P(C.c_double)]),
    "svr_mesh_positions": (C.c_int, [C.c_void_p, C.c_uint64, _P(C.c_double), _P(cudaVolume), C.c_void_p]),
    "svr_mesh_last_ms": (C.c_int, [_P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "svr_resample_grid_box": (C.c_int, [_P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(ResampleGrid)]),
    "svr_resample_grid_spacing": (C.c_int, [_P(C.c_int32), _P(C.c_double), _P(C.c_int32), _P(C.c_int32), _P(C.c_double), _P(ResampleGrid),
                                            _P(C.c_double)]),
    "svr_resample_grid_dims": (C.c_int, [_P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(ResampleGrid)]),
    "svr_resample_grid_place": (C.c_int, [_P(cudaVolume), _P(C.c_int32), _P(ResampleGrid), _P(cudaVolume)]),
    "svr_volume_resample": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, _P(ResampleGrid), C.c_int, C.c_void_p]),
    "svr_region_resample": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(ResampleGrid), C.c_void_p]),
    "svr_region_label_resample": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(ResampleGrid), C.c_void_p]),
    "svr_region_paste": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_int]),
    "svr_region_mask_expand": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int, C.c_void_p]),
    "svr_volume_resample_last_ms": (C.c_int, [_P(C.c_float)]),
    "svr_get_counters": (C.c_int, [_P(Counters)]),
    "svr_reset_counters": (C.c_int, []),
    "svr_get_kernel_time": (C.c_int, [_P(C.c_double), _P(C.c_uint64)]),
    "svr_reset_kernel_time": (C.c_int, []),
    "svr_device_info": (C.c_char_p, []),
    "svr_abi_version": (C.c_int, []),
    # include/svr_io.h: the host-side rows N1-N4
    "svr_mhd_read_header": (C.c_int, [C.c_char_p, _P(MhdHeader)]),
    "svr_mhd_read_elements": (C.c_int, [_P(MhdHeader), C.c_void_p, C.c_size_t]),
    "svr_volume_preprocess": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_double), C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_uint32, _P(VolumeInfo)]),
    "svr_load_mhd": (C.c_int, [C.c_char_p, C.c_int, _P(cudaVolume), _P(VolumeInfo), C.c_void_p, C.c_uint32]),
    "svr_volume_preprocess_last_ms": (C.c_int, [_P(C.c_float), _P(C.c_uint64)]),
    "svr_tf_build_table": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, _P(C.c_float)]),
    "svr_tf_save": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "svr_tf_load": (C.c_int, [C.c_char_p, C.c_void_p, _P(C.c_int), C.c_void_p, _P(C.c_int)]),
    "svr_hdr_load": (C.c_int, [C.c_char_p, _P(C.c_int), _P(C.c_int), C.c_void_p, C.c_size_t]),
    "svr_load_env_map": (C.c_int, [C.c_char_p, _P(cudaEnvironmentLight)]),
    "svr_mhd_write": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, _P(C.c_int32), _P(C.c_double), _P(C.c_double), C.c_int]),
    "svr_tga_write": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_void_p]),
    "svr_tga_encode": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "svr_stl_write": (C.c_int, [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "svr_ply_write": (C.c_int, [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
}

_lib = None


def library_path() -> Path:
    return LIB_PATH


def load() -> C.CDLL:
    """Load libsvr_hip.so and bind every prototype.  Raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m sunvolumerender_amd._build` "
            "(or __graft_entry__.build()).  There is no CPU fallback."
        )
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
