// svr_api.hip -- C-ABI layer of libsvr_hip.so (include/svr_abi.h): the context, errors, initialisation and shutdown, the scene setters,
// the options, the counters and the test hooks.  The rest of the layer lives in svr_api_*.hip, one file per concern, over the state of
// svr_api_state.hpp.
//
// Holds what the reference keeps in __constant__ globals (pathtracer.cu:34-68) as a
// per-process host-side scene, resolves the opaque texture handles into software-sampler
// descriptors, and launches the gfx950 kernels.  No CPU rendering path exists here: every
// entry point either launches HIP work or reports an error.
#include "svr_api_state.hpp"
#include "svr_hits.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

static_assert(sizeof(svr_vec3) == 12, "glm::vec3 layout");
static_assert(sizeof(svr_bbox) == 36, "cudaBBox layout");
static_assert(sizeof(svr_volume) == 112 && offsetof(svr_volume, tex) == 40 && offsetof(svr_volume, densityScale) == 48 &&
              offsetof(svr_volume, spacing) == 60 && offsetof(svr_volume, invSpacing) == 72 && offsetof(svr_volume, x_clip) == 84 &&
              offsetof(svr_volume, z_clip) == 100, "cudaVolume layout");
static_assert(sizeof(svr_transfer_function) == 16 && offsetof(svr_transfer_function, maxOpacity) == 8, "cudaTransferFunction layout");
static_assert(sizeof(svr_camera) == 76 && offsetof(svr_camera, pos) == 28 && offsetof(svr_camera, w) == 64, "cudaCamera layout");
static_assert(sizeof(svr_disk) == 28, "cudaDisk layout");
static_assert(sizeof(svr_area_light) == 44 && offsetof(svr_area_light, color) == 28 && offsetof(svr_area_light, intensity) == 40, "cudaAreaLight layout");
static_assert(sizeof(svr_environment_light) == 32 && offsetof(svr_environment_light, defaultRadiance) == 8 &&
              offsetof(svr_environment_light, intensity) == 20 && offsetof(svr_environment_light, offset) == 24, "cudaEnvironmentLight layout");
static_assert(sizeof(svr_render_params) == 16 && offsetof(svr_render_params, hdrBuffer) == 8, "RenderParams layout");
static_assert(sizeof(svr_counters) == 8 * svr::CNT_N, "counter block");
static_assert(sizeof(svr_denoise_params) == 28 && offsetof(svr_denoise_params, step) == 24, "svr_denoise_params layout");
static_assert(sizeof(svr_noise_estimate) == 48 && offsetof(svr_noise_estimate, tiles_x) == 16 && offsetof(svr_noise_estimate, pixels) == 24 &&
              offsetof(svr_noise_estimate, sse) == 40, "svr_noise_estimate layout");
static_assert(sizeof(svr::NoiseTotals) == 32, "noise totals");
static_assert(sizeof(svr_adaptive_result) == 64 && offsetof(svr_adaptive_result, pixel_frames) == 24 && offsetof(svr_adaptive_result, sse) == 48 &&
              offsetof(svr_adaptive_result, tile_max) == 60, "svr_adaptive_result layout");
static_assert(sizeof(svr_hit) == 40 && sizeof(svr_hit) == svr::HIT_WORDS * 4 && offsetof(svr_hit, sample) == 4 && offsetof(svr_hit, t) == 8 && offsetof(svr_hit, value) == 12 &&
              offsetof(svr_hit, position) == 16 && offsetof(svr_hit, normal) == 28, "svr_hit layout");
static_assert(sizeof(svr_hit_params) == 12 && offsetof(svr_hit_params, alpha) == 4 && offsetof(svr_hit_params, iso) == 8, "svr_hit_params layout");
static_assert(SVR_HIT_OPACITY == svr::HIT_OPACITY && SVR_HIT_ISO == svr::HIT_ISO && SVR_HIT_MAX == svr::HIT_MAX && SVR_HIT_STATUS_MISS == svr::HIT_STATUS_MISS &&
              SVR_HIT_STATUS_NONE == svr::HIT_STATUS_NONE && SVR_HIT_STATUS_FOUND == svr::HIT_STATUS_FOUND, "SVR_HIT_* constants");
static_assert(sizeof(svr_projection_params) == 20 && offsetof(svr_projection_params, flags) == 4 && offsetof(svr_projection_params, iso) == 8 &&
              offsetof(svr_projection_params, window_lo) == 12 && offsetof(svr_projection_params, window_hi) == 16, "svr_projection_params layout");
static_assert(sizeof(svr_slice_params) == 60 && offsetof(svr_slice_params, u) == 12 && offsetof(svr_slice_params, v) == 24 && offsetof(svr_slice_params, thickness) == 36 &&
              offsetof(svr_slice_params, step) == 40 && offsetof(svr_slice_params, mode) == 44 && offsetof(svr_slice_params, flags) == 48 &&
              offsetof(svr_slice_params, window_lo) == 52 && offsetof(svr_slice_params, window_hi) == 56, "svr_slice_params layout");

using namespace svr_host;

namespace svr_host {

Context g;
std::mutex g_mu;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g.err_code = code ? code : -1;
    g.err_msg = buf;
    if (g.fatal) {
        // utils/helper_cuda.h:966-977 behaviour: report and die
        fprintf(stderr, "libsvr_hip error %d: %s\n", g.err_code, buf);
        hipDeviceReset();
        exit(EXIT_FAILURE);
    }
    return g.err_code;
}

// record an error without the fatal-mode exit: misuse that cannot have corrupted anything (e.g. destroying a
// handle twice from a copied host object)
int soft_fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g.err_code = code ? code : -1;
    g.err_msg = buf;
    if (g.fatal) fprintf(stderr, "libsvr_hip warning %d: %s\n", g.err_code, buf);
    return g.err_code;
}

int ensure_init()
{
    if (g.inited) return 0;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail((int)e, "no HIP device available (hipGetDevice: %s)", hipGetErrorName(e));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    g.device = dev;
    g.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    char buf[256];
    snprintf(buf, sizeof buf, "%s %d.%d %s CUs=%d", prop.name, prop.major, prop.minor, prop.gcnArchName, g.num_cus);
    g.info = buf;
    HIP_TRY(hipMalloc((void**)&g.d_counters, sizeof(svr_counters) + DEBUG_WORDS * 8));       // + the phase profile of experiment builds
    HIP_TRY(hipMemset(g.d_counters, 0, sizeof(svr_counters) + DEBUG_WORDS * 8));
    HIP_TRY(hipMalloc((void**)&g.d_ticket, sizeof(uint32_t) * (svr::TICKET_SHARDS * svr::TICKET_STRIDE * (Context::NSETS + 1) + 64)));       // (+ 64 words behind the last set of task counters)
    HIP_TRY(hipMemset(g.d_ticket, 0, sizeof(uint32_t) * (svr::TICKET_SHARDS * svr::TICKET_STRIDE * (Context::NSETS + 1) + 64)));
    HIP_TRY(hipMalloc((void**)&g.d_mask, svr::ACCEL_WORDS * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&g.d_mask_tmp, 2 * (size_t)svr::MASK_WORDS_MAX * 32));
    for (int i = 0; i < Context::NSETS; ++i) {
        HIP_TRY(hipStreamCreateWithFlags(&g.sets[i].stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&g.sets[i].traced, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&g.sets[i].resolved, hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&g.queue_done, hipEventDisableTiming));
    for (int i = 0; i < Context::EV_RING; ++i) {
        HIP_TRY(hipEventCreate(&g.ev0[i]));
        HIP_TRY(hipEventCreate(&g.ev1[i]));
    }
    g.inited = true;
    return 0;
}

Texture* find_tex(uint64_t h, int kind)
{
    auto it = g.textures.find(h);
    if (it == g.textures.end()) return nullptr;
    Texture* t = it->second;
    if (t->magic != TEX_MAGIC || t->kind != kind) return nullptr;
    return t;
}

bool finite3(const svr_vec3& v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }

// argument checks that the image calls (ray caster, projection, slice) share; `who` is the name the message reports
int check_step(const char* who, float stepSize)
{
    if (!(stepSize > 0.f) || !std::isfinite(stepSize)) return fail(-3, "%s: stepSize must be finite and > 0 (got %g)", who, (double)stepSize);
    return 0;
}
int check_window(const char* who, float lo, float hi)
{
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo))
        return fail(-3, "%s: the window must be finite with window_hi > window_lo (got %g .. %g)", who, (double)lo, (double)hi);
    return 0;
}
// (the skipping argument of svr_walk.hpp, raw_bound, needs a monotone, non-negative sampler)
int check_density_scale(const char* who, float densityScale)
{
    if (!std::isfinite(densityScale) || densityScale < 0.f) return fail(-3, "%s: densityScale must be finite and >= 0 (got %g)", who, (double)densityScale);
    return 0;
}

} // namespace svr_host

// hooks for the other translation units of the library (svr_internal.hpp)
namespace svr {
int report_error(int code, const char* msg) { return fail(code, "%s", msg); }
int ensure_ready() { return ensure_init(); }
hipStream_t current_stream() { return g.stream; }
void image_work(DevWork& work, uint32_t W, uint32_t H, bool whole) { if (whole) fill_work_full(work, W, H); else fill_work(work, W, H); }
int device_cus() { return g.num_cus; }
}

extern "C" {

int svr_abi_version(void) { return 1; }

int svr_init(int device)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (g.inited && g.device == device) return 0;
    if (g.inited) return fail(-5, "svr_init(%d): already initialised on device %d (one scene per process, like the reference)", device, g.device);
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail((int)e, "hipSetDevice(%d) failed: %s", device, hipGetErrorName(e));
    return ensure_init();
}

void svr_shutdown(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g.inited) return;
    hipDeviceSynchronize();
    for (auto& kv : g.textures) free_texture(kv.second);
    g.textures.clear();
    for (auto& st : g.sets) {
        if (st.lbuf) hipFree(st.lbuf);
        for (auto& p : st.planes) if (p) hipFree(p);
        if (st.wf_counts) hipFree(st.wf_counts);
        if (st.stream) hipStreamDestroy(st.stream);
        if (st.traced) hipEventDestroy(st.traced);
        if (st.resolved) hipEventDestroy(st.resolved);
    }
    if (g.d_mask) hipFree(g.d_mask);
    if (g.d_mask_tmp) hipFree(g.d_mask_tmp);
    if (g.d_fine_mask) hipFree(g.d_fine_mask);
    if (g.d_sub8) hipFree(g.d_sub8);
    if (g.d_pick) hipFree(g.d_pick);
    if (g.d_bnd8) hipFree(g.d_bnd8);
    if (g.d_counters) hipFree(g.d_counters);
    if (g.d_ticket) hipFree(g.d_ticket);
    if (g.d_queue) hipFree(g.d_queue);
    if (g.d_pend) hipFree(g.d_pend);
    if (g.queue_done) hipEventDestroy(g.queue_done);
    if (g.d_guides) hipFree(g.d_guides);
    if (g.d_dn_scratch) hipFree(g.d_dn_scratch);
    if (g.ns.d_snap) hipFree(g.ns.d_snap);
    if (g.ns.buf.mem) hipFree(g.ns.buf.mem);
    if (g.nb_call.mem) hipFree(g.nb_call.mem);
    if (g.d_ad_list) hipFree(g.d_ad_list);
    free_stage();
    for (int i = 0; i < Context::EV_RING; ++i) {
        if (g.ev0[i]) hipEventDestroy(g.ev0[i]);
        if (g.ev1[i]) hipEventDestroy(g.ev1[i]);
    }
    int fatal = g.fatal;
    g = Context();
    g.fatal = fatal;
}

int svr_set_stream(void* hip_stream)
{
    if (ensure_init()) return g.err_code;
    HIP_TRY(hipDeviceSynchronize());
    collect_timing();
    for (auto& st : g.sets) st.used = false;
    g.stream = (hipStream_t)hip_stream;
    return 0;
}

int svr_device_synchronize(void)
{
    // canvas.cpp:106 synchronises so that the image can be shown: everything that touches the CALLER's buffers (accumulator, image, counters)
    // runs on the launch stream or is ordered into it with events.  Frames being traced ahead on the library's own streams write only the
    // library's scratch slots and are NOT waited for -- a host that synchronises after every render_pathtracer call (the reference's
    // paintGL) would otherwise stall on the next batch at every batch boundary.
    if (ensure_init()) return g.err_code;
    HIP_TRY(hipStreamSynchronize(g.stream));
    return 0;
}

void svr_set_error_mode(int fatal) { g.fatal = fatal ? 1 : 0; }
const char* svr_last_error(void) { return g.err_msg.c_str(); }
int svr_last_error_code(void) { return g.err_code; }
void svr_clear_error(void) { g.err_code = 0; g.err_msg.clear(); }
const char* svr_device_info(void) { ensure_init(); return g.info.c_str(); }

// ---------------- memory helpers ----------------
void* svr_device_malloc(size_t bytes)
{
    if (ensure_init()) return nullptr;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) { fail((int)e, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorName(e)); return nullptr; }
    return p;
}
int svr_device_free(void* p) { if (ensure_init()) return g.err_code; HIP_TRY(hipFree(p)); return 0; }
int svr_memcpy_h2d(void* dst, const void* src, size_t bytes) { if (ensure_init()) return g.err_code; HIP_TRY(hipStreamSynchronize(g.stream)); HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return 0; }
int svr_memcpy_d2h(void* dst, const void* src, size_t bytes) { if (ensure_init()) return g.err_code; HIP_TRY(hipStreamSynchronize(g.stream)); HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return 0; }
int svr_memset_device(void* dst, int value, size_t bytes) { if (ensure_init()) return g.err_code; HIP_TRY(hipMemsetAsync(dst, value, bytes, g.stream)); return 0; }

int svr_render_params_setup_hdr(svr_render_params* p, uint32_t w, uint32_t h)
{
    // render_parameters.h:17-23
    if (ensure_init()) return g.err_code;
    if (!p) return fail(-4, "svr_render_params_setup_hdr: null");
    if (svr_render_params_clear(p)) return g.err_code;
    size_t bytes = sizeof(float) * 3 * (size_t)w * h;
    HIP_TRY(hipMalloc(&p->hdrBuffer, bytes));
    HIP_TRY(hipMemset(p->hdrBuffer, 0, bytes));
    return 0;
}

int svr_render_params_clear(svr_render_params* p)
{
    // render_parameters.h:25-32
    if (ensure_init()) return g.err_code;
    if (p && p->hdrBuffer) {
        HIP_TRY(hipStreamSynchronize(g.stream));
        HIP_TRY(hipFree(p->hdrBuffer));
        p->hdrBuffer = nullptr;
    }
    return 0;
}

// ---------------- the reference's setup_* (pathtracer.cu:34-68) ----------------
void setup_volume(const svr_volume* vol)
{
    if (ensure_init()) return;
    if (!vol) { fail(-4, "setup_volume: null"); return; }
    g.vol = *vol; g.have_vol = true;
}
void setup_transferfunction(const svr_transfer_function* tf)
{
    if (ensure_init()) return;
    if (!tf) { fail(-4, "setup_transferfunction: null"); return; }
    g.tf = *tf; g.have_tf = true;
}
void setup_camera(const svr_camera* cam)
{
    if (ensure_init()) return;
    if (!cam) { fail(-4, "setup_camera: null"); return; }
    g.cam = *cam; g.have_cam = true;
}
void setup_env_lights(const svr_environment_light* light)
{
    if (ensure_init()) return;
    if (!light) { fail(-4, "setup_env_lights: null"); return; }
    g.env = *light;
}
void setup_area_lights(svr_area_light* lights, uint32_t n)
{
    if (ensure_init()) return;
    if (n > SVR_MAX_LIGHT_SOURCES) n = SVR_MAX_LIGHT_SOURCES;     // the reference's host guard is off by one (lights.cpp:94)
    if (n && !lights) { fail(-4, "setup_area_lights: null"); return; }
    g.num_lights = n;
    for (uint32_t i = 0; i < n; ++i) g.lights[i] = lights[i];
}

// ---------------- extensions ----------------
int svr_set_row_shard(uint32_t strip_rows, uint32_t rank, uint32_t world)
{
    if (world <= 1 || strip_rows == 0) { g.strip_rows = 0; g.rank = 0; g.world = 1; return 0; }
    if (rank >= world) return fail(-6, "svr_set_row_shard: rank %u >= world %u", rank, world);
    if (strip_rows % 8 != 0) return fail(-6, "svr_set_row_shard: strip_rows must be a multiple of 8 (got %u)", strip_rows);
    g.strip_rows = strip_rows; g.rank = rank; g.world = world;
    return 0;
}

int svr_set_render_window(int x0, int y0, int x1, int y1)
{
    g.wx0 = x0; g.wy0 = y0; g.wx1 = x1; g.wy1 = y1;
    return 0;
}

int svr_set_option(int key, int value)
{
    switch (key) {
    case SVR_OPT_ENV_ON_ESCAPE: g.opt_env_on_escape = value ? 1 : 0; return 0;
    case SVR_OPT_KERNEL:
        if (value < 0 || value > 4) return fail(-6, "SVR_OPT_KERNEL: bad value %d", value);
        g.opt_kernel = value; return 0;
    case SVR_OPT_COUNT: g.opt_count = value ? 1 : 0; return 0;
    case SVR_OPT_TIMING: g.opt_timing = value ? 1 : 0; return 0;
    case SVR_OPT_SKIP_TONEMAP: g.opt_skip_tonemap = value ? 1 : 0; return 0;
    case SVR_OPT_DENOISE_PREVIEW:
        if (value < 0) return fail(-6, "SVR_OPT_DENOISE_PREVIEW: bad value %d (0 = off, N > 0 = frames)", value);
        g.opt_denoise_preview = value; return 0;
    case SVR_OPT_NOISE_ESTIMATE:
        if (value != 0 && value != 1) return fail(-6, "SVR_OPT_NOISE_ESTIMATE: bad value %d (0 off, 1 on)", value);
        g.opt_noise_estimate = value; return 0;
    case SVR_OPT_BLOCKS_PER_CU:
        if (value < 0 || value > 8) return fail(-6, "SVR_OPT_BLOCKS_PER_CU: bad value %d", value);
        g.opt_blocks_per_cu = value; return 0;
    case SVR_OPT_PIPELINE: g.opt_pipeline = value ? 1 : 0; return 0;
    case SVR_OPT_EMPTY_SKIP: g.opt_empty_skip = value ? 1 : 0; return 0;
    case SVR_OPT_RAY_SKIP: g.opt_ray_skip = value ? 1 : 0; return 0;
    case SVR_OPT_BOUND_CULL:
        if (value < 0 || value > 2) return fail(-6, "SVR_OPT_BOUND_CULL: bad value %d (0 off, 1 auto, 2 always)", value);
        g.opt_bound_cull = value; return 0;
    case SVR_OPT_FOLD: g.opt_fold = value ? 1 : 0; return 0;
    case SVR_OPT_GROUP_FRAMES:
        if (value != 8 && value != 16 && value != 32 && value != 64 && value != 128 && value != 256)
            return fail(-6, "SVR_OPT_GROUP_FRAMES: bad value %d (8, 16, 32, 64, 128, 256)", value);
        g.opt_group_frames = value; return 0;
    case SVR_OPT_ROW_ORDER: g.opt_row_order = value ? 1 : 0; return 0;
    case SVR_OPT_FINE_MASK:
        if (value < 0 || value > 2) return fail(-6, "SVR_OPT_FINE_MASK: bad value %d (0 off, 1 auto, 2 always)", value);
        g.opt_fine_mask = value; return 0;
    case SVR_OPT_FAST_MATH: g.opt_fast_math = value ? 1 : 0; invalidate_ahead(); return 0;
    case SVR_OPT_LIGHT_CULL: g.opt_light_cull = value ? 1 : 0; return 0;
    case SVR_OPT_LM_SUBCELLS:
        if (value < 0 || value > 2) return fail(-6, "SVR_OPT_LM_SUBCELLS: bad value %d (0 off, 1 auto, 2 always)", value);
        g.opt_lm_sub = value; invalidate_ahead(); return 0;
    case SVR_OPT_LM_TUNE: {
        const int steps = value & 0xff, refill = (value >> 8) & 0xff, ended = (value >> 16) & 0xff, tasks = (value >> 24) & 0x7f;
        if (value != 0 && (steps < 1 || steps > 64 || refill < 1 || refill > 64 || ended < 1 || ended > 64 || tasks > 23 || value < 0)) return fail(-6, "SVR_OPT_LM_TUNE: bad value 0x%x (cells per turn | idle lanes << 8 | ended walks << 16, each 1..64, | tasks per batch of the depth-1 pool << 24, 0 = default .. 23)", value);
        g.opt_lm_tune = value; return 0;
    }
    case SVR_OPT_LOCAL_MAJORANT:
        if (value < 0 || value > 2) return fail(-6, "SVR_OPT_LOCAL_MAJORANT: bad value %d (0 off, 1 on, 2 on with straight-line paths only)", value);
        g.opt_local_majorant = value; invalidate_ahead(); return 0;
    case SVR_OPT_QUEUE:
        if (value < 0 || value > 2) return fail(-6, "SVR_OPT_QUEUE: bad value %d (0 off, 1 auto, 2 always)", value);
        g.opt_queue = value; g.queue_alloc_failed = false; return 0;
    case SVR_OPT_PINHOLE_FAST: g.opt_pinhole_fast = value ? 1 : 0; return 0;
    case SVR_OPT_POOL:
        if (value < 0 || value > 2) return fail(-6, "SVR_OPT_POOL: bad value %d (0 off, 1 auto, 2 always)", value);
        g.opt_pool = value; return 0;
    case SVR_OPT_TRIPS:
        if (value < 0 || value > 2) return fail(-6, "SVR_OPT_TRIPS: bad value %d (0 off, 1 auto, 2 always)", value);
        g.opt_trips = value; return 0;
    case SVR_OPT_PARK_CHEAP:
        if (value < 1 || value > 64) return fail(-6, "SVR_OPT_PARK_CHEAP: bad value %d (1..64)", value);
        g.opt_park_cheap = value; return 0;
    case SVR_OPT_PARK_END:
        if (value < 1 || value > 64) return fail(-6, "SVR_OPT_PARK_END: bad value %d (1..64)", value);
        g.opt_park_end = value; return 0;
    case SVR_OPT_SPLIT:
        if (value < 0 || value > 2) return fail(-6, "SVR_OPT_SPLIT: bad value %d (0 off, 1 or 2 on)", value);
        g.opt_split = value; return 0;
    case SVR_OPT_ENV_NEE: g.opt_env_nee = value ? 1 : 0; invalidate_ahead(); return 0;
    case SVR_OPT_NAN_GUARD: g.opt_nan_guard = value ? 1 : 0; return 0;
    case SVR_OPT_FAST_BOUND: g.opt_fast_bound = value ? 1 : 0; return 0;
    case SVR_OPT_MACRO_SHIFT_MIN:
        if (value < 0 || value > 6) return fail(-6, "SVR_OPT_MACRO_SHIFT_MIN: bad value %d (0..6)", value);
        g.opt_macro_shift_min = value; return 0;
#ifdef SVR_TEST_HOOKS
    // experiment builds only (tools/exp.py; `SVR_EXTRA_HIPCC_FLAGS=-DSVR_TEST_HOOKS python -m sunvolumerender_amd._build --force`)
    case 100: g.opt_debug_stop = value; return 0;      // timing ablation: stop every path after a phase (wrong images)
#endif
    case 101: g.opt_unit = value; return 0;            // tasks per ticket of the tile kernel (0: one; placement only -- tests/test_task_loop_gpu.py)
    case SVR_OPT_FRAME_AHEAD: g.opt_frame_ahead = value ? 1 : 0; invalidate_ahead(); return 0;
    case SVR_OPT_RAYCAST_LANES_LOG2:
        if (value < 0 || value > 5) return fail(-6, "SVR_OPT_RAYCAST_LANES_LOG2: bad value %d (0..5)", value);
        g.opt_rc_lanes = value; return 0;
    case SVR_OPT_FRAMES_PER_WAVE_LOG2:
        if (value < -1 || value > 6) return fail(-6, "SVR_OPT_FRAMES_PER_WAVE_LOG2: bad value %d (-1..6)", value);
        g.opt_frames_log2 = value; return 0;
    case SVR_OPT_REFILL_MIN_IDLE:
        if (value < 1 || value > 64) return fail(-6, "SVR_OPT_REFILL_MIN_IDLE: bad value %d (1..64)", value);
        g.opt_refill = value; return 0;
    default: return fail(-6, "svr_set_option: unknown key %d", key);
    }
}

int svr_get_option(int key)
{
    switch (key) {
    case SVR_OPT_ENV_ON_ESCAPE: return g.opt_env_on_escape;
    case SVR_OPT_KERNEL: return g.opt_kernel;
    case SVR_OPT_COUNT: return g.opt_count;
    case SVR_OPT_TIMING: return g.opt_timing;
    case SVR_OPT_SKIP_TONEMAP: return g.opt_skip_tonemap;
    case SVR_OPT_DENOISE_PREVIEW: return g.opt_denoise_preview;
    case SVR_OPT_NOISE_ESTIMATE: return g.opt_noise_estimate;
    case SVR_OPT_BLOCKS_PER_CU: return g.opt_blocks_per_cu;
    case SVR_OPT_PIPELINE: return g.opt_pipeline;
    case SVR_OPT_EMPTY_SKIP: return g.opt_empty_skip;
    case SVR_OPT_RAY_SKIP: return g.opt_ray_skip;
    case SVR_OPT_BOUND_CULL: return g.opt_bound_cull;
    case SVR_OPT_FOLD: return g.opt_fold;
    case SVR_OPT_GROUP_FRAMES: return g.opt_group_frames;
    case SVR_OPT_ROW_ORDER: return g.opt_row_order;
    case SVR_OPT_FINE_MASK: return g.opt_fine_mask;
    case SVR_OPT_FAST_MATH: return g.opt_fast_math;
    case SVR_OPT_LOCAL_MAJORANT: return g.opt_local_majorant;
    case SVR_OPT_LIGHT_CULL: return g.opt_light_cull;
    case SVR_OPT_LM_TUNE: return g.opt_lm_tune;
    case SVR_OPT_LM_SUBCELLS: return g.opt_lm_sub;
    case SVR_OPT_QUEUE: return g.opt_queue;
    case SVR_OPT_PARK_END: return g.opt_park_end;
    case SVR_OPT_PARK_CHEAP: return g.opt_park_cheap;
    case SVR_OPT_PINHOLE_FAST: return g.opt_pinhole_fast;
    case SVR_OPT_POOL: return g.opt_pool;
    case SVR_OPT_TRIPS: return g.opt_trips;
    case SVR_OPT_SPLIT: return g.opt_split;
    case SVR_OPT_ENV_NEE: return g.opt_env_nee;
    case SVR_OPT_FAST_BOUND: return g.opt_fast_bound;
    case SVR_OPT_NAN_GUARD: return g.opt_nan_guard;
    case SVR_OPT_MACRO_SHIFT_MIN: return g.opt_macro_shift_min;
    case SVR_OPT_REFILL_MIN_IDLE: return g.opt_refill;
    case SVR_OPT_FRAMES_PER_WAVE_LOG2: return g.opt_frames_log2;
    case SVR_OPT_RAYCAST_LANES_LOG2: return g.opt_rc_lanes;
    case SVR_OPT_FRAME_AHEAD: return g.opt_frame_ahead;
    case 101: return g.opt_unit;
    default: return -1;
    }
}

// test hook (not part of the rendering API): runs the ray caster's chain primitives on n items of (t, h, bound, steps)
int svr_selftest_chain(const float* items, float* results, uint32_t n)
{
    if (ensure_init()) return g.err_code;
    if (!items || !results || n == 0) return fail(-4, "svr_selftest_chain: bad arguments");
    float4* d_buf = nullptr;                                  // items, then results
    HIP_TRY(hipMalloc((void**)&d_buf, (size_t)n * 32));
    hipError_t e = hipMemcpy(d_buf, items, (size_t)n * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = svr::launch_chain_selftest(d_buf, d_buf + n, n, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e == hipSuccess) e = hipMemcpy(results, d_buf + n, (size_t)n * 16, hipMemcpyDeviceToHost);
    hipFree(d_buf);
    if (e != hipSuccess) return fail((int)e, "svr_selftest_chain failed: %s", hipGetErrorName(e));
    return 0;
}

// test hook: device-side known-answer tests of the numeric contract (csrc/svr_selftest.hip)
int svr_selftest_math(int fn, const float* in, uint32_t in_stride, float* out, uint32_t n)
{
    if (ensure_init()) return g.err_code;
    if (!in || !out || n == 0 || in_stride == 0 || in_stride > 4) return fail(-4, "svr_selftest_math: bad arguments");
    float* d_in = nullptr; float* d_out = nullptr;
    HIP_TRY(hipMalloc((void**)&d_in, (size_t)n * in_stride * sizeof(float)));
    hipError_t e = hipMalloc((void**)&d_out, (size_t)n * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d_in, in, (size_t)n * in_stride * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = svr::launch_math_selftest(fn, d_in, in_stride, d_out, n, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    hipFree(d_in);
    if (d_out) hipFree(d_out);
    if (e != hipSuccess) return fail((int)e, "svr_selftest_math(%d) failed: %s", fn, hipGetErrorName(e));
    return 0;
}

// test hook: property test of the fast bound look-up on the CURRENT scene (set up as for render_pathtracer): csrc/svr_selftest.hip
int svr_selftest_bound8(const float* rays, uint32_t n, uint32_t* out)
{
    if (ensure_init()) return g.err_code;
    if (!rays || !out || n == 0) return fail(-4, "svr_selftest_bound8: bad arguments");
    if (!g.have_vol || !g.have_tf || !g.have_cam) return fail(-4, "svr_selftest_bound8 before setup_volume/setup_transferfunction/setup_camera");
    svr::DevScene s;
    if (build_scene(g.vol, g.tf, g.cam, s)) return g.err_code;
    if (ensure_mask(s, g.vol, g.tf)) return g.err_code;
    if (s.bnd8 == nullptr) return fail(-3, "svr_selftest_bound8: the fast bound look-up is not in use for this scene");
    float* d_rays = nullptr; uint32_t* d_out = nullptr;
    HIP_TRY(hipMalloc((void**)&d_rays, (size_t)n * 7 * sizeof(float)));
    hipError_t e = hipMalloc((void**)&d_out, (size_t)n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(d_rays, rays, (size_t)n * 7 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = svr::launch_bound8_selftest(s, d_rays, n, d_out, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    hipFree(d_rays);
    if (d_out) hipFree(d_out);
    if (e != hipSuccess) return fail((int)e, "svr_selftest_bound8 failed: %s", hipGetErrorName(e));
    return 0;
}

// test hook: property test of the shared whole-ray march on the CURRENT scene and image size: csrc/svr_selftest.hip
int svr_selftest_group_march(uint32_t frame0, uint64_t out[8])
{
    if (ensure_init()) return g.err_code;
    if (!out) return fail(-4, "svr_selftest_group_march: bad arguments");
    if (!g.have_vol || !g.have_tf || !g.have_cam) return fail(-4, "svr_selftest_group_march before setup_volume/setup_transferfunction/setup_camera");
    svr::DevScene s;
    if (build_scene(g.vol, g.tf, g.cam, s)) return g.err_code;
    if (ensure_mask(s, g.vol, g.tf)) return g.err_code;
    if (s.empty_mask == nullptr || !s.ray_skip) return fail(-3, "svr_selftest_group_march: the scene has no whole-ray test (SVR_OPT_EMPTY_SKIP off, or a clip box beyond the volume)");
    unsigned long long* d_out = nullptr;
    HIP_TRY(hipMalloc((void**)&d_out, 8 * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_out, 0, 8 * sizeof(unsigned long long), g.stream);
    if (e == hipSuccess) e = svr::launch_group_march_selftest(s, frame0, d_out, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    hipFree(d_out);
    if (e != hipSuccess) return fail((int)e, "svr_selftest_group_march failed: %s", hipGetErrorName(e));
    return 0;
}

// test hook: the skipping tables of the CURRENT scene as the kernels will read them (tests/accel_ref.py restates them in numpy)
int svr_selftest_accel(int table, void* out, size_t out_bytes, int32_t info[16])
{
    if (ensure_init()) return g.err_code;
    if (!info || table < 0 || table > 7 || (table != 0 && !out)) return fail(-4, "svr_selftest_accel: bad arguments");
    if (!g.have_vol || !g.have_tf || !g.have_cam) return fail(-4, "svr_selftest_accel before setup_volume/setup_transferfunction/setup_camera");
    svr::DevScene s;
    if (build_scene(g.vol, g.tf, g.cam, s)) return g.err_code;
    if (ensure_mask(s, g.vol, g.tf)) return g.err_code;
    const Texture* tv = find_tex(g.vol.tex, TEX_VOLUME);
    if (s.empty_mask == nullptr || !tv) return fail(-3, "svr_selftest_accel: the scene has no acceleration data (SVR_OPT_EMPTY_SKIP off?)");
    const int hgx = (tv->mc_gx + 1) / 2, hgy = (tv->mc_gy + 1) / 2, hgz = (tv->mc_gz + 1) / 2;
    const size_t n = (size_t)tv->mc_gx * tv->mc_gy * tv->mc_gz, hn = (size_t)hgx * hgy * hgz;
    const size_t fn = tv->mm_fine ? (size_t)tv->fg_x * tv->fg_y * tv->fg_z : 0;
    const int32_t filled[16] = {tv->mc_shift, tv->mc_gx, tv->mc_gy, tv->mc_gz, hgx, hgy, hgz, tv->mm_fine ? tv->fg_x : 0, tv->mm_fine ? tv->fg_y : 0,
                                tv->mm_fine ? tv->fg_z : 0, (int32_t)s.mask_words, (int32_t)s.dist_words, (g.bnd8_valid ? 1 : 0) | (s.bnd8 ? 2 : 0),
                                g.sub8_valid ? 1 : 0, (int32_t)svr::ACCEL_WORDS, (int32_t)svr::BOUND8_BYTES};
    memcpy(info, filled, sizeof filled);
    const void* src = nullptr;
    size_t bytes = 0;
    switch (table) {
    case 0: return 0;
    case 1: src = tv->mm; bytes = n * 2 * sizeof(uint16_t); break;
    case 2: src = tv->mm_fine; bytes = fn * 2 * sizeof(uint16_t); break;
    case 3: src = tv->mm_wide; bytes = hn * 2 * sizeof(uint16_t); break;
    case 4: src = g.d_mask; bytes = (size_t)svr::ACCEL_WORDS * sizeof(uint32_t); break;
    case 5: src = tv->mm_fine ? g.d_fine_mask : nullptr; bytes = (fn + 31) / 32 * sizeof(uint32_t); break;
    case 6: src = g.sub8_valid ? g.d_sub8 : nullptr; bytes = n; break;
    default: src = g.bnd8_valid ? g.d_bnd8 : nullptr; bytes = svr::BOUND8_BYTES; break;
    }
    if (!src) return fail(-3, "svr_selftest_accel: the scene has no table %d", table);
    if (out_bytes != bytes) return fail(-4, "svr_selftest_accel: table %d has %zu bytes, not %zu", table, bytes, out_bytes);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

#ifdef SVR_TEST_HOOKS
// experiment builds: the lane machine's phase profile (svr_lanes.hpp), n <= 32 words, cleared by svr_reset_counters
extern "C" int svr_debug_phase_profile(uint64_t* out, int n)
{
    if (ensure_init()) return g.err_code;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, g.d_counters + svr::CNT_N, sizeof(uint64_t) * (size_t)(n < (int)DEBUG_WORDS ? n : (int)DEBUG_WORDS), hipMemcpyDeviceToHost));
    return 0;
}
#endif

int svr_get_counters(svr_counters* out)
{
    if (ensure_init()) return g.err_code;
    if (!out) return fail(-4, "svr_get_counters: null");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, g.d_counters, sizeof(svr_counters), hipMemcpyDeviceToHost));
    return 0;
}

int svr_reset_counters(void)
{
    if (ensure_init()) return g.err_code;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(g.d_counters, 0, sizeof(svr_counters) + DEBUG_WORDS * 8));
    return 0;
}

int svr_get_kernel_time(double* total_ms, uint64_t* launches)
{
    if (ensure_init()) return g.err_code;
    collect_timing();
    if (total_ms) *total_ms = g.kernel_ms;
    if (launches) *launches = g.kernel_launches;
    return 0;
}

int svr_reset_kernel_time(void)
{
    if (ensure_init()) return g.err_code;
    collect_timing();
    g.kernel_ms = 0.0;
    g.kernel_launches = 0;
    return 0;
}

} // extern "C"
