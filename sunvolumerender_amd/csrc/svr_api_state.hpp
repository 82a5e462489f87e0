// svr_api_state.hpp -- the host state of the C-ABI layer and what its translation units (svr_api.hip, svr_api_*.hip) share: the context,
// error reporting, the argument checks and the functions that cross files.  Host only, and for those files only: the volume-op files keep
// to svr_internal.hpp.
#pragma once
#include "../../include/svr_abi.h"
#include "svr_kernels.hpp"
#include "svr_noise.hpp"

#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace svr_host {

enum TexKind { TEX_VOLUME = 1, TEX_TF = 2, TEX_ENV = 3 };
constexpr size_t DEBUG_WORDS = 32;

struct Texture {
    uint32_t magic;
    int kind;
    void* data;          // device
    int nx, ny, nz;      // volume dims / tf n / env w,h
    int layout;
    int sy, sz, bnx, bny;
    size_t bytes;
    // volume: per-macro-cell min/max of the raw voxels (empty-space skipping)
    uint16_t* mm = nullptr;
    int mc_shift = 0, mc_gx = 0, mc_gy = 0, mc_gz = 0;
    // a second, finer level (macro-cells of half the edge) when the LDS-resident grid is coarse (mc_shift >= 1): its `empty`
    // bits live in global memory and are consulted for fetches in cells the coarse level cannot rule out
    uint16_t* mm_fine = nullptr;
    uint16_t* nbmax = nullptr;         // largest raw voxel over a macro-cell and its neighbours (leaps of svr_render_projection; built at its first call)
    uint32_t nb_zero = 0;              // ... and how many macro-cells have an all-zero neighbourhood (where a mean projection can leap)
    uint16_t* mm_wide = nullptr;       // min/max per HALF-resolution macro-cell over a footprint one voxel wider per side (the fast bound look-up, svr_accel.hip k_bound8)
    int fg_x = 0, fg_y = 0, fg_z = 0;
    // environment map: sampling table of SVR_OPT_ENV_NEE (svr_kernels.hip launch_env_cdf), built with the texture
    float* env_cdf = nullptr;
    // transfer function: prefix count of exactly-zero alphas of the padded table, and an edit counter
    uint32_t* zero_prefix = nullptr;
    uint64_t version = 0;
};
constexpr uint32_t TEX_MAGIC = 0x53565254u;   // "SVRT"
// defaults of the denoised preview (include/svr_abi.h, svr_denoise_params): the setting of the sweep over small_head, c3 and c2 at 1 and 4 spp
// (tools/denoise_sweep.py, profiles/denoise_sweep.txt) with the smallest worst-case drift of the mean luminance whose RMSE ratios all stay below 0.6
constexpr svr_denoise_params DN_DEFAULT = {5, 0.5f, 32.f, 0.4f, 0.8f, 0.f, 0.f};

struct Context {
    bool inited = false;
    int device = -1;
    hipStream_t stream = nullptr;
    int num_cus = 256;
    std::string info;
    // scene (the reference's __constant__ globals)
    bool have_vol = false, have_tf = false, have_cam = false;
    svr_volume vol{};
    svr_transfer_function tf{};
    svr_camera cam{};
    svr_environment_light env{};
    uint32_t num_lights = 0;
    svr_area_light lights[SVR_MAX_LIGHT_SOURCES]{};
    // options
    int opt_env_on_escape = 0, opt_kernel = 0, opt_count = 0, opt_timing = 0, opt_skip_tonemap = 0, opt_blocks_per_cu = 0;
    // sharding
    uint32_t strip_rows = 0, rank = 0, world = 1;
    int wx0 = 0, wy0 = 0, wx1 = -1, wy1 = -1;
    // device scratch
    unsigned long long* d_counters = nullptr;
    uint32_t* d_ticket = nullptr;
    uint32_t* d_queue = nullptr;        // scatter-record queues of the tile kernel's folding launches (they run one at a time)
    float* d_pend = nullptr;            // ... and the waves' pending-radiance rows
    uint32_t queue_blocks = 0;          // blocks both are sized for
    bool queue_alloc_failed = false;    // SVR_OPT_QUEUE = 1 and the device had no room for them: straight-line launches
    hipEvent_t prev_traced = nullptr;   // `traced` event of the latest trace launch (owned by its set)
    hipEvent_t queue_done = nullptr;    // recorded behind every launch that uses d_queue / d_pend (there is ONE such memory: its users run one after the other, on whatever stream)
    bool queue_used = false;
    // frames traced ahead of the host's render_pathtracer calls (render_frames)
    struct Ahead {
        bool valid = false;
        svr::DevScene scene;
        svr::DevWork shape;             // window / shard of the launch
        uint64_t content = 0;
        uint32_t first = 0, count = 0, depth = 0;
        int set = -1;
    } ahead[2];                         // the batch being consumed and the one traced while it is consumed
    uint64_t content_version = 0;       // bumped whenever texture contents or handles change
    int opt_frame_ahead = 1;
    // Frame pipelining: a render call is cut into groups of <= GROUP frames; each group is traced on
    // one of NSETS internal streams into that set's scratch slots and resolved (running mean + tone map)
    // on the caller's stream, so the trace kernels of consecutive frames/calls overlap on the GPU while
    // the accumulator is still updated strictly in frame order.
#ifndef SVR_GROUP
#define SVR_GROUP 32     // frames per trace launch: 8 / 16 / 32 / 64 measured 0.185 / 0.178 / 0.166 / 0.161 ms per frame on c3
#endif
    static constexpr int NSETS = 4, GROUP = SVR_GROUP;
    static constexpr int AHEAD_MAX = 64;                     // frames per launch of the steady state of frame-ahead tracing (a wave = one pixel x 64 frames, like a folding launch)
    static constexpr uint64_t CHAIN_MIN_PATHS = 12u << 20;   // paths of a trace launch from which launches are chained
    struct SlotSet {
        float* lbuf = nullptr;
        hipStream_t stream = nullptr;
        hipEvent_t traced = nullptr, resolved = nullptr;
        bool used = false;
        float4* planes[svr::WF_QUEUE_PLANES] = {};   // wavefront queues (allocated on first use)
        uint32_t* wf_counts = nullptr;
    } sets[NSETS];
    size_t queue_capacity = 0;
    size_t slot_floats = 0;        // floats per scratch slot currently allocated (3*W*H)
    uint32_t slots_per_set = 0;    // slots currently allocated per set
    int next_set = 0;
    int opt_pipeline = 1;             // SVR_OPT_PIPELINE
    int opt_refill = 16;              // SVR_OPT_REFILL_MIN_IDLE
    int opt_empty_skip = 1;           // SVR_OPT_EMPTY_SKIP
    int opt_ray_skip = 1;             // SVR_OPT_RAY_SKIP
    int opt_debug_stop = 0;           // key 100, SVR_TEST_HOOKS builds only
    int opt_frames_log2 = -1;         // SVR_OPT_FRAMES_PER_WAVE_LOG2
    int opt_unit = 0;                 // key 101
    int opt_rc_lanes = 3;             // SVR_OPT_RAYCAST_LANES_LOG2
    int opt_bound_cull = 1;           // SVR_OPT_BOUND_CULL
    int opt_park_end = 32;            // SVR_OPT_PARK_END
    int opt_fold = 1;                 // SVR_OPT_FOLD
    int opt_queue = 1;                // SVR_OPT_QUEUE
    int opt_fast_math = 0;            // SVR_OPT_FAST_MATH
    int opt_fine_mask = 0;            // SVR_OPT_FINE_MASK
    int opt_row_order = 0;            // SVR_OPT_ROW_ORDER
    int opt_group_frames = 256;       // SVR_OPT_GROUP_FRAMES
    int opt_local_majorant = 0;       // SVR_OPT_LOCAL_MAJORANT
    int opt_light_cull = 1;           // SVR_OPT_LIGHT_CULL
    int opt_lm_tune = 0;              // SVR_OPT_LM_TUNE
    int opt_lm_sub = 1;               // SVR_OPT_LM_SUBCELLS
    int opt_park_cheap = 16;          // SVR_OPT_PARK_CHEAP
    int opt_pinhole_fast = 1;         // SVR_OPT_PINHOLE_FAST
    int opt_pool = 1;                 // SVR_OPT_POOL
    int opt_trips = 1;                // SVR_OPT_TRIPS
    int opt_nan_guard = 0;            // SVR_OPT_NAN_GUARD
    int opt_macro_shift_min = 0;      // SVR_OPT_MACRO_SHIFT_MIN
    int opt_split = 0;                // SVR_OPT_SPLIT
    int opt_env_nee = 0;              // SVR_OPT_ENV_NEE
    int opt_fast_bound = 1;           // SVR_OPT_FAST_BOUND
    // empty-space bitmask of the current (volume, transfer function, densityScale)
    uint32_t* d_mask = nullptr;
    uint32_t* d_fine_mask = nullptr;   // `empty` bits of the fine level (global memory), sized for the current volume
    size_t fine_mask_words = 0;
    uint8_t* d_bnd8 = nullptr;         // byte table of the fast bound look-up (svr::BOUND8_BYTES)
    uint8_t* d_sub8 = nullptr;         // occupancy of the fine cells inside every macro-cell (local-majorant walks), MASK_WORDS_MAX * 32 bytes
    bool sub8_valid = false;
    bool bnd8_valid = false;
    uint8_t* d_mask_tmp = nullptr;     // scratch of the distance transform
    uint32_t* d_pick = nullptr;        // device copy of svr_pick's pixel list (SVR_PICK_MAX pairs; allocated at the first pick)
    bool mask_valid = false;
    uint64_t mask_vol = 0, mask_tf = 0, mask_tf_version = 0;
    uint32_t mask_ds_bits = 0, mask_sigma_bits = 0;
    bool mask_cull_useful = false, mask_has_empty = true;
    uint32_t mask_words = 0;
    // denoised preview (SVR_OPT_DENOISE_PREVIEW, svr_denoise.hip): the guides of the current scene, cached under what they depend on -- the
    // scene PODs of build_scene (volume, transfer function, camera, image size; not lights, not the env map), the transfer function's edit
    // counter, the march step and the skipping mode -- and the filter's ping-pong scratch
    int opt_denoise_preview = 0;
    svr_denoise_params dn = DN_DEFAULT;
    float4* d_guides = nullptr;
    size_t guides_px = 0;
    bool guides_valid = false;
    svr::DevScene guides_key{};
    uint64_t guides_vol = 0, guides_tf = 0, guides_tf_version = 0;
    float guides_h = 0.f;
    int guides_skip = -1;
    uint64_t guide_builds = 0;
    float4* d_dn_scratch = nullptr;
    size_t dn_scratch_px = 0;
    // noise estimate (SVR_OPT_NOISE_ESTIMATE, svr_noise.hip): the render it follows, its snapshot A(m) and the latest estimate.  A tracked
    // render is a run of consecutive render calls (render_calls counts every call) on one accumulator, size, shape and trace depth
    int opt_noise_estimate = 0;
    uint64_t render_calls = 0;
    struct NoiseBuf {                   // per-tile results + totals of one estimate: totals | tile_sse | tile_rmse | tile_cnt, one allocation
        void* mem = nullptr;
        size_t tiles = 0;
        svr::NoiseTotals* totals() const { return (svr::NoiseTotals*)mem; }
        double* sse() const { return (double*)((char*)mem + sizeof(svr::NoiseTotals)); }
        float* rmse() const { return (float*)(sse() + tiles); }
        uint32_t* cnt() const { return (uint32_t*)(rmse() + tiles); }
    };
    struct Noise {
        bool tracking = false, unavailable = false;
        uint64_t call = 0;              // render_calls after the last tracked call
        void* hdr = nullptr;
        uint32_t W = 0, H = 0, depth = 0;
        svr::DevWork shape{};
        uint32_t last_n = 0;            // frame count at the end of the last tracked call
        uint32_t m = 0;                 // frames in the snapshot; 0 = none yet
        bool have = false;              // an estimate of this render exists (in buf, on the stream)
        uint32_t est_n = 0, est_m = 0, tiles_x = 0, tiles_y = 0;
        float* d_snap = nullptr;
        size_t snap_px = 0;
        NoiseBuf buf;
    } ns;
    NoiseBuf nb_call;                   // svr_estimate_noise
    // adaptive sampling (svr_render_pathtracer_adaptive): the device tile list + active map of its launches (one allocation: ad_cap uint32 list
    // entries, then ad_cap bytes), and the per-tile results of the last call
    uint32_t* d_ad_list = nullptr;
    uint8_t* d_ad_map = nullptr;
    size_t ad_cap = 0;
    uint32_t ad_len = 0;
    bool ad_have = false;
    uint32_t ad_tx = 0, ad_ty = 0;
    std::vector<uint32_t> ad_frames;
    std::vector<float> ad_rmse;
    // ring of HIP event pairs around the path-tracing kernel (SVR_OPT_TIMING); drained lazily so the
    // timed launches never synchronise with the host
    static constexpr int EV_RING = 512;
    hipEvent_t ev0[EV_RING] = {}, ev1[EV_RING] = {};
    int ev_head = 0, ev_count = 0;
    double kernel_ms = 0.0;
    uint64_t kernel_launches = 0;
    // textures
    std::unordered_map<uint64_t, Texture*> textures;
    // errors
    int fatal = 1;
    int err_code = 0;
    std::string err_msg;
};

extern Context g;      // svr_api.hip

// nothing traced ahead of the calls (render_ahead) may be shown any more
inline void invalidate_ahead() { g.ahead[0].valid = g.ahead[1].valid = false; }

// ---- svr_api.hip ----
int fail(int code, const char* fmt, ...);
int soft_fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail((int)_e, "HIP error at %s:%d code=%d(%s) \"%s\"", __FILE__, __LINE__, \
                        (int)_e, hipGetErrorName(_e), #expr);                              \
    } while (0)

int ensure_init();
Texture* find_tex(uint64_t h, int kind);
bool finite3(const svr_vec3& v);
int check_step(const char* who, float stepSize);
int check_window(const char* who, float lo, float hi);
int check_density_scale(const char* who, float densityScale);

// ---- svr_api_texture.hip ----
void free_texture(Texture* t);
int ensure_nbmax(const char* who, Texture* tv);

// ---- svr_api_scene.hip ----
void use_macro_grid(svr::DevScene& s, const Texture* tv);
int build_scene(const svr_volume& vol, const svr_transfer_function& tf, const svr_camera& cam, svr::DevScene& s);
int add_lights_env(svr::DevScene& s);
int fill_work(svr::DevWork& w, uint32_t W, uint32_t H);
void fill_work_full(svr::DevWork& w, uint32_t W, uint32_t H);
int image_scene(const svr_volume& vol, const svr_transfer_function& tf, const svr_camera& cam, void* img, svr::DevScene& s, svr::DevWork& w);
bool partial_frame(uint32_t W, uint32_t H);
int ensure_mask(svr::DevScene& s, const svr_volume& vol, const svr_transfer_function& tf);
bool leaps_allowed(const svr::DevScene& s, const svr_volume& vol, const Texture* tv, float mc_scale[3]);
int fill_march_tables(const char* who, svr::DevScene& s, const svr_volume& vol, Texture* tv, svr::MarchTables& tb);

// ---- svr_api_trace.hip ----
// The launches of an adaptive call (svr_render_pathtracer_adaptive).  Such a call never traces frames ahead; once a tile has frozen
// (list set) its launches trace the listed tiles only.
struct TileList {
    const uint32_t* list = nullptr;     // active tiles, packed tx | ty << 16, in centre-out tile-row order (null: the whole frame)
    uint32_t count = 0;                 // entries of list
    const uint8_t* active = nullptr;    // per-tile map, 1 = traced
};
void collect_timing();
bool same_shape(const svr::DevWork& a, const svr::DevWork& b);
int render_frames_traced(void* img, const svr_render_params* rp, uint32_t nframes, bool tonemap, const TileList* adaptive);
int show_full_frame(void* img, const void* hdr, bool denoise);
int render_frames(void* img, const svr_render_params* rp, uint32_t nframes, bool tonemap);

// ---- svr_api_converge.hip ----
int denoise_frame(void* img, float* hdr_out, const void* hdr, uint32_t W, uint32_t H, const svr_denoise_params& p, bool soft, bool& ok);
int noise_after_render(const svr_render_params* rp, uint32_t nframes, uint64_t call);

// ---- svr_api_dist.hip ----
void free_stage();

} // namespace svr_host
