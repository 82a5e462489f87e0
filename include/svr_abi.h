/*
 * svr_abi.h -- C ABI of libsvr_hip.so, the MI355X (gfx950) drop-in for the render
 * launch of sunwj/SunVolumeRender.
 *
 * Plain C: POD structs, plain pointers and sizes, no C++/torch types.  Two groups:
 *
 *  (A) The seven entry points of the reference's device layer, with the SAME symbol
 *      names, so host code written against the reference (gui/canvas.cpp) links
 *      unchanged.  In the reference they are `extern "C"` functions taking C++
 *      references (pathtracer.h:17-24, raycasting.h:8); a reference is a pointer at
 *      the ABI level, so the C prototypes below are binary-identical.  The POD
 *      structs reproduce the reference classes byte for byte;
 *      include/sunvolumerender/host_api.hpp gives C++ hosts the reference's class
 *      names and methods over these layouts.
 *
 *  (B) svr_* helpers that stand in for the CUDA runtime calls the reference's HOST
 *      code makes around that layer (texture objects, cudaMalloc of the HDR buffer,
 *      device selection), plus documented extensions (render window for tile
 *      sharding, multi-frame batches, counters, timing).  gfx950 has no texture
 *      hardware exposed to HIP, so a "texture object" here is an opaque handle to a
 *      software-sampler descriptor; it is carried in the same 64-bit field the
 *      reference uses for cudaTextureObject_t.
 *
 * Error behaviour: the reference's functions return void and die through
 * checkCudaErrors (utils/helper_cuda.h:966-977: print, cudaDeviceReset, exit).  The
 * default here is the same (print to stderr, exit(EXIT_FAILURE)); with
 * svr_set_error_mode(0) errors are recorded instead and readable through
 * svr_last_error()/svr_last_error_code(), and svr_* functions return non-zero.
 *
 * Threading: like the reference (global __constant__ scene, pathtracer.cu:34-68) the
 * scene is per-process, per-device state; calls are not re-entrant.
 */
#ifndef SVR_ABI_H
#define SVR_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_MAX_LIGHT_SOURCES 8            /* common.h:11 */
#define SVR_TF_TABLE_SIZE 1024             /* gui/transferfunction.h:29 */

/* ---- POD layouts (all 4-byte floats; glm::vec3 is a packed 12-byte triple) ---- */
typedef struct svr_vec2 { float x, y; } svr_vec2;
typedef struct svr_vec3 { float x, y, z; } svr_vec3;

typedef struct svr_bbox {                  /* cudaBBox, core/geometry/cuda_bbox.h:66-69; 36 B */
    svr_vec3 vmin, vmax, invSize;
} svr_bbox;

typedef struct svr_volume {                /* cudaVolume, core/cuda_volume.h:111-121; 112 B, align 8 */
    svr_bbox bbox;                         /*   0 */
    uint32_t _pad0;                        /*  36 */
    uint64_t tex;                          /*  40  handle from svr_create_volume_texture */
    float densityScale;                    /*  48 */
    float invMaxMagnitude;                 /*  52 */
    float gradientFactor;                  /*  56 */
    svr_vec3 spacing;                      /*  60 */
    svr_vec3 invSpacing;                   /*  72 */
    svr_vec2 x_clip, y_clip, z_clip;       /*  84, 92, 100 */
    uint32_t _pad1;                        /* 108 */
} svr_volume;

typedef struct svr_transfer_function {     /* cudaTransferFunction, core/cuda_transfer_function.h:57-59; 16 B */
    uint64_t tex;                          /* handle from svr_create_tf_texture */
    float maxOpacity;                      /* Woodcock majorant */
    uint32_t _pad;
} svr_transfer_function;

typedef struct svr_camera {                /* cudaCamera, core/cuda_camera.h:98-106; 76 B */
    uint32_t imageW, imageH;
    float exposure, apeture, focalLength, aspectRatio, tanFovxOverTwo;
    svr_vec3 pos, u, v, w;
} svr_camera;

typedef struct svr_disk {                  /* cudaDisk, core/geometry/cuda_disk.h:58-61; 28 B */
    float radius;
    svr_vec3 center, normal;
} svr_disk;

typedef struct svr_area_light {            /* cudaAreaLight, core/lights/cuda_arealight.h:68-71; 44 B */
    svr_disk disk;
    svr_vec3 color;
    float intensity;
} svr_area_light;

typedef struct svr_environment_light {     /* cudaEnvironmentLight, core/lights/cuda_environment_light.h:74-78; 32 B */
    uint64_t tex;                          /* 0 = constant defaultRadiance; else handle from svr_create_env_texture */
    svr_vec3 defaultRadiance;
    float intensity;
    svr_vec2 offset;
} svr_environment_light;

typedef struct svr_render_params {         /* RenderParams, core/render_parameters.h:34-37; 16 B */
    uint32_t traceDepth;                   /* default 1 */
    uint32_t frameNo;                      /* default 0 */
    void* hdrBuffer;                       /* device pointer, W*H packed float3 (glm::vec3*) */
} svr_render_params;

/* =====================================================================
 * (A) the reference's device-layer entry points (same symbol names)
 * ===================================================================== */

#ifndef SVR_ABI_NO_REFERENCE_PROTOTYPES   /* host_api.hpp re-declares these seven with the reference's C++ signatures */
/* pathtracer.h:17 / pathtracer.cu:292-304.  One call = one sample per pixel: clears the
 * accumulator iff frameNo==0, traces one path per pixel with seed wangHash(frameNo) +
 * y*W + x, folds it into the running mean in hdrBuffer and tone-maps into img (device
 * pointer, W*H RGBA8).  W,H come from the last setup_camera (the reference bakes 640x640,
 * common.h:8-9).  Asynchronous on the launch stream, like the reference. */
void render_pathtracer(void* img, const svr_render_params* renderParams);

/* pathtracer.h:20-24 / pathtracer.cu:34-68: copy the POD into the per-device scene. */
void setup_volume(const svr_volume* vol);
void setup_transferfunction(const svr_transfer_function* tf);
void setup_camera(const svr_camera* cam);
void setup_env_lights(const svr_environment_light* light);
void setup_area_lights(svr_area_light* lights, uint32_t n);   /* n is clamped to SVR_MAX_LIGHT_SOURCES */

/* raycasting.h:8 / raycasting.cu:15-75: emission-absorption ray caster; scene passed by
 * argument, not through the setup_* state, as in the reference. */
void render_raycasting(void* img, svr_volume* volume, svr_transfer_function* transferFunction,
                       svr_camera* camera, float stepSize);
#endif /* SVR_ABI_NO_REFERENCE_PROTOTYPES */

/* =====================================================================
 * (B) helpers replacing the CUDA runtime calls of the reference's host code
 * ===================================================================== */

/* main.cpp:7-33 chooseBestDevice + cudaSetDevice: select the HIP device for this process. */
int svr_init(int device);
void svr_shutdown(void);
/* launch stream for every kernel (a hipStream_t; NULL = the null stream).  Lets a host
 * that owns streams (e.g. PyTorch) order the renderer with its own work. */
int svr_set_stream(void* hip_stream);
int svr_device_synchronize(void);                     /* canvas.cpp:106 cudaDeviceSynchronize */

void svr_set_error_mode(int fatal);                   /* 1 (default): checkCudaErrors behaviour */
const char* svr_last_error(void);
int svr_last_error_code(void);
void svr_clear_error(void);

/* VolumeReader.cpp:138-172 (cudaMalloc3DArray + cudaMemcpy3D + cudaCreateTextureObject,
 * border / linear / normalized-float / normalized coords): voxels is [nz][ny][nx] u16.
 * src_is_device: voxels is a device pointer.  layout: SVR_LAYOUT_*.  Returns 0 on error. */
#define SVR_LAYOUT_AUTO 0
#define SVR_LAYOUT_LINEAR 1          /* [z][y][x] with a 2-voxel zero apron */
#define SVR_LAYOUT_BRICK 2           /* 8x4x4-voxel bricks (256 B), 2-voxel zero apron */
#define SVR_LAYOUT_PAIR 3            /* the same bricks with 32-bit elements: voxel x | voxel x+1 << 16 (half the gather instructions per
                                        trilinear fetch, twice the memory; 32-bit byte offsets: volumes up to ~1000^3); what AUTO falls back to
                                        when CELL does not fit the addressing limits or the device memory */
#define SVR_LAYOUT_CELL 4            /* the same bricks with 16-byte elements: the 8 voxels of a trilinear cell -- one 16-byte load per fetch, one
                                     * sector instead of four; 8 x the memory of the u16 volume (2.2 GB for 512^3, 17 GB for 1024^3); 32-bit element
                                     * index, 64-bit byte offsets.  What AUTO picks FIRST (then PAIR, then BRICK, then LINEAR: the next one when
                                     * the addressing limits or hipErrorOutOfMemory rule one out; csrc/svr_api_texture.hip, create_volume_texture) */
uint64_t svr_create_volume_texture(const uint16_t* voxels, int nx, int ny, int nz,
                                   int src_is_device, int layout);
/* gui/transferfunction.cpp:30-44 (1D float4 array, clamp / linear / normalized coords). */
uint64_t svr_create_tf_texture(const float* rgba, int n, int src_is_device);
/* gui/transferfunction.cpp:128-176: re-upload after an edit (same n). */
int svr_update_tf_texture(uint64_t handle, const float* rgba, int n, int src_is_device);
/* core/lights/lights.cpp:41-74 (2D float4 array, wrap / linear / normalized coords). */
uint64_t svr_create_env_texture(const float* rgba, int w, int h, int src_is_device);
int svr_destroy_texture(uint64_t handle);             /* cudaDestroyTextureObject + cudaFreeArray */

/* core/render_parameters.h:17-32: RenderParams::SetupHDRBuffer / Clear. */
int svr_render_params_setup_hdr(svr_render_params* p, uint32_t w, uint32_t h);
int svr_render_params_clear(svr_render_params* p);

void* svr_device_malloc(size_t bytes);
int svr_device_free(void* p);
int svr_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes);
int svr_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes);   /* canvas.cpp:100 */
int svr_memset_device(void* dst_device, int value, size_t bytes);

/* ---- documented extensions (not in the reference) ---- */

/* Restrict render_pathtracer / render_raycasting to the rows y with
 * (y / strip_rows) % world == rank (interleaved row strips; multi-GPU tile sharding).
 * Seeds stay global (y*W+x), so the union over ranks is bit-identical to one GPU.
 * strip_rows=0 or world<=1 resets to the full frame. */
int svr_set_row_shard(uint32_t strip_rows, uint32_t rank, uint32_t world);
/* Restrict to the pixel window [x0,x1) x [y0,y1) (combined with the row shard). Negative x1/y1 = full. */
int svr_set_render_window(int x0, int y0, int x1, int y1);

/* ---- frame assembly for row-sharded renders: the native counterpart of sunvolumerender_amd/dist.py's FrameAssembler ----
 * A rank's accumulator holds the rows it owns (svr_set_row_shard) and zeros elsewhere.  The rows of rank r, in increasing
 * y, form its PACKED buffer: svr_strip_rows_owned() rows of W x float3.  One collective per output frame: every rank packs
 * and sends its rows to `root`, root unpacks them into the full frame -- with RCCL one point-to-point transfer per peer
 * over its own xGMI link (1.5 MB per peer at 1024^2 on 8 GPUs).
 * The two index functions are plain host code (no GPU needed). */
uint32_t svr_strip_rows_owned(uint32_t H, uint32_t strip_rows, uint32_t rank, uint32_t world);
/* y of the p-th owned row (p < svr_strip_rows_owned); 0xffffffff if p is out of range */
uint32_t svr_strip_row_to_y(uint32_t p, uint32_t H, uint32_t strip_rows, uint32_t rank, uint32_t world);
/* device buffers, on the library's stream: packed <- the rows of `rank` out of the full-size W x H x float3 `hdr`, and back */
int svr_pack_strips(void* packed, const void* hdr, uint32_t W, uint32_t H, uint32_t strip_rows, uint32_t rank, uint32_t world);
int svr_unpack_strips(void* frame, const void* packed, uint32_t W, uint32_t H, uint32_t strip_rows, uint32_t rank, uint32_t world);
/* The whole exchange, for a host that holds an RCCL communicator (one process per GPU, as with sunvolumerender_amd.dist):
 * nccl_comm = the host's ncclComm_t (world ranks; rank / world must be its rank / size).  Every rank packs its rows of
 * hdr_local (its accumulator; not modified) and ncclSend()s them to `root`; root ncclRecv()s the peers' rows and unpacks all of
 * them into frame_on_root (W x H x float3, device; ignored on the other ranks).  Enqueued on the library's stream
 * (svr_set_stream); the staging buffer is the library's.  RCCL is resolved at the first call from the library the process
 * has already loaded (dlopen("librccl.so")), so libsvr_hip.so itself does not link against it.
 * Afterwards svr_hdr_to_ldr_frame(img, frame_on_root, W, H) tone-maps the assembled frame on root. */
int svr_assemble_frame(void* nccl_comm, void* frame_on_root, const void* hdr_local, uint32_t W, uint32_t H,
                       uint32_t strip_rows, uint32_t rank, uint32_t world, uint32_t root);

#define SVR_OPT_ENV_ON_ESCAPE 1   /* 1: add T*env(dir) when a path leaves the volume (the line the reference
                                     comments out, pathtracer.cu:233).  default 0 = reference behaviour */
#define SVR_OPT_KERNEL 2          /* 0 auto (= 2); 1 one block per 16x16 tile (reference-shaped baseline);
                                     2 persistent waves, one 8x8 tile-task per wave, empty-space skipping (default);
                                     3 persistent waves with per-lane state machine and ballot/mbcnt lane regeneration;
                                     4 wavefront: gen / walk / shade kernels over dense queues with ballot + prefix-sum compaction */
#define SVR_OPT_COUNT 3           /* 1: count volume taps etc. (slower; for roofline accounting) */
#define SVR_OPT_TIMING 4          /* 1: bracket the path-tracing kernel with HIP events */
#define SVR_OPT_SKIP_TONEMAP 5    /* 1: render_pathtracer does not run hdr_to_ldr (batch rendering) */
#define SVR_OPT_BLOCKS_PER_CU 6   /* persistent kernel: workgroups per CU (0 = default) */
#define SVR_OPT_PIPELINE 7        /* 1 (default): trace kernels of consecutive frame groups run on internal streams
                                     and overlap; the accumulator is still updated in frame order on the caller's
                                     stream.  0: everything on the caller's stream */
#define SVR_OPT_EMPTY_SKIP 9       /* 1 (default): skip the voxel fetches of Woodcock iterations in macro-cells where the
                                     transfer function is exactly transparent (bit-identical results; RNG still advanced) */
#define SVR_OPT_RAY_SKIP 10        /* 1 (default): per-ray conservative march over the dilated empty mask: a walk that can
                                     never meet a non-transparent macro-cell ends at once when no random draw follows it,
                                     and other walks skip cell tests up to their first possibly-occupied cell (bit-identical) */
#define SVR_OPT_BOUND_CULL 15       /* 0 off, 1 (default) where it pays (>= 2 % of the occupied coarse macro-cells have a bound below 1), 2 always:
                                     majorant-bound fetch culling -- a Woodcock iteration draws its accept number first and
                                     fetches only if it is below (largest alpha reachable in the macro-cell) / sigma_max; bit-identical
                                     results, same random-number stream (csrc/svr_accel.hip, k_bound_class) */
#define SVR_OPT_PARK_END 19         /* lane machine of the tile kernel at traceDepth > 1 (csrc/svr_lanes.hpp): a round of services (BSDF sampling /
                                     shading of the waiting paths) runs when this many lanes of the wave could be put to work by it (or none
                                     walks); 1..64, default 32.  Speed only */
#define SVR_OPT_QUEUE 18            /* the tile kernel shades the first scatter events of a task in place, queues the paths and continues them on a
                                     per-lane state machine that keeps the 64 lanes of a wave walking (csrc/svr_lanes.hpp): 0 never, 2 always (on
                                     folding launches), 1 (default) where it pays: empty-space skipping on and traceDepth >= 2, a medium without
                                     exactly transparent space, or a launch large enough to drain every wave's queue 4 times.  Results identical */
#define SVR_OPT_FOLD 17             /* 1 (default): a many-frame launch of the tile kernel folds its frames into the HDR accumulator itself (running
                                     mean in frame order, in the wave that traced them); 0: scratch slot per frame + resolve kernel */
#define SVR_OPT_FAST_MATH 14        /* OPT-IN, default 0: the tile kernel's fast-math build (v_log_f32 in the walk, reciprocal division, fma contraction;
                                     in the spirit of the reference's -use_fast_math, CMakeLists.txt:9-10).  NOT bit-identical to the default mode:
                                     converged images agree within Monte-Carlo noise (tests/test_fast_math_gpu.py) */
#define SVR_OPT_FINE_MASK 20        /* second, finer level of `empty` macro-cells (half the edge) in global memory for the per-fetch test:
                                     0 (default) off, 1 when the LDS-resident cells are >= 16 voxels (volumes beyond 512^3), 2 whenever it exists.
                                     Fewer fetches (c5: 3.9 instead of 5.9 per path), same speed: the test costs a dependent cached load */
#define SVR_OPT_ROW_ORDER 21        /* tile kernel work distribution: 1 = each of the 8 ticket counters (one per XCD group of blocks) owns whole tile
                                     rows, so neighbouring tiles share an XCD's L2; 0 = every 8th task.  Speed only */
#define SVR_OPT_GROUP_FRAMES 22     /* frames per folding launch of svr_render_pathtracer_frames: 8, 16, 32 or 64 (default: a wave = one pixel x 64 frames); 128 or 256: that many frames in one launch, as whole groups of 64, where the call's kernel has the form for it (depth 1, empty-space skipping, pinhole camera, full grid), 64 elsewhere.  Speed only */
#define SVR_OPT_LOCAL_MAJORANT 23   /* OPT-IN, default 0: "Woodcock max-density acceleration" -- the free-flight sampler tracks against per-macro-cell
                                     * (local) majorants instead of the reference's single global one (core/woodcock_tracking.h:29-31): same law of the
                                     * collision point, far fewer iterations, but a different consumption of random numbers.  NOT bit-identical to
                                     * the default mode; converged images agree within Monte-Carlo noise (tests/test_local_majorant_gpu.py).  Needs
                                     * SVR_OPT_EMPTY_SKIP = 1 and clip planes inside the volume; otherwise the default kernel renders.
                                     * Meant for volumes >= 512^3 at >= 1024^2 pixels, fog-like media and deeper paths (c3n 2.1 x, c5 + 34 %, c3 + 8 %, depth 4 + 9 %); on a
                                     * 256^3 volume at 512^2 (c2) the default kernel has little left to skip and the pool's batches cost more than they save: - 24 % there.
                                     * 1 = the pool kernels; 2 = the straight-line form of the same algorithm (identical results, slower: the
                                     * reference the pool kernels are tested against) */
#define SVR_OPT_LIGHT_CULL 24       /* 1 (default): area lights that no camera ray can reach (behind the lens plane or outside the view frustum, lens
                                     * and pixel jitter included; conservative host-side test) are skipped by the primary rays' nearest-light test
                                     * (core/lights/light_sample.h:23-49).  Results unchanged */
#define SVR_OPT_LM_TUNE 25          /* local-majorant pool kernel, speed only: macro-cells a walking lane may cross per turn | idle lanes that trigger a
                                     * refill << 8 | ended walks that trigger their settling << 16 (each 1..64) | tasks per batch of the traceDepth-1 pool << 24
                                     * (0 = the default for the scene; < 16 selects the 10-task build, >= 16 the 21-task build); 0 (default) = everything chosen per scene */
#define SVR_OPT_LM_SUBCELLS 26      /* local-majorant mode: a walk spends its free path only in the occupied eighths (2 x 2 x 2 fine cells) of a macro-cell --
                                     * fewer wasted tentative collisions where a surface cuts a cell.  0 off, 1 (default) where macro-cells are >= 16 voxels
                                     * (volumes beyond 512^3), 2 always.  Changes the random numbers a path
                                     * consumes (another, equally valid estimate), so it is part of the mode's definition, not a speed-only switch */
#define SVR_OPT_PARK_CHEAP 27       /* lane machine of the tile kernel at traceDepth 1: ended shadow walks + idle lanes with a record waiting before the wave
                                     * settles / refills them (1..64, default 16).  Speed only */
#define SVR_OPT_PINHOLE_FAST 28     /* 1 (default): with apeture == 0 (the reference's default) the camera ray skips the square root and the sine / cosine of
                                     * the lens sample, which is (+-0, +-0) and provably changes no bit of the ray; the draws are consumed.  Results unchanged */
#define SVR_OPT_POOL 29             /* tile kernel with the queue machine: the primary walks are pooled too (a task only generates its camera
                                     * rays; the lane machine walks them, the collisions are shaded 64 at a time).  0 off, 1 (default) for media without
                                     * exactly transparent space (their walks are not coherent within a wave), 2 always.  Results unchanged */
#define SVR_OPT_TRIPS 30            /* lane machine of the tile kernel (pooled walks at traceDepth 1, every walk of deeper paths): the walking lanes run FIVE
                                     * Woodcock iterations per turn with the generator as a circular buffer (no register moves), a lane that needs a fetch waits
                                     * for the end of the trip.  0 off, 1 (default) for media without exactly transparent space, 2 always.  Results unchanged */
#define SVR_OPT_NAN_GUARD 31        /* OPT-IN, default 0 = the reference's behaviour: running_estimate (pathtracer.cu:81-84,279) keeps a NaN for good, and the
                                     * reference's own arithmetic yields one (0/0 in the microfacet term, pathtracer.cu:106-131, core/bsdf/microfacet.h:52-68) for a
                                     * handful of paths in 10^8..10^9 -- a permanently dead pixel.  1: a non-finite sample (per channel) is replaced by the running mean
                                     * before it is folded in, i.e. dropped.  Every other sample and pixel keeps its bits */
#define SVR_OPT_MACRO_SHIFT_MIN 32  /* volume textures created from now on get macro-cells of at least 2^v voxels per axis (0..6; default 0 = the smallest cells
                                     * whose grid fits 64^3).  Coarser acceleration data; the default mode's results are unchanged (bit-exact), the local-majorant
                                     * mode's estimate changes with its grid.  For tests of the coarse-grid code paths on small volumes */
#define SVR_OPT_SPLIT 33            /* RETIRED, default 0; 0 / 1 / 2 are accepted and stored, and select nothing.  It chose a two-kernel form of many-frame launches of
                                     * deeper paths whose results were always identical to the one-kernel form's, and which ran 0.5-1.5 % behind it with a record pool of up
                                     * to 14 GB.  The one-kernel form now serves these launches whatever the value */
#define SVR_OPT_ENV_NEE 34          /* OPT-IN, default 0: importance sampling of the environment MAP (csrc/svr_trace_env.hip).  With SVR_OPT_ENV_ON_ESCAPE the environment lights the
                                     * medium only through the directions the BSDF / phase sampling picks (core/lights/cuda_environment_light.h:58-72 is a lookup, nothing more).
                                     * 1: every scatter event that is followed by a bounce also draws one direction from the map's luminance (a table built on the GPU by
                                     * svr_create_env_texture), walks a shadow ray along it and combines the two estimates with the balance heuristic.  Same image in expectation
                                     * -- the reference's throughput update, reported pdfs and roulette are reproduced term by term (tests/test_env_nee_gpu.py: means within 4
                                     * standard errors at 4 096 spp) -- far less noise under a small bright sun; NOT bit-identical (the path's random stream shifts).  Needs an
                                     * env texture, SVR_OPT_ENV_ON_ESCAPE = 1 and traceDepth >= 2; otherwise inert.  Straight-line paths: about half the speed of the default kernel */
#define SVR_OPT_FAST_BOUND 35       /* default 1: media without exactly transparent space (walks of tens of iterations under bound culling: the pooled lane machine of the tile
                                     * kernel) look the fetch bound of an iteration up from the ray parameter -- one fma per axis into a byte table whose cells cover one more
                                     * voxel per side, compared with the top 8 bits of the accept draw's random word (csrc/svr_accel.hip k_bound8) -- instead of from the exact
                                     * trilinear cell and a class threshold.  Any valid bound culls correctly: results unchanged (bit-exact); c3n +17 %, c3n at depth 2 / 4 +32 % / +31 % (same box).  Needs the clipped box inside the volume and the camera within 2^21 / (16 N) volume extents (else, and with 0: the exact cell) */
#define SVR_OPT_DENOISE_PREVIEW 36    /* default 0 = off.  N > 0: render_pathtracer and svr_render_pathtracer_frames write an edge-aware DENOISED tone map to img
                                     * while the frame shown has at most N samples per pixel (frameNo + nframes <= N), the ordinary one after that
                                     * (svr_denoise_to_ldr with the parameters of svr_set_denoise_params; csrc/svr_denoise.hip).  Only the RGBA8 image changes:
                                     * the accumulator (hdrBuffer) is never written by the filter, so convergence and bit-exactness are untouched.  Inert
                                     * under a row shard, a render window or SVR_OPT_SKIP_TONEMAP.  If the guide / scratch memory cannot be allocated the
                                     * frame gets the ordinary tone map and svr_last_error() says so (no error code: the render does not fail) */
#define SVR_OPT_NOISE_ESTIMATE 37      /* 0 (default) = off (no memory, no launch, no state change); 1: render_pathtracer and svr_render_pathtracer_frames follow the
                                     * render and estimate its remaining noise from the accumulator alone (csrc/svr_noise.hip; see svr_noise_estimate below).
                                     * A call with frameNo 0, a frameNo that is not the previous call's end, or another hdrBuffer / image size / window /
                                     * shard / trace depth starts a new render; the first call that ends at n >= 4 frames takes a snapshot A(m) = A(n)
                                     * (12 B per pixel, allocated once), every later call that ends at n >= 2m estimates A(n) against it and takes
                                     * the snapshot A(n), m = n: estimates at 8, 16, 32 ... frames for one frame per call.  Everything runs on the
                                     * library's stream behind the call; the accumulator and the image are unchanged.  If the memory cannot be
                                     * allocated there is no estimate and svr_last_error() says so (no error code: the render does not fail) */
#define SVR_OPT_FRAME_AHEAD 13           /* render_pathtracer traces frames ahead of the calls that ask for them (batches of 1, 2, 4 ... 32 frames; results unchanged); default 1 */
#define SVR_OPT_RAYCAST_LANES_LOG2 12   /* ray caster: 1 << v adjacent lanes share one ray (samples of a chunk in parallel, composited in order); 0..5, default 3 */
#define SVR_OPT_FRAMES_PER_WAVE_LOG2 11 /* tile kernel: a wave traces (64 >> f) pixels x (1 << f) frames of a group; -1 (default) = up to 8 frames */
#define SVR_OPT_REFILL_MIN_IDLE 8 /* persistent kernel: regenerate lanes once this many of a wave's 64 lanes are idle
                                     (64 = a wave finishes its 8x8 tile before taking the next; default) */
int svr_set_option(int key, int value);
int svr_get_option(int key);

/* render_pathtracer for nframes consecutive frame numbers (renderParams->frameNo ...
 * +nframes-1) in ONE launch; bit-identical to nframes calls, tone-maps once at the end. */
int svr_render_pathtracer_frames(void* img, const svr_render_params* renderParams, uint32_t nframes);

/* hdr_to_ldr alone (pathtracer.cu:282-290), over the pixels this process owns (row shard / window). */
int svr_hdr_to_ldr(void* img, const svr_render_params* renderParams);
/* hdr_to_ldr over a WHOLE w x h frame, whatever shard or window is set: the tone map of the frame rank 0 has
 * assembled from the ranks' strips (hdr: device pointer, w*h packed float3; exposure of the last setup_camera). */
int svr_hdr_to_ldr_frame(void* img, const void* hdr, uint32_t w, uint32_t h);

typedef struct svr_counters {
    uint64_t paths;
    uint64_t vol_taps;         /* 8-voxel trilinear fetches of the algorithm (what the reference issues) */
    uint64_t woodcock_iters;
    uint64_t scatter_events;
    uint64_t shadow_walks;
    uint64_t raycast_steps;
    uint64_t loop_iters;       /* persistent kernels: wave-level scheduler iterations / tile tasks */
    uint64_t vol_taps_executed; /* fetches actually issued (<= vol_taps: empty-space skipping, reused scatter tap) */
    uint64_t walks_ray_skipped; /* Woodcock walks a non-counting build ends at once (whole-ray test) */
    uint64_t iters_ray_skipped; /* ... and the Woodcock iterations those walks contain */
    uint64_t iters_prefix_skipped; /* iterations before a walk's first possibly-occupied macro-cell (no cell test) */
    uint64_t taps_bound_culled; /* fetches of non-empty cells not issued because the accept draw was above the cell's bound */
} svr_counters;
/* test hook: the ray caster's sample-chain replay on n items (t, h, bound, steps) -> (count <, count <=, t after steps, flags) */
int svr_selftest_chain(const float* items, float* results, uint32_t n);
/* test hook: device-side known-answer tests of the numeric contract.  out[i] = fn(in[i*in_stride ...]) evaluated by the
 * device functions the kernels use: 0 schlick_fresnel(ni, no, cos)  1 logf  2 expf  3 sinf  4 cosf  5 acosf
 * 6 atan2f(y, x)  7 powf(x, y)  8 k-th curand_uniform of curand_init(seed bits, 0, 0): in = (seed bits, k)
 * 9 wangHash(bits) as bits  10 log(1 - u) of the Woodcock walk (logf_unit) */
int svr_selftest_math(int fn, const float* in, uint32_t in_stride, float* out, uint32_t n);
/* test hook: property test of SVR_OPT_FAST_BOUND's table on the scene set up as for render_pathtracer.  rays = n x 7 floats (origin, direction, u):
 * at the point t = tMin + u (tMax - tMin) of the ray's box interval, the byte the lane machine would read against the product the reference's
 * accept test forms there (exact cell, fetch, alpha, invSigmaMax).  out[i] = 1 tested | 2 VIOLATION (a draw the byte culls could be accepted)
 * | 4 index outside the table | byte << 8; 0 = the ray misses the box.  Fails (-3) when the look-up is not in use for the scene */
int svr_selftest_bound8(const float* rays, uint32_t n, uint32_t* out);
/* test hook: property test of the whole-ray march that neighbouring pixels share (csrc/svr_walk.hpp, walk_setup_shared) on the scene and image size set
 * up as for render_pathtracer: the set-up of the primary walk for every pixel, row by row from left to right, x the frames frame0 .. frame0 + 63; every
 * lane that hits the box then walks its ray in steps of 1/8 macro-cell and counts the points that the returned parameter or the map calls clear but
 * that lie in a macro-cell which is not empty.  out = { VIOLATIONS (must be 0), points tested, marches for a pixel pair, reuses of a kept march,
 * kept marches refused, marches for a pixel that cannot share, lanes that hit the box, lanes with a valid map }.  Fails (-3) without whole-ray tests */
int svr_selftest_group_march(uint32_t frame0, uint64_t out[8]);
/* The macro-cell grid a volume texture of nx x ny x nz voxels gets (plain host code, no GPU needed): the smallest shift >= shift_min whose grid
 * (ceil(n / 2^shift) cells per axis) has at most 64^3 cells AND whose half-resolution grid (ceil(g / 2) per axis: the 4-bit distance and
 * bound-class tables) has at most 32^3 -- a flat or line-like volume is limited by the second.  out = { shift, gx, gy, gz, hgx, hgy, hgz,
 * words of the packed half-resolution tables }.  Returns the shift, -1 on bad arguments */
int svr_macro_grid(int nx, int ny, int nz, int shift_min, int out[8]);
/* test hook: the skipping tables of the scene set up as for render_pathtracer, copied to the host exactly as the kernels read them.
 * info (always filled) = { shift, gx, gy, gz, hgx, hgy, hgz, fgx, fgy, fgz (0 without a fine level), mask_words, dist_words,
 * bound8 (1 built | 2 in use for this scene), sub8 built, words of the accel buffer, bytes of the bound8 table }.
 * table: 0 none (info only)  1 mm (gx gy gz x {min, max} u16)  2 mm_fine (fgx fgy fgz x 2 u16)  3 mm_wide (hgx hgy hgz x 2 u16)
 * 4 the accel buffer (u32: dist | deep | empty | classes | thresholds | census)  5 fine `empty` bits (ceil(fgx fgy fgz / 32) u32)
 * 6 sub8 (gx gy gz bytes)  7 bound8 (bytes).  out_bytes must be the table's size; -3 when the scene has no such table */
int svr_selftest_accel(int table, void* out, size_t out_bytes, int32_t info[16]);
/* ---- denoised preview (SVR_OPT_DENOISE_PREVIEW; csrc/svr_denoise.hip) ----
 * GUIDES: one deterministic ray per pixel (the pinhole centre ray, cuda_camera.h:85-95) is marched through the clipped box
 * (the path tracer's interval, tNear < 0 -> 1e-6) at a fixed step h with the path tracer's extinction sigma = TF alpha of
 * volume(p): first-collision weight w_i = T_i (1 - exp(-sigma_i h)), T_{i+1} = T_i exp(-sigma_i h), T_0 = 1, until T < 2^-10.
 * Per pixel 8 floats, two float4: [0] = (N.x, N.y, N.z, D), [1] = (A.r, A.g, A.b, O) with opacity O = sum w, expected depth
 * D = sum w t / O, albedo A = sum w rgb_TF / O, normal N = normalize(sum w grad) (the central-difference gradient,
 * cuda_volume.h:54-61; 0 if the sum is 0).  O == 0 (the ray misses the box or sees only exactly transparent medium):
 * D = -1, N = 0, A = 1.  Cached; recomputed only when the scene PODs (volume, transfer function, camera, image size), the
 * transfer function's contents, the march step or SVR_OPT_EMPTY_SKIP change -- not for lights or the environment.
 * FILTER: edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) over c = hdr / max(A, 1e-3), `passes` passes at steps
 * 1, 2, 4 ..., 5 x 5 B3-spline taps (1/16, 1/4, 3/8, 1/4, 1/16), weights normalised per pixel.  Weight of q for p (q != p):
 *   h(q) exp(-( |D_p - D_q| / (sigma_depth step D_p f) + |A_p - A_q|^2 / sigma_albedo^2 + |O_p - O_q| / sigma_opacity
 *              + (lum(c_p) - lum(c_q))^2 / (sigma_color^2 2^-k) )) max(0, N_p . N_q)^sigma_normal
 * on pass k (step = 2^k), f = 2 tanFovxOverTwo / (H - 1) (pixel footprint per unit depth), lum = 0.2126 r + 0.7152 g + 0.0722 b;
 * a sigma of 0 switches its term off.  Neighbours outside the image, with O == 0 or a non-finite colour get weight 0; the centre
 * has weight h(p).  A pixel with O == 0 passes through untouched.  The result is remodulated by max(A, 1e-3) and tone-mapped
 * like svr_hdr_to_ldr. */
typedef struct svr_denoise_params {
    int32_t passes;            /* 1..10; default 5 (steps 1, 2, 4, 8, 16) */
    float sigma_depth;         /* default 0.5 */
    float sigma_normal;        /* exponent; default 32 */
    float sigma_albedo;        /* default 0.4 */
    float sigma_opacity;       /* default 0.8 */
    float sigma_color;         /* 0 (default) = off: at 1-4 spp a colour term mostly stops the filter from removing noise */
    float step;                /* march step of the guides in world units; 0 (default) = half the smallest voxel edge */
} svr_denoise_params;
int svr_denoise_params_default(svr_denoise_params* p);
int svr_set_denoise_params(const svr_denoise_params* p);     /* the parameters of SVR_OPT_DENOISE_PREVIEW and of p == NULL below */
int svr_get_denoise_params(svr_denoise_params* p);
/* the W x H x 8-float guide buffer of the current setup_* scene into a device buffer (on the library's stream) */
int svr_render_guides(void* guides);
/* denoise a WHOLE w x h accumulator (device, packed float3; read only) with the current scene's guides and tone-map it into img (device,
 * RGBA8); w x h must be the camera's image size.  Ignores any row shard or window, like svr_hdr_to_ldr_frame: the call rank 0 makes
 * after svr_assemble_frame.  p == NULL: the current parameters */
int svr_denoise_to_ldr(void* img, const void* hdr, uint32_t w, uint32_t h, const svr_denoise_params* p);
/* the same filter, HDR result (remodulated, not tone-mapped) into out (device, w x h packed float3) */
int svr_denoise_hdr(void* out, const void* hdr, uint32_t w, uint32_t h, const svr_denoise_params* p);
/* number of times the guides have been computed (cache test hook) */
uint64_t svr_guide_builds(void);

/* ---- noise estimate of a progressive render (SVR_OPT_NOISE_ESTIMATE; csrc/svr_noise.hip) ----
 * A(k) = the accumulator after k frames.  From A(m) and A(n), m < n: B = (n A(n) - m A(m)) / (n - m), the mean of frames m+1 .. n (independent
 * of A(m)); with the tone curve before quantisation T(L) = (1 - e^(-16 exposure max(L, 0)))^2.2 per channel,
 *   d^2_p = mean over the 3 channels of (T(A(m)) - T(B))^2,   e^2_p = d^2_p m (n - m) / n^2
 * is the predicted squared error of T(A(n)) in [0, 1] tone-mapped units (delta method; e^2 = d^2 / 4 at n = 2m).  A pixel counts when all 6
 * values are finite and the process owns it (row shard, window); owned pixels with a non-finite value are counted in `nonfinite`.  Tiles:
 * 16 x 16 pixels aligned to the image.  The estimate applies to n frames; for n' > n frames of the same render it scales by sqrt(n / n'). */
typedef struct svr_noise_estimate {
    uint32_t frames;           /* n; 0 = no estimate (yet) */
    uint32_t frames_ref;       /* m */
    float rmse;                /* sqrt(sse / pixels); NaN if no pixel counted */
    float tile_max;            /* largest tile RMSE sqrt(mean e^2 over the tile's counted pixels); NaN if no tile has one */
    uint32_t tiles_x, tiles_y; /* ceil(W / 16), ceil(H / 16): the tile map, row-major */
    uint64_t pixels;           /* counted pixels */
    uint64_t nonfinite;        /* owned pixels left out for a non-finite value */
    double sse;                /* sum of e^2 over the counted pixels: add the sse and pixels of the ranks of a row shard for the frame's rmse */
} svr_noise_estimate;
/* the latest estimate of the render SVR_OPT_NOISE_ESTIMATE (or svr_render_pathtracer_until) follows; frames = 0 if there is none.  Like the scene, the
 * estimate is per process: it belongs to the render the library last followed, whichever accumulator that was (a host with several
 * canvases checks tiles_x / tiles_y, or calls with tile_rmse_device = NULL first).  tile_rmse_device (may be NULL): receives tiles_x * tiles_y
 * floats, NaN for tiles without a counted pixel; an error if it is not a device allocation that large.  Synchronises the library's stream */
int svr_get_noise_estimate(svr_noise_estimate* out, float* tile_rmse_device);
/* stateless: the estimate of A(n) = hdr_n against A(m) = hdr_m (device, w x h packed float3 each; 0 < m < n) over the WHOLE frame, whatever
 * shard or window is set (the call rank 0 makes after svr_assemble_frame; hosts that keep their own copies), with the exposure of the last
 * setup_camera.  tile_rmse_device may be NULL.  Synchronises the library's stream */
int svr_estimate_noise(const void* hdr_m, uint32_t m, const void* hdr_n, uint32_t n, uint32_t w, uint32_t h, float* tile_rmse_device,
                       svr_noise_estimate* out);
/* render from renderParams->frameNo until the predicted noise meets the targets: frames go in folding many-frame launches that end at the
 * checkpoints of SVR_OPT_NOISE_ESTIMATE (the snapshot, then doubling frame counts), one stream synchronisation per estimate; the call stops at
 * the first estimate with rmse <= target_rmse and tile_max <= target_tile_rmse (a target of 0 is not checked; both 0: exactly max_frames), or
 * after max_frames frames.  Works with the option off (the estimator runs for the call's duration).  The accumulator is bit-identical to
 * *frames_done calls of render_pathtracer; renderParams->frameNo advances by *frames_done (frames_done may be NULL) and img holds the tone map
 * of the last frame (SVR_OPT_DENOISE_PREVIEW / SVR_OPT_SKIP_TONEMAP as for any call) */
int svr_render_pathtracer_until(void* img, svr_render_params* renderParams, float target_rmse, float target_tile_rmse, uint32_t max_frames,
                                uint32_t* frames_done);

/* ---- adaptive sampling: 16 x 16 tiles stop being traced once their predicted noise meets a target ----
 * The accumulator holds a uniform render of f0 = renderParams->frameNo frames (0: a fresh render).  The call renders like
 * svr_render_pathtracer_until -- the snapshot at n = max(f0 + 1, 4) frames, then estimates at n = 2m -- but only the tiles still active:
 * a tile freezes at an estimate when n >= min_frames and its tile RMSE was <= target_tile_rmse at this estimate and at the one before (a tile
 * without a counted pixel counts as below the target), so the earliest freeze is at 16 frames of a fresh render.  A frozen tile is never
 * traced or written again and keeps its estimate; a tile still active at the end has its last estimate scaled by sqrt(n_est / n_final).
 * The call ends when no tile is active or after max_frames frames.  Every pixel then equals the uniform render of its tile's frame count, bit
 * for bit.  renderParams->frameNo advances by frames_max - f0; img holds the tone map of the final accumulator (SVR_OPT_SKIP_TONEMAP,
 * SVR_OPT_DENOISE_PREVIEW as for any call).  The noise estimate is left with no render followed and no estimate: the next render call starts a
 * new render.  Continuing with render_pathtracer from renderParams->frameNo MIS-WEIGHTS the frozen tiles (they hold fewer frames): restart
 * at frame 0 instead.  Whole frame, one process: under a row shard or a render window, and with SVR_OPT_KERNEL 1, 3 or 4, the call fails
 * with -6 and changes nothing; so do a target that is not > 0 and finite, max_frames == 0 and f0 + max_frames >= 2^32.  Frames are never
 * traced ahead for the call. */
typedef struct svr_adaptive_result {
    uint32_t frames_max, frames_min;   /* most / fewest frames a tile's pixels hold at the end (counting from 0, i.e. including f0) */
    uint32_t tiles_x, tiles_y;         /* ceil(W / 16), ceil(H / 16): the tile maps, row-major */
    uint32_t tiles_active;             /* tiles not frozen when the call ended (max_frames reached) */
    uint32_t checkpoints;              /* estimates made */
    uint64_t pixel_frames;             /* samples traced by this call: sum over tiles of pixels(t) * (frames_t - f0) */
    uint64_t pixels, nonfinite;        /* as svr_noise_estimate, over the final accumulator */
    double sse;                        /* sum over tiles of the tile's e^2 sum, each scaled to the tile's final frame count */
    float rmse, tile_max;              /* sqrt(sse / pixels); largest final tile RMSE (NaN if there is none) */
} svr_adaptive_result;
int svr_render_pathtracer_adaptive(void* img, svr_render_params* renderParams, float target_tile_rmse, uint32_t min_frames, uint32_t max_frames,
                                   svr_adaptive_result* out);
/* per-tile maps of the last adaptive call of this process: its frame count and final tile RMSE (NaN: no counted pixel).  Either pointer may be
 * NULL; otherwise a device allocation of tiles_x * tiles_y elements.  An error before any adaptive call or if a buffer is too small.
 * Synchronises the library's stream */
int svr_get_adaptive_tiles(uint32_t* tile_frames_device, float* tile_rmse_device);

/* ---- projection modes of the ray caster (csrc/svr_project.hip) ----
 * One deterministic ray per pixel, stateless, scene by argument like render_raycasting.  Everything below is float32 without contraction.
 * RAY AND SAMPLES: exactly the ray caster's.  The pinhole centre ray of the pixel (cuda_camera.h:85-95), the clipped box interval
 *   [tNear, tFar] of volume.Intersect, samples t_0 = tNear, t_{n+1} = fl(t_n + h) with h = stepSize * 0.5f, while t_n <= tFar;
 *   p(t) = orig + dir * t and I_n = volume(p(t_n)), the ray caster's sampler (trilinear on raw u16, x 1/65535, x densityScale).
 *   N = the number of samples the mode looks at: all of them for MIP and MEAN; for ISO the samples up to and including the first
 *   crossing n*, all of them if there is none.
 * MISS (no intersection): RGBA8 (0, 0, 0, 0).
 * MIP:  M = max(0.0f, I_0, ..., I_{N-1}).
 * MEAN: S_0 = 0, S_{n+1} = fl(S_n + I_n) in sample order, M = S_N / (float)N (a correctly rounded division).
 * COLOUR of MIP / MEAN: grey g = clamp((M - window_lo) / (window_hi - window_lo), 0, 1) -- one subtraction each, one correctly rounded
 *   division -- rgb = (g, g, g).  With SVR_PROJ_COLOR_TF: rgb = the transfer function's rgb at M (the ray caster's table look-up), each
 *   channel clamped to [0, 1].  Alpha 255.  Conversion to u8 as the ray caster's: truncation of c * 255.
 * ISO:  n* = the first n with I_n >= iso; none: RGBA8 (0, 0, 0, 0).  If n* = 0 the surface parameter is t_0 (the box face or a clip cap).
 *   Otherwise bisect 8 times: lo = t_{n*-1}, hi = t_{n*}; mid = 0.5f * (lo + hi); volume(p(mid)) >= iso ? hi = mid : lo = mid.  The
 *   surface point is P = p(hi).  Shading is the ray caster's head-light term (raycasting.cu:40-58) with opacity 1: the central-difference
 *   gradient at P, cosTerm = 1 and specularTerm = 0 unless its magnitude is > 1e-3, else normal = normalize(gradient), lightDir =
 *   normalize(cam.pos - P) (normalize(v) = v * (1 / sqrt(dot))), cosTerm = |dot(normal, lightDir)|, specularTerm = powf(cosTerm, 30);
 *   channel = base * 1 * cosTerm * 0.8f + 1 * specularTerm * 0.2f, clamped to 1, with base = 1 (white) or, with SVR_PROJ_COLOR_TF, the
 *   transfer function's rgb at volume(P) (a value the search has already fetched).  Alpha 255.
 * The call honours svr_set_row_shard, svr_set_render_window (pixels outside stay untouched), svr_set_stream, the error mode,
 * SVR_OPT_EMPTY_SKIP (1: samples that provably cannot change the result are not fetched, and runs of them are passed in closed form;
 * 0: every sample is fetched; identical images) and SVR_OPT_COUNT: raycast_steps += N, vol_taps += the fetches of the definition (N per
 * ray, + 8 per bisected pixel, + 6 for the gradient of a surface pixel), vol_taps_executed += the fetches issued.
 * It returns non-zero and leaves img untouched for: a null argument, an unknown mode or flag, a stepSize that is not finite and > 0, a
 * non-finite iso, a non-finite window or window_hi <= window_lo, a negative or non-finite densityScale. */
#define SVR_PROJ_MIP  1   /* largest sample along the ray */
#define SVR_PROJ_MEAN 2   /* mean of the samples along the ray */
#define SVR_PROJ_ISO  3   /* first crossing of `iso`, refined, head-light shaded */

#define SVR_PROJ_COLOR_TF 1u  /* flags: colour from the transfer function, else grey / white */

typedef struct svr_projection_params {
    int32_t  mode;            /* SVR_PROJ_* */
    uint32_t flags;
    float    iso;             /* SVR_PROJ_ISO: level, in the units volume(p) returns */
    float    window_lo, window_hi;   /* grey mapping for MIP / MEAN */
} svr_projection_params;

int svr_projection_params_default(svr_projection_params* p);   /* MIP, grey, window 0..1, iso 0.5 */
int svr_render_projection(void* img, const svr_volume* volume, const svr_transfer_function* tf,
                          const svr_camera* camera, float stepSize, const svr_projection_params* p);

/* ---- slice views: a plane through the volume, optionally thickened into a slab (csrc/svr_slice.hip) ----
 * One deterministic pixel value per pixel, stateless, scene by argument, no camera: the image is an orthographic window of w x h pixels
 * onto the plane through `center` spanned by u and v.  Everything below is float32 without contraction; x, y, w, h, k are converted to
 * float exactly.
 * FRAME: cr = cross(u, v) = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x) (two products and one subtraction per
 *   component), n = cr * (1 / sqrt((cr.x * cr.x + cr.y * cr.y) + cr.z * cr.z)) (correctly rounded square root and division).
 * SLICE k of a stack (k = 0 .. count - 1; svr_render_slice is slice 0 alone): center_0 = center; for k > 0
 *   center_k = center + n * fl(spacing * (float)k), per component one product and one addition.
 * PLANE POINT of pixel (x, y), y counted downwards: a = ((float)x + 0.5f) - 0.5f * (float)w, b = ((float)y + 0.5f) - 0.5f * (float)h,
 *   c = (center_k + u * a) + v * b, per component one product and one addition each, in this order.
 * SLAB SAMPLES: thickness == 0: K = 1 and d_0 = 0 (step and mode are not looked at beyond the checks below).  thickness > 0:
 *   K = (int)floor(thickness / step) + 1 (a correctly rounded division) and d_j = fl(fl((float)j * step) - fl(0.5f * thickness)) -- a
 *   product, not a running sum.  Sample point p_j = c + n * d_j, per component one product and one addition, j = 0 .. K - 1.
 * BOX: the box volume.Intersect clips to (core/geometry/cuda_bbox.h:38-39): per axis e0 = bbox.vmin * (-clip.x), e1 = bbox.vmax * clip.y
 *   (clip = x_clip, y_clip, z_clip), lo = min(e0, e1), hi = max(e0, e1).  Sample j COUNTS iff lo <= p_j <= hi on all three axes (closed
 *   comparisons on the float p_j itself).  I_j = volume(p_j), the ray caster's sampler (trilinear on raw u16, x 1/65535, x densityScale).
 * VALUE: no sample counts: the pixel is RGBA8 (0, 0, 0, 0).  Otherwise alpha is 255 and, over the counting samples in the order of j,
 *   thickness == 0: M = I_0;  SVR_SLAB_MIP: M = max(0.0f, I_j ...);  SVR_SLAB_MINIP: M = min(I_j ...);
 *   SVR_SLAB_MEAN: S = 0, S = fl(S + I_j), M = S / (float)N with N the number of counting samples (a correctly rounded division).
 * COLOUR: as MIP / MEAN of the projection section: grey g = clamp((M - window_lo) / (window_hi - window_lo), 0, 1), rgb = (g, g, g); with
 *   SVR_SLICE_COLOR_TF the transfer function's rgb at M, each channel clamped to [0, 1].  u8 by truncation of c * 255.
 * The calls honour svr_set_row_shard and svr_set_render_window (pixels outside stay untouched; for a stack, in every image),
 * svr_set_stream, the error mode, SVR_OPT_EMPTY_SKIP (1: samples that provably cannot change M are not fetched; identical images) and
 * SVR_OPT_COUNT: raycast_steps += counting samples, vol_taps += the same, vol_taps_executed += the fetches issued.  They keep no state.
 * They return non-zero and leave the image(s) untouched for: a null argument; w or h of 0; a non-finite member of center, u, v,
 * thickness, step, window_lo, window_hi or spacing; a cross(u, v) whose length is 0 or not finite; thickness < 0; thickness > 0 with a
 * step that is not > 0, with an unknown mode or with floor(thickness / step) + 1 > SVR_SLICE_MAX_SAMPLES (refused, not clamped); unknown
 * flags; window_hi <= window_lo; a negative or non-finite densityScale; count == 0; more than 2^32 - 1 tile tasks (tiles x count). */
#define SVR_SLAB_MIP   1   /* largest sample of the slab */
#define SVR_SLAB_MINIP 2   /* smallest sample of the slab */
#define SVR_SLAB_MEAN  3   /* mean of the samples of the slab */

#define SVR_SLICE_COLOR_TF 1u   /* flags: colour from the transfer function, else grey through the window */
#define SVR_SLICE_MAX_SAMPLES 4096   /* most samples K of a slab */

typedef struct svr_slice_params {
    svr_vec3 center;               /* world point shown at the image centre */
    svr_vec3 u, v;                 /* world displacement of one pixel to the right / one pixel down (length = pixel size) */
    float    thickness;            /* slab thickness along n = normalize(cross(u, v)), world units; 0 = a single plane */
    float    step;                 /* distance between slab samples along n; not used when thickness == 0 */
    int32_t  mode;                 /* SVR_SLAB_*; not used when thickness == 0 */
    uint32_t flags;
    float    window_lo, window_hi; /* grey mapping */
} svr_slice_params;                /* 4-byte members only, no padding: 60 bytes */

/* centre 0, u = (1, 0, 0), v = (0, 1, 0), thickness 0, step 1, SVR_SLAB_MIP, grey, window 0..1.  Plain host code */
int svr_slice_params_default(svr_slice_params* p);
/* The plane perpendicular to world axis 0 / 1 / 2 (x / y / z) at `position` in [0, 1] across the CLIPPED box (0 = its lo face, 1 = its hi
 * face, the BOX of the contract), fitted to w x h pixels with square pixels and the whole box face visible and centred.  Image right /
 * down are world +y / -z for axis 0, +x / -z for axis 1, +x / -y for axis 2 (so n = -x, +y, -z); pixel size = max(extent_right /
 * w, extent_down / h); thickness 0, step = the pixel size, SVR_SLAB_MIP, grey, window 0..1.  Plain host code: no GPU is needed.  Non-zero
 * for a null argument, an axis outside 0..2, a position outside [0, 1], w or h of 0, a box that is not finite or has no extent. */
int svr_slice_params_axis(svr_slice_params* p, const svr_volume* volume, int axis, float position, uint32_t w, uint32_t h);
/* one slice into img (w x h RGBA8, device memory) */
int svr_render_slice(void* img, const svr_volume* volume, const svr_transfer_function* tf, uint32_t w, uint32_t h,
                     const svr_slice_params* p);
/* `count` parallel slices in one launch: slice k as defined above; writes count images of w x h RGBA8 back to back */
int svr_render_slice_stack(void* imgs, const svr_volume* volume, const svr_transfer_function* tf, uint32_t w, uint32_t h,
                           const svr_slice_params* p, uint32_t count, float spacing);
/* svr_slice_params_axis through a world point instead of at a relative position: every field as svr_slice_params_axis fills it, except
 * that the component of `center` on `axis` is the point's component, taken verbatim (the link from a picked point, svr_pick below, to
 * the slice views).  Plain host code.  Non-zero for what svr_slice_params_axis refuses, for a non-finite point, and for a point outside
 * the clipped box on that axis (the faces are inside). */
int svr_slice_params_through(svr_slice_params* p, const svr_volume* volume, int axis, const svr_vec3* point, uint32_t w, uint32_t h);

/* ---- hit maps and picks (csrc/svr_hits.hip) ----
 * Where in the volume a pixel's ray meets what the picture shows: one deterministic ray per pixel, stateless, scene by argument like
 * render_raycasting.  Everything below is float32 without contraction.
 * RAY AND SAMPLES: exactly those of the projection section.  The pinhole centre ray of the pixel, the clipped box interval
 *   [tNear, tFar] of volume.Intersect, samples t_0 = tNear, t_{n+1} = fl(t_n + h) with h = stepSize * 0.5f, while t_n <= tFar;
 *   p(t) = orig + dir * t (per component one product and one addition) and I_n = volume(p(t_n)).  tNear may be negative (the camera inside
 *   the box), so the status is a member of its own and is not encoded in t.
 * STATUS: SVR_HIT_STATUS_MISS: the ray does not intersect the clipped box.  SVR_HIT_STATUS_NONE: it does, and no sample meets the mode's
 *   condition; `sample` = the number of samples N of the ray.  SVR_HIT_STATUS_FOUND: `sample` = the index n of the hit sample, t = the ray
 *   parameter of the hit, position = p(t), value = volume(position), normal as below.  Members not named for a status are +0.
 * SVR_HIT_OPACITY: a_n = the alpha channel of the ray caster's transfer-function look-up at I_n; A_0 = 0,
 *   A_{n+1} = fl(A_n + fl(fl(1 - A_n) * a_n)), the ray caster's accumulation.  The hit is the first n with A_{n+1} > alpha; no refinement:
 *   t = t_n, value = I_n.  alpha lies in [0, 0.95]: 0 gives the first sample with any opacity, 0.95 the sample at which render_raycasting
 *   stops.
 * SVR_HIT_ISO: the search and the 8 bisections of SVR_PROJ_ISO, to the letter: n* = the first n with I_n >= iso; if n* = 0, hi = t_0;
 *   otherwise lo = t_{n*-1}, hi = t_{n*}, 8 times mid = 0.5f * (lo + hi), volume(p(mid)) >= iso ? hi = mid : lo = mid.  sample = n*, t = hi,
 *   position = p(hi) -- the point svr_render_projection shades -- and value = the fetch the search made at hi.
 * SVR_HIT_MAX: M = max(0.0f, I_0, ...) with strict updates (I_n > M), the SVR_PROJ_MIP value; the hit is the first n with I_n == M,
 *   t = t_n, value = M.  M == 0: NONE.
 * NORMAL, every mode: g = the ray caster's central-difference gradient at position (cuda_volume.h:54-61).  If sqrt(dot(g, g)) > 1e-3 (the
 *   ray caster's comparison) normal = g * (1 / sqrt(dot(g, g))), else (0, 0, 0).  It is not flipped towards the camera.
 * svr_render_hits honours svr_set_row_shard and svr_set_render_window (records outside stay untouched); svr_pick is a query and ignores
 * both.  Both honour svr_set_stream, the error mode, SVR_OPT_EMPTY_SKIP (1: samples that provably cannot change the result are not
 * fetched -- ISO and MAX by the projection's rules, OPACITY by the ray caster's `empty` macro-cells, where a_n = 0 exactly -- and runs of
 * them are passed in closed form; 0: every sample is fetched; identical records) and SVR_OPT_COUNT: raycast_steps += the samples looked
 * at (n + 1 for an OPACITY or ISO hit at n, else N), vol_taps += the fetches of the definition (one per sample looked at, + 8 for a
 * bisected pixel, + 6 for the gradient of a FOUND pixel), vol_taps_executed += the fetches issued.  They keep no state.
 * Both return non-zero and leave the output untouched for: a null argument, an unknown mode, a stepSize that is not finite and > 0, a
 * non-finite iso, an alpha outside [0, 0.95] or non-finite, a negative or non-finite densityScale; svr_pick also for n == 0,
 * n > SVR_PICK_MAX and a pixel outside the image. */
#define SVR_HIT_OPACITY 1   /* where the ray caster's accumulated opacity first exceeds `alpha` */
#define SVR_HIT_ISO     2   /* the refined first crossing of `iso`: the point SVR_PROJ_ISO shades */
#define SVR_HIT_MAX     3   /* the first sample that attains the SVR_PROJ_MIP maximum */

#define SVR_HIT_STATUS_MISS  0  /* the ray does not intersect the clipped box */
#define SVR_HIT_STATUS_NONE  1  /* it does, and no sample meets the mode's condition */
#define SVR_HIT_STATUS_FOUND 2

#define SVR_PICK_MAX 4096       /* most pixels of one svr_pick call */

typedef struct svr_hit {      /* 4-byte members only, 40 bytes */
    int32_t  status;          /* SVR_HIT_STATUS_* */
    int32_t  sample;          /* FOUND: the index n of the hit sample; NONE: the number of samples N; MISS: 0 */
    float    t;               /* ray parameter of the hit */
    float    value;           /* volume(position) */
    svr_vec3 position;        /* world */
    svr_vec3 normal;          /* normalize(gradient) at position, or (0,0,0) */
} svr_hit;

typedef struct svr_hit_params {
    int32_t mode;             /* SVR_HIT_* */
    float   alpha;            /* SVR_HIT_OPACITY: opacity level in [0, 0.95] */
    float   iso;              /* SVR_HIT_ISO: level, in the units volume(p) returns */
} svr_hit_params;

int svr_hit_params_default(svr_hit_params* p);   /* OPACITY, alpha 0.5, iso 0.5.  Plain host code */
/* imageW x imageH svr_hit records, row-major, into hits (device memory) */
int svr_render_hits(void* hits, const svr_volume* volume, const svr_transfer_function* tf, const svr_camera* camera, float stepSize,
                    const svr_hit_params* p);
/* the records of the n pixels (x_i, y_i) = (pixels_xy[2 i], pixels_xy[2 i + 1]) of a HOST array, in list order, into hits (device
 * memory, n records) in one launch; record i is bit-identical to record (x_i, y_i) of the full map.  The list is read before the call
 * returns */
int svr_pick(void* hits, const uint32_t* pixels_xy, uint32_t n, const svr_volume* volume, const svr_transfer_function* tf,
             const svr_camera* camera, float stepSize, const svr_hit_params* p);

/* ---- seeded region growing: pick a point, segment, measure, show (csrc/svr_region.hip) ----
 * Integers only; every result is exact.
 * INPUT: a plain u16 volume [nz][ny][nx] (host, or device with src_is_device = 1, as svr_create_volume_texture takes it; at most 2^31
 *   voxels, which keeps sum_sq inside 64 bits), 1 .. SVR_REGION_MAX_SEEDS seed voxels (x, y, z), an inclusive raw-value window
 *   lo <= v <= hi, a connectivity 6 (faces), 18 (faces and edges) or 26 (faces, edges and corners), and an inclusive voxel box
 *   box_min .. box_max that growth may not leave (it is intersected with the volume; the default 0 .. INT32_MAX is the whole volume).
 * REGION: candidates = {voxel in the box : lo <= v <= hi}.  The region is the union, over the seeds, of the connected component
 *   (chosen connectivity) of the candidates that contains the seed; a seed that is not a candidate contributes nothing, and if none is
 *   the region is empty: status SVR_REGION_STATUS_EMPTY, return 0 -- not an error.  The region is the least fixpoint of a monotone rule
 *   and therefore unique: the mask is defined bit for bit, whatever order the GPU grows in.
 * MASK: uint32 words on the device; voxel (x, y, z) is bit x & 31 of word (z * ny + y) * wx + (x >> 5), wx = (nx + 31) / 32; padding bits
 *   are 0.  svr_region_mask_words(nx, ny, nz) = wx * ny * nz is the word count (0 for a dimension <= 0).
 * STATS (svr_region_stats): voxels = the region's size; sum, sum_sq = the sums of v and v^2 over it; sum_x, sum_y, sum_z = the sums of
 *   the voxel indices; faces_x / _y / _z = the number of pairs (region voxel, neighbour at +-1 on that axis) whose neighbour is outside
 *   the region or outside the volume; vmin, vmax = the extreme values (65535 and 0 for an empty region); bbox_min, bbox_max = the
 *   inclusive index bounds (the dimensions and -1 for an empty region); sweeps = the grow passes launched (0 from svr_region_stats_of).
 * MEASURE (svr_region_measure; plain host code, double): volume = voxels sx sy sz; mean = sum / voxels; stddev = the population
 *   standard deviation sqrt(voxels sum_sq - sum^2) / voxels (the radicand in exact integers); centroid = (sum_x, sum_y, sum_z) / voxels,
 *   in voxel index space; surface_area = faces_x sy sz + faces_y sx sz + faces_z sx sy.  An empty region gives zeros.
 * SWEEPS: growth runs in passes over tiles of 128 x 8 x 8 voxels; a pass that adds a voxel moves the front of the region across at least
 *   one tile boundary, so a region whose way out from its seeds enters every tile at most twice is complete after 2 T passes (T = the
 *   number of tiles) and one more that confirms it.  The default cap (max_sweeps = 0) is svr_region_default_max_sweeps = min(64 + 2 T,
 *   65536) launches; a region that winds through its tiles more often needs max_sweeps set by the caller.  At the cap the call returns
 *   SVR_REGION_ERR_SWEEPS, the mask holds the part grown so far and stats->sweeps the launches; it does not go on.
 * All calls run on the library's stream (svr_set_stream); svr_region_grow and svr_region_stats_of synchronise it, since they return
 * host statistics.  None touches the scene, the options or the render accumulators.  Arguments are checked before the device is
 * touched.  A negative code is returned, with svr_last_error() set and nothing written, for: a null pointer (-4); a dimension <= 0 or
 * more than 2^31 voxels (-6); lo > hi or hi > 65535, a connectivity other than 6 / 18 / 26, nseeds == 0 or > SVR_REGION_MAX_SEEDS, a seed
 * outside the volume, a box with box_min > box_max on an axis or with no voxel of the volume in it, an unknown mode, a fill > 65535, a
 * point outside the volume's box, a spacing that is not positive and finite (-3). */
#define SVR_REGION_MAX_SEEDS 64
#define SVR_REGION_KEEP   1     /* svr_region_apply: voxels outside the region become `fill` */
#define SVR_REGION_REMOVE 2     /* svr_region_apply: voxels inside the region become `fill` */
#define SVR_REGION_STATUS_OK    0
#define SVR_REGION_STATUS_EMPTY 1
#define SVR_REGION_ERR_SWEEPS (-9)   /* the region was still growing after max_sweeps passes */

typedef struct svr_region_params {   /* 4-byte members only, 40 bytes */
    uint32_t lo, hi;                 /* inclusive raw-value window */
    int32_t  connectivity;           /* 6, 18 or 26 */
    int32_t  box_min[3], box_max[3]; /* inclusive voxel box (x, y, z) */
    uint32_t max_sweeps;             /* 0 = svr_region_default_max_sweeps(nx, ny, nz) */
} svr_region_params;

typedef struct svr_region_stats {    /* 112 bytes */
    uint64_t voxels, sum, sum_sq, sum_x, sum_y, sum_z;
    uint64_t faces_x, faces_y, faces_z;
    uint32_t vmin, vmax;
    int32_t  bbox_min[3], bbox_max[3];
    uint32_t sweeps;
    int32_t  status;                 /* SVR_REGION_STATUS_* */
} svr_region_stats;

typedef struct svr_region_measurement {   /* 56 bytes */
    double volume, mean, stddev;
    double centroid[3];
    double surface_area;
} svr_region_measurement;

/* window 0..65535, connectivity 6, the whole volume, max_sweeps 0.  Plain host code */
int svr_region_params_default(svr_region_params* p);
uint64_t svr_region_mask_words(int nx, int ny, int nz);
uint32_t svr_region_default_max_sweeps(int nx, int ny, int nz);
/* seeds_xyz: a HOST array of 3 * nseeds int32 (x, y, z).  mask_device (svr_region_mask_words words) is overwritten */
int svr_region_grow(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, const int32_t* seeds_xyz, uint32_t nseeds,
                    const svr_region_params* params, uint32_t* mask_device, svr_region_stats* stats_host);
/* the same statistics for any mask in this format (padding bits 0), e.g. one the caller edited */
int svr_region_stats_of(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, const uint32_t* mask_device,
                        svr_region_stats* stats_host);
/* out (device, nx * ny * nz u16) = the volume with the voxels outside (SVR_REGION_KEEP) or inside (SVR_REGION_REMOVE) the region set to
 * `fill`.  out may be the device `voxels` itself.  Asynchronous on the library's stream for a device source */
int svr_region_apply(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, const uint32_t* mask_device, int mode, uint32_t fill,
                     uint16_t* out_u16_device);
/* the voxel whose cell contains a world point (e.g. svr_hit.position), by the mapping with which the sampler addresses the texture: the
 * float32 texture coordinate c = (point - bbox.vmin) * bbox.invSize per axis (the unclipped box); voxel i covers [i / n, (i + 1) / n),
 * i = floor(c n), and c = 1 (the far face) belongs to voxel n - 1.  A point with a c outside [0, 1] is refused.  Plain host code */
int svr_region_seed_from_world(const svr_volume* volume, int nx, int ny, int nz, const svr_vec3* point, int32_t ijk[3]);
int svr_region_measure(const svr_region_stats* stats, const double spacing[3], svr_region_measurement* out);
/* HIP-event times of the phases of the last svr_region_grow: classify (with the seeds), grow (all sweeps), stats.  Pointers may be NULL */
int svr_region_last_ms(float* classify_ms, float* grow_ms, float* stats_ms);

/* ---- operations on region masks: morphology, set operations, regrowth, hole filling, leak cutting (csrc/svr_morph.hip) ----
 * Every mask is a DEVICE pointer to svr_region_mask_words(nx, ny, nz) words in the layout above.  The calls are stateless: they run on the
 * library's stream and touch no scene, option or accumulator; results are exact (integers) and feed svr_region_stats_of, _measure, _apply.
 * PADDING: the bits of a row's last word at x >= nx are ignored on input, whatever they hold, and are 0 on output.
 * NEIGHBOURS: element / connectivity 6 = the face neighbours of a voxel, 18 = faces and edges, 26 = faces, edges and corners.
 * MORPH: the unit structuring element is a voxel and its element-neighbours; radius r applies it r times (the iterated definition).
 *   DILATE: a voxel is set if it or one of its element-neighbours INSIDE the volume is set; nothing enters from outside.
 *   ERODE is the dual, erode(M) = NOT dilate(NOT M) inside the volume: a voxel stays if it and all its element-neighbours inside the volume
 *   are set, so a region touching a face of the volume is not eroded from that face.  OPEN = erode then dilate, CLOSE = dilate then erode;
 *   open(M) is a subset of M, M of close(M), and both are idempotent.  (scipy.ndimage: binary_dilation(border_value=0) and
 *   binary_erosion(border_value=1), iterations=radius, generate_binary_structure(3, 1 | 2 | 3).)
 * COMBINE: AND, OR, ANDNOT (a & ~b), XOR, NOT (~a; b must be NULL).  out may alias a or b.
 * RECONSTRUCT: out = the union of the connected components (connectivity 6 / 18 / 26) of `cand` that contain a voxel of marker & cand;
 *   empty, with return 0, if there is none.  It is svr_region_grow's fixpoint with masks in place of the window and the seed list, and runs
 *   on the same kernel and sweeps: max_sweeps = 0 means svr_region_default_max_sweeps, and at the cap the call returns SVR_REGION_ERR_SWEEPS
 *   with the part grown so far in out.  *sweeps_out (may be NULL) = the passes launched.
 * FILL HOLES: out = NOT reconstruct(marker = every voxel on the six faces of the volume, cand = NOT in, background_connectivity): `in` and
 *   every background voxel that cannot reach a face.  background_connectivity 6 is scipy.ndimage.binary_fill_holes' default.  At the sweep
 *   cap (SVR_REGION_ERR_SWEEPS) out holds the complement of the background reached so far: more than the filled mask.
 * DETACH: cuts from a grown region what hangs on it by connections thinner than the element: E = erode(in, element, radius); K =
 *   reconstruct(marker = dilate(the seed voxels, element, radius), cand = E, connectivity); out = dilate(K, element, radius) & in.  The
 *   marker is the dilated seed, so a seed that the erosion removes still finds its core whenever it lies in the opening of `in`; if it does
 *   not, the result is empty: *status = SVR_REGION_STATUS_EMPTY, return 0.  Seeds are a HOST array as in svr_region_grow.
 * The library allocates and frees the temporaries (a morph that takes more than one launch -- open, close, a radius of 3 or above 4: one mask;
 * reconstruct and fill_holes: one mask; detach: four); a call that used one synchronises the stream before it returns, svr_region_combine
 * and a one-launch morph (dilate or erode by 1, 2 or 4) are asynchronous.
 * REFUSED, before the device is touched: a null pointer (-4); a dimension <= 0 or more than 2^31 voxels (-6); an unknown op, an element or
 * connectivity other than 6 / 18 / 26, a radius outside 1 .. SVR_MORPH_MAX_RADIUS, b != NULL with SVR_MASK_NOT, nseeds == 0 or >
 * SVR_REGION_MAX_SEEDS, a seed outside the volume, an `out` that overlaps an input of morph, reconstruct, fill_holes or detach (-3). */
#define SVR_MORPH_DILATE 1
#define SVR_MORPH_ERODE  2
#define SVR_MORPH_OPEN   3
#define SVR_MORPH_CLOSE  4
#define SVR_MORPH_MAX_RADIUS 32
#define SVR_MASK_AND    1
#define SVR_MASK_OR     2
#define SVR_MASK_ANDNOT 3
#define SVR_MASK_XOR    4
#define SVR_MASK_NOT    5
int svr_region_morph(const uint32_t* in_mask_device, int nx, int ny, int nz, int op, int element, uint32_t radius, uint32_t* out_mask_device);
int svr_region_combine(const uint32_t* a_device, const uint32_t* b_device, int nx, int ny, int nz, int op, uint32_t* out_device);
int svr_region_reconstruct(const uint32_t* marker_device, const uint32_t* cand_device, int nx, int ny, int nz, int connectivity, uint32_t max_sweeps,
                           uint32_t* out_device, uint32_t* sweeps_out);
int svr_region_fill_holes(const uint32_t* in_device, int nx, int ny, int nz, int background_connectivity, uint32_t max_sweeps, uint32_t* out_device);
int svr_region_detach(const uint32_t* in_device, int nx, int ny, int nz, const int32_t* seeds_xyz, uint32_t nseeds, int element, uint32_t radius,
                      int connectivity, uint32_t max_sweeps, uint32_t* out_device, int32_t* status);
/* HIP-event time of the device work of the last of the five calls above (waits for it) */
int svr_region_mask_last_ms(float* ms);

/* ---- connected components of region masks: label, measure per component, keep the largest, drop the small (csrc/svr_label.hip;
 *      DESIGN.md 8j) ----
 * Masks are DEVICE pointers in the layout above; the calls are stateless: they run on the library's stream and touch no scene, option
 * or accumulator; results are exact (integers) and unique, whatever order the GPU works in.  Input padding bits are ignored, output
 * padding bits are 0.
 * THRESHOLD: out = the candidate mask of svr_region_grow without any seed, {voxel in the box : lo <= v <= hi}.  box_min / box_max are
 *   HOST arrays of 3 int32 (x, y, z), inclusive, intersected with the volume; both NULL = the whole volume.  The volume is a u16 array
 *   [nz][ny][nx], host or device (src_is_device), as in svr_region_grow.  Asynchronous for a device source.
 * LABEL: labels_device is a dense uint32 array [nz][ny][nx] (4 nx ny nz bytes).  0 = background; the connected components of the mask
 *   under connectivity 6 / 18 / 26 are numbered 1 .. K in ascending order of their smallest linear voxel index (z ny + y) nx + x, which
 *   makes the array unique (it is scipy.ndimage.label's numbering with generate_binary_structure(3, 1 | 2 | 3)).  *count_out = K.  An
 *   empty mask gives K = 0, all labels 0 and return 0.  The call allocates and frees its temporaries (about 1 / 32 of the label array)
 *   and synchronises the stream.  The work is union-find with walks that only ever move to smaller indices; every walk also counts its
 *   steps against the voxel count, and a walk that reached that cap -- which no valid state can -- makes the call return
 *   SVR_REGION_ERR_LABEL with the labels invalid; it does not go on.
 * TABLE (svr_region_component[count], indexed by label - 1): voxels = the component's size; first = its smallest linear voxel index;
 *   bbox_min, bbox_max = its inclusive bounds in x, y, z; sum = the sum of the raw values over it (0 when voxels_or_null is NULL).
 *   Labels above `count` are ignored.  Any label array will do, not only svr_region_label's: a voxel counts for the entry of its label,
 *   whatever its neighbours hold (the zones of svr_region_split).  Asynchronous for a device source or none.
 * SELECT: out = the voxels whose label has a non-zero entry in keep_device (uint8 [count + 1], indexed by label; entry 0 is ignored:
 *   background never enters; labels above count are dropped).  Asynchronous.
 * SELECT BY SIZE: keeps the components with at least min_voxels voxels that are among the largest_k largest (0 = no limit); ties in size
 *   go to the lower label.  The sizes are read back and ranked in host code, so the call synchronises.  *kept_out = the components
 *   kept; 0 of them is an empty mask and return 0.
 * K = 0: a caller whose mask has no component has nothing to tabulate or select; count == 0 is refused.
 * REFUSED, before the device is touched: a null pointer (-4); a dimension <= 0 or more than 2^31 voxels (-6); lo > hi or hi > 65535, a box
 *   with one pointer NULL, with box_min > box_max on an axis or with no voxel of the volume in it, a connectivity other than 6 / 18 / 26,
 *   count == 0 (-3). */
#define SVR_REGION_ERR_LABEL (-10)   /* a union-find walk reached its iteration cap: the labels are not valid */

typedef struct svr_region_component {   /* 40 bytes */
    uint32_t voxels;
    uint32_t first;
    int32_t  bbox_min[3], bbox_max[3];
    uint64_t sum;
} svr_region_component;

int svr_region_threshold(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, uint32_t lo, uint32_t hi, const int32_t* box_min,
                         const int32_t* box_max, uint32_t* out_mask_device);
int svr_region_label(const uint32_t* in_mask_device, int nx, int ny, int nz, int connectivity, uint32_t* labels_device, uint32_t* count_out);
int svr_region_label_table(const uint32_t* labels_device, const uint16_t* voxels_or_null, int nx, int ny, int nz, int src_is_device, uint32_t count,
                           svr_region_component* table_device);
int svr_region_select(const uint32_t* labels_device, int nx, int ny, int nz, uint32_t count, const uint8_t* keep_device, uint32_t* out_mask_device);
int svr_region_select_by_size(const uint32_t* labels_device, int nx, int ny, int nz, uint32_t count, const svr_region_component* table_device,
                              uint32_t min_voxels, uint32_t largest_k, uint32_t* out_mask_device, uint32_t* kept_out);
/* HIP-event time of the device work of the last of the five calls above (waits for it) */
int svr_region_label_last_ms(float* ms);

/* ---- exact Euclidean distance maps of region masks and ball morphology (csrc/svr_distance.hip) ----
 * Masks are DEVICE pointers in the layout above; input padding bits are ignored whatever they hold, output padding bits are 0.  The calls
 * are stateless: they run on the library's stream and touch no scene, option or accumulator.  Integers only; every result is exact and
 * unique, whatever order the GPU works in.
 * WEIGHTS AND THE MEASURE: `weights` is a HOST array of three uint32 (x, y, z), each >= 1; NULL means 1, 1, 1.  The squared distance between
 *   voxels p and q is wx (px - qx)^2 + wy (py - qy)^2 + wz (pz - qz)^2.  A map is a dense uint32 array [nz][ny][nx] on the device;
 *   SVR_DIST_NONE means "there is no target voxel at all".  A call is refused when wx (nx - 1)^2 + wy (ny - 1)^2 + wz (nz - 1)^2, taken in
 *   64-bit host arithmetic, exceeds 0xFFFFFFFE -- which also bounds every axis at 65536.
 * DISTANCE: target SVR_DIST_TO_SET: every voxel gets the smallest squared distance to a set voxel (set voxels get 0); SVR_DIST_TO_UNSET:
 *   to an unset voxel OF THE VOLUME (unset voxels get 0) -- nothing outside the volume counts as background and padding bits are not
 *   voxels: scipy.ndimage.distance_transform_edt(mask, sampling=sqrt(w)) squared, and the border rule of svr_region_morph's ERODE.  With
 *   no target voxel every entry is SVR_DIST_NONE and the return is 0.  The call allocates and frees its workspace -- 8 bytes per voxel: a
 *   second map and the envelope stacks of the column passes -- and synchronises the stream.
 * SELECT: out = the voxels with lo2 <= d2 <= hi2, so SVR_DIST_NONE is selected only by hi2 == 0xFFFFFFFF.  Margins are 0 .. r2 of a TO_SET
 *   map, shells a2 .. b2.  Asynchronous.
 * BALL: svr_region_morph's ops with the ball {offset : weighted d^2 <= r2} as the element.  DILATE = d2_to_set <= r2 (an empty mask stays
 *   empty whatever r2); ERODE = d2_to_unset > r2, so a region touching a face of the volume is not eroded from that face, and a full mask
 *   stays full; OPEN = erode then dilate, CLOSE = dilate then erode.  r2 = 0 is the identity with the padding cleared.  With weights 1, 1,
 *   1 the ball of r2 = 1 / 2 / 3 is the unit element 6 / 18 / 26.  The cost does not depend on r2.  The last pass of each transform compares
 *   with r2 and writes mask words: no map is stored.  Workspace 12 bytes per voxel (and one mask for open / close); the call synchronises
 *   unless r2 = 0.  out may not overlap in.
 * MAX: looks at the voxels of the mask, or at all voxels when the mask is NULL: *max_d2 = the largest value other than SVR_DIST_NONE among
 *   them, *first_index = the smallest linear voxel index (z ny + y) nx + x that attains it -- on a TO_UNSET map the centre of the largest
 *   inscribed ball.  When there is no such voxel *status = SVR_REGION_STATUS_EMPTY (both outputs 0) and the return is 0.  Synchronises.
 * VOLUME: out = min(65535, isqrt(d2 scale^2)) as u16 [nz][ny][nx], isqrt the exact integer floor square root of the 64-bit product;
 *   SVR_DIST_NONE becomes 65535; scale in 1 .. 65535.  The result is ready for svr_create_volume_texture.  Asynchronous.
 * WEIGHTS FROM A SPACING (plain host code): unit = min(spacing) / 2^k for the largest k in 4, 3, 2, 1, 0 for which the weights
 *   w[a] = max(1, llround((spacing[a] / unit)^2)) pass the overflow bound; a length L in the spacing's units is then r2 = floor((L / unit)^2)
 *   and a map value d2 means sqrt(d2) unit.
 * REFUSED, before the device is touched: a null pointer (-4); a dimension <= 0 or more than 2^31 voxels (-6); a weight of 0, the overflow
 *   bound, an unknown target or op, lo2 > hi2, a scale outside 1 .. 65535, an `out` that overlaps `in` of svr_region_ball, a spacing that
 *   is not positive and finite or that no k fits (-3). */
#define SVR_DIST_NONE     0xFFFFFFFFu
#define SVR_DIST_TO_SET   1
#define SVR_DIST_TO_UNSET 2
int svr_region_distance(const uint32_t* in_mask_device, int nx, int ny, int nz, const uint32_t* weights_or_null, int target, uint32_t* d2_device);
int svr_region_distance_select(const uint32_t* d2_device, int nx, int ny, int nz, uint32_t lo2, uint32_t hi2, uint32_t* out_mask_device);
int svr_region_ball(const uint32_t* in_mask_device, int nx, int ny, int nz, int op, const uint32_t* weights_or_null, uint32_t r2,
                    uint32_t* out_mask_device);
int svr_region_distance_max(const uint32_t* d2_device, const uint32_t* mask_device_or_null, int nx, int ny, int nz, uint32_t* max_d2,
                            uint32_t* first_index, int32_t* status);
int svr_region_distance_volume(const uint32_t* d2_device, int nx, int ny, int nz, uint32_t scale, uint16_t* out_u16_device);
int svr_region_distance_weights(const double spacing[3], int nx, int ny, int nz, uint32_t weights[3], double* unit_out);
/* HIP-event time of the device work of the last of the calls above (waits for it) */
int svr_region_distance_last_ms(float* ms);
/* HIP-event times of the row, y and z pass of the last transform run (svr_region_distance, or the second half of an open / close).
 * Pointers may be NULL */
int svr_region_distance_pass_ms(float* rows_ms, float* y_ms, float* z_ms);

/* ---- exact volume filters: median / min / max and binomial smoothing of the raw voxels, before they are segmented
 *      (csrc/svr_filter.hip) ----
 * A volume is a u16 array [nz][ny][nx], host or device (src_is_device), as in svr_region_grow; `out` is DEVICE memory of nx ny nz u16
 * and is ready for svr_create_volume_texture and for every svr_region_* call.  The calls are stateless: they run on the library's
 * stream and touch no scene, option or accumulator.  Integers only; every result is exact and unique, whatever order the GPU works in.
 * BORDER: it replicates.  A neighbour index outside the volume is clamped per axis, so a window always holds its full count of values
 *   (with repeats) and a binomial sum all its taps: numpy's pad mode 'edge', scipy's mode='nearest'.
 * RANK: the window of a voxel is the voxel and its neighbours under the unit element 6 / 18 / 26 of svr_region_morph: 7 / 19 / 27 values.
 *   SVR_FILTER_MEDIAN = the value of rank 3 / 9 / 13 (0-based) of the sorted window, SVR_FILTER_MIN = rank 0, SVR_FILTER_MAX = the last
 *   rank; values are compared as unsigned 16-bit numbers.  `iterations` in 1 .. SVR_FILTER_MAX_ITERATIONS applies the filter that many
 *   times to its own output.  This is scipy.ndimage.median_filter / minimum_filter / maximum_filter with
 *   footprint=generate_binary_structure(3, 1 | 2 | 3) and mode='nearest'.
 * SMOOTH: separable binomial smoothing.  radii_xyz is a HOST array of three uint32 (x, y, z), each in 0 .. SVR_SMOOTH_MAX_RADIUS; the
 *   passes run in the order x, y, z, and a pass of radius r > 0 along an axis replaces v[i] by
 *     (sum_{k = 0 .. 2r} C(2r, k) v[clamp(i - r + k)] + 2^(2r - 1)) >> 2r
 *   -- the binomial kernel of order 2r, rounded half up ONCE PER AXIS, so the result of a pass is a u16 volume again and the whole is
 *   defined by the passes alone.  The sum is at most 65535 * 4^8 + 2^15 < 2^32: it fits an unsigned 32-bit integer exactly, which is what
 *   caps the radius at 8.  Radius 0 is the identity on its axis; (0, 0, 0) is a copy.  The variance of a pass is r / 2 voxels^2, so
 *   radius 8 is sigma = 2 voxels.
 * RADII FROM A SIGMA (plain host code): radii[a] = llround(2 (sigma / spacing[a])^2), the radius whose variance is nearest to sigma^2 in
 *   the spacing's units; sigma_out[a] (may be NULL) = sqrt(radii[a] / 2) spacing[a], the sigma actually applied.  sigma = 0 gives 0, 0, 0.
 * WORKSPACE AND SYNCHRONISATION: a call with more than one pass (iterations > 1; more than one radius > 0) allocates one temporary
 *   volume of nx ny nz u16 and frees it, and a host source is uploaded to a temporary; such calls synchronise the stream before they
 *   return.  A one-pass call on a device source, and the (0, 0, 0) copy of one, are asynchronous.  `voxels` is never written.
 * REFUSED, before the device is touched and with nothing written: a null pointer (-4); a dimension <= 0 or more than 2^31 voxels (-6);
 *   an unknown op, an element other than 6 / 18 / 26, iterations of 0 or above the cap, a radius above 8, an `out` that overlaps a device
 *   `voxels`; for svr_volume_smooth_radii a spacing that is not positive and finite, a sigma that is negative or not finite, or one that
 *   needs a radius above 8 on some axis (-3). */
#define SVR_FILTER_MEDIAN 1
#define SVR_FILTER_MIN    2
#define SVR_FILTER_MAX    3
#define SVR_FILTER_MAX_ITERATIONS 64
#define SVR_SMOOTH_MAX_RADIUS 8
int svr_volume_rank(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, int op, int element, uint32_t iterations,
                    uint16_t* out_u16_device);
int svr_volume_smooth(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, const uint32_t* radii_xyz, uint16_t* out_u16_device);
int svr_volume_smooth_radii(const double spacing[3], double sigma, uint32_t radii[3], double sigma_out[3]);
/* HIP-event time of the device work of the last svr_volume_rank / svr_volume_smooth call (waits for it) */
int svr_volume_filter_last_ms(float* ms);

/* ---- geodesic distances and influence zones inside region masks; splitting a region at its necks (csrc/svr_geodesic.hip;
 *      DESIGN.md 8m) ----
 * Masks are DEVICE pointers in the layout above; input padding bits are ignored whatever they hold, output padding bits are 0.  Label,
 * distance and zone arrays are dense uint32 [nz][ny][nx] on the device.  The calls are stateless: they run on the library's stream and
 * touch no scene, option or accumulator.  Integers only; every result is exact and unique, whatever order the GPU works in.
 * MOVES AND WEIGHTS: a move changes one, two or three coordinates of a voxel by +-1; its class is the set of coordinates it changes.
 *   `step_weights` is a HOST array of seven uint32, one per class in the order x, y, z, xy, xz, yz, xyz: the cost of a move of the class.
 *   A weight of 0 forbids the class (6-connectivity is w, w, w, 0, 0, 0, 0; 18-connectivity has the last weight 0); NULL means the chamfer
 *   weights 3, 3, 3, 4, 4, 4, 5.  A shortest path visits no voxel twice, and since a voxel has one writer and its value only falls, every
 *   value that is ever stored is the cost of such a path: at most wmax (nx ny nz - 1).  A call is refused when that product, taken in
 *   64-bit host arithmetic, exceeds 0xFFFFFFFE, and the device needs no overflow check.
 * GEODESIC: the sources are the voxels of the domain mask whose marker label is non-zero (0 = no marker; any other 32-bit value is a
 *   label, e.g. what svr_region_label writes; a label outside the domain is ignored).  dist(v) = the cost of the cheapest path of allowed
 *   moves from any source to v that stays inside the domain; zone(v) = the SMALLEST label among the sources that attain dist(v).
 *   Equivalently key = (dist, zone) is (0, label) on a source and elsewhere in the domain the lexicographic minimum over the allowed
 *   neighbours u in the domain of (dist(u) + w(u -> v), zone(u)); weights >= 1 make that system's solution unique.  dist is
 *   SVR_GEO_NONE and zone 0 outside the domain and where no source reaches.  Either output may be NULL, not both; zones_device may be
 *   marker_labels_device itself.  With no source at all every dist is SVR_GEO_NONE, every zone 0, and the return is 0.
 *   The work is chaotic relaxation of packed 64-bit keys in tiles of 32 x 8 x 8 voxels, swept until a sweep lowers nothing; workspace
 *   8 bytes per voxel, allocated and freed by the call, which synchronises the stream.  *sweeps_out (may be NULL) = the sweeps launched.
 * SWEEPS: a sweep finishes every voxel whose shortest path crosses one tile face more than those finished before, so C + 2 sweeps are
 *   enough when no shortest path needs more than C crossings; 968 T + 2 (T tiles, 968 voxels on the faces of each) always is, and is no
 *   use as a guard.  max_sweeps = 0 means svr_region_geodesic_default_max_sweeps = min(64 + 16 T, 65536): shortest paths that enter a
 *   tile 16 times on average, e.g. one-voxel corridors between one-voxel walls along x.  A domain that winds more needs max_sweeps from
 *   the caller.  At the cap the call returns SVR_REGION_ERR_SWEEPS; the outputs then hold upper bounds and are NOT valid, *sweeps_out
 *   holds the launches, and the call does not go on.
 * SEED LABELS: zero-fills labels_device and gives the voxel of seed i (a HOST array of (x, y, z), as in svr_region_grow) the label i + 1;
 *   of several seeds on one voxel the lowest i wins.  Asynchronous.
 * WEIGHTS FROM A SPACING (plain host code): unit = min(spacing) / 2^k for the largest k in 3, 2, 1, 0 whose weights
 *   w = max(1, llround(len / unit)), len the Euclidean length of a move of the class in the spacing's units, pass the overflow bound; the
 *   classes beyond `connectivity` (6: one coordinate, 18: up to two, 26: all) get 0.  An isotropic spacing gives 8, 11, 14 at k = 3.  A map
 *   value d then means about d unit.  CHAMFER ERROR: a path of moves is never shorter than the straight line; with exact move lengths and
 *   no obstacle it is longer by at most 12.8 % (26), 22.5 % (18: sqrt(1.5)) or 73.2 % (6: sqrt(3)) in the worst direction, and the rounding
 *   of a weight moves it by at most 0.5 / w (6 % at k = 3).  The chamfer weights 3, 4, 5 give between 5.7 % less
 *   and 10.6 % more than three times the Euclidean length.
 * SPLIT: E = svr_region_ball(in, SVR_MORPH_ERODE, dist_weights, r2); (labels, K) = svr_region_label(E, connectivity); zones = the zones
 *   of those labels inside `in`.  NULL step weights mean the chamfer weights with the classes beyond `connectivity` set to 0.
 *   *count_out = K: zone k is the part of `in` around the k-th core in svr_region_label's numbering.  *unreached_out = the voxels of `in`
 *   with zone 0: pieces too thin to hold a core.  K = 0 gives all zeros, unreached = |in| and return 0.  The zones feed
 *   svr_region_label_table, svr_region_select and svr_region_select_by_size unchanged.  Workspace: that of the three steps, one after
 *   the other, and one mask.  count_out, unreached_out are required, sweeps_out may be NULL.  Synchronises.
 * ZONE CUT: a voxel is kept iff its zone is non-zero and none of its connectivity-neighbours inside the volume has a non-zero zone that
 *   is SMALLER: of every adjacent pair in different zones the larger label goes, so the cut is one voxel thick and every connected
 *   component of `out` lies in one zone.  Asynchronous.
 * REFUSED, before the device is touched and with nothing written: a null pointer where one is required, or both outputs NULL (-4); a
 *   dimension <= 0 or more than 2^31 voxels (-6); all seven weights 0, the overflow bound, a connectivity other than 6 / 18 / 26, nseeds
 *   == 0 or > SVR_REGION_MAX_SEEDS, a seed outside the volume, the weight and bound refusals of svr_region_ball for dist_weights, an `out`
 *   that overlaps an input other than zones over marker labels, a spacing that is not positive and finite or that no k fits (-3). */
#define SVR_GEO_NONE 0xFFFFFFFFu
uint32_t svr_region_geodesic_default_max_sweeps(int nx, int ny, int nz);
int svr_region_geodesic(const uint32_t* marker_labels_device, const uint32_t* domain_mask_device, int nx, int ny, int nz,
                        const uint32_t* step_weights_or_null, uint32_t max_sweeps, uint32_t* dist_device_or_null, uint32_t* zones_device_or_null,
                        uint32_t* sweeps_out);
int svr_region_seed_labels(const int32_t* seeds_xyz, uint32_t nseeds, int nx, int ny, int nz, uint32_t* labels_device);
int svr_region_geodesic_weights(const double spacing[3], int connectivity, int nx, int ny, int nz, uint32_t weights[7], double* unit_out);
int svr_region_split(const uint32_t* in_mask_device, int nx, int ny, int nz, const uint32_t* dist_weights_or_null, uint32_t r2, int connectivity,
                     const uint32_t* step_weights_or_null, uint32_t max_sweeps, uint32_t* zones_device, uint32_t* count_out, uint32_t* unreached_out,
                     uint32_t* sweeps_out);
int svr_region_zone_cut(const uint32_t* zones_device, int nx, int ny, int nz, int connectivity, uint32_t* out_mask_device);
/* HIP-event time of the device work of the last svr_region_geodesic, the zones step of the last svr_region_split, or the last
 * svr_region_seed_labels / svr_region_zone_cut, whichever came last (waits for it) */
int svr_region_geodesic_last_ms(float* ms);

/* ---- grow from seeds: multi-label segmentation by image-weighted shortest paths (csrc/svr_growcut.hip) ----
 * The user marks a few voxels of every class (1 = the object, 2 = the background, ...); every voxel of the domain then goes to the class
 * whose markers reach it over the path that crosses the least image contrast: Fast GrowCut (Zhu et al.), the shortest-path form of
 * GrowCut.  Masks, label, cost and zone arrays are as in the geodesic section; dimensions are const int32_t dims[3] = (x, y, z).
 * Integers only; every result is exact and unique, whatever order the GPU works in.
 * THE COST OF A MOVE between allowed neighbours u, v of class c (the classes and `step_weights` of the geodesic section; 0 forbids a
 *   class):  cost(u, v) = step_weights[c] + contrast_gain * (|I(u) - I(v)| >> contrast_shift),  I the raw u16 voxel as in svr_volume_rank.
 *   It is symmetric and at least 1.  contrast_gain lies in 0 .. 65535, contrast_shift in 0 .. 15, and a call is refused when
 *   wmax + contrast_gain * (65535 >> contrast_shift) > 0x7FFFFFFF: dist(u) + cost then stays below 2^33 and 64-bit arithmetic needs no
 *   further check.
 * THE RESULT, with sat(x) = min(x, SVR_GROWCUT_CAP): key(v) = (cost, zone) is the lexicographic minimum, over all walks inside the domain
 *   from a source to v, of (sat(cost of the walk), label of its source).  Sources are the voxels of the domain with a non-zero marker
 *   label; their key is (0, label).  Outside the domain and where no source reaches, cost is SVR_GEO_NONE and zone 0.  A NULL domain means
 *   the whole volume.  Either output may be NULL, not both; zones_device may be marker_labels_device itself.  With no source at all every
 *   cost is SVR_GEO_NONE, every zone 0, and the return is 0.  With contrast_gain = 0 the result is svr_region_geodesic's, bit for bit.
 *   voxels is host memory, or device memory with src_is_device; a host source is uploaded once.  Workspace 8 bytes per voxel; the call
 *   synchronises the stream.  *info_or_null receives the sweeps launched, the voxels of the domain that no source reaches, and the
 *   voxels whose cost is the cap.
 * SATURATION: the a-priori bound of the geodesic call, wmax (voxels - 1) <= 0xFFFFFFFE, is NOT applied here -- it would allow 31 per move
 *   at 512^3.  The device adds with saturation at SVR_GROWCUT_CAP instead.  Since sat(sat(a) + w) = sat(a + w), saturating after every
 *   move equals saturating a walk's sum, so every key ever stored is the (sat(cost), label) of a real walk, and the state in which no
 *   voxel can fall is the minimum over walks above: one solution, reached in any order from "all NONE" (DESIGN.md 8q).  If info->saturated
 *   is non-zero the call returns SVR_REGION_ERR_RANGE and the error text says to raise contrast_shift or lower contrast_gain; the outputs
 *   then hold the saturated solution above -- defined, but flagged: on the plateau cost = CAP the zone is the smallest label that reaches
 *   it at all.
 * SWEEPS: params->max_sweeps = 0 means svr_region_geodesic_default_max_sweeps of the dimensions; at the cap the call returns
 *   SVR_REGION_ERR_SWEEPS as svr_region_geodesic does (outputs are upper bounds and NOT valid; info->sweeps holds the launches).
 * PARAMS DEFAULT (plain host code): weight 1 on the classes of connectivity 6 / 18 / 26 and 0 on the others, gain 1, shift 0, max_sweeps 0.
 * SEED CLASSES: zero-fills labels_device and gives the voxel of seed i (HOST arrays of (x, y, z) and of classes) the label classes[i]; of
 *   several seeds on one voxel the lowest i wins.  Asynchronous.
 * LABEL PAINT: writes `label` (non-zero) on every voxel whose mask bit is set, or only where the current label is 0 when only_unlabelled
 *   is set; padding bits are ignored.  This is how a brush stroke becomes a marker: a seed mask dilated by svr_region_ball, or any mask
 *   the chain made.  Asynchronous.
 * REFUSED, before the device is touched and with nothing written: a null pointer where one is required, or both outputs NULL (-4); a
 *   dimension <= 0 or more than 2^31 voxels (-6); (-3) all seven weights 0, a gain above 65535, a shift above 15, the move-cost bound, a
 *   connectivity other than 6 / 18 / 26, a class or label of 0, nseeds == 0 or > SVR_REGION_MAX_SEEDS, a seed outside the volume, an
 *   output that overlaps an input other than zones over marker labels, labels that overlap the mask. */
typedef struct svr_growcut_params {
    uint32_t step_weights[7];   /* per move class x, y, z, xy, xz, yz, xyz as in svr_region_geodesic; 0 forbids the class */
    uint32_t contrast_gain;     /* 0 .. 65535 */
    uint32_t contrast_shift;    /* 0 .. 15 */
    uint32_t max_sweeps;        /* 0 = svr_region_geodesic_default_max_sweeps of the dims */
} svr_growcut_params;           /* 40 bytes */
typedef struct svr_growcut_info { uint32_t sweeps; uint64_t unreached; uint64_t saturated; } svr_growcut_info;   /* 24 bytes */
#define SVR_GROWCUT_CAP 0xFFFFFFFEu
#define SVR_REGION_ERR_RANGE (-12)   /* costs reached SVR_GROWCUT_CAP: the outputs hold the saturated solution */

int svr_region_growcut_params_default(svr_growcut_params* p, int connectivity);
int svr_region_growcut(const uint16_t* voxels, const int32_t dims[3], int src_is_device,
                       const uint32_t* marker_labels_device, const uint32_t* domain_mask_device_or_null,
                       const svr_growcut_params* params,
                       uint32_t* cost_device_or_null, uint32_t* zones_device_or_null, svr_growcut_info* info_or_null);
int svr_region_seed_classes(const int32_t* seeds_xyz, const uint32_t* classes, uint32_t nseeds, const int32_t dims[3], uint32_t* labels_device);
int svr_region_label_paint(uint32_t* labels_device, const int32_t dims[3], const uint32_t* mask_device, uint32_t label, int only_unlabelled);
/* HIP-event time of the device work of the last svr_region_growcut / _seed_classes / _label_paint, whichever came last (waits for it) */
int svr_region_growcut_last_ms(float* ms);

/* ---- histograms of the u16 voxels: whole volume, inside a mask, per label; exact Otsu and quantiles (csrc/svr_histogram.hip;
 *      DESIGN.md 8r) ----
 * The histogram of the voxels the chain works on (after svr_volume_rank / _smooth / _resample), optionally inside a region mask (the
 * layout of the region section; padding bits are ignored, whatever they hold) or per part of a label array (any uint32 per voxel: the
 * components of svr_region_label, the zones of svr_region_split, the classes of svr_region_growcut).  Dimensions are const int32_t
 * dims[3] = (x, y, z).  Integers only; every result is exact and unique, whatever order the GPU works in.  The calls are stateless,
 * run on the library's stream and touch no scene, option or accumulator.
 * PARAMS: a voxel of value v counts iff it lies in the inclusive box (cut to the volume) and lo <= v <= hi; its bin is (v - lo) >> shift.
 *   There are svr_histogram_bins = ((hi - lo) >> shift) + 1 bins (at most 65536); the last may be narrower than 1 << shift.  Voxels
 *   outside the window are not counted (they are not clamped into the end bins).  params == NULL means the defaults: 0 .. 65535,
 *   shift 0, the whole volume.  svr_histogram_bin_range gives the raw values of a bin, lo + (bin << shift) .. min(hi, lo + ((bin + 1) <<
 *   shift) - 1): the window that svr_region_threshold takes.
 * VOLUME HISTOGRAM: counts_device[b], svr_histogram_bins entries, = the number of voxels in the box whose mask bit is set (every voxel
 *   with a NULL mask) and whose value falls in bin b.  A count fits in uint32 because a volume has at most 2^31 voxels.  The output is
 *   overwritten, not accumulated.  voxels is host memory, or device memory with src_is_device; a host source is uploaded once and the
 *   call then synchronises the stream; with a device source the call is asynchronous.
 * LABEL HISTOGRAM: counts_device is [count + 1][bins]; row l counts the voxels whose label is l, row 0 the background; labels above
 *   `count` are ignored as in svr_region_label_table.  count == 0 is allowed and gives the background row alone.  (count + 1) * bins
 *   may not exceed SVR_HISTOGRAM_MAX_CELLS.
 * REFUSED, before the device is touched: a null pointer (-4); a dimension <= 0 or more than 2^31 voxels (-6); (-3) lo > hi, hi > 65535,
 *   shift > 15, a box that is inverted or has no voxel of the volume in it, more than SVR_HISTOGRAM_MAX_CELLS cells, a counts_device
 *   that overlaps an input.
 * ANALYSIS of a HOST histogram is plain host code: no device, any uint32 counts (a row of the label table, a caller's own).  `bins`
 *   >= 1; indices below are bin indices.  With N = the total count, N == 0 returns SVR_HISTOGRAM_STATUS_EMPTY with the outputs 0
 *   (a status, not an error: svr_last_error_code is unchanged); bins == 0 or a null pointer is refused (-3 / -4).
 *   MOMENTS: n = sum c[b], sum = sum b c[b], sum_sq = sum b^2 c[b], added in 128 bits; a histogram of a volume (N <= 2^31, bins
 *     <= 65536) stays below 2^63, and a caller's counts whose sums do not fit 64 bits are refused (-3).
 *   QUANTILE (den > 0, num <= den, else -3): with C(b) the count through bin b, the smallest b with C(b) > 0 and den * C(b) >= num * N,
 *     compared in 128 bits.  num = 0 gives the first occupied bin, num = den the last; for 0 < q <= 1 this is numpy's
 *     percentile(method="inverted_cdf").
 *   OTSU: classes = 2, or 3 with bins <= 256 (anything else -3; coarsen with `shift`).  thresholds_out receives classes - 1 values
 *     t_1 < ... , each in 0 .. bins - 2: the LAST bins of the lower classes (class j spans t_{j-1} + 1 .. t_j, t_0 = -1, the last class
 *     ends at bins - 1).  Chosen is the tuple that maximises sum_j S_j^2 / N_j (N_j the count of class j, S_j = sum b c[b] over it, an
 *     empty class contributes 0), which has the maximiser of the between-class variance; the comparison is exact (256-bit cross
 *     products), and ties go to the lexicographically smallest tuple.  bins < classes (no such tuple) is -3.  *eta_out (may be NULL)
 *     = between-class variance / total variance as a double (0 when the total variance is 0): informative only. */
#define SVR_HISTOGRAM_MAX_CELLS 16777216u     /* (count + 1) * bins of svr_region_label_histogram: 64 MB of counters */
#define SVR_HISTOGRAM_STATUS_EMPTY 1
typedef struct svr_histogram_params {   /* 4-byte members only, 36 bytes */
    uint32_t lo, hi;                    /* inclusive raw-value window; voxels outside it are not counted */
    uint32_t shift;                     /* 0 .. 15: bin(v) = (v - lo) >> shift */
    int32_t  box_min[3], box_max[3];    /* inclusive voxel box, intersected with the volume */
} svr_histogram_params;
int      svr_histogram_params_default(svr_histogram_params* p);      /* 0 .. 65535, shift 0, 0 .. INT32_MAX */
uint32_t svr_histogram_bins(const svr_histogram_params* p);          /* ((hi - lo) >> shift) + 1; 0 for invalid params */
int      svr_histogram_bin_range(const svr_histogram_params* p, uint32_t bin, uint32_t* v_lo, uint32_t* v_hi);

int svr_volume_histogram(const uint16_t* voxels, const int32_t dims[3], int src_is_device, const uint32_t* mask_device_or_null,
                         const svr_histogram_params* params_or_null, uint32_t* counts_device);
int svr_region_label_histogram(const uint32_t* labels_device, const uint16_t* voxels, const int32_t dims[3], int src_is_device,
                               uint32_t count, const svr_histogram_params* params_or_null, uint32_t* counts_device);
/* HIP-event time of the device work of the last svr_volume_histogram / svr_region_label_histogram (waits for it) */
int svr_volume_histogram_last_ms(float* ms);

int svr_histogram_moments(const uint32_t* counts, uint32_t bins, uint64_t* n, uint64_t* sum, uint64_t* sum_sq);
int svr_histogram_quantile(const uint32_t* counts, uint32_t bins, uint32_t num, uint32_t den, uint32_t* bin_out);
int svr_histogram_otsu(const uint32_t* counts, uint32_t bins, uint32_t classes, uint32_t* thresholds_out, double* eta_out);

/* ---- overlays: region masks and label maps on slices and 3D views (csrc/svr_overlay.hip) ----
 * Per-pixel region ids, outlines, and a blend onto the RGBA8 images that svr_render_slice, svr_render_slice_stack, render_raycasting and
 * svr_render_projection write.  Integers only, but for the sample points of a slice, which are the float32 points of the slice section;
 * every result is exact.
 * SOURCE: exactly one pointer of svr_overlay_source is non-NULL.  mask_device: a bit mask in the region layout (padding bits ignored,
 *   whatever they hold); labels_device: the dense uint32 [nz][ny][nx] of svr_region_label / svr_region_split.  The ID of voxel (x, y, z) is
 *   its mask bit (0 or 1) or its label.
 * VOXEL OF A POINT p: the mapping of svr_region_seed_from_world, to the letter.  Per axis tc = fl(fl(p - bbox.vmin) * bbox.invSize) on the
 *   UNCLIPPED box, i = floor(tc * n) with the product taken exactly (a float32 times an int below 2^31 is exact in double), i = n clamped
 *   to n - 1.  A point with any tc outside [0, 1], or NaN, has id 0: it is not refused.  The linear index is formed in 64 bits.
 * ID OF A SLICE PIXEL: the samples are those of the slice section (FRAME, SLICE k, PLANE POINT, SLAB SAMPLES, BOX) with the same counting
 *   rule; the pixel's id is the SMALLEST NON-ZERO id among the voxels of its counting samples, 0 if there is none or no sample counts.
 *   (Independent of the order of the samples.)  mode, window_lo, window_hi and flags of the params are not looked at; thickness, step,
 *   count and spacing are checked as svr_render_slice_stack checks them.
 * ID OF A HIT PIXEL: a record with status SVR_HIT_STATUS_FOUND has the id of the voxel of `position`; any other record has id 0.  Only
 *   `status` and `position` are read.
 * EDGE: a pixel with id k != 0 is an edge pixel iff one of its four neighbours (x +- 1, y), (x, y +- 1) INSIDE the image has an id != k.
 *   Neighbours outside the image are not looked at; in a stack only neighbours in the same slice count.
 * STYLE: fill_alpha and edge_alpha lie in 0 .. 255, flags must be 0.  palette is a HOST array of palette_count RGBA8 entries (r in the low
 *   byte, a in the high byte), 1 .. SVR_OVERLAY_MAX_PALETTE, read before the call returns (it travels to the kernel by value).  palette ==
 *   NULL with palette_count == 0 selects the built-in table of SVR_OVERLAY_DEFAULT_PALETTE fully opaque colours:
 *     (230, 25, 75) (60, 180, 75) (255, 225, 25) (0, 130, 200) (245, 130, 48) (145, 30, 180)
 *     (70, 240, 240) (240, 50, 230) (210, 245, 60) (250, 190, 212) (0, 0, 128) (170, 110, 40).
 * BLEND of a pixel with id k != 0: e = palette[(k - 1) mod palette_count], A = edge ? edge_alpha : fill_alpha, a = (A * e.a + 127) / 255.
 *   a == 0: the pixel is not written.  Otherwise each of r, g, b becomes (in * (255 - a) + e.c * a + 127) / 255 (integer division); the
 *   alpha byte stays.  A pixel with id 0 is never written; an entry with e.a == 0 hides its labels.
 * svr_slice_ids writes `count` id images of w x h uint32, back to back; it honours svr_set_row_shard and svr_set_render_window (ids
 *   outside stay untouched).  svr_hit_ids writes one id image from a FULL hit map of w x h records and svr_overlay_ids blends `count` id
 *   images over `count` RGBA8 images in place; both are whole-image post-processes and ignore shard and window.  svr_overlay_slice is
 *   svr_slice_ids followed by svr_overlay_ids in one kernel, without the id images: it writes the owned pixels only and judges their
 *   edges from the true ids of their neighbours, owned or not, so a sharded or windowed overlay equals the cut-out of the full one.
 *   All honour svr_set_stream and are asynchronous.
 * REFUSED, before the device is touched and with nothing written: a null argument (-4); a dimension <= 0 or more than 2^31 voxels (-6);
 *   both or neither source pointer, an alpha above 255, flags != 0, palette_count > SVR_OVERLAY_MAX_PALETTE, a palette without a count
 *   or a count without a palette, w, h or count of 0, a non-finite bbox, and what svr_render_slice_stack refuses about center, u, v,
 *   thickness, step, count and spacing (-3). */
#define SVR_OVERLAY_MAX_PALETTE 256
#define SVR_OVERLAY_DEFAULT_PALETTE 12

typedef struct svr_overlay_source {
    const uint32_t* mask_device;     /* bit mask in the region layout, or NULL */
    const uint32_t* labels_device;   /* uint32 [nz][ny][nx], or NULL */
} svr_overlay_source;

typedef struct svr_overlay_style {
    uint32_t fill_alpha, edge_alpha; /* 0 .. 255: opacity of the tint inside a part / on its outline */
    uint32_t palette_count, flags;
    const uint32_t* palette;         /* HOST array of palette_count RGBA8 entries, or NULL with palette_count 0: the built-in table */
} svr_overlay_style;

int svr_overlay_style_default(svr_overlay_style* style);             /* fill 96, edge 255, built-in palette.  Plain host code */
/* the first n <= SVR_OVERLAY_DEFAULT_PALETTE entries of the built-in table.  Plain host code */
int svr_overlay_palette_default(uint32_t* out, uint32_t n);
/* (nx, ny, nz: the dimensions of the mask or label array, which the image calls below only index) */
int svr_slice_ids(uint32_t* ids_device, const svr_volume* volume,
                  int nx, int ny, int nz, uint32_t w, uint32_t h, const svr_slice_params* p, uint32_t count, float spacing,
                  const svr_overlay_source* source);
int svr_hit_ids(uint32_t* ids_device, const void* hits_device, uint32_t w, uint32_t h, const svr_volume* volume,
                int nx, int ny, int nz, const svr_overlay_source* source);
int svr_overlay_ids(void* imgs, const uint32_t* ids_device, uint32_t w, uint32_t h, uint32_t count, const svr_overlay_style* style);
int svr_overlay_slice(void* imgs, const svr_volume* volume,
                      int nx, int ny, int nz, uint32_t w, uint32_t h, const svr_slice_params* p, uint32_t count, float spacing,
                      const svr_overlay_source* source, const svr_overlay_style* style);
/* HIP-event time of the device work of the last of the four device calls above (waits for it) */
int svr_overlay_last_ms(float* ms);

/* ---- surface meshes of region masks and isosurfaces by surface nets (csrc/svr_mesh.hip) ----
 * Integers only; the mesh is defined index for index, whatever order the GPU works in.
 * FIELD: a u16 volume [nz][ny][nx] with a raw level in 1 .. 65535; sample (x, y, z) is INSIDE iff v >= level.  A region mask is the
 *   field with value 2 inside and 0 outside at level 1 (padding bits ignored, whatever they hold).  The volume is surrounded by one
 *   layer of virtual samples of value 0, so every mesh is closed, also where the object touches a face of the volume.  Padded sample
 *   coordinates are x' = x + 1, in 0 .. nx + 1.
 * CELLS: cell (i, j, k), i in 0 .. nx (likewise j, k), has the eight padded samples i .. i + 1 x j .. j + 1 x k .. k + 1 as corners; it is
 *   ACTIVE iff its corners are neither all inside nor all outside.
 * CROSSING POINT: a cell edge crosses the surface when one end is inside (value vi) and the other outside (value vo); the point lies
 *   q = floor(256 (level - vo) / (vi - vo)) from the outside end, i.e. q from the edge's lower-coordinate end if that end is outside
 *   and 256 - q otherwise.
 * VERTEX: non-negative int32 (x, y, z) in units of 1/256 voxel on the padded grid, u = 256 x': real sample x sits at 256 (x + 1).  An
 *   active cell with m crossing edges (3 .. 12) has per axis the coordinate 256 i + (2 S + m) / (2 m) (integer division), S = the sum
 *   of the crossing points' cell-relative coordinates (each 0 .. 256).  Vertices are numbered in ascending linear cell index
 *   (k (ny + 1) + j)(nx + 1) + i.
 * QUADS: one per crossing edge from padded sample s to s + e_a; (a, b, c) cyclic: x -> (y, z), y -> (z, x), z -> (x, y).  With the
 *   four cells that contain the edge written by their (b, c) offsets from the cell with index s, the quad is C(-1,-1), C(0,-1),
 *   C(0,0), C(-1,0) if s is inside and C(-1,-1), C(-1,0), C(0,0), C(0,-1) if s + e_a is: normals point out of the object.  Quads
 *   are ordered by the key 3 ((z' (ny + 2) + y')(nx + 2) + x') + a; quad n = (q0, q1, q2, q3) is the triangles (q0, q1, q2) at 2 n
 *   and (q0, q2, q3) at 2 n + 1.  Two objects that touch along an edge or at a corner share vertices there (a non-manifold edge).
 * RELAXATION (relax = 0 .. SVR_MESH_MAX_RELAX Jacobi steps; meant for masks): two active cells are LINKED iff they share a face whose
 *   four corners are mixed; every active cell has at least 3 links.  Per step and axis a vertex becomes (2 T + m) / (2 m), T = the
 *   sum of its m linked neighbours' previous coordinates, then is clamped to its own cell [256 i, 256 i + 256].  Connectivity never
 *   changes.  It shrinks convex shapes by a few per cent over many steps; nothing compensates for that.
 * MEASURES (svr_mesh_measure): *volume6_units = the sum of a . (b x c) over the triangles in wrap-around 64-bit arithmetic = 6 * 256^3
 *   times the enclosed volume in voxels (exact; the same wherever a closed mesh lies); *area = the sum of 1/2 |((b - a) o s) x
 *   ((c - a) o s)| in double with the per-axis scale s (spacing / 256), summed in a fixed order.
 * SIZING: both output pointers NULL is a counting call: only *info_host is filled, return 0.  A capacity (in vertices / triangles)
 *   that is too small returns SVR_MESH_ERR_CAPACITY with *info_host filled and nothing written to the outputs.
 * INFO: bbox_min / bbox_max = the inclusive bounds of the vertex coordinates after relaxation (256 (n + 2) per axis and -1 for an
 *   empty mesh, which has status SVR_REGION_STATUS_EMPTY and return 0).
 * svr_mesh_positions (plain host code): float32 positions of `nv` host vertices.  volume_or_null == NULL: millimetres, (u / 256 - 1 +
 *   0.5) * spacing.  With a volume: world coordinates by the sampler's mapping that svr_region_seed_from_world documents -- sample x
 *   sits at texture coordinate (x + 0.5) / nx of the unclipped box, i.e. at bbox.vmin + (u / 256 - 0.5) * volume->spacing; `spacing` is
 *   then not looked at and may be NULL.  Evaluated in double, rounded once.
 * All device calls run on the library's stream and synchronise it.  REFUSED, before the device is touched and with nothing written: a
 *   null pointer (-4); a dimension <= 0 or above SVR_MESH_MAX_DIM, or more than 2^31 cells (-6); level 0 or above 65535, relax above
 *   SVR_MESH_MAX_RELAX, exactly one output pointer NULL, a spacing or scale that is not positive and finite (-3).  A mesh of more than
 *   2^32 / 3 vertices or 2^31 quads is refused (-6) after the classify pass; svr_mesh_measure refuses a triangle that names a vertex >= nv (-3). */
#define SVR_MESH_MAX_RELAX 64
#define SVR_MESH_MAX_DIM 8388606         /* 256 (n + 2) <= 2^31 */
#define SVR_MESH_ERR_CAPACITY (-11)      /* an output array is too small: info holds the sizes, nothing was written */

typedef struct svr_mesh_params {     /* 8 bytes */
    uint32_t level;                  /* 1 .. 65535; ignored for a mask */
    uint32_t relax;                  /* 0 .. SVR_MESH_MAX_RELAX */
} svr_mesh_params;

typedef struct svr_mesh_info {       /* 56 bytes */
    uint64_t vertices, quads, triangles;
    int32_t  bbox_min[3], bbox_max[3];
    int32_t  status;                 /* SVR_REGION_STATUS_* */
    uint32_t _pad;
} svr_mesh_info;

int svr_mesh_params_default(svr_mesh_params* p);                     /* level 32768, relax 0.  Plain host code */
/* voxels: host, or device with src_is_device = 1.  vertices_xyz_device: 3 int32 per vertex; triangles_device: 3 uint32 per triangle */
int svr_mesh_isosurface(const uint16_t* voxels,
                        int nx, int ny, int nz, int src_is_device, const svr_mesh_params* params, int32_t* vertices_xyz_device,
                        uint64_t vertex_capacity, uint32_t* triangles_device, uint64_t triangle_capacity, svr_mesh_info* info_host);
int svr_mesh_region(const uint32_t* mask_device,
                    int nx, int ny, int nz, const svr_mesh_params* params, int32_t* vertices_xyz_device, uint64_t vertex_capacity,
                    uint32_t* triangles_device, uint64_t triangle_capacity, svr_mesh_info* info_host);
int svr_mesh_measure(const int32_t* vertices_device, uint64_t nv, const uint32_t* triangles_device, uint64_t nt, const double scale[3],
                     int64_t* volume6_units, double* area);
int svr_mesh_positions(const int32_t* vertices_host, uint64_t nv, const double spacing[3], const svr_volume* volume_or_null, float* xyz_host);
/* HIP-event times of the phases of the last svr_mesh_isosurface / _region: classify (with the scans), emit, relax (0 for a phase that
 * did not run).  Pointers may be NULL */
int svr_mesh_last_ms(float* classify_ms, float* emit_ms, float* relax_ms);

/* ---- crop and resample volumes, masks and label maps; paste a mask back (csrc/svr_resample.hip) ----
 * Every other volume operation works on the grid the file came in.  These calls change the grid: a crop to a box (cheaper steps on a
 * region of interest), a resampling to another spacing (isotropic voxels for the voxel-unit elements of svr_region_morph and
 * svr_volume_rank) or to other dimensions (a preview-sized copy), and the way back for a mask made on a crop.  Integers only; every
 * result is defined bit for bit and does not depend on scheduling.  Dimensions are const int32_t dims[3] = (x, y, z).
 *
 * THE GRID: per axis an svr_axis_map in Q16 source EDGE coordinates -- source voxel i covers [i << 16, (i + 1) << 16).  Output cell j
 *   covers [a, a + step) with a = origin + j * step (int64).  A crop is step 65536 and origin = b0 << 16.
 * RESAMPLING runs per axis in the order x, y, z on u16 volumes, one rounding per axis (as svr_volume_smooth); the border replicates:
 *   clamp(i) = min(max(i, 0), n - 1).  With c = a + (step >> 1) and arithmetic shifts:
 *     SVR_RESAMPLE_NEAREST  out = v[clamp(c >> 16)]: the source voxel whose cell holds the centre of the output cell.
 *     SVR_RESAMPLE_LINEAR   t = c - 32768, i = t >> 16, f = t & 65535: out = (v[clamp(i)] (65536 - f) + v[clamp(i + 1)] f + 32768) >> 16.
 *     SVR_RESAMPLE_AREA     out = (2 S + step) / (2 step), S = sum_i v[clamp(i)] ov_i over i = a >> 16 .. (a + step - 1) >> 16, where
 *                           ov_i = min(a + step, (i + 1) << 16) - max(a, i << 16) is the overlap of the cell with voxel i (they sum to step).
 *     SVR_RESAMPLE_AUTO     per axis LINEAR where step <= 65536 (the grid is as fine or finer), AREA where it is coarser.
 *   An axis with step 65536 and an origin that is a multiple of 65536 is a shifted copy under every mode and costs no pass of its own.
 * GRID HELPERS (plain host code; null -4, dimensions <= 0 or more than 2^31 voxels -6, everything else -3).  A box is inclusive and is
 *   cut to the volume as the region calls do; NULL box pointers mean the whole volume.
 *     _grid_box      a crop: origin = b0 << 16, step = 65536, count = b1 - b0 + 1.
 *     _grid_spacing  per axis step = llround(65536 target / source), refused outside the step limits; origin = b0 << 16; count =
 *                    max(1, ((b1 - b0 + 1) * 65536 + (step >> 1)) / step); spacing_out (may be NULL) = source * step / 65536, the spacing
 *                    actually applied.  The first cell's lower edge is the box's lower face: the result fills the same physical box up
 *                    to the rounding of count.
 *     _grid_dims     target dimensions: step = ((b1 - b0 + 1) * 65536 + out_dim / 2) / out_dim, origin = b0 << 16, count = out_dim.
 *     _grid_place    *out = *src with bbox (vmin, vmax, invSize), spacing and invSpacing replaced, so that the result is drawn where it
 *                    lay inside the source volume's box: vmin + origin / 65536 * spacing and vmin + (origin + count * step) / 65536 *
 *                    spacing per axis, in double, rounded to float; spacing * step / 65536.  tex is copied unchanged (the caller
 *                    replaces it); invMaxMagnitude, densityScale, gradientFactor and the clips are copied, so a crop shades as the
 *                    full volume does -- and a RESAMPLED volume keeps the source's gradient normalisation, although its gradients are
 *                    taken over other distances.
 * svr_volume_resample: voxels is host memory, or device memory with src_is_device; out holds count_x * count_y * count_z u16.  The
 *   library allocates and frees at most two intermediate volumes; a call that used one, or that uploaded a host source, synchronises
 *   before it returns.  A one-kernel call (a crop, NEAREST, or one resampled axis) on a device source is asynchronous on the library's stream.
 * svr_region_resample: NEAREST on bit masks in the layout of svr_region_grow -- the mask of the NEAREST-resampled 0 / 1 volume.  Input
 *   padding bits are ignored, output padding bits are 0.
 * svr_region_label_resample: NEAREST on uint32 maps: label maps and zone maps on any grid.  A squared-distance map may be CROPPED with
 *   it; a resampled distance is not a distance on the new grid.
 * svr_region_paste: the inverse of a crop.  The sub-mask lies at offset_xyz inside the full mask; inside that box the full mask takes
 *   the sub-mask's bits (SVR_PASTE_REPLACE), gains them (SVR_MASK_OR) or loses them (SVR_MASK_ANDNOT); bits outside the box keep their
 *   value, also in the words the box's x faces cut through.  A sub-volume that does not fit at the offset is refused (-3).
 * svr_region_mask_expand: one byte per voxel, `value` (1 .. 255) inside the mask and 0 outside: what a mask is saved from
 *   (svr_mhd_write).  The way back: svr_region_threshold with the window 1 .. 65535 on the loaded file.
 * Refused before the device is touched, with nothing written: a null pointer (-4); source or output dimensions <= 0 or more than 2^31
 *   voxels (-6); (-3) a step outside SVR_RESAMPLE_MIN_STEP .. _MAX_STEP, count == 0, an axis whose cells [origin, origin + count * step)
 *   do not meet the source extent [0, n << 16), |origin| >= 2^47, an unknown mode, op or value, an `out` that overlaps an input. */
#define SVR_RESAMPLE_NEAREST 0
#define SVR_RESAMPLE_LINEAR  1
#define SVR_RESAMPLE_AREA    2
#define SVR_RESAMPLE_AUTO    3
#define SVR_RESAMPLE_MIN_STEP 1024u      /* 1 / 64 voxel */
#define SVR_RESAMPLE_MAX_STEP 4194304u   /* 64 voxels */
#define SVR_PASTE_REPLACE 0              /* the other ops of svr_region_paste are SVR_MASK_OR and SVR_MASK_ANDNOT */

typedef struct svr_axis_map {        /* 16 bytes */
    int64_t  origin;                 /* lower edge of output cell 0, in source edge coordinates, Q16 */
    uint32_t step;                   /* width of an output cell, Q16 */
    uint32_t count;                  /* output voxels on this axis, >= 1 */
} svr_axis_map;
typedef struct svr_resample_grid { svr_axis_map axis[3]; } svr_resample_grid;   /* x, y, z; 48 bytes */

int svr_resample_grid_box(const int32_t src_dims[3], const int32_t box_min[3], const int32_t box_max[3], svr_resample_grid* grid);
int svr_resample_grid_spacing(const int32_t src_dims[3], const double src_spacing[3], const int32_t* box_min_or_null,
                              const int32_t* box_max_or_null, const double target_spacing[3], svr_resample_grid* grid, double* spacing_out);
int svr_resample_grid_dims(const int32_t src_dims[3], const int32_t* box_min_or_null, const int32_t* box_max_or_null,
                           const int32_t out_dims[3], svr_resample_grid* grid);
int svr_resample_grid_place(const svr_volume* src, const int32_t src_dims[3], const svr_resample_grid* grid, svr_volume* out);
int svr_volume_resample(const uint16_t* voxels, const int32_t src_dims[3], int src_is_device, const svr_resample_grid* grid, int mode,
                        uint16_t* out_u16_device);
int svr_region_resample(const uint32_t* in_mask_device, const int32_t src_dims[3], const svr_resample_grid* grid, uint32_t* out_mask_device);
int svr_region_label_resample(const uint32_t* in_u32_device, const int32_t src_dims[3], const svr_resample_grid* grid, uint32_t* out_u32_device);
int svr_region_paste(const uint32_t* sub_mask_device, const int32_t sub_dims[3], uint32_t* full_mask_device, const int32_t full_dims[3],
                     const int32_t offset_xyz[3], int op);
int svr_region_mask_expand(const uint32_t* mask_device, const int32_t dims[3], int value, uint8_t* out_u8_device);
/* HIP-event time of the device work of the last svr_volume_resample / svr_region_resample / _label_resample / _paste / _mask_expand */
int svr_volume_resample_last_ms(float* ms);

/* ---- comparing segmentations: surfaces, overlap tables and exact surface distances (csrc/svr_compare.hip) ----
 * Masks are DEVICE pointers in the layout of the region section; input padding bits are ignored whatever they hold (and count as unset
 * neighbours), output padding bits are 0.  Maps and label arrays are dense uint32 [nz][ny][nx] on the device.  Dimensions are nx, ny,
 * nz, or const int32_t dims[3] = (x, y, z).  Integers only on the device; every result is exact and unique, whatever order the GPU
 * works in.  The calls are stateless, run on the library's stream and touch no scene, option or accumulator.
 * SURFACE: out = the voxels of `in` that have a neighbour under the unit element 6 / 18 / 26 that is unset OR LIES OUTSIDE THE VOLUME:
 *   in & ~binary_erosion(in, border_value=0), the convention of the usual surface-distance tools and of this library's meshes, which
 *   are closed at the faces of the volume.  This is NOT the border rule of svr_region_morph's ERODE (there nothing outside the volume
 *   counts as background, and a region is not eroded from a face): in & ~ERODE(in) misses the voxels that touch a face.  out may not
 *   overlap in.  Asynchronous.
 * OVERLAP: counts_host[4] = the voxels of the domain (every voxel when it is NULL) that are in both masks, in A only, in B only, in
 *   neither (SVR_OVERLAP_*).  Synchronises.
 * LABEL OVERLAP: table_device is uint32 [count_a + 1][count_b + 1]; cell la * (count_b + 1) + lb = the number of voxels with label la
 *   in A and lb in B; row 0 and column 0 are the backgrounds.  A voxel with a label above its count is not counted.  count_a, count_b
 *   >= 1, and the cells may not exceed SVR_HISTOGRAM_MAX_CELLS.  The table is overwritten, not accumulated.  Asynchronous.
 * OVERLAP MATCH (plain host code, on a host copy of that table): best_b_for_a[la - 1], la = 1 .. count_a, = the label lb in 1 ..
 *   count_b with the largest Jaccard index inter / (|la| + |lb| - inter), inter = cell (la, lb), |la| = the sum of row la and |lb| = the
 *   sum of column lb, background cells included; fractions are compared exactly by 64-bit cross-multiplication (in 128 bits); ties go
 *   to the lower label; 0 where no lb has inter > 0.  best_a_for_b_or_null[lb - 1] is the same the other way round.
 * SUMMARY of a uint32 map (squared distances, geodesic distances, growcut costs) over the voxels of a mask (all voxels when NULL):
 *   svr_distance_summary below.  tolerances2: a HOST array of ntol <= SVR_COMPARE_MAX_TOLERANCES values (NULL with ntol = 0).
 *   Synchronises.
 * HISTOGRAM of such a map over a mask: counts_device[(v - lo) >> shift] for the values lo <= v <= hi; bins = ((hi - lo) >> shift) + 1,
 *   at most 65536; shift <= 31.  Values outside lo .. hi are not counted, so SVR_DIST_NONE is counted only when hi reaches it.  The
 *   counts are overwritten, not accumulated.  Asynchronous.
 * QUANTILE: *value_out = the smallest value v other than SVR_DIST_NONE with C(v) > 0 and den C(v) >= num N, C the cumulative count and
 *   N the number of such values: the rule of svr_histogram_quantile on the values themselves (numpy's inverted_cdf for 0 < num / den
 *   <= 1).  Two histogram passes: 0 .. max at the smallest shift that fits 65536 bins, then the chosen bin's values at shift 0.  With no
 *   such value *status = SVR_REGION_STATUS_EMPTY, *value_out = 0 and the return is 0.  Synchronises.
 * COMPARE: the overlap counts of A and B, their surfaces S(A), S(B) under params->element, and per direction the summary and the
 *   quantile of the squared distance to the other surface: ab = svr_region_distance(S(B), weights, SVR_DIST_TO_SET) over S(A), ba the
 *   reverse.  params == NULL means svr_compare_params_default: element 6, weights 1, 1, 1, quantile 95 / 100, no tolerances.  An empty
 *   mask sets SVR_COMPARE_A_EMPTY / _B_EMPTY in status and the return stays 0: the directed fields of a direction FROM an empty mask are
 *   all 0, those of a direction TO an empty mask are 0 but for none = the surface voxels of the other mask (every distance is
 *   SVR_DIST_NONE).  Workspace at its peak: one map (4 bytes per voxel), svr_region_distance's own (8 bytes per voxel), two masks, and
 *   256 KB of counters.  Synchronises.
 * MEASURE (plain host code): svr_compare_measurement from a svr_region_comparison; `unit` is the length of sqrt(d2) = 1 (the unit_out
 *   of svr_region_distance_weights, or 1 for voxel units).  With n_ab = ab.voxels, A = both + a_only, B = both + b_only:
 *     dice = 2 both / (2 both + a_only + b_only);  jaccard = both / (both + a_only + b_only);
 *     volume_difference = 2 (A - B) / (A + B)                                   (signed: positive when A is larger);
 *     hausdorff_ab = unit sqrt(ab.max), hausdorff_ba likewise, hausdorff = the larger of the two;
 *     hausdorff_q_ab = unit sqrt(quantile_ab), hausdorff_q_ba likewise, hausdorff_q = the larger of the two;
 *     assd = unit (ab.sum_root_q8 + ba.sum_root_q8) / 256 / (n_ab + n_ba);
 *     rms = unit sqrt((ab.sum + ba.sum) / (n_ab + n_ba));
 *     surface_dice[k] = (ab.within[k] + ba.within[k]) / (surface[0] + surface[1]) for k < ntol, 0 for the others.
 *   Every operand is converted to double first and the operations are made in the order written.  A value whose denominator is 0 is
 *   NaN; a directed distance with n = 0 is NaN, and so is a symmetric one when either direction is.
 * REFUSED, before the device is touched: a null pointer (-4); a dimension <= 0 or more than 2^31 voxels (-6); (-3) an element that is
 *   not 6, 18 or 26, a weight of 0 or the overflow bound of svr_region_distance, lo > hi, more than 65536 bins, shift > 31, ntol > 8,
 *   den == 0 or num > den, count_a == 0 or count_b == 0, more than SVR_HISTOGRAM_MAX_CELLS cells, an output that overlaps an input. */
#define SVR_OVERLAP_BOTH    0
#define SVR_OVERLAP_A_ONLY  1
#define SVR_OVERLAP_B_ONLY  2
#define SVR_OVERLAP_NEITHER 3
#define SVR_COMPARE_MAX_TOLERANCES 8
#define SVR_COMPARE_A_EMPTY 1
#define SVR_COMPARE_B_EMPTY 2
typedef struct svr_distance_summary {   /* 72 bytes: four uint64, then ten uint32 */
    uint64_t voxels;                    /* the voxels of the mask whose value is not SVR_DIST_NONE */
    uint64_t none;                      /* the voxels of the mask whose value is SVR_DIST_NONE */
    uint64_t sum;                       /* the sum of the values (of `voxels`, as all that follows) */
    uint64_t sum_root_q8;               /* the sum of isqrt(v 2^16) = floor(256 sqrt(v)), isqrt as in svr_region_distance_volume */
    uint32_t max;                       /* the largest value; 0 when voxels == 0 */
    uint32_t first_max;                 /* the smallest linear index (z ny + y) nx + x that attains it; 0 when voxels == 0 */
    uint32_t within[SVR_COMPARE_MAX_TOLERANCES];   /* within[k] = the values <= tolerances2[k]; 0 for k >= ntol */
} svr_distance_summary;
typedef struct svr_compare_params {     /* 4-byte members only, 60 bytes */
    int32_t  element;                   /* 6 / 18 / 26: the element of the surfaces */
    uint32_t weights[3];                /* the weights (x, y, z) of the squared distance, as in svr_region_distance */
    uint32_t q_num, q_den;              /* the quantile of the directed distances */
    uint32_t ntol;                      /* 0 .. SVR_COMPARE_MAX_TOLERANCES */
    uint32_t tolerances2[SVR_COMPARE_MAX_TOLERANCES];   /* squared tolerances, in the units of the map */
} svr_compare_params;
typedef struct svr_region_comparison {  /* 208 bytes; integers only */
    uint64_t overlap[4];                /* SVR_OVERLAP_*: both, A only, B only, neither */
    uint64_t surface[2];                /* the voxels of S(A), S(B) */
    svr_distance_summary ab, ba;        /* the squared distances from S(A) to S(B), from S(B) to S(A) */
    uint32_t quantile_ab, quantile_ba;  /* their q_num / q_den quantiles (squared); 0 when there is no value */
    uint32_t ntol;                      /* as in the params */
    int32_t  status;                    /* SVR_COMPARE_A_EMPTY | SVR_COMPARE_B_EMPTY */
} svr_region_comparison;
typedef struct svr_compare_measurement {   /* 19 doubles, 152 bytes; the formulas are above */
    double dice, jaccard, volume_difference;
    double hausdorff_ab, hausdorff_ba, hausdorff;
    double hausdorff_q_ab, hausdorff_q_ba, hausdorff_q;
    double assd, rms;
    double surface_dice[SVR_COMPARE_MAX_TOLERANCES];
} svr_compare_measurement;
int svr_region_surface(const uint32_t* in_mask_device,
                       int nx, int ny, int nz, int element, uint32_t* out_mask_device);
int svr_region_overlap(const uint32_t* a_mask_device, const uint32_t* b_mask_device,
                       int nx, int ny, int nz, const uint32_t* domain_mask_device_or_null, uint64_t counts_host[4]);
int svr_region_label_overlap(const uint32_t* a_labels_device, uint32_t count_a, const uint32_t* b_labels_device, uint32_t count_b,
                             const int32_t dims[3], uint32_t* table_device);
int svr_overlap_match(const uint32_t* table_host, uint32_t count_a, uint32_t count_b, uint32_t* best_b_for_a, uint32_t* best_a_for_b_or_null);
int svr_region_distance_summary(const uint32_t* map_device, const uint32_t* mask_device_or_null,
                                int nx, int ny, int nz, const uint32_t* tolerances2_or_null, uint32_t ntol, svr_distance_summary* out_host);
int svr_region_distance_histogram(const uint32_t* map_device, const uint32_t* mask_device_or_null, const int32_t dims[3], uint32_t lo,
                                  uint32_t hi, uint32_t shift, uint32_t* counts_device);
int svr_region_distance_quantile(const uint32_t* map_device, const uint32_t* mask_device_or_null, const int32_t dims[3], uint32_t num,
                                 uint32_t den, uint32_t* value_out, int32_t* status);
int svr_compare_params_default(svr_compare_params* p);
int svr_region_compare(const uint32_t* a_mask_device, const uint32_t* b_mask_device,
                       int nx, int ny, int nz, const svr_compare_params* params_or_null, svr_region_comparison* out_host);
int svr_region_compare_measure(const svr_region_comparison* c, double unit, svr_compare_measurement* out);
/* HIP-event time of the device work of the last of the device calls above (waits for it); for svr_region_compare it spans the two
 * svr_region_distance runs as well */
int svr_region_compare_last_ms(float* ms);

/* ---- scissors: cut and paint region masks with a polygon drawn on a view (csrc/svr_scissor.hip) ----
 * The direction the views lack: from a voxel to the pixel it is seen at.  A polygon drawn on the picture is filled on the pixel grid (a
 * STENCIL), and every voxel whose centre is seen inside the fill (the PRISM) is selected, removed from, kept in or added to a mask.
 * STENCIL LAYOUT: the stencil of a w x h image is the region mask of a w x h x 1 volume in the layout of the region section: uint32
 *   [h][ceil(w / 32)], pixel (x, y) is bit x & 31 of word y * wx + (x >> 5), padding bits 0 on output.  svr_region_combine,
 *   svr_region_morph and svr_region_stats_of therefore work on stencils with nx = w, ny = h, nz = 1; dilating a stencil is the width of
 *   a brush.
 * POLYGON: vertices_xy_q8 is a HOST array of (x, y) pairs in 1/256 pixel; the centre of pixel (px, py) is (256 px + 128, 256 py + 128).
 *   contour_counts[k] is the number of vertices of contour k, the contours follow one another in the array and each is closed
 *   implicitly.  The edge set E is the union of all contours' edges, so a second contour inside the first is a hole.
 * FILL RULE: even-odd with the half-open crossing rule, exact in int64.  For pixel centre c and edge (a, b) the edge COUNTS iff
 *   (a.y > c.y) != (b.y > c.y) and c lies strictly to the left of the edge's crossing of the line y = c.y:
 *   cross = (b.x - a.x)(c.y - a.y) - (b.y - a.y)(c.x - a.x), with cross > 0 when b.y > a.y and cross < 0 otherwise.  The pixel is set
 *   iff an odd number of edges count.  Horizontal edges never count.  Polygons that share an edge tile the plane: no pixel is in both
 *   and none in neither.
 * LIMITS: every coordinate satisfies |v| <= 2^23 (SVR_STENCIL_MAX_COORD), so every product stays below 2^49 (a pixel outside the
 *   polygon's bounding box is unset without looking at an edge); at most SVR_STENCIL_MAX_VERTICES vertices in total; each contour has at
 *   least 3; ncontours >= 1; w, h >= 1 and w h <= 2^31.  svr_stencil_polygon is asynchronous on the library's stream; the vertex list is
 *   read before the call returns.  svr_stencil_rect (plain host code) writes the four vertices of the inclusive pixel rectangle x0 ..
 *   x1, y0 .. y1 -- its corners lie on pixel corners: (256 x0, 256 y0), (256 (x1 + 1), 256 y0), (256 (x1 + 1), 256 (y1 + 1)),
 *   (256 x0, 256 (y1 + 1)); it refuses x1 < x0, y1 < y0 and a corner beyond the coordinate limit.
 * PROJECTION: the pixel and the depth at which a view sees a world point P.  Everything is float32 without contraction, with correctly
 *   rounded division; dot(p, q) = (p.x q.x + p.y q.y) + p.z q.z.
 *   CAMERA: the inverse of the pinhole centre ray of the projection section (wm1 = (float)imageW - 1, hm1 = (float)imageH - 1).
 *     d = P - pos per component, a = dot(d, u), b = dot(d, v), c = -dot(d, w), depth = c.  If c > 0 is false (behind the pinhole, or
 *     NaN) the point is seen at no pixel.  Otherwise s = ((a / (c * (aspectRatio * tanFovxOverTwo)) + 1) * 0.5f) * wm1 and
 *     r = ((b / (c * tanFovxOverTwo) + 1) * 0.5f) * hm1, every operation rounded.  The frame u, v, w is TAKEN to be orthonormal, as the
 *     reference's camera makes it; the calls do not check it.
 *   SLICE: the inverse of the PLANE POINT of the slice section for slice 0 of the params on a w x h image.  d = P - center,
 *     a = dot(d, u) / dot(u, u), b = dot(d, v) / dot(v, v), s = a + 0.5f * (float)w, r = b + 0.5f * (float)h, depth = dot(d, n) with n
 *     the FRAME normal of the slice section.  The inverse is exact when u and v are perpendicular, which every svr_slice_params_axis /
 *     _through result satisfies; thickness, step, mode, flags and the window are not looked at.
 *   PIXEL: (floor(s), floor(r)) if 0 <= s < (float)W and 0 <= r < (float)H (comparisons of floats), otherwise none.
 *   svr_scissor_project_camera / _slice are plain host code that runs the very function the kernel runs: 0 with the pixel in xy, 1
 *   with xy = (-1, -1) when the point is seen at no pixel; *depth is written in both cases.
 * VOXEL CENTRE: per axis tc = ((float)i + 0.5f) / (float)n and P = bbox.vmin + (bbox.vmax - bbox.vmin) * tc, every operation rounded,
 *   on the UNCLIPPED box: the mapping that svr_region_seed_from_world inverts.
 * PRISM: voxel (i, j, k) is in the prism iff its centre is seen at a pixel, that pixel's stencil bit is set, and depth_lo <= depth <=
 *   depth_hi (closed, on the float depth itself).  The stencil is that of the camera's imageW x imageH, or of the slice call's w x h.
 *   Depth is a world distance along the view axis: in a slice view depth -t/2 .. t/2 is a slab of thickness t around the plane.
 * OP: SVR_SCISSOR_SELECT out = prism (in may be NULL and is not read); _ERASE_INSIDE out = in & ~prism; _ERASE_OUTSIDE out = in & prism;
 *   _FILL_INSIDE out = in | prism.  out may be in.  Input padding bits are ignored, output padding bits are 0.  Asynchronous.
 * REFUSED, before the device is touched: a null pointer, except `in` with SELECT (-4); a dimension <= 0 or more than 2^31 voxels (-6);
 *   (-3) an unknown op, flags != 0, a NaN depth bound, depth_lo > depth_hi, a non-finite bbox.vmin / vmax, camera frame or position, an
 *   imageW or imageH of 0 or more than 2^31 pixels, a tanFovxOverTwo or aspectRatio that is not finite and > 0; for a slice: w or h of
 *   0 or more than 2^31 pixels, a non-finite member of center, u or v, a cross(u, v) whose length is 0 or not finite; for a polygon:
 *   what LIMITS names. */
#define SVR_STENCIL_MAX_VERTICES 4096
#define SVR_STENCIL_MAX_COORD 8388608      /* 2^23 */
#define SVR_SCISSOR_SELECT        0
#define SVR_SCISSOR_ERASE_INSIDE  1
#define SVR_SCISSOR_ERASE_OUTSIDE 2
#define SVR_SCISSOR_FILL_INSIDE   3
typedef struct svr_scissor_params {     /* 4-byte members only, 16 bytes */
    int32_t  op;                        /* SVR_SCISSOR_* */
    float    depth_lo, depth_hi;        /* the closed depth interval of the prism */
    uint32_t flags;                     /* must be 0 */
} svr_scissor_params;
int svr_scissor_params_default(svr_scissor_params* p);   /* SELECT, -INF .. +INF.  Plain host code */
int svr_stencil_rect(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t vertices_xy_q8[8]);
int svr_stencil_polygon(const int32_t* vertices_xy_q8, const uint32_t* contour_counts, uint32_t ncontours, uint32_t w, uint32_t h,
                        uint32_t* stencil_device);
int svr_scissor_project_camera(const svr_camera* camera, const svr_vec3* point, int32_t xy[2], float* depth);
int svr_scissor_project_slice(const svr_slice_params* slice, uint32_t w, uint32_t h, const svr_vec3* point, int32_t xy[2], float* depth);
int svr_region_scissor_camera(const uint32_t* in_mask_device_or_null,
                              int nx, int ny, int nz, const svr_volume* volume, const svr_camera* camera,
                              const uint32_t* stencil_device, const svr_scissor_params* p, uint32_t* out_mask_device);
int svr_region_scissor_slice(const uint32_t* in_mask_device_or_null,
                             int nx, int ny, int nz, const svr_volume* volume, const svr_slice_params* slice, uint32_t w, uint32_t h,
                             const uint32_t* stencil_device, const svr_scissor_params* p, uint32_t* out_mask_device);
/* HIP-event time of the device work of the last svr_stencil_polygon / svr_region_scissor_camera / _slice (waits for it) */
int svr_region_scissor_last_ms(float* ms);

/* ---- fill between slices: interpolate a region drawn on a few slices (csrc/svr_fillbetween.hip) ----
 * A region drawn on every fifth or tenth slice of one axis (svr_region_scissor_slice with FILL_INSIDE, say) becomes a solid region: the
 * slices between two drawn ones are filled by shape-based interpolation (Raya and Udupa), decided in integers, so the result is unique.
 * Masks are device pointers in the layout of the region section; input padding bits are ignored, output padding bits are 0.  The calls
 * run on the library's stream and touch no scene, option or accumulator.
 * AXIS: 0, 1 or 2 (x, y, z), the slicing axis; slice k is the set of voxels whose coordinate on it is k, and the axis has n_axis of
 *   them.  The two other axes are the in-plane axes u < v (by axis number), of lengths nu and nv; a planar array of a slice is
 *   [nv][nu], u fastest.
 * WEIGHTS: as in svr_region_distance, a host uint32[3], each >= 1, NULL = 1, 1, 1.  The weight of the slicing axis is not used: slices
 *   are equally spaced and the interpolation is linear in the slice index.  The planar squared distance of two voxels of one slice is
 *   wu du^2 + wv dv^2.
 * PLANAR MAP of a slice: a uint32 per voxel of the slice -- for a set voxel the smallest planar squared distance to an unset voxel of
 *   the same slice, for an unset voxel the smallest planar squared distance to a set voxel of the same slice, SVR_DIST_NONE where the
 *   slice holds no voxel of the other kind.  Nothing outside the volume counts, as in svr_region_distance.  The voxel's own mask bit is
 *   the sign.  With unit weights this is round(distance_transform_edt(s)^2) on the set voxels and round(distance_transform_edt(~s)^2)
 *   on the unset ones, per 2D slice.
 * FILL: given keys k_0 < k_1 < ... < k_(m-1), the output equals the input on the key slices and outside k_0 .. k_(m-1).  For a slice k
 *   with a < k < b between consecutive keys a, b let n = b - a, t = k - a, and A, B the planar map values of the voxel's in-plane
 *   position in slices a and b, SVR_DIST_NONE entering as the number 2^32 - 1.  The voxel is set if it is set in both keys, unset if
 *   it is unset in both; set in a only: set iff (n - t)^2 A > t^2 B; set in b only: set iff t^2 B > (n - t)^2 A.  Equality gives
 *   unset.  This is the sign of (n - t) s_a + t s_b for the signed distances s = +-sqrt(map), decided without a square root; both
 *   products fit uint64 because n <= 65535 and the maps are below 2^32.  With SVR_FILL_KEEP_BETWEEN the input bits of the slices between
 *   keys are OR-ed into the result; without it they are replaced.  Consecutive keys with n == 1 have nothing between them; a GAP is a
 *   pair with n >= 2.  Fewer than two keys, or no gap, gives out = in with the padding cleared and the return 0.
 *   KNOWN LIMIT of the method: the shapes of two keys that do not overlap in projection do not travel from one to the other, they fade
 *   out and in.  Two discs of radius 6 (113 voxels) whose centres lie 20 voxels apart in the plane, drawn eight slices apart, give
 *   the per-slice counts 113, 59, 8, 0, 0, 0, 8, 59, 113.
 * svr_region_slice_counts: counts_host[k] = the set voxels of slice k, n_axis entries: how keys are found and how a user interface
 *   marks the slices that hold a drawing.  Synchronises.
 * svr_region_slice_distance: the planar maps of the listed slices, maps_device[nslices][nv][nu]; a NULL list means all n_axis slices in
 *   order (nslices is then not looked at).  The list is a host array, in any order, repeats allowed.  The call allocates and frees its
 *   workspace -- per voxel of the slices it works on together (all of them up to 2^26 voxels, at least one slice) 12 bytes and one bit
 *   -- and synchronises.
 * svr_region_fill_between: params.keys is a host array of nkeys strictly increasing slices inside the axis; NULL means every slice that
 *   holds a set voxel (nkeys is then not looked at).  Explicit keys may name empty slices: that is how a shape is ended.  weights 0, 0, 0
 *   means 1, 1, 1.  out may be in (no other overlap).  *info (may be NULL) receives what was done.  The call counts the slices, makes
 *   planar maps only of the keys that border a gap, uploads a table of n_axis slices (16 bytes each) and fills in ONE pass over the mask.
 *   WORKSPACE, freed on return and reported in info.workspace_bytes: 4 bytes per voxel of the bordering key slices for the maps, the
 *   workspace of svr_region_slice_distance on them, the table, 8 bytes per slice for the counts.  If the maps of all bordering keys
 *   exceed SVR_FILL_MAP_BUDGET_BYTES, or with SVR_FILL_GAP_BY_GAP, the call works in runs of consecutive gaps whose maps fit the
 *   budget (GAP_BY_GAP: one gap, two maps at a time), one pass over the mask per run, with the same result; info.launches counts them.
 *   Synchronises.
 * REFUSED, before the device is touched: a null pointer other than info, a list or keys (-4); a dimension <= 0 or more than 2^31 voxels
 *   (-6); (-3) an axis outside 0 .. 2, a weight of 0 (when any weight of the params is not 0), wu (nu - 1)^2 + wv (nv - 1)^2 >
 *   0xFFFFFFFE, n_axis > 65536 (maps and fill), keys that do not increase strictly or lie outside the axis, nkeys < 0 with keys,
 *   nslices <= 0 with a list, a listed slice outside the axis, unknown flag bits. */
#define SVR_FILL_KEEP_BETWEEN 1u
#define SVR_FILL_GAP_BY_GAP   2u
#define SVR_FILL_MAP_BUDGET_BYTES 1073741824u     /* 2^30: the planar maps svr_region_fill_between keeps at a time */
typedef struct svr_fill_between_params {  /* 32 bytes */
    int32_t  axis;                        /* 0, 1, 2 */
    uint32_t flags;                       /* SVR_FILL_* */
    uint32_t weights[3];                  /* 0, 0, 0 = 1, 1, 1 */
    int32_t  nkeys;
    const int32_t* keys;                  /* host; NULL = every non-empty slice */
} svr_fill_between_params;
typedef struct svr_fill_between_info {    /* 56 bytes */
    int32_t  axis;
    uint32_t keys, gaps, filled_slices;   /* the keys used, the pairs of consecutive keys with n >= 2, the slices between them */
    int32_t  first_key, last_key;         /* -1 without a key */
    uint32_t launches;                    /* passes over the mask: 0 without a gap, 1 unless the map budget or GAP_BY_GAP splits the work */
    uint32_t reserved;
    uint64_t voxels_in, voxels_out;       /* set voxels of the input and of the result */
    uint64_t workspace_bytes;             /* the device memory the call held at its peak */
} svr_fill_between_info;
int svr_fill_between_params_default(svr_fill_between_params* p);   /* axis 2, everything else 0.  Plain host code */
/* (the dimensions stand on a line of their own, as those of the scissor calls do: tests/golden/volume_op_refusals.json lists the calls
 * whose first line holds them and is closed; tests/test_fillbetween_cpu.py holds the refusals of these three) */
int svr_region_slice_counts(const uint32_t* mask_device,
                            int nx, int ny, int nz, int axis, uint64_t* counts_host);
int svr_region_slice_distance(const uint32_t* mask_device,
                              int nx, int ny, int nz, int axis, const uint32_t* weights_or_null,
                              const int32_t* slices_host_or_null, int nslices, uint32_t* maps_device);
int svr_region_fill_between(const uint32_t* in_mask_device,
                            int nx, int ny, int nz, const svr_fill_between_params* p,
                            uint32_t* out_mask_device, svr_fill_between_info* info_or_null);
/* HIP-event time of the device work of the last of the three calls above, without their allocations (waits for it); for a fill: the
 * first count, and from the planar maps to the count of the result, without the wait and the allocations between the two */
int svr_region_fill_between_last_ms(float* ms);
/* of the last svr_region_fill_between that had a gap: the first count of the slices, the planar maps and the fill pass (of the last
 * launch where there were several); 0 where there was none.  Any pointer may be NULL */
int svr_region_fill_between_pass_ms(float* counts_ms, float* maps_ms, float* fill_ms);

/* ---- smoothing region masks and label maps: box count, majority, binomial, mode (csrc/svr_smooth.hip) ----
 * The ragged one-voxel boundary of a thresholded or grown mask is smoothed without shifting it: OPEN and CLOSE of svr_region_morph only
 * remove or only add; the filters here treat a region and its complement alike.  Masks and label maps are device pointers in the
 * layouts of the region section; a row's padding bits are ignored on input, whatever they hold, and are 0 on output.  Integers only:
 * every result is defined bit for bit.  The calls run on the library's stream and touch no scene, option or accumulator.
 * RADII: radii_xyz is a HOST array of three uint32 (x, y, z), each 0 .. SVR_REGION_SMOOTH_MAX_RADIUS.  The WINDOW of voxel (x, y, z) is
 *   every (x + dx, y + dy, z + dz) with |dx| <= rx, |dy| <= ry, |dz| <= rz; an index outside the volume is CLAMPED per axis (numpy's pad
 *   mode `edge`, scipy's mode='nearest', the border rule of svr_volume_rank), so a window always holds exactly N = (2rx+1)(2ry+1)(2rz+1)
 *   values (svr_region_box_size; 0 for a NULL pointer or a radius above the cap).  Radius 0 makes the window one voxel thick on that
 *   axis; (0, 0, 0) copies (and clears the padding).
 * COUNT (svr_region_box_count): out[z][y][x] = the set voxels in the window, a u16 volume [nz][ny][nx] -- ready for
 *   svr_create_volume_texture, svr_region_threshold and svr_volume_histogram: a local volume fraction (BV/TV of a bone mask).  It equals
 *   scipy.ndimage.correlate(mask.astype(int32), ones((2rz+1, 2ry+1, 2rx+1)), mode='nearest').  With rx = ry = rz = r, count >= 1 is
 *   svr_region_morph(DILATE, 26, r) and count == N is svr_region_morph(ERODE, 26, r): a clamped index always lies inside the window, so
 *   the replicated border agrees with "nothing enters from outside" and with its dual.  One launch, no workspace, asynchronous.
 *   svr_region_box_density (an addition for display) is the same call with out = floor(65535 count / N): the local volume fraction
 *   on the full range of a u16 volume, whatever the radii.
 * MAJORITY (svr_region_smooth, SVR_SMOOTH_MAJORITY): out is set iff 2 count > N.  N is odd, so there is no tie: the median of the binary
 *   window, scipy.ndimage.median_filter(mask.astype(uint8), size=(2rz+1, 2ry+1, 2rx+1), mode='nearest').  It is self-dual (smoothing
 *   the complement gives the complement); the full volume, the empty volume and every axis-aligned half-space are fixed points.
 * BINOMIAL (svr_region_smooth, SVR_SMOOTH_BINOMIAL): out = { v : S(v) >= 32768 }, S = svr_volume_smooth(E, radii), E the u16 volume
 *   with 65535 on the set voxels and 0 elsewhere: the binomial passes of that call with their single rounding per axis.  Radii for a
 *   sigma come from svr_volume_smooth_radii.  NOT exactly self-dual: halves round up and 32768 is above the middle of 0 .. 65535.
 *   The call runs svr_volume_smooth itself, once per iteration: svr_volume_filter_last_ms afterwards reports the last of those runs.
 * MODE (svr_region_label_smooth): labels is a uint32 map [nz][ny][nx] with values 0 .. count, count <= SVR_LABEL_SMOOTH_MAX_COUNT; a
 *   value above count is read as 0, as svr_region_select drops it.  Label 0, the background, takes part like any other.  With c_l(v)
 *   the window voxels of label l, out(v) is the centre's own label if it attains max_l c_l(v), else the SMALLEST label that attains it.
 *   With count == 1 this is MAJORITY of the mask labels == 1.  Parts stay disjoint and leave no gaps: that is joint smoothing.
 * ITERATIONS: 1 .. SVR_REGION_SMOOTH_MAX_ITERATIONS; the op is applied that many times to its own output.
 * changed_or_null: when not NULL it receives the voxels at which the final output differs from the input (for labels: from the input
 *   as it is read, a value above count being 0).
 * svr_region_smooth_radii (plain host code): with q = size / spacing[a], radii[a] = max(0, llround((q - 1) / 2)), the odd window
 *   nearest to the size (q = 1, 3, 4, 5 give 0, 1, 2, 2); size_out[a] (may be NULL) = (2 radii[a] + 1) spacing[a].  Refused (-3) with
 *   nothing written: a spacing that is not positive and finite, a size that is negative or not finite, a radius above the cap.
 * WORKSPACE AND SYNCHRONISATION: svr_region_box_count and a MAJORITY of one iteration without `changed` are one launch: nothing is
 *   allocated and the call is asynchronous.  MAJORITY with more iterations holds one temporary mask; BINOMIAL holds two u16 volumes (E
 *   and S) and, with more than one radius above 0, the temporary of svr_volume_smooth; MODE holds bits(count) <= 8 bit planes of the
 *   labels in mask layout and, with more than one iteration, one temporary label map; `changed` adds 8 bytes.  A call that allocated
 *   or that reports `changed` synchronises the stream before it returns.
 * REFUSED, before the device is touched and with nothing written: a null pointer other than changed_or_null (-4); a dimension <= 0 or
 *   more than 2^31 voxels (-6); (-3) an unknown op, a radius above 8, iterations of 0 or above 16, count of 0 or above 255, an out that
 *   overlaps an input. */
#define SVR_SMOOTH_MAJORITY 1
#define SVR_SMOOTH_BINOMIAL 2
#define SVR_REGION_SMOOTH_MAX_RADIUS     8     /* = SVR_SMOOTH_MAX_RADIUS; N <= 17^3 = 4913 fits 13 bits and a u16 */
#define SVR_REGION_SMOOTH_MAX_ITERATIONS 16
#define SVR_LABEL_SMOOTH_MAX_COUNT       255
uint32_t svr_region_box_size(const uint32_t radii_xyz[3]);             /* N; 0 for a radius above the cap.  Plain host code */
int svr_region_smooth_radii(const double spacing[3], double size, uint32_t radii[3], double size_out[3]);   /* plain host code */
int svr_region_box_count(const uint32_t* mask_device, const int32_t dims[3], const uint32_t* radii_xyz, uint16_t* out_u16_device);
int svr_region_box_density(const uint32_t* mask_device, const int32_t dims[3], const uint32_t* radii_xyz, uint16_t* out_u16_device);
int svr_region_smooth(const uint32_t* in_mask_device, const int32_t dims[3], int op, const uint32_t* radii_xyz, uint32_t iterations,
                      uint32_t* out_mask_device, uint64_t* changed_or_null);
int svr_region_label_smooth(const uint32_t* labels_device, const int32_t dims[3], uint32_t count, const uint32_t* radii_xyz,
                            uint32_t iterations, uint32_t* out_labels_device, uint64_t* changed_or_null);
/* HIP-event time of the device work of the last of the four device calls above, without their allocations (waits for it) */
int svr_region_smooth_last_ms(float* ms);

int svr_get_counters(svr_counters* out);              /* synchronises the launch stream */
int svr_reset_counters(void);

/* accumulated HIP-event time of the path-tracing kernel since the last reset (SVR_OPT_TIMING) */
int svr_get_kernel_time(double* total_ms, uint64_t* launches);
int svr_reset_kernel_time(void);

/* "name major.minor gcnArch CUs" of the active device, for logs */
const char* svr_device_info(void);
int svr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SVR_ABI_H */
