// svr_overlay.hip -- region masks and label maps as overlays on slices and 3D views (svr_slice_ids, svr_hit_ids, svr_overlay_ids,
// svr_overlay_slice; the contract is in include/svr_abi.h, "overlays", the design in DESIGN.md 8n).  Integers only, but for the sample
// points of a slice: those are the float32 points of svr_slice.hip, computed by the same operations in the same order (this file is
// compiled without contraction like every other).  The volume's voxels are never read: a sample costs its address arithmetic and one
// dependent 4-byte load from the mask or the label array.
//
// THE ID OF A POINT is svr_region_seed_from_world's mapping: tc = (p - vmin) * invSize in float32, i = floor(tc * n) with the product in
// double, where it is exact (24 x 31 bits), and non-negative, so the conversion to int is the floor.
//
// k_slice_ids and k_overlay_slice take k_slice's task scheme: persistent 256-thread blocks whose waves pull (slice, 8 x 8 tile) tasks of
// the owned pixels from the sharded tickets.  In k_overlay_slice a lane cannot decide EDGE alone: the wave keeps the ids of its tile and
// of the 32 ring pixels beside the tile's four sides (the corners have no 4-neighbour in the tile) in a 10 x 10 LDS patch of its own, so
// it needs no block barrier.  Lanes 0 .. 31 compute one ring pixel each after their own; a tile without a non-zero id among its owned
// pixels writes nothing and skips the ring.  The rows of a tile are consecutive image rows under a window and under a row shard alike
// (strip_rows is a multiple of 8 and tiles are aligned to 8 owned rows), which a 16 x 16 tile would not be under a shard of 8-row strips.
#include "svr_kernel_common.hpp"
#include "svr_mask.hpp"
#include "svr_volume_host.hpp"

#include <cmath>
#include <cstring>

namespace svr {

#define SVR_OV_THREADS 256
#define SVR_OV_MAX_CHUNK 16u

struct OvSource {
    const uint32_t* mask;                // exactly one of the two is set
    const uint32_t* labels;
    int nx, ny, nz, wx;                  // wx: words of a mask row (svr_mask.hpp)
    float vmin[3], invSize[3];           // the unclipped box
};

// the geometry of svr_slice.hpp's DevSlice: what a sample point and its counting need
struct OvSlice {
    float center[3], u[3], v[3], n[3];
    float box_lo[3], box_hi[3];
    float half_thickness, step, spacing;
    uint32_t K, count;
    uint32_t W, H;
    uint32_t chunk;                      // tasks per ticket, 1 .. SVR_OV_MAX_CHUNK
};

struct OvStyle {
    uint32_t fill_alpha, edge_alpha, count;
    uint32_t pal[SVR_OVERLAY_MAX_PALETTE];       // by value: a kernel argument needs no allocation and is safe on any stream
};

SVR_DEV uint32_t voxel_id(const OvSource& s, float px, float py, float pz)
{
    const float tx = (px - s.vmin[0]) * s.invSize[0], ty = (py - s.vmin[1]) * s.invSize[1], tz = (pz - s.vmin[2]) * s.invSize[2];
    if (!((tx >= 0.f) & (tx <= 1.f) & (ty >= 0.f) & (ty <= 1.f) & (tz >= 0.f) & (tz <= 1.f))) return 0u;       // (NaN: outside)
    const int ix = min((int)((double)tx * (double)s.nx), s.nx - 1);
    const int iy = min((int)((double)ty * (double)s.ny), s.ny - 1);
    const int iz = min((int)((double)tz * (double)s.nz), s.nz - 1);
    const uint64_t row = (uint64_t)iz * (uint32_t)s.ny + (uint32_t)iy;
    if (s.mask) return (s.mask[row * (uint32_t)s.wx + (uint32_t)(ix >> 5)] >> (ix & 31)) & 1u;
    return s.labels[row * (uint32_t)s.nx + (uint32_t)ix];
}

// the smallest non-zero id among the counting samples of pixel (x, y) of slice `slice`; 0 if there is none.  ids are compared as id - 1
// (0 wraps to the largest value), so the running minimum needs no test for 0 and a found 1 ends the search.
SVR_DEV uint32_t slice_pixel_id(const OvSlice& sl, const OvSource& src, uint32_t x, uint32_t y, uint32_t slice)
{
    const v3 U = V3(sl.u[0], sl.u[1], sl.u[2]), V = V3(sl.v[0], sl.v[1], sl.v[2]), N = V3(sl.n[0], sl.n[1], sl.n[2]);
    v3 ck = V3(sl.center[0], sl.center[1], sl.center[2]);
    if (slice != 0u) ck = ck + N * (sl.spacing * (float)slice);
    const float a = ((float)x + 0.5f) - 0.5f * (float)sl.W;
    const float b = ((float)y + 0.5f) - 0.5f * (float)sl.H;
    const v3 c = (ck + U * a) + V * b;
    uint32_t best = 0xffffffffu;
    for (uint32_t j = 0; j < sl.K && best != 0u; ++j) {
        const float d = (float)j * sl.step - sl.half_thickness;
        const v3 p = c + N * d;
        const bool inside = (p.x >= sl.box_lo[0]) & (p.x <= sl.box_hi[0]) & (p.y >= sl.box_lo[1]) & (p.y <= sl.box_hi[1]) &
                            (p.z >= sl.box_lo[2]) & (p.z <= sl.box_hi[2]);
        if (!inside) continue;
        best = min(best, voxel_id(src, p.x, p.y, p.z) - 1u);
    }
    return best + 1u;
}

// BLEND of the header: pixel value `in` of a pixel with id k != 0; returns false if the pixel is not to be written
SVR_DEV bool blend(const OvStyle& st, uint32_t k, bool edge, uint32_t in, uint32_t& out)
{
    const uint32_t e = st.pal[(k - 1u) % st.count];
    const uint32_t A = edge ? st.edge_alpha : st.fill_alpha;
    const uint32_t a = (A * (e >> 24) + 127u) / 255u;
    if (a == 0u) return false;
    const uint32_t na = 255u - a;
    const uint32_t r = ((in & 255u) * na + (e & 255u) * a + 127u) / 255u;
    const uint32_t g = (((in >> 8) & 255u) * na + ((e >> 8) & 255u) * a + 127u) / 255u;
    const uint32_t b = (((in >> 16) & 255u) * na + ((e >> 16) & 255u) * a + 127u) / 255u;
    out = r | (g << 8) | (b << 16) | (in & 0xff000000u);
    return true;
}

// The task loop of k_slice, with one change: a ticket grants sl.chunk consecutive tasks.  A task here is address arithmetic and one gather
// per sample, and with one atomic per tile the eight ticket words bound a stack (256 slices of 1024 x 1024 took the time
// of 4.2 M atomics whatever the kernel did per tile).  The host sizes the chunk so that every wave still finds several tickets.
// The body runs per (slice, tile) task with slice, tx, ty and lane in scope, wave-uniform.
#define SVR_OV_TASK_LOOP(...)                                                                                       \
    const uint32_t lane = threadIdx.x & 63u;                                                                        \
    const uint32_t wv = w.x1 - w.x0;                                                                                \
    const uint32_t tiles_x = (wv + 7u) >> 3, tiles_y = (w.n_rows + 7u) >> 3;                                        \
    const uint32_t tiles = tiles_x * tiles_y;                                                                       \
    const uint32_t n_tasks = tiles * sl.count;                      /* < 2^32, checked on the host */              \
    const uint32_t per_shard = (n_tasks + TICKET_SHARDS - 1u) / TICKET_SHARDS;                                      \
    const uint32_t shard0 = blockIdx.x % TICKET_SHARDS;                                                             \
    for (uint32_t si = 0; si < TICKET_SHARDS; ++si) {                                                               \
        const uint32_t shard = (shard0 + si) % TICKET_SHARDS;                                                       \
        const uint32_t t_begin = shard * per_shard;                                                                 \
        const uint32_t t_count = t_begin >= n_tasks ? 0u : min(per_shard, n_tasks - t_begin);                       \
        uint32_t* ticket = w.ticket + shard * TICKET_STRIDE;                                                        \
        for (;;) {                                                                                                  \
            uint32_t tk0 = 0;                                                                                       \
            if (lane == 0) tk0 = atomicAdd(ticket, sl.chunk);                                                       \
            tk0 = __builtin_amdgcn_readfirstlane(tk0);                                                              \
            if (tk0 >= t_count) break;                                                                              \
            const uint32_t tk1 = min(tk0 + sl.chunk, t_count);                                                      \
            for (uint32_t tk = tk0; tk < tk1; ++tk) {                                                               \
                const uint32_t task = t_begin + tk;                                                                 \
                const uint32_t slice = task / tiles, tile = task - slice * tiles;                                   \
                const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;                                       \
                __VA_ARGS__                                                                                         \
            }                                                                                                       \
        }                                                                                                           \
    }

__global__ __launch_bounds__(SVR_OV_THREADS) void k_slice_ids(const DevWork w, const OvSlice sl, const OvSource src, uint32_t* __restrict__ ids)
{
    SVR_OV_TASK_LOOP({
        const uint32_t px = (tx << 3) + (lane & 7u), r = (ty << 3) + (lane >> 3);
        if (px < wv && r < w.n_rows) {
            const uint32_t x = w.x0 + px, y = owned_row_to_y(w, r);
            ids[((size_t)slice * sl.H + y) * sl.W + x] = slice_pixel_id(sl, src, x, y, slice);
        }
    })
}

__global__ __launch_bounds__(SVR_OV_THREADS) void k_overlay_slice(const DevWork w, const OvSlice sl, const OvSource src, const OvStyle st,
                                                                  uint32_t* __restrict__ imgs)
{
    __shared__ uint32_t patches[SVR_OV_THREADS / 64][100];
    uint32_t* patch = patches[threadIdx.x >> 6];                    // [10][10]: cell (1 + ly, 1 + lx) is pixel (lx, ly) of the tile
    SVR_OV_TASK_LOOP({
        const uint32_t lx = lane & 7u, ly = lane >> 3;
        const uint32_t x_left = w.x0 + (tx << 3), y_top = owned_row_to_y(w, ty << 3);
        const uint32_t x = x_left + lx, y = y_top + ly;
        const bool owned = (tx << 3) + lx < wv && (ty << 3) + ly < w.n_rows;
        // (a pixel of the tile that is not owned but lies in the image is a neighbour of owned ones: it needs its true id)
        const uint32_t id = (x < sl.W && y < sl.H) ? slice_pixel_id(sl, src, x, y, slice) : 0u;
        if (__ballot(owned && id != 0u) == 0ull) continue;
        // the writes of this task follow the reads of the previous one
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        patch[(ly + 1u) * 10u + lx + 1u] = id;
        if (lane < 32u) {
            // sides: above, below, left, right.  A coordinate of -1 wraps and lies outside the image like one past the end
            const uint32_t side = lane >> 3, i = lane & 7u;
            const uint32_t rx = side == 2u ? x_left - 1u : side == 3u ? x_left + 8u : x_left + i;
            const uint32_t ry = side == 0u ? y_top - 1u : side == 1u ? y_top + 8u : y_top + i;
            const uint32_t cell = side == 0u ? i + 1u : side == 1u ? 90u + i + 1u : side == 2u ? (i + 1u) * 10u : (i + 1u) * 10u + 9u;
            patch[cell] = (rx < sl.W && ry < sl.H) ? slice_pixel_id(sl, src, rx, ry, slice) : 0u;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (owned && id != 0u) {
            const uint32_t c = (ly + 1u) * 10u + lx + 1u;
            const bool edge = (x > 0u && patch[c - 1u] != id) || (x + 1u < sl.W && patch[c + 1u] != id) ||
                              (y > 0u && patch[c - 10u] != id) || (y + 1u < sl.H && patch[c + 10u] != id);
            uint32_t* px = imgs + ((size_t)slice * sl.H + y) * sl.W + x;
            uint32_t out;
            if (blend(st, id, edge, *px, out)) *px = out;
        }
    })
}

// one thread per record of a full hit map: svr_hit is 10 words, status in word 0, position in words 4 .. 6
__global__ __launch_bounds__(SVR_OV_THREADS) void k_hit_ids(const uint32_t* __restrict__ hits, size_t n, const OvSource src, uint32_t* __restrict__ ids)
{
    for (size_t i = (size_t)blockIdx.x * SVR_OV_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * SVR_OV_THREADS) {
        const uint32_t* rec = hits + i * 10u;
        uint32_t id = 0u;
        if ((int32_t)rec[0] == SVR_HIT_STATUS_FOUND) id = voxel_id(src, u2f(rec[4]), u2f(rec[5]), u2f(rec[6]));
        ids[i] = id;
    }
}

// one thread per pixel of `count` images: EDGE from the id images, BLEND in place
__global__ __launch_bounds__(SVR_OV_THREADS) void k_overlay_ids(uint32_t* __restrict__ imgs, const uint32_t* __restrict__ ids, uint32_t W, uint32_t H,
                                                                size_t n, const OvStyle st)
{
    for (size_t i = (size_t)blockIdx.x * SVR_OV_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * SVR_OV_THREADS) {
        const uint32_t id = ids[i];
        if (id == 0u) continue;
        const size_t row = i / W;
        const uint32_t x = (uint32_t)(i - row * W), y = (uint32_t)(row % H);
        const bool edge = (x > 0u && ids[i - 1u] != id) || (x + 1u < W && ids[i + 1u] != id) ||
                          (y > 0u && ids[i - W] != id) || (y + 1u < H && ids[i + W] != id);
        uint32_t out;
        if (blend(st, id, edge, imgs[i], out)) imgs[i] = out;
    }
}

} // namespace svr

namespace {

using svr::failf;

const uint32_t DEFAULT_PALETTE[SVR_OVERLAY_DEFAULT_PALETTE] = {          // include/svr_abi.h, STYLE: r in the low byte, a = 255
    0xFF4B19E6u, 0xFF4BB43Cu, 0xFF19E1FFu, 0xFFC88200u, 0xFF3082F5u, 0xFFB41E91u,
    0xFFF0F046u, 0xFFE632F0u, 0xFF3CF5D2u, 0xFFD4BEFAu, 0xFF800000u, 0xFF286EAAu};

CallEvents g_events;                                                     // behind svr_overlay_last_ms

bool finite3(const svr_vec3& v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }

// SOURCE and the VOXEL OF A POINT mapping; -4 / -6 / -3 in this order
int check_source(const char* who, const svr_volume* volume, int nx, int ny, int nz, const svr_overlay_source* source, svr::OvSource& s)
{
    if (!volume || !source) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if ((source->mask_device != nullptr) == (source->labels_device != nullptr))
        return failf(-3, "%s: exactly one of source.mask_device and source.labels_device must be set", who);
    if (!finite3(volume->bbox.vmin) || !finite3(volume->bbox.vmax) || !finite3(volume->bbox.invSize)) return failf(-3, "%s: the volume's bbox is not finite", who);
    const RegionDims d = make_dims(nx, ny, nz);
    s.mask = source->mask_device; s.labels = source->labels_device;
    s.nx = nx; s.ny = ny; s.nz = nz; s.wx = d.wx;
    s.vmin[0] = volume->bbox.vmin.x; s.vmin[1] = volume->bbox.vmin.y; s.vmin[2] = volume->bbox.vmin.z;
    s.invSize[0] = volume->bbox.invSize.x; s.invSize[1] = volume->bbox.invSize.y; s.invSize[2] = volume->bbox.invSize.z;
    return 0;
}

// The geometry of a slice call: the checks svr_render_slice_stack (svr_api_views.hip) makes on center, u, v, thickness, step, count and spacing,
// in its order, and its FRAME and BOX.  mode, flags and the window are not looked at.
int check_slice(const char* who, const svr_volume& vol, uint32_t w, uint32_t h, const svr_slice_params* p, uint32_t count, float spacing, svr::OvSlice& sl)
{
    if (w == 0 || h == 0) return failf(-3, "%s: image size is zero", who);
    if (count == 0) return failf(-3, "%s: count is zero", who);
    if (!finite3(p->center) || !finite3(p->u) || !finite3(p->v) || !std::isfinite(p->thickness) || !std::isfinite(p->step) || !std::isfinite(spacing))
        return failf(-3, "%s: center, u, v, thickness, step and spacing must be finite", who);
    if (p->thickness < 0.f) return failf(-3, "%s: thickness must be >= 0 (got %g)", who, (double)p->thickness);
    memset(&sl, 0, sizeof sl);
    sl.K = 1u;
    if (p->thickness > 0.f) {
        if (!(p->step > 0.f)) return failf(-3, "%s: a slab needs step > 0 (got %g)", who, (double)p->step);
        const float q = std::floor(p->thickness / p->step);
        if (!(q < (float)SVR_SLICE_MAX_SAMPLES)) return failf(-3, "%s: thickness / step gives more than %d samples", who, SVR_SLICE_MAX_SAMPLES);
        sl.K = (uint32_t)q + 1u;
        sl.step = p->step;
        sl.half_thickness = 0.5f * p->thickness;
    }
    // n = normalize(cross(u, v)), the operations the header names (this file is compiled without contraction)
    const float crx = p->u.y * p->v.z - p->u.z * p->v.y, cry = p->u.z * p->v.x - p->u.x * p->v.z, crz = p->u.x * p->v.y - p->u.y * p->v.x;
    const float len2 = (crx * crx + cry * cry) + crz * crz;
    const float inv = 1.f / std::sqrt(len2);
    if (!(len2 > 0.f) || !std::isfinite(inv) || !std::isfinite(crx * inv) || !std::isfinite(cry * inv) || !std::isfinite(crz * inv))
        return failf(-3, "%s: cross(u, v) has no length (u and v must span a plane)", who);
    const uint64_t n_tasks = (uint64_t)((w + 7u) >> 3) * ((h + 7u) >> 3) * count;
    if (n_tasks > 0xffffffffull - svr::TICKET_SHARDS) return failf(-3, "%s: %u slices of %u x %u are more than 2^32 - 1 tile tasks", who, count, w, h);
    sl.center[0] = p->center.x; sl.center[1] = p->center.y; sl.center[2] = p->center.z;
    sl.u[0] = p->u.x; sl.u[1] = p->u.y; sl.u[2] = p->u.z;
    sl.v[0] = p->v.x; sl.v[1] = p->v.y; sl.v[2] = p->v.z;
    sl.n[0] = crx * inv; sl.n[1] = cry * inv; sl.n[2] = crz * inv;
    const float e0[3] = {vol.bbox.vmin.x * (-vol.x_clip.x), vol.bbox.vmin.y * (-vol.y_clip.x), vol.bbox.vmin.z * (-vol.z_clip.x)};
    const float e1[3] = {vol.bbox.vmax.x * vol.x_clip.y, vol.bbox.vmax.y * vol.y_clip.y, vol.bbox.vmax.z * vol.z_clip.y};
    for (int a = 0; a < 3; ++a) { sl.box_lo[a] = std::min(e0[a], e1[a]); sl.box_hi[a] = std::max(e0[a], e1[a]); }
    sl.spacing = spacing; sl.count = count;
    sl.W = w; sl.H = h;
    return 0;
}

int check_style(const char* who, const svr_overlay_style* style, svr::OvStyle& st)
{
    if (style->fill_alpha > 255u || style->edge_alpha > 255u)
        return failf(-3, "%s: fill_alpha and edge_alpha must lie in 0 .. 255 (got %u, %u)", who, style->fill_alpha, style->edge_alpha);
    if (style->flags != 0u) return failf(-3, "%s: unknown style flags 0x%x", who, (unsigned)style->flags);
    if (style->palette_count > SVR_OVERLAY_MAX_PALETTE) return failf(-3, "%s: palette_count must be <= %d (got %u)", who, SVR_OVERLAY_MAX_PALETTE, style->palette_count);
    if ((style->palette == nullptr) != (style->palette_count == 0u))
        return failf(-3, "%s: a palette needs a palette_count and a palette_count a palette (NULL with 0: the built-in table)", who);
    memset(&st, 0, sizeof st);
    st.fill_alpha = style->fill_alpha; st.edge_alpha = style->edge_alpha;
    st.count = style->palette ? style->palette_count : (uint32_t)SVR_OVERLAY_DEFAULT_PALETTE;
    memcpy(st.pal, style->palette ? style->palette : DEFAULT_PALETTE, sizeof(uint32_t) * st.count);
    return 0;
}

// the blocks of a one-thread-per-item kernel with a grid-stride loop
uint32_t item_blocks(size_t n) { return (uint32_t)std::min<size_t>((n + SVR_OV_THREADS - 1) / SVR_OV_THREADS, (size_t)1u << 20); }

// the persistent blocks of a task-loop kernel over the pixels of `work` (a wave per task, at most 8 blocks of 4 waves per CU) and the
// tasks a ticket grants: as many as leave every wave of the grid four tickets, SVR_OV_MAX_CHUNK at the most
bool slice_grid(const svr::DevWork& work, uint32_t count, dim3& grid, uint32_t& chunk)
{
    if (work.x1 == work.x0 || work.n_rows == 0u) return false;
    const uint64_t n_tasks = (uint64_t)((work.x1 - work.x0 + 7u) >> 3) * ((work.n_rows + 7u) >> 3) * count;
    const uint64_t need = (n_tasks + SVR_OV_THREADS / 64 - 1u) / (SVR_OV_THREADS / 64);
    grid = dim3(svr::persistent_blocks(need, (uint32_t)svr::device_cus() * 8u));
    const uint64_t waves = (uint64_t)grid.x * (SVR_OV_THREADS / 64);
    chunk = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(n_tasks / (4u * waves), 1u), SVR_OV_MAX_CHUNK);
    return true;
}

// svr_slice_ids (style null) and svr_overlay_slice
int slice_call(const char* who, void* out, const svr_volume* volume, int nx, int ny, int nz, uint32_t w, uint32_t h, const svr_slice_params* p,
               uint32_t count, float spacing, const svr_overlay_source* source, const svr_overlay_style* style, bool styled)
{
    if (!out || !volume || !p || !source || (styled && !style)) return failf(-4, "%s: null argument", who);
    svr::OvSource src;
    svr::OvSlice sl;
    svr::OvStyle st;
    if (int e = check_source(who, volume, nx, ny, nz, source, src)) return e;
    if (styled) if (int e = check_style(who, style, st)) return e;
    if (int e = check_slice(who, *volume, w, h, p, count, spacing, sl)) return e;
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t stream = svr::current_stream();
    svr::DevWork work;
    svr::image_work(work, w, h, false);
    dim3 grid;
    if (!slice_grid(work, count, grid, sl.chunk)) return 0;
    CallTimer timer(g_events, stream);
    SVR_HIP_TRY(hipMemsetAsync(work.ticket, 0, sizeof(uint32_t) * svr::TICKET_SHARDS * svr::TICKET_STRIDE, stream));
    if (styled) hipLaunchKernelGGL(svr::k_overlay_slice, grid, dim3(SVR_OV_THREADS), 0, stream, work, sl, src, st, (uint32_t*)out);
    else hipLaunchKernelGGL(svr::k_slice_ids, grid, dim3(SVR_OV_THREADS), 0, stream, work, sl, src, (uint32_t*)out);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace

extern "C" {

int svr_overlay_style_default(svr_overlay_style* style)
{
    if (!style) return failf(-4, "svr_overlay_style_default: null argument");
    memset(style, 0, sizeof *style);
    style->fill_alpha = 96u; style->edge_alpha = 255u;
    return 0;
}

int svr_overlay_palette_default(uint32_t* out, uint32_t n)
{
    if (!out) return failf(-4, "svr_overlay_palette_default: null argument");
    if (n > SVR_OVERLAY_DEFAULT_PALETTE) return failf(-3, "svr_overlay_palette_default: the built-in table has %d entries (asked for %u)", SVR_OVERLAY_DEFAULT_PALETTE, n);
    memcpy(out, DEFAULT_PALETTE, sizeof(uint32_t) * n);
    return 0;
}

int svr_slice_ids(uint32_t* ids_device, const svr_volume* volume, int nx, int ny, int nz, uint32_t w, uint32_t h, const svr_slice_params* p,
                  uint32_t count, float spacing, const svr_overlay_source* source)
{
    return slice_call("svr_slice_ids", ids_device, volume, nx, ny, nz, w, h, p, count, spacing, source, nullptr, false);
}

int svr_overlay_slice(void* imgs, const svr_volume* volume, int nx, int ny, int nz, uint32_t w, uint32_t h, const svr_slice_params* p,
                      uint32_t count, float spacing, const svr_overlay_source* source, const svr_overlay_style* style)
{
    return slice_call("svr_overlay_slice", imgs, volume, nx, ny, nz, w, h, p, count, spacing, source, style, true);
}

int svr_hit_ids(uint32_t* ids_device, const void* hits_device, uint32_t w, uint32_t h, const svr_volume* volume, int nx, int ny, int nz,
                const svr_overlay_source* source)
{
    const char* who = "svr_hit_ids";
    if (!ids_device || !hits_device || !volume || !source) return failf(-4, "%s: null argument", who);
    svr::OvSource src;
    if (int e = check_source(who, volume, nx, ny, nz, source, src)) return e;
    if (w == 0 || h == 0) return failf(-3, "%s: image size is zero", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t stream = svr::current_stream();
    CallTimer timer(g_events, stream);
    const size_t n = (size_t)w * h;
    hipLaunchKernelGGL(svr::k_hit_ids, dim3(item_blocks(n)), dim3(SVR_OV_THREADS), 0, stream, (const uint32_t*)hits_device, n, src, ids_device);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_overlay_ids(void* imgs, const uint32_t* ids_device, uint32_t w, uint32_t h, uint32_t count, const svr_overlay_style* style)
{
    const char* who = "svr_overlay_ids";
    if (!imgs || !ids_device || !style) return failf(-4, "%s: null argument", who);
    svr::OvStyle st;
    if (int e = check_style(who, style, st)) return e;
    if (w == 0 || h == 0) return failf(-3, "%s: image size is zero", who);
    if (count == 0) return failf(-3, "%s: count is zero", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t stream = svr::current_stream();
    CallTimer timer(g_events, stream);
    const size_t n = (size_t)w * h * count;
    hipLaunchKernelGGL(svr::k_overlay_ids, dim3(item_blocks(n)), dim3(SVR_OV_THREADS), 0, stream, (uint32_t*)imgs, ids_device, w, h, n, st);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_overlay_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_overlay_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

} // extern "C"
