// svr_scissor.hip -- scissors: a polygon drawn on a view, filled on the pixel grid, and the voxels seen inside the fill selected,
// removed from, kept in or added to a region mask (svr_stencil_polygon, svr_stencil_rect, svr_scissor_project_camera / _slice,
// svr_region_scissor_camera / _slice; the contract is in include/svr_abi.h, the design in DESIGN.md 8u).  The host scaffolding is
// svr_volume_host.hpp's, the mask layout svr_mask.hpp's: a stencil is the mask of a w x h x 1 volume.
//
// STENCIL (k_stencil): one lane per pixel, 32 lanes per stencil word (lane_at / lane_grid), the word formed by half_ballot and written
//   by one lane.  The edges (ax, ay, bx, by as one int4) are staged in LDS STENCIL_EDGE_CHUNK at a time; every lane of the block reads
//   the same edge at the same time, an LDS broadcast.  The fill rule is evaluated in int64, exactly.  A lane whose pixel centre lies
//   outside the bounding box of the vertices skips the edge loop (no edge can count for it, and this is what keeps the products below
//   2^49 on images wider than the coordinate limit); a block none of whose lanes is inside writes zeros without staging anything.
//   The call is asynchronous: the edges go through a pinned staging buffer and a device buffer that live as long as the library, and
//   the next call waits for the event behind the previous call's kernel before it overwrites the staging buffer.
// PROJECTION (project_camera, project_slice): one host / device function per view kind; the kernel and the host helpers compile the same
//   text, under the same flags (no contraction, correctly rounded division), so their results agree to the bit.  What depends on the view
//   alone (aspectRatio * tanFovxOverTwo, dot(u, u), 0.5f * (float)w, the FRAME normal) is computed once on the host, by the operations
//   the header names.
// PRISM (k_scissor<OP, View>): one lane per voxel, 32 lanes per mask word.  The kernel is DRIVEN BY THE MASK WORDS: the 32 lanes of a word
//   load it (one address: a broadcast); for the two ERASE ops a zero word is written as zero and for FILL a full word is copied, with
//   no projection; the padding lanes project nothing.  Otherwise every lane maps its voxel centre to the world, projects it, loads the
//   stencil word of its pixel (a plain global load: the stencil is 2D and small, it stays in cache) and tests the depth; the word of
//   the prism is a half_ballot, combined with the input word and written by one lane.  out may be in: a word is read and written by
//   the same half wave, the read first.  The projection is evaluated directly for every voxel -- the result is defined bit for bit,
//   and stepping along a row would not reproduce it.  No block waits for another.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"

#include "svr_mask.hpp"             // the mask layout
#include "svr_volume_host.hpp"      // the argument checks, CallTimer, SVR_HIP_TRY

using svr::failf;

namespace {

constexpr int STENCIL_EDGE_CHUNK = 1024;                 // edges staged in LDS at a time: 16 KB

// ---------------- the projection: one function per view kind, for the kernel and for the host helpers ----------------
struct CameraView {
    float pos[3], u[3], v[3], w[3];
    float tx, ty;                    // fl(aspectRatio * tanFovxOverTwo), tanFovxOverTwo
    float wm1, hm1, fw, fh;          // (float)imageW - 1, (float)imageH - 1, (float)imageW, (float)imageH
    uint32_t W, H;
};
struct SliceView {
    float center[3], u[3], v[3], n[3];
    float uu, vv;                    // dot(u, u), dot(v, v)
    float half_w, half_h, fw, fh;    // fl(0.5f * (float)w), fl(0.5f * (float)h), (float)w, (float)h
    uint32_t W, H;
};

__host__ __device__ inline float dot3(float px, float py, float pz, const float q[3]) { return (px * q[0] + py * q[1]) + pz * q[2]; }

// PIXEL of the header: (floor(s), floor(r)) if 0 <= s < (float)W and 0 <= r < (float)H.  (A float below (float)W is below W itself,
// also where W is no float; the integer test says so again, for the stencil load's sake.)
__host__ __device__ inline bool pixel_of(float s, float r, float fw, float fh, uint32_t W, uint32_t H, int32_t& x, int32_t& y)
{
    if (!(s >= 0.f && s < fw && r >= 0.f && r < fh)) return false;
    const uint32_t px = (uint32_t)floorf(s), py = (uint32_t)floorf(r);
    if (px >= W || py >= H) return false;
    x = (int32_t)px; y = (int32_t)py;
    return true;
}

__host__ __device__ inline bool project_camera(const CameraView& c, float px, float py, float pz, int32_t& x, int32_t& y, float& depth)
{
    const float dx = px - c.pos[0], dy = py - c.pos[1], dz = pz - c.pos[2];
    const float a = dot3(dx, dy, dz, c.u), b = dot3(dx, dy, dz, c.v), cc = -dot3(dx, dy, dz, c.w);
    depth = cc;
    if (!(cc > 0.f)) return false;
    const float s = ((a / (cc * c.tx) + 1.f) * 0.5f) * c.wm1;
    const float r = ((b / (cc * c.ty) + 1.f) * 0.5f) * c.hm1;
    return pixel_of(s, r, c.fw, c.fh, c.W, c.H, x, y);
}

__host__ __device__ inline bool project_slice(const SliceView& c, float px, float py, float pz, int32_t& x, int32_t& y, float& depth)
{
    const float dx = px - c.center[0], dy = py - c.center[1], dz = pz - c.center[2];
    const float a = dot3(dx, dy, dz, c.u) / c.uu, b = dot3(dx, dy, dz, c.v) / c.vv;
    const float s = a + c.half_w, r = b + c.half_h;
    depth = dot3(dx, dy, dz, c.n);
    return pixel_of(s, r, c.fw, c.fh, c.W, c.H, x, y);
}

__host__ __device__ inline bool project(const CameraView& c, float px, float py, float pz, int32_t& x, int32_t& y, float& depth) { return project_camera(c, px, py, pz, x, y, depth); }
__host__ __device__ inline bool project(const SliceView& c, float px, float py, float pz, int32_t& x, int32_t& y, float& depth) { return project_slice(c, px, py, pz, x, y, depth); }

// VOXEL CENTRE of the header, one axis
__host__ __device__ inline float centre_of(int i, int n, float vmin, float extent) { return vmin + extent * (((float)i + 0.5f) / (float)n); }

// ---------------- the stencil ----------------
struct StencilBox { int32_t x0, y0, x1, y1; };           // the bounding box of the vertices, Q8

__global__ __launch_bounds__(MASK_THREADS) void k_stencil(const int4* __restrict__ edges, uint32_t nedges, StencilBox box, RegionDims d, size_t words,
                                                          uint32_t* __restrict__ out)
{
    __shared__ int4 se[STENCIL_EDGE_CHUNK];
    const LaneAt a = lane_at(d, words);
    const long long cx = 256ll * a.x + 128ll, cy = 256ll * a.y + 128ll;
    const bool live = a.inside && cx >= box.x0 && cx <= box.x1 && cy >= box.y0 && cy <= box.y1;
    uint32_t parity = 0u;
    if (__syncthreads_or(live ? 1 : 0)) {                                         // (the same for every thread of the block)
        for (uint32_t base = 0u; base < nedges; base += (uint32_t)STENCIL_EDGE_CHUNK) {
            const uint32_t n = nedges - base < (uint32_t)STENCIL_EDGE_CHUNK ? nedges - base : (uint32_t)STENCIL_EDGE_CHUNK;
            if (base) __syncthreads();                                           // the chunk before is read
            for (uint32_t k = threadIdx.x; k < n; k += MASK_THREADS) se[k] = edges[base + k];
            __syncthreads();
            if (live)
                for (uint32_t k = 0u; k < n; ++k) {
                    const int4 e = se[k];                                        // a = (x, y), b = (z, w)
                    if ((e.y > cy) != (e.w > cy)) {
                        const long long cross = (long long)(e.z - e.x) * (cy - e.y) - (long long)(e.w - e.y) * (cx - e.x);
                        parity ^= (e.w > e.y ? cross > 0 : cross < 0) ? 1u : 0u;
                    }
                }
        }
    }
    const uint32_t word = half_ballot(parity != 0u);
    if (a.word_ok && a.bit == 0) out[a.i] = word;
}

// the staging of the edges: pinned host memory and device memory for SVR_STENCIL_MAX_VERTICES edges, made on first use and kept; `done`
// is recorded behind the kernel that reads the device copy
struct EdgeStage {
    int4* host = nullptr;
    int4* dev = nullptr;
    hipEvent_t done = nullptr;
    bool pending = false;
};
EdgeStage g_stage;

hipError_t stage_ready()
{
    if (g_stage.done) return hipSuccess;
    const size_t bytes = (size_t)SVR_STENCIL_MAX_VERTICES * sizeof(int4);
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&g_stage.host), bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&g_stage.dev), bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g_stage.done, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (g_stage.host) hipHostFree(g_stage.host);
        if (g_stage.dev) hipFree(g_stage.dev);
        g_stage = EdgeStage();
    }
    return e;
}

// ---------------- the prism ----------------
struct VoxelMap { float vmin[3], extent[3]; };            // bbox.vmin and fl(bbox.vmax - bbox.vmin)

template <int OP, class View>
__global__ __launch_bounds__(MASK_THREADS) void k_scissor(const uint32_t* in, const uint32_t* __restrict__ stencil, View view, VoxelMap vm, float depth_lo,
                                                          float depth_hi, RegionDims d, size_t words, uint32_t* out)
{
    const LaneAt a = lane_at(d, words);
    const uint32_t valid = valid_bits(a.gw, d);
    uint32_t m = 0u;
    if (OP != SVR_SCISSOR_SELECT && a.word_ok) m = in[a.i] & valid;
    bool need = a.inside;                                                        // the padding lanes project nothing
    if (OP == SVR_SCISSOR_ERASE_INSIDE || OP == SVR_SCISSOR_ERASE_OUTSIDE) need = need && m != 0u;
    if (OP == SVR_SCISSOR_FILL_INSIDE) need = need && m != valid;
    bool hit = false;
    if (need) {
        const float px = centre_of(a.x, d.nx, vm.vmin[0], vm.extent[0]), py = centre_of(a.y, d.ny, vm.vmin[1], vm.extent[1]),
                    pz = centre_of(a.z, d.nz, vm.vmin[2], vm.extent[2]);
        int32_t x = 0, y = 0;
        float depth;
        if (project(view, px, py, pz, x, y, depth) && depth_lo <= depth && depth <= depth_hi) {
            const uint32_t sw = stencil[(size_t)y * ((view.W + 31u) >> 5) + ((uint32_t)x >> 5)];
            hit = (sw >> ((uint32_t)x & 31u)) & 1u;
        }
    }
    const uint32_t prism = half_ballot(hit);                                     // (only bits of voxels: hit needs a.inside)
    if (a.word_ok && a.bit == 0) {
        uint32_t r;
        if (OP == SVR_SCISSOR_SELECT) r = prism;
        else if (OP == SVR_SCISSOR_ERASE_INSIDE) r = m & ~prism;
        else if (OP == SVR_SCISSOR_ERASE_OUTSIDE) r = m & prism;
        else r = m | prism;
        out[a.i] = r;
    }
}

template <class View>
hipError_t launch_scissor(hipStream_t st, int op, const uint32_t* in, const uint32_t* stencil, const View& view, const VoxelMap& vm, float lo, float hi,
                          const RegionDims& d, uint32_t* out)
{
    const size_t words = mask_words(d);
    const dim3 g = lane_grid(words), b(MASK_THREADS);
    switch (op) {
    case SVR_SCISSOR_SELECT: hipLaunchKernelGGL((k_scissor<SVR_SCISSOR_SELECT, View>), g, b, 0, st, in, stencil, view, vm, lo, hi, d, words, out); break;
    case SVR_SCISSOR_ERASE_INSIDE: hipLaunchKernelGGL((k_scissor<SVR_SCISSOR_ERASE_INSIDE, View>), g, b, 0, st, in, stencil, view, vm, lo, hi, d, words, out); break;
    case SVR_SCISSOR_ERASE_OUTSIDE: hipLaunchKernelGGL((k_scissor<SVR_SCISSOR_ERASE_OUTSIDE, View>), g, b, 0, st, in, stencil, view, vm, lo, hi, d, words, out); break;
    default: hipLaunchKernelGGL((k_scissor<SVR_SCISSOR_FILL_INSIDE, View>), g, b, 0, st, in, stencil, view, vm, lo, hi, d, words, out); break;
    }
    return hipGetLastError();
}

// ---------------- the checks ----------------
bool finite3(const svr_vec3& a) { return std::isfinite(a.x) && std::isfinite(a.y) && std::isfinite(a.z); }
void put3(float o[3], const svr_vec3& a) { o[0] = a.x; o[1] = a.y; o[2] = a.z; }

int check_image(const char* who, uint32_t w, uint32_t h)
{
    if (w == 0u || h == 0u) return failf(-3, "%s: image size is zero", who);
    if ((unsigned long long)w * h > (1ull << 31)) return failf(-3, "%s: an image of %u x %u has more than 2^31 pixels", who, w, h);
    return 0;
}

int check_camera(const char* who, const svr_camera* c, CameraView& cv)
{
    if (int e = check_image(who, c->imageW, c->imageH)) return e;
    if (!finite3(c->pos) || !finite3(c->u) || !finite3(c->v) || !finite3(c->w)) return failf(-3, "%s: the camera's pos, u, v and w must be finite", who);
    if (!(c->tanFovxOverTwo > 0.f) || !std::isfinite(c->tanFovxOverTwo) || !(c->aspectRatio > 0.f) || !std::isfinite(c->aspectRatio))
        return failf(-3, "%s: tanFovxOverTwo and aspectRatio must be finite and > 0 (got %g, %g)", who, (double)c->tanFovxOverTwo, (double)c->aspectRatio);
    put3(cv.pos, c->pos); put3(cv.u, c->u); put3(cv.v, c->v); put3(cv.w, c->w);
    cv.tx = c->aspectRatio * c->tanFovxOverTwo; cv.ty = c->tanFovxOverTwo;
    cv.fw = (float)c->imageW; cv.fh = (float)c->imageH;
    cv.wm1 = cv.fw - 1.f; cv.hm1 = cv.fh - 1.f;
    cv.W = c->imageW; cv.H = c->imageH;
    return 0;
}

// what svr_render_slice refuses about the image size, center, u and v, and its FRAME
int check_slice_view(const char* who, const svr_slice_params* p, uint32_t w, uint32_t h, SliceView& sv)
{
    if (int e = check_image(who, w, h)) return e;
    if (!finite3(p->center) || !finite3(p->u) || !finite3(p->v)) return failf(-3, "%s: center, u and v must be finite", who);
    const float crx = p->u.y * p->v.z - p->u.z * p->v.y, cry = p->u.z * p->v.x - p->u.x * p->v.z, crz = p->u.x * p->v.y - p->u.y * p->v.x;
    const float len2 = (crx * crx + cry * cry) + crz * crz;
    const float inv = 1.f / std::sqrt(len2);
    if (!(len2 > 0.f) || !std::isfinite(inv) || !std::isfinite(crx * inv) || !std::isfinite(cry * inv) || !std::isfinite(crz * inv))
        return failf(-3, "%s: cross(u, v) has no length (u and v must span a plane)", who);
    put3(sv.center, p->center); put3(sv.u, p->u); put3(sv.v, p->v);
    sv.n[0] = crx * inv; sv.n[1] = cry * inv; sv.n[2] = crz * inv;
    sv.uu = dot3(p->u.x, p->u.y, p->u.z, sv.u); sv.vv = dot3(p->v.x, p->v.y, p->v.z, sv.v);
    sv.fw = (float)w; sv.fh = (float)h;
    sv.half_w = 0.5f * sv.fw; sv.half_h = 0.5f * sv.fh;
    sv.W = w; sv.H = h;
    return 0;
}

int check_prism(const char* who, const uint32_t* in, const svr_volume* volume, const void* view, const uint32_t* stencil, const svr_scissor_params* p,
                const uint32_t* out, int nx, int ny, int nz, VoxelMap& vm)
{
    if (!volume || !view || !stencil || !p || !out) return failf(-4, "%s: null argument", who);
    if (!in && p->op != SVR_SCISSOR_SELECT) return failf(-4, "%s: null argument (in may be NULL with SVR_SCISSOR_SELECT alone)", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (p->op < SVR_SCISSOR_SELECT || p->op > SVR_SCISSOR_FILL_INSIDE) return failf(-3, "%s: unknown op %d", who, (int)p->op);
    if (p->flags != 0u) return failf(-3, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
    if (std::isnan(p->depth_lo) || std::isnan(p->depth_hi) || p->depth_lo > p->depth_hi)
        return failf(-3, "%s: the depth bounds %g .. %g are NaN or inverted", who, (double)p->depth_lo, (double)p->depth_hi);
    if (!finite3(volume->bbox.vmin) || !finite3(volume->bbox.vmax)) return failf(-3, "%s: the volume's bbox is not finite", who);
    put3(vm.vmin, volume->bbox.vmin);
    vm.extent[0] = volume->bbox.vmax.x - volume->bbox.vmin.x; vm.extent[1] = volume->bbox.vmax.y - volume->bbox.vmin.y;
    vm.extent[2] = volume->bbox.vmax.z - volume->bbox.vmin.z;
    return 0;
}

CallEvents g_events;

template <class View>
int run_scissor(const char* who, const uint32_t* in, int nx, int ny, int nz, const View& view, const VoxelMap& vm, const uint32_t* stencil,
                const svr_scissor_params* p, uint32_t* out)
{
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(launch_scissor(st, p->op, in, stencil, view, vm, p->depth_lo, p->depth_hi, make_dims(nx, ny, nz), out));
    return 0;
}

int write_pixel(bool seen, int32_t x, int32_t y, int32_t xy[2])
{
    xy[0] = seen ? x : -1; xy[1] = seen ? y : -1;
    return seen ? 0 : 1;
}

} // namespace

extern "C" {

int svr_scissor_params_default(svr_scissor_params* p)
{
    if (!p) return failf(-4, "svr_scissor_params_default: null argument");
    memset(p, 0, sizeof *p);
    p->op = SVR_SCISSOR_SELECT;
    p->depth_lo = -std::numeric_limits<float>::infinity(); p->depth_hi = std::numeric_limits<float>::infinity();
    return 0;
}

int svr_stencil_rect(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t vertices_xy_q8[8])
{
    const char* who = "svr_stencil_rect";
    if (!vertices_xy_q8) return failf(-4, "%s: null argument", who);
    if (x1 < x0 || y1 < y0) return failf(-3, "%s: the rectangle %d .. %d, %d .. %d is inverted", who, (int)x0, (int)x1, (int)y0, (int)y1);
    const long long c[4] = {256ll * x0, 256ll * y0, 256ll * ((long long)x1 + 1), 256ll * ((long long)y1 + 1)};
    for (long long v : c)
        if (v < -(long long)SVR_STENCIL_MAX_COORD || v > (long long)SVR_STENCIL_MAX_COORD)
            return failf(-3, "%s: a corner of the rectangle lies beyond the coordinate limit of 2^23", who);
    const int32_t q[8] = {(int32_t)c[0], (int32_t)c[1], (int32_t)c[2], (int32_t)c[1], (int32_t)c[2], (int32_t)c[3], (int32_t)c[0], (int32_t)c[3]};
    memcpy(vertices_xy_q8, q, sizeof q);
    return 0;
}

int svr_stencil_polygon(const int32_t* vertices_xy_q8, const uint32_t* contour_counts, uint32_t ncontours, uint32_t w, uint32_t h, uint32_t* stencil_device)
{
    const char* who = "svr_stencil_polygon";
    if (!vertices_xy_q8 || !contour_counts || !stencil_device) return failf(-4, "%s: null argument", who);
    if (int e = check_image(who, w, h)) return e;
    if (ncontours == 0u) return failf(-3, "%s: ncontours is zero", who);
    uint64_t total = 0u;
    for (uint32_t k = 0; k < ncontours; ++k) {
        if (contour_counts[k] < 3u) return failf(-3, "%s: contour %u has %u vertices (at least 3)", who, k, contour_counts[k]);
        total += contour_counts[k];
        if (total > (uint64_t)SVR_STENCIL_MAX_VERTICES) return failf(-3, "%s: more than %d vertices", who, SVR_STENCIL_MAX_VERTICES);
    }
    StencilBox box = {INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN};
    for (uint64_t i = 0; i < total; ++i) {
        const int32_t x = vertices_xy_q8[2u * i], y = vertices_xy_q8[2u * i + 1u];
        if (x < -SVR_STENCIL_MAX_COORD || x > SVR_STENCIL_MAX_COORD || y < -SVR_STENCIL_MAX_COORD || y > SVR_STENCIL_MAX_COORD)
            return failf(-3, "%s: vertex %llu (%d, %d) lies beyond the coordinate limit of 2^23", who, (unsigned long long)i, (int)x, (int)y);
        box.x0 = x < box.x0 ? x : box.x0; box.x1 = x > box.x1 ? x : box.x1;
        box.y0 = y < box.y0 ? y : box.y0; box.y1 = y > box.y1 ? y : box.y1;
    }
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    SVR_HIP_TRY(stage_ready());
    if (g_stage.pending) SVR_HIP_TRY(hipEventSynchronize(g_stage.done));          // the call before has read the staging buffer
    g_stage.pending = false;
    uint32_t nedges = 0u;
    const int32_t* v = vertices_xy_q8;
    for (uint32_t k = 0; k < ncontours; ++k) {
        const uint32_t n = contour_counts[k];
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t j = i + 1u < n ? i + 1u : 0u;
            g_stage.host[nedges++] = make_int4(v[2u * i], v[2u * i + 1u], v[2u * j], v[2u * j + 1u]);
        }
        v += 2u * n;
    }
    const RegionDims d = make_dims((int)w, (int)h, 1);
    const size_t words = mask_words(d);
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(hipMemcpyAsync(g_stage.dev, g_stage.host, (size_t)nedges * sizeof(int4), hipMemcpyHostToDevice, st));
    g_stage.pending = true;                                                       // (from here on the stream may read the staging buffer)
    hipLaunchKernelGGL(k_stencil, lane_grid(words), dim3(MASK_THREADS), 0, st, g_stage.dev, nedges, box, d, words, stencil_device);
    SVR_HIP_TRY(hipGetLastError());
    SVR_HIP_TRY(hipEventRecord(g_stage.done, st));
    return 0;
}

int svr_scissor_project_camera(const svr_camera* camera, const svr_vec3* point, int32_t xy[2], float* depth)
{
    const char* who = "svr_scissor_project_camera";
    if (!camera || !point || !xy || !depth) return failf(-4, "%s: null argument", who);
    CameraView cv;
    if (int e = check_camera(who, camera, cv)) return e;
    int32_t x = 0, y = 0;
    const bool seen = project_camera(cv, point->x, point->y, point->z, x, y, *depth);
    return write_pixel(seen, x, y, xy);
}

int svr_scissor_project_slice(const svr_slice_params* slice, uint32_t w, uint32_t h, const svr_vec3* point, int32_t xy[2], float* depth)
{
    const char* who = "svr_scissor_project_slice";
    if (!slice || !point || !xy || !depth) return failf(-4, "%s: null argument", who);
    SliceView sv;
    if (int e = check_slice_view(who, slice, w, h, sv)) return e;
    int32_t x = 0, y = 0;
    const bool seen = project_slice(sv, point->x, point->y, point->z, x, y, *depth);
    return write_pixel(seen, x, y, xy);
}

int svr_region_scissor_camera(const uint32_t* in_mask_device_or_null, int nx, int ny, int nz, const svr_volume* volume, const svr_camera* camera,
                              const uint32_t* stencil_device, const svr_scissor_params* p, uint32_t* out_mask_device)
{
    const char* who = "svr_region_scissor_camera";
    VoxelMap vm;
    if (int e = check_prism(who, in_mask_device_or_null, volume, camera, stencil_device, p, out_mask_device, nx, ny, nz, vm)) return e;
    CameraView cv;
    if (int e = check_camera(who, camera, cv)) return e;
    return run_scissor(who, in_mask_device_or_null, nx, ny, nz, cv, vm, stencil_device, p, out_mask_device);
}

int svr_region_scissor_slice(const uint32_t* in_mask_device_or_null, int nx, int ny, int nz, const svr_volume* volume, const svr_slice_params* slice,
                             uint32_t w, uint32_t h, const uint32_t* stencil_device, const svr_scissor_params* p, uint32_t* out_mask_device)
{
    const char* who = "svr_region_scissor_slice";
    VoxelMap vm;
    if (int e = check_prism(who, in_mask_device_or_null, volume, slice, stencil_device, p, out_mask_device, nx, ny, nz, vm)) return e;
    SliceView sv;
    if (int e = check_slice_view(who, slice, w, h, sv)) return e;
    return run_scissor(who, in_mask_device_or_null, nx, ny, nz, sv, vm, stencil_device, p, out_mask_device);
}

int svr_region_scissor_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_region_scissor_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

} // extern "C"
