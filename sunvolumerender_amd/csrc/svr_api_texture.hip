// svr_api_texture.hip -- the texture store of the C-ABI layer (svr_api.hip): volume, transfer-function and environment textures, the
// tables built with them or at their first use, and their release.
#include "svr_api_state.hpp"
#include "svr_project.hpp"   // launch_nbmax

#include <algorithm>
#include <vector>

using namespace svr_host;

namespace svr_host {

// the device memory of a texture and the texture itself (svr_destroy_texture, svr_shutdown)
void free_texture(Texture* t)
{
    if (t->data) hipFree(t->data);
    if (t->mm) hipFree(t->mm);
    if (t->mm_fine) hipFree(t->mm_fine);
    if (t->mm_wide) hipFree(t->mm_wide);
    if (t->nbmax) hipFree(t->nbmax);
    if (t->zero_prefix) hipFree(t->zero_prefix);
    if (t->env_cdf) hipFree(t->env_cdf);
    t->magic = 0;
    delete t;
}

// the neighbour-max table of a volume texture (svr_project.hip, k_nbmax), built at the first call that leaps over it
int ensure_nbmax(const char* who, Texture* tv)
{
    if (tv->nbmax) return 0;
    hipError_t e = hipMalloc((void**)&tv->nbmax, (size_t)tv->mc_gx * tv->mc_gy * tv->mc_gz * sizeof(uint16_t));
    if (e == hipSuccess) e = svr::launch_nbmax(tv->mm, tv->nbmax, tv->mc_gx, tv->mc_gy, tv->mc_gz, g.stream);
    std::vector<uint16_t> nb((size_t)tv->mc_gx * tv->mc_gy * tv->mc_gz);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e == hipSuccess) e = hipMemcpy(nb.data(), tv->nbmax, nb.size() * sizeof(uint16_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        if (tv->nbmax) { hipFree(tv->nbmax); tv->nbmax = nullptr; }
        return fail((int)e, "%s: neighbourhood table failed: %s", who, hipGetErrorName(e));
    }
    tv->nb_zero = (uint32_t)std::count(nb.begin(), nb.end(), (uint16_t)0);
    return 0;
}

} // namespace svr_host

extern "C" {

// The macro-cell grid of a volume (plain host code): the smallest cells, of 2^shift >= 2^shift_min voxels per axis, whose tables fit the
// fixed LDS arrays of the walks (svr_walk.hpp) -- one bit per cell in MASK_WORDS_MAX words (`empty`, deep-empty) AND one nibble per
// HALF-resolution cell in DIST_WORDS_MAX words (distances, bound classes).  For a box-like volume the half-resolution grid has about an
// eighth of the cells and the first limit decides; a flat volume (512 x 512 x 1: a quarter) or a line (a half) is limited by the second.
int svr_macro_grid(int nx, int ny, int nz, int shift_min, int out[8])
{
    if (nx <= 0 || ny <= 0 || nz <= 0 || shift_min < 0 || shift_min > 30 || !out) return -1;
    for (int sh = shift_min;; ++sh) {
        const size_t gx = (((size_t)nx - 1) >> sh) + 1, gy = (((size_t)ny - 1) >> sh) + 1, gz = (((size_t)nz - 1) >> sh) + 1;
        const size_t hgx = (gx + 1) / 2, hgy = (gy + 1) / 2, hgz = (gz + 1) / 2;
        if (gx * gy * gz <= (size_t)svr::MASK_WORDS_MAX * 32 && hgx * hgy * hgz <= (size_t)svr::DIST_WORDS_MAX * 8) {      // (sh = 31: one cell)
            out[0] = sh; out[1] = (int)gx; out[2] = (int)gy; out[3] = (int)gz; out[4] = (int)hgx; out[5] = (int)hgy; out[6] = (int)hgz;
            out[7] = (int)((hgx * hgy * hgz + 7) / 8);
            return sh;
        }
    }
}

// oom != null: running out of device memory is reported through *oom instead of as an error (the caller retries with a smaller layout)
// auto_rank: under AUTO, 0 = best layout that fits the addressing limits, 1 = skip CELL, 2 = skip CELL and PAIR
static uint64_t create_volume_texture(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, int layout, int auto_rank, bool* oom)
{
    if (ensure_init()) return 0;
    if (!voxels || nx <= 0 || ny <= 0 || nz <= 0) { fail(-6, "svr_create_volume_texture: bad arguments (%p, %d, %d, %d)", (const void*)voxels, nx, ny, nz); return 0; }
    if (layout != SVR_LAYOUT_AUTO && layout != SVR_LAYOUT_LINEAR && layout != SVR_LAYOUT_BRICK && layout != SVR_LAYOUT_PAIR && layout != SVR_LAYOUT_CELL) { fail(-6, "svr_create_volume_texture: unknown layout %d", layout); return 0; }
    {
        // BRICK needs 24-bit brick-row / brick-slab strides (svr_trace_tile.hip); AUTO picks it when they fit
        size_t bx = ((size_t)nx + 2 * svr::VOL_PAD + svr::BRICK_X - 1) / svr::BRICK_X;
        size_t by = ((size_t)ny + 2 * svr::VOL_PAD + svr::BRICK_Y - 1) / svr::BRICK_Y;
        bool brick_ok = (bx * by * 256) < ((size_t)1 << 24);
        // PAIR: the same bricks with 32-bit elements -- strides and byte offsets double
        const size_t bz_ = ((size_t)nz + 2 * svr::VOL_PAD + svr::BRICK_Z - 1) / svr::BRICK_Z;
        const bool pair_ok = (bx * by * 512) < ((size_t)1 << 24) && bx * by * bz_ * 512 < ((size_t)1 << 32);
        // CELL: 16-byte elements -- the element index uses 24-bit multiplies by the brick-row / brick-slab strides, the byte offset 32 bits
        const bool cell_ok = (bx * by * 128) < ((size_t)1 << 24) && bx * by * bz_ * 128 < ((size_t)1 << 32);      // 32-bit element index, 64-bit byte offset
        // AUTO: CELL (one 16-byte load per fetch; 8 x the memory of the u16 volume -- 2.2 GB for 512^3, 17 GB for 1024^3 of a 288 GB
        // device), else PAIR, else BRICK; on hipErrorOutOfMemory the next smaller one is tried (svr_create_volume_texture)
        if (layout == SVR_LAYOUT_AUTO) layout = auto_rank <= 0 && cell_ok ? SVR_LAYOUT_CELL : (auto_rank <= 1 && pair_ok ? SVR_LAYOUT_PAIR : (brick_ok ? SVR_LAYOUT_BRICK : SVR_LAYOUT_LINEAR));
        if (layout == SVR_LAYOUT_CELL && !cell_ok) { fail(-6, "svr_create_volume_texture: %dx%dx%d is too large for the CELL layout; use PAIR or BRICK", nx, ny, nz); return 0; }
        if (layout == SVR_LAYOUT_PAIR && !pair_ok) { fail(-6, "svr_create_volume_texture: %dx%dx%d is too large for the PAIR layout (32-bit byte offsets); use BRICK", nx, ny, nz); return 0; }
        if (layout == SVR_LAYOUT_BRICK && !brick_ok) { fail(-6, "svr_create_volume_texture: %dx%d slices are too large for the BRICK layout; use LINEAR", nx, ny); return 0; }
    }
    Texture* t = new Texture();
    t->magic = TEX_MAGIC; t->kind = TEX_VOLUME; t->nx = nx; t->ny = ny; t->nz = nz; t->layout = layout;
    size_t px = (size_t)nx + 2 * svr::VOL_PAD, py = (size_t)ny + 2 * svr::VOL_PAD, pz = (size_t)nz + 2 * svr::VOL_PAD;
    size_t elems;
    if (layout == SVR_LAYOUT_LINEAR) {
        t->sy = (int)px; t->sz = (int)(px * py); t->bnx = 0; t->bny = 0;
        elems = px * py * pz;
    } else {
        size_t bx = (px + svr::BRICK_X - 1) / svr::BRICK_X, by = (py + svr::BRICK_Y - 1) / svr::BRICK_Y, bz = (pz + svr::BRICK_Z - 1) / svr::BRICK_Z;
        t->bnx = (int)bx; t->bny = (int)by; t->sy = 0; t->sz = 0;
        elems = bx * by * bz * (size_t)(svr::BRICK_X * svr::BRICK_Y * svr::BRICK_Z);
    }
    if (elems >= ((size_t)1 << 32) || (layout != SVR_LAYOUT_CELL && elems >= ((size_t)1 << 31))) { delete t; fail(-6, "svr_create_volume_texture: %zu padded voxels exceed 32-bit byte offsets", elems); return 0; }
    // macro-cell grid for empty-space skipping (SVR_OPT_MACRO_SHIFT_MIN: coarser cells on request)
    {
        int mg[8];
        t->mc_shift = svr_macro_grid(nx, ny, nz, g.opt_macro_shift_min, mg);
        t->mc_gx = mg[1]; t->mc_gy = mg[2]; t->mc_gz = mg[3];
    }
    t->bytes = elems * (layout == SVR_LAYOUT_CELL ? 16u : (layout == SVR_LAYOUT_PAIR ? sizeof(uint32_t) : sizeof(uint16_t)));
    size_t src_bytes = (size_t)nx * ny * nz * sizeof(uint16_t);
    const uint16_t* d_src = voxels;
    uint16_t* staged = nullptr;
    hipError_t e;
    if (!src_is_device) {
        e = hipMalloc((void**)&staged, src_bytes);
        if (e == hipSuccess) e = hipMemcpy(staged, voxels, src_bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { if (staged) hipFree(staged); delete t; fail((int)e, "volume upload failed: %s", hipGetErrorName(e)); return 0; }
        d_src = staged;
    }
    e = hipMalloc(&t->data, t->bytes);
    if (e == hipSuccess && layout != SVR_LAYOUT_CELL) e = hipMemsetAsync(t->data, 0, t->bytes, g.stream);      // (the CELL repack writes every element)
    if (e == hipSuccess) e = svr::launch_repack(d_src, (uint16_t*)t->data, nx, ny, nz, layout, t->sy, t->sz, t->bnx, t->bny, g.stream);
    if (e == hipSuccess) e = hipMalloc((void**)&t->mm, (size_t)t->mc_gx * t->mc_gy * t->mc_gz * 2 * sizeof(uint16_t));
    if (e == hipSuccess) e = svr::launch_minmax(d_src, t->mm, nx, ny, nz, t->mc_shift, t->mc_gx, t->mc_gy, t->mc_gz, g.stream);
    if (e == hipSuccess && t->mc_shift >= 1) {
        const int fs = t->mc_shift - 1;
        t->fg_x = ((nx - 1) >> fs) + 1; t->fg_y = ((ny - 1) >> fs) + 1; t->fg_z = ((nz - 1) >> fs) + 1;
        e = hipMalloc((void**)&t->mm_fine, (size_t)t->fg_x * t->fg_y * t->fg_z * 2 * sizeof(uint16_t));
        if (e == hipSuccess) e = svr::launch_minmax(d_src, t->mm_fine, nx, ny, nz, fs, t->fg_x, t->fg_y, t->fg_z, g.stream);
    }
    if (e == hipSuccess) {
        // the wide table of the fast bound look-up: half-resolution macro-cells (cells of 2^(shift + 1)), footprints one voxel wider per side
        const int hgx = (t->mc_gx + 1) / 2, hgy = (t->mc_gy + 1) / 2, hgz = (t->mc_gz + 1) / 2;
        e = hipMalloc((void**)&t->mm_wide, (size_t)hgx * hgy * hgz * 2 * sizeof(uint16_t));
        if (e == hipSuccess) e = svr::launch_minmax(d_src, t->mm_wide, nx, ny, nz, t->mc_shift + 1, hgx, hgy, hgz, g.stream, 1);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (staged) hipFree(staged);
    if (e != hipSuccess) {
        const bool retry = oom != nullptr && e == hipErrorOutOfMemory && (layout == SVR_LAYOUT_PAIR || layout == SVR_LAYOUT_CELL);
        if (t->data) hipFree(t->data);
        if (t->mm) hipFree(t->mm);
        if (t->mm_fine) hipFree(t->mm_fine);
        if (t->mm_wide) hipFree(t->mm_wide);
        delete t;
        if (retry) { (void)hipGetLastError(); *oom = true; return 0; }
        fail((int)e, "volume texture creation failed: %s", hipGetErrorName(e));
        return 0;
    }
    uint64_t h = (uint64_t)(uintptr_t)t;
    g.textures[h] = t;
    return h;
}

uint64_t svr_create_volume_texture(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, int layout)
{
    // AUTO prefers the layouts that trade memory for fewer gathers (CELL: 8 x the u16 volume, PAIR: 2 x); if the device has no
    // room for one, the next smaller one is tried before giving up
    if (layout != SVR_LAYOUT_AUTO) return create_volume_texture(voxels, nx, ny, nz, src_is_device, layout, 0, nullptr);
    uint64_t h = 0;
    for (int rank = 0; rank <= 2 && h == 0; ++rank) {
        bool oom = false;
        h = create_volume_texture(voxels, nx, ny, nz, src_is_device, SVR_LAYOUT_AUTO, rank, rank < 2 ? &oom : nullptr);
        if (h == 0 && !oom) break;
    }
    return h;
}

static uint64_t create_float4_texture(int kind, const float* rgba, int w, int h, int src_is_device)
{
    if (ensure_init()) return 0;
    if (!rgba || w <= 0 || h <= 0) { fail(-6, "texture creation: bad arguments"); return 0; }
    Texture* t = new Texture();
    t->magic = TEX_MAGIC; t->kind = kind; t->nx = w; t->ny = h; t->nz = 1; t->layout = 0;
    t->bytes = (size_t)w * h * 4 * sizeof(float);
    hipError_t e = hipMalloc(&t->data, t->bytes);
    // a device-side table may still be being written by work queued on the caller's stream (torch pool streams do not
    // synchronise with the null stream): order the copy after it
    if (e == hipSuccess && src_is_device) e = hipStreamSynchronize(g.stream);
    if (e == hipSuccess) e = hipMemcpy(t->data, rgba, t->bytes, src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (t->data) hipFree(t->data); delete t; fail((int)e, "texture upload failed: %s", hipGetErrorName(e)); return 0; }
    uint64_t hd = (uint64_t)(uintptr_t)t;
    g.textures[hd] = t;
    return hd;
}

// zero_prefix[e] = number of entries < e of the padded alpha table (entry e = alpha of texel clamp(e-1),
// e in [0, n+2]) that are exactly zero; n+4 words
static int upload_zero_prefix(Texture* t)
{
    int n = t->nx;
    std::vector<float> host((size_t)n * 4);
    hipError_t e = hipMemcpy(host.data(), t->data, host.size() * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail((int)e, "transfer-function read-back failed: %s", hipGetErrorName(e));
    std::vector<uint32_t> pre((size_t)n + 4, 0u);
    for (int k = 0; k < n + 3; ++k) {
        int tex = k - 1 < 0 ? 0 : (k - 1 > n - 1 ? n - 1 : k - 1);
        pre[(size_t)k + 1] = pre[(size_t)k] + (host[(size_t)tex * 4 + 3] == 0.f ? 1u : 0u);
    }
    if (!t->zero_prefix) {
        e = hipMalloc((void**)&t->zero_prefix, pre.size() * sizeof(uint32_t));
        if (e != hipSuccess) return fail((int)e, "hipMalloc failed: %s", hipGetErrorName(e));
    }
    e = hipMemcpy(t->zero_prefix, pre.data(), pre.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail((int)e, "zero-prefix upload failed: %s", hipGetErrorName(e));
    t->version++;
    g.content_version++;
    return 0;
}

uint64_t svr_create_tf_texture(const float* rgba, int n, int src_is_device)
{
    if (n > SVR_TF_TABLE_SIZE) { ensure_init(); fail(-6, "transfer-function table of %d entries exceeds the LDS-resident limit of %d", n, SVR_TF_TABLE_SIZE); return 0; }
    uint64_t h = create_float4_texture(TEX_TF, rgba, n, 1, src_is_device);
    if (h && upload_zero_prefix(find_tex(h, TEX_TF))) return 0;
    return h;
}

int svr_update_tf_texture(uint64_t handle, const float* rgba, int n, int src_is_device)
{
    if (ensure_init()) return g.err_code;
    Texture* t = find_tex(handle, TEX_TF);
    if (!t) return fail(-2, "svr_update_tf_texture: bad handle");
    if (n != t->nx || !rgba) return fail(-6, "svr_update_tf_texture: size mismatch (%d vs %d)", n, t->nx);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(t->data, rgba, t->bytes, src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return upload_zero_prefix(t);
}

uint64_t svr_create_env_texture(const float* rgba, int w, int h, int src_is_device)
{
    const uint64_t hd = create_float4_texture(TEX_ENV, rgba, w, h, src_is_device);
    if (!hd) return 0;
    // the sampling table of SVR_OPT_ENV_NEE (a luminance distribution over the texels), built on the device
    Texture* t = find_tex(hd, TEX_ENV);
    float* tmp = nullptr;
    hipError_t e = hipMalloc((void**)&t->env_cdf, ((size_t)h * (w + 1) + h + 1) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&tmp, ((size_t)w * h + 1) * sizeof(float));
    if (e == hipSuccess) e = svr::launch_env_cdf((const float*)t->data, w, h, t->env_cdf, tmp, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (tmp) hipFree(tmp);
    if (e != hipSuccess) { svr_destroy_texture(hd); fail((int)e, "environment sampling table: %s", hipGetErrorName(e)); return 0; }
    return hd;
}

int svr_destroy_texture(uint64_t handle)
{
    if (ensure_init()) return g.err_code;
    auto it = g.textures.find(handle);
    if (it == g.textures.end()) return soft_fail(-2, "svr_destroy_texture: 0x%llx is not a live texture handle (destroyed twice?)", (unsigned long long)handle);
    HIP_TRY(hipDeviceSynchronize());
    Texture* t = it->second;
    free_texture(t);
    if (g.mask_vol == handle || g.mask_tf == handle) g.mask_valid = false;
    if (g.guides_vol == handle || g.guides_tf == handle) g.guides_valid = false;
    g.textures.erase(it);
    g.content_version++;
    return 0;
}

} // extern "C"
