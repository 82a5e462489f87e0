// svr_geodesic.hip -- geodesic distances and influence zones inside region masks, and the splitting of a region at its necks that they
// make possible (svr_region_geodesic, _seed_labels, _geodesic_weights, _split, _zone_cut; the contract is in include/svr_abi.h, the design
// in DESIGN.md 8m).  The keys, the relaxation under PlainCost and its host driver are in svr_geo_relax.hpp; here are the step weights
// and their overflow bound, the default sweep cap, the split and k_zone_cut (one lane per voxel).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"
#include "svr_geo_relax.hpp"        // PlainCost, geo_run, place_seeds, check_geo_outputs, classes_of; the mask layout and the host scaffolding

using svr::failf;

namespace {

template <int CONN>
__global__ __launch_bounds__(LANE_THREADS) void k_zone_cut(const uint32_t* __restrict__ zones, RegionDims d, size_t words, uint32_t* __restrict__ out)
{
    const LaneAt a = lane_at(d, words);
    bool keep = false;
    if (a.inside) {
        const uint32_t z = zones[a.v];
        keep = z != 0u;
        if (keep)
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int k = (dx != 0) + (dy != 0) + (dz != 0);
                        if (k == 0 || k > (CONN == 6 ? 1 : CONN == 18 ? 2 : 3)) continue;
                        const int x = a.x + dx, y = a.y + dy, zz = a.z + dz;
                        if (x < 0 || x >= d.nx || y < 0 || y >= d.ny || zz < 0 || zz >= d.nz) continue;
                        const uint32_t n = zones[((size_t)zz * d.ny + y) * d.nx + x];
                        if (n != 0u && n < z) keep = false;
                    }
    }
    const uint32_t word = half_ballot(keep);
    if (a.bit == 0 && a.word_ok) out[a.i] = word;
}

// ---------------- host side ----------------
constexpr uint32_t CHAMFER[7] = {3u, 3u, 3u, 4u, 4u, 4u, 5u};

// wmax (voxels - 1) <= 0xFFFFFFFE: the cost of the longest simple path fits (voxels <= 2^31, wmax < 2^32: the product is below 2^63)
bool step_weights_fit(const uint64_t w[7], int nx, int ny, int nz)
{
    uint64_t wmax = 0;
    for (int c = 0; c < 7; ++c) wmax = w[c] > wmax ? w[c] : wmax;
    if (wmax > 0xFFFFFFFFull) return false;
    return wmax * ((uint64_t)nx * (uint64_t)ny * (uint64_t)nz - 1ull) <= 0xFFFFFFFEull;
}

// the weights of a call: the caller's, or the chamfer weights of the classes that `connectivity` allows
int check_step_weights(const char* who, const uint32_t* weights_or_null, int connectivity, int nx, int ny, int nz, GeoWeights* out)
{
    uint64_t w64[7];
    bool any = false;
    for (int c = 0; c < 7; ++c) {
        out->w[c] = weights_or_null ? weights_or_null[c] : c < classes_of(connectivity) ? CHAMFER[c] : 0u;
        w64[c] = out->w[c];
        any = any || out->w[c] != 0u;
    }
    if (!any) return failf(-3, "%s: all seven step weights are 0: no move is allowed", who);
    if (!step_weights_fit(w64, nx, ny, nz))
        return failf(-3, "%s: the longest path of %d x %d x %d under step weights %u, %u, %u, %u, %u, %u, %u would overflow 32 bits", who, nx, ny, nz, out->w[0],
                     out->w[1], out->w[2], out->w[3], out->w[4], out->w[5], out->w[6]);
    out->reach = geo_reach(out->w);
    return 0;
}

uint64_t geo_tiles(int nx, int ny, int nz) { return (uint64_t)((nx + GX - 1) / GX) * (uint64_t)((ny + GY - 1) / GY) * (uint64_t)((nz + GZ - 1) / GZ); }

CallEvents g_events;                                     // around the device work of the last call of this file (svr_region_geodesic_last_ms)

// geo_run under PlainCost.  *sweeps_out and *unreached (either may be NULL) are written when the sweeps ran; the count of capped voxels
// is ignored: a geodesic distance may be 0xFFFFFFFE.
int geodesic_run(const char* who, const uint32_t* labels, const uint32_t* mask, const RegionDims& d, const PlainCost& cost, uint32_t max_sweeps, uint32_t* dist,
                 uint32_t* zones, uint32_t* unreached, uint32_t* sweeps_out)
{
    GeoResult res;
    const int e = geo_run(who, g_events, cost, nullptr, labels, mask, d, max_sweeps, dist, zones, &res);
    if (e && e != SVR_REGION_ERR_SWEEPS) return e;
    if (sweeps_out) *sweeps_out = res.sweeps;
    if (unreached) *unreached = res.unreached;
    return e;
}

} // namespace

extern "C" {

uint32_t svr_region_geodesic_default_max_sweeps(int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0u;
    const uint64_t cap = 64u + 16u * geo_tiles(nx, ny, nz);
    return (uint32_t)(cap < 65536u ? cap : 65536u);
}

int svr_region_geodesic(const uint32_t* marker_labels_device, const uint32_t* domain_mask_device, int nx, int ny, int nz,
                        const uint32_t* step_weights_or_null, uint32_t max_sweeps, uint32_t* dist_device_or_null, uint32_t* zones_device_or_null,
                        uint32_t* sweeps_out)
{
    const char* who = "svr_region_geodesic";
    if (!marker_labels_device || !domain_mask_device) return failf(-4, "%s: null argument", who);
    if (!dist_device_or_null && !zones_device_or_null) return failf(-4, "%s: both outputs are null", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    PlainCost cost;
    if (int e = check_step_weights(who, step_weights_or_null, 26, nx, ny, nz, &cost.gw)) return e;
    const RegionDims d = make_dims(nx, ny, nz);
    if (int e = check_geo_outputs(who, marker_labels_device, (size_t)nx * ny * nz * sizeof(uint32_t), domain_mask_device, mask_words(d) * sizeof(uint32_t), nullptr, 0,
                                  dist_device_or_null, zones_device_or_null))
        return e;
    return geodesic_run(who, marker_labels_device, domain_mask_device, d, cost, max_sweeps, dist_device_or_null, zones_device_or_null, nullptr, sweeps_out);
}

int svr_region_seed_labels(const int32_t* seeds_xyz, uint32_t nseeds, int nx, int ny, int nz, uint32_t* labels_device)
{
    const char* who = "svr_region_seed_labels";
    if (!seeds_xyz || !labels_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (int e = check_seeds(who, seeds_xyz, nseeds, nx, ny, nz)) return e;
    return place_seeds(who, g_events, seeds_xyz, nullptr, nseeds, nx, ny, nz, labels_device);     // the class of seed i is i + 1
}

int svr_region_geodesic_weights(const double spacing[3], int connectivity, int nx, int ny, int nz, uint32_t weights[7], double* unit_out)
{
    const char* who = "svr_region_geodesic_weights";
    if (!spacing || !weights || !unit_out) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (int e = check_connectivity(who, "connectivity", connectivity)) return e;
    for (int a = 0; a < 3; ++a)
        if (!(spacing[a] > 0.0) || !std::isfinite(spacing[a])) return failf(-3, "%s: the spacing must be positive and finite (got %g, %g, %g)", who, spacing[0], spacing[1], spacing[2]);
    const double sx = spacing[0], sy = spacing[1], sz = spacing[2];
    const double len[7] = {sx, sy, sz, std::sqrt(sx * sx + sy * sy), std::sqrt(sx * sx + sz * sz), std::sqrt(sy * sy + sz * sz), std::sqrt(sx * sx + sy * sy + sz * sz)};
    const double smin = std::fmin(sx, std::fmin(sy, sz));
    for (int k = 3; k >= 0; --k) {
        const double unit = smin / (double)(1 << k);
        uint64_t w[7];
        bool ok = unit > 0.0;
        for (int c = 0; c < 7 && ok; ++c) {
            w[c] = 0;
            if (c >= classes_of(connectivity)) continue;
            const double r = len[c] / unit;
            if (!(r < 4294967295.5)) { ok = false; break; }
            const long long v = std::llround(r);
            w[c] = v < 1 ? 1ull : (uint64_t)v;
        }
        if (!ok || !step_weights_fit(w, nx, ny, nz)) continue;
        for (int c = 0; c < 7; ++c) weights[c] = (uint32_t)w[c];
        *unit_out = unit;
        return 0;
    }
    return failf(-3, "%s: no unit of min(spacing) / 2^k, k = 3 .. 0, keeps the path costs of %d x %d x %d at spacing %g, %g, %g inside 32 bits", who, nx, ny, nz,
                 sx, sy, sz);
}

int svr_region_split(const uint32_t* in_mask_device, int nx, int ny, int nz, const uint32_t* dist_weights_or_null, uint32_t r2, int connectivity,
                     const uint32_t* step_weights_or_null, uint32_t max_sweeps, uint32_t* zones_device, uint32_t* count_out, uint32_t* unreached_out,
                     uint32_t* sweeps_out)
{
    const char* who = "svr_region_split";
    if (!in_mask_device || !zones_device || !count_out || !unreached_out) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (int e = check_connectivity(who, "connectivity", connectivity)) return e;
    PlainCost cost;
    if (int e = check_step_weights(who, step_weights_or_null, connectivity, nx, ny, nz, &cost.gw)) return e;
    uint32_t dw[3];
    if (int e = svr::check_distance_weights(who, dist_weights_or_null, nx, ny, nz, dw)) return e;
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t words = mask_words(d);
    if (overlap(zones_device, (size_t)nx * ny * nz * sizeof(uint32_t), in_mask_device, words * sizeof(uint32_t)))
        return failf(-3, "%s: zones must not overlap the input mask", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    uint32_t count = 0u;
    {
        DeviceBuffer cores;                              // the eroded mask: freed at the end of this block, before the keys are allocated
        SVR_HIP_TRY(cores.alloc(words * sizeof(uint32_t)));
        int e = svr_region_ball(in_mask_device, nx, ny, nz, SVR_MORPH_ERODE, dw, r2, cores.as<uint32_t>());
        if (!e) e = svr_region_label(cores.as<uint32_t>(), nx, ny, nz, connectivity, zones_device, &count);   // the labels go where the zones will
        if (e) return e;
        SVR_HIP_TRY(hipStreamSynchronize(svr::current_stream()));                                 // (an r2 = 0 ball and the label are done with `cores`)
    }
    uint32_t lost = 0u;
    const int e = geodesic_run(who, zones_device, in_mask_device, d, cost, max_sweeps, nullptr, zones_device, &lost, sweeps_out);
    if (e) return e;
    *count_out = count;
    *unreached_out = lost;
    return 0;
}

int svr_region_zone_cut(const uint32_t* zones_device, int nx, int ny, int nz, int connectivity, uint32_t* out_mask_device)
{
    const char* who = "svr_region_zone_cut";
    if (!zones_device || !out_mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (int e = check_connectivity(who, "connectivity", connectivity)) return e;
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t words = mask_words(d);
    if (overlap(out_mask_device, words * sizeof(uint32_t), zones_device, (size_t)nx * ny * nz * sizeof(uint32_t)))
        return failf(-3, "%s: out must not overlap the zones", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    const dim3 g = lane_grid(words), b(LANE_THREADS);
    if (connectivity == 6) hipLaunchKernelGGL((k_zone_cut<6>), g, b, 0, st, zones_device, d, words, out_mask_device);
    else if (connectivity == 18) hipLaunchKernelGGL((k_zone_cut<18>), g, b, 0, st, zones_device, d, words, out_mask_device);
    else hipLaunchKernelGGL((k_zone_cut<26>), g, b, 0, st, zones_device, d, words, out_mask_device);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_region_geodesic_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_region_geodesic_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

} // extern "C"
