// svr_geodesic.hip -- geodesic distances and influence zones inside region masks, and the splitting of a region at its necks that they
// make possible (svr_region_geodesic, _seed_labels, _geodesic_weights, _split, _zone_cut; the contract is in include/svr_abi.h, the design
// in DESIGN.md 8m).  Integers only, on the mask layout of svr_mask.hpp.
//
// Every voxel has one packed key (dist << 32) | zone in a workspace of 8 bytes per voxel; ~0 = "outside the domain or not reached".  A
// source has (0, label); every other voxel of the domain wants the lexicographic minimum over its allowed neighbours u of
// (dist(u) + w(u -> v), zone(u)) -- a plain unsigned 64-bit minimum of key(u) + (w << 32).  That system has one solution (induction on
// dist: weights are >= 1), and relaxing voxels in ANY order from ~0 reaches it: a key only falls, every key ever stored is the (cost,
// source label) of a real path, so it never falls below the solution, and a state in which no voxel can fall is the solution.
//   k_geo_init    one lane per voxel: the key from the label and the domain bit; a source marks its tile dirty.
//   k_geo_relax   one block per dirty tile of 32 x 8 x 8 voxels (a tile is one mask word wide).  The keys of the tile and of a halo of one
//     voxel go to LDS (34 x 10 x 10 x 8 B = 27200 B: rows of consecutive 8-byte words, which ds_read_b64 serves a half-wave at a time
//     without bank conflicts); a thread owns the column (lx, ly, 0 .. 7) and holds its eight domain bits in a register.  The block relaxes
//     its own voxels in place until an iteration lowers none, stores the voxels that fell, and marks the neighbour tiles that see a face
//     layer with a fallen voxel dirty for the next sweep -- the dirty-map protocol of svr_region_grow.hpp and the host loop of svr_sweep.hpp.
//   k_geo_finish  one lane per voxel: splits the keys into dist and zones and counts the unreached voxels of the domain.
//   k_geo_seeds, k_zone_cut: one lane per seed / per voxel.
// ONE WRITER, WHOLE PAIRS: a key in global memory is written by its tile's block alone, and every access to a key that another thread
//   may write -- halo loads and result stores in global memory, all LDS traffic of the relaxation -- is ONE aligned 64-bit atomic access
//   (relaxed; agent scope in global memory, workgroup scope in LDS), so a reader gets distance and zone from the same write.  A stale
//   key only delays a voxel (its tile is marked dirty by whoever lowers the key later); a torn one could pair a new distance with an
//   old, smaller label and would never be repaired.
// NO OVERFLOW: the host refuses wmax (voxels - 1) > 0xFFFFFFFE; a stored key is the cost of a simple path, so key + (w << 32) wraps only
//   for the key ~0, which the comparison `candidate > key` filters out.
// TERMINATION: no lane or block waits for another.  The relaxation of a tile works on a halo that is fixed in LDS, and an iteration
//   relaxes every voxel from values no worse than a Jacobi step would see, so it is over after at most one iteration per voxel of the
//   tile (Bellman-Ford); the loop is also counted against that number.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"
#include "svr_geo_keys.hpp"         // GeoWeights, move_class, the whole-pair accesses lds_get / lds_put / key_get / key_put
#include "svr_mask.hpp"             // RegionDims, lane_at, half_ballot, the grids
#include "svr_sweep.hpp"
#include "svr_volume_host.hpp"

using svr::failf;

namespace {

constexpr int GX = 32, GY = 8, GZ = 8;                   // tile in voxels; GX = one mask word
constexpr int GEO_THREADS = GX * GY;                     // one thread per column of GZ voxels
static_assert(GEO_THREADS == 256 && GX == 32, "the lane mapping assumes a tile one mask word wide and 256 threads");
constexpr uint64_t KEY_NONE = ~0ull;
constexpr int LANE_THREADS = MASK_THREADS;               // the one-lane-per-voxel kernels

struct GeoSeeds { uint32_t n; uint32_t at[SVR_REGION_MAX_SEEDS]; };   // at[i] = the voxel of seed i, or ~0 if a lower seed has it

__global__ __launch_bounds__(LANE_THREADS) void k_geo_init(const uint32_t* labels, const uint32_t* __restrict__ mask, RegionDims d, size_t words, int nty,
                                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ dirty)
{
    const LaneAt a = lane_at(d, words);
    if (!a.inside) return;
    const uint32_t lab = labels[a.v];
    const bool source = lab != 0u && ((mask[a.i] >> a.bit) & 1u);
    keys[a.v] = source ? (uint64_t)lab : KEY_NONE;
    if (source) dirty[((size_t)(a.z / GZ) * nty + a.y / GY) * d.wx + a.x / GX] = 1u;
}

__global__ __launch_bounds__(GEO_THREADS) void k_geo_relax(uint64_t* keys, const uint32_t* __restrict__ mask, RegionDims d, GeoWeights gw, int nty, int ntz,
                                                           uint32_t* dirty_cur, uint32_t* dirty_next, uint32_t* added)
{
    const size_t tile = blockIdx.x;
    if (!dirty_cur[tile]) return;
    __shared__ uint64_t K[GZ + 2][GY + 2][GX + 2];
    __shared__ uint32_t s_flags;
    const int tid = threadIdx.x;
    const int ntx = d.wx;
    const int tx = (int)(tile % ntx), ty = (int)((tile / ntx) % nty), tz = (int)(tile / ((size_t)ntx * nty));
    for (int i = tid; i < (GZ + 2) * (GY + 2) * (GX + 2); i += GEO_THREADS) {
        const int hx = i % (GX + 2), hy = (i / (GX + 2)) % (GY + 2), hz = i / ((GX + 2) * (GY + 2));
        const int gx = tx * GX + hx - 1, gy = ty * GY + hy - 1, gz = tz * GZ + hz - 1;
        uint64_t k = KEY_NONE;
        if (gx >= 0 && gx < d.nx && gy >= 0 && gy < d.ny && gz >= 0 && gz < d.nz) k = key_get(&keys[((size_t)gz * d.ny + gy) * d.nx + gx]);
        K[hz][hy][hx] = k;
    }
    const int lx = tid % GX, ly = tid / GX;
    const int gx = tx * GX + lx, gy = ty * GY + ly;
    uint32_t dom = 0u;                                   // bit lz: voxel (lx, ly, lz) of the tile is in the domain
    if (gx < d.nx && gy < d.ny)
        for (int lz = 0; lz < GZ; ++lz) {
            const int gz = tz * GZ + lz;
            if (gz < d.nz) dom |= ((mask[((size_t)gz * d.ny + gy) * d.wx + tx] >> lx) & 1u) << lz;
        }
    if (tid == 0) s_flags = 0u;
    __syncthreads();
    if (tid == 0) dirty_cur[tile] = 0u;                  // (every thread has read the flag: this buffer is the sweep after next's)
    uint32_t fell = 0u;                                  // bit lz: this thread lowered voxel (lx, ly, lz)
    for (int it = 0; it <= GX * GY * GZ; ++it) {
        int changed = 0;
#pragma unroll 1
        for (int lz = 0; lz < GZ; ++lz) {
            if (!((dom >> lz) & 1u)) continue;
            uint64_t* const own = &K[lz + 1][ly + 1][lx + 1];
            const uint64_t k0 = lds_get(own);
            uint64_t best = k0;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (dx == 0 && dy == 0 && dz == 0) continue;
                        const uint32_t w = gw.w[move_class(dx, dy, dz)];
                        if (w == 0u) continue;
                        const uint64_t u = lds_get(own + (dz * (GY + 2) + dy) * (GX + 2) + dx);
                        const uint64_t c = u + ((uint64_t)w << 32);                  // wraps only for u = ~0 (see the head of the file)
                        if (c > u && c < best) best = c;
                    }
            if (best < k0) {
                lds_put(own, best);
                fell |= 1u << lz;
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    if (fell) {
        uint32_t f = 64u;
        if (lx == 0) f |= 1u;
        if (lx == GX - 1) f |= 2u;
        if (ly == 0) f |= 4u;
        if (ly == GY - 1) f |= 8u;
        if (fell & 1u) f |= 16u;
        if (fell >> (GZ - 1)) f |= 32u;
        for (int lz = 0; lz < GZ; ++lz)
            if ((fell >> lz) & 1u) key_put(&keys[((size_t)(tz * GZ + lz) * d.ny + gy) * d.nx + gx], K[lz + 1][ly + 1][lx + 1]);
        atomicOr(&s_flags, f);
    }
    __syncthreads();
    const uint32_t flags = s_flags;
    if (tid == 0 && (flags & 64u)) atomicAdd(added, 1u);
    if (tid < 27) {
        // the neighbour tile in direction (dx, dy, dz) sees the layers of this tile that lie on all the faces the direction names
        const int dx = tid % 3 - 1, dy = (tid / 3) % 3 - 1, dz = tid / 9 - 1;
        if ((dx == 0 && dy == 0 && dz == 0) || !((gw.reach >> move_class(dx, dy, dz)) & 1u)) return;
        const uint32_t need = (dx < 0 ? 1u : dx > 0 ? 2u : 0u) | (dy < 0 ? 4u : dy > 0 ? 8u : 0u) | (dz < 0 ? 16u : dz > 0 ? 32u : 0u);
        const int ax = tx + dx, ay = ty + dy, az = tz + dz;
        if ((flags & need) == need && ax >= 0 && ax < ntx && ay >= 0 && ay < nty && az >= 0 && az < ntz)
            dirty_next[((size_t)az * nty + ay) * ntx + ax] = 1u;
    }
}

__global__ __launch_bounds__(LANE_THREADS) void k_geo_finish(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ mask, RegionDims d, size_t words,
                                                             uint32_t* dist, uint32_t* zones, uint32_t* unreached)
{
    const LaneAt a = lane_at(d, words);
    bool lost = false;
    if (a.inside) {
        const uint64_t k = keys[a.v];
        const uint32_t dd = (uint32_t)(k >> 32);
        if (dist) dist[a.v] = dd;
        if (zones) zones[a.v] = dd == SVR_GEO_NONE ? 0u : (uint32_t)k;
        lost = dd == SVR_GEO_NONE && ((mask[a.i] >> a.bit) & 1u);
    }
    const unsigned long long b = __ballot(lost);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(unreached, (uint32_t)__popcll(b));
}

__global__ void k_geo_seeds(GeoSeeds s, uint32_t* __restrict__ labels)
{
    const uint32_t i = threadIdx.x;
    if (i < s.n && s.at[i] != 0xFFFFFFFFu) labels[s.at[i]] = i + 1u;
}

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

int classes_of(int connectivity) { return connectivity == 6 ? 3 : connectivity == 18 ? 6 : 7; }

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

// the checked core of svr_region_geodesic and of the zones step of svr_region_split.  *unreached (may be NULL) = the voxels of the
// domain that no source reaches.  Synchronises the stream.
int geodesic_run(const char* who, const uint32_t* labels, const uint32_t* mask, const RegionDims& d, const GeoWeights& gw, uint32_t max_sweeps, uint32_t* dist,
                 uint32_t* zones, uint32_t* unreached, uint32_t* sweeps_out)
{
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const size_t n = (size_t)d.nx * d.ny * d.nz, words = mask_words(d);
    const int nty = (d.ny + GY - 1) / GY, ntz = (d.nz + GZ - 1) / GZ;
    const size_t tiles = (size_t)d.wx * nty * ntz;
    const uint32_t cap = max_sweeps ? max_sweeps : svr_region_geodesic_default_max_sweeps(d.nx, d.ny, d.nz);
    DeviceBuffer buf;                                    // the keys, then the two dirty maps, the batch counters and the unreached count
    const size_t small = 2 * tiles + SVR_REGION_BATCH + 1;
    SVR_HIP_TRY(buf.alloc(n * sizeof(uint64_t) + small * sizeof(uint32_t)));
    uint64_t* const keys = buf.as<uint64_t>();
    uint32_t* const dirty = (uint32_t*)(keys + n);
    uint32_t* const added = dirty + 2 * tiles;
    uint32_t* const lost = added + SVR_REGION_BATCH;
    CallTimer timer(g_events, st);                       // (the launches, not the allocation)
    SVR_HIP_TRY(hipMemsetAsync(dirty, 0, small * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_geo_init, lane_grid(words), dim3(LANE_THREADS), 0, st, labels, mask, d, words, nty, keys, dirty);
    SVR_HIP_TRY(hipGetLastError());
    uint32_t sweeps = 0u;
    bool done = false;
    SVR_HIP_TRY(sweep_to_fixpoint(st, tiles, dirty, added, cap, &sweeps, &done, [&](uint32_t* cur, uint32_t* next, uint32_t* add) {
        hipLaunchKernelGGL(k_geo_relax, dim3((uint32_t)tiles), dim3(GEO_THREADS), 0, st, keys, mask, d, gw, nty, ntz, cur, next, add);
    }));
    hipLaunchKernelGGL(k_geo_finish, lane_grid(words), dim3(LANE_THREADS), 0, st, keys, mask, d, words, dist, zones, lost);
    SVR_HIP_TRY(hipGetLastError());
    timer.stop();
    uint32_t lost_host = 0u;
    SVR_HIP_TRY(hipMemcpyAsync(&lost_host, lost, sizeof lost_host, hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));               // (buf is freed on return)
    if (sweeps_out) *sweeps_out = sweeps;
    if (unreached) *unreached = lost_host;
    if (!done) return failf(SVR_REGION_ERR_SWEEPS, "%s: keys were still falling after %u sweeps; the outputs are upper bounds, not the map", who, sweeps);
    return 0;
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
    GeoWeights gw;
    if (int e = check_step_weights(who, step_weights_or_null, 26, nx, ny, nz, &gw)) return e;
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t map_bytes = (size_t)nx * ny * nz * sizeof(uint32_t), mask_bytes = mask_words(d) * sizeof(uint32_t);
    uint32_t* const outs[2] = {dist_device_or_null, zones_device_or_null};
    for (int i = 0; i < 2; ++i) {
        if (!outs[i]) continue;
        const bool alias = i == 1 && outs[i] == marker_labels_device;                 // zones in place over the labels
        if (overlap(outs[i], map_bytes, domain_mask_device, mask_bytes) || (!alias && overlap(outs[i], map_bytes, marker_labels_device, map_bytes)))
            return failf(-3, "%s: an output must not overlap an input (only zones may be the marker labels themselves)", who);
    }
    if (outs[0] && outs[1] && overlap(outs[0], map_bytes, outs[1], map_bytes)) return failf(-3, "%s: the two outputs must not overlap", who);
    return geodesic_run(who, marker_labels_device, domain_mask_device, d, gw, max_sweeps, dist_device_or_null, zones_device_or_null, nullptr, sweeps_out);
}

int svr_region_seed_labels(const int32_t* seeds_xyz, uint32_t nseeds, int nx, int ny, int nz, uint32_t* labels_device)
{
    const char* who = "svr_region_seed_labels";
    if (!seeds_xyz || !labels_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (int e = check_seeds(who, seeds_xyz, nseeds, nx, ny, nz)) return e;
    GeoSeeds seeds;
    memset(&seeds, 0, sizeof seeds);
    seeds.n = nseeds;
    uint32_t at[SVR_REGION_MAX_SEEDS];
    for (uint32_t i = 0; i < nseeds; ++i) {
        const int32_t x = seeds_xyz[3u * i], y = seeds_xyz[3u * i + 1u], z = seeds_xyz[3u * i + 2u];
        at[i] = (uint32_t)(((size_t)z * ny + y) * nx + x);                // below 2^31
        seeds.at[i] = at[i];
        for (uint32_t j = 0; j < i; ++j)
            if (at[j] == at[i]) seeds.at[i] = 0xFFFFFFFFu;                // the lowest seed on a voxel wins
    }
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(hipMemsetAsync(labels_device, 0, (size_t)nx * ny * nz * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_geo_seeds, dim3(1), dim3(SVR_REGION_MAX_SEEDS), 0, st, seeds, labels_device);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
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
    GeoWeights gw;
    if (int e = check_step_weights(who, step_weights_or_null, connectivity, nx, ny, nz, &gw)) return e;
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
    const int e = geodesic_run(who, zones_device, in_mask_device, d, gw, max_sweeps, nullptr, zones_device, &lost, sweeps_out);
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
