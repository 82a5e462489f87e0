// svr_growcut.hip -- grow-from-seeds: every voxel goes to the class whose markers reach it over the path that crosses the least image
// contrast (Fast GrowCut, Zhu et al.: the shortest-path form of GrowCut), and the two calls that turn picks and masks into class markers
// (svr_region_growcut, _growcut_params_default, _seed_classes, _label_paint, _growcut_last_ms; the contract is in include/svr_abi.h, the
// design in DESIGN.md 8q).  Integers only, on the mask layout of svr_mask.hpp.
//
// The machinery is that of svr_geodesic.hip, which see: one packed key (cost << 32) | zone per voxel in a workspace of 8 bytes per voxel,
// ~0 = "outside the domain or not reached"; tiles of 32 x 8 x 8 voxels, one thread per column of 8; ONE WRITER per key and WHOLE PAIRS in
// every access to a key that another thread may write (svr_geo_keys.hpp); the dirty-tile sweeps of svr_sweep.hpp; no lane or block waits
// for another.
//   k_gc_init     one lane per voxel: the key from the marker and the domain bit (a NULL domain is the whole volume); a source marks
//     dirty every tile that holds it or one of its neighbours.
//   k_gc_relax    one block per dirty tile: k_geo_relax with the voxel values of the tile and its halo beside the keys in LDS.
//   k_gc_finish   one lane per voxel: splits the keys into cost and zones, counts the unreached and the saturated voxels of the domain.
//   k_gc_seeds, k_gc_paint: one lane per seed / per voxel.
// What is new:
// THE MOVE COST: cost(u, v) = w[class] + gain * (|I(u) - I(v)| >> shift), I the raw u16 voxel: symmetric, >= 1 on an allowed move and, by
//   the host's refusal of wmax + gain * (65535 >> shift) > 0x7FFFFFFF, below 2^31.
// SATURATION: the a-priori bound of the geodesic call (wmax (voxels - 1) <= 0xFFFFFFFE) would refuse every real volume here, so the device
//   adds with saturation: sat(x) = min(x, CAP), CAP = SVR_GROWCUT_CAP = 0xFFFFFFFE, one below the NONE of an unreached voxel.  A stored cost
//   is <= CAP and a move costs < 2^31, so the 64-bit sum is below 2^33 and needs no further check.
//   THE RESULT IS STILL UNIQUE.  Define key*(v) = the lexicographic minimum over all walks inside the domain from a source to v of
//   (sat(cost of the walk), label of its source).  Because sat(sat(a) + w) = sat(a + w), saturating after every move of a walk gives the
//   same number as saturating its sum once.  So, relaxing from "all NONE" in any order: (1) every key ever stored is (sat(cost), label) of
//   a real walk -- by induction over the stores, a candidate being the stored key of a neighbour extended by one move -- hence never below
//   key*; (2) keys only fall and take finitely many values, so the relaxation stops; (3) in a state where no voxel can fall, key(v) <=
//   (sat(cost), label) for every walk to v, by induction over the walk's length (the source holds (0, label) or less; one more move is
//   one more relaxation that cannot lower v).  (1) and (3) give key = key* everywhere.  (The fixpoint EQUATIONS alone have other solutions
//   on the plateau cost = CAP, where voxels could hold up one another's label with no source behind it; they are not reachable from NONE.)
// TERMINATION INSIDE A TILE: with the halo fixed in LDS, the limit of a tile's relaxation is the minimum over walks inside the tile from a
//   halo or source voxel.  Cutting a cycle out of a walk keeps its source and does not raise its saturated cost (sat is monotone), so the
//   minimum is attained on a walk that visits no voxel of the tile twice: fewer than GX GY GZ moves.  An iteration relaxes every voxel
//   from values no worse than a Jacobi step would see, so after k iterations every key is at most the minimum over walks of k moves,
//   whether a move added cost or -- on the saturated plateau -- none, where only the label can still fall; that is again one move of a
//   simple walk.  One iteration per voxel of the tile therefore reaches the limit, as in k_geo_relax, and the loop is counted against it.
// LDS: the keys of the tile and its halo as in k_geo_relax (34 x 10 x 10 x 8 B = 27200 B) and their voxel values as u16 (6800 B): 34000 B a
//   block, four blocks a CU by LDS.  A half-wave (one x row of the tile) reads 32 consecutive u16 of a value row: 64 consecutive bytes, 16
//   or 17 consecutive dwords with two lanes on each, which ds_read_u16 serves in one pass (bank = dword index mod 32; lanes that share a
//   dword are a broadcast).  The value rows need no padding, and being a separate array they leave the 8-byte alignment and the
//   conflict-free rows of the keys as they were.  A thread keeps its own column's eight values packed in two 64-bit registers.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"
#include "svr_geo_keys.hpp"         // GeoWeights, move_class, geo_reach, the whole-pair accesses
#include "svr_mask.hpp"             // RegionDims, lane_at, the grids
#include "svr_sweep.hpp"
#include "svr_volume_host.hpp"

using svr::failf;

namespace {

constexpr int GX = 32, GY = 8, GZ = 8;                   // tile in voxels; GX = one mask word
constexpr int GC_THREADS = GX * GY;                      // one thread per column of GZ voxels
static_assert(GC_THREADS == 256 && GX == 32 && GZ == 8, "the lane mapping assumes a tile one mask word wide, 256 threads and columns of 8");
constexpr uint64_t KEY_NONE = ~0ull;
constexpr uint64_t CAP = SVR_GROWCUT_CAP;
constexpr int LANE_THREADS = MASK_THREADS;               // the one-lane-per-voxel kernels

struct GrowCost { GeoWeights gw; uint32_t gain, shift; };
// at[i] = the voxel of seed i, or ~0 if a lower seed has it; cls[i] = its class
struct ClassSeeds { uint32_t n; uint32_t at[SVR_REGION_MAX_SEEDS]; uint32_t cls[SVR_REGION_MAX_SEEDS]; };

// a NULL mask is the whole volume
__device__ inline bool in_domain(const uint32_t* __restrict__ mask, size_t word, int bit) { return !mask || ((mask[word] >> bit) & 1u); }

__global__ __launch_bounds__(LANE_THREADS) void k_gc_init(const uint32_t* labels, const uint32_t* __restrict__ mask, RegionDims d, size_t words, int nty,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ dirty)
{
    const LaneAt a = lane_at(d, words);
    if (!a.inside) return;
    const uint32_t lab = labels[a.v];
    const bool source = lab != 0u && in_domain(mask, a.i, a.bit);
    keys[a.v] = source ? (uint64_t)lab : KEY_NONE;
    if (!source) return;
    // every tile that holds the source or a neighbour of it: a source never falls, so its own tile's block would not mark the tile
    // across a face for it -- and on a thin or sparse domain no other voxel of that face layer need fall either
    const int x0 = max(a.x - 1, 0) / GX, x1 = min(a.x + 1, d.nx - 1) / GX, y0 = max(a.y - 1, 0) / GY, y1 = min(a.y + 1, d.ny - 1) / GY;
    const int z0 = max(a.z - 1, 0) / GZ, z1 = min(a.z + 1, d.nz - 1) / GZ;
    for (int tz = z0; tz <= z1; ++tz)
        for (int ty = y0; ty <= y1; ++ty)
            for (int tx = x0; tx <= x1; ++tx) dirty[((size_t)tz * nty + ty) * d.wx + tx] = 1u;
}

__global__ __launch_bounds__(GC_THREADS) void k_gc_relax(uint64_t* keys, const uint16_t* __restrict__ vox, const uint32_t* __restrict__ mask, RegionDims d,
                                                         GrowCost gc, int nty, int ntz, uint32_t* dirty_cur, uint32_t* dirty_next, uint32_t* added)
{
    const size_t tile = blockIdx.x;
    if (!dirty_cur[tile]) return;
    __shared__ uint64_t K[GZ + 2][GY + 2][GX + 2];
    __shared__ uint16_t V[GZ + 2][GY + 2][GX + 2];
    __shared__ uint32_t s_flags;
    const int tid = threadIdx.x;
    const int ntx = d.wx;
    const int tx = (int)(tile % ntx), ty = (int)((tile / ntx) % nty), tz = (int)(tile / ((size_t)ntx * nty));
    for (int i = tid; i < (GZ + 2) * (GY + 2) * (GX + 2); i += GC_THREADS) {
        const int hx = i % (GX + 2), hy = (i / (GX + 2)) % (GY + 2), hz = i / ((GX + 2) * (GY + 2));
        const int gx = tx * GX + hx - 1, gy = ty * GY + hy - 1, gz = tz * GZ + hz - 1;
        uint64_t k = KEY_NONE;
        uint16_t v = 0;                                  // (outside the volume the key is NONE and the value is never used)
        if (gx >= 0 && gx < d.nx && gy >= 0 && gy < d.ny && gz >= 0 && gz < d.nz) {
            const size_t at = ((size_t)gz * d.ny + gy) * d.nx + gx;
            k = key_get(&keys[at]);
            v = vox[at];
        }
        K[hz][hy][hx] = k;
        V[hz][hy][hx] = v;
    }
    const int lx = tid % GX, ly = tid / GX;
    const int gx = tx * GX + lx, gy = ty * GY + ly;
    uint32_t dom = 0u;                                   // bit lz: voxel (lx, ly, lz) of the tile is in the domain
    if (gx < d.nx && gy < d.ny)
        for (int lz = 0; lz < GZ; ++lz) {
            const int gz = tz * GZ + lz;
            if (gz < d.nz) dom |= (in_domain(mask, ((size_t)gz * d.ny + gy) * d.wx + tx, lx) ? 1u : 0u) << lz;
        }
    if (tid == 0) s_flags = 0u;
    __syncthreads();
    if (tid == 0) dirty_cur[tile] = 0u;                  // (every thread has read the flag: this buffer is the sweep after next's)
    uint64_t mine[2] = {0ull, 0ull};                     // the column's own values: lz 0 .. 3 and 4 .. 7, 16 bits each
#pragma unroll
    for (int lz = 0; lz < GZ; ++lz) mine[lz >> 2] |= (uint64_t)V[lz + 1][ly + 1][lx + 1] << (16 * (lz & 3));
    uint32_t fell = 0u;                                  // bit lz: this thread lowered voxel (lx, ly, lz)
    for (int it = 0; it <= GX * GY * GZ; ++it) {
        int changed = 0;
#pragma unroll 1
        for (int lz = 0; lz < GZ; ++lz) {
            if (!((dom >> lz) & 1u)) continue;
            const int at = ((lz + 1) * (GY + 2) + ly + 1) * (GX + 2) + lx + 1;
            uint64_t* const own = &K[0][0][0] + at;
            const uint16_t* const val = &V[0][0][0] + at;
            const int32_t iv = (int32_t)(((lz & 4) ? mine[1] : mine[0]) >> (16 * (lz & 3)) & 0xFFFFull);
            const uint64_t k0 = lds_get(own);
            uint64_t best = k0;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (dx == 0 && dy == 0 && dz == 0) continue;
                        const uint32_t w = gc.gw.w[move_class(dx, dy, dz)];
                        if (w == 0u) continue;
                        const int off = (dz * (GY + 2) + dy) * (GX + 2) + dx;
                        const uint64_t u = lds_get(own + off);
                        const int32_t iu = (int32_t)val[off];
                        const uint32_t diff = (uint32_t)(iu > iv ? iu - iv : iv - iu);
                        const uint64_t cost = (uint64_t)(w + gc.gain * (diff >> gc.shift));      // below 2^31 (the host's refusal)
                        const uint64_t du = u >> 32;
                        uint64_t c = du + cost;                                                    // below 2^33
                        c = c < CAP ? c : CAP;
                        c = (c << 32) | (u & 0xFFFFFFFFull);
                        if (du != (uint64_t)SVR_GEO_NONE && c < best) best = c;
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
        if ((dx == 0 && dy == 0 && dz == 0) || !((gc.gw.reach >> move_class(dx, dy, dz)) & 1u)) return;
        const uint32_t need = (dx < 0 ? 1u : dx > 0 ? 2u : 0u) | (dy < 0 ? 4u : dy > 0 ? 8u : 0u) | (dz < 0 ? 16u : dz > 0 ? 32u : 0u);
        const int ax = tx + dx, ay = ty + dy, az = tz + dz;
        if ((flags & need) == need && ax >= 0 && ax < ntx && ay >= 0 && ay < nty && az >= 0 && az < ntz)
            dirty_next[((size_t)az * nty + ay) * ntx + ax] = 1u;
    }
}

// counts[0] = the voxels of the domain that no source reaches, counts[1] = those whose cost is the cap
__global__ __launch_bounds__(LANE_THREADS) void k_gc_finish(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ mask, RegionDims d, size_t words,
                                                            uint32_t* cost, uint32_t* zones, uint32_t* counts)
{
    const LaneAt a = lane_at(d, words);
    bool lost = false, capped = false;
    if (a.inside) {
        const uint64_t k = keys[a.v];
        const uint32_t dd = (uint32_t)(k >> 32);
        if (cost) cost[a.v] = dd;
        if (zones) zones[a.v] = dd == SVR_GEO_NONE ? 0u : (uint32_t)k;
        lost = dd == SVR_GEO_NONE && in_domain(mask, a.i, a.bit);
        capped = dd == SVR_GROWCUT_CAP;                  // (a key below NONE is a voxel of the domain)
    }
    const unsigned long long bl = __ballot(lost), bc = __ballot(capped);
    if ((threadIdx.x & 63) == 0) {
        if (bl) atomicAdd(&counts[0], (uint32_t)__popcll(bl));
        if (bc) atomicAdd(&counts[1], (uint32_t)__popcll(bc));
    }
}

__global__ void k_gc_seeds(ClassSeeds s, uint32_t* __restrict__ labels)
{
    const uint32_t i = threadIdx.x;
    if (i < s.n && s.at[i] != 0xFFFFFFFFu) labels[s.at[i]] = s.cls[i];
}

__global__ __launch_bounds__(LANE_THREADS) void k_gc_paint(uint32_t* __restrict__ labels, const uint32_t* __restrict__ mask, RegionDims d, size_t words,
                                                           uint32_t label, int only_unlabelled)
{
    const LaneAt a = lane_at(d, words);
    if (!a.inside || !((mask[a.i] >> a.bit) & 1u)) return;
    if (only_unlabelled && labels[a.v] != 0u) return;
    labels[a.v] = label;
}

// ---------------- host side ----------------
int classes_of(int connectivity) { return connectivity == 6 ? 3 : connectivity == 18 ? 6 : 7; }

int check_dims3(const char* who, const int32_t* d) { return check_dims(who, d[0], d[1], d[2]); }

int check_params(const char* who, const svr_growcut_params* p, GrowCost* out)
{
    uint64_t wmax = 0;
    for (int c = 0; c < 7; ++c) {
        out->gw.w[c] = p->step_weights[c];
        wmax = p->step_weights[c] > wmax ? p->step_weights[c] : wmax;
    }
    if (wmax == 0) return failf(-3, "%s: all seven step weights are 0: no move is allowed", who);
    if (p->contrast_gain > 65535u) return failf(-3, "%s: contrast_gain must lie in 0 .. 65535 (got %u)", who, p->contrast_gain);
    if (p->contrast_shift > 15u) return failf(-3, "%s: contrast_shift must lie in 0 .. 15 (got %u)", who, p->contrast_shift);
    if (wmax + (uint64_t)p->contrast_gain * (uint64_t)(65535u >> p->contrast_shift) > 0x7FFFFFFFull)
        return failf(-3, "%s: a move could cost more than 0x7FFFFFFF under the largest step weight %llu, contrast_gain %u and contrast_shift %u", who,
                     (unsigned long long)wmax, p->contrast_gain, p->contrast_shift);
    out->gw.reach = geo_reach(out->gw.w);
    out->gain = p->contrast_gain;
    out->shift = p->contrast_shift;
    return 0;
}

CallEvents g_events;                                     // around the device work of the last call of this file (svr_region_growcut_last_ms)

} // namespace

extern "C" {

int svr_region_growcut_params_default(svr_growcut_params* p, int connectivity)
{
    const char* who = "svr_region_growcut_params_default";
    if (!p) return failf(-4, "%s: null argument", who);
    if (int e = check_connectivity(who, "connectivity", connectivity)) return e;
    memset(p, 0, sizeof *p);
    for (int c = 0; c < classes_of(connectivity); ++c) p->step_weights[c] = 1u;
    p->contrast_gain = 1u;
    return 0;
}

int svr_region_growcut(const uint16_t* voxels, const int32_t dims[3], int src_is_device, const uint32_t* marker_labels_device,
                       const uint32_t* domain_mask_device_or_null, const svr_growcut_params* params, uint32_t* cost_device_or_null,
                       uint32_t* zones_device_or_null, svr_growcut_info* info_or_null)
{
    const char* who = "svr_region_growcut";
    if (!voxels || !dims || !marker_labels_device || !params) return failf(-4, "%s: null argument", who);
    if (!cost_device_or_null && !zones_device_or_null) return failf(-4, "%s: both outputs are null", who);
    if (int e = check_dims3(who, dims)) return e;
    GrowCost gc;
    if (int e = check_params(who, params, &gc)) return e;
    const RegionDims d = make_dims(dims[0], dims[1], dims[2]);
    const size_t n = (size_t)d.nx * d.ny * d.nz, words = mask_words(d);
    const size_t map_bytes = n * sizeof(uint32_t), mask_bytes = words * sizeof(uint32_t);
    uint32_t* const outs[2] = {cost_device_or_null, zones_device_or_null};
    for (int i = 0; i < 2; ++i) {
        if (!outs[i]) continue;
        const bool alias = i == 1 && outs[i] == marker_labels_device;                 // zones in place over the markers
        if ((domain_mask_device_or_null && overlap(outs[i], map_bytes, domain_mask_device_or_null, mask_bytes)) ||
            (src_is_device && overlap(outs[i], map_bytes, voxels, n * sizeof(uint16_t))) ||
            (!alias && overlap(outs[i], map_bytes, marker_labels_device, map_bytes)))
            return failf(-3, "%s: an output must not overlap an input (only zones may be the marker labels themselves)", who);
    }
    if (outs[0] && outs[1] && overlap(outs[0], map_bytes, outs[1], map_bytes)) return failf(-3, "%s: the two outputs must not overlap", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const int nty = (d.ny + GY - 1) / GY, ntz = (d.nz + GZ - 1) / GZ;
    const size_t tiles = (size_t)d.wx * nty * ntz;
    const uint32_t cap = params->max_sweeps ? params->max_sweeps : svr_region_geodesic_default_max_sweeps(d.nx, d.ny, d.nz);
    DeviceVoxels vox;                                    // a host source is uploaded once
    SVR_HIP_TRY(vox.get(voxels, n, src_is_device, st));
    DeviceBuffer buf;                                    // the keys, then the two dirty maps, the batch counters and the two counts
    const size_t small = 2 * tiles + SVR_REGION_BATCH + 2;
    SVR_HIP_TRY(buf.alloc(n * sizeof(uint64_t) + small * sizeof(uint32_t)));
    uint64_t* const keys = buf.as<uint64_t>();
    uint32_t* const dirty = (uint32_t*)(keys + n);
    uint32_t* const added = dirty + 2 * tiles;
    uint32_t* const counts = added + SVR_REGION_BATCH;
    CallTimer timer(g_events, st);                       // (the launches, not the allocation or the upload)
    SVR_HIP_TRY(hipMemsetAsync(dirty, 0, small * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_gc_init, lane_grid(words), dim3(LANE_THREADS), 0, st, marker_labels_device, domain_mask_device_or_null, d, words, nty, keys, dirty);
    SVR_HIP_TRY(hipGetLastError());
    uint32_t sweeps = 0u;
    bool done = false;
    SVR_HIP_TRY(sweep_to_fixpoint(st, tiles, dirty, added, cap, &sweeps, &done, [&](uint32_t* cur, uint32_t* next, uint32_t* add) {
        hipLaunchKernelGGL(k_gc_relax, dim3((uint32_t)tiles), dim3(GC_THREADS), 0, st, keys, vox.p, domain_mask_device_or_null, d, gc, nty, ntz, cur, next, add);
    }));
    hipLaunchKernelGGL(k_gc_finish, lane_grid(words), dim3(LANE_THREADS), 0, st, keys, domain_mask_device_or_null, d, words, cost_device_or_null,
                       zones_device_or_null, counts);
    SVR_HIP_TRY(hipGetLastError());
    timer.stop();
    uint32_t counts_host[2] = {0u, 0u};
    SVR_HIP_TRY(hipMemcpyAsync(counts_host, counts, sizeof counts_host, hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));               // (buf and an upload are freed on return)
    if (info_or_null) {
        info_or_null->sweeps = sweeps;
        info_or_null->unreached = counts_host[0];
        info_or_null->saturated = counts_host[1];
    }
    if (!done) return failf(SVR_REGION_ERR_SWEEPS, "%s: keys were still falling after %u sweeps; the outputs are upper bounds, not the map", who, sweeps);
    if (counts_host[1])
        return failf(SVR_REGION_ERR_RANGE, "%s: the cost of %u voxels reached the cap 0x%X: raise contrast_shift or lower contrast_gain (the outputs hold "
                     "the saturated solution)", who, counts_host[1], SVR_GROWCUT_CAP);
    return 0;
}

int svr_region_seed_classes(const int32_t* seeds_xyz, const uint32_t* classes, uint32_t nseeds, const int32_t dims[3], uint32_t* labels_device)
{
    const char* who = "svr_region_seed_classes";
    if (!seeds_xyz || !classes || !dims || !labels_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, dims)) return e;
    const int nx = dims[0], ny = dims[1], nz = dims[2];
    if (int e = check_seeds(who, seeds_xyz, nseeds, nx, ny, nz)) return e;
    ClassSeeds seeds;
    memset(&seeds, 0, sizeof seeds);
    seeds.n = nseeds;
    uint32_t at[SVR_REGION_MAX_SEEDS];
    for (uint32_t i = 0; i < nseeds; ++i) {
        if (classes[i] == 0u) return failf(-3, "%s: seed %u has class 0 (classes are non-zero)", who, i);
        const int32_t x = seeds_xyz[3u * i], y = seeds_xyz[3u * i + 1u], z = seeds_xyz[3u * i + 2u];
        at[i] = (uint32_t)(((size_t)z * ny + y) * nx + x);                // below 2^31
        seeds.at[i] = at[i];
        seeds.cls[i] = classes[i];
        for (uint32_t j = 0; j < i; ++j)
            if (at[j] == at[i]) seeds.at[i] = 0xFFFFFFFFu;                // the lowest seed on a voxel wins
    }
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(hipMemsetAsync(labels_device, 0, (size_t)nx * ny * nz * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_gc_seeds, dim3(1), dim3(SVR_REGION_MAX_SEEDS), 0, st, seeds, labels_device);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_region_label_paint(uint32_t* labels_device, const int32_t dims[3], const uint32_t* mask_device, uint32_t label, int only_unlabelled)
{
    const char* who = "svr_region_label_paint";
    if (!labels_device || !dims || !mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, dims)) return e;
    if (label == 0u) return failf(-3, "%s: the label must be non-zero", who);
    const RegionDims d = make_dims(dims[0], dims[1], dims[2]);
    const size_t words = mask_words(d);
    if (overlap(labels_device, (size_t)d.nx * d.ny * d.nz * sizeof(uint32_t), mask_device, words * sizeof(uint32_t)))
        return failf(-3, "%s: the labels must not overlap the mask", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    hipLaunchKernelGGL(k_gc_paint, lane_grid(words), dim3(LANE_THREADS), 0, st, labels_device, mask_device, d, words, label, only_unlabelled);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_region_growcut_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_region_growcut_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

} // extern "C"
