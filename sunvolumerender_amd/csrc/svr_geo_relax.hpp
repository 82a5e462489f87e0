// svr_geo_relax.hpp -- the relaxation on packed (cost << 32) | zone keys that svr_geodesic.hip (geodesic distances and influence zones)
// and svr_growcut.hip (grow-from-seeds) share: the classes of a move and their weights, the two cost policies, the kernels, the host
// driver, and the argument handling the two families have in common.  The contracts are in include/svr_abi.h, the design in DESIGN.md
// 8m and 8q.  Integers only, on the mask layout of svr_mask.hpp.
//
// Every voxel has one packed key (cost << 32) | zone in a workspace of 8 bytes per voxel; ~0 = "outside the domain or not reached".  A
// source has (0, label); every other voxel of the domain wants the lexicographic minimum over its allowed neighbours u of
// (cost(u) + cost(u -> v), zone(u)) -- a plain unsigned 64-bit minimum.  Under PlainCost that system has one solution (induction on the
// cost: weights are >= 1), and relaxing voxels in ANY order from ~0 reaches it: a key only falls, every key ever stored is the (cost,
// source label) of a real path, so it never falls below the solution, and a state in which no voxel can fall is the solution.  Under
// ContrastCost the same holds for the minimum over walks: see there.
//   k_geo_init    one lane per voxel: the key from the label and the domain bit (a NULL domain is the whole volume); a source marks
//     dirty every tile that holds it or one of its neighbours.
//   k_relax<Cost> one block per dirty tile of 32 x 8 x 8 voxels (a tile is one mask word wide).  The keys of the tile and of a halo of
//     one voxel go to LDS (34 x 10 x 10 x 8 B = 27200 B: rows of consecutive 8-byte words, which ds_read_b64 serves a half-wave at a
//     time without bank conflicts); a thread owns the column (lx, ly, 0 .. 7) and holds its eight domain bits in a register.  The block
//     relaxes its own voxels in place until an iteration lowers none, stores the voxels that fell, and marks the neighbour tiles that
//     see a face layer with a fallen voxel dirty for the next sweep -- the dirty-map protocol of svr_region_grow.hpp and the host loop
//     of svr_sweep.hpp.  A cost that reads the voxels (Cost::VALUES) has them beside the keys in LDS.
//   k_geo_finish  one lane per voxel: splits the keys into cost and zones, counts the unreached and the capped voxels of the domain.
//   k_geo_seeds   one lane per seed.
// ONE WRITER, WHOLE PAIRS: a key in global memory is written by its tile's block alone, and every access to a key that another thread
//   may write -- halo loads and result stores in global memory, all LDS traffic of the relaxation -- is ONE aligned 64-bit atomic access
//   (relaxed; agent scope in global memory, workgroup scope in LDS), so a reader gets cost and zone from the same write.  A stale key
//   only delays a voxel (its tile is marked dirty by whoever lowers the key later); a torn one could pair a new cost with an old,
//   smaller label and would never be repaired.
// TERMINATION: no lane or block waits for another.  With the halo fixed in LDS, the limit of a tile's relaxation is the minimum over
//   walks inside the tile from a halo or source voxel.  Cutting a cycle out of a walk keeps its source and does not raise its cost
//   (moves cost >= 1; under ContrastCost sat is monotone), so the minimum is attained on a walk that visits no voxel of the tile twice:
//   fewer than GX GY GZ moves.  An iteration relaxes every voxel from values no worse than a Jacobi step would see, so after k
//   iterations every key is at most the minimum over walks of k moves (Bellman-Ford) -- whether a move added cost or, on ContrastCost's
//   saturated plateau, none, where only the label can still fall; that is again one move of a simple walk.  One iteration per voxel of
//   the tile therefore reaches the limit, and the loop is counted against it.
// LDS: the keys of the tile and its halo, and under Cost::VALUES their voxel values as u16 (6800 B): 34000 B a block, four blocks a CU
//   by LDS (five without the values).  A half-wave (one x row of the tile) reads 32 consecutive u16 of a value row: 64 consecutive
//   bytes, 16 or 17 consecutive dwords with two lanes on each, which ds_read_u16 serves in one pass (bank = dword index mod 32; lanes
//   that share a dword are a broadcast).  The value rows need no padding, and being a separate array they leave the 8-byte alignment
//   and the conflict-free rows of the keys as they are.  A thread keeps its own column's eight values packed in two 64-bit registers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"
#include "svr_mask.hpp"             // RegionDims, lane_at, half_ballot, the grids
#include "svr_sweep.hpp"
#include "svr_volume_host.hpp"

namespace {

constexpr int GX = 32, GY = 8, GZ = 8;                   // tile in voxels; GX = one mask word
constexpr int GEO_THREADS = GX * GY;                     // one thread per column of GZ voxels
static_assert(GEO_THREADS == 256 && GX == 32 && GZ == 8, "the lane mapping assumes a tile one mask word wide, 256 threads and columns of 8");
constexpr uint64_t KEY_NONE = ~0ull;
constexpr int LANE_THREADS = MASK_THREADS;               // the one-lane-per-voxel kernels

// w[c]: the weight of move class c (x, y, z, xy, xz, yz, xyz); reach bit c: a tile in a direction of class c can see this tile's keys
struct GeoWeights { uint32_t w[7]; uint32_t reach; };

// the class of a move or direction from the coordinates it changes
__host__ __device__ constexpr int move_class(int dx, int dy, int dz)
{
    const int m = (dx != 0 ? 1 : 0) | (dy != 0 ? 2 : 0) | (dz != 0 ? 4 : 0);
    return m == 1 ? 0 : m == 2 ? 1 : m == 4 ? 2 : m == 3 ? 3 : m == 5 ? 4 : m == 6 ? 5 : 6;
}

// a tile in a direction that changes the coordinates S sees this tile through the moves that change at least S
inline uint32_t geo_reach(const uint32_t w[7])
{
    static const int bits[7] = {1, 2, 4, 3, 5, 6, 7};
    uint32_t reach = 0u;
    for (int dir = 0; dir < 7; ++dir)
        for (int c = 0; c < 7; ++c)
            if (w[c] && (bits[c] & bits[dir]) == bits[dir]) reach |= 1u << dir;
    return reach;
}

__device__ inline uint64_t lds_get(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void lds_put(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline uint64_t key_get(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void key_put(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a NULL mask is the whole volume
__device__ inline bool in_domain(const uint32_t* __restrict__ mask, size_t word, int bit) { return !mask || ((mask[word] >> bit) & 1u); }

// ---------------- the cost policies of k_relax ----------------
// A policy holds the weights, says whether a move reads the voxel values (VALUES) and whether the mask may be NULL, and extends the
// key u of a neighbour by one move of weight w across the value difference `diff`: false if u cannot be relaxed from.

// svr_region_geodesic, svr_region_split: cost(u, v) = w[class].
// NO OVERFLOW: the host refuses wmax (voxels - 1) > 0xFFFFFFFE; a stored key is the cost of a simple path, so key + (w << 32) wraps
//   only for the key ~0, which the comparison `candidate > key` filters out.
struct PlainCost {
    static constexpr bool VALUES = false, NULL_MASK = false;
    GeoWeights gw;
    __device__ bool extend(uint64_t u, uint32_t w, uint32_t, uint64_t* c) const
    {
        *c = u + ((uint64_t)w << 32);
        return *c > u;
    }
};

// svr_region_growcut: cost(u, v) = w[class] + gain * (|I(u) - I(v)| >> shift), I the raw u16 voxel: symmetric, >= 1 on an allowed move
// and, by the host's refusal of wmax + gain * (65535 >> shift) > 0x7FFFFFFF, below 2^31.
// SATURATION: the a-priori bound of PlainCost would refuse every real volume here, so the device adds with saturation: sat(x) =
//   min(x, CAP), CAP = SVR_GROWCUT_CAP = 0xFFFFFFFE, one below the NONE of an unreached voxel.  A stored cost is <= CAP and a move costs
//   < 2^31, so the 64-bit sum is below 2^33 and needs no further check.
//   THE RESULT IS STILL UNIQUE.  Define key*(v) = the lexicographic minimum over all walks inside the domain from a source to v of
//   (sat(cost of the walk), label of its source).  Because sat(sat(a) + w) = sat(a + w), saturating after every move of a walk gives the
//   same number as saturating its sum once.  So, relaxing from "all NONE" in any order: (1) every key ever stored is (sat(cost), label) of
//   a real walk -- by induction over the stores, a candidate being the stored key of a neighbour extended by one move -- hence never below
//   key*; (2) keys only fall and take finitely many values, so the relaxation stops; (3) in a state where no voxel can fall, key(v) <=
//   (sat(cost), label) for every walk to v, by induction over the walk's length (the source holds (0, label) or less; one more move is
//   one more relaxation that cannot lower v).  (1) and (3) give key = key* everywhere.  (The fixpoint EQUATIONS alone have other solutions
//   on the plateau cost = CAP, where voxels could hold up one another's label with no source behind it; they are not reachable from NONE.)
struct ContrastCost {
    static constexpr bool VALUES = true, NULL_MASK = true;
    GeoWeights gw;
    uint32_t gain, shift;
    __device__ bool extend(uint64_t u, uint32_t w, uint32_t diff, uint64_t* c) const
    {
        constexpr uint64_t CAP = SVR_GROWCUT_CAP;
        const uint64_t cost = (uint64_t)(w + gain * (diff >> shift));                    // below 2^31 (the host's refusal)
        const uint64_t du = u >> 32;
        uint64_t s = du + cost;                                                           // below 2^33
        s = s < CAP ? s : CAP;
        *c = (s << 32) | (u & 0xFFFFFFFFull);
        return du != (uint64_t)SVR_GEO_NONE;
    }
};

// ---------------- kernels ----------------
__global__ __launch_bounds__(LANE_THREADS) void k_geo_init(const uint32_t* labels, const uint32_t* __restrict__ mask, RegionDims d, size_t words, int nty,
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

// vox is read only under Cost::VALUES; mask may be NULL only under Cost::NULL_MASK
template <class Cost>
__global__ __launch_bounds__(GEO_THREADS) void k_relax(uint64_t* keys, const uint16_t* __restrict__ vox, const uint32_t* __restrict__ mask, RegionDims d,
                                                       Cost cost, int nty, int ntz, uint32_t* dirty_cur, uint32_t* dirty_next, uint32_t* added)
{
    const size_t tile = blockIdx.x;
    if (!dirty_cur[tile]) return;
    __shared__ uint64_t K[GZ + 2][GY + 2][GX + 2];
    __shared__ uint16_t V[Cost::VALUES ? GZ + 2 : 1][GY + 2][GX + 2];
    __shared__ uint32_t s_flags;
    const int tid = threadIdx.x;
    const int ntx = d.wx;
    const int tx = (int)(tile % ntx), ty = (int)((tile / ntx) % nty), tz = (int)(tile / ((size_t)ntx * nty));
    for (int i = tid; i < (GZ + 2) * (GY + 2) * (GX + 2); i += GEO_THREADS) {
        const int hx = i % (GX + 2), hy = (i / (GX + 2)) % (GY + 2), hz = i / ((GX + 2) * (GY + 2));
        const int gx = tx * GX + hx - 1, gy = ty * GY + hy - 1, gz = tz * GZ + hz - 1;
        uint64_t k = KEY_NONE;
        uint16_t v = 0;                                  // (outside the volume the key is NONE and the value is never used)
        if (gx >= 0 && gx < d.nx && gy >= 0 && gy < d.ny && gz >= 0 && gz < d.nz) {
            const size_t at = ((size_t)gz * d.ny + gy) * d.nx + gx;
            k = key_get(&keys[at]);
            if constexpr (Cost::VALUES) v = vox[at];
        }
        K[hz][hy][hx] = k;
        if constexpr (Cost::VALUES) V[hz][hy][hx] = v;
    }
    const int lx = tid % GX, ly = tid / GX;
    const int gx = tx * GX + lx, gy = ty * GY + ly;
    uint32_t dom = 0u;                                   // bit lz: voxel (lx, ly, lz) of the tile is in the domain
    if (gx < d.nx && gy < d.ny)
        for (int lz = 0; lz < GZ; ++lz) {
            const int gz = tz * GZ + lz;
            if (gz >= d.nz) continue;
            const size_t word = ((size_t)gz * d.ny + gy) * d.wx + tx;
            const bool in = Cost::NULL_MASK ? in_domain(mask, word, lx) : ((mask[word] >> lx) & 1u) != 0u;
            dom |= (in ? 1u : 0u) << lz;
        }
    if (tid == 0) s_flags = 0u;
    __syncthreads();
    if (tid == 0) dirty_cur[tile] = 0u;                  // (every thread has read the flag: this buffer is the sweep after next's)
    uint64_t mine[2] = {0ull, 0ull};                     // the column's own values: lz 0 .. 3 and 4 .. 7, 16 bits each
    if constexpr (Cost::VALUES)
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
                        const uint32_t w = cost.gw.w[move_class(dx, dy, dz)];
                        if (w == 0u) continue;
                        const int off = (dz * (GY + 2) + dy) * (GX + 2) + dx;
                        const uint64_t u = lds_get(own + off);
                        uint32_t diff = 0u;
                        if constexpr (Cost::VALUES) {
                            const int32_t iu = (int32_t)val[off];
                            diff = (uint32_t)(iu > iv ? iu - iv : iv - iu);
                        }
                        uint64_t c;
                        if (cost.extend(u, w, diff, &c) && c < best) best = c;
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
        if ((dx == 0 && dy == 0 && dz == 0) || !((cost.gw.reach >> move_class(dx, dy, dz)) & 1u)) return;
        const uint32_t need = (dx < 0 ? 1u : dx > 0 ? 2u : 0u) | (dy < 0 ? 4u : dy > 0 ? 8u : 0u) | (dz < 0 ? 16u : dz > 0 ? 32u : 0u);
        const int ax = tx + dx, ay = ty + dy, az = tz + dz;
        if ((flags & need) == need && ax >= 0 && ax < ntx && ay >= 0 && ay < nty && az >= 0 && az < ntz)
            dirty_next[((size_t)az * nty + ay) * ntx + ax] = 1u;
    }
}

// counts[0] = the voxels of the domain that no source reaches, counts[1] = those whose cost is SVR_GROWCUT_CAP
__global__ __launch_bounds__(LANE_THREADS) void k_geo_finish(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ mask, RegionDims d, size_t words,
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

// at[i] = the voxel of seed i, or ~0 if a lower seed has it; cls[i] = its label
struct GeoSeeds { uint32_t n; uint32_t at[SVR_REGION_MAX_SEEDS]; uint32_t cls[SVR_REGION_MAX_SEEDS]; };

__global__ void k_geo_seeds(GeoSeeds s, uint32_t* __restrict__ labels)
{
    const uint32_t i = threadIdx.x;
    if (i < s.n && s.at[i] != 0xFFFFFFFFu) labels[s.at[i]] = s.cls[i];
}

// ---------------- host side ----------------
int classes_of(int connectivity) { return connectivity == 6 ? 3 : connectivity == 18 ? 6 : 7; }

// the two outputs of a call against its inputs and each other; a NULL mask or volume is no input on the device
int check_geo_outputs(const char* who, const uint32_t* labels, size_t map_bytes, const uint32_t* mask_or_null, size_t mask_bytes, const uint16_t* vox_or_null,
                      size_t vox_bytes, uint32_t* cost_or_null, uint32_t* zones_or_null)
{
    uint32_t* const outs[2] = {cost_or_null, zones_or_null};
    for (int i = 0; i < 2; ++i) {
        if (!outs[i]) continue;
        const bool alias = i == 1 && outs[i] == labels;                               // zones in place over the labels
        if ((mask_or_null && overlap(outs[i], map_bytes, mask_or_null, mask_bytes)) || (vox_or_null && overlap(outs[i], map_bytes, vox_or_null, vox_bytes)) ||
            (!alias && overlap(outs[i], map_bytes, labels, map_bytes)))
            return svr::failf(-3, "%s: an output must not overlap an input (only zones may be the marker labels themselves)", who);
    }
    if (outs[0] && outs[1] && overlap(outs[0], map_bytes, outs[1], map_bytes)) return svr::failf(-3, "%s: the two outputs must not overlap", who);
    return 0;
}

struct GeoResult { uint32_t sweeps, unreached, capped; };     // the launched sweeps; the counts of k_geo_finish

// The checked core of a call: keys from the labels, sweeps of k_relax<Cost> to the fixpoint or the cap (max_sweeps, 0 = the default of
// the dims), the outputs and *res, which is written when the sweeps ran: on 0 and on SVR_REGION_ERR_SWEEPS, not on a HIP error.  `vox`
// is on the device (PlainCost: NULL).  The time of the launches, not of the allocation, goes to `events`.  Synchronises the stream.
template <class Cost>
int geo_run(const char* who, CallEvents& events, const Cost& cost, const uint16_t* vox, const uint32_t* labels, const uint32_t* mask, const RegionDims& d,
            uint32_t max_sweeps, uint32_t* cost_out, uint32_t* zones_out, GeoResult* res)
{
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const size_t n = (size_t)d.nx * d.ny * d.nz, words = mask_words(d);
    const int nty = (d.ny + GY - 1) / GY, ntz = (d.nz + GZ - 1) / GZ;
    const size_t tiles = (size_t)d.wx * nty * ntz;
    const uint32_t cap = max_sweeps ? max_sweeps : svr_region_geodesic_default_max_sweeps(d.nx, d.ny, d.nz);
    DeviceBuffer buf;                                    // the keys, then the two dirty maps, the batch counters and the two counts
    const size_t small = 2 * tiles + SVR_REGION_BATCH + 2;
    SVR_HIP_TRY(buf.alloc(n * sizeof(uint64_t) + small * sizeof(uint32_t)));
    uint64_t* const keys = buf.as<uint64_t>();
    uint32_t* const dirty = (uint32_t*)(keys + n);
    uint32_t* const added = dirty + 2 * tiles;
    uint32_t* const counts = added + SVR_REGION_BATCH;
    CallTimer timer(events, st);
    SVR_HIP_TRY(hipMemsetAsync(dirty, 0, small * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_geo_init, lane_grid(words), dim3(LANE_THREADS), 0, st, labels, mask, d, words, nty, keys, dirty);
    SVR_HIP_TRY(hipGetLastError());
    uint32_t sweeps = 0u;
    bool done = false;
    SVR_HIP_TRY(sweep_to_fixpoint(st, tiles, dirty, added, cap, &sweeps, &done, [&](uint32_t* cur, uint32_t* next, uint32_t* add) {
        hipLaunchKernelGGL(k_relax<Cost>, dim3((uint32_t)tiles), dim3(GEO_THREADS), 0, st, keys, vox, mask, d, cost, nty, ntz, cur, next, add);
    }));
    hipLaunchKernelGGL(k_geo_finish, lane_grid(words), dim3(LANE_THREADS), 0, st, keys, mask, d, words, cost_out, zones_out, counts);
    SVR_HIP_TRY(hipGetLastError());
    timer.stop();
    uint32_t counts_host[2] = {0u, 0u};
    SVR_HIP_TRY(hipMemcpyAsync(counts_host, counts, sizeof counts_host, hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));               // (buf is freed on return)
    *res = GeoResult{sweeps, counts_host[0], counts_host[1]};
    if (!done) return svr::failf(SVR_REGION_ERR_SWEEPS, "%s: keys were still falling after %u sweeps; the outputs are upper bounds, not the map", who, sweeps);
    return 0;
}

// labels = 0 everywhere but classes_or_null[i] (NULL: i + 1) on the voxel of seed i; the lowest seed on a voxel wins.  The seeds are
// checked (check_seeds) and the classes non-zero.
int place_seeds(const char* who, CallEvents& events, const int32_t* seeds_xyz, const uint32_t* classes_or_null, uint32_t nseeds, int nx, int ny, int nz,
                uint32_t* labels_device)
{
    GeoSeeds seeds;
    memset(&seeds, 0, sizeof seeds);
    seeds.n = nseeds;
    for (uint32_t i = 0; i < nseeds; ++i) {
        const int32_t x = seeds_xyz[3u * i], y = seeds_xyz[3u * i + 1u], z = seeds_xyz[3u * i + 2u];
        const uint32_t at = (uint32_t)(((size_t)z * ny + y) * nx + x);                   // below 2^31
        seeds.at[i] = at;
        seeds.cls[i] = classes_or_null ? classes_or_null[i] : i + 1u;
        for (uint32_t j = 0; j < i; ++j)
            if (seeds.at[j] == at) seeds.at[i] = 0xFFFFFFFFu;                             // the lowest seed on a voxel wins
    }
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(events, st);
    SVR_HIP_TRY(hipMemsetAsync(labels_device, 0, (size_t)nx * ny * nz * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_geo_seeds, dim3(1), dim3(SVR_REGION_MAX_SEEDS), 0, st, seeds, labels_device);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace
