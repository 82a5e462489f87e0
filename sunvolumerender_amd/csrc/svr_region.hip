// svr_region.hip -- seeded region growing on a plain u16 volume, the statistics of a region and the "keep / remove" copy of the volume
// (svr_region_*; the contract is in include/svr_abi.h, the design in DESIGN.md 8h).  Integers only: a region is a bit mask in the
// layout of svr_mask.hpp, and every result is compared exactly.  The host scaffolding is svr_volume_host.hpp's.
//
// CLASSIFY (k_region_classify): one read of the volume writes the candidate mask (window and box) and zeroes the region mask; a lane
//   reads V voxels of a row (V = 8: one 16-byte load, when nx % 8 == 0 and the rows are 16-byte aligned; else V = 1) and the lanes of a
//   word OR their bits together (a wave64 ballot for V = 1, two xor shuffles for V = 8).  k_region_seed then sets the seeds that are
//   candidates and marks the 27 tiles around every seed dirty.
// GROW (k_region_grow<CONN> and the sweep loop, in svr_region_grow.hpp: svr_morph.hip runs the same code): tiles of TWX x TY x TZ = 4 words x 8 rows x 8 slices (128 x 8 x 8 voxels), one 256-thread block per tile,
//   one thread per word.  The block copies the region words of the tile and of a one-word / one-row halo into LDS (2.4 KB), keeps its
//   candidate word in a register and iterates: new = fill(r | (neighbours & c), c), where `neighbours` ORs the words of the 3 x 3 rows
//   around it that the connectivity admits -- shifted by one bit to either side, across the word boundary, where a step in x is part of
//   the move -- and fill() extends the bits along the runs of c (a Kogge-Stone fill, 5 steps each way).  The loop ends at the first
//   iteration in which no thread changed its word (__syncthreads_or); the block then ORs its new bits into the region mask with atomics,
//   counts itself in `added` if it had any, and marks dirty -- for the NEXT sweep -- the neighbour tiles that can see the boundary layers
//   in which it gained a bit (faces; with 18 also edges; with 26 also corners).  A sweep is one launch over all tiles in which a block
//   whose tile is not dirty returns at once; the host launches sweeps until one adds nothing.
//
//   No block waits for another: there is no flag to spin on and no barrier wider than the block, so a mistake costs a wrong mask and
//   never a hang.  Bits are only ever set.  TERMINATION: claim -- at the start of every sweep, each tile that is NOT dirty is at its
//   local fixpoint with respect to the mask as it stands (own words and halo).  A tile that ran in sweep j ended at a fixpoint of the
//   halo it READ; a halo bit it could have missed was set by a neighbour during sweep j or later, i.e. it is a gain in that neighbour's
//   boundary layer, and every such gain marks this tile dirty for the sweep after it.  Tiles that never ran hold no bit and see no bit
//   (the seed kernel marks the whole 27-neighbourhood of a seed).  So if a sweep adds nothing, the tiles it ran are at their fixpoints
//   by construction, the others by the claim, no tile is marked for the next sweep, and the mask is the global fixpoint: the least one
//   above the seeds, because a bit is only set next to a set bit inside the candidates.  Stale halo reads only delay a voxel a sweep.
//
//   The host reads `added` after a batch of SVR_REGION_BATCH sweeps (one counter per sweep of the batch): the sweeps after the
//   fixpoint find no dirty tile and cost a launch of blocks that return at once, which is less than a stream synchronisation per sweep.
//   `sweeps` reports the launches, surplus included.  The number of sweeps is capped (svr_region_params.max_sweeps; the default is
//   derived in svr_abi.h); at the cap the call returns SVR_REGION_ERR_SWEEPS.
// STATS (k_region_stats): one pass over mask and volume; a wave skips 64 V voxels whose mask words are 0.  Face counts come from the
//   mask words of the six neighbours; lanes keep 64-bit sums, a wave reduces by shuffles, a block through LDS, and one thread issues one
//   set of 64-bit atomics per block, spread over 64 accumulators that the host adds up.
// APPLY (k_region_apply): one streaming pass, a lane reads and writes its own V voxels (so `out` may alias the volume).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"

#include "svr_region_grow.hpp"      // k_region_grow<CONN>, its tiles and the sweep loop (shared with svr_morph.hip); svr_mask.hpp
#include "svr_volume_host.hpp"      // the argument checks, DeviceBuffer / DeviceVoxels, SVR_HIP_TRY

using svr::failf;

namespace {

constexpr int THREADS = 256;
constexpr int ACC_SLOTS = 64;                           // k_region_stats spreads its atomics over this many accumulators

struct RegionBox { int x0, y0, z0, x1, y1, z1; };        // inclusive
struct RegionSeeds { int n; int xyz[SVR_REGION_MAX_SEEDS][3]; };
struct RegionAcc {                                       // device accumulators of k_region_stats
    unsigned long long u[9];                             // voxels, sum, sum_sq, sum_x, sum_y, sum_z, faces_x, faces_y, faces_z
    uint32_t vmin, vmax;
    int32_t bmin[3], bmax[3];
};

// the V voxels of a lane: x .. x + V - 1 of row `row`
template <int V>
__device__ inline void load_voxels(const uint16_t* vox, size_t at, uint32_t v[V])
{
    if (V == 8) {
        const uint4 q = *reinterpret_cast<const uint4*>(vox + at);
        v[0] = q.x & 0xffffu; v[1] = q.x >> 16; v[2] = q.y & 0xffffu; v[3] = q.y >> 16;
        v[4] = q.z & 0xffffu; v[5] = q.z >> 16; v[6] = q.w & 0xffffu; v[7] = q.w >> 16;
    } else {
        v[0] = vox[at];
    }
}

// a wave walks the spans (64 V voxels of one row) of the volume; tasks = rows * spans
__device__ inline unsigned long long span_first() { return (unsigned long long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); }
__device__ inline unsigned long long span_stride() { return (unsigned long long)gridDim.x * (THREADS / 64); }

template <int V>
__global__ __launch_bounds__(THREADS) void k_region_classify(const uint16_t* __restrict__ vox, RegionDims d, uint32_t lo, uint32_t hi, RegionBox b,
                                                             uint32_t* __restrict__ cand, uint32_t* __restrict__ region)
{
    const int lane = threadIdx.x & 63;
    const int spans = (d.nx + 64 * V - 1) / (64 * V);
    const unsigned long long tasks = (unsigned long long)d.ny * d.nz * spans;
    for (unsigned long long task = span_first(); task < tasks; task += span_stride()) {
        const size_t row = (size_t)(task / spans);
        const int span = (int)(task % spans);
        const int y = (int)(row % d.ny), z = (int)(row / d.ny);
        const int x = span * 64 * V + lane * V;
        uint32_t bits = 0;
        if (y >= b.y0 && y <= b.y1 && z >= b.z0 && z <= b.z1 && x < d.nx) {          // (rows outside the box are not read)
            uint32_t v[V];
            load_voxels<V>(vox, row * d.nx + x, v);
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (v[j] >= lo && v[j] <= hi && x + j >= b.x0 && x + j <= b.x1) bits |= 1u << j;
        }
        if (V == 1) {
            const unsigned long long m = __ballot(bits != 0u);
            if ((lane & 31) == 0 && (x >> 5) < d.wx) {
                const size_t w = row * d.wx + (x >> 5);
                cand[w] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
                region[w] = 0u;
            }
        } else {
            uint32_t w = bits << ((lane & 3) * 8);
            w |= __shfl_xor(w, 1);
            w |= __shfl_xor(w, 2);
            if ((lane & 3) == 0 && x < d.nx) {
                const size_t at = row * d.wx + (x >> 5);
                cand[at] = w;
                region[at] = 0u;
            }
        }
    }
}

// sets the seeds that are candidates; marks the 27 tiles around every seed dirty for the first sweep
__global__ void k_region_seed(RegionSeeds s, RegionDims d, int ntx, int nty, int ntz, const uint32_t* __restrict__ cand, uint32_t* region,
                              uint32_t* dirty)
{
    const int i = threadIdx.x;
    if (i >= s.n) return;
    const int x = s.xyz[i][0], y = s.xyz[i][1], z = s.xyz[i][2];
    const size_t w = ((size_t)z * d.ny + y) * d.wx + (x >> 5);
    const uint32_t bit = 1u << (x & 31);
    if (!(cand[w] & bit)) return;
    atomicOr(&region[w], bit);
    const int tx = (x >> 5) / TWX, ty = y / TY, tz = z / TZ;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int ax = tx + dx, ay = ty + dy, az = tz + dz;
                if (ax >= 0 && ax < ntx && ay >= 0 && ay < nty && az >= 0 && az < ntz) dirty[((size_t)az * nty + ay) * ntx + ax] = 1u;
            }
}

__device__ inline unsigned long long wave_sum(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline int wave_min(int v) { for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ inline int wave_max(int v) { for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }

template <int V>
__global__ __launch_bounds__(THREADS) void k_region_stats(const uint16_t* __restrict__ vox, const uint32_t* __restrict__ mask, RegionDims d, RegionAcc* acc)
{
    const int lane = threadIdx.x & 63;
    const int spans = (d.nx + 64 * V - 1) / (64 * V);
    const unsigned long long tasks = (unsigned long long)d.ny * d.nz * spans;
    constexpr uint32_t VM = (1u << V) - 1u;
    unsigned long long u[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int vmin = 65535, vmax = 0;
    int bmin[3] = {d.nx, d.ny, d.nz}, bmax[3] = {-1, -1, -1};
    for (unsigned long long task = span_first(); task < tasks; task += span_stride()) {
        const size_t row = (size_t)(task / spans);
        const int span = (int)(task % spans);
        const int y = (int)(row % d.ny), z = (int)(row / d.ny);
        const int x = span * 64 * V + lane * V;
        const int wi = x >> 5, sh = x & 31;
        const size_t at = row * d.wx + wi;
        const uint32_t wc = x < d.nx ? mask[at] : 0u;
        const uint32_t bits = (wc >> sh) & VM;
        if (!bits) continue;                             // (a span without a bit costs its mask words only)
        const uint32_t left = sh > 0 ? (wc >> (sh - 1)) & 1u : x > 0 ? mask[at - 1] >> 31 : 0u;
        const uint32_t right = sh + V < 32 ? (wc >> (sh + V)) & 1u : wi + 1 < d.wx ? mask[at + 1] & 1u : 0u;
        const uint32_t ext = (bits << 1) | left | (right << (V + 1));               // bit j + 1 = voxel j of the lane
        const uint32_t ym = y > 0 ? (mask[at - d.wx] >> sh) & VM : 0u;
        const uint32_t yp = y + 1 < d.ny ? (mask[at + d.wx] >> sh) & VM : 0u;
        const uint32_t zm = z > 0 ? (mask[at - (size_t)d.wx * d.ny] >> sh) & VM : 0u;
        const uint32_t zp = z + 1 < d.nz ? (mask[at + (size_t)d.wx * d.ny] >> sh) & VM : 0u;
        const uint32_t cnt = __popc(bits);
        u[0] += cnt;
        u[4] += (unsigned long long)cnt * (uint32_t)y;
        u[5] += (unsigned long long)cnt * (uint32_t)z;
        u[6] += __popc(bits & ~ext) + __popc(bits & ~(ext >> 2));
        u[7] += __popc(bits & ~ym) + __popc(bits & ~yp);
        u[8] += __popc(bits & ~zm) + __popc(bits & ~zp);
        uint32_t v[V];
        load_voxels<V>(vox, row * d.nx + x, v);
#pragma unroll
        for (int j = 0; j < V; ++j)
            if ((bits >> j) & 1u) {
                u[1] += v[j];
                u[2] += (unsigned long long)v[j] * v[j];
                u[3] += (uint32_t)(x + j);
                vmin = min(vmin, (int)v[j]);
                vmax = max(vmax, (int)v[j]);
            }
        bmin[0] = min(bmin[0], x + (__ffs(bits) - 1)); bmax[0] = max(bmax[0], x + 31 - __clz(bits));
        bmin[1] = min(bmin[1], y); bmax[1] = max(bmax[1], y);
        bmin[2] = min(bmin[2], z); bmax[2] = max(bmax[2], z);
    }
    __shared__ RegionAcc part[THREADS / 64];
    const int wave = threadIdx.x >> 6;
    for (int i = 0; i < 9; ++i) { const unsigned long long s = wave_sum(u[i]); if (lane == 0) part[wave].u[i] = s; }
    vmin = wave_min(vmin); vmax = wave_max(vmax);
    for (int a = 0; a < 3; ++a) { bmin[a] = wave_min(bmin[a]); bmax[a] = wave_max(bmax[a]); }
    if (lane == 0) {
        part[wave].vmin = (uint32_t)vmin; part[wave].vmax = (uint32_t)vmax;
        for (int a = 0; a < 3; ++a) { part[wave].bmin[a] = bmin[a]; part[wave].bmax[a] = bmax[a]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        RegionAcc t = part[0];
        for (int w = 1; w < THREADS / 64; ++w) {
            for (int i = 0; i < 9; ++i) t.u[i] += part[w].u[i];
            t.vmin = min(t.vmin, part[w].vmin); t.vmax = max(t.vmax, part[w].vmax);
            for (int a = 0; a < 3; ++a) { t.bmin[a] = min(t.bmin[a], part[w].bmin[a]); t.bmax[a] = max(t.bmax[a], part[w].bmax[a]); }
        }
        if (t.u[0]) {
            acc += blockIdx.x % ACC_SLOTS;               // (2048 blocks on one address serialise: 64 slots, summed on the host)
            for (int i = 0; i < 9; ++i) atomicAdd(&acc->u[i], t.u[i]);
            atomicMin(&acc->vmin, t.vmin); atomicMax(&acc->vmax, t.vmax);
            for (int a = 0; a < 3; ++a) { atomicMin(&acc->bmin[a], t.bmin[a]); atomicMax(&acc->bmax[a], t.bmax[a]); }
        }
    }
}

template <int V>
__global__ __launch_bounds__(THREADS) void k_region_apply(const uint16_t* vox, const uint32_t* __restrict__ mask, RegionDims d, uint32_t keep_inside,
                                                          uint32_t fill, uint16_t* out)
{
    const int lane = threadIdx.x & 63;
    const int spans = (d.nx + 64 * V - 1) / (64 * V);
    const unsigned long long tasks = (unsigned long long)d.ny * d.nz * spans;
    for (unsigned long long task = span_first(); task < tasks; task += span_stride()) {
        const size_t row = (size_t)(task / spans);
        const int span = (int)(task % spans);
        const int x = span * 64 * V + lane * V;
        if (x >= d.nx) continue;
        const uint32_t bits = mask[row * d.wx + (x >> 5)] >> (x & 31);
        uint32_t v[V];
        load_voxels<V>(vox, row * d.nx + x, v);                                     // (read before the store: out may alias vox)
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (((bits >> j) & 1u) != keep_inside) v[j] = fill;
        if (V == 8) {
            uint4 q;
            q.x = v[0] | (v[1] << 16); q.y = v[2] | (v[3] << 16); q.z = v[4] | (v[5] << 16); q.w = v[6] | (v[7] << 16);
            *reinterpret_cast<uint4*>(out + row * d.nx + x) = q;
        } else {
            out[row * d.nx + x] = (uint16_t)v[0];
        }
    }
}

// ---------------- host side ----------------
float g_ms[3] = {0.f, 0.f, 0.f};                         // classify (with the seeds), grow, stats of the last svr_region_grow

int span_blocks(const RegionDims& d, int V)
{
    const unsigned long long tasks = (unsigned long long)d.ny * d.nz * ((d.nx + 64 * V - 1) / (64 * V));
    const unsigned long long want = (tasks + THREADS / 64 - 1) / (THREADS / 64);
    return (int)(want < 2048ull ? want : 2048ull);       // 256 CUs x 8 blocks; the waves stride over the rest
}

bool vec8_ok(const RegionDims& d, const void* a, const void* b = nullptr)
{
    return d.nx % 8 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0;
}

hipError_t launch_stats(const uint16_t* vox, const uint32_t* mask, const RegionDims& d, RegionAcc* d_acc, hipStream_t st)
{
    RegionAcc init;
    memset(&init, 0, sizeof init);
    init.vmin = 65535u; init.vmax = 0u;
    init.bmin[0] = d.nx; init.bmin[1] = d.ny; init.bmin[2] = d.nz;
    init.bmax[0] = init.bmax[1] = init.bmax[2] = -1;
    static RegionAcc inits[ACC_SLOTS];                   // (static: the copy is asynchronous)
    for (RegionAcc& a : inits) a = init;
    hipError_t e = hipMemcpyAsync(d_acc, inits, sizeof inits, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    if (vec8_ok(d, vox)) hipLaunchKernelGGL((k_region_stats<8>), dim3(span_blocks(d, 8)), dim3(THREADS), 0, st, vox, mask, d, d_acc);
    else hipLaunchKernelGGL((k_region_stats<1>), dim3(span_blocks(d, 1)), dim3(THREADS), 0, st, vox, mask, d, d_acc);
    return hipGetLastError();
}

void stats_from(const RegionAcc* slots, svr_region_stats* s)
{
    RegionAcc a = slots[0];
    for (int k = 1; k < ACC_SLOTS; ++k) {
        for (int i = 0; i < 9; ++i) a.u[i] += slots[k].u[i];
        a.vmin = slots[k].vmin < a.vmin ? slots[k].vmin : a.vmin; a.vmax = slots[k].vmax > a.vmax ? slots[k].vmax : a.vmax;
        for (int i = 0; i < 3; ++i) {
            a.bmin[i] = slots[k].bmin[i] < a.bmin[i] ? slots[k].bmin[i] : a.bmin[i];
            a.bmax[i] = slots[k].bmax[i] > a.bmax[i] ? slots[k].bmax[i] : a.bmax[i];
        }
    }
    s->voxels = a.u[0]; s->sum = a.u[1]; s->sum_sq = a.u[2]; s->sum_x = a.u[3]; s->sum_y = a.u[4]; s->sum_z = a.u[5];
    s->faces_x = a.u[6]; s->faces_y = a.u[7]; s->faces_z = a.u[8];
    s->vmin = a.vmin; s->vmax = a.vmax;
    for (int i = 0; i < 3; ++i) { s->bbox_min[i] = a.bmin[i]; s->bbox_max[i] = a.bmax[i]; }
    s->status = a.u[0] ? SVR_REGION_STATUS_OK : SVR_REGION_STATUS_EMPTY;
}

} // namespace

extern "C" {

int svr_region_params_default(svr_region_params* p)
{
    if (!p) return failf(-4, "svr_region_params_default: null argument");
    p->lo = 0u; p->hi = 65535u;
    p->connectivity = 6;
    for (int a = 0; a < 3; ++a) { p->box_min[a] = 0; p->box_max[a] = INT32_MAX; }
    p->max_sweeps = 0u;
    return 0;
}

uint64_t svr_region_mask_words(int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0u;
    return (uint64_t)((nx + 31) / 32) * (uint64_t)ny * (uint64_t)nz;
}

uint32_t svr_region_default_max_sweeps(int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0u;
    const uint64_t tiles = (uint64_t)(((nx + 31) / 32 + TWX - 1) / TWX) * (uint64_t)((ny + TY - 1) / TY) * (uint64_t)((nz + TZ - 1) / TZ);
    const uint64_t cap = 64u + 2u * tiles;
    return (uint32_t)(cap < 65536u ? cap : 65536u);
}

int svr_region_grow(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, const int32_t* seeds_xyz, uint32_t nseeds,
                    const svr_region_params* params, uint32_t* mask_device, svr_region_stats* stats_host)
{
    const char* who = "svr_region_grow";
    if (!voxels || !seeds_xyz || !params || !mask_device || !stats_host) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (params->lo > params->hi || params->hi > 65535u) return failf(-3, "%s: the window must satisfy lo <= hi <= 65535 (got %u .. %u)", who, params->lo, params->hi);
    if (int e = check_connectivity(who, "connectivity", (int)params->connectivity)) return e;
    if (int e = check_seeds(who, seeds_xyz, nseeds, nx, ny, nz)) return e;
    RegionSeeds seeds;
    memset(&seeds, 0, sizeof seeds);
    seeds.n = (int)nseeds;
    for (uint32_t i = 0; i < nseeds; ++i)
        for (int a = 0; a < 3; ++a) seeds.xyz[i][a] = seeds_xyz[3u * i + a];
    int b0[3], b1[3];
    if (int e = clamp_box(who, params->box_min, params->box_max, nx, ny, nz, b0, b1)) return e;
    const RegionBox box = {b0[0], b0[1], b0[2], b1[0], b1[1], b1[2]};
    const uint32_t cap = params->max_sweeps ? params->max_sweeps : svr_region_default_max_sweeps(nx, ny, nz);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();

    const RegionDims d = make_dims(nx, ny, nz);
    const size_t n = (size_t)nx * ny * nz, words = (size_t)svr_region_mask_words(nx, ny, nz);
    RegionSweep sw(d);
    const int ntx = sw.ntx, nty = sw.nty, ntz = sw.ntz;
    const size_t tiles = sw.tiles;
    DeviceVoxels dv;
    DeviceBuffer cand_buf, dirty_buf, added_buf, acc_buf;
    DeviceEvent ev[4];
    if (tiles > 0x7fffffffull) return failf(-6, "%s: %zu tiles exceed one launch", who, tiles);
    SVR_HIP_TRY(dv.get(voxels, n, src_is_device, st));
    SVR_HIP_TRY(cand_buf.alloc(words * sizeof(uint32_t)));
    SVR_HIP_TRY(dirty_buf.alloc(2 * tiles * sizeof(uint32_t)));
    SVR_HIP_TRY(added_buf.alloc(SVR_REGION_BATCH * sizeof(uint32_t)));
    SVR_HIP_TRY(acc_buf.alloc(ACC_SLOTS * sizeof(RegionAcc)));
    for (DeviceEvent& e : ev) SVR_HIP_TRY(e.create());
    uint32_t *const d_cand = cand_buf.as<uint32_t>(), *const d_dirty = dirty_buf.as<uint32_t>();
    RegionAcc* const d_acc = acc_buf.as<RegionAcc>();

    SVR_HIP_TRY(hipEventRecord(ev[0].e, st));
    SVR_HIP_TRY(hipMemsetAsync(d_dirty, 0, 2 * tiles * sizeof(uint32_t), st));
    if (vec8_ok(d, dv.p))
        hipLaunchKernelGGL((k_region_classify<8>), dim3(span_blocks(d, 8)), dim3(THREADS), 0, st, dv.p, d, params->lo, params->hi, box, d_cand, mask_device);
    else
        hipLaunchKernelGGL((k_region_classify<1>), dim3(span_blocks(d, 1)), dim3(THREADS), 0, st, dv.p, d, params->lo, params->hi, box, d_cand, mask_device);
    SVR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_region_seed, dim3(1), dim3(64), 0, st, seeds, d, ntx, nty, ntz, d_cand, mask_device, d_dirty);
    SVR_HIP_TRY(hipGetLastError());
    SVR_HIP_TRY(hipEventRecord(ev[1].e, st));

    uint32_t sweeps = 0u;
    bool done = false;
    sw.dirty = d_dirty; sw.added = added_buf.as<uint32_t>();
    SVR_HIP_TRY(region_sweep_to_fixpoint(st, (int)params->connectivity, d_cand, mask_device, d, sw, cap, &sweeps, &done));
    SVR_HIP_TRY(hipEventRecord(ev[2].e, st));
    stats_host->sweeps = sweeps;
    if (!done) {
        SVR_HIP_TRY(hipStreamSynchronize(st));           // (the buffers are freed on return)
        return failf(SVR_REGION_ERR_SWEEPS, "%s: the region was still growing after %u sweeps (max_sweeps); the mask is incomplete", who, sweeps);
    }
    SVR_HIP_TRY(launch_stats(dv.p, mask_device, d, d_acc, st));
    SVR_HIP_TRY(hipEventRecord(ev[3].e, st));
    RegionAcc acc[ACC_SLOTS];
    SVR_HIP_TRY(hipMemcpyAsync(acc, d_acc, sizeof acc, hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) SVR_HIP_TRY(hipEventElapsedTime(&g_ms[i], ev[i].e, ev[i + 1].e));
    stats_from(acc, stats_host);
    stats_host->sweeps = sweeps;
    return 0;
}

int svr_region_last_ms(float* classify_ms, float* grow_ms, float* stats_ms)
{
    if (classify_ms) *classify_ms = g_ms[0];
    if (grow_ms) *grow_ms = g_ms[1];
    if (stats_ms) *stats_ms = g_ms[2];
    return 0;
}

int svr_region_stats_of(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, const uint32_t* mask_device, svr_region_stats* stats_host)
{
    const char* who = "svr_region_stats_of";
    if (!voxels || !mask_device || !stats_host) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const RegionDims d = make_dims(nx, ny, nz);
    DeviceVoxels dv;
    DeviceBuffer acc_buf;
    SVR_HIP_TRY(dv.get(voxels, (size_t)nx * ny * nz, src_is_device, st));
    SVR_HIP_TRY(acc_buf.alloc(ACC_SLOTS * sizeof(RegionAcc)));
    SVR_HIP_TRY(launch_stats(dv.p, mask_device, d, acc_buf.as<RegionAcc>(), st));
    RegionAcc acc[ACC_SLOTS];
    SVR_HIP_TRY(hipMemcpyAsync(acc, acc_buf.p, sizeof acc, hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));
    stats_from(acc, stats_host);
    stats_host->sweeps = 0u;
    return 0;
}

int svr_region_apply(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, const uint32_t* mask_device, int mode, uint32_t fill,
                     uint16_t* out_u16_device)
{
    const char* who = "svr_region_apply";
    if (!voxels || !mask_device || !out_u16_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (mode != SVR_REGION_KEEP && mode != SVR_REGION_REMOVE) return failf(-3, "%s: unknown mode %d", who, mode);
    if (fill > 65535u) return failf(-3, "%s: fill must be <= 65535 (got %u)", who, fill);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const RegionDims d = make_dims(nx, ny, nz);
    DeviceVoxels dv;
    SVR_HIP_TRY(dv.get(voxels, (size_t)nx * ny * nz, src_is_device, st));
    const uint32_t keep_inside = mode == SVR_REGION_KEEP ? 1u : 0u;
    if (vec8_ok(d, dv.p, out_u16_device))
        hipLaunchKernelGGL((k_region_apply<8>), dim3(span_blocks(d, 8)), dim3(THREADS), 0, st, dv.p, mask_device, d, keep_inside, fill, out_u16_device);
    else
        hipLaunchKernelGGL((k_region_apply<1>), dim3(span_blocks(d, 1)), dim3(THREADS), 0, st, dv.p, mask_device, d, keep_inside, fill, out_u16_device);
    SVR_HIP_TRY(hipGetLastError());
    if (dv.owned()) SVR_HIP_TRY(hipStreamSynchronize(st));   // the upload is freed on return
    return 0;
}

int svr_region_seed_from_world(const svr_volume* volume, int nx, int ny, int nz, const svr_vec3* point, int32_t ijk[3])
{
    const char* who = "svr_region_seed_from_world";
    if (!volume || !point || !ijk) return failf(-4, "%s: null argument", who);
    if (nx <= 0 || ny <= 0 || nz <= 0) return failf(-6, "%s: bad dimensions %d x %d x %d", who, nx, ny, nz);
    // the sampler's texture coordinate, float32: (p - bbox.vmin) * bbox.invSize; texel i is centred at (i + 0.5) / n
    const float tc[3] = {(point->x - volume->bbox.vmin.x) * volume->bbox.invSize.x, (point->y - volume->bbox.vmin.y) * volume->bbox.invSize.y,
                         (point->z - volume->bbox.vmin.z) * volume->bbox.invSize.z};
    const int dims[3] = {nx, ny, nz};
    int32_t out[3];
    for (int a = 0; a < 3; ++a) {
        if (!(tc[a] >= 0.f && tc[a] <= 1.f))
            return failf(-3, "%s: the point (%g, %g, %g) lies outside the volume's box", who, (double)point->x, (double)point->y, (double)point->z);
        const int i = (int)std::floor((double)tc[a] * (double)dims[a]);               // exact: 24 x 31 bits
        out[a] = i >= dims[a] ? dims[a] - 1 : i;                                      // the far face belongs to the last voxel
    }
    for (int a = 0; a < 3; ++a) ijk[a] = out[a];
    return 0;
}

int svr_region_measure(const svr_region_stats* s, const double spacing[3], svr_region_measurement* out)
{
    const char* who = "svr_region_measure";
    if (!s || !spacing || !out) return failf(-4, "%s: null argument", who);
    for (int a = 0; a < 3; ++a) if (!(spacing[a] > 0.0) || !std::isfinite(spacing[a])) return failf(-3, "%s: the spacing must be positive and finite", who);
    memset(out, 0, sizeof *out);
    const double sx = spacing[0], sy = spacing[1], sz = spacing[2];
    out->surface_area = (double)s->faces_x * sy * sz + (double)s->faces_y * sx * sz + (double)s->faces_z * sx * sy;
    if (s->voxels == 0u) return 0;
    const double n = (double)s->voxels;
    out->volume = n * sx * sy * sz;
    out->mean = (double)s->sum / n;
    // n * sum_sq - sum^2 exactly (128-bit integers), then one conversion: no cancellation of rounded terms
    const unsigned __int128 num = (unsigned __int128)s->voxels * s->sum_sq - (unsigned __int128)s->sum * s->sum;
    out->stddev = std::sqrt((double)num) / n;
    out->centroid[0] = (double)s->sum_x / n; out->centroid[1] = (double)s->sum_y / n; out->centroid[2] = (double)s->sum_z / n;
    return 0;
}

} // extern "C"
