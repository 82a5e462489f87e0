// svr_region_grow.hpp -- the grow kernel of the region calls and the host loop that sweeps it to the fixpoint, shared by
// svr_region.hip (svr_region_grow: candidates from a window, seeds from a list) and svr_morph.hip (svr_region_reconstruct: candidates
// and seeds from masks).  The kernel, its tiles and the termination argument are described at the head of svr_region.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "svr_mask.hpp"        // RegionDims: the mask layout
#include "svr_sweep.hpp"

namespace {

constexpr int TWX = 4, TY = 8, TZ = 8;                  // tile: words in x, rows, slices
constexpr int GROW_THREADS = TWX * TY * TZ;             // one thread per word
static_assert(GROW_THREADS == 256, "the halo load and the 27 marker threads assume 256 threads");

// the bits of g extended along the runs of p, both ways (g is a subset of p)
__device__ inline uint32_t fill_runs(uint32_t g, uint32_t p)
{
    uint32_t a = g, q = p;
    a |= q & (a << 1); q &= q << 1;
    a |= q & (a << 2); q &= q << 2;
    a |= q & (a << 4); q &= q << 4;
    a |= q & (a << 8); q &= q << 8;
    a |= q & (a << 16);
    q = p;
    a |= q & (a >> 1); q &= q >> 1;
    a |= q & (a >> 2); q &= q >> 2;
    a |= q & (a >> 4); q &= q >> 4;
    a |= q & (a >> 8); q &= q >> 8;
    a |= q & (a >> 16);
    return a;
}

template <int CONN>
__global__ __launch_bounds__(GROW_THREADS) void k_region_grow(const uint32_t* __restrict__ cand, uint32_t* region, RegionDims d, int ntx, int nty,
                                                              int ntz, uint32_t* dirty_cur, uint32_t* dirty_next, uint32_t* added)
{
    const size_t tile = blockIdx.x;
#ifndef SVR_REGION_ALL_TILES                             // (the A/B build of tools/region_time.py sweeps every tile every pass)
    if (!dirty_cur[tile]) return;
#endif
    __shared__ uint32_t R[TZ + 2][TY + 2][TWX + 2];
    __shared__ uint32_t s_flags;
    const int tid = threadIdx.x;
    const int tx = (int)(tile % ntx), ty = (int)((tile / ntx) % nty), tz = (int)(tile / ((size_t)ntx * nty));
    for (int i = tid; i < (TZ + 2) * (TY + 2) * (TWX + 2); i += GROW_THREADS) {
        const int hx = i % (TWX + 2), hy = (i / (TWX + 2)) % (TY + 2), hz = i / ((TWX + 2) * (TY + 2));
        const int gw = tx * TWX + hx - 1, gy = ty * TY + hy - 1, gz = tz * TZ + hz - 1;
        uint32_t r = 0u;
        if (gw >= 0 && gw < d.wx && gy >= 0 && gy < d.ny && gz >= 0 && gz < d.nz) r = region[((size_t)gz * d.ny + gy) * d.wx + gw];
        R[hz][hy][hx] = r;
    }
    const int lx = tid % TWX, ly = (tid / TWX) % TY, lz = tid / (TWX * TY);
    const int gw = tx * TWX + lx, gy = ty * TY + ly, gz = tz * TZ + lz;
    const bool valid = gw < d.wx && gy < d.ny && gz < d.nz;
    const size_t at = valid ? ((size_t)gz * d.ny + gy) * d.wx + gw : 0;
    const uint32_t c = valid ? cand[at] : 0u;
    if (tid == 0) s_flags = 0u;
    __syncthreads();
    if (tid == 0) dirty_cur[tile] = 0u;                  // (every thread has read the flag: this buffer is the sweep after next's)
    const uint32_t r0 = R[lz + 1][ly + 1][lx + 1];
    uint32_t r = r0;
    for (;;) {
        uint32_t n = 0u;
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int k = (dz != 0) + (dy != 0);                                 // steps of the move besides the one in x
                const bool plain = k == 0 ? false : k == 1 ? true : CONN >= 18;      // (dx = 0; the centre word itself is r)
                const bool shifted = k == 0 ? true : k == 1 ? CONN >= 18 : CONN == 26;   // dx = +-1
                if (!plain && !shifted) continue;
                const uint32_t m = R[lz + 1 + dz][ly + 1 + dy][lx + 1];
                if (plain) n |= m;
                if (shifted) n |= (m << 1) | (m >> 1) | (R[lz + 1 + dz][ly + 1 + dy][lx] >> 31) | (R[lz + 1 + dz][ly + 1 + dy][lx + 2] << 31);
            }
        const uint32_t nr = fill_runs(r | (n & c), c);
        const int changed = nr != r;
        if (changed) { R[lz + 1][ly + 1][lx + 1] = nr; r = nr; }
        if (!__syncthreads_or(changed)) break;
    }
    const uint32_t nb = r & ~r0;
    if (nb) {
        atomicOr(&region[at], nb);
        uint32_t f = 64u;
        if (lx == 0 && (nb & 1u)) f |= 1u;
        if (lx == TWX - 1 && (nb >> 31)) f |= 2u;
        if (ly == 0) f |= 4u;
        if (ly == TY - 1) f |= 8u;
        if (lz == 0) f |= 16u;
        if (lz == TZ - 1) f |= 32u;
        atomicOr(&s_flags, f);
    }
    __syncthreads();
    const uint32_t flags = s_flags;
    if (tid == 0 && (flags & 64u)) atomicAdd(added, 1u);
    if (tid < 27) {
        // the neighbour tile in direction (dx, dy, dz) sees the layers of this tile that lie on all the faces the direction names
        const int dx = tid % 3 - 1, dy = (tid / 3) % 3 - 1, dz = tid / 9 - 1;
        const int k = (dx != 0) + (dy != 0) + (dz != 0);
        if (k == 0 || k > (CONN == 6 ? 1 : CONN == 18 ? 2 : 3)) return;
        const uint32_t need = (dx < 0 ? 1u : dx > 0 ? 2u : 0u) | (dy < 0 ? 4u : dy > 0 ? 8u : 0u) | (dz < 0 ? 16u : dz > 0 ? 32u : 0u);
        const int ax = tx + dx, ay = ty + dy, az = tz + dz;
        if ((flags & need) == need && ax >= 0 && ax < ntx && ay >= 0 && ay < nty && az >= 0 && az < ntz)
            dirty_next[((size_t)az * nty + ay) * ntx + ax] = 1u;
    }
}

// The tiles of a volume and the device words of one run of sweeps: two dirty maps (this sweep's and the next's) and the `added`
// counters of a batch.  The caller zeroes `dirty` (2 * tiles words) and marks dirty[0] for the first sweep.
struct RegionSweep {
    int ntx, nty, ntz;
    size_t tiles;
    uint32_t* dirty;                                     // 2 * tiles words
    uint32_t* added;                                     // SVR_REGION_BATCH words
    RegionSweep(const RegionDims& d)
        : ntx((d.wx + TWX - 1) / TWX), nty((d.ny + TY - 1) / TY), ntz((d.nz + TZ - 1) / TZ), tiles((size_t)ntx * nty * ntz), dirty(nullptr), added(nullptr) {}
};

// Sweeps k_region_grow<connectivity> over `region` inside `cand` until a sweep adds nothing or `cap` sweeps are launched.
inline hipError_t region_sweep_to_fixpoint(hipStream_t st, int connectivity, const uint32_t* cand, uint32_t* region, const RegionDims& d,
                                           const RegionSweep& s, uint32_t cap, uint32_t* sweeps_out, bool* done_out)
{
    return sweep_to_fixpoint(st, s.tiles, s.dirty, s.added, cap, sweeps_out, done_out, [&](uint32_t* cur, uint32_t* next, uint32_t* added) {
        const dim3 g((uint32_t)s.tiles), b(GROW_THREADS);
        if (connectivity == 6) hipLaunchKernelGGL((k_region_grow<6>), g, b, 0, st, cand, region, d, s.ntx, s.nty, s.ntz, cur, next, added);
        else if (connectivity == 18) hipLaunchKernelGGL((k_region_grow<18>), g, b, 0, st, cand, region, d, s.ntx, s.nty, s.ntz, cur, next, added);
        else hipLaunchKernelGGL((k_region_grow<26>), g, b, 0, st, cand, region, d, s.ntx, s.nty, s.ntz, cur, next, added);
    });
}

} // namespace
