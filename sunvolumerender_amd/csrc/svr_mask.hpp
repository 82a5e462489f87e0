// svr_mask.hpp -- the bit-mask layout of the region calls (svr_region_*; the contract is in include/svr_abi.h, the design in DESIGN.md
// 8h) and the helpers that every file working on it needs: the words of a row, the lanes of a word, the launch grids.  Included by
// svr_region_grow.hpp (svr_region.hip, svr_morph.hip), svr_label.hip, svr_dist_passes.hpp (svr_distance.hip, svr_fillbetween.hip),
// svr_geo_relax.hpp (svr_geodesic.hip, svr_growcut.hip) and svr_resample.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

// THE LAYOUT: a mask of an nx x ny x nz volume is uint32 [nz][ny][wx], wx = ceil(nx / 32) words per row; voxel (x, y, z) is bit x & 31
// of word (z * ny + y) * wx + (x >> 5).  PADDING: the bits of a row's last word at x >= nx are ignored on input, whatever they hold,
// and are 0 on output.
struct RegionDims { int nx, ny, nz, wx; };

constexpr int MASK_THREADS = 256;                        // the block of the one-thread-per-word and one-lane-per-voxel kernels

// the bits of word gw (0 <= gw < wx) that are voxels: all but the padding of a row's last word
__device__ inline uint32_t valid_bits(int gw, const RegionDims& d)
{
    const int rem = d.nx - gw * 32;
    return rem >= 32 ? 0xffffffffu : (1u << rem) - 1u;
}

// the 32 bits of this lane's half of the wave: with one lane per voxel, the mask word of the lane's 32 voxels
__device__ inline uint32_t half_ballot(bool p)
{
    const unsigned long long b = __ballot(p);
    return (threadIdx.x & 32) ? (uint32_t)(b >> 32) : (uint32_t)b;
}

// A lane of the one-lane-per-voxel kernels, 32 lanes per mask word: lane t is bit `bit` of word i (word gw of row `row`), voxel v =
// (x, y, z).  word_ok: the word exists (the lanes past the last word take word 0's coordinates); inside: the voxel exists.  A kernel
// pays for the fields it reads.  (svr_distance.hip, svr_geo_relax.hpp and its two files use it; svr_label.hip keeps its own form, see there.)
struct LaneAt { size_t i, v, row; int bit, gw, x, y, z; bool word_ok, inside; };
__device__ inline LaneAt lane_at(size_t t, const RegionDims& d, size_t words)
{
    LaneAt a;
    a.i = t >> 5;
    a.bit = (int)(t & 31u);
    a.word_ok = a.i < words;
    const size_t i = a.word_ok ? a.i : 0;
    a.gw = (int)(i % (unsigned)d.wx);
    a.row = i / (unsigned)d.wx;
    a.x = a.gw * 32 + a.bit;
    a.y = (int)(a.row % (unsigned)d.ny);
    a.z = (int)(a.row / (unsigned)d.ny);
    a.inside = a.word_ok && a.x < d.nx;
    a.v = a.row * (size_t)d.nx + (size_t)a.x;
    return a;
}
// the thread of a lane_grid (below) in launch order: blockIdx.y counts planes of gridDim.x blocks
__device__ inline size_t lane_thread() { return ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * MASK_THREADS + threadIdx.x; }
__device__ inline LaneAt lane_at(const RegionDims& d, size_t words) { return lane_at(lane_thread(), d, words); }

inline RegionDims make_dims(int nx, int ny, int nz) { return RegionDims{nx, ny, nz, (nx + 31) / 32}; }
inline size_t mask_words(const RegionDims& d) { return (size_t)d.wx * d.ny * d.nz; }

// The grids of MASK_THREADS threads: one thread per item (a mask word, mostly), one lane per voxel of `words` mask words.  A volume has
// at most 2^31 voxels, so at most 2^31 items: 2^23 blocks.  A row has fewer words than voxels, so words <= 2^31 as well, and the lanes
// of the narrowest rows (nx = 1: 32 lanes per voxel) make up to 2^28 blocks of 2^36 threads.  The runtime refuses a launch of more than
// 2^32 - 1 threads along one dimension (hipErrorInvalidConfiguration: 2^27 words of rows with nx <= 32 reach exactly 2^32), so the
// blocks past LANE_GRID_X go to planes along y: at most 2^6.  The kernels take their lane from lane_thread(); the blocks that the last
// plane has too many find no word (word_ok, or their own test against `words`).
constexpr uint32_t LANE_GRID_X = 1u << 22;               // 2^30 threads along x
inline dim3 word_grid(size_t items) { return dim3((uint32_t)((items + MASK_THREADS - 1) / MASK_THREADS)); }
inline dim3 lane_grid(size_t words)
{
    const size_t blocks = (words * 32 + MASK_THREADS - 1) / MASK_THREADS;
    if (blocks <= LANE_GRID_X) return dim3((uint32_t)blocks);
    return dim3(LANE_GRID_X, (uint32_t)((blocks + LANE_GRID_X - 1) / LANE_GRID_X));
}

} // namespace
