// svr_compare.hip -- comparing segmentations: the surface of a mask, the overlap counts of two masks and the overlap table of two label
// maps, the reduction / histogram / quantile of a uint32 map over a (sparse) mask, and their composition into Dice, Hausdorff and
// surface distances (svr_region_surface, _overlap, _label_overlap, svr_overlap_match, svr_region_distance_summary / _histogram /
// _quantile, svr_region_compare, svr_region_compare_measure; the contract is in include/svr_abi.h, the design in DESIGN.md 8t).
// Integers only on the device (but for the double square root of the isqrt, as in svr_distance.hip's k_dist_volume): every result is
// exact, whatever order the GPU works in.  The host scaffolding is svr_volume_host.hpp's, the mask layout svr_mask.hpp's.
//
// SURFACE (k_surface<ELEMENT>): one thread per mask word, the plain / shifted table of svr_morph.hip's k_morph_step, as an AND: e = the
//   AND over the neighbours of the element, a word outside the volume and the padding reading as 0 (UNSET -- the one difference from
//   ERODE, whose complemented loads make them read as set), out = in & ~e.  The carry into bit 0 of a row's first word and into the
//   last voxel of a row (bit 31 of an unpadded last word: the word past the row's end; bit nx % 32 - 1 of a padded one: the padding
//   bit above it) is therefore 0, and those voxels are surface.
// OVERLAP (k_overlap): popcounts of a & b, a & ~b, ~a & b, ~a & ~b under the domain and the valid bits, a capped grid striding over the
//   words, a wave reduction by shuffles, a block reduction through LDS, then one 64-bit atomic add per block and count.
// LABEL OVERLAP (k_label_overlap): the cell of a voxel is la * (count_b + 1) + lb, so this is the counting problem of svr_histogram.hip's
//   k_histogram, WRITTEN AGAIN here (its chunk walk carries a box, a mask and u16 loads that a table of two label arrays has no use
//   for; svr_histogram.hip is untouched): flat chunks of V = 4 voxels (one 16-byte load of each array; V = 1 for unaligned arrays), a
//   lane adds a run of equal neighbouring cells once, a wave trip whose counting voxels all fall in one cell adds nothing and extends a
//   (cell, count) pair in registers, and the counters are LDS up to the same switches: OVL_LDS_CELLS_SMALL cells in 64 KB, up to 2 *
//   OVL_LDS_CELLS_LARGE in passes of 128 KB blocks (blockIdx.y), global atomics beyond.
// SUMMARY, HISTOGRAM (k_map_summary, k_map_histogram) are driven by the MASK WORDS (visit_masked): a wave loads 64 consecutive words,
//   one per lane, ballots the non-zero ones and visits those two at a time, the lower half of the wave on one word and the upper half
//   on the next, one lane per voxel (half_ballot's geometry): a zero word costs its 4 bytes and no map load, and the map loads of a
//   word are 128 contiguous bytes.  With no mask every word reads as its valid bits.  A capped grid (CMP_MAX_BLOCKS blocks of
//   CMP_THREADS) strides over the words with 64-bit indices.  The summary reduces in the lane, then the wave, then the block, and ends
//   in 64-bit integer atomics, one per block and field; max and first_max come from one atomicMax on (max << 32) | (0xFFFFFFFF -
//   index).  The histogram counts in LDS up to CMP_HIST_LDS_BINS bins (global atomics beyond); a visit whose counting lanes all fall
//   in one bin (the zeros of two agreeing surfaces) adds its population once.
// No block waits for another: there is no flag to spin on and no barrier wider than a block.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"

#include "svr_mask.hpp"             // the mask layout
#include "svr_volume_host.hpp"      // the argument checks, DeviceBuffer, CallTimer, SVR_HIP_TRY

using svr::failf;

namespace {

constexpr int CMP_THREADS = 256;                         // 4 waves
constexpr int CMP_MAX_BLOCKS = 1024;                     // the capped grid: one trip covers CMP_MAX_BLOCKS * CMP_THREADS mask words
constexpr int CMP_HIST_LDS_BINS = 16384;                 // bins of the 64 KB LDS histogram
constexpr int CMP_MAX_BINS = 65536;
constexpr int OVL_THREADS = 1024;                        // the label table: the block, grid and switches of svr_histogram.hip
constexpr int OVL_MAX_BLOCKS = 512;
constexpr int OVL_LDS_CELLS_SMALL = 16384;
constexpr int OVL_LDS_CELLS_LARGE = 32768;
constexpr uint32_t NONE = SVR_DIST_NONE;
constexpr uint32_t NO_CELL = 0xffffffffu;
constexpr int MAX_TOL = SVR_COMPARE_MAX_TOLERANCES;

// ---- the accumulators of one overlap or summary launch: uint64 words in device memory ----
constexpr int ACC_VOXELS = 0, ACC_NONE = 1, ACC_SUM = 2, ACC_ROOT = 3, ACC_KEY = 4, ACC_WITHIN = 5, ACC_WORDS = ACC_WITHIN + MAX_TOL;

__device__ inline unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}
__device__ inline unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// ---------------- the surface ----------------
template <int ELEMENT>
__global__ __launch_bounds__(MASK_THREADS) void k_surface(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, RegionDims d, unsigned long long words)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * MASK_THREADS + threadIdx.x;
    if (i >= words) return;
    const int gw = (int)(i % (unsigned)d.wx);
    const unsigned long long row = i / (unsigned)d.wx;
    const int gy = (int)(row % (unsigned)d.ny), gz = (int)(row / (unsigned)d.ny);
    // a word of the input; 0 (unset) outside the volume and in the padding
    auto word = [&](int w, int y, int z) -> uint32_t {
        if (w < 0 || w >= d.wx || y < 0 || y >= d.ny || z < 0 || z >= d.nz) return 0u;
        return in[((size_t)z * d.ny + y) * d.wx + w] & valid_bits(w, d);
    };
    uint32_t e = 0xffffffffu;                                                            // the voxels whose neighbours are all set
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int k = (dz != 0) + (dy != 0);                                         // steps of the move besides the one in x
            const bool plain = k <= 1 ? true : ELEMENT >= 18;                            // dx = 0 (the centre word included)
            const bool shifted = k == 0 ? true : k == 1 ? ELEMENT >= 18 : ELEMENT == 26; // dx = +-1
            if (!plain && !shifted) continue;
            const uint32_t m = word(gw, gy + dy, gz + dz);
            if (plain) e &= m;
            if (shifted) e &= ((m << 1) | (word(gw - 1, gy + dy, gz + dz) >> 31)) & ((m >> 1) | (word(gw + 1, gy + dy, gz + dz) << 31));
        }
    out[i] = in[i] & ~e & valid_bits(gw, d);
}

// ---------------- the overlap counts of two masks ----------------
__global__ __launch_bounds__(CMP_THREADS) void k_overlap(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ domain,
                                                          RegionDims d, unsigned long long words, unsigned long long* acc)
{
    __shared__ unsigned long long part[CMP_THREADS / 64][4];
    uint32_t c[4] = {0u, 0u, 0u, 0u};                                                    // a thread sees at most 2^31 voxels
    const unsigned long long stride = (unsigned long long)gridDim.x * CMP_THREADS;
    for (unsigned long long i = (unsigned long long)blockIdx.x * CMP_THREADS + threadIdx.x; i < words; i += stride) {
        uint32_t dom = valid_bits((int)((uint32_t)i % (uint32_t)d.wx), d);               // i < words <= 2^31
        if (domain) dom &= domain[i];
        const uint32_t x = a[i], y = b[i];
        c[SVR_OVERLAP_BOTH] += (uint32_t)__popc(x & y & dom);
        c[SVR_OVERLAP_A_ONLY] += (uint32_t)__popc(x & ~y & dom);
        c[SVR_OVERLAP_B_ONLY] += (uint32_t)__popc(~x & y & dom);
        c[SVR_OVERLAP_NEITHER] += (uint32_t)__popc(~x & ~y & dom);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long s = wave_sum(c[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long s = 0ull;
        for (int w = 0; w < CMP_THREADS / 64; ++w) s += part[w][threadIdx.x];
        if (s) atomicAdd(&acc[threadIdx.x], s);
    }
}

// ---------------- the overlap table of two label maps ----------------
struct OverlapJob {
    const uint32_t *a, *b;
    uint32_t* table;
    unsigned long long n, chunks;
    uint32_t count_a, count_b, cells;
};

// LDS_CELLS > 0: the block counts the cells [pass * LDS_CELLS, (pass + 1) * LDS_CELLS) in LDS, pass = blockIdx.y; 0: global atomics
template <int V, int LDS_CELLS>
__global__ __launch_bounds__(OVL_THREADS) void k_label_overlap(OverlapJob j)
{
    __shared__ uint32_t lh[LDS_CELLS > 0 ? LDS_CELLS : 1];
    const uint32_t base = LDS_CELLS > 0 ? blockIdx.y * (uint32_t)LDS_CELLS : 0u;
    const uint32_t mine = LDS_CELLS > 0 ? (j.cells - base < (uint32_t)LDS_CELLS ? j.cells - base : (uint32_t)LDS_CELLS) : j.cells;
    if (LDS_CELLS > 0) {
        for (uint32_t c = threadIdx.x; c < mine; c += OVL_THREADS) lh[c] = 0u;
        __syncthreads();
    }
    uint32_t* const tgt = LDS_CELLS > 0 ? lh : j.table;
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t row = j.count_b + 1u;
    uint32_t hot_cell = NO_CELL, hot_count = 0u;                                 // wave-uniform: the cell of the last uniform trips
    // all 64 lanes of a wave make the same trips: the ballots and shuffles below see a full wave
    const unsigned long long stride = (unsigned long long)gridDim.x * OVL_THREADS;
    for (unsigned long long c0 = (unsigned long long)blockIdx.x * OVL_THREADS + (threadIdx.x & ~63u); c0 < j.chunks; c0 += stride) {
        const unsigned long long c = c0 + lane;
        uint32_t cell[V];
#pragma unroll
        for (int k = 0; k < V; ++k) cell[k] = NO_CELL;
        if (c < j.chunks) {
            const unsigned long long i0 = c * V;
            uint32_t la[V], lb[V];
            if (V == 4 && i0 + 4 <= j.n) {
                const uint4 p = *reinterpret_cast<const uint4*>(j.a + i0), q = *reinterpret_cast<const uint4*>(j.b + i0);
                la[0] = p.x; la[1 % V] = p.y; la[2 % V] = p.z; la[3 % V] = p.w;
                lb[0] = q.x; lb[1 % V] = q.y; lb[2 % V] = q.z; lb[3 % V] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const bool in = i0 + k < j.n;
                    la[k] = in ? j.a[i0 + k] : NO_CELL;                          // (above every count: not counted)
                    lb[k] = in ? j.b[i0 + k] : NO_CELL;
                }
            }
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (la[k] <= j.count_a && lb[k] <= j.count_b) cell[k] = la[k] * row + lb[k];
        }
        uint32_t first = NO_CELL, cnt = 0u;
        bool single = true;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (cell[k] != NO_CELL && cell[k] - base >= mine) cell[k] = NO_CELL;          // another pass counts it
            if (cell[k] != NO_CELL) {
                if (first == NO_CELL) first = cell[k];
                single = single && cell[k] == first;
                ++cnt;
            }
        }
        const unsigned long long any = __ballot(cnt != 0u);
        if (any == 0ull) continue;
        const uint32_t b0 = (uint32_t)__shfl((int)first, (int)__builtin_ctzll(any), 64);
        if (__ballot(cnt == 0u || (single && first == b0)) == ~0ull) {
            uint32_t total = 0u;                                                 // the wave's sum of cnt (0 .. 4 a lane): one ballot per bit
#pragma unroll
            for (int k = 0; k < 3; ++k) total += (uint32_t)__builtin_popcountll(__ballot((cnt >> k) & 1u)) << k;
            if (b0 != hot_cell) {
                if (hot_count && lane == 0u) atomicAdd(&tgt[hot_cell - base], hot_count);
                hot_cell = b0; hot_count = 0u;
            }
            hot_count += total;
        } else {
            uint32_t run = 0u;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if (cell[k] == NO_CELL) continue;
                ++run;
                if (k == V - 1 || cell[(k + 1) % V] != cell[k]) { atomicAdd(&tgt[cell[k] - base], run); run = 0u; }
            }
        }
    }
    if (hot_count && lane == 0u) atomicAdd(&tgt[hot_cell - base], hot_count);
    if (LDS_CELLS > 0) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < mine; c += OVL_THREADS) {
            const uint32_t n = lh[c];
            if (n) atomicAdd(&j.table[base + c], n);
        }
    }
}

template <int V>
hipError_t launch_label_overlap(OverlapJob j, hipStream_t st)
{
    j.chunks = (j.n + V - 1) / V;
    const unsigned long long want = (j.chunks + OVL_THREADS - 1) / OVL_THREADS;
    const uint32_t blocks = (uint32_t)(want < (unsigned long long)OVL_MAX_BLOCKS ? want : (unsigned long long)OVL_MAX_BLOCKS);
    if (j.cells <= (uint32_t)OVL_LDS_CELLS_SMALL)
        hipLaunchKernelGGL((k_label_overlap<V, OVL_LDS_CELLS_SMALL>), dim3(blocks), dim3(OVL_THREADS), 0, st, j);
    else if (j.cells <= 2u * (uint32_t)OVL_LDS_CELLS_LARGE)
        hipLaunchKernelGGL((k_label_overlap<V, OVL_LDS_CELLS_LARGE>), dim3(blocks, (j.cells + OVL_LDS_CELLS_LARGE - 1) / OVL_LDS_CELLS_LARGE),
                           dim3(OVL_THREADS), 0, st, j);
    else
        hipLaunchKernelGGL((k_label_overlap<V, 0>), dim3(blocks), dim3(OVL_THREADS), 0, st, j);
    return hipGetLastError();
}

// ---------------- a uint32 map over the voxels of a mask ----------------
// Calls f(on, v, value) for every voxel of the mask, wave by wave: `on` lanes hold a voxel (linear index v, map value); every lane of
// the wave calls f together, so f may ballot and shuffle.  All 64 lanes of a wave make the same trips.
template <class F>
__device__ inline void visit_masked(const uint32_t* __restrict__ map, const uint32_t* __restrict__ mask, const RegionDims& d, unsigned long long words, F&& f)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * CMP_THREADS;
    for (unsigned long long w0 = (unsigned long long)blockIdx.x * CMP_THREADS + (threadIdx.x & ~63u); w0 < words; w0 += stride) {
        const unsigned long long i = w0 + lane;
        uint32_t m = 0u;
        if (i < words) m = (mask ? mask[i] : 0xffffffffu) & valid_bits((int)((uint32_t)i % (uint32_t)d.wx), d);      // i < words <= 2^31
        unsigned long long live = __ballot(m != 0u);
        while (live) {                                                           // two words a visit: the lower half of the wave, the upper half
            const int s0 = __builtin_ctzll(live);
            live &= live - 1ull;
            const bool two = live != 0ull;
            const int s1 = two ? __builtin_ctzll(live) : s0;
            live &= live - 1ull;                                                 // (0 stays 0)
            const bool upper = lane >= 32u;
            const int src = upper ? s1 : s0;
            const uint32_t mw = (uint32_t)__shfl((int)m, src, 64);
            const bool on = (!upper || two) && ((mw >> (lane & 31u)) & 1u);
            size_t v = 0;
            uint32_t value = 0u;
            if (on) {
                const uint32_t wi = (uint32_t)(w0 + (unsigned)src);              // a word that exists: below 2^31
                const uint32_t row = wi / (uint32_t)d.wx, gw = wi - row * (uint32_t)d.wx;
                v = (size_t)row * (size_t)d.nx + gw * 32u + (lane & 31u);
                value = map[v];
            }
            f(on, v, value);
        }
    }
}

struct SummaryJob {
    const uint32_t* map;
    const uint32_t* mask;            // or nullptr
    RegionDims d;
    unsigned long long words;
    uint32_t ntol, tol[MAX_TOL];
    unsigned long long* acc;         // ACC_WORDS
};

// floor(256 sqrt(v)) = isqrt(v 2^16): the product is below 2^48, exact in a double, whose correctly rounded root is off by at most one
__device__ inline uint64_t root_q8(uint32_t v)
{
    const uint64_t p = (uint64_t)v << 16;
    uint64_t s = (uint64_t)sqrt((double)p);
    if (s * s > p) --s;
    else if ((s + 1u) * (s + 1u) <= p) ++s;
    return s;
}

__global__ __launch_bounds__(CMP_THREADS) void k_map_summary(SummaryJob j)
{
    __shared__ unsigned long long part[CMP_THREADS / 64][ACC_WORDS];
    uint32_t cnt = 0u, none = 0u, within[MAX_TOL];                               // a lane sees at most 2^31 voxels
    unsigned long long sum = 0ull, root = 0ull, key = 0ull;                      // key 0 = nothing: 0xFFFFFFFF - index is never 0
#pragma unroll
    for (int k = 0; k < MAX_TOL; ++k) within[k] = 0u;
    visit_masked(j.map, j.mask, j.d, j.words, [&](bool on, size_t v, uint32_t value) {
        if (!on) return;
        if (value == NONE) { ++none; return; }
        ++cnt;
        sum += value;
        root += root_q8(value);
        const unsigned long long k64 = ((unsigned long long)value << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)v);
        key = k64 > key ? k64 : key;
#pragma unroll
        for (int k = 0; k < MAX_TOL; ++k) within[k] += (k < (int)j.ntol && value <= j.tol[k]) ? 1u : 0u;
    });
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long r[ACC_WORDS];
    r[ACC_VOXELS] = wave_sum(cnt); r[ACC_NONE] = wave_sum(none); r[ACC_SUM] = wave_sum(sum); r[ACC_ROOT] = wave_sum(root); r[ACC_KEY] = wave_max(key);
#pragma unroll
    for (int k = 0; k < MAX_TOL; ++k) r[ACC_WITHIN + k] = wave_sum(within[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < ACC_WORDS; ++k) part[wave][k] = r[k];
    }
    __syncthreads();
    if (threadIdx.x < ACC_WORDS) {
        const int k = threadIdx.x;
        unsigned long long s = 0ull;
        for (int w = 0; w < CMP_THREADS / 64; ++w) {
            const unsigned long long p = part[w][k];
            s = k == ACC_KEY ? (p > s ? p : s) : s + p;
        }
        if (s) {
            if (k == ACC_KEY) atomicMax(&j.acc[k], s);
            else atomicAdd(&j.acc[k], s);
        }
    }
}

struct MapHistJob {
    const uint32_t* map;
    const uint32_t* mask;            // or nullptr
    RegionDims d;
    unsigned long long words;
    uint32_t lo, hi, shift, bins;
    uint32_t* counts;
};

template <bool LDS>
__global__ __launch_bounds__(CMP_THREADS) void k_map_histogram(MapHistJob j)
{
    __shared__ uint32_t lh[LDS ? CMP_HIST_LDS_BINS : 1];
    if (LDS) {
        for (uint32_t c = threadIdx.x; c < j.bins; c += CMP_THREADS) lh[c] = 0u;
        __syncthreads();
    }
    uint32_t* const tgt = LDS ? lh : j.counts;
    const unsigned lane = threadIdx.x & 63u;
    visit_masked(j.map, j.mask, j.d, j.words, [&](bool on, size_t, uint32_t value) {
        const bool counts = on && value >= j.lo && value <= j.hi;
        const uint32_t bin = counts ? (value - j.lo) >> j.shift : NO_CELL;
        const unsigned long long any = __ballot(counts);
        if (any == 0ull) return;
        const unsigned leader = (unsigned)__builtin_ctzll(any);
        const uint32_t b0 = (uint32_t)__shfl((int)bin, (int)leader, 64);
        if (__ballot(!counts || bin == b0) == ~0ull) {                           // one bin: its population, once
            if (lane == leader) atomicAdd(&tgt[b0], (uint32_t)__builtin_popcountll(any));
        } else if (counts) {
            atomicAdd(&tgt[bin], 1u);
        }
    });
    if (LDS) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < j.bins; c += CMP_THREADS) {
            const uint32_t n = lh[c];
            if (n) atomicAdd(&j.counts[c], n);
        }
    }
}

// ---------------- host side ----------------
CallEvents g_events;

uint32_t capped_blocks(size_t words)
{
    const size_t want = (words + CMP_THREADS - 1) / CMP_THREADS;
    return (uint32_t)(want < (size_t)CMP_MAX_BLOCKS ? want : (size_t)CMP_MAX_BLOCKS);
}

hipError_t launch_surface(hipStream_t st, const uint32_t* in, const RegionDims& d, int element, uint32_t* out)
{
    const unsigned long long words = mask_words(d);
    const dim3 g = word_grid(words), b(MASK_THREADS);
    if (element == 6) hipLaunchKernelGGL((k_surface<6>), g, b, 0, st, in, out, d, words);
    else if (element == 18) hipLaunchKernelGGL((k_surface<18>), g, b, 0, st, in, out, d, words);
    else hipLaunchKernelGGL((k_surface<26>), g, b, 0, st, in, out, d, words);
    return hipGetLastError();
}

// Each reduction is a launch (the accumulators cleared, then the kernel: the device work that a CallTimer spans) and a fetch (the
// accumulators copied to the host: synchronises).
hipError_t fetch_words(hipStream_t st, const unsigned long long* acc, unsigned long long* host, int n)
{
    const hipError_t e = hipMemcpyAsync(host, acc, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// acc: 4 device words
hipError_t launch_overlap(hipStream_t st, const uint32_t* a, const uint32_t* b, const uint32_t* domain, const RegionDims& d, unsigned long long* acc)
{
    const hipError_t e = hipMemsetAsync(acc, 0, 4 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const unsigned long long words = mask_words(d);
    hipLaunchKernelGGL(k_overlap, dim3(capped_blocks(words)), dim3(CMP_THREADS), 0, st, a, b, domain, d, words, acc);
    return hipGetLastError();
}
hipError_t fetch_overlap(hipStream_t st, const unsigned long long* acc, uint64_t counts[4])
{
    unsigned long long host[4];
    const hipError_t e = fetch_words(st, acc, host, 4);
    if (e != hipSuccess) return e;
    for (int k = 0; k < 4; ++k) counts[k] = host[k];
    return hipSuccess;
}
hipError_t run_overlap(hipStream_t st, const uint32_t* a, const uint32_t* b, const uint32_t* domain, const RegionDims& d, unsigned long long* acc,
                       uint64_t counts[4])
{
    const hipError_t e = launch_overlap(st, a, b, domain, d, acc);
    return e != hipSuccess ? e : fetch_overlap(st, acc, counts);
}

// acc: ACC_WORDS device words
hipError_t launch_summary(hipStream_t st, const uint32_t* map, const uint32_t* mask, const RegionDims& d, const uint32_t* tol, uint32_t ntol,
                          unsigned long long* acc)
{
    const hipError_t e = hipMemsetAsync(acc, 0, ACC_WORDS * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    SummaryJob j;
    j.map = map; j.mask = mask; j.d = d; j.words = mask_words(d); j.ntol = ntol; j.acc = acc;
    for (int k = 0; k < MAX_TOL; ++k) j.tol[k] = k < (int)ntol ? tol[k] : 0u;
    hipLaunchKernelGGL(k_map_summary, dim3(capped_blocks(j.words)), dim3(CMP_THREADS), 0, st, j);
    return hipGetLastError();
}
hipError_t fetch_summary(hipStream_t st, const unsigned long long* acc, svr_distance_summary* out)
{
    unsigned long long host[ACC_WORDS];
    const hipError_t e = fetch_words(st, acc, host, ACC_WORDS);
    if (e != hipSuccess) return e;
    memset(out, 0, sizeof *out);
    out->voxels = host[ACC_VOXELS]; out->none = host[ACC_NONE]; out->sum = host[ACC_SUM]; out->sum_root_q8 = host[ACC_ROOT];
    out->max = (uint32_t)(host[ACC_KEY] >> 32);
    out->first_max = host[ACC_KEY] ? 0xFFFFFFFFu - (uint32_t)host[ACC_KEY] : 0u;
    for (int k = 0; k < MAX_TOL; ++k) out->within[k] = (uint32_t)host[ACC_WITHIN + k];
    return hipSuccess;
}
hipError_t run_summary(hipStream_t st, const uint32_t* map, const uint32_t* mask, const RegionDims& d, const uint32_t* tol, uint32_t ntol,
                       unsigned long long* acc, svr_distance_summary* out)
{
    const hipError_t e = launch_summary(st, map, mask, d, tol, ntol, acc);
    return e != hipSuccess ? e : fetch_summary(st, acc, out);
}

uint32_t bins_of(uint32_t lo, uint32_t hi, uint32_t shift) { return ((hi - lo) >> shift) + 1u; }

hipError_t launch_map_histogram(hipStream_t st, const uint32_t* map, const uint32_t* mask, const RegionDims& d, uint32_t lo, uint32_t hi, uint32_t shift,
                                uint32_t* counts)
{
    MapHistJob j;
    j.map = map; j.mask = mask; j.d = d; j.words = mask_words(d); j.lo = lo; j.hi = hi; j.shift = shift; j.bins = bins_of(lo, hi, shift); j.counts = counts;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)j.bins * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const dim3 g(capped_blocks(j.words)), b(CMP_THREADS);
    if (j.bins <= (uint32_t)CMP_HIST_LDS_BINS) hipLaunchKernelGGL((k_map_histogram<true>), g, b, 0, st, j);
    else hipLaunchKernelGGL((k_map_histogram<false>), g, b, 0, st, j);
    return hipGetLastError();
}

// the first index b of c[0 .. bins) with before + C(b) > 0 and den (before + C(b)) >= num total; `before` is left at the count below it
uint32_t quantile_index(const uint32_t* c, uint32_t bins, uint32_t num, uint32_t den, uint64_t total, uint64_t* before)
{
    const unsigned __int128 want = (unsigned __int128)num * total;
    uint64_t sum = *before;
    for (uint32_t b = 0; b < bins; ++b) {
        if (sum + c[b] > 0u && (unsigned __int128)den * (sum + c[b]) >= want) { *before = sum; return b; }
        sum += c[b];
    }
    *before = sum;
    return bins - 1u;                                     // (not reached: C(bins - 1) = total satisfies the test)
}

// the quantile of the `total` > 0 values 0 .. maxv of the map over the mask; counts: CMP_MAX_BINS device words; synchronises
hipError_t run_quantile(hipStream_t st, const uint32_t* map, const uint32_t* mask, const RegionDims& d, uint32_t num, uint32_t den, uint32_t maxv,
                        uint64_t total, uint32_t* counts, uint32_t* value)
{
    uint32_t shift = 0u;
    while ((maxv >> shift) + 1u > (uint32_t)CMP_MAX_BINS) ++shift;
    std::vector<uint32_t> host((size_t)CMP_MAX_BINS);
    uint32_t lo = 0u, hi = maxv;
    uint64_t before = 0u;
    for (;;) {
        const uint32_t bins = bins_of(lo, hi, shift);
        hipError_t e = launch_map_histogram(st, map, mask, d, lo, hi, shift, counts);
        if (e != hipSuccess) return e;
        if ((e = hipMemcpyAsync(host.data(), counts, (size_t)bins * sizeof(uint32_t), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        const uint32_t b = quantile_index(host.data(), bins, num, den, total, &before);
        if (shift == 0u) { *value = lo + b; return hipSuccess; }
        lo = b << shift;                                  // the values of bin b, one bin each (lo was 0)
        hi = lo + ((1u << shift) - 1u) < maxv ? lo + ((1u << shift) - 1u) : maxv;
        shift = 0u;
    }
}

int check_tolerances(const char* who, const uint32_t* tol, uint32_t ntol)
{
    if (ntol > (uint32_t)MAX_TOL) return failf(-3, "%s: ntol must be at most %d (got %u)", who, MAX_TOL, ntol);
    if (ntol && !tol) return failf(-4, "%s: null argument", who);
    return 0;
}

int check_quantile(const char* who, uint32_t num, uint32_t den)
{
    if (den == 0u || num > den) return failf(-3, "%s: the quantile %u / %u is not in 0 .. 1", who, num, den);
    return 0;
}

double nan_value() { return std::numeric_limits<double>::quiet_NaN(); }

} // namespace

extern "C" {

int svr_region_surface(const uint32_t* in_mask_device, int nx, int ny, int nz, int element, uint32_t* out_mask_device)
{
    const char* who = "svr_region_surface";
    if (!in_mask_device || !out_mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (int e = check_connectivity(who, "element", element)) return e;
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t bytes = mask_words(d) * sizeof(uint32_t);
    if (overlap(in_mask_device, bytes, out_mask_device, bytes)) return failf(-3, "%s: out must not overlap in", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(launch_surface(st, in_mask_device, d, element, out_mask_device));
    return 0;
}

int svr_region_overlap(const uint32_t* a_mask_device, const uint32_t* b_mask_device, int nx, int ny, int nz, const uint32_t* domain_mask_device_or_null,
                       uint64_t counts_host[4])
{
    const char* who = "svr_region_overlap";
    if (!a_mask_device || !b_mask_device || !counts_host) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    DeviceBuffer acc;
    SVR_HIP_TRY(acc.alloc(4 * sizeof(unsigned long long)));
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(launch_overlap(st, a_mask_device, b_mask_device, domain_mask_device_or_null, make_dims(nx, ny, nz), acc.as<unsigned long long>()));
    timer.stop();
    SVR_HIP_TRY(fetch_overlap(st, acc.as<unsigned long long>(), counts_host));
    return 0;
}

int svr_region_label_overlap(const uint32_t* a_labels_device, uint32_t count_a, const uint32_t* b_labels_device, uint32_t count_b, const int32_t dims[3],
                             uint32_t* table_device)
{
    const char* who = "svr_region_label_overlap";
    if (!a_labels_device || !b_labels_device || !dims || !table_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, dims[0], dims[1], dims[2])) return e;
    if (count_a == 0u || count_b == 0u) return failf(-3, "%s: count_a and count_b must be at least 1 (got %u, %u)", who, count_a, count_b);
    const unsigned long long cells = ((unsigned long long)count_a + 1ull) * ((unsigned long long)count_b + 1ull);
    if (cells > SVR_HISTOGRAM_MAX_CELLS)
        return failf(-3, "%s: (count_a + 1) * (count_b + 1) = %llu cells is more than SVR_HISTOGRAM_MAX_CELLS (%u)", who, cells, SVR_HISTOGRAM_MAX_CELLS);
    const size_t n = (size_t)dims[0] * dims[1] * dims[2];
    const size_t out_bytes = (size_t)cells * sizeof(uint32_t);
    if (overlap(table_device, out_bytes, a_labels_device, n * sizeof(uint32_t)) || overlap(table_device, out_bytes, b_labels_device, n * sizeof(uint32_t)))
        return failf(-3, "%s: table_device must not overlap an input", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(hipMemsetAsync(table_device, 0, out_bytes, st));
    OverlapJob j;
    j.a = a_labels_device; j.b = b_labels_device; j.table = table_device; j.n = n; j.chunks = 0ull;
    j.count_a = count_a; j.count_b = count_b; j.cells = (uint32_t)cells;
    const bool vec4 = (uintptr_t)a_labels_device % 16 == 0 && (uintptr_t)b_labels_device % 16 == 0;
    SVR_HIP_TRY(vec4 ? launch_label_overlap<4>(j, st) : launch_label_overlap<1>(j, st));
    return 0;
}

int svr_overlap_match(const uint32_t* table_host, uint32_t count_a, uint32_t count_b, uint32_t* best_b_for_a, uint32_t* best_a_for_b_or_null)
{
    const char* who = "svr_overlap_match";
    if (!table_host || !best_b_for_a) return failf(-4, "%s: null argument", who);
    if (count_a == 0u || count_b == 0u) return failf(-3, "%s: count_a and count_b must be at least 1 (got %u, %u)", who, count_a, count_b);
    const size_t ra = (size_t)count_a + 1u, rb = (size_t)count_b + 1u;
    std::vector<uint64_t> size_a(ra, 0u), size_b(rb, 0u);
    for (size_t la = 0; la < ra; ++la)
        for (size_t lb = 0; lb < rb; ++lb) {
            const uint32_t c = table_host[la * rb + lb];
            size_a[la] += c;
            size_b[lb] += c;
        }
    // inter / uni > best_inter / best_uni, exactly; every operand is below 2^64
    auto better = [](uint64_t inter, uint64_t uni, uint64_t best_inter, uint64_t best_uni) {
        return (unsigned __int128)inter * best_uni > (unsigned __int128)best_inter * uni;
    };
    for (size_t la = 1; la < ra; ++la) {
        uint64_t bi = 0u, bu = 1u;
        uint32_t best = 0u;
        for (size_t lb = 1; lb < rb; ++lb) {
            const uint64_t inter = table_host[la * rb + lb];
            if (inter && better(inter, size_a[la] + size_b[lb] - inter, bi, bu)) { bi = inter; bu = size_a[la] + size_b[lb] - inter; best = (uint32_t)lb; }
        }
        best_b_for_a[la - 1u] = best;
    }
    if (best_a_for_b_or_null)
        for (size_t lb = 1; lb < rb; ++lb) {
            uint64_t bi = 0u, bu = 1u;
            uint32_t best = 0u;
            for (size_t la = 1; la < ra; ++la) {
                const uint64_t inter = table_host[la * rb + lb];
                if (inter && better(inter, size_a[la] + size_b[lb] - inter, bi, bu)) { bi = inter; bu = size_a[la] + size_b[lb] - inter; best = (uint32_t)la; }
            }
            best_a_for_b_or_null[lb - 1u] = best;
        }
    return 0;
}

int svr_region_distance_summary(const uint32_t* map_device, const uint32_t* mask_device_or_null, int nx, int ny, int nz, const uint32_t* tolerances2_or_null,
                                uint32_t ntol, svr_distance_summary* out_host)
{
    const char* who = "svr_region_distance_summary";
    if (!map_device || !out_host) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (int e = check_tolerances(who, tolerances2_or_null, ntol)) return e;
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    DeviceBuffer acc;
    SVR_HIP_TRY(acc.alloc(ACC_WORDS * sizeof(unsigned long long)));
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(launch_summary(st, map_device, mask_device_or_null, make_dims(nx, ny, nz), tolerances2_or_null, ntol, acc.as<unsigned long long>()));
    timer.stop();
    SVR_HIP_TRY(fetch_summary(st, acc.as<unsigned long long>(), out_host));
    return 0;
}

int svr_region_distance_histogram(const uint32_t* map_device, const uint32_t* mask_device_or_null, const int32_t dims[3], uint32_t lo, uint32_t hi,
                                  uint32_t shift, uint32_t* counts_device)
{
    const char* who = "svr_region_distance_histogram";
    if (!map_device || !dims || !counts_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, dims[0], dims[1], dims[2])) return e;
    if (lo > hi) return failf(-3, "%s: lo (%u) is above hi (%u)", who, lo, hi);
    if (shift > 31u) return failf(-3, "%s: shift must be <= 31 (got %u)", who, shift);
    if (((hi - lo) >> shift) >= (uint32_t)CMP_MAX_BINS)
        return failf(-3, "%s: %u .. %u at shift %u is more than %d bins: raise shift or narrow the window", who, lo, hi, shift, CMP_MAX_BINS);
    const RegionDims d = make_dims(dims[0], dims[1], dims[2]);
    const size_t n = (size_t)d.nx * d.ny * d.nz, out_bytes = (size_t)bins_of(lo, hi, shift) * sizeof(uint32_t);
    if (overlap(counts_device, out_bytes, map_device, n * sizeof(uint32_t)) ||
        (mask_device_or_null && overlap(counts_device, out_bytes, mask_device_or_null, mask_words(d) * sizeof(uint32_t))))
        return failf(-3, "%s: counts_device must not overlap an input", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(launch_map_histogram(st, map_device, mask_device_or_null, d, lo, hi, shift, counts_device));
    return 0;
}

int svr_region_distance_quantile(const uint32_t* map_device, const uint32_t* mask_device_or_null, const int32_t dims[3], uint32_t num, uint32_t den,
                                 uint32_t* value_out, int32_t* status)
{
    const char* who = "svr_region_distance_quantile";
    if (!map_device || !dims || !value_out || !status) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, dims[0], dims[1], dims[2])) return e;
    if (int e = check_quantile(who, num, den)) return e;
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const RegionDims d = make_dims(dims[0], dims[1], dims[2]);
    DeviceBuffer buf;                                     // the accumulators, then the counters
    SVR_HIP_TRY(buf.alloc(ACC_WORDS * sizeof(unsigned long long) + (size_t)CMP_MAX_BINS * sizeof(uint32_t)));
    unsigned long long* const acc = buf.as<unsigned long long>();
    uint32_t* const counts = reinterpret_cast<uint32_t*>(acc + ACC_WORDS);
    CallTimer timer(g_events, st);
    svr_distance_summary s;
    SVR_HIP_TRY(run_summary(st, map_device, mask_device_or_null, d, nullptr, 0u, acc, &s));
    *value_out = 0u;
    *status = s.voxels ? SVR_REGION_STATUS_OK : SVR_REGION_STATUS_EMPTY;
    if (s.voxels) SVR_HIP_TRY(run_quantile(st, map_device, mask_device_or_null, d, num, den, s.max, s.voxels, counts, value_out));
    return 0;
}

int svr_compare_params_default(svr_compare_params* p)
{
    if (!p) return failf(-4, "svr_compare_params_default: null argument");
    memset(p, 0, sizeof *p);
    p->element = 6;
    p->weights[0] = p->weights[1] = p->weights[2] = 1u;
    p->q_num = 95u; p->q_den = 100u;
    return 0;
}

int svr_region_compare(const uint32_t* a_mask_device, const uint32_t* b_mask_device, int nx, int ny, int nz, const svr_compare_params* params_or_null,
                       svr_region_comparison* out_host)
{
    const char* who = "svr_region_compare";
    if (!a_mask_device || !b_mask_device || !out_host) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    svr_compare_params p;
    if (params_or_null) p = *params_or_null;
    else svr_compare_params_default(&p);
    if (int e = check_connectivity(who, "element", p.element)) return e;
    uint32_t w[3];
    if (int e = svr::check_distance_weights(who, p.weights, nx, ny, nz, w)) return e;
    if (int e = check_quantile(who, p.q_num, p.q_den)) return e;
    if (int e = check_tolerances(who, p.tolerances2, p.ntol)) return e;
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t words = mask_words(d), n = (size_t)nx * ny * nz;
    DeviceBuffer buf;                                     // the accumulators, the counters, the map, the two surfaces
    SVR_HIP_TRY(buf.alloc(ACC_WORDS * sizeof(unsigned long long) + ((size_t)CMP_MAX_BINS + n + 2 * words) * sizeof(uint32_t)));
    unsigned long long* const acc = buf.as<unsigned long long>();
    uint32_t* const counts = reinterpret_cast<uint32_t*>(acc + ACC_WORDS);
    uint32_t* const map = counts + CMP_MAX_BINS;
    uint32_t* const surf[2] = {map + n, map + n + words};
    CallTimer timer(g_events, st);
    svr_region_comparison c;
    memset(&c, 0, sizeof c);
    c.ntol = p.ntol;
    SVR_HIP_TRY(run_overlap(st, a_mask_device, b_mask_device, nullptr, d, acc, c.overlap));
    SVR_HIP_TRY(launch_surface(st, a_mask_device, d, p.element, surf[0]));
    SVR_HIP_TRY(launch_surface(st, b_mask_device, d, p.element, surf[1]));
    uint64_t sc[4];
    SVR_HIP_TRY(run_overlap(st, surf[0], surf[1], nullptr, d, acc, sc));
    c.surface[0] = sc[SVR_OVERLAP_BOTH] + sc[SVR_OVERLAP_A_ONLY];
    c.surface[1] = sc[SVR_OVERLAP_BOTH] + sc[SVR_OVERLAP_B_ONLY];
    if (c.surface[0] == 0u) c.status |= SVR_COMPARE_A_EMPTY;                     // a mask is empty exactly when its surface is
    if (c.surface[1] == 0u) c.status |= SVR_COMPARE_B_EMPTY;
    for (int dir = 0; dir < 2; ++dir) {                                          // 0: from S(A) to S(B); 1: the reverse
        svr_distance_summary& s = dir ? c.ba : c.ab;
        uint32_t& q = dir ? c.quantile_ba : c.quantile_ab;
        const uint32_t *from = surf[dir], *to = surf[1 - dir];
        if (c.surface[dir] == 0u) continue;
        if (c.surface[1 - dir] == 0u) { s.none = c.surface[dir]; continue; }     // every distance is SVR_DIST_NONE
        if (int e = svr_region_distance(to, nx, ny, nz, w, SVR_DIST_TO_SET, map)) return e;
        SVR_HIP_TRY(run_summary(st, map, from, d, p.tolerances2, p.ntol, acc, &s));
        if (s.voxels) SVR_HIP_TRY(run_quantile(st, map, from, d, p.q_num, p.q_den, s.max, s.voxels, counts, &q));
    }
    timer.stop();
    *out_host = c;
    return 0;
}

int svr_region_compare_measure(const svr_region_comparison* c, double unit, svr_compare_measurement* out)
{
    const char* who = "svr_region_compare_measure";
    if (!c || !out) return failf(-4, "%s: null argument", who);
    if (c->ntol > (uint32_t)MAX_TOL) return failf(-3, "%s: ntol must be at most %d (got %u)", who, MAX_TOL, c->ntol);
    const double nan = nan_value();
    const double both = (double)c->overlap[SVR_OVERLAP_BOTH], a_only = (double)c->overlap[SVR_OVERLAP_A_ONLY], b_only = (double)c->overlap[SVR_OVERLAP_B_ONLY];
    const double va = both + a_only, vb = both + b_only, uni = both + a_only + b_only;
    const double n_ab = (double)c->ab.voxels, n_ba = (double)c->ba.voxels, n = n_ab + n_ba;
    memset(out, 0, sizeof *out);
    out->dice = uni > 0.0 ? 2.0 * both / (2.0 * both + a_only + b_only) : nan;
    out->jaccard = uni > 0.0 ? both / uni : nan;
    out->volume_difference = va + vb > 0.0 ? 2.0 * (va - vb) / (va + vb) : nan;
    out->hausdorff_ab = n_ab > 0.0 ? unit * std::sqrt((double)c->ab.max) : nan;
    out->hausdorff_ba = n_ba > 0.0 ? unit * std::sqrt((double)c->ba.max) : nan;
    out->hausdorff_q_ab = n_ab > 0.0 ? unit * std::sqrt((double)c->quantile_ab) : nan;
    out->hausdorff_q_ba = n_ba > 0.0 ? unit * std::sqrt((double)c->quantile_ba) : nan;
    const bool two = n_ab > 0.0 && n_ba > 0.0;
    out->hausdorff = two ? (out->hausdorff_ab > out->hausdorff_ba ? out->hausdorff_ab : out->hausdorff_ba) : nan;
    out->hausdorff_q = two ? (out->hausdorff_q_ab > out->hausdorff_q_ba ? out->hausdorff_q_ab : out->hausdorff_q_ba) : nan;
    out->assd = n > 0.0 ? unit * ((double)c->ab.sum_root_q8 + (double)c->ba.sum_root_q8) / 256.0 / n : nan;
    out->rms = n > 0.0 ? unit * std::sqrt(((double)c->ab.sum + (double)c->ba.sum) / n) : nan;
    const double surf = (double)c->surface[0] + (double)c->surface[1];
    for (uint32_t k = 0; k < c->ntol; ++k) out->surface_dice[k] = surf > 0.0 ? ((double)c->ab.within[k] + (double)c->ba.within[k]) / surf : nan;
    return 0;
}

int svr_region_compare_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_region_compare_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

} // extern "C"
