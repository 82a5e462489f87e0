// svr_dist_passes.hpp -- the row pass and the column pass of the exact squared Euclidean distance transform on the mask layout of
// svr_mask.hpp, shared by svr_distance.hip (the transform of a volume: rows, y, z; DESIGN.md 8k, where the passes are described) and
// svr_fillbetween.hip (the planar transform of slices: rows and one column pass).  The text of the kernels is the one
// svr_distance.hip held; each file that includes this header compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/svr_abi.h"
#include "svr_mask.hpp"             // RegionDims, valid_bits, lane_at, half_ballot, the grids

namespace {

constexpr int THREADS = MASK_THREADS;                    // the block of both passes; k_dist_columns runs one column per thread
constexpr uint32_t NONE = SVR_DIST_NONE;
constexpr int OUT_MAP = 0, OUT_LE = 1, OUT_GT = 2;

// one column pass: `rows` groups of nx columns; column (r, x) starts at r * row_stride + x and has n entries `stride` apart.  The
// mask word of level u of the columns of word gw of group r is r * mask_row + u * mask_level + gw.
struct ColPass {
    uint32_t n, rows, nx, wx, w;
    size_t stride, row_stride, mask_row, mask_level, cols;   // cols = rows * nx, the stack's second dimension
};

__device__ inline uint64_t sq_diff(uint32_t a, uint32_t b)
{
    const uint32_t d = a > b ? a - b : b - a;              // below 65536
    return (uint64_t)(d * d);
}

// the target bits of mask word i (word gw of its row): the set voxels, or the unset voxels of the volume
__device__ inline uint32_t target_word(const uint32_t* __restrict__ mask, size_t i, int gw, const RegionDims& d, bool unset)
{
    const uint32_t m = mask[i];
    return (unset ? ~m : m) & valid_bits(gw, d);
}

__global__ __launch_bounds__(THREADS) void k_dist_rows(const uint32_t* __restrict__ mask, uint32_t* __restrict__ out, RegionDims d, size_t words, uint32_t w,
                                                       int unset)
{
    const LaneAt a = lane_at(d, words);
    if (!a.word_ok) return;
    const uint32_t m = target_word(mask, a.i, a.gw, d, unset != 0);
    uint32_t best = 0xffffffffu;                          // the distance in voxels to the nearest target of the row
    const uint32_t left = m & (0xffffffffu >> (31 - a.bit)), right = m & (0xffffffffu << a.bit);
    if (left) best = (uint32_t)(a.bit - (31 - __clz(left)));
    if (right) best = min(best, (uint32_t)(__ffs(right) - 1 - a.bit));
    if (!left)                                            // the nearest non-zero word to the left, while it can still be nearer
        for (int j = a.gw - 1; j >= 0 && (uint32_t)((a.gw - j) * 32 + a.bit - 31) < best; --j) {
            const uint32_t mm = target_word(mask, a.i - (size_t)(a.gw - j), j, d, unset != 0);
            if (mm) { best = min(best, (uint32_t)((a.gw - j) * 32 + a.bit - (31 - __clz(mm)))); break; }
        }
    if (!right)
        for (int j = a.gw + 1; j < d.wx && (uint32_t)((j - a.gw) * 32 - a.bit) < best; ++j) {
            const uint32_t mm = target_word(mask, a.i + (size_t)(j - a.gw), j, d, unset != 0);
            if (mm) { best = min(best, (uint32_t)((j - a.gw) * 32 + __ffs(mm) - 1 - a.bit)); break; }
        }
    if (a.inside) out[a.v] = best == 0xffffffffu ? NONE : w * best * best;
}

// what a column pass does with the value of entry u of its column
template <int MODE>
__device__ inline void emit(uint32_t v, uint32_t u, bool active, size_t at, uint32_t* __restrict__ out, const ColPass& p, uint32_t r2, uint32_t r,
                            uint32_t gw, int bit)
{
    if (MODE == OUT_MAP) {
        if (active) out[at] = v;
    } else {
        const bool on = active && (MODE == OUT_LE ? (v != NONE && v <= r2) : (v == NONE || v > r2));
        const uint32_t word = half_ballot(on);
        if (bit == 0 && r < p.rows) out[(size_t)r * p.mask_row + (size_t)u * p.mask_level + gw] = word;
    }
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void k_dist_columns(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t* __restrict__ stack, ColPass p,
                                                          uint32_t r2)
{
    const size_t t = lane_thread();
    const size_t wi = t >> 5;
    const int bit = (int)(t & 31u);
    const uint32_t gw = (uint32_t)(wi % p.wx);
    const size_t rr = wi / p.wx;
    const uint32_t r = rr < p.rows ? (uint32_t)rr : p.rows;
    const uint32_t x = gw * 32u + (uint32_t)bit;
    const bool active = r < p.rows && x < p.nx;           // (the other lanes of the wave run the loops too: the ballots need them)
    const size_t base = active ? (size_t)r * p.row_stride + x : 0;
    const uint64_t w = p.w;
#ifdef SVR_DISTANCE_BRUTE
    (void)stack;
    for (uint32_t u = 0; u < p.n; ++u) {
        uint64_t best = NONE;
        if (active)
            for (uint32_t i = 0; i < p.n; ++i) {
                const uint32_t g = in[base + (size_t)i * p.stride];
                if (g != NONE) best = min(best, (uint64_t)g + w * sq_diff(u, i));
            }
        emit<MODE>((uint32_t)best, u, active, base + (size_t)u * p.stride, out, p, r2, r, gw, bit);
    }
#else
    uint32_t* const st = stack + (active ? (size_t)r * p.nx + x : 0);       // entry k of this column: st[k * cols]
    int q = -1;                                           // the top of the stack; its entry and its g are kept in registers
    uint32_t s_top = 0u, t_top = 0u, g_top = 0u;
    uint32_t g_next = active ? in[base] : NONE;
    for (uint32_t u = 0; u < p.n; ++u) {
        const uint32_t gu = g_next;
        if (active && u + 1u < p.n) g_next = in[base + (size_t)(u + 1u) * p.stride];
        if (gu == NONE) continue;                         // no parabola here (and none in a lane without a column)
        for (uint32_t pops = 0; q >= 0 && pops <= p.n; ++pops) {
            if ((uint64_t)g_top + w * sq_diff(t_top, s_top) <= (uint64_t)gu + w * sq_diff(t_top, u)) break;   // the top holds its own start
            if (--q >= 0) {
                const uint32_t e = st[(size_t)q * p.cols];
                s_top = e & 0xffffu;
                t_top = e >> 16;
                g_top = in[base + (size_t)s_top * p.stride];
            }
        }
        if (q < 0) {
            q = 0; s_top = u; t_top = 0u; g_top = gu;
            st[0] = u;
        } else {
            // the last coordinate at which s_top is still at least as good as u; s_top wins at t_top >= 0, so the numerator is >= 0
            const uint64_t num = (uint64_t)gu + w * (uint64_t)(u * u - s_top * s_top) - (uint64_t)g_top, den = 2ull * w * (uint64_t)(u - s_top);
            uint64_t sep = (uint64_t)((double)num / (double)den);
            if (sep * den > num) --sep;
            else if ((sep + 1ull) * den <= num) ++sep;
            if (sep + 1ull < (uint64_t)p.n) {
                ++q; s_top = u; t_top = (uint32_t)sep + 1u; g_top = gu;
                st[(size_t)q * p.cols] = (t_top << 16) | u;
            }
        }
    }
    for (uint32_t u = p.n; u-- > 0u;) {
        uint32_t v = NONE;
        if (q >= 0) {
            v = (uint32_t)((uint64_t)g_top + w * sq_diff(u, s_top));
            if (u == t_top && q > 0) {
                const uint32_t e = st[(size_t)(--q) * p.cols];
                s_top = e & 0xffffu;
                t_top = e >> 16;
                g_top = in[base + (size_t)s_top * p.stride];
            }
        }
        emit<MODE>(v, u, active, base + (size_t)u * p.stride, out, p, r2, r, gw, bit);
    }
#endif
}

} // namespace
