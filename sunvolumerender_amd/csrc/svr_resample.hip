// svr_resample.hip -- volumes, masks and label maps on another grid: crop to a box, resample to another spacing or to other dimensions,
// and paste a mask made on a crop back (svr_resample_grid_*, svr_volume_resample, svr_region_resample, _label_resample, _paste,
// _mask_expand, svr_volume_resample_last_ms; the contract is in include/svr_abi.h, the design in DESIGN.md 8p).  Integers only; volumes
// are [nz][ny][nx]; a source index outside the volume is clamped per axis.
//
// THE GRID of an axis is (origin, step, count) in Q16 source edge coordinates: output cell j covers [a, a + step), a = origin + j step.
// GATHER (k_gather<T>): NEAREST on all three axes -- a crop is its special case -- is one kernel for u16 volumes and uint32 maps: the
//   three per-axis selections commute, so the three passes of the definition collapse into one read and one write per output voxel.
// PASSES (k_pass<MODE, ALONG_X>): LINEAR and AREA run one pass per axis that resamples, in the order x, y, z.  A pass resamples its own
//   axis and maps the two others by an integer offset with the clamp, so the axes that only crop are folded into the FIRST pass and cost
//   no pass of their own; later passes see offsets 0.  In a y or z pass a lane owns two x-adjacent columns: every tap is a coalesced
//   row read and the pair is stored as one 32-bit word where its address is 4-byte aligned and both voxels exist, else as u16 stores
//   (with an odd nx every other row starts at an odd u16 offset); the loads follow the same rule.  In an x pass a lane owns one output
//   and gathers its taps along the row.  AREA divides 2 S + step < 2^40 by 2 step <= 2^23 in 64 bits.
// MASKS: k_mask_crop is the funnel form, one output word per lane, for a crop whose x range lies inside the source; k_mask_gather is the
//   general form, one lane per output voxel and a ballot per 32 of them.  k_paste gives one thread one destination word.
//
// No block waits for another, and every loop runs to a bound that the host checked (an AREA cell meets at most 65 source voxels).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"

#include "svr_mask.hpp"
#include "svr_volume_host.hpp"

using svr::failf;

namespace {

constexpr int THREADS = 256;
constexpr uint32_t ROWS = 4;                              // the output rows one block walks

struct Axis { long long origin; uint32_t step; };         // the resampled axis of a pass, the three axes of a gather
struct Dims3 { int n[3]; };                               // x, y, z

__device__ inline int clampi(long long v, int hi) { return v < 0 ? 0 : (v > (long long)hi ? hi : (int)v); }

// the row group of a block: rows row0 .. row0 + ROWS - 1 of `rows` (row = z * ny + y of the OUTPUT)
__device__ inline uint32_t first_row() { return (blockIdx.z * gridDim.y + blockIdx.y) * ROWS; }

// One output (pair) of mode MODE at cell lower edge a: fetch(i, v0, v1) reads the values at the CLAMPED source index i of the axis.
template <int MODE, class F>
__device__ inline void resample_at(long long a, uint32_t step, int last, F fetch, uint32_t& o0, uint32_t& o1)
{
    if (MODE == SVR_RESAMPLE_NEAREST) {
        fetch(clampi((a + (long long)(step >> 1)) >> 16, last), o0, o1);
    } else if (MODE == SVR_RESAMPLE_LINEAR) {
        const long long t = a + (long long)(step >> 1) - 32768;
        const long long i = t >> 16;
        const uint32_t f = (uint32_t)(t & 65535), g = 65536u - f;
        uint32_t p0, p1, q0, q1;
        fetch(clampi(i, last), p0, p1);
        fetch(clampi(i + 1, last), q0, q1);
        o0 = (p0 * g + q0 * f + 32768u) >> 16;            // at most 65535 * 65536 + 32768 < 2^32
        o1 = (p1 * g + q1 * f + 32768u) >> 16;
    } else {
        const long long b = a + (long long)step;
        unsigned long long s0 = 0, s1 = 0;
        for (long long i = a >> 16; i <= (b - 1) >> 16; ++i) {
            const long long lo = i << 16, hi = lo + 65536;
            const uint32_t ov = (uint32_t)((b < hi ? b : hi) - (a > lo ? a : lo));
            uint32_t p0, p1;
            fetch(clampi(i, last), p0, p1);
            s0 += (unsigned long long)p0 * ov;
            s1 += (unsigned long long)p1 * ov;
        }
        o0 = (uint32_t)((2ull * s0 + step) / (2ull * step));
        o1 = (uint32_t)((2ull * s1 + step) / (2ull * step));
    }
}

// One pass along `axis` (ALONG_X: axis 0).  in: src dims; out: dst dims, equal to src on the other axes unless this pass crops them by
// off[] (source index = clamp(output index + off)).  Block (x segment, row group) as k_smooth of svr_filter.hip.
template <int MODE, bool ALONG_X>
__global__ __launch_bounds__(THREADS) void k_pass(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, Dims3 src, Dims3 dst, Axis ax,
                                                  int axis, Dims3 off, uint32_t rows)
{
    const uint32_t row0 = first_row();
    const int sx = src.n[0], sy = src.n[1];
    if (ALONG_X) {
        const int x = (int)(blockIdx.x * THREADS + threadIdx.x);
        if (x >= dst.n[0]) return;
        const long long a = ax.origin + (long long)x * (long long)ax.step;
#pragma unroll 1
        for (uint32_t row = row0; row < row0 + ROWS && row < rows; ++row) {
            const uint32_t z = row / (uint32_t)dst.n[1], y = row - z * (uint32_t)dst.n[1];
            const int qy = clampi((long long)y + off.n[1], sy - 1), qz = clampi((long long)z + off.n[2], src.n[2] - 1);
            const uint16_t* line = in + ((size_t)qz * (size_t)sy + (size_t)qy) * (size_t)sx;
            uint32_t o0, o1;
            resample_at<MODE>(a, ax.step, sx - 1, [&](int i, uint32_t& v0, uint32_t& v1) { v0 = line[i]; v1 = 0u; }, o0, o1);
            out[(size_t)row * (size_t)dst.n[0] + (size_t)x] = (uint16_t)o0;
        }
    } else {
        const int x = 2 * (int)(blockIdx.x * THREADS + threadIdx.x);
        if (x >= dst.n[0]) return;
        const bool two = x + 1 < dst.n[0];
        // the source columns of the pair: adjacent unless the clamp folds them (then they are loaded one by one)
        const int q0 = clampi((long long)x + off.n[0], sx - 1), q1 = clampi((long long)x + 1 + off.n[0], sx - 1);
        const bool adjacent = two && q1 == q0 + 1;
        const int last = src.n[axis] - 1;
#pragma unroll 1
        for (uint32_t row = row0; row < row0 + ROWS && row < rows; ++row) {
            const uint32_t z = row / (uint32_t)dst.n[1], y = row - z * (uint32_t)dst.n[1];
            const long long a = ax.origin + (long long)(axis == 1 ? y : z) * (long long)ax.step;
            // the other axis of the pair (y, z) is an offset copy; the resampled one is set by fetch
            const int fy = clampi((long long)y + off.n[1], sy - 1), fz = clampi((long long)z + off.n[2], src.n[2] - 1);
            auto fetch = [&](int i, uint32_t& v0, uint32_t& v1) {
                const int qy = axis == 1 ? i : fy, qz = axis == 2 ? i : fz;
                const uint16_t* p = in + ((size_t)qz * (size_t)sy + (size_t)qy) * (size_t)sx;
                if (adjacent && ((uintptr_t)(p + q0) & 3u) == 0) {
                    const uint32_t w = *reinterpret_cast<const uint32_t*>(p + q0);
                    v0 = w & 65535u;
                    v1 = w >> 16;
                } else {
                    v0 = p[q0];
                    v1 = p[q1];
                }
            };
            uint32_t o0, o1;
            resample_at<MODE>(a, ax.step, last, fetch, o0, o1);
            uint16_t* q = out + (size_t)row * (size_t)dst.n[0] + (size_t)x;
            if (two && ((uintptr_t)q & 3u) == 0) {
                *reinterpret_cast<uint32_t*>(q) = o0 | (o1 << 16);
            } else {
                q[0] = (uint16_t)o0;
                if (two) q[1] = (uint16_t)o1;
            }
        }
    }
}

// NEAREST on the three axes at once, one thread per output voxel: out(x, y, z) = in(sel_x(x), sel_y(y), sel_z(z))
template <class T>
__global__ __launch_bounds__(THREADS) void k_gather(const T* __restrict__ in, T* __restrict__ out, Dims3 src, Dims3 dst, Axis gx, Axis gy, Axis gz,
                                                    uint32_t rows)
{
    const int x = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (x >= dst.n[0]) return;
    const int qx = clampi((gx.origin + (long long)x * (long long)gx.step + (long long)(gx.step >> 1)) >> 16, src.n[0] - 1);
    const uint32_t row0 = first_row();
#pragma unroll 1
    for (uint32_t row = row0; row < row0 + ROWS && row < rows; ++row) {
        const uint32_t z = row / (uint32_t)dst.n[1], y = row - z * (uint32_t)dst.n[1];
        const int qy = clampi((gy.origin + (long long)y * (long long)gy.step + (long long)(gy.step >> 1)) >> 16, src.n[1] - 1);
        const int qz = clampi((gz.origin + (long long)z * (long long)gz.step + (long long)(gz.step >> 1)) >> 16, src.n[2] - 1);
        out[(size_t)row * (size_t)dst.n[0] + (size_t)x] = in[((size_t)qz * (size_t)src.n[1] + (size_t)qy) * (size_t)src.n[0] + (size_t)qx];
    }
}

// the general mask form: one lane per output voxel (32 lanes a word, svr_mask.hpp), the lane's source bit, a ballot per word
__global__ __launch_bounds__(MASK_THREADS) void k_mask_gather(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, RegionDims src, RegionDims dst,
                                                              Axis gx, Axis gy, Axis gz, size_t words)
{
    const LaneAt l = lane_at(dst, words);
    bool bit = false;
    if (l.inside) {
        const int qx = clampi((gx.origin + (long long)l.x * (long long)gx.step + (long long)(gx.step >> 1)) >> 16, src.nx - 1);
        const int qy = clampi((gy.origin + (long long)l.y * (long long)gy.step + (long long)(gy.step >> 1)) >> 16, src.ny - 1);
        const int qz = clampi((gz.origin + (long long)l.z * (long long)gz.step + (long long)(gz.step >> 1)) >> 16, src.nz - 1);
        bit = (in[((size_t)qz * (size_t)src.ny + (size_t)qy) * (size_t)src.wx + (size_t)(qx >> 5)] >> (qx & 31)) & 1u;
    }
    const uint32_t w = half_ballot(bit);                  // every lane of the wave takes part
    if (l.word_ok && l.bit == 0) out[l.i] = w;
}

// the crop of a mask whose x range lies inside the source: output word gw of a row is source bits ox + 32 gw .. + 31, two words funnelled
__global__ __launch_bounds__(MASK_THREADS) void k_mask_crop(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, RegionDims src, RegionDims dst,
                                                            int ox, int oy, int oz, size_t words)
{
    const size_t i = (size_t)blockIdx.x * MASK_THREADS + threadIdx.x;
    if (i >= words) return;
    const int gw = (int)(i % (unsigned)dst.wx);
    const size_t row = i / (unsigned)dst.wx;
    const int y = (int)(row % (unsigned)dst.ny), z = (int)(row / (unsigned)dst.ny);
    const int qy = clampi((long long)y + oy, src.ny - 1), qz = clampi((long long)z + oz, src.nz - 1);
    const uint32_t* line = in + ((size_t)qz * (size_t)src.ny + (size_t)qy) * (size_t)src.wx;
    const int sx0 = ox + gw * 32, k = sx0 >> 5, s = sx0 & 31;     // 0 <= sx0 < src.nx: the host checked the x range
    const uint32_t lo = line[k], hi = (s != 0 && k + 1 < src.wx) ? line[k + 1] : 0u;
    const uint32_t w = s ? (lo >> s) | (hi << (32 - s)) : lo;
    out[i] = w & valid_bits(gw, dst);                     // the source's padding can only reach bits past the output's width
}

// paste: one thread per word of `full` that the box touches.  t: word index among the touched words of a row, times the box's rows
__global__ __launch_bounds__(MASK_THREADS) void k_paste(const uint32_t* __restrict__ sub, RegionDims ds, uint32_t* __restrict__ full, RegionDims df,
                                                        int ox, int oy, int oz, int gw0, int gws, int op, size_t items)
{
    const size_t t = (size_t)blockIdx.x * MASK_THREADS + threadIdx.x;
    if (t >= items) return;
    const int gw = gw0 + (int)(t % (unsigned)gws);
    const size_t row = t / (unsigned)gws;
    const int y = (int)(row % (unsigned)ds.ny), z = (int)(row / (unsigned)ds.ny);
    const uint32_t* line = sub + ((size_t)z * (size_t)ds.ny + (size_t)y) * (size_t)ds.wx;
    auto sub_word = [&](int k) { return (k >= 0 && k < ds.wx) ? line[k] & valid_bits(k, ds) : 0u; };   // the sub-mask's padding is ignored
    // bit b of the destination word is sub-mask voxel x = gw * 32 + b - ox
    const int rel = gw * 32 - ox;                         // > -32: the word touches the box
    uint32_t bits, box;
    if (rel < 0) {
        bits = sub_word(0) << (-rel);
        box = 0xffffffffu << (-rel);
    } else {
        const int k = rel >> 5, s = rel & 31;
        bits = s ? (sub_word(k) >> s) | (sub_word(k + 1) << (32 - s)) : sub_word(k);
        box = 0xffffffffu;
    }
    const int end = ox + ds.nx - gw * 32;                 // the box ends before bit `end` of this word (>= 1)
    if (end < 32) box &= (1u << end) - 1u;
    bits &= box;
    uint32_t* q = full + ((size_t)(z + oz) * (size_t)df.ny + (size_t)(y + oy)) * (size_t)df.wx + (size_t)gw;
    const uint32_t old = *q;
    *q = op == SVR_PASTE_REPLACE ? (old & ~box) | bits : (op == SVR_MASK_OR ? old | bits : old & ~bits);
}

// one byte per voxel: `value` inside the mask, 0 outside
__global__ __launch_bounds__(MASK_THREADS) void k_expand(const uint32_t* __restrict__ mask, uint8_t* __restrict__ out, RegionDims d, uint32_t value, size_t n)
{
    const size_t v = (size_t)blockIdx.x * MASK_THREADS + threadIdx.x;
    if (v >= n) return;
    const size_t row = v / (unsigned)d.nx;
    const int x = (int)(v - row * (unsigned)d.nx);
    out[v] = (uint8_t)(((mask[row * (size_t)d.wx + (size_t)(x >> 5)] >> (x & 31)) & 1u) ? value : 0u);
}

// ---------------- host side ----------------
CallEvents g_events;                                      // around the device work of the last call of this file (svr_volume_resample_last_ms)

int check_dims3(const char* who, const int32_t* d) { return check_dims(who, d[0], d[1], d[2]); }

bool is_copy(const svr_axis_map& m) { return m.step == 65536u && (m.origin & 65535) == 0; }

// a grid against its source: the -6 of the output dimensions first, then the -3 list of svr_abi.h
int check_grid(const char* who, const int32_t* src, const svr_resample_grid* g)
{
    unsigned long long voxels = 1;
    bool zero = false;
    for (int a = 0; a < 3; ++a) {
        const uint32_t c = g->axis[a].count;
        if (c == 0u) { zero = true; continue; }
        if (c > 0x7fffffffu || (voxels *= c) > (1ull << 31))
            return failf(-6, "%s: the output %u x %u x %u is more than 2^31 voxels", who, g->axis[0].count, g->axis[1].count, g->axis[2].count);
    }
    for (int a = 0; a < 3; ++a) {
        const svr_axis_map& m = g->axis[a];
        if (m.step < SVR_RESAMPLE_MIN_STEP || m.step > SVR_RESAMPLE_MAX_STEP)
            return failf(-3, "%s: the step %u of axis %d lies outside %u .. %u", who, m.step, a, SVR_RESAMPLE_MIN_STEP, SVR_RESAMPLE_MAX_STEP);
        if (zero && m.count == 0u) return failf(-3, "%s: the count of axis %d is 0", who, a);
        if (m.origin >= (1ll << 47) || m.origin <= -(1ll << 47)) return failf(-3, "%s: the origin %lld of axis %d is 2^47 or more in size", who, (long long)m.origin, a);
        const long long end = m.origin + (long long)m.count * (long long)m.step;     // below 2^47 + 2^54
        if (end <= 0 || m.origin >= ((long long)src[a] << 16))
            return failf(-3, "%s: the cells of axis %d, %lld .. %lld, do not meet the source extent 0 .. %lld", who, a, (long long)m.origin, end,
                         (long long)src[a] << 16);
    }
    return 0;
}

Dims3 grid_dims(const svr_resample_grid* g) { return Dims3{{(int)g->axis[0].count, (int)g->axis[1].count, (int)g->axis[2].count}}; }
size_t voxels_of(const Dims3& d) { return (size_t)d.n[0] * (size_t)d.n[1] * (size_t)d.n[2]; }
Axis axis_of(const svr_axis_map& m) { return Axis{(long long)m.origin, m.step}; }

// blocks of THREADS items along x, row groups of ROWS in y and z
dim3 row_grid(uint32_t items_x, uint32_t rows)
{
    const uint32_t groups = (rows + ROWS - 1) / ROWS;
    const uint32_t gy = groups < 65535u ? groups : 65535u, gz = (groups + gy - 1) / gy;
    return dim3((items_x + THREADS - 1) / THREADS, gy, gz);
}

void launch_pass(int mode, int axis, hipStream_t st, const uint16_t* in, uint16_t* out, const Dims3& src, const Dims3& dst, const Axis& ax, const Dims3& off)
{
    const uint32_t rows = (uint32_t)((size_t)dst.n[1] * (size_t)dst.n[2]);
    const dim3 grid = row_grid(axis == 0 ? (uint32_t)dst.n[0] : ((uint32_t)dst.n[0] + 1u) / 2u, rows);
#define PASS_CASE(M)                                                                                                                    \
    case M:                                                                                                                             \
        if (axis == 0) hipLaunchKernelGGL((k_pass<M, true>), grid, dim3(THREADS), 0, st, in, out, src, dst, ax, axis, off, rows);       \
        else hipLaunchKernelGGL((k_pass<M, false>), grid, dim3(THREADS), 0, st, in, out, src, dst, ax, axis, off, rows);                \
        break
    switch (mode) {
        PASS_CASE(SVR_RESAMPLE_NEAREST); PASS_CASE(SVR_RESAMPLE_LINEAR); PASS_CASE(SVR_RESAMPLE_AREA);
        default: break;
    }
#undef PASS_CASE
}

template <class T>
void launch_gather(hipStream_t st, const T* in, T* out, const Dims3& src, const svr_resample_grid* g)
{
    const Dims3 dst = grid_dims(g);
    const uint32_t rows = (uint32_t)((size_t)dst.n[1] * (size_t)dst.n[2]);
    hipLaunchKernelGGL((k_gather<T>), row_grid((uint32_t)dst.n[0], rows), dim3(THREADS), 0, st, in, out, src, dst, axis_of(g->axis[0]),
                       axis_of(g->axis[1]), axis_of(g->axis[2]), rows);
}

// the box argument of the grid helpers: NULL pointers mean the whole volume
int helper_box(const char* who, const int32_t* src, const int32_t* box_min, const int32_t* box_max, int b0[3], int b1[3])
{
    int32_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = box_min ? box_min[a] : 0;
        hi[a] = box_max ? box_max[a] : src[a] - 1;
    }
    return clamp_box(who, lo, hi, src[0], src[1], src[2], b0, b1);
}

} // namespace

extern "C" {

int svr_resample_grid_box(const int32_t src_dims[3], const int32_t box_min[3], const int32_t box_max[3], svr_resample_grid* grid)
{
    const char* who = "svr_resample_grid_box";
    if (!src_dims || !box_min || !box_max || !grid) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, src_dims)) return e;
    int b0[3], b1[3];
    if (int e = clamp_box(who, box_min, box_max, src_dims[0], src_dims[1], src_dims[2], b0, b1)) return e;
    for (int a = 0; a < 3; ++a) grid->axis[a] = svr_axis_map{(int64_t)b0[a] << 16, 65536u, (uint32_t)(b1[a] - b0[a] + 1)};
    return 0;
}

int svr_resample_grid_spacing(const int32_t src_dims[3], const double src_spacing[3], const int32_t* box_min_or_null, const int32_t* box_max_or_null,
                              const double target_spacing[3], svr_resample_grid* grid, double* spacing_out)
{
    const char* who = "svr_resample_grid_spacing";
    if (!src_dims || !src_spacing || !target_spacing || !grid) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, src_dims)) return e;
    for (int a = 0; a < 3; ++a)
        if (!(src_spacing[a] > 0.0) || !std::isfinite(src_spacing[a]) || !(target_spacing[a] > 0.0) || !std::isfinite(target_spacing[a]))
            return failf(-3, "%s: the spacings must be positive and finite (axis %d: source %g, target %g)", who, a, src_spacing[a], target_spacing[a]);
    int b0[3], b1[3];
    if (int e = helper_box(who, src_dims, box_min_or_null, box_max_or_null, b0, b1)) return e;
    svr_resample_grid g;
    for (int a = 0; a < 3; ++a) {
        const double r = 65536.0 * target_spacing[a] / src_spacing[a];
        const long long step = (r < 1e12) ? std::llround(r) : (1ll << 40);
        if (step < (long long)SVR_RESAMPLE_MIN_STEP || step > (long long)SVR_RESAMPLE_MAX_STEP)
            return failf(-3, "%s: the target spacing %g at the source spacing %g needs the step %lld on axis %d, outside %u .. %u", who, target_spacing[a],
                         src_spacing[a], step, a, SVR_RESAMPLE_MIN_STEP, SVR_RESAMPLE_MAX_STEP);
        const long long count = ((long long)(b1[a] - b0[a] + 1) * 65536 + (step >> 1)) / step;
        g.axis[a] = svr_axis_map{(int64_t)b0[a] << 16, (uint32_t)step, (uint32_t)(count < 1 ? 1 : count)};
    }
    if (int e = check_grid(who, src_dims, &g)) return e;
    *grid = g;
    if (spacing_out)
        for (int a = 0; a < 3; ++a) spacing_out[a] = src_spacing[a] * (double)g.axis[a].step / 65536.0;
    return 0;
}

int svr_resample_grid_dims(const int32_t src_dims[3], const int32_t* box_min_or_null, const int32_t* box_max_or_null, const int32_t out_dims[3],
                           svr_resample_grid* grid)
{
    const char* who = "svr_resample_grid_dims";
    if (!src_dims || !out_dims || !grid) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, src_dims)) return e;
    if (int e = check_dims3(who, out_dims)) return e;
    int b0[3], b1[3];
    if (int e = helper_box(who, src_dims, box_min_or_null, box_max_or_null, b0, b1)) return e;
    svr_resample_grid g;
    for (int a = 0; a < 3; ++a) {
        const long long step = ((long long)(b1[a] - b0[a] + 1) * 65536 + out_dims[a] / 2) / out_dims[a];
        if (step < (long long)SVR_RESAMPLE_MIN_STEP || step > (long long)SVR_RESAMPLE_MAX_STEP)
            return failf(-3, "%s: %d output voxels for %d source voxels need the step %lld on axis %d, outside %u .. %u", who, (int)out_dims[a],
                         b1[a] - b0[a] + 1, step, a, SVR_RESAMPLE_MIN_STEP, SVR_RESAMPLE_MAX_STEP);
        g.axis[a] = svr_axis_map{(int64_t)b0[a] << 16, (uint32_t)step, (uint32_t)out_dims[a]};
    }
    if (int e = check_grid(who, src_dims, &g)) return e;
    *grid = g;
    return 0;
}

int svr_resample_grid_place(const svr_volume* src, const int32_t src_dims[3], const svr_resample_grid* grid, svr_volume* out)
{
    const char* who = "svr_resample_grid_place";
    if (!src || !src_dims || !grid || !out) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, src_dims)) return e;
    if (int e = check_grid(who, src_dims, grid)) return e;
    svr_volume v = *src;
    const float vmin[3] = {src->bbox.vmin.x, src->bbox.vmin.y, src->bbox.vmin.z}, sp[3] = {src->spacing.x, src->spacing.y, src->spacing.z};
    float lo[3], hi[3], inv[3], s[3], is[3];
    for (int a = 0; a < 3; ++a) {
        const svr_axis_map& m = grid->axis[a];
        const double e0 = (double)m.origin / 65536.0, e1 = ((double)m.origin + (double)m.count * (double)m.step) / 65536.0;
        lo[a] = (float)((double)vmin[a] + e0 * (double)sp[a]);
        hi[a] = (float)((double)vmin[a] + e1 * (double)sp[a]);
        inv[a] = 1.f / (hi[a] - lo[a]);
        s[a] = (float)((double)sp[a] * (double)m.step / 65536.0);
        is[a] = 1.f / s[a];
    }
    v.bbox.vmin = svr_vec3{lo[0], lo[1], lo[2]};
    v.bbox.vmax = svr_vec3{hi[0], hi[1], hi[2]};
    v.bbox.invSize = svr_vec3{inv[0], inv[1], inv[2]};
    v.spacing = svr_vec3{s[0], s[1], s[2]};
    v.invSpacing = svr_vec3{is[0], is[1], is[2]};
    *out = v;
    return 0;
}

int svr_volume_resample(const uint16_t* voxels, const int32_t src_dims[3], int src_is_device, const svr_resample_grid* grid, int mode,
                        uint16_t* out_u16_device)
{
    const char* who = "svr_volume_resample";
    if (!voxels || !src_dims || !grid || !out_u16_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, src_dims)) return e;
    if (int e = check_grid(who, src_dims, grid)) return e;
    if (mode != SVR_RESAMPLE_NEAREST && mode != SVR_RESAMPLE_LINEAR && mode != SVR_RESAMPLE_AREA && mode != SVR_RESAMPLE_AUTO)
        return failf(-3, "%s: unknown mode %d", who, mode);
    const Dims3 src{{src_dims[0], src_dims[1], src_dims[2]}}, dst = grid_dims(grid);
    const size_t n = voxels_of(src);
    if (src_is_device && overlap(voxels, n * sizeof(uint16_t), out_u16_device, voxels_of(dst) * sizeof(uint16_t)))
        return failf(-3, "%s: out must not overlap voxels", who);
    // the passes: the axes that are not a shifted copy, each with its own mode
    int axes[3], modes[3], passes = 0;
    for (int a = 0; a < 3; ++a)
        if (!is_copy(grid->axis[a])) {
            modes[passes] = mode != SVR_RESAMPLE_AUTO ? mode : (grid->axis[a].step <= 65536u ? SVR_RESAMPLE_LINEAR : SVR_RESAMPLE_AREA);
            axes[passes++] = a;
        }
    const bool gather = mode == SVR_RESAMPLE_NEAREST || passes == 0;
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    DeviceVoxels dv;
    DeviceBuffer tmp[2];
    SVR_HIP_TRY(dv.get(voxels, n, src_is_device, st));
    // the volume after pass i: the resampled axes so far and every copy axis at the output's size, the others at the source's
    Dims3 mid[3];
    if (!gather) {
        Dims3 d = src;
        for (int a = 0; a < 3; ++a)
            if (is_copy(grid->axis[a])) d.n[a] = dst.n[a];
        for (int i = 0; i < passes; ++i) {
            d.n[axes[i]] = dst.n[axes[i]];
            mid[i] = d;
            if (i + 1 < passes) SVR_HIP_TRY(tmp[i].alloc(voxels_of(d) * sizeof(uint16_t)));
        }
    }
    CallTimer timer(g_events, st);
    if (gather) {
        launch_gather<uint16_t>(st, dv.p, out_u16_device, src, grid);
    } else {
        const uint16_t* in = dv.p;
        Dims3 from = src;
        for (int i = 0; i < passes; ++i) {
            Dims3 off{{0, 0, 0}};
            if (i == 0)
                for (int a = 0; a < 3; ++a)
                    if (is_copy(grid->axis[a])) off.n[a] = (int)(grid->axis[a].origin >> 16);    // |origin >> 16| < 2^31: check_grid's extent test
            uint16_t* to = i + 1 < passes ? tmp[i].as<uint16_t>() : out_u16_device;
            launch_pass(modes[i], axes[i], st, in, to, from, mid[i], axis_of(grid->axis[axes[i]]), off);
            in = to;
            from = mid[i];
        }
    }
    SVR_HIP_TRY(hipGetLastError());
    timer.stop();
    if (dv.owned() || tmp[0]) SVR_HIP_TRY(hipStreamSynchronize(st));      // the upload and the temporaries are freed on return
    return 0;
}

int svr_region_resample(const uint32_t* in_mask_device, const int32_t src_dims[3], const svr_resample_grid* grid, uint32_t* out_mask_device)
{
    const char* who = "svr_region_resample";
    if (!in_mask_device || !src_dims || !grid || !out_mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, src_dims)) return e;
    if (int e = check_grid(who, src_dims, grid)) return e;
    const RegionDims ds = make_dims(src_dims[0], src_dims[1], src_dims[2]);
    const RegionDims dd = make_dims((int)grid->axis[0].count, (int)grid->axis[1].count, (int)grid->axis[2].count);
    const size_t words = mask_words(dd);
    if (overlap(in_mask_device, mask_words(ds) * 4, out_mask_device, words * 4)) return failf(-3, "%s: out must not overlap the input mask", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const svr_axis_map* m = grid->axis;
    // the funnel form: a crop whose x range lies inside the source (y and z may still clamp)
    const bool crop = is_copy(m[0]) && is_copy(m[1]) && is_copy(m[2]) && m[0].origin >= 0 && (m[0].origin >> 16) + (long long)m[0].count <= (long long)ds.nx;
    CallTimer timer(g_events, st);
    if (crop)
        hipLaunchKernelGGL(k_mask_crop, word_grid(words), dim3(MASK_THREADS), 0, st, in_mask_device, out_mask_device, ds, dd, (int)(m[0].origin >> 16),
                           (int)(m[1].origin >> 16), (int)(m[2].origin >> 16), words);
    else
        hipLaunchKernelGGL(k_mask_gather, lane_grid(words), dim3(MASK_THREADS), 0, st, in_mask_device, out_mask_device, ds, dd, axis_of(m[0]), axis_of(m[1]),
                           axis_of(m[2]), words);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_region_label_resample(const uint32_t* in_u32_device, const int32_t src_dims[3], const svr_resample_grid* grid, uint32_t* out_u32_device)
{
    const char* who = "svr_region_label_resample";
    if (!in_u32_device || !src_dims || !grid || !out_u32_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, src_dims)) return e;
    if (int e = check_grid(who, src_dims, grid)) return e;
    const Dims3 src{{src_dims[0], src_dims[1], src_dims[2]}};
    if (overlap(in_u32_device, voxels_of(src) * 4, out_u32_device, voxels_of(grid_dims(grid)) * 4)) return failf(-3, "%s: out must not overlap the input map", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    launch_gather<uint32_t>(st, in_u32_device, out_u32_device, src, grid);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_region_paste(const uint32_t* sub_mask_device, const int32_t sub_dims[3], uint32_t* full_mask_device, const int32_t full_dims[3],
                     const int32_t offset_xyz[3], int op)
{
    const char* who = "svr_region_paste";
    if (!sub_mask_device || !sub_dims || !full_mask_device || !full_dims || !offset_xyz) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, sub_dims)) return e;
    if (int e = check_dims3(who, full_dims)) return e;
    for (int a = 0; a < 3; ++a)
        if (offset_xyz[a] < 0 || (long long)offset_xyz[a] + sub_dims[a] > (long long)full_dims[a])
            return failf(-3, "%s: %d voxels at offset %d do not fit the %d of axis %d", who, (int)sub_dims[a], (int)offset_xyz[a], (int)full_dims[a], a);
    if (op != SVR_PASTE_REPLACE && op != SVR_MASK_OR && op != SVR_MASK_ANDNOT) return failf(-3, "%s: unknown op %d", who, op);
    const RegionDims ds = make_dims(sub_dims[0], sub_dims[1], sub_dims[2]), df = make_dims(full_dims[0], full_dims[1], full_dims[2]);
    if (overlap(sub_mask_device, mask_words(ds) * 4, full_mask_device, mask_words(df) * 4)) return failf(-3, "%s: the full mask must not overlap the sub-mask", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const int gw0 = offset_xyz[0] >> 5, gws = ((offset_xyz[0] + ds.nx - 1) >> 5) - gw0 + 1;
    const size_t items = (size_t)gws * (size_t)ds.ny * (size_t)ds.nz;
    CallTimer timer(g_events, st);
    hipLaunchKernelGGL(k_paste, word_grid(items), dim3(MASK_THREADS), 0, st, sub_mask_device, ds, full_mask_device, df, (int)offset_xyz[0], (int)offset_xyz[1],
                       (int)offset_xyz[2], gw0, gws, op, items);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_region_mask_expand(const uint32_t* mask_device, const int32_t dims[3], int value, uint8_t* out_u8_device)
{
    const char* who = "svr_region_mask_expand";
    if (!mask_device || !dims || !out_u8_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, dims)) return e;
    if (value < 1 || value > 255) return failf(-3, "%s: the value must lie in 1 .. 255 (got %d)", who, value);
    const RegionDims d = make_dims(dims[0], dims[1], dims[2]);
    const size_t n = (size_t)d.nx * (size_t)d.ny * (size_t)d.nz;
    if (overlap(mask_device, mask_words(d) * 4, out_u8_device, n)) return failf(-3, "%s: out must not overlap the mask", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    hipLaunchKernelGGL(k_expand, word_grid(n), dim3(MASK_THREADS), 0, st, mask_device, out_u8_device, d, (uint32_t)value, n);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_volume_resample_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_volume_resample_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

} // extern "C"
