// svr_smooth.hip -- smoothing of region masks and label maps: the box count, the majority (binary median) filter, binomial smoothing
// of a mask and the mode filter of a label map (svr_region_box_size, _smooth_radii, _box_count, _box_density, _smooth, _label_smooth,
// _smooth_last_ms; the contract is in include/svr_abi.h, the design in DESIGN.md 8w).  Integers only, on the mask layout and padding
// rule of svr_mask.hpp; the border replicates (an index outside the volume is clamped per axis), so a window always holds its N =
// (2rx+1)(2ry+1)(2rz+1) values.
//
// BIT-SLICED COUNTERS: a number per voxel is held as P words, plane p holding bit p of the numbers of the 32 voxels of one mask word.
//   Two such numbers are added by a ripple of full adders on whole words (full_add, planes_add), compared by a ripple over the planes.
// TILE COUNT (tile_count<PX, PY, PZ>): a block of 256 threads owns a tile of 4 words x 8 rows x 8 slices.  It loads the tile with a
//   halo of one word in x and ry rows, rz slices into LDS -- the clamp happens there, once per cell; a word left of the row is filled
//   with the row's voxel 0, a word right of it and the padding of the last word with voxel nx - 1, so the x pass knows no border --
//   and makes the three passes there: x (the 2rx+1 funnel-shifted words, the pair +-k entering through one full adder, into PX
//   planes), y (the 2ry+1 rows of x counts added into PY planes), z (the 2rz+1 slices of xy counts added into PZ planes, in the
//   registers of the thread that owns the word).  The xy counts overlay the loaded words.  PX, PY, PZ follow the largest radius: (2,
//   4, 5) up to 1, (3, 6, 9) up to 3, (5, 9, 13) up to 8.  No counter goes through global memory.
// MAJORITY (k_box<.., false>): the count is compared with (N - 1) / 2 by a ripple over the planes; the result is the mask word.
// COUNT (k_box<.., true>): the planes go to LDS and are gathered per voxel, so the u16 stores are coalesced; the density form scales
//   the value there.
// BINOMIAL: literally E = 65535 on the set voxels (k_expand), svr_volume_smooth(E), >= 32768 (k_upper_half).  The call is the public
//   one: it allocates its own temporary per iteration and its time becomes svr_volume_filter_last_ms; an error of it is reported
//   under this call's name.
// MODE (k_label_mode): k_label_planes transposes the labels (values above `count` read as 0) into bits(count) planes in mask layout;
//   a class's membership word is the AND of the planes or their complements.  A tile first takes the OR of "a voxel has bit b set" and
//   of "a voxel has bit b clear" over its halo: a class that contradicts them is absent, and when no bit is free the halo holds one
//   label and the tile is written without counting.  Otherwise the classes go through tile_count in ascending order; an empty
//   membership tile is skipped; best count, best label and the centre's own count stay bit-sliced (compare and select on words); the
//   strict > keeps the smallest label, and the centre's label wins where its count equals the best.
//
// No block waits for another; the only atomic is the one of the `changed` reductions.  Index arithmetic is size_t.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"

#include "svr_mask.hpp"
#include "svr_volume_host.hpp"

using svr::failf;

namespace {

constexpr int THREADS = MASK_THREADS;
constexpr int TW = 4, TY = 8, TZ = 8;                     // the tile in words, rows, slices: a thread per word
static_assert(TW * TY * TZ == THREADS, "a thread owns one word of the tile");
constexpr int MAX_PLANES = 13;                            // 17^3 = 4913 < 2^13
constexpr int LABEL_PLANES = 8;                           // count <= 255

struct BoxGeo { RegionDims d; int rx, ry, rz, ntx, nty; uint32_t half, n; };    // half = (N - 1) / 2: set iff count > half; n = N

__device__ inline int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ inline void full_add(uint32_t a, uint32_t b, uint32_t c, uint32_t& sum, uint32_t& carry)
{
    const uint32_t t = a ^ b;
    sum = t ^ c;
    carry = (a & b) | (c & t);
}

// acc += v on bit-sliced numbers; the sum fits PA planes by construction
template <int PA, int PV>
__device__ inline void planes_add(uint32_t (&acc)[PA], const uint32_t (&v)[PV])
{
    static_assert(PV <= PA, "the accumulator is the wider number");
    uint32_t carry = 0u;
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        if (p < PV) {
            uint32_t s, k;
            full_add(acc[p], v[p], carry, s, k);
            acc[p] = s;
            carry = k;
        } else {
            const uint32_t s = acc[p] ^ carry;
            carry &= acc[p];
            acc[p] = s;
        }
    }
}

// word gw of a row of wx words, gw in -1 .. anything: the row continued past both ends by its edge voxels.  word(w) gives word w of
// the row, 0 <= w < wx, whatever its padding holds
template <class Word>
__device__ inline uint32_t ext_word(Word word, int gw, const RegionDims& d)
{
    if (gw < 0) return (word(0) & 1u) ? 0xffffffffu : 0u;
    const int last = d.wx - 1;
    if (gw < last) return word(gw);
    const uint32_t lw = word(last), vb = valid_bits(last, d);
    const bool edge = ((lw >> ((d.nx - 1) & 31)) & 1u) != 0u;
    if (gw > last) return edge ? 0xffffffffu : 0u;
    return edge ? (lw | ~vb) : (lw & vb);
}

struct TileAt { int w0, y0, z0; };
__device__ inline TileAt tile_at(const BoxGeo& g)
{
    const size_t tile = blockIdx.x;
    return TileAt{(int)(tile % (unsigned)g.ntx) * TW, (int)((tile / (unsigned)g.ntx) % (unsigned)g.nty) * TY,
                  (int)(tile / ((size_t)g.ntx * (unsigned)g.nty)) * TZ};
}

// the LDS of a tile, in words: [0, low) the loaded words and later the xy counts, [low, low + PX * cells_a) the x counts
struct TileLds { int hy, hz, cells_in, cells_a, cells_b, low; };
template <int PX, int PY>
__host__ __device__ inline TileLds tile_lds(int ry, int rz)
{
    TileLds t;
    t.hy = TY + 2 * ry;
    t.hz = TZ + 2 * rz;
    t.cells_in = (TW + 2) * t.hy * t.hz;
    t.cells_a = TW * t.hy * t.hz;
    t.cells_b = TW * TY * t.hz;
    t.low = t.cells_in > PY * t.cells_b ? t.cells_in : PY * t.cells_b;
    return t;
}
template <int PX, int PY>
inline size_t tile_lds_bytes(int ry, int rz)
{
    const TileLds t = tile_lds<PX, PY>(ry, rz);
    const size_t words = (size_t)t.low + (size_t)PX * t.cells_a, out_stage = (size_t)MAX_PLANES * THREADS;
    return (words > out_stage ? words : out_stage) * sizeof(uint32_t);
}

// loads the tile's words with their halo: cell i of [hz][hy][TW + 2].  row_word(row, w): word w of row `row` = z * ny + y.
// Returns whether this thread loaded a set bit.  The caller synchronises.
template <class RowWord>
__device__ inline bool tile_load(uint32_t* lds, const BoxGeo& g, const TileLds& t, const TileAt& at, RowWord row_word)
{
    bool any = false;
    for (int i = threadIdx.x; i < t.cells_in; i += THREADS) {
        const int hx = i % (TW + 2), hy = (i / (TW + 2)) % t.hy, hz = i / ((TW + 2) * t.hy);
        const int gy = clampi(at.y0 + hy - g.ry, g.d.ny - 1), gz = clampi(at.z0 + hz - g.rz, g.d.nz - 1);
        const size_t row = (size_t)gz * (size_t)g.d.ny + (size_t)gy;
        const uint32_t m = ext_word([&](int w) { return row_word(row, w); }, at.w0 + hx - 1, g.d);
        lds[i] = m;
        any |= m != 0u;
    }
    return any;
}

// the three passes on a loaded tile (synchronised by the caller): c = the count of this thread's word.  Ends with LDS still being read
// by other threads: the caller synchronises before it writes LDS again.
template <int PX, int PY, int PZ>
__device__ inline void tile_count(uint32_t* lds, const BoxGeo& g, const TileLds& t, uint32_t (&c)[PZ])
{
    uint32_t* const xs = lds + t.low;                     // x counts: plane p of cell i of [hz][hy][TW] at xs[p * cells_a + i]
    uint32_t* const xy = lds;                             // xy counts: plane p of cell i of [hz][TY][TW] at xy[p * cells_b + i]
    for (int i = threadIdx.x; i < t.cells_a; i += THREADS) {
        const uint32_t* w = lds + (i / TW) * (TW + 2) + i % TW;
        const uint32_t prev = w[0], cur = w[1], next = w[2];
        uint32_t a[PX];
        a[0] = cur;
#pragma unroll
        for (int p = 1; p < PX; ++p) a[p] = 0u;
#pragma unroll 1
        for (int k = 1; k <= g.rx; ++k) {
            const uint32_t left = __builtin_amdgcn_alignbit(cur, prev, 32 - k), right = __builtin_amdgcn_alignbit(next, cur, k);   // voxels x - k, x + k
            uint32_t carry;
            full_add(a[0], left, right, a[0], carry);
#pragma unroll
            for (int p = 1; p < PX; ++p) {
                const uint32_t s = a[p] ^ carry;
                carry &= a[p];
                a[p] = s;
            }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) xs[p * t.cells_a + i] = a[p];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < t.cells_b; i += THREADS) {
        const int hx = i % TW, ly = (i / TW) % TY, hz = i / (TW * TY);
        uint32_t acc[PY];
#pragma unroll
        for (int p = 0; p < PY; ++p) acc[p] = 0u;
#pragma unroll 1
        for (int dy = 0; dy <= 2 * g.ry; ++dy) {
            const int j = (hz * t.hy + ly + dy) * TW + hx;
            uint32_t v[PX];
#pragma unroll
            for (int p = 0; p < PX; ++p) v[p] = xs[p * t.cells_a + j];
            planes_add(acc, v);
        }
#pragma unroll
        for (int p = 0; p < PY; ++p) xy[p * t.cells_b + i] = acc[p];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < PZ; ++p) c[p] = 0u;
#pragma unroll 1
    for (int dz = 0; dz <= 2 * g.rz; ++dz) {
        const int j = dz * (TW * TY) + (int)threadIdx.x;   // cell (lz + dz, ly, lx) of the xy counts
        uint32_t v[PY];
#pragma unroll
        for (int p = 0; p < PY; ++p) v[p] = xy[p * t.cells_b + j];
        planes_add(c, v);
    }
}

// the numbers of the tile, `planes` planes at lds[p * THREADS + cell], to one value per voxel, x fastest: two tile rows per trip.
// scale_n != 0: the value v is stored as floor(65535 v / scale_n)
template <class T>
__device__ inline void tile_store_values(const uint32_t* lds, int planes, const BoxGeo& g, const TileAt& at, T* out, uint32_t scale_n = 0u)
{
    const int xin = threadIdx.x % (TW * 32), gx = at.w0 * 32 + xin;
#pragma unroll 1
    for (int r = threadIdx.x / (TW * 32); r < TY * TZ; r += THREADS / (TW * 32)) {
        const int gy = at.y0 + r % TY, gz = at.z0 + r / TY;
        if (gx >= g.d.nx || gy >= g.d.ny || gz >= g.d.nz) continue;
        const uint32_t* w = lds + r * TW + xin / 32;
        uint32_t v = 0u;
        for (int p = 0; p < planes; ++p) v |= ((w[p * THREADS] >> (xin & 31)) & 1u) << p;
        if (scale_n) v = v * 65535u / scale_n;            // v <= scale_n <= 4913
        out[((size_t)gz * (size_t)g.d.ny + (size_t)gy) * (size_t)g.d.nx + (size_t)gx] = (T)v;
    }
}

template <int PX, int PY, int PZ, bool COUNT>
__global__ __launch_bounds__(THREADS) void k_box(const uint32_t* __restrict__ in, uint32_t* __restrict__ out_mask, uint16_t* __restrict__ out_count,
                                                 uint32_t scale_n, BoxGeo g)
{
    extern __shared__ uint32_t lds[];
    const TileLds t = tile_lds<PX, PY>(g.ry, g.rz);
    const TileAt at = tile_at(g);
    tile_load(lds, g, t, at, [&](size_t row, int w) { return in[row * (size_t)g.d.wx + (size_t)w]; });
    __syncthreads();
    uint32_t c[PZ];
    tile_count<PX, PY, PZ>(lds, g, t, c);
    if (COUNT) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < PZ; ++p) lds[p * THREADS + threadIdx.x] = c[p];
        __syncthreads();
        tile_store_values(lds, PZ, g, at, out_count, scale_n);
        return;
    }
    const int tid = threadIdx.x;
    const int gw = at.w0 + tid % TW, gy = at.y0 + (tid / TW) % TY, gz = at.z0 + tid / (TW * TY);
    if (gw >= g.d.wx || gy >= g.d.ny || gz >= g.d.nz) return;
    uint32_t gt = 0u;                                     // count > half, from the lowest plane up: a higher plane that differs decides
#pragma unroll
    for (int p = 0; p < PZ; ++p) gt = ((g.half >> p) & 1u) ? (c[p] & gt) : (c[p] | gt);
    out_mask[((size_t)gz * (size_t)g.d.ny + (size_t)gy) * (size_t)g.d.wx + (size_t)gw] = gt & valid_bits(gw, g.d);
}

// plane b of the labels: bit b of every voxel's label, a label above `count` read as 0; padding bits 0
__global__ __launch_bounds__(THREADS) void k_label_planes(const uint32_t* __restrict__ labels, uint32_t count, int nplanes, RegionDims d, size_t words,
                                                          uint32_t* __restrict__ planes)
{
    const LaneAt a = lane_at(d, words);
    uint32_t l = a.inside ? labels[a.v] : 0u;
    if (l > count) l = 0u;
    for (int b = 0; b < nplanes; ++b) {
        const uint32_t w = half_ballot(((l >> b) & 1u) != 0u);
        if (a.word_ok && a.bit == 0) planes[(size_t)b * words + a.i] = w;
    }
}

// the voxels of class l in a word whose label planes are p[0 .. nplanes)
__device__ inline uint32_t class_word(const uint32_t* p, size_t stride, int nplanes, uint32_t l)
{
    uint32_t m = 0xffffffffu;
    for (int b = 0; b < nplanes; ++b) m &= ((l >> b) & 1u) ? p[(size_t)b * stride] : ~p[(size_t)b * stride];
    return m;
}

template <int PX, int PY, int PZ>
__global__ __launch_bounds__(THREADS) void k_label_mode(const uint32_t* __restrict__ planes, int nplanes, uint32_t count, size_t words,
                                                        uint32_t* __restrict__ out, BoxGeo g)
{
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t s_seen[THREADS / 64][2];
    const TileLds t = tile_lds<PX, PY>(g.ry, g.rz);
    const TileAt at = tile_at(g);
    const int tid = threadIdx.x;

    // which bits are set in some voxel of the halo, which are clear in some voxel (clamped cells repeat voxels, they bring no label)
    uint32_t ones = 0u, zeros = 0u;
    for (int i = tid; i < t.cells_in; i += THREADS) {
        const int hx = i % (TW + 2), hy = (i / (TW + 2)) % t.hy, hz = i / ((TW + 2) * t.hy);
        const int gw = clampi(at.w0 + hx - 1, g.d.wx - 1), gy = clampi(at.y0 + hy - g.ry, g.d.ny - 1), gz = clampi(at.z0 + hz - g.rz, g.d.nz - 1);
        const uint32_t* p = planes + ((size_t)gz * (size_t)g.d.ny + (size_t)gy) * (size_t)g.d.wx + (size_t)gw;
        const uint32_t vb = valid_bits(gw, g.d);
        for (int b = 0; b < nplanes; ++b) {
            const uint32_t w = p[(size_t)b * words];
            ones |= (w & vb) ? 1u << b : 0u;
            zeros |= (~w & vb) ? 1u << b : 0u;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        ones |= __shfl_xor(ones, o);
        zeros |= __shfl_xor(zeros, o);
    }
    if ((tid & 63) == 0) { s_seen[tid >> 6][0] = ones; s_seen[tid >> 6][1] = zeros; }
    __syncthreads();
    ones = zeros = 0u;
    for (int w = 0; w < THREADS / 64; ++w) { ones |= s_seen[w][0]; zeros |= s_seen[w][1]; }
    const uint32_t all = (1u << nplanes) - 1u, must = ones & ~zeros, free_bits = ones & zeros;   // a present label is `must` | a subset of free_bits

    const int gw = at.w0 + tid % TW, gy = at.y0 + (tid / TW) % TY, gz = at.z0 + tid / (TW * TY);
    const bool mine = gw < g.d.wx && gy < g.d.ny && gz < g.d.nz;
    uint32_t ob[LABEL_PLANES];                            // the planes of the result
    if (free_bits == 0u) {                                // one label in the whole halo: it is every window's mode
#pragma unroll
        for (int b = 0; b < LABEL_PLANES; ++b) ob[b] = ((must >> b) & 1u) ? 0xffffffffu : 0u;
    } else {
        uint32_t own[LABEL_PLANES];                       // the label planes of this thread's word
#pragma unroll
        for (int b = 0; b < LABEL_PLANES; ++b)
            own[b] = (mine && b < nplanes) ? planes[(size_t)b * words + ((size_t)gz * (size_t)g.d.ny + (size_t)gy) * (size_t)g.d.wx + (size_t)gw] : 0u;
        uint32_t best[PZ], centre[PZ], label[LABEL_PLANES];
#pragma unroll
        for (int p = 0; p < PZ; ++p) best[p] = centre[p] = 0u;
#pragma unroll
        for (int b = 0; b < LABEL_PLANES; ++b) label[b] = 0u;
#pragma unroll 1
        for (uint32_t l = 0u; l <= count; ++l) {
            if ((l & ~free_bits & all) != must) continue; // a bit that is the same in every voxel of the halo differs in l
            const bool any = tile_load(lds, g, t, at, [&](size_t row, int w) {
                return class_word(planes + row * (size_t)g.d.wx + (size_t)w, words, nplanes, l);
            });
            if (!__syncthreads_or(any)) continue;         // no voxel of the class in the halo: its count is 0 everywhere
            uint32_t c[PZ];
            tile_count<PX, PY, PZ>(lds, g, t, c);
            uint32_t gt = 0u;                             // c > best
#pragma unroll
            for (int p = 0; p < PZ; ++p) gt = (c[p] & ~best[p]) | (~(c[p] ^ best[p]) & gt);
            uint32_t own_class = 0xffffffffu;
#pragma unroll
            for (int b = 0; b < LABEL_PLANES; ++b) {
                const bool bit = ((l >> b) & 1u) != 0u;
                own_class &= bit ? own[b] : ~own[b];
                label[b] = bit ? (label[b] | gt) : (label[b] & ~gt);
            }
#pragma unroll
            for (int p = 0; p < PZ; ++p) {
                best[p] = (c[p] & gt) | (best[p] & ~gt);
                centre[p] |= c[p] & own_class;
            }
            __syncthreads();                              // the xy counts are read: the next class loads over them
        }
        uint32_t eq = 0xffffffffu;                        // the centre's own count attains the maximum
#pragma unroll
        for (int p = 0; p < PZ; ++p) eq &= ~(centre[p] ^ best[p]);
#pragma unroll
        for (int b = 0; b < LABEL_PLANES; ++b) ob[b] = (own[b] & eq) | (label[b] & ~eq);
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < LABEL_PLANES; ++b) lds[b * THREADS + tid] = ob[b];
    __syncthreads();
    tile_store_values(lds, nplanes, g, at, out);
}

// BINOMIAL: the mask as a u16 volume, and the upper half of a u16 volume as a mask
__global__ __launch_bounds__(THREADS) void k_expand(const uint32_t* __restrict__ mask, uint16_t* __restrict__ e, RegionDims d, size_t words)
{
    const LaneAt a = lane_at(d, words);
    if (a.inside) e[a.v] = ((mask[a.i] >> a.bit) & 1u) ? (uint16_t)65535u : (uint16_t)0u;
}
__global__ __launch_bounds__(THREADS) void k_upper_half(const uint16_t* __restrict__ s, uint32_t* __restrict__ mask, RegionDims d, size_t words)
{
    const LaneAt a = lane_at(d, words);
    const uint32_t w = half_ballot(a.inside && s[a.v] >= 32768u);
    if (a.word_ok && a.bit == 0) mask[a.i] = w;
}

__device__ inline void add_to(unsigned long long* total, uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(total, (unsigned long long)v);
}
// the voxels at which two masks differ, the voxels at which a label map (as it is read) differs from another
__global__ __launch_bounds__(THREADS) void k_mask_diff(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, RegionDims d, size_t words,
                                                       unsigned long long* total)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    add_to(total, i < words ? (uint32_t)__popc((a[i] ^ b[i]) & valid_bits((int)(i % (unsigned)d.wx), d)) : 0u);
}
__global__ __launch_bounds__(THREADS) void k_label_diff(const uint32_t* __restrict__ in, const uint32_t* __restrict__ out, uint32_t count, size_t n,
                                                        unsigned long long* total)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    uint32_t differs = 0u;
    if (i < n) {
        const uint32_t l = in[i];
        differs = (l > count ? 0u : l) != out[i] ? 1u : 0u;
    }
    add_to(total, differs);
}

// ---------------- host side ----------------
CallEvents g_events;                                      // around the device work of the last call (svr_region_smooth_last_ms)

int check_dims3(const char* who, const int32_t* d) { return check_dims(who, d[0], d[1], d[2]); }

int check_radii(const char* who, const uint32_t* r)
{
    for (int a = 0; a < 3; ++a)
        if (r[a] > SVR_REGION_SMOOTH_MAX_RADIUS)
            return failf(-3, "%s: a radius must be at most %d (got %u, %u, %u)", who, SVR_REGION_SMOOTH_MAX_RADIUS, r[0], r[1], r[2]);
    return 0;
}

int check_iterations(const char* who, uint32_t iterations)
{
    if (iterations < 1u || iterations > SVR_REGION_SMOOTH_MAX_ITERATIONS)
        return failf(-3, "%s: iterations must lie in 1 .. %d (got %u)", who, SVR_REGION_SMOOTH_MAX_ITERATIONS, iterations);
    return 0;
}

BoxGeo make_geo(const RegionDims& d, const uint32_t* r)
{
    const uint32_t n = (2u * r[0] + 1u) * (2u * r[1] + 1u) * (2u * r[2] + 1u);
    return BoxGeo{d, (int)r[0], (int)r[1], (int)r[2], (d.wx + TW - 1) / TW, (d.ny + TY - 1) / TY, (n - 1u) / 2u, n};
}
// ceil(wx / 4) ceil(ny / 8) ceil(nz / 8) tiles: at most 2^31 / 64
dim3 tile_grid(const BoxGeo& g) { return dim3((uint32_t)((size_t)g.ntx * g.nty * (size_t)((g.d.nz + TZ - 1) / TZ))); }

// A tile with its halo needs up to 72 KiB of dynamic LDS at radius 8, more than a kernel may ask for by default: every instantiation
// is allowed the LDS of its largest radii, once (the `static` of its launcher)
template <int PX, int PY, class K>
hipError_t allow_lds(K kernel)
{
    const int r = SVR_REGION_SMOOTH_MAX_RADIUS;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_lds_bytes<PX, PY>(r, r));
}

template <int PX, int PY, int PZ>
hipError_t launch_box_planes(hipStream_t st, const uint32_t* in, uint32_t* out_mask, uint16_t* out_count, uint32_t scale_n, const BoxGeo& g)
{
    const size_t lds = tile_lds_bytes<PX, PY>(g.ry, g.rz);
    if (out_count) {
        static const hipError_t allowed = allow_lds<PX, PY>(k_box<PX, PY, PZ, true>);
        if (allowed != hipSuccess) return allowed;
        hipLaunchKernelGGL((k_box<PX, PY, PZ, true>), tile_grid(g), dim3(THREADS), lds, st, in, out_mask, out_count, scale_n, g);
    } else {
        static const hipError_t allowed = allow_lds<PX, PY>(k_box<PX, PY, PZ, false>);
        if (allowed != hipSuccess) return allowed;
        hipLaunchKernelGGL((k_box<PX, PY, PZ, false>), tile_grid(g), dim3(THREADS), lds, st, in, out_mask, out_count, scale_n, g);
    }
    return hipGetLastError();
}
// MAJORITY into out_mask, or (out_count set) COUNT, as it is or (density) scaled to 0 .. 65535
hipError_t launch_box(hipStream_t st, const uint32_t* in, uint32_t* out_mask, uint16_t* out_count, const BoxGeo& g, bool density = false)
{
    const int r = g.rx > g.ry ? (g.rx > g.rz ? g.rx : g.rz) : (g.ry > g.rz ? g.ry : g.rz);
    if (r <= 1) return launch_box_planes<2, 4, 5>(st, in, out_mask, out_count, density ? g.n : 0u, g);
    if (r <= 3) return launch_box_planes<3, 6, 9>(st, in, out_mask, out_count, density ? g.n : 0u, g);
    return launch_box_planes<5, 9, 13>(st, in, out_mask, out_count, density ? g.n : 0u, g);
}

template <int PX, int PY, int PZ>
hipError_t launch_mode_planes(hipStream_t st, const uint32_t* planes, int nplanes, uint32_t count, size_t words, uint32_t* out, const BoxGeo& g)
{
    const size_t lds = tile_lds_bytes<PX, PY>(g.ry, g.rz);
    static const hipError_t allowed = allow_lds<PX, PY>(k_label_mode<PX, PY, PZ>);
    if (allowed != hipSuccess) return allowed;
    hipLaunchKernelGGL((k_label_mode<PX, PY, PZ>), tile_grid(g), dim3(THREADS), lds, st, planes, nplanes, count, words, out, g);
    return hipGetLastError();
}
hipError_t launch_mode(hipStream_t st, const uint32_t* planes, int nplanes, uint32_t count, size_t words, uint32_t* out, const BoxGeo& g)
{
    const int r = g.rx > g.ry ? (g.rx > g.rz ? g.rx : g.rz) : (g.ry > g.rz ? g.ry : g.rz);
    if (r <= 1) return launch_mode_planes<2, 4, 5>(st, planes, nplanes, count, words, out, g);
    if (r <= 3) return launch_mode_planes<3, 6, 9>(st, planes, nplanes, count, words, out, g);
    return launch_mode_planes<5, 9, 13>(st, planes, nplanes, count, words, out, g);
}
// svr_region_box_count and _box_density
int box_count(const char* who, const uint32_t* mask_device, const int32_t dims[3], const uint32_t* radii_xyz, uint16_t* out_u16_device, bool density)
{
    if (!mask_device || !dims || !radii_xyz || !out_u16_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, dims)) return e;
    if (int e = check_radii(who, radii_xyz)) return e;
    const RegionDims d = make_dims(dims[0], dims[1], dims[2]);
    const size_t n = (size_t)d.nx * d.ny * d.nz;
    if (overlap(mask_device, mask_words(d) * sizeof(uint32_t), out_u16_device, n * sizeof(uint16_t))) return failf(-3, "%s: out must not overlap the mask", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(launch_box(st, mask_device, nullptr, out_u16_device, make_geo(d, radii_xyz), density));
    return 0;
}

static_assert(SVR_REGION_SMOOTH_MAX_RADIUS == 8 && SVR_REGION_SMOOTH_MAX_RADIUS == SVR_SMOOTH_MAX_RADIUS && SVR_LABEL_SMOOTH_MAX_COUNT == 255,
              "13 count planes, 8 label planes, one word of halo in x, the radii of svr_volume_smooth");

} // namespace

extern "C" {

uint32_t svr_region_box_size(const uint32_t radii_xyz[3])
{
    if (!radii_xyz) return 0u;
    for (int a = 0; a < 3; ++a)
        if (radii_xyz[a] > SVR_REGION_SMOOTH_MAX_RADIUS) return 0u;
    return (2u * radii_xyz[0] + 1u) * (2u * radii_xyz[1] + 1u) * (2u * radii_xyz[2] + 1u);
}

int svr_region_smooth_radii(const double spacing[3], double size, uint32_t radii[3], double size_out[3])
{
    const char* who = "svr_region_smooth_radii";
    if (!spacing || !radii) return failf(-4, "%s: null argument", who);
    for (int a = 0; a < 3; ++a)
        if (!(spacing[a] > 0.0) || !std::isfinite(spacing[a]))
            return failf(-3, "%s: the spacing must be positive and finite (got %g, %g, %g)", who, spacing[0], spacing[1], spacing[2]);
    if (!(size >= 0.0) || !std::isfinite(size)) return failf(-3, "%s: the size must be finite and not negative (got %g)", who, size);
    uint32_t r[3];
    for (int a = 0; a < 3; ++a) {
        const double h = (size / spacing[a] - 1.0) / 2.0;             // the window 2 r + 1 nearest to size / spacing
        if (!(h < (double)SVR_REGION_SMOOTH_MAX_RADIUS + 0.5))
            return failf(-3, "%s: size %g at spacing %g needs a radius above %d on axis %d", who, size, spacing[a], SVR_REGION_SMOOTH_MAX_RADIUS, a);
        const long long v = std::llround(h);
        r[a] = v > 0 ? (uint32_t)v : 0u;
    }
    for (int a = 0; a < 3; ++a) {
        radii[a] = r[a];
        if (size_out) size_out[a] = (double)(2u * r[a] + 1u) * spacing[a];
    }
    return 0;
}

int svr_region_box_count(const uint32_t* mask_device, const int32_t dims[3], const uint32_t* radii_xyz, uint16_t* out_u16_device)
{
    return box_count("svr_region_box_count", mask_device, dims, radii_xyz, out_u16_device, false);
}

int svr_region_box_density(const uint32_t* mask_device, const int32_t dims[3], const uint32_t* radii_xyz, uint16_t* out_u16_device)
{
    return box_count("svr_region_box_density", mask_device, dims, radii_xyz, out_u16_device, true);
}

int svr_region_smooth(const uint32_t* in_mask_device, const int32_t dims[3], int op, const uint32_t* radii_xyz, uint32_t iterations,
                      uint32_t* out_mask_device, uint64_t* changed_or_null)
{
    const char* who = "svr_region_smooth";
    if (!in_mask_device || !dims || !radii_xyz || !out_mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, dims)) return e;
    if (op != SVR_SMOOTH_MAJORITY && op != SVR_SMOOTH_BINOMIAL) return failf(-3, "%s: unknown op %d", who, op);
    if (int e = check_radii(who, radii_xyz)) return e;
    if (int e = check_iterations(who, iterations)) return e;
    const RegionDims d = make_dims(dims[0], dims[1], dims[2]);
    const size_t words = mask_words(d), bytes = words * sizeof(uint32_t), n = (size_t)d.nx * d.ny * d.nz;
    if (overlap(in_mask_device, bytes, out_mask_device, bytes)) return failf(-3, "%s: out must not overlap in", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    DeviceBuffer tmp, total;
    if (op == SVR_SMOOTH_MAJORITY && iterations > 1u) SVR_HIP_TRY(tmp.alloc(bytes));
    if (op == SVR_SMOOTH_BINOMIAL) SVR_HIP_TRY(tmp.alloc(2 * n * sizeof(uint16_t)));      // E and S
    if (changed_or_null) SVR_HIP_TRY(total.alloc(sizeof(unsigned long long)));
    CallTimer timer(g_events, st);
    const uint32_t* src = in_mask_device;
    if (op == SVR_SMOOTH_MAJORITY) {
        const BoxGeo g = make_geo(d, radii_xyz);
        for (uint32_t i = 0; i < iterations; ++i) {
            uint32_t* dst = (iterations - 1u - i) % 2u == 0u ? out_mask_device : tmp.as<uint32_t>();  // the last pass writes `out`
            SVR_HIP_TRY(launch_box(st, src, dst, nullptr, g));
            src = dst;
        }
    } else {
        uint16_t *e = tmp.as<uint16_t>(), *s = e + n;
        for (uint32_t i = 0; i < iterations; ++i) {      // `out` is written from S alone, so every pass may write it
            hipLaunchKernelGGL(k_expand, lane_grid(words), dim3(THREADS), 0, st, src, e, d, words);
            SVR_HIP_TRY(hipGetLastError());
            if (const int rc = svr_volume_smooth(e, d.nx, d.ny, d.nz, 1, radii_xyz, s)) {
                const std::string inner = svr_last_error();              // (failf writes over it)
                return failf(rc, "%s: %s", who, inner.c_str());
            }
            hipLaunchKernelGGL(k_upper_half, lane_grid(words), dim3(THREADS), 0, st, s, out_mask_device, d, words);
            SVR_HIP_TRY(hipGetLastError());
            src = out_mask_device;
        }
    }
    unsigned long long changed = 0ull;
    if (changed_or_null) {
        SVR_HIP_TRY(hipMemsetAsync(total.p, 0, sizeof changed, st));
        hipLaunchKernelGGL(k_mask_diff, word_grid(words), dim3(THREADS), 0, st, in_mask_device, out_mask_device, d, words, total.as<unsigned long long>());
        SVR_HIP_TRY(hipGetLastError());
        SVR_HIP_TRY(hipMemcpyAsync(&changed, total.p, sizeof changed, hipMemcpyDeviceToHost, st));
    }
    timer.stop();
    if (tmp || total) SVR_HIP_TRY(hipStreamSynchronize(st));          // the temporaries are freed on return; the count is the host's
    if (changed_or_null) *changed_or_null = changed;
    return 0;
}

int svr_region_label_smooth(const uint32_t* labels_device, const int32_t dims[3], uint32_t count, const uint32_t* radii_xyz,
                            uint32_t iterations, uint32_t* out_labels_device, uint64_t* changed_or_null)
{
    const char* who = "svr_region_label_smooth";
    if (!labels_device || !dims || !radii_xyz || !out_labels_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, dims)) return e;
    if (count < 1u || count > SVR_LABEL_SMOOTH_MAX_COUNT)
        return failf(-3, "%s: count must lie in 1 .. %d (got %u)", who, SVR_LABEL_SMOOTH_MAX_COUNT, count);
    if (int e = check_radii(who, radii_xyz)) return e;
    if (int e = check_iterations(who, iterations)) return e;
    const RegionDims d = make_dims(dims[0], dims[1], dims[2]);
    const size_t words = mask_words(d), n = (size_t)d.nx * d.ny * d.nz, bytes = n * sizeof(uint32_t);
    if (overlap(labels_device, bytes, out_labels_device, bytes)) return failf(-3, "%s: out must not overlap the labels", who);
    int nplanes = 1;
    while ((count >> nplanes) != 0u) ++nplanes;          // bits(count): 1 .. 8
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    DeviceBuffer planes, tmp, total;
    SVR_HIP_TRY(planes.alloc((size_t)nplanes * words * sizeof(uint32_t)));
    if (iterations > 1u) SVR_HIP_TRY(tmp.alloc(bytes));
    if (changed_or_null) SVR_HIP_TRY(total.alloc(sizeof(unsigned long long)));
    CallTimer timer(g_events, st);
    const BoxGeo g = make_geo(d, radii_xyz);
    const uint32_t* src = labels_device;
    for (uint32_t i = 0; i < iterations; ++i) {
        uint32_t* dst = (iterations - 1u - i) % 2u == 0u ? out_labels_device : tmp.as<uint32_t>();
        hipLaunchKernelGGL(k_label_planes, lane_grid(words), dim3(THREADS), 0, st, src, count, nplanes, d, words, planes.as<uint32_t>());
        SVR_HIP_TRY(hipGetLastError());
        SVR_HIP_TRY(launch_mode(st, planes.as<uint32_t>(), nplanes, count, words, dst, g));
        src = dst;
    }
    unsigned long long changed = 0ull;
    if (changed_or_null) {
        SVR_HIP_TRY(hipMemsetAsync(total.p, 0, sizeof changed, st));
        hipLaunchKernelGGL(k_label_diff, word_grid(n), dim3(THREADS), 0, st, labels_device, out_labels_device, count, n, total.as<unsigned long long>());
        SVR_HIP_TRY(hipGetLastError());
        SVR_HIP_TRY(hipMemcpyAsync(&changed, total.p, sizeof changed, hipMemcpyDeviceToHost, st));
    }
    timer.stop();
    SVR_HIP_TRY(hipStreamSynchronize(st));               // the planes are freed on return
    if (changed_or_null) *changed_or_null = changed;
    return 0;
}

int svr_region_smooth_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_region_smooth_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

} // extern "C"
