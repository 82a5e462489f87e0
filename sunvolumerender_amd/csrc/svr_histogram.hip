// svr_histogram.hip -- histograms of the u16 voxels (whole volume, inside a region mask, per label of a label array) and the analysis of
// a host histogram: moments, quantiles, exact Otsu thresholds (svr_volume_histogram, svr_region_label_histogram, svr_histogram_*; the
// contract is in include/svr_abi.h, the design in DESIGN.md 8r).  Integers only: every count is exact, whatever order the GPU works in.
// The host scaffolding is svr_volume_host.hpp's, the mask layout svr_mask.hpp's.
//
// CELLS: a voxel that counts falls into one cell: its bin (v - lo) >> shift, plus label * bins in the per-label table.  Both calls run
//   the same kernel over cells = bins or (count + 1) * bins counters.
// WORK: the volume is walked as a FLAT array in chunks of V voxels, one chunk per lane, 64 chunks per wave trip, a capped grid
//   (HIST_MAX_BLOCKS blocks of HIST_THREADS) striding over the chunks with 64-bit indices.  V = 8 (one 16-byte load of the voxels, two
//   of the labels) when the arrays are 16-byte aligned, whatever nx is: a flat chunk is aligned even where a row starts at an odd
//   element.  The price is that a chunk may straddle rows; those chunks (and the last, partial one) take a per-voxel path for their
//   mask bits and loads.  V = 1 serves unaligned arrays.  A lane first works out WHICH of its voxels can count (box, mask bits -- never
//   a padding bit: the fast path lies inside one row, the slow path steps from x = nx - 1 to x = 0 of the next row) and loads nothing
//   when none can: a zero mask word costs its own 4 bytes and no voxel.  Slices outside the box's z range are not visited at all.
//   When the box is whole in x and y and the mask has no padding (nx % 32 == 0, or no mask) the coordinates are not needed: the mask
//   is then a flat bit array over the flat voxel index, and the lane skips the two divisions (the FLAT path: the whole-volume case).
// AGGREGATION, before any atomic: (1) a lane adds a run of equal neighbouring cells once; (2) when every counting voxel of a wave trip
//   falls in ONE cell (air: 68 % of the head), the wave adds nothing at all: it keeps (cell, count) in registers and extends the count
//   while the following trips agree, so an all-equal volume costs one atomic per wave, not one per voxel.  The counters a wave can
//   reach are 32 bits everywhere; a count is at most 2^31, so none can wrap.
// COUNTERS: cells <= HIST_LDS_BINS_SMALL (16384): 64 KB of LDS counters per block, two blocks per CU.  Up to 2 * HIST_LDS_BINS_LARGE
//   (65536, every volume histogram): blocks with HIST_LDS_BINS_LARGE (32768) counters, 128 KB of the CU's 160, and one PASS per 32768
//   cells (blockIdx.y): a pass counts the cells of its range only, so 65536 bins read the voxels twice.  Packed 16-bit counters would
//   read once but need an overflow flush that the all-equal case makes the common path; global atomics would be tens of millions
//   of scattered 4-byte adds on the head's 18 252 occupied bins (not built, not measured).  A block adds its LDS counters to the output once, at the
//   end, 64 consecutive cells per wave instruction, zeros skipped.  More cells (label tables only): the aggregated adds go straight
//   to the table in global memory.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <memory>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"

#include "svr_mask.hpp"             // the mask layout
#include "svr_volume_host.hpp"      // the argument checks, DeviceBuffer / DeviceVoxels, CallTimer, SVR_HIP_TRY

using svr::failf;

namespace {

constexpr int HIST_THREADS = 1024;                       // 16 waves: one block of the large kind still fills half a CU's wave slots
constexpr int HIST_MAX_BLOCKS = 512;                     // the capped grid: two blocks for each of 256 CUs
constexpr int HIST_LDS_BINS_SMALL = 16384;               // cells of the 64 KB block
constexpr int HIST_LDS_BINS_LARGE = 32768;               // cells of the 128 KB block, and of one pass
constexpr uint32_t NO_CELL = 0xffffffffu;

struct HistJob {
    const uint16_t* vox;
    const uint32_t* mask;            // or nullptr
    const uint32_t* labels;          // or nullptr
    uint32_t* counts;
    RegionDims d;
    int x0, x1, y0, y1, z0, z1;      // the box, inclusive (the chunk range covers z0 .. z1 and, rounded to chunks, a little more)
    unsigned long long first_chunk, end_chunk;
    unsigned long long first_voxel, end_voxel;       // the slices z0 .. z1 as a flat range
    unsigned long long n;            // voxels of the volume
    int flat;                        // the box is whole in x and y and the mask, if any, has no padding (nx % 32 == 0): no coordinates are needed
    uint32_t lo, hi, shift, bins, label_count, cells;
};

// the cell of a voxel that passed box and mask, NO_CELL if its value or label does not count
__device__ inline uint32_t cell_of(const HistJob& j, uint32_t v, uint32_t label)
{
    if (v < j.lo || v > j.hi || label > j.label_count) return NO_CELL;
    return label * j.bins + ((v - j.lo) >> j.shift);
}

template <int V> __device__ inline uint32_t low_bits(int n) { return n >= 32 ? 0xffffffffu : (1u << n) - 1u; }

// which of the V voxels from flat index i0 can count: bit k for voxel i0 + k
template <int V>
__device__ inline uint32_t counting_voxels(const HistJob& j, unsigned long long i0)
{
    const RegionDims& d = j.d;
    if (j.flat) {                                                                // voxel i0 + k is bit (i0 + k) & 31 of mask word (i0 + k) >> 5
        const long long a = (long long)j.first_voxel - (long long)i0, b = (long long)j.end_voxel - (long long)i0;      // b > 0
        uint32_t bits = low_bits<V>(b >= V ? V : (int)b) & ~low_bits<V>(a > 0 ? (int)a : 0);
        if (j.mask) bits &= j.mask[i0 >> 5] >> (i0 & 31u);                       // (a chunk starts at a multiple of V: inside one word)
        return bits;
    }
    // i0 < 2^31: the divisions are 32-bit
    uint32_t row = (uint32_t)i0 / (uint32_t)d.nx;
    int x = (int)((uint32_t)i0 - row * (uint32_t)d.nx);
    uint32_t z = row / (uint32_t)d.ny;
    int y = (int)(row - z * (uint32_t)d.ny);
    if (x + V <= d.nx) {                                                         // inside one row (and so inside the volume)
        if (y < j.y0 || y > j.y1 || (int)z < j.z0 || (int)z > j.z1) return 0u;
        const int a = j.x0 - x > 0 ? j.x0 - x : 0, b = j.x1 - x < V - 1 ? j.x1 - x : V - 1;
        if (a > b) return 0u;
        uint32_t bits = low_bits<V>(b + 1) & ~low_bits<V>(a);
        if (j.mask) {
            const uint32_t* w = j.mask + (size_t)row * d.wx + (x >> 5);
            const int s = x & 31;
            uint32_t m = w[0] >> s;
            if (s + V > 32) m |= w[1] << (32 - s);                               // x + V - 1 < nx lies in the next word: it exists
            bits &= m;
        }
        return bits;
    }
    uint32_t bits = 0u;                                                          // the chunk straddles rows or the end of the volume
#pragma unroll
    for (int k = 0; k < V; ++k) {
        if (i0 + k >= j.n) break;
        if (x == d.nx) { x = 0; ++row; if (++y == d.ny) { y = 0; ++z; } }
        if (y >= j.y0 && y <= j.y1 && (int)z >= j.z0 && (int)z <= j.z1 && x >= j.x0 && x <= j.x1 &&
            (!j.mask || ((j.mask[(size_t)row * d.wx + (x >> 5)] >> (x & 31)) & 1u))) bits |= 1u << k;
        ++x;
    }
    return bits;
}

// the cells of the V voxels from i0 (NO_CELL where bit k of `bits` is clear or the voxel does not count); bits != 0
template <int V>
__device__ inline void load_cells(const HistJob& j, unsigned long long i0, uint32_t bits, uint32_t cell[V])
{
    uint32_t v[V], l[V];
    if (V == 8 && i0 + 8 <= j.n) {
        const uint4 q = *reinterpret_cast<const uint4*>(j.vox + i0);
        v[0] = q.x & 0xffffu; v[1 % V] = q.x >> 16; v[2 % V] = q.y & 0xffffu; v[3 % V] = q.y >> 16;
        v[4 % V] = q.z & 0xffffu; v[5 % V] = q.z >> 16; v[6 % V] = q.w & 0xffffu; v[7 % V] = q.w >> 16;
        if (j.labels) {
            const uint4 a = *reinterpret_cast<const uint4*>(j.labels + i0), b = *reinterpret_cast<const uint4*>(j.labels + i0 + 4);
            l[0] = a.x; l[1 % V] = a.y; l[2 % V] = a.z; l[3 % V] = a.w; l[4 % V] = b.x; l[5 % V] = b.y; l[6 % V] = b.z; l[7 % V] = b.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const bool on = (bits >> k) & 1u;                                    // (a clear bit may lie past the end of the volume)
            v[k] = on ? (uint32_t)j.vox[i0 + k] : 0u;
            l[k] = on && j.labels ? j.labels[i0 + k] : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) cell[k] = ((bits >> k) & 1u) ? cell_of(j, v[k], j.labels ? l[k] : 0u) : NO_CELL;
}

// LDS_CELLS > 0: the block counts the cells [pass * LDS_CELLS, (pass + 1) * LDS_CELLS) in LDS, pass = blockIdx.y; 0: global atomics
template <int V, int LDS_CELLS>
__global__ __launch_bounds__(HIST_THREADS) void k_histogram(HistJob j)
{
    __shared__ uint32_t lh[LDS_CELLS > 0 ? LDS_CELLS : 1];
    const uint32_t base = LDS_CELLS > 0 ? blockIdx.y * (uint32_t)LDS_CELLS : 0u;
    const uint32_t mine = LDS_CELLS > 0 ? (j.cells - base < (uint32_t)LDS_CELLS ? j.cells - base : (uint32_t)LDS_CELLS) : j.cells;
    if (LDS_CELLS > 0) {
        for (uint32_t c = threadIdx.x; c < mine; c += HIST_THREADS) lh[c] = 0u;
        __syncthreads();
    }
    uint32_t* const tgt = LDS_CELLS > 0 ? lh : j.counts;
    const unsigned lane = threadIdx.x & 63u;
    uint32_t hot_cell = NO_CELL, hot_count = 0u;                                 // wave-uniform: the cell of the last uniform trips
    // all 64 lanes of a wave make the same trips: the ballots and shuffles below see a full wave
    const unsigned long long stride = (unsigned long long)gridDim.x * HIST_THREADS;
    for (unsigned long long c0 = j.first_chunk + (unsigned long long)blockIdx.x * HIST_THREADS + (threadIdx.x & ~63u); c0 < j.end_chunk; c0 += stride) {
        const unsigned long long c = c0 + lane;
        uint32_t cell[V];
#pragma unroll
        for (int k = 0; k < V; ++k) cell[k] = NO_CELL;
        if (c < j.end_chunk) {
            const unsigned long long i0 = c * V;
            const uint32_t bits = counting_voxels<V>(j, i0);
            if (bits) load_cells<V>(j, i0, bits, cell);
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
            uint32_t total = 0u;                                                 // the wave's sum of cnt (0 .. 8 a lane): one ballot per bit
#pragma unroll
            for (int k = 0; k < 4; ++k) total += (uint32_t)__builtin_popcountll(__ballot((cnt >> k) & 1u)) << k;
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
        for (uint32_t c = threadIdx.x; c < mine; c += HIST_THREADS) {
            const uint32_t n = lh[c];
            if (n) atomicAdd(&j.counts[base + c], n);
        }
    }
}

template <int V>
hipError_t launch_histogram(HistJob j, unsigned long long first_voxel, unsigned long long end_voxel, hipStream_t st)
{
    j.first_voxel = first_voxel; j.end_voxel = end_voxel;
    j.first_chunk = first_voxel / V;
    j.end_chunk = (end_voxel + V - 1) / V;
    const unsigned long long chunks = j.end_chunk - j.first_chunk;
    const unsigned long long want = (chunks + HIST_THREADS - 1) / HIST_THREADS;
    const uint32_t blocks = (uint32_t)(want < (unsigned long long)HIST_MAX_BLOCKS ? want : (unsigned long long)HIST_MAX_BLOCKS);
    if (j.cells <= (uint32_t)HIST_LDS_BINS_SMALL)
        hipLaunchKernelGGL((k_histogram<V, HIST_LDS_BINS_SMALL>), dim3(blocks), dim3(HIST_THREADS), 0, st, j);
    else if (j.cells <= 2u * (uint32_t)HIST_LDS_BINS_LARGE)
        hipLaunchKernelGGL((k_histogram<V, HIST_LDS_BINS_LARGE>), dim3(blocks, (j.cells + HIST_LDS_BINS_LARGE - 1) / HIST_LDS_BINS_LARGE),
                           dim3(HIST_THREADS), 0, st, j);
    else
        hipLaunchKernelGGL((k_histogram<V, 0>), dim3(blocks), dim3(HIST_THREADS), 0, st, j);
    return hipGetLastError();
}

CallEvents g_events;

int check_params(const char* who, const svr_histogram_params* p)
{
    if (p->lo > p->hi) return failf(-3, "%s: lo (%u) is above hi (%u)", who, p->lo, p->hi);
    if (p->hi > 65535u) return failf(-3, "%s: hi must be <= 65535 (got %u)", who, p->hi);
    if (p->shift > 15u) return failf(-3, "%s: shift must be <= 15 (got %u)", who, p->shift);
    return 0;
}

bool params_ok(const svr_histogram_params* p) { return p && p->lo <= p->hi && p->hi <= 65535u && p->shift <= 15u; }
uint32_t bins_of(const svr_histogram_params& p) { return ((p.hi - p.lo) >> p.shift) + 1u; }

// both entry points after their null checks; labels == nullptr for the volume histogram
int histogram_call(const char* who, const uint32_t* labels, const uint16_t* voxels, const int32_t* dims, int src_is_device, const uint32_t* mask,
                   uint32_t count, const svr_histogram_params* params_or_null, uint32_t* counts)
{
    if (int e = check_dims(who, dims[0], dims[1], dims[2])) return e;
    svr_histogram_params p;
    if (params_or_null) p = *params_or_null;
    else svr_histogram_params_default(&p);
    if (int e = check_params(who, &p)) return e;
    const RegionDims d = make_dims(dims[0], dims[1], dims[2]);
    int b0[3], b1[3];
    if (int e = clamp_box(who, p.box_min, p.box_max, d.nx, d.ny, d.nz, b0, b1)) return e;
    const uint32_t bins = bins_of(p);
    const unsigned long long cells = ((unsigned long long)count + 1ull) * bins;
    if (cells > SVR_HISTOGRAM_MAX_CELLS)
        return failf(-3, "%s: (count + 1) * bins = %llu cells is more than SVR_HISTOGRAM_MAX_CELLS (%u): raise shift or narrow the window", who, cells,
                     SVR_HISTOGRAM_MAX_CELLS);
    const size_t n = (size_t)d.nx * d.ny * d.nz;
    const size_t out_bytes = (size_t)cells * sizeof(uint32_t);
    if (overlap(counts, out_bytes, voxels, n * sizeof(uint16_t)) || (mask && overlap(counts, out_bytes, mask, mask_words(d) * sizeof(uint32_t))) ||
        (labels && overlap(counts, out_bytes, labels, n * sizeof(uint32_t))))
        return failf(-3, "%s: counts_device must not overlap an input", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    DeviceVoxels dv;
    SVR_HIP_TRY(dv.get(voxels, n, src_is_device, st));
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(hipMemsetAsync(counts, 0, out_bytes, st));
    HistJob j;
    j.vox = dv.p; j.mask = mask; j.labels = labels; j.counts = counts; j.d = d;
    j.x0 = b0[0]; j.x1 = b1[0]; j.y0 = b0[1]; j.y1 = b1[1]; j.z0 = b0[2]; j.z1 = b1[2];
    j.first_chunk = j.end_chunk = j.first_voxel = j.end_voxel = 0ull;
    j.flat = b0[0] == 0 && b1[0] == d.nx - 1 && b0[1] == 0 && b1[1] == d.ny - 1 && (!mask || d.nx % 32 == 0);
    j.n = n;
    j.lo = p.lo; j.hi = p.hi; j.shift = p.shift; j.bins = bins; j.label_count = count; j.cells = (uint32_t)cells;
    const unsigned long long slice = (unsigned long long)d.nx * d.ny;
    const unsigned long long first = slice * (unsigned)b0[2], end = slice * ((unsigned)b1[2] + 1u);
    const bool vec8 = (uintptr_t)dv.p % 16 == 0 && (!labels || (uintptr_t)labels % 16 == 0);
    SVR_HIP_TRY(vec8 ? launch_histogram<8>(j, first, end, st) : launch_histogram<1>(j, first, end, st));
    timer.stop();
    if (dv.owned()) SVR_HIP_TRY(hipStreamSynchronize(st));   // the upload is freed on return
    return 0;
}

// ---- the analysis of a host histogram: unsigned integers of 512 bits, enough for every cross product of any uint32 counts ----
// (a histogram of a volume, N <= 2^31, needs 218 bits for two classes and 230 for three; a caller's own counts reach N = 2^48 and
// sums of 2^64, whose three-class cross products stay below 2^372)
struct Wide {
    uint64_t w[8];
    Wide() { memset(w, 0, sizeof w); }
    Wide(unsigned __int128 v) { memset(w, 0, sizeof w); w[0] = (uint64_t)v; w[1] = (uint64_t)(v >> 64); }
};
Wide operator*(const Wide& a, const Wide& b)                 // the low 512 bits; the callers' products fit
{
    Wide r;
    for (int i = 0; i < 8; ++i) {
        if (!a.w[i]) continue;
        uint64_t carry = 0;
        for (int k = 0; i + k < 8; ++k) {
            const unsigned __int128 t = (unsigned __int128)a.w[i] * b.w[k] + r.w[i + k] + carry;
            r.w[i + k] = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
    }
    return r;
}
Wide operator+(const Wide& a, const Wide& b)
{
    Wide r;
    uint64_t carry = 0;
    for (int i = 0; i < 8; ++i) {
        const unsigned __int128 t = (unsigned __int128)a.w[i] + b.w[i] + carry;
        r.w[i] = (uint64_t)t;
        carry = (uint64_t)(t >> 64);
    }
    return r;
}
bool operator>(const Wide& a, const Wide& b)
{
    for (int i = 7; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
    return false;
}
double to_double(const Wide& a)
{
    double r = 0.0;
    for (int i = 7; i >= 0; --i) r = r * 18446744073709551616.0 + (double)a.w[i];
    return r;
}

// the criterion sum_j S_j^2 / N_j of up to three classes as one fraction num / den (an empty class: 0 / 1)
struct Criterion { Wide num, den; };
Criterion criterion(const unsigned __int128* n, const unsigned __int128* s, int classes)
{
    Wide a[3], m[3];
    for (int k = 0; k < classes; ++k) {
        a[k] = n[k] ? Wide(s[k]) * Wide(s[k]) : Wide(0);
        m[k] = Wide(n[k] ? n[k] : (unsigned __int128)1);
    }
    Criterion c;
    if (classes == 2) { c.num = a[0] * m[1] + a[1] * m[0]; c.den = m[0] * m[1]; }
    else { c.num = a[0] * (m[1] * m[2]) + a[1] * (m[0] * m[2]) + a[2] * (m[0] * m[1]); c.den = m[0] * m[1] * m[2]; }
    return c;
}
bool better(const Criterion& a, const Criterion& b) { return a.num * b.den > b.num * a.den; }      // a > b, exactly

int check_counts(const char* who, const uint32_t* counts, uint32_t bins, const void* out)
{
    if (!counts || !out) return failf(-4, "%s: null argument", who);
    if (bins == 0u) return failf(-3, "%s: bins must be at least 1", who);
    return 0;
}

} // namespace

extern "C" {

int svr_histogram_params_default(svr_histogram_params* p)
{
    if (!p) return failf(-4, "svr_histogram_params_default: null argument");
    p->lo = 0u; p->hi = 65535u; p->shift = 0u;
    for (int a = 0; a < 3; ++a) { p->box_min[a] = 0; p->box_max[a] = INT32_MAX; }
    return 0;
}

uint32_t svr_histogram_bins(const svr_histogram_params* p) { return params_ok(p) ? bins_of(*p) : 0u; }

int svr_histogram_bin_range(const svr_histogram_params* p, uint32_t bin, uint32_t* v_lo, uint32_t* v_hi)
{
    const char* who = "svr_histogram_bin_range";
    if (!p || !v_lo || !v_hi) return failf(-4, "%s: null argument", who);
    if (int e = check_params(who, p)) return e;
    if (bin >= bins_of(*p)) return failf(-3, "%s: bin %u of %u", who, bin, bins_of(*p));
    const uint32_t first = p->lo + (bin << p->shift), last = first + (1u << p->shift) - 1u;
    *v_lo = first;
    *v_hi = last < p->hi ? last : p->hi;
    return 0;
}

int svr_volume_histogram(const uint16_t* voxels, const int32_t dims[3], int src_is_device, const uint32_t* mask_device_or_null,
                         const svr_histogram_params* params_or_null, uint32_t* counts_device)
{
    const char* who = "svr_volume_histogram";
    if (!voxels || !dims || !counts_device) return failf(-4, "%s: null argument", who);
    return histogram_call(who, nullptr, voxels, dims, src_is_device, mask_device_or_null, 0u, params_or_null, counts_device);
}

int svr_region_label_histogram(const uint32_t* labels_device, const uint16_t* voxels, const int32_t dims[3], int src_is_device,
                               uint32_t count, const svr_histogram_params* params_or_null, uint32_t* counts_device)
{
    const char* who = "svr_region_label_histogram";
    if (!labels_device || !voxels || !dims || !counts_device) return failf(-4, "%s: null argument", who);
    return histogram_call(who, labels_device, voxels, dims, src_is_device, nullptr, count, params_or_null, counts_device);
}

int svr_volume_histogram_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_volume_histogram_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

int svr_histogram_moments(const uint32_t* counts, uint32_t bins, uint64_t* n, uint64_t* sum, uint64_t* sum_sq)
{
    const char* who = "svr_histogram_moments";
    if (!n || !sum) return failf(-4, "%s: null argument", who);
    if (int e = check_counts(who, counts, bins, sum_sq)) return e;
    unsigned __int128 t[3] = {0, 0, 0};
    for (uint32_t b = 0; b < bins; ++b) {
        t[0] += counts[b];
        t[1] += (unsigned __int128)counts[b] * b;
        t[2] += (unsigned __int128)counts[b] * b * b;
    }
    for (int k = 0; k < 3; ++k)
        if (t[k] >> 64) return failf(-3, "%s: the sums of these counts do not fit 64 bits", who);
    *n = (uint64_t)t[0]; *sum = (uint64_t)t[1]; *sum_sq = (uint64_t)t[2];
    return t[0] ? 0 : SVR_HISTOGRAM_STATUS_EMPTY;
}

int svr_histogram_quantile(const uint32_t* counts, uint32_t bins, uint32_t num, uint32_t den, uint32_t* bin_out)
{
    const char* who = "svr_histogram_quantile";
    if (int e = check_counts(who, counts, bins, bin_out)) return e;
    if (den == 0u || num > den) return failf(-3, "%s: the quantile %u / %u is not in 0 .. 1", who, num, den);
    uint64_t total = 0;
    for (uint32_t b = 0; b < bins; ++b) total += counts[b];
    *bin_out = 0u;
    if (!total) return SVR_HISTOGRAM_STATUS_EMPTY;
    const unsigned __int128 want = (unsigned __int128)num * total;             // den * C(b) < 2^80
    uint64_t c = 0;
    for (uint32_t b = 0; b < bins; ++b) {
        c += counts[b];
        if (c > 0u && (unsigned __int128)den * c >= want) { *bin_out = b; return 0; }
    }
    return failf(-1, "%s: internal error", who);                                // (C(bins - 1) = N satisfies the test)
}

int svr_histogram_otsu(const uint32_t* counts, uint32_t bins, uint32_t classes, uint32_t* thresholds_out, double* eta_out)
{
    const char* who = "svr_histogram_otsu";
    if (int e = check_counts(who, counts, bins, thresholds_out)) return e;
    if (classes != 2u && classes != 3u) return failf(-3, "%s: classes must be 2 or 3 (got %u)", who, classes);
    if (classes == 3u && bins > 256u) return failf(-3, "%s: three classes need bins <= 256 (got %u): coarsen with shift", who, bins);
    if (bins < classes) return failf(-3, "%s: %u classes need at least as many bins (got %u)", who, classes, bins);
    // prefix sums: cn[b], cs[b] = count and sum of bin index x count over the bins below b
    std::unique_ptr<unsigned __int128[]> cn(new unsigned __int128[bins + 1u]), cs(new unsigned __int128[bins + 1u]);
    unsigned __int128 ss = 0;
    cn[0] = cs[0] = 0;
    for (uint32_t b = 0; b < bins; ++b) {
        cn[b + 1u] = cn[b] + counts[b];
        cs[b + 1u] = cs[b] + (unsigned __int128)counts[b] * b;
        ss += (unsigned __int128)counts[b] * b * b;
    }
    const unsigned __int128 N = cn[bins], S = cs[bins];
    for (uint32_t k = 0; k + 1u < classes; ++k) thresholds_out[k] = 0u;
    if (eta_out) *eta_out = 0.0;
    if (!N) return SVR_HISTOGRAM_STATUS_EMPTY;
    Criterion best;
    bool have = false;
    unsigned __int128 n[3], s[3];
    if (classes == 2u) {
        for (uint32_t t = 0; t + 1u < bins; ++t) {
            n[0] = cn[t + 1u]; s[0] = cs[t + 1u]; n[1] = N - n[0]; s[1] = S - s[0];
            const Criterion c = criterion(n, s, 2);
            if (!have || better(c, best)) { best = c; have = true; thresholds_out[0] = t; }     // strictly better: ties keep the lower t
        }
    } else {
        for (uint32_t t1 = 0; t1 + 2u < bins; ++t1)
            for (uint32_t t2 = t1 + 1u; t2 + 1u < bins; ++t2) {
                n[0] = cn[t1 + 1u]; s[0] = cs[t1 + 1u];
                n[1] = cn[t2 + 1u] - n[0]; s[1] = cs[t2 + 1u] - s[0];
                n[2] = N - cn[t2 + 1u]; s[2] = S - cs[t2 + 1u];
                const Criterion c = criterion(n, s, 3);
                if (!have || better(c, best)) { best = c; have = true; thresholds_out[0] = t1; thresholds_out[1] = t2; }
            }
    }
    if (eta_out) {
        // (criterion - S^2 / N) / (sum_sq - S^2 / N): between-class over total variance
        const double mean_term = (double)S * (double)S / (double)N;
        const double total = (double)ss - mean_term;
        const double between = to_double(best.num) / to_double(best.den) - mean_term;
        *eta_out = total > 0.0 ? between / total : 0.0;
        if (*eta_out < 0.0) *eta_out = 0.0;
        if (*eta_out > 1.0) *eta_out = 1.0;
    }
    return 0;
}

} // extern "C"
