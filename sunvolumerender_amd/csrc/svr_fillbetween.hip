// svr_fillbetween.hip -- fill between slices: a region drawn on a few slices of one axis, interpolated on the slices between them by the
// sign of the linearly interpolated signed planar distance (shape-based interpolation, Raya and Udupa), and what it is made of: the set
// voxels of every slice and the planar distance maps of slices (svr_region_slice_counts, svr_region_slice_distance,
// svr_region_fill_between; the contract is in include/svr_abi.h, the design in DESIGN.md 8v).  Integers only, on the mask layout and
// padding rule of svr_mask.hpp; the host scaffolding is svr_volume_host.hpp's.
//
// COUNTS  axis y / z (k_slice_counts_words): one thread per mask word.  The 256 words of a block lie in at most 256 rows, so an LDS bin
//   per row (y) or per slice (z) of the block takes the popcounts -- by one LDS atomic per wave where the wave's words share a bin, the sum
//   made by shuffles -- and one global 64-bit atomic per non-empty bin follows.  axis x (k_slice_counts_bits) needs the count of every
//   bit column: one lane per x, the lanes of a block walk the rows gridDim.y apart (32 lanes read one word: a broadcast), each lane counts
//   its bit in a register and issues one global atomic at the end.
// PLANAR MAPS (planar_maps): the listed slices are gathered into the mask of an nu x nv x C volume (k_gather_slices: one lane per slot,
//   the word by half_ballot), C slices at a time, and that volume goes through the row pass and ONE column pass of svr_dist_passes.hpp:
//   the transform of DESIGN 8k with the pass along the third axis left out, so a slice never sees another.  It runs for both targets;
//   the TO_SET map is written in place, the TO_UNSET map beside it, and k_merge_maps takes the second where the mask bit is set.  The
//   slices of axis x are gathered into rows as well, so they too have a row pass by bit tricks.
// FILL (k_fill): one lane per voxel slot of the whole mask (lane_at).  The lane reads the entry of its slice in the slice table -- the
//   ordinals of the key below and above among the keys that have maps, t and n; n == 0 means copy -- and, if its slice lies strictly
//   between the keys of this launch, the mask bits of its in-plane position in both keys and, where they differ, the two map values; the
//   comparison is in uint64.  The word is a half_ballot, written by one lane; no bit is written alone and there are no atomics.  Lanes of
//   copied slices pass their input bit on and load no map.  out may be in: a word is read and written by the same half wave, and the key
//   slices, which other lanes read, are written with the bits they have.
// No lane or block waits for another; every loop runs to an axis length or a row count.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"

#include "svr_mask.hpp"             // the mask layout
#include "svr_dist_passes.hpp"      // k_dist_rows, k_dist_columns<OUT_MAP>, ColPass
#include "svr_volume_host.hpp"      // the argument checks, DeviceBuffer, CallTimer, SVR_HIP_TRY

using svr::failf;

namespace {

constexpr size_t PLANAR_CHUNK_VOXELS = (size_t)1 << 26;                  // voxels of the slices that go through the passes together
constexpr size_t MAP_BUDGET_VOXELS = (size_t)SVR_FILL_MAP_BUDGET_BYTES / 4u;   // map values that svr_region_fill_between keeps at a time
constexpr uint32_t COUNT_ROW_PLANES = 1024u;                             // gridDim.y of k_slice_counts_bits at the most

// the slicing axis and the two in-plane axes u < v of a volume
struct SliceAxes {
    int axis, n, nu, nv;                                                  // the lengths of the slicing axis and of u and v
    size_t plane() const { return (size_t)nu * nv; }
};
SliceAxes slice_axes(int axis, int nx, int ny, int nz)
{
    if (axis == 0) return {0, nx, ny, nz};
    if (axis == 1) return {1, ny, nx, nz};
    return {2, nz, nx, ny};
}

// voxel (x, y, z) of slice k, in-plane position (u, v)
__device__ inline void slice_voxel(int axis, int k, int u, int v, int& x, int& y, int& z)
{
    if (axis == 0) { x = k; y = u; z = v; }
    else if (axis == 1) { x = u; y = k; z = v; }
    else { x = u; y = v; z = k; }
}

__device__ inline uint32_t mask_bit(const uint32_t* mask, const RegionDims& d, int x, int y, int z)
{
    return (mask[((size_t)z * d.ny + y) * d.wx + (x >> 5)] >> (x & 31)) & 1u;
}

__device__ inline uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}

// ---------------- counts ----------------
__global__ __launch_bounds__(MASK_THREADS) void k_slice_counts_words(const uint32_t* __restrict__ mask, RegionDims d, size_t words, int axis,
                                                                     unsigned long long* __restrict__ counts)
{
    __shared__ uint32_t bins[MASK_THREADS];
    const size_t i0 = (size_t)blockIdx.x * MASK_THREADS, i = i0 + threadIdx.x;
    const size_t row0 = i0 / (unsigned)d.wx;
    bins[threadIdx.x] = 0u;
    __syncthreads();
    const size_t ic = i < words ? i : words - 1;                                  // (a lane past the end counts nothing, in a bin that exists)
    const size_t row = ic / (unsigned)d.wx;
    const uint32_t c = i < words ? (uint32_t)__popc(mask[i] & valid_bits((int)(ic % (unsigned)d.wx), d)) : 0u;
    const uint32_t key = axis == 2 ? (uint32_t)(row / (unsigned)d.ny - row0 / (unsigned)d.ny) : (uint32_t)(row - row0);   // below 256
    const uint32_t first = (uint32_t)__shfl((int)key, 0);
    if (__all(key == first)) {
        const uint32_t sum = wave_sum(c);
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&bins[first], sum);
    } else if (c) {
        atomicAdd(&bins[key], c);
    }
    __syncthreads();
    const uint32_t mine = bins[threadIdx.x];
    if (mine) {
        const size_t slice = axis == 2 ? row0 / (unsigned)d.ny + threadIdx.x : (row0 + threadIdx.x) % (unsigned)d.ny;
        atomicAdd(&counts[slice], (unsigned long long)mine);
    }
}

__global__ __launch_bounds__(MASK_THREADS) void k_slice_counts_bits(const uint32_t* __restrict__ mask, RegionDims d, size_t rows,
                                                                    unsigned long long* __restrict__ counts)
{
    const size_t x = (size_t)blockIdx.x * MASK_THREADS + threadIdx.x;
    if (x >= (size_t)d.nx) return;
    const size_t gw = x >> 5;
    const uint32_t bit = (uint32_t)(x & 31u);
    uint32_t c = 0u;                                                             // at most rows <= 2^31
    for (size_t r = blockIdx.y; r < rows; r += gridDim.y) c += (mask[r * (unsigned)d.wx + gw] >> bit) & 1u;
    if (c) atomicAdd(&counts[x], (unsigned long long)c);
}

// counts[0 .. n_axis) += the set voxels of every slice; counts is zeroed here
hipError_t launch_counts(hipStream_t st, const uint32_t* mask, const RegionDims& d, const SliceAxes& ax, unsigned long long* counts)
{
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)ax.n * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const size_t words = mask_words(d), rows = (size_t)d.ny * d.nz;
    if (ax.axis == 0) {
        const size_t planes = (rows + 511) / 512;
        const dim3 g((uint32_t)(((size_t)d.nx + MASK_THREADS - 1) / MASK_THREADS), (uint32_t)(planes < COUNT_ROW_PLANES ? planes : COUNT_ROW_PLANES));
        hipLaunchKernelGGL(k_slice_counts_bits, g, dim3(MASK_THREADS), 0, st, mask, d, rows, counts);
    } else {
        hipLaunchKernelGGL(k_slice_counts_words, word_grid(words), dim3(MASK_THREADS), 0, st, mask, d, words, ax.axis, counts);
    }
    return hipGetLastError();
}

// ---------------- planar maps ----------------
// the mask of the nu x nv x count volume whose slice s is slice slices[s] of the axis
__global__ __launch_bounds__(MASK_THREADS) void k_gather_slices(const uint32_t* __restrict__ mask, RegionDims d, int axis, const int32_t* __restrict__ slices,
                                                                RegionDims ds, size_t swords, uint32_t* __restrict__ out)
{
    const LaneAt a = lane_at(ds, swords);
    bool on = false;
    if (a.inside) {
        int x, y, z;
        slice_voxel(axis, slices[a.z], a.x, a.y, x, y, z);
        on = mask_bit(mask, d, x, y, z) != 0u;
    }
    const uint32_t word = half_ballot(on);
    if (a.word_ok && a.bit == 0) out[a.i] = word;
}

// the planar map: to_set holds the TO_SET map and gets the TO_UNSET value where the voxel is set
__global__ __launch_bounds__(MASK_THREADS) void k_merge_maps(const uint32_t* __restrict__ smask, const uint32_t* __restrict__ to_unset, RegionDims ds, size_t swords,
                                                             uint32_t* __restrict__ to_set)
{
    const LaneAt a = lane_at(ds, swords);
    if (a.inside && ((smask[a.i] >> a.bit) & 1u)) to_set[a.v] = to_unset[a.v];
}

// the workspace of planar_maps for up to `nslices` slices at a time: the list, the gathered mask, the row pass's output, the TO_UNSET map
// and the stacks -- per voxel of the `chunk` slices that go through the passes together 12 bytes and one bit
struct PlanarWork {
    DeviceBuffer list, work;
    size_t chunk = 0, plane = 0, smask_words = 0;
    static size_t chunk_of(size_t plane, size_t nslices)
    {
        const size_t c = PLANAR_CHUNK_VOXELS / plane;
        return c < 1 ? 1 : (c > nslices ? nslices : c);
    }
    static size_t bytes(const SliceAxes& ax, size_t nslices)
    {
        const size_t c = chunk_of(ax.plane(), nslices);
        return ((size_t)((ax.nu + 31) / 32) * ax.nv * c + 3u * c * ax.plane()) * sizeof(uint32_t) + nslices * sizeof(int32_t);
    }
    hipError_t alloc(const SliceAxes& ax, size_t nslices)
    {
        plane = ax.plane();
        chunk = chunk_of(plane, nslices);
        smask_words = (size_t)((ax.nu + 31) / 32) * ax.nv * chunk;
        const hipError_t e = list.alloc(nslices * sizeof(int32_t));
        return e != hipSuccess ? e : work.alloc((smask_words + 3u * chunk * plane) * sizeof(uint32_t));
    }
};

// enqueues the planar maps of slices[0 .. nslices) (a HOST list that lives until the stream has been waited for) into maps[nslices][nv][nu]
hipError_t planar_maps(hipStream_t st, const PlanarWork& pw, const uint32_t* mask, const RegionDims& d, const SliceAxes& ax, uint32_t wu, uint32_t wv,
                       const int32_t* slices, size_t nslices, uint32_t* maps)
{
    const size_t plane = pw.plane, chunk = pw.chunk;
    hipError_t e = hipMemcpyAsync(pw.list.p, slices, nslices * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    uint32_t *smask = pw.work.as<uint32_t>(), *rows = smask + pw.smask_words, *unset_map = rows + chunk * plane, *stack = unset_map + chunk * plane;
    for (size_t s0 = 0; s0 < nslices; s0 += chunk) {
        const size_t c = nslices - s0 < chunk ? nslices - s0 : chunk;
        const RegionDims ds = make_dims(ax.nu, ax.nv, (int)c);
        const size_t swords = mask_words(ds);
        uint32_t* const out = maps + s0 * plane;
        hipLaunchKernelGGL(k_gather_slices, lane_grid(swords), dim3(MASK_THREADS), 0, st, mask, d, ax.axis, pw.list.as<int32_t>() + s0, ds, swords, smask);
        const ColPass pv = {(uint32_t)ds.ny, (uint32_t)ds.nz, (uint32_t)ds.nx, (uint32_t)ds.wx, wv, (size_t)ds.nx, plane, (size_t)ds.ny * ds.wx, (size_t)ds.wx,
                            (size_t)ds.nz * ds.nx};
        const dim3 gv = lane_grid((size_t)ds.nz * ds.wx);
        for (int unset = 0; unset < 2; ++unset) {                                 // rows -> `rows`, then the v pass -> the map
            hipLaunchKernelGGL(k_dist_rows, lane_grid(swords), dim3(THREADS), 0, st, smask, rows, ds, swords, wu, unset);
            hipLaunchKernelGGL((k_dist_columns<OUT_MAP>), gv, dim3(THREADS), 0, st, rows, unset ? unset_map : out, stack, pv, 0u);
        }
        hipLaunchKernelGGL(k_merge_maps, lane_grid(swords), dim3(MASK_THREADS), 0, st, smask, unset_map, ds, swords, out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---------------- the fill ----------------
// a slice of the table: the ordinals, among the keys that have maps, of the key below and the key above, t = k - a and n = b - a; n == 0: copy
struct SliceEntry { int32_t ia, ib, t, n; };

// the slices strictly between lo and hi that have n != 0 are filled from maps[(ordinal - first)][nv][nu]; every other slice keeps src's bits
__global__ __launch_bounds__(MASK_THREADS) void k_fill(const uint32_t* src, const SliceEntry* __restrict__ table, const uint32_t* __restrict__ maps, RegionDims d,
                                                       size_t words, int axis, int nu, size_t plane, int lo, int hi, int first, uint32_t keep, uint32_t* out)
{
    const LaneAt a = lane_at(d, words);
    const uint32_t m = a.word_ok ? src[a.i] : 0u;
    bool on = a.inside && ((m >> a.bit) & 1u);
    const int k = axis == 0 ? a.x : (axis == 1 ? a.y : a.z);
    if (a.inside && k > lo && k < hi) {
        const SliceEntry e = table[k];
        if (e.n != 0) {
            const int u = axis == 0 ? a.y : a.x, v = axis == 2 ? a.y : a.z;
            int x, y, z;
            slice_voxel(axis, k - e.t, u, v, x, y, z);
            const uint32_t sa = mask_bit(src, d, x, y, z);
            slice_voxel(axis, k - e.t + e.n, u, v, x, y, z);
            const uint32_t sb = mask_bit(src, d, x, y, z);
            bool r = sa != 0u;                                                    // (both set, or both unset)
            if (sa != sb) {
                const size_t p = (size_t)v * nu + u;
                const uint64_t A = maps[(size_t)(e.ia - first) * plane + p], B = maps[(size_t)(e.ib - first) * plane + p];
                const uint64_t t = (uint64_t)e.t, nt = (uint64_t)(e.n - e.t);
                const uint64_t pa = nt * nt * A, pb = t * t * B;                  // below 2^64: n <= 65535, the maps below 2^32
                r = sa ? pa > pb : pb > pa;
            }
            on = r || (keep && on);
        }
    }
    const uint32_t word = half_ballot(on);
    if (a.word_ok && a.bit == 0) out[a.i] = word;
}

__global__ __launch_bounds__(MASK_THREADS) void k_fill_copy(const uint32_t* in, uint32_t* out, RegionDims d, size_t words)
{
    const size_t i = (size_t)blockIdx.x * MASK_THREADS + threadIdx.x;
    if (i < words) out[i] = in[i] & valid_bits((int)(i % (unsigned)d.wx), d);
}

// ---------------- the checks ----------------
// axis, weights (NULL = 1, 1, 1) and the lengths: -3; w gets the weights of u and v
int check_planar(const char* who, int axis, const uint32_t* weights_or_null, int nx, int ny, int nz, SliceAxes& ax, uint32_t& wu, uint32_t& wv)
{
    if (axis < 0 || axis > 2) return failf(-3, "%s: the axis must be 0, 1 or 2 (got %d)", who, axis);
    ax = slice_axes(axis, nx, ny, nz);
    uint32_t w[3];
    // the slicing axis takes no part in a planar distance: the bound is that of a volume one slice thick
    if (int e = svr::check_distance_weights(who, weights_or_null, axis == 0 ? 1 : nx, axis == 1 ? 1 : ny, axis == 2 ? 1 : nz, w)) return e;
    if (ax.n > 65536) return failf(-3, "%s: axis %d has %d slices (at most 65536)", who, axis, ax.n);
    wu = w[axis == 0 ? 1 : 0];
    wv = w[axis == 2 ? 1 : 2];
    return 0;
}

CallEvents g_events;
// the last svr_region_fill_between: [0] .. [1] the first count, [2] .. [3] the planar maps and [3] .. [4] the fill pass of its last launch
hipEvent_t g_pass_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
bool g_passes = false;                                    // g_pass_ev have been recorded, all five
bool g_fill_counts_ms = false;                            // the last call was a fill: its first count ran before g_events' pair, see there

} // namespace

extern "C" {

int svr_fill_between_params_default(svr_fill_between_params* p)
{
    if (!p) return failf(-4, "svr_fill_between_params_default: null argument");
    memset(p, 0, sizeof *p);
    p->axis = 2;
    return 0;
}

int svr_region_slice_counts(const uint32_t* mask_device, int nx, int ny, int nz, int axis, uint64_t* counts_host)
{
    const char* who = "svr_region_slice_counts";
    if (!mask_device || !counts_host) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (axis < 0 || axis > 2) return failf(-3, "%s: the axis must be 0, 1 or 2 (got %d)", who, axis);
    const SliceAxes ax = slice_axes(axis, nx, ny, nz);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    DeviceBuffer buf;
    SVR_HIP_TRY(buf.alloc((size_t)ax.n * sizeof(unsigned long long)));
    g_fill_counts_ms = false;
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(launch_counts(st, mask_device, make_dims(nx, ny, nz), ax, buf.as<unsigned long long>()));
    timer.stop();
    SVR_HIP_TRY(hipMemcpyAsync(counts_host, buf.p, (size_t)ax.n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int svr_region_slice_distance(const uint32_t* mask_device, int nx, int ny, int nz, int axis, const uint32_t* weights_or_null, const int32_t* slices_host_or_null,
                              int nslices, uint32_t* maps_device)
{
    const char* who = "svr_region_slice_distance";
    if (!mask_device || !maps_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    SliceAxes ax;
    uint32_t wu, wv;
    if (int e = check_planar(who, axis, weights_or_null, nx, ny, nz, ax, wu, wv)) return e;
    std::vector<int32_t> all;
    if (slices_host_or_null) {
        if (nslices <= 0) return failf(-3, "%s: a slice list needs nslices >= 1 (got %d)", who, nslices);
        for (int s = 0; s < nslices; ++s)
            if (slices_host_or_null[s] < 0 || slices_host_or_null[s] >= ax.n)
                return failf(-3, "%s: slice %d of the list is %d, outside 0 .. %d", who, s, (int)slices_host_or_null[s], ax.n - 1);
    } else {
        all.resize((size_t)ax.n);
        for (int k = 0; k < ax.n; ++k) all[(size_t)k] = k;
        nslices = ax.n;
    }
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    PlanarWork pw;
    SVR_HIP_TRY(pw.alloc(ax, (size_t)nslices));
    g_fill_counts_ms = false;
    CallTimer timer(g_events, st);                        // (the launches, not the allocation)
    SVR_HIP_TRY(planar_maps(st, pw, mask_device, make_dims(nx, ny, nz), ax, wu, wv, slices_host_or_null ? slices_host_or_null : all.data(), (size_t)nslices,
                            maps_device));
    timer.stop();
    SVR_HIP_TRY(hipStreamSynchronize(st));                // (the workspace is freed on return)
    return 0;
}

int svr_region_fill_between(const uint32_t* in_mask_device, int nx, int ny, int nz, const svr_fill_between_params* p, uint32_t* out_mask_device,
                            svr_fill_between_info* info_or_null)
{
    const char* who = "svr_region_fill_between";
    if (!in_mask_device || !p || !out_mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    const bool unit = !p->weights[0] && !p->weights[1] && !p->weights[2];
    SliceAxes ax;
    uint32_t wu, wv;
    if (int e = check_planar(who, p->axis, unit ? nullptr : p->weights, nx, ny, nz, ax, wu, wv)) return e;
    if (p->flags & ~(uint32_t)(SVR_FILL_KEEP_BETWEEN | SVR_FILL_GAP_BY_GAP)) return failf(-3, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
    if (p->nkeys < 0) return failf(-3, "%s: nkeys is %d", who, (int)p->nkeys);
    if (p->keys)
        for (int i = 0; i < p->nkeys; ++i) {
            if (p->keys[i] < 0 || p->keys[i] >= ax.n) return failf(-3, "%s: key %d is %d, outside 0 .. %d", who, i, (int)p->keys[i], ax.n - 1);
            if (i && p->keys[i] <= p->keys[i - 1]) return failf(-3, "%s: the keys must increase strictly (key %d is %d after %d)", who, i, (int)p->keys[i], (int)p->keys[i - 1]);
        }
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t words = mask_words(d), plane = ax.plane();

    // The keys are known only after the first count, and the workspace only with the keys: the call counts (between g_pass_ev[0] and
    // [1]), waits, allocates, and only then starts the timer of the rest, so that no section's time holds a hipMalloc;
    // svr_region_fill_between_last_ms adds the two pieces.
    DeviceBuffer count_buf, table_buf, map_buf;
    PlanarWork pw;
    std::vector<uint64_t> counts((size_t)ax.n);
    SVR_HIP_TRY(count_buf.alloc((size_t)ax.n * sizeof(unsigned long long)));
    const bool ev = events_ready(g_pass_ev, 5);
    g_passes = g_fill_counts_ms = false;
    if (ev) hipEventRecord(g_pass_ev[0], st);
    SVR_HIP_TRY(launch_counts(st, in_mask_device, d, ax, count_buf.as<unsigned long long>()));
    if (ev) hipEventRecord(g_pass_ev[1], st);
    SVR_HIP_TRY(hipMemcpyAsync(counts.data(), count_buf.p, counts.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));

    svr_fill_between_info info;
    memset(&info, 0, sizeof info);
    info.axis = p->axis;
    info.first_key = info.last_key = -1;
    std::vector<int32_t> keys;
    if (p->keys) keys.assign(p->keys, p->keys + p->nkeys);
    for (int k = 0; k < ax.n; ++k) {
        info.voxels_in += counts[(size_t)k];
        if (!p->keys && counts[(size_t)k]) keys.push_back(k);
    }
    info.keys = (uint32_t)keys.size();
    if (!keys.empty()) { info.first_key = keys.front(); info.last_key = keys.back(); }

    // the keys that border a gap, in order, and the table of the slices inside the gaps
    struct Gap { int32_t a, b, ia, ib; };
    std::vector<Gap> gaps;
    std::vector<int32_t> bordering;
    std::vector<SliceEntry> table((size_t)ax.n, SliceEntry{0, 0, 0, 0});
    for (size_t i = 0; i + 1 < keys.size(); ++i) {
        const int32_t a = keys[i], b = keys[i + 1];
        if (b - a < 2) continue;
        if (bordering.empty() || bordering.back() != a) bordering.push_back(a);
        bordering.push_back(b);
        const int32_t ib = (int32_t)bordering.size() - 1;
        gaps.push_back(Gap{a, b, ib - 1, ib});
        for (int32_t k = a + 1; k < b; ++k) table[(size_t)k] = SliceEntry{ib - 1, ib, k - a, b - a};
        info.filled_slices += (uint32_t)(b - a - 1);
    }
    info.gaps = (uint32_t)gaps.size();
    info.workspace_bytes = (uint64_t)ax.n * sizeof(unsigned long long);

    // the launches: runs of consecutive gaps whose keys' maps fit the budget (at least one gap: two maps); GAP_BY_GAP: one gap each
    const size_t fit = MAP_BUDGET_VOXELS / plane;
    const size_t max_keys = (p->flags & SVR_FILL_GAP_BY_GAP) || fit < 2 ? 2 : fit;
    const auto run_end = [&](size_t g0) {
        size_t g1 = g0 + 1;
        while (g1 < gaps.size() && (size_t)(gaps[g1].ib - gaps[g0].ia + 1) <= max_keys) ++g1;
        return g1;
    };
    size_t widest = 0;
    for (size_t g0 = 0, g1; g0 < gaps.size(); g0 = g1) {
        g1 = run_end(g0);
        const size_t nk = (size_t)(gaps[g1 - 1].ib - gaps[g0].ia + 1);
        widest = nk > widest ? nk : widest;
    }
    if (!gaps.empty()) {
        SVR_HIP_TRY(table_buf.alloc(table.size() * sizeof(SliceEntry)));
        SVR_HIP_TRY(map_buf.alloc(widest * plane * sizeof(uint32_t)));
        SVR_HIP_TRY(pw.alloc(ax, widest));
        info.workspace_bytes += table.size() * sizeof(SliceEntry) + widest * plane * sizeof(uint32_t) + PlanarWork::bytes(ax, widest);
    }
    g_fill_counts_ms = ev;
    CallTimer timer(g_events, st);
    if (gaps.empty()) {
        hipLaunchKernelGGL(k_fill_copy, word_grid(words), dim3(MASK_THREADS), 0, st, in_mask_device, out_mask_device, d, words);
        SVR_HIP_TRY(hipGetLastError());
    } else {
        SVR_HIP_TRY(hipMemcpyAsync(table_buf.p, table.data(), table.size() * sizeof(SliceEntry), hipMemcpyHostToDevice, st));
        const uint32_t* src = in_mask_device;
        for (size_t g0 = 0, g1; g0 < gaps.size(); g0 = g1) {
            g1 = run_end(g0);
            const int first = gaps[g0].ia, last = gaps[g1 - 1].ib;
            if (ev) hipEventRecord(g_pass_ev[2], st);
            SVR_HIP_TRY(planar_maps(st, pw, in_mask_device, d, ax, wu, wv, bordering.data() + first, (size_t)(last - first + 1), map_buf.as<uint32_t>()));
            if (ev) hipEventRecord(g_pass_ev[3], st);
            hipLaunchKernelGGL(k_fill, lane_grid(words), dim3(MASK_THREADS), 0, st, src, table_buf.as<SliceEntry>(), map_buf.as<uint32_t>(), d, words, ax.axis, ax.nu,
                               plane, (int)gaps[g0].a, (int)gaps[g1 - 1].b, first, (p->flags & SVR_FILL_KEEP_BETWEEN) ? 1u : 0u, out_mask_device);
            SVR_HIP_TRY(hipGetLastError());
            if (ev) { hipEventRecord(g_pass_ev[4], st); g_passes = true; }
            src = out_mask_device;                                               // the launches after the first go on from the result so far
            ++info.launches;
        }
    }
    SVR_HIP_TRY(launch_counts(st, out_mask_device, d, ax, count_buf.as<unsigned long long>()));
    timer.stop();
    SVR_HIP_TRY(hipMemcpyAsync(counts.data(), count_buf.p, counts.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));                                        // (the table, the maps and the counters are freed on return)
    for (uint64_t c : counts) info.voxels_out += c;
    if (info_or_null) *info_or_null = info;
    return 0;
}

int svr_region_fill_between_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_region_fill_between_last_ms: null argument");
    *ms = g_events.last_ms();
    if (g_fill_counts_ms) *ms += elapsed_ms(g_pass_ev[0], g_pass_ev[1]);         // a fill counts before it can allocate, and times the rest after
    return 0;
}

int svr_region_fill_between_pass_ms(float* counts_ms, float* maps_ms, float* fill_ms)
{
    float* const out[3] = {counts_ms, maps_ms, fill_ms};
    const int from[3] = {0, 2, 3};
    for (int i = 0; i < 3; ++i)
        if (out[i]) *out[i] = g_passes ? elapsed_ms(g_pass_ev[from[i]], g_pass_ev[from[i] + 1]) : 0.f;
    return 0;
}

} // extern "C"
