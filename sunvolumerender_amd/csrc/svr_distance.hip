// svr_distance.hip -- exact squared Euclidean distance maps of region masks with per-axis integer weights, and what is one cheap pass
// away from them: selection by distance, ball morphology, the largest inscribed ball, the map as a u16 volume (svr_region_distance,
// _distance_select, _ball, _distance_max, _distance_volume, _distance_weights; the contract is in include/svr_abi.h, the design in
// DESIGN.md 8k).  Integers only, on the mask layout and padding rule of svr_mask.hpp.
//
// The transform is separable: D(x, y, z) = min over (i, j, k) targets of wx (x - i)^2 + wy (y - j)^2 + wz (z - k)^2
//   = min_k [ wz (z - k)^2 + min_j [ wy (y - j)^2 + min_i wx (x - i)^2 ] ], and every min is over exact integers, so any correct
//   evaluation gives the same array.  SVR_DIST_NONE marks "no target on this row / in this slice / at all"; it is never added to.
//   (k_dist_rows and k_dist_columns live in svr_dist_passes.hpp, which svr_fillbetween.hip includes as well.)
//   k_dist_rows     one lane per voxel, 32 lanes per mask word: the nearest target bit at or left of the lane's bit and at or right of it,
//     by __clz / __ffs on the word and, where the word has none on that side, on the nearest non-zero word of the row on that side (a
//     scan of at most wx - 1 words that stops as soon as it cannot beat the other side).  TO_UNSET works on the complemented words with
//     the padding of the row's last word forced to "not a target".  Writes wx d^2 (4 B per voxel, coalesced rows).
//   k_dist_columns<MODE>  one thread per column of the axis (y, then z), lanes along x: the lower envelope of the parabolas
//     g(i) + w (u - i)^2 by Meijster's two scans.  The forward scan keeps a stack of (site s, first coordinate t at which s is the
//     minimiser), packed t << 16 | s in a GLOBAL workspace laid out [k][column] -- a site pushed has t < n <= 65536, so both fit 16 bits --
//     with the top entry and its g in registers; g of an entry uncovered by a pop is read back from the pass's input, which is why a pass
//     never writes the array it reads (rows -> A, y: A -> B, z: B -> A or the mask).  The separator of sites i < u,
//     floor((g(u) - g(i) + w (u^2 - i^2)) / (2 w (u - i))), is only ever taken when site i wins at its own t >= 0, which makes the
//     numerator non-negative: it is computed in double (both terms are below 2^50, so the quotient is within one of the floor) and fixed
//     up in 64-bit integers.  The backward scan walks u = n - 1 .. 0, evaluates the top site and pops at u == t.
//     MODE 0 writes the map; MODE 1 / 2 (the last pass of svr_region_ball) compare with r2 and write mask WORDS by ballot: d2 <= r2
//     (dilate, on the TO_SET map) or d2 > r2 (erode, on the TO_UNSET map) -- no 4 B per voxel map is written for a select to read back.
//     With SVR_DISTANCE_BRUTE the kernel is the literal O(n^2) min-plus product instead: the A/B build of tools/distance_time.py.
//   k_dist_select, k_dist_volume, k_dist_max: one lane per voxel.  k_dist_max reduces (d2 << 32) | ~index in the lane, then in the wave,
//     and issues one 64-bit atomicMax per wave: the largest d2 and, among equals, the smallest index.
// TERMINATION: no lane or block waits for another.  Every for loop runs to an axis length or a word count; the pop loop of the forward
//   scan removes one entry per turn from a stack that has received at most one entry per turn of the outer loop, so its turns total at
//   most n per column, and it is also counted against n.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"
#include "svr_mask.hpp"             // RegionDims, valid_bits, lane_at, half_ballot, the grids
#include "svr_dist_passes.hpp"      // k_dist_rows, k_dist_columns<MODE>, ColPass, THREADS, NONE, OUT_*
#include "svr_volume_host.hpp"

using svr::failf;

#define SVR_DISTANCE_COLUMN_BLOCK 256   // columns of a column pass that one block covers (= its threads); sunvolumerender_amd/abi.py mirrors it

namespace {

static_assert(SVR_DISTANCE_COLUMN_BLOCK == THREADS, "k_dist_columns runs one column per thread");

__global__ __launch_bounds__(THREADS) void k_dist_select(const uint32_t* __restrict__ d2, RegionDims d, size_t words, uint32_t lo2, uint32_t hi2,
                                                         uint32_t* __restrict__ out)
{
    const LaneAt a = lane_at(d, words);
    bool on = false;
    if (a.inside) {
        const uint32_t v = d2[a.v];
        on = v >= lo2 && v <= hi2;
    }
    const uint32_t word = half_ballot(on);
    if (a.bit == 0 && a.word_ok) out[a.i] = word;
}

__global__ __launch_bounds__(THREADS) void k_mask_clean(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, RegionDims d, size_t words)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < words) out[i] = in[i] & valid_bits((int)(i % (unsigned)d.wx), d);
}

__global__ __launch_bounds__(THREADS) void k_dist_volume(const uint32_t* __restrict__ d2, size_t n, uint32_t scale, uint16_t* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = d2[i];
    uint32_t res = 65535u;
    const uint64_t prod = (uint64_t)v * (uint64_t)(scale * scale);       // below 2^64: v < 2^32, scale^2 < 2^32
    if (v != NONE && prod < 65535ull * 65535ull) {        // the floor square root of a value below 2^32
        const uint32_t pv = (uint32_t)prod;
        uint32_t s = (uint32_t)sqrt((double)pv);
        if ((uint64_t)s * s > pv) --s;
        else if ((uint64_t)(s + 1u) * (s + 1u) <= pv) ++s;
        res = s;
    }
    out[i] = (uint16_t)res;
}

__global__ __launch_bounds__(THREADS) void k_dist_max(const uint32_t* __restrict__ d2, const uint32_t* __restrict__ mask, RegionDims d, size_t words,
                                                      unsigned long long* best)
{
    unsigned long long key = 0ull;                        // (d2 << 32) | ~index; 0 = none: ~index is never 0 for an index below 2^31
    const size_t total = words * 32u, step = (size_t)gridDim.x * THREADS;
    for (size_t t = (size_t)blockIdx.x * THREADS + threadIdx.x; t < total; t += step) {
        const LaneAt a = lane_at(t, d, words);
        if (!a.inside || (mask && !((mask[a.i] >> a.bit) & 1u))) continue;
        const uint32_t v = d2[a.v];
        if (v == NONE) continue;
        const unsigned long long k = ((unsigned long long)v << 32) | (unsigned long long)(uint32_t)~(uint32_t)a.v;
        key = k > key ? k : key;
    }
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)key, lane ^ off), hi = (uint32_t)__shfl((int)(uint32_t)(key >> 32), lane ^ off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        key = o > key ? o : key;
    }
    if (lane == 0 && key) atomicMax(best, key);
}

// ---------------- host side ----------------
// wx (nx - 1)^2 + wy (ny - 1)^2 + wz (nz - 1)^2 <= 0xFFFFFFFE, in 64-bit arithmetic that cannot wrap
bool weights_fit(const uint64_t w[3], int nx, int ny, int nz)
{
    const int dims[3] = {nx, ny, nz};
    uint64_t total = 0;
    for (int a = 0; a < 3; ++a) {
        const uint64_t e = (uint64_t)(dims[a] - 1), s = e * e;           // below 2^62
        if (s == 0) continue;
        if (w[a] > 0xFFFFFFFEull / s) return false;
        total += w[a] * s;                                // each term and the running sum stay below 2^34
        if (total > 0xFFFFFFFEull) return false;
    }
    return true;
}

int check_weights(const char* who, const uint32_t* weights_or_null, int nx, int ny, int nz, uint32_t w[3])
{
    for (int a = 0; a < 3; ++a) w[a] = weights_or_null ? weights_or_null[a] : 1u;
    if (!w[0] || !w[1] || !w[2]) return failf(-3, "%s: every weight must be at least 1 (got %u, %u, %u)", who, w[0], w[1], w[2]);
    const uint64_t w64[3] = {w[0], w[1], w[2]};
    if (!weights_fit(w64, nx, ny, nz))
        return failf(-3, "%s: the largest squared distance of %d x %d x %d under weights %u, %u, %u would overflow 32 bits", who, nx, ny, nz, w[0], w[1], w[2]);
    return 0;
}

CallEvents g_events;                                      // around the device work of the last call of this file (svr_region_distance_last_ms)
hipEvent_t g_pass_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // around the three passes of the last transform
bool g_passes = false;                                    // g_pass_ev have been recorded

// one transform: mask -> rows into a -> y pass into b -> z pass into a (MODE OUT_MAP; a is then the map) or into out_mask (OUT_LE / OUT_GT)
hipError_t transform(hipStream_t st, const uint32_t* mask, const RegionDims& d, const uint32_t w[3], bool unset, int mode, uint32_t r2, uint32_t* a,
                     uint32_t* b, uint32_t* stack, uint32_t* out_mask)
{
    const size_t words = mask_words(d), plane = (size_t)d.nx * d.ny;
    const bool ev = events_ready(g_pass_ev, 4);
    if (ev) hipEventRecord(g_pass_ev[0], st);
    hipLaunchKernelGGL(k_dist_rows, lane_grid(words), dim3(THREADS), 0, st, mask, a, d, words, w[0], unset ? 1 : 0);
    if (ev) hipEventRecord(g_pass_ev[1], st);
    ColPass py = {(uint32_t)d.ny, (uint32_t)d.nz, (uint32_t)d.nx, (uint32_t)d.wx, w[1], (size_t)d.nx, plane, (size_t)d.ny * d.wx, (size_t)d.wx,
                  (size_t)d.nz * d.nx};
    hipLaunchKernelGGL((k_dist_columns<OUT_MAP>), lane_grid((size_t)d.nz * d.wx), dim3(THREADS), 0, st, a, b, stack, py, 0u);
    if (ev) hipEventRecord(g_pass_ev[2], st);
    ColPass pz = {(uint32_t)d.nz, (uint32_t)d.ny, (uint32_t)d.nx, (uint32_t)d.wx, w[2], plane, (size_t)d.nx, (size_t)d.wx, (size_t)d.ny * d.wx,
                  (size_t)d.ny * d.nx};
    const dim3 gz = lane_grid((size_t)d.ny * d.wx);
    if (mode == OUT_MAP) hipLaunchKernelGGL((k_dist_columns<OUT_MAP>), gz, dim3(THREADS), 0, st, b, a, stack, pz, 0u);
    else if (mode == OUT_LE) hipLaunchKernelGGL((k_dist_columns<OUT_LE>), gz, dim3(THREADS), 0, st, b, out_mask, stack, pz, r2);
    else hipLaunchKernelGGL((k_dist_columns<OUT_GT>), gz, dim3(THREADS), 0, st, b, out_mask, stack, pz, r2);
    if (ev) { hipEventRecord(g_pass_ev[3], st); g_passes = true; }
    return hipGetLastError();
}

} // namespace

int svr::check_distance_weights(const char* who, const unsigned* weights_or_null, int nx, int ny, int nz, unsigned w[3])
{
    return check_weights(who, weights_or_null, nx, ny, nz, w);
}

extern "C" {

int svr_region_distance(const uint32_t* in_mask_device, int nx, int ny, int nz, const uint32_t* weights_or_null, int target, uint32_t* d2_device)
{
    const char* who = "svr_region_distance";
    if (!in_mask_device || !d2_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    uint32_t w[3];
    if (int e = check_weights(who, weights_or_null, nx, ny, nz, w)) return e;
    if (target != SVR_DIST_TO_SET && target != SVR_DIST_TO_UNSET) return failf(-3, "%s: unknown target %d", who, target);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t n = (size_t)nx * ny * nz;
    DeviceBuffer buf;                                     // the second map and the stacks: 8 bytes per voxel
    SVR_HIP_TRY(buf.alloc(2 * n * sizeof(uint32_t)));
    CallTimer timer(g_events, st);                        // (the launches, not the allocation)
    SVR_HIP_TRY(transform(st, in_mask_device, d, w, target == SVR_DIST_TO_UNSET, OUT_MAP, 0u, d2_device, buf.as<uint32_t>(), buf.as<uint32_t>() + n, nullptr));
    timer.stop();
    SVR_HIP_TRY(hipStreamSynchronize(st));                // (buf is freed on return)
    return 0;
}

int svr_region_distance_select(const uint32_t* d2_device, int nx, int ny, int nz, uint32_t lo2, uint32_t hi2, uint32_t* out_mask_device)
{
    const char* who = "svr_region_distance_select";
    if (!d2_device || !out_mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (lo2 > hi2) return failf(-3, "%s: the range must satisfy lo2 <= hi2 (got %u .. %u)", who, lo2, hi2);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t words = mask_words(d);
    hipLaunchKernelGGL(k_dist_select, lane_grid(words), dim3(THREADS), 0, st, d2_device, d, words, lo2, hi2, out_mask_device);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_region_ball(const uint32_t* in_mask_device, int nx, int ny, int nz, int op, const uint32_t* weights_or_null, uint32_t r2, uint32_t* out_mask_device)
{
    const char* who = "svr_region_ball";
    if (!in_mask_device || !out_mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (op != SVR_MORPH_DILATE && op != SVR_MORPH_ERODE && op != SVR_MORPH_OPEN && op != SVR_MORPH_CLOSE) return failf(-3, "%s: unknown op %d", who, op);
    uint32_t w[3];
    if (int e = check_weights(who, weights_or_null, nx, ny, nz, w)) return e;
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t words = mask_words(d), n = (size_t)nx * ny * nz;
    if (overlap(in_mask_device, words * sizeof(uint32_t), out_mask_device, words * sizeof(uint32_t))) return failf(-3, "%s: out must not overlap in", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    if (r2 == 0u) {                                       // the ball is the voxel itself: the identity, padding cleared
        CallTimer timer(g_events, st);
        hipLaunchKernelGGL(k_mask_clean, word_grid(words), dim3(THREADS), 0, st, in_mask_device, out_mask_device, d, words);
        SVR_HIP_TRY(hipGetLastError());
        return 0;
    }
    const bool two = op == SVR_MORPH_OPEN || op == SVR_MORPH_CLOSE;
    DeviceBuffer buf;                                     // two maps, the stacks, and the mask between the two halves of open / close
    SVR_HIP_TRY(buf.alloc((3 * n + (two ? words : 0)) * sizeof(uint32_t)));
    uint32_t *a = buf.as<uint32_t>(), *b = a + n, *stack = a + 2 * n, *mid = a + 3 * n;
    CallTimer timer(g_events, st);
    const bool erode_first = op == SVR_MORPH_ERODE || op == SVR_MORPH_OPEN;
    // dilate: d2 to the set voxels <= r2; erode: d2 to the unset voxels of the volume > r2
    SVR_HIP_TRY(transform(st, in_mask_device, d, w, erode_first, erode_first ? OUT_GT : OUT_LE, r2, a, b, stack, two ? mid : out_mask_device));
    if (two) SVR_HIP_TRY(transform(st, mid, d, w, !erode_first, erode_first ? OUT_LE : OUT_GT, r2, a, b, stack, out_mask_device));
    timer.stop();
    SVR_HIP_TRY(hipStreamSynchronize(st));                // (buf is freed on return)
    return 0;
}

int svr_region_distance_max(const uint32_t* d2_device, const uint32_t* mask_device_or_null, int nx, int ny, int nz, uint32_t* max_d2, uint32_t* first_index,
                            int32_t* status)
{
    const char* who = "svr_region_distance_max";
    if (!d2_device || !max_d2 || !first_index || !status) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    DeviceBuffer best_buf;
    SVR_HIP_TRY(best_buf.alloc(sizeof(unsigned long long)));
    unsigned long long* const d_best = best_buf.as<unsigned long long>();
    CallTimer timer(g_events, st);
    SVR_HIP_TRY(hipMemsetAsync(d_best, 0, sizeof(unsigned long long), st));
    const RegionDims d = make_dims(nx, ny, nz);
    const size_t words = mask_words(d);
    const size_t blocks = std::min<size_t>((words * 32 + THREADS - 1) / THREADS, 2048);       // the rest by the grid-stride loop
    hipLaunchKernelGGL(k_dist_max, dim3((uint32_t)blocks), dim3(THREADS), 0, st, d2_device, mask_device_or_null, d, words, d_best);
    SVR_HIP_TRY(hipGetLastError());
    timer.stop();
    unsigned long long best = 0ull;
    SVR_HIP_TRY(hipMemcpyAsync(&best, d_best, sizeof best, hipMemcpyDeviceToHost, st));
    SVR_HIP_TRY(hipStreamSynchronize(st));
    *max_d2 = (uint32_t)(best >> 32);
    *first_index = best ? ~(uint32_t)best : 0u;
    *status = best ? SVR_REGION_STATUS_OK : SVR_REGION_STATUS_EMPTY;
    return 0;
}

int svr_region_distance_volume(const uint32_t* d2_device, int nx, int ny, int nz, uint32_t scale, uint16_t* out_u16_device)
{
    const char* who = "svr_region_distance_volume";
    if (!d2_device || !out_u16_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (scale < 1u || scale > 65535u) return failf(-3, "%s: the scale must lie in 1 .. 65535 (got %u)", who, scale);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    const size_t n = (size_t)nx * ny * nz;
    hipLaunchKernelGGL(k_dist_volume, word_grid(n), dim3(THREADS), 0, st, d2_device, n, scale, out_u16_device);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_region_distance_weights(const double spacing[3], int nx, int ny, int nz, uint32_t weights[3], double* unit_out)
{
    const char* who = "svr_region_distance_weights";
    if (!spacing || !weights || !unit_out) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    for (int a = 0; a < 3; ++a)
        if (!(spacing[a] > 0.0) || !std::isfinite(spacing[a])) return failf(-3, "%s: the spacing must be positive and finite (got %g, %g, %g)", who, spacing[0], spacing[1], spacing[2]);
    const double smin = std::fmin(spacing[0], std::fmin(spacing[1], spacing[2]));
    for (int k = 4; k >= 0; --k) {
        const double unit = smin / (double)(1 << k);
        uint64_t w[3];
        bool ok = unit > 0.0;
        for (int a = 0; a < 3 && ok; ++a) {
            const double r = spacing[a] / unit, x = r * r;
            if (!(x < 4294967295.5)) { ok = false; break; }
            const long long v = std::llround(x);
            w[a] = v < 1 ? 1ull : (uint64_t)v;
        }
        if (!ok || !weights_fit(w, nx, ny, nz)) continue;
        for (int a = 0; a < 3; ++a) weights[a] = (uint32_t)w[a];
        *unit_out = unit;
        return 0;
    }
    return failf(-3, "%s: no unit of min(spacing) / 2^k, k = 4 .. 0, keeps the squared distances of %d x %d x %d at spacing %g, %g, %g inside 32 bits", who, nx, ny,
                 nz, spacing[0], spacing[1], spacing[2]);
}

int svr_region_distance_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_region_distance_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

int svr_region_distance_pass_ms(float* rows_ms, float* y_ms, float* z_ms)
{
    float* const out[3] = {rows_ms, y_ms, z_ms};
    for (int i = 0; i < 3; ++i)
        if (out[i]) *out[i] = g_passes ? elapsed_ms(g_pass_ev[i], g_pass_ev[i + 1]) : 0.f;
    return 0;
}

} // extern "C"
