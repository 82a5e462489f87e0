// svr_filter.hip -- exact filters that turn a u16 volume into a cleaner u16 volume before it is segmented: median / min / max over the
// unit element 6 / 18 / 26, and separable binomial smoothing (svr_volume_rank, _smooth, _smooth_radii, _filter_last_ms; the contract is
// in include/svr_abi.h, the design in DESIGN.md 8l).  Integers only; volumes are [nz][ny][nx]; the border replicates (an index outside
// the volume is clamped per axis), so a window always holds its 7 / 19 / 27 values and a binomial sum its 2 r + 1 taps.
//
// RANK (k_rank<OP, ELEMENT>): one block of 256 threads owns a tile of 128 x 8 x 8 outputs.  It fills an LDS tile of 130 x 10 x 10
//   voxels -- the outputs and a one-voxel halo, held as 65 x 10 x 10 packed pairs of u16 (26 000 bytes), a wave per tile row -- and the
//   clamp happens there, once per tile voxel, not per tap.  A thread then makes 16 PAIRS of x-adjacent outputs, (x, x + 1) with x even in the tile:
//   of each of the 9 rows around the pair it reads the two aligned words (c0 c1) and (c2 c3) that cover columns x - 1 .. x + 2 and
//   forms (c1 c2) from them; the three are the left neighbours, the centres and the right neighbours of BOTH outputs, so every
//   compare-exchange that follows is one v_pk_min_u16 and one v_pk_max_u16 for two outputs.  The element decides which rows give all
//   three and which only the centre.  Median is the selection of svr_rank_select.hpp; min and max fold the window.  All compares are
//   unsigned 16-bit.  No private array is indexed at run time: every loop over the window is unrolled.
//   A pair is stored as one 32-bit word where its address is 4-byte aligned and both voxels exist, else as u16 stores: with an odd nx
//   every other row starts at an odd u16 offset.  Global loads are u16 loads for the same reason.
// SMOOTH (k_smooth<R, ALONG_X>): one pass per axis with a radius > 0, in the order x, y, z.  One thread per output voxel, lanes along x
//   for every axis, so each of the 2 R + 1 taps is a coalesced row read (the repeats come from the caches).  The sum is an unsigned
//   32-bit integer: at most 65535 * 4^8 + 2^15 < 2^32.  The binomial coefficients are compile-time constants of the instantiation.
//   Only a voxel nearer than R to an end of its line clamps its tap indices; the others step one address by the stride.
// PASSES ping-pong between `out` and one temporary volume so that the last one lands in `out`; the source is never written.
//
// No block waits for another, and every loop runs to a compile-time bound or a tile count.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"

#include "svr_rank_select.hpp"
#include "svr_volume_host.hpp"      // (no mask here: FilterDims is this file's own)

using svr::failf;

namespace {

#ifndef SVR_FILTER_TILE_Z
#define SVR_FILTER_TILE_Z 8                               // the slices of a rank tile (an A/B knob of tools/filter_time.py)
#endif

constexpr int THREADS = 256;
constexpr int TX = 128, TY = 8, TZ = SVR_FILTER_TILE_Z;   // the outputs of a rank tile
constexpr int LW = TX / 2 + 1, LY = TY + 2, LZ = TZ + 2;  // the LDS tile in packed pairs: column pair j holds x0 - 1 + 2 j and the next
static_assert(TX / 2 * 4 == THREADS && TY % 4 == 0, "a thread owns one column pair of every fourth row");
static_assert(LW == 65 && LZ * LY <= THREADS, "the fill: 64 lanes a row, the 65th pair by one thread per row");

#ifndef SVR_SMOOTH_ROWS
#define SVR_SMOOTH_ROWS 8                                 // the rows one block of a smoothing pass walks (an A/B knob)
#endif
constexpr uint32_t SMOOTH_ROWS = SVR_SMOOTH_ROWS;

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

struct FilterDims { int nx, ny, nz; uint32_t tiles_x, tiles_y; };

__device__ inline us2 as_pair(uint32_t w) { return __builtin_bit_cast(us2, w); }
__device__ inline uint32_t as_word(us2 p) { return __builtin_bit_cast(uint32_t, p); }
__device__ inline int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// how much of row (dy, dz) the element admits: 3 = left, centre and right; 1 = the centre only; 0 = nothing
template <int ELEMENT>
__device__ constexpr int row_taps(int dy, int dz)
{
    const int off = (dy != 0) + (dz != 0);                // the row's own distance from the centre row, in steps
    return ELEMENT == 26 ? 3 : (ELEMENT == 18 ? (off == 2 ? 1 : 3) : (off == 0 ? 3 : (off == 1 ? 1 : 0)));
}

template <int OP, int ELEMENT>
__global__ __launch_bounds__(THREADS) void k_rank(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, FilterDims d)
{
    __shared__ uint32_t tile[LZ * LY * LW];
    const uint32_t b = blockIdx.x;
    const uint32_t tx = b % d.tiles_x, byz = b / d.tiles_x;
    const int x0 = (int)tx * TX, y0 = (int)(byz % d.tiles_y) * TY, z0 = (int)(byz / d.tiles_y) * TZ;

    // a wave fills every fourth row of the tile, a lane one column pair of it (the row's address is then the wave's, not the lane's);
    // the 65th pair of the rows is left to the first LZ * LY threads
    auto fill = [&](int r, int j) {
        const int y = clampi(y0 - 1 + r % LY, d.ny - 1), z = clampi(z0 - 1 + r / LY, d.nz - 1);
        const uint16_t* row = in + ((size_t)z * d.ny + y) * (size_t)d.nx;
        const uint32_t lo = row[clampi(x0 - 1 + 2 * j, d.nx - 1)], hi = row[clampi(x0 + 2 * j, d.nx - 1)];
        tile[r * LW + j] = lo | (hi << 16);
    };
    for (int r = threadIdx.x >> 6; r < LZ * LY; r += THREADS / 64) fill(r, threadIdx.x & 63);
    if (threadIdx.x < LZ * LY) fill(threadIdx.x, LW - 1);
    __syncthreads();

    constexpr int N = ELEMENT + 1;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int x = x0 + 2 * lx;
#pragma unroll 1
    for (int s = 0; s < TZ * TY / 4; ++s) {
        const int oy = (s % (TY / 4)) * 4 + ly, oz = s / (TY / 4);
        const int y = y0 + oy, z = z0 + oz;
        if (x >= d.nx || y >= d.ny || z >= d.nz) continue;
        us2 w[N];
        us2 acc = OP == SVR_FILTER_MIN ? (us2)(65535) : (us2)(0);
        int n = 0;
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int taps = row_taps<ELEMENT>(dy, dz);
                if (taps == 0) continue;
                const uint32_t* p = tile + ((oz + 1 + dz) * LY + (oy + 1 + dy)) * LW + lx;
                const uint32_t a = p[0], c = p[1];        // columns (x - 1, x) and (x + 1, x + 2)
                const us2 mid = as_pair((a >> 16) | (c << 16));
                if (OP == SVR_FILTER_MEDIAN) {
                    w[n++] = mid;
                    if (taps == 3) { w[n++] = as_pair(a); w[n++] = as_pair(c); }
                } else if (OP == SVR_FILTER_MIN) {
                    acc = svr_rank::rank_min(acc, mid);
                    if (taps == 3) acc = svr_rank::rank_min(acc, svr_rank::rank_min(as_pair(a), as_pair(c)));
                } else {
                    acc = svr_rank::rank_max(acc, mid);
                    if (taps == 3) acc = svr_rank::rank_max(acc, svr_rank::rank_max(as_pair(a), as_pair(c)));
                }
            }
        if (OP == SVR_FILTER_MEDIAN) acc = svr_rank::median<N>(w);
        uint16_t* q = out + ((size_t)z * d.ny + y) * (size_t)d.nx + x;
        if (x + 1 < d.nx && ((uintptr_t)q & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(q) = as_word(acc);
        } else {
            q[0] = acc.x;
            if (x + 1 < d.nx) q[1] = acc.y;
        }
    }
}

__host__ __device__ constexpr uint32_t binomial(int n, int k)
{
    uint64_t c = 1;
    for (int i = 1; i <= k; ++i) c = c * (uint64_t)(n - k + i) / (uint64_t)i;
    return (uint32_t)c;
}

// one binomial pass of radius R along `axis` (ALONG_X: axis 0, where the taps are neighbours in memory).  Block (x segment, row group):
// blockIdx.x = the segment of 256 x; the block walks the SMOOTH_ROWS rows from (blockIdx.z * gridDim.y + blockIdx.y) * SMOOTH_ROWS on,
// row = z * ny + y -- a block per row measured slower: 524 288 blocks of about a hundred instructions per thread at 512^3.  A voxel at least R from both ends of its
// line takes its taps one stride apart from one address; only the others clamp an index per tap (in a y or z pass a whole wave is
// on one side of that branch)
template <int R, bool ALONG_X>
__global__ __launch_bounds__(THREADS) void k_smooth(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, FilterDims d, uint32_t rows, int axis)
{
    const int x = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (x >= d.nx) return;
    const uint32_t row0 = (blockIdx.z * gridDim.y + blockIdx.y) * SMOOTH_ROWS;
#pragma unroll 1
    for (uint32_t row = row0; row < row0 + SMOOTH_ROWS && row < rows; ++row) {
        const size_t at = (size_t)row * (size_t)d.nx + (size_t)x;
        int pos, last;
        size_t stride;
        if (ALONG_X) { pos = x; last = d.nx - 1; stride = 1; }
        else {
            const uint32_t z = row / (uint32_t)d.ny, y = row - z * (uint32_t)d.ny;
            if (axis == 1) { pos = (int)y; last = d.ny - 1; stride = (size_t)d.nx; }
            else { pos = (int)z; last = d.nz - 1; stride = (size_t)d.nx * (size_t)d.ny; }
        }
        uint32_t acc = 1u << (2 * R - 1);
#ifndef SVR_SMOOTH_CLAMP_ALWAYS                              // (an A/B build of tools/filter_time.py clamps every tap)
        if (pos >= R && pos + R <= last) {
            const uint16_t* p = in + (at - (size_t)R * stride);
#pragma unroll
            for (int k = 0; k <= 2 * R; ++k) {
                acc += binomial(2 * R, k) * (uint32_t)*p;
                p += stride;
            }
        } else
#endif
        {
            const uint16_t* line = in + (at - (size_t)pos * stride);  // entry 0 of this voxel's line along the axis
#pragma unroll
            for (int k = 0; k <= 2 * R; ++k) acc += binomial(2 * R, k) * (uint32_t)line[(size_t)clampi(pos - R + k, last) * stride];
        }
        out[at] = (uint16_t)(acc >> (2 * R));
    }
}

// ---------------- host side ----------------
CallEvents g_events;                                      // around the device work of the last rank / smooth call (svr_volume_filter_last_ms)

FilterDims make_dims(int nx, int ny, int nz)
{
    return FilterDims{nx, ny, nz, (uint32_t)((nx + TX - 1) / TX), (uint32_t)((ny + TY - 1) / TY)};
}

template <int OP>
void launch_rank_op(int element, dim3 grid, hipStream_t st, const uint16_t* in, uint16_t* out, const FilterDims& d)
{
    if (element == 6) hipLaunchKernelGGL((k_rank<OP, 6>), grid, dim3(THREADS), 0, st, in, out, d);
    else if (element == 18) hipLaunchKernelGGL((k_rank<OP, 18>), grid, dim3(THREADS), 0, st, in, out, d);
    else hipLaunchKernelGGL((k_rank<OP, 26>), grid, dim3(THREADS), 0, st, in, out, d);
}

void launch_rank(int op, int element, hipStream_t st, const uint16_t* in, uint16_t* out, const FilterDims& d)
{
    // ceil(nx / 128) ceil(ny / 8) ceil(nz / 8) tiles: below the voxel count, so below 2^31, unless the volume is one voxel and one tile
    const dim3 grid((uint32_t)((size_t)d.tiles_x * d.tiles_y * (size_t)((d.nz + TZ - 1) / TZ)));
    if (op == SVR_FILTER_MEDIAN) launch_rank_op<SVR_FILTER_MEDIAN>(element, grid, st, in, out, d);
    else if (op == SVR_FILTER_MIN) launch_rank_op<SVR_FILTER_MIN>(element, grid, st, in, out, d);
    else launch_rank_op<SVR_FILTER_MAX>(element, grid, st, in, out, d);
}

void launch_smooth(int axis, uint32_t r, hipStream_t st, const uint16_t* in, uint16_t* out, const FilterDims& d)
{
    const uint32_t rows = (uint32_t)((size_t)d.ny * (size_t)d.nz);   // at most 2^31
    const uint32_t groups = (rows + SMOOTH_ROWS - 1) / SMOOTH_ROWS;
    const uint32_t gy = groups < 65535u ? groups : 65535u, gz = (groups + gy - 1) / gy;          // gz <= 32769
    const dim3 grid((uint32_t)((d.nx + THREADS - 1) / THREADS), gy, gz);
#define SMOOTH_CASE(R)                                                                                          \
    case R:                                                                                                     \
        if (axis == 0) hipLaunchKernelGGL((k_smooth<R, true>), grid, dim3(THREADS), 0, st, in, out, d, rows, axis);  \
        else hipLaunchKernelGGL((k_smooth<R, false>), grid, dim3(THREADS), 0, st, in, out, d, rows, axis);          \
        break
    switch (r) {
        SMOOTH_CASE(1); SMOOTH_CASE(2); SMOOTH_CASE(3); SMOOTH_CASE(4); SMOOTH_CASE(5); SMOOTH_CASE(6); SMOOTH_CASE(7); SMOOTH_CASE(8);
        default: break;
    }
#undef SMOOTH_CASE
    static_assert(SVR_SMOOTH_MAX_RADIUS == 8, "two instantiations of k_smooth per radius");
}

} // namespace

extern "C" {

int svr_volume_rank(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, int op, int element, uint32_t iterations,
                    uint16_t* out_u16_device)
{
    const char* who = "svr_volume_rank";
    if (!voxels || !out_u16_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    if (op != SVR_FILTER_MEDIAN && op != SVR_FILTER_MIN && op != SVR_FILTER_MAX) return failf(-3, "%s: unknown op %d", who, op);
    if (int e = check_connectivity(who, "element", element)) return e;
    if (iterations < 1u || iterations > SVR_FILTER_MAX_ITERATIONS)
        return failf(-3, "%s: iterations must lie in 1 .. %d (got %u)", who, SVR_FILTER_MAX_ITERATIONS, iterations);
    const size_t n = (size_t)nx * ny * nz, bytes = n * sizeof(uint16_t);
    if (src_is_device && overlap(voxels, bytes, out_u16_device, bytes)) return failf(-3, "%s: out must not overlap voxels", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const FilterDims d = make_dims(nx, ny, nz);
    DeviceVoxels dv;
    DeviceBuffer tmp;
    SVR_HIP_TRY(dv.get(voxels, n, src_is_device, st));
    if (iterations > 1u) SVR_HIP_TRY(tmp.alloc(bytes));
    CallTimer timer(g_events, st);
    const uint16_t* src = dv.p;
    for (uint32_t i = 0; i < iterations; ++i) {
        uint16_t* dst = (iterations - 1u - i) % 2u == 0u ? out_u16_device : tmp.as<uint16_t>();    // the last pass writes `out`
        launch_rank(op, element, st, src, dst, d);
        src = dst;
    }
    SVR_HIP_TRY(hipGetLastError());
    timer.stop();
    if (dv.owned() || tmp) SVR_HIP_TRY(hipStreamSynchronize(st));     // the upload and the temporary are freed on return
    return 0;
}

int svr_volume_smooth(const uint16_t* voxels, int nx, int ny, int nz, int src_is_device, const uint32_t* radii_xyz, uint16_t* out_u16_device)
{
    const char* who = "svr_volume_smooth";
    if (!voxels || !radii_xyz || !out_u16_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims(who, nx, ny, nz)) return e;
    for (int a = 0; a < 3; ++a)
        if (radii_xyz[a] > SVR_SMOOTH_MAX_RADIUS)
            return failf(-3, "%s: a radius must be at most %d (got %u, %u, %u)", who, SVR_SMOOTH_MAX_RADIUS, radii_xyz[0], radii_xyz[1], radii_xyz[2]);
    const size_t n = (size_t)nx * ny * nz, bytes = n * sizeof(uint16_t);
    if (src_is_device && overlap(voxels, bytes, out_u16_device, bytes)) return failf(-3, "%s: out must not overlap voxels", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    const FilterDims d = make_dims(nx, ny, nz);
    int axes[3], passes = 0;
    for (int a = 0; a < 3; ++a)
        if (radii_xyz[a] > 0u) axes[passes++] = a;
    if (passes == 0) {                                    // a copy
        CallTimer timer(g_events, st);
        SVR_HIP_TRY(hipMemcpyAsync(out_u16_device, voxels, bytes, src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        timer.stop();
        if (!src_is_device) SVR_HIP_TRY(hipStreamSynchronize(st));    // the host array is the caller's again on return
        return 0;
    }
    DeviceVoxels dv;
    DeviceBuffer tmp;
    SVR_HIP_TRY(dv.get(voxels, n, src_is_device, st));
    if (passes > 1) SVR_HIP_TRY(tmp.alloc(bytes));
    CallTimer timer(g_events, st);
    const uint16_t* src = dv.p;
    for (int i = 0; i < passes; ++i) {
        uint16_t* dst = (passes - 1 - i) % 2 == 0 ? out_u16_device : tmp.as<uint16_t>();
        launch_smooth(axes[i], radii_xyz[axes[i]], st, src, dst, d);
        src = dst;
    }
    SVR_HIP_TRY(hipGetLastError());
    timer.stop();
    if (dv.owned() || tmp) SVR_HIP_TRY(hipStreamSynchronize(st));     // the upload and the temporary are freed on return
    return 0;
}

int svr_volume_smooth_radii(const double spacing[3], double sigma, uint32_t radii[3], double sigma_out[3])
{
    const char* who = "svr_volume_smooth_radii";
    if (!spacing || !radii) return failf(-4, "%s: null argument", who);
    for (int a = 0; a < 3; ++a)
        if (!(spacing[a] > 0.0) || !std::isfinite(spacing[a]))
            return failf(-3, "%s: the spacing must be positive and finite (got %g, %g, %g)", who, spacing[0], spacing[1], spacing[2]);
    if (!(sigma >= 0.0) || !std::isfinite(sigma)) return failf(-3, "%s: sigma must be finite and not negative (got %g)", who, sigma);
    uint32_t r[3];
    for (int a = 0; a < 3; ++a) {
        const double q = sigma / spacing[a], v = 2.0 * q * q;        // the variance of radius r is r / 2 voxels^2
        if (!(v < (double)SVR_SMOOTH_MAX_RADIUS + 0.5))
            return failf(-3, "%s: sigma %g at spacing %g needs a radius above %d on axis %d", who, sigma, spacing[a], SVR_SMOOTH_MAX_RADIUS, a);
        r[a] = (uint32_t)std::llround(v);
    }
    for (int a = 0; a < 3; ++a) {
        radii[a] = r[a];
        if (sigma_out) sigma_out[a] = std::sqrt((double)r[a] / 2.0) * spacing[a];
    }
    return 0;
}

int svr_volume_filter_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_volume_filter_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

} // extern "C"
