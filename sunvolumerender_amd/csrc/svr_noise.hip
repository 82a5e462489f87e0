// svr_noise.hip -- noise estimate of a progressive render from two of its accumulators (SVR_OPT_NOISE_ESTIMATE, svr_estimate_noise).
//
//  k_noise_tiles  A(m) and A(n) (running means after m < n frames) -> per pixel, in the tone-mapped domain T(L) = (1 - e^(-16 exposure L))^2.2
//                 (tonemapping.h:13-27 before quantisation; T(0) = 0, both arguments clamped at 0):
//                   B    = A(n) + m / (n - m) (A(n) - A(m))          the mean of frames m+1 .. n, independent of A(m)
//                   d^2  = mean over the 3 channels of (T(A(m)) - T(B))^2
//                   e^2  = d^2 m (n - m) / n^2                       predicted squared error of T(A(n)) (delta method)
//                 summed per 16 x 16 tile over the COUNTED pixels: owned (row shard / window) with all 6 values finite; owned pixels with a
//                 non-finite value are counted apart.  Writes the tile RMSE sqrt(sum e^2 / counted) (NaN for a tile without a counted
//                 pixel), the tile's sum (double) and its two counts; optionally A(n) over A(m) in the same pass (the snapshot of the
//                 library's state).  A block = 64 x 16 pixels = 4 tiles side by side: a wave reads 64 consecutive pixels of a row (768 B).
//                 With a tile map (adaptive sampling: 1 = the tile is still traced) the other tiles are neither estimated nor snapshotted and
//                 their tile arrays keep their values, so k_noise_total sums them with the rest.
//  k_noise_total  one block: the sums over all tiles (double, fixed order: deterministic) and the largest tile RMSE.
// Purely memory-bound: 24 B read + 12 B written per pixel (fused form).  The trace kernels and the accumulator are not touched.
#include "svr_noise.hpp"

namespace svr {

namespace {

constexpr uint32_t NB_X = 64, NB_ROWS = 4;     // block: 64 pixels x 4 rows, 4 passes over the 16 rows of a tile row

// the tone curve before quantisation; k = -16 exposure.  expm1f keeps the relative precision of dark pixels (1 - e^x cancels)
__device__ __forceinline__ float noise_tm(float L, float k)
{
    const float l = -expm1f(fmaxf(L, 0.f) * k);
    return l > 0.f ? exp2f(2.2f * log2f(l)) : 0.f;
}

__device__ __forceinline__ bool fin(float v) { return __builtin_isfinite(v); }

template <bool WRITE_REF>
__global__ __launch_bounds__(256) void k_noise_tiles(float* __restrict__ ref, const float* __restrict__ hdr, const NoiseArgs a,
                                                      float* __restrict__ tile_rmse, double* __restrict__ tile_sse, uint32_t* __restrict__ tile_cnt,
                                                      const uint8_t* __restrict__ active)
{
    __shared__ double s_sse[256];
    __shared__ uint32_t s_cnt[256], s_nf[256];
    const uint32_t px = threadIdx.x & (NB_X - 1u), rg = threadIdx.x / NB_X;
    const uint32_t x = blockIdx.x * NB_X + px;
    const float k = -16.f * a.exposure;
    double sse = 0.0;
    uint32_t cnt = 0, nf = 0;
    bool col_owned = x < a.W && x >= a.x0 && x < a.x1;
    if (active != nullptr && col_owned && !active[(size_t)blockIdx.y * a.tiles_x + x / NOISE_TILE]) col_owned = false;
#pragma unroll
    for (uint32_t r = 0; r < NOISE_TILE / NB_ROWS; ++r) {
        const uint32_t y = blockIdx.y * NOISE_TILE + r * NB_ROWS + rg;
        if (!col_owned || y >= a.H || y < a.y0 || y >= a.y1) continue;
        if (a.world > 1u && (y / a.strip_rows) % a.world != a.rank) continue;
        const size_t off = 3u * ((size_t)y * a.W + x);
        const float n0 = hdr[off], n1 = hdr[off + 1], n2 = hdr[off + 2];
        const float m0 = ref[off], m1 = ref[off + 1], m2 = ref[off + 2];
        if (WRITE_REF) { ref[off] = n0; ref[off + 1] = n1; ref[off + 2] = n2; }
        if (!(fin(n0) && fin(n1) && fin(n2) && fin(m0) && fin(m1) && fin(m2))) { ++nf; continue; }
        const float dd0 = noise_tm(m0, k) - noise_tm(n0 + a.ratio * (n0 - m0), k);
        const float dd1 = noise_tm(m1, k) - noise_tm(n1 + a.ratio * (n1 - m1), k);
        const float dd2 = noise_tm(m2, k) - noise_tm(n2 + a.ratio * (n2 - m2), k);
        const float d2 = (dd0 * dd0 + dd1 * dd1 + dd2 * dd2) / 3.f;
        sse += (double)d2 * (double)a.scale;
        ++cnt;
    }
    s_sse[threadIdx.x] = sse;
    s_cnt[threadIdx.x] = cnt;
    s_nf[threadIdx.x] = nf;
    __syncthreads();
    // thread t < 4 sums tile t of the block: its 16 columns in each of the 4 row groups, in a fixed order
    const uint32_t t = threadIdx.x;
    const uint32_t tx = blockIdx.x * (NB_X / NOISE_TILE) + t;
    if (t >= NB_X / NOISE_TILE || tx >= a.tiles_x) return;
    if (active != nullptr && !active[(size_t)blockIdx.y * a.tiles_x + tx]) return;
    double s = 0.0;
    uint32_t c = 0, f = 0;
    for (uint32_t g = 0; g < NB_ROWS; ++g)
        for (uint32_t l = 0; l < NOISE_TILE; ++l) {
            const uint32_t i = g * NB_X + t * NOISE_TILE + l;
            s += s_sse[i];
            c += s_cnt[i];
            f += s_nf[i];
        }
    const size_t ti = (size_t)blockIdx.y * a.tiles_x + tx;
    tile_rmse[ti] = c ? (float)sqrt(s / (double)c) : __builtin_nanf("");
    tile_sse[ti] = s;
    tile_cnt[2 * ti] = c;
    tile_cnt[2 * ti + 1] = f;
}

__global__ __launch_bounds__(1024) void k_noise_total(const float* __restrict__ tile_rmse, const double* __restrict__ tile_sse,
                                                      const uint32_t* __restrict__ tile_cnt, uint32_t ntiles, NoiseTotals* __restrict__ out)
{
    __shared__ double s_sse[1024];
    __shared__ unsigned long long s_cnt[1024], s_nf[1024];
    __shared__ float s_max[1024];
    const uint32_t t = threadIdx.x;
    double s = 0.0;
    unsigned long long c = 0, f = 0;
    float mx = -1.f;
    for (uint32_t i = t; i < ntiles; i += 1024u) {
        s += tile_sse[i];
        c += tile_cnt[2 * i];
        f += tile_cnt[2 * i + 1];
        if (tile_cnt[2 * i] != 0u) mx = fmaxf(mx, tile_rmse[i]);
    }
    s_sse[t] = s; s_cnt[t] = c; s_nf[t] = f; s_max[t] = mx;
    __syncthreads();
    for (uint32_t h = 512; h > 0; h >>= 1) {
        if (t < h) {
            s_sse[t] += s_sse[t + h];
            s_cnt[t] += s_cnt[t + h];
            s_nf[t] += s_nf[t + h];
            s_max[t] = fmaxf(s_max[t], s_max[t + h]);
        }
        __syncthreads();
    }
    if (t == 0) {
        NoiseTotals r;
        r.sse = s_sse[0];
        r.pixels = s_cnt[0];
        r.nonfinite = s_nf[0];
        r.tile_max = s_max[0] < 0.f ? __builtin_nanf("") : s_max[0];
        r._pad = 0;
        *out = r;
    }
}

} // namespace

hipError_t launch_noise(float* ref, const float* hdr, bool write_ref, const NoiseArgs& a, float* tile_rmse, double* tile_sse,
                        uint32_t* tile_cnt, NoiseTotals* totals, hipStream_t stream, const uint8_t* active)
{
    const dim3 grid((a.W + NB_X - 1u) / NB_X, a.tiles_y);
    if (write_ref) hipLaunchKernelGGL(k_noise_tiles<true>, grid, dim3(256), 0, stream, ref, hdr, a, tile_rmse, tile_sse, tile_cnt, active);
    else hipLaunchKernelGGL(k_noise_tiles<false>, grid, dim3(256), 0, stream, ref, hdr, a, tile_rmse, tile_sse, tile_cnt, active);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_noise_total, dim3(1), dim3(1024), 0, stream, tile_rmse, tile_sse, tile_cnt, a.tiles_x * a.tiles_y, totals);
    return hipGetLastError();
}

} // namespace svr
