// svr_noise.hpp -- launch interface of the noise estimate of progressive renders (svr_noise.hip) for the C-ABI layer (svr_api_converge.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svr {

constexpr uint32_t NOISE_TILE = 16;            // tiles of the estimate: 16 x 16 pixels, aligned to the image

struct NoiseArgs {
    uint32_t W, H;                             // the whole frame (both accumulators are W x H packed float3)
    uint32_t tiles_x, tiles_y;                 // ceil(W / 16), ceil(H / 16)
    uint32_t x0, x1, y0, y1;                   // owned pixels: [x0, x1) x [y0, y1) ...
    uint32_t strip_rows, rank, world;          // ... and, if world > 1, the rows y with (y / strip_rows) % world == rank
    float exposure;                            // of the tone map
    float ratio;                               // m / (n - m): the mean of frames m+1 .. n is B = A(n) + ratio (A(n) - A(m))
    float scale;                               // m (n - m) / n^2: predicted squared error e^2 = d^2 scale
};

// sums over the tiles (k_noise_total); 32 B
struct NoiseTotals {
    double sse;                                // sum of e^2 over the counted pixels
    unsigned long long pixels, nonfinite;      // counted pixels, owned pixels with a non-finite value in A(m) or A(n)
    float tile_max;                            // largest tile RMSE (NaN if no tile has a counted pixel)
    uint32_t _pad;
};

// Per-tile buffers: tile_rmse (float), tile_sse (double) and tile_cnt (2 x uint32: counted, non-finite) of tiles_x * tiles_y tiles.
// ref = A(m) (W x H packed float3); write_ref: A(n) is written over it in the same pass (each element is read, then overwritten, by the
// same thread).  Both kernels run on `stream`: the tile pass, then one block that sums the tiles into *totals.  active (adaptive sampling):
// null = every tile, else one byte per tile (row-major): the tiles with 0 are skipped and keep their values in the tile arrays.
hipError_t launch_noise(float* ref, const float* hdr, bool write_ref, const NoiseArgs& args, float* tile_rmse, double* tile_sse,
                        uint32_t* tile_cnt, NoiseTotals* totals, hipStream_t stream, const uint8_t* active = nullptr);

} // namespace svr
