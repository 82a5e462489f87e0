// svr_denoise.hpp -- launch interface of the denoised preview (svr_denoise.hip) for the C-ABI layer (svr_api_converge.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "svr_scene.hpp"

namespace svr {

struct DenoiseArgs {
    uint32_t W, H;
    int passes;                    // a-trous passes, steps 1, 2, 4 ... 2^(passes-1)
    float sigma_depth, sigma_normal, sigma_albedo, sigma_opacity, sigma_color;   // <= 0: the term is off
    float pix_scale;               // pixel footprint per unit of depth: 2 tan(fovx / 2) / (H - 1)
    float exposure;                // of the tone map
};

// guides of the scene: 2 float4 per pixel, (N.xyz, D) and (A.rgb, O); h = march step (world units).  Uses scene.empty_mask if set.
hipError_t launch_guides(const DevScene& scene, float4* guides, float h, hipStream_t stream);
// the filter over a whole W x H accumulator: scratch = 2 W H float4; img (RGBA8, tone-mapped) or, if null, hdr_out (float3)
hipError_t launch_denoise(const float* hdr, const float4* guides, float4* scratch, uint8_t* img, float* hdr_out, const DenoiseArgs& args,
                          hipStream_t stream);

} // namespace svr
