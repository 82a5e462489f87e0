// svr_project.hpp -- launch interface of the projection kernel (svr_project.hip): maximum / mean intensity projection
// and the shaded isosurface of svr_render_projection (include/svr_abi.h).
#pragma once
#include "svr_kernels.hpp"

namespace svr {

enum { PROJ_MIP = 1, PROJ_MEAN = 2, PROJ_ISO = 3 };          // SVR_PROJ_*
constexpr uint32_t PROJ_COLOR_TF = 1u;                        // SVR_PROJ_COLOR_TF

// what the kernel needs beyond the scene.  The macro grid itself (mc_shift, mc_gx .. mc_gxy) travels in DevScene.
struct DevProjection {
    int32_t mode;                  // PROJ_*
    uint32_t flags;
    float iso, window_lo, window_hi;
    MarchTables tb;                // skipping (MarchTables, svr_kernels.hpp): mm, and nbmax if leap; mm null = every sample is fetched
};

// nbmax[m] = max of mm[2 m' + 1] over the in-grid 3 x 3 x 3 neighbourhood of m
hipError_t launch_nbmax(const uint16_t* mm, uint16_t* nbmax, int gx, int gy, int gz, hipStream_t stream);
// one projection image over the owned pixels of work (work.img: RGBA8)
hipError_t launch_projection(const DevScene& scene, const DevWork& work, const DevProjection& pj, float stepSize, bool count, int num_cus, hipStream_t stream);

} // namespace svr
