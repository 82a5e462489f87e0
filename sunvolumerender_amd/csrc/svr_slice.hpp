// svr_slice.hpp -- launch interface of the slice kernel (svr_slice.hip): planes and slabs through the volume,
// svr_render_slice / svr_render_slice_stack (include/svr_abi.h).
#pragma once
#include "svr_kernels.hpp"

namespace svr {

enum { SLICE_PLANE = 0, SLAB_MIP = 1, SLAB_MINIP = 2, SLAB_MEAN = 3 };   // SVR_SLAB_*; PLANE: thickness 0, the single sample
constexpr uint32_t SLICE_COLOR_TF = 1u;                                 // SVR_SLICE_COLOR_TF

// what the kernel needs beyond the scene and the work window.  The macro grid (mc_shift, mc_gx .. mc_gxy) travels in DevScene,
// the image size in DevScene::imageW / imageH.
struct DevSlice {
    float center[3], u[3], v[3], n[3];   // n = normalize(cross(u, v)), computed on the host as the header defines it
    float box_lo[3], box_hi[3];          // the clipped box, lo <= hi per axis
    float half_thickness;                // 0.5f * thickness
    float step;                          // 0 for SLICE_PLANE (d_0 = 0)
    float spacing;                       // between the slices of a stack
    uint32_t K;                          // samples per pixel
    uint32_t count;                      // slices
    int32_t mode;                        // SLICE_PLANE or SLAB_*
    uint32_t flags;
    float window_lo, window_hi;
    uint32_t counting;                   // SVR_OPT_COUNT
    const uint16_t* mm;                  // the volume's min/max table (2 x u16 per macro-cell); null = every counting sample is fetched
};

// count images over the owned pixels of work (work.img: count x RGBA8 images of scene.imageW x scene.imageH, back to back)
hipError_t launch_slice(const DevScene& scene, const DevWork& work, const DevSlice& sl, int num_cus, hipStream_t stream);

} // namespace svr
