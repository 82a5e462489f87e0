// svr_hits.hpp -- launch interface of the hit kernel (svr_hits.hip): the hit maps of svr_render_hits and the point picks of
// svr_pick (include/svr_abi.h, "hit maps and picks").
#pragma once
#include "svr_kernels.hpp"

namespace svr {

enum { HIT_OPACITY = 1, HIT_ISO = 2, HIT_MAX = 3 };               // SVR_HIT_*
enum { HIT_STATUS_MISS = 0, HIT_STATUS_NONE = 1, HIT_STATUS_FOUND = 2 };   // SVR_HIT_STATUS_*
constexpr uint32_t HIT_WORDS = 10;                                // svr_hit: ten 4-byte members

// what the kernel needs beyond the scene.  The macro grid itself (mc_shift, mc_gx .. mc_gxy) travels in DevScene.
struct DevHits {
    int32_t mode;                  // HIT_*
    float alpha, iso;
    uint32_t* out;                 // svr_hit records: the map (imageW x imageH, row-major) or the pick list (n_pick)
    const uint32_t* pixels;        // device copy of the pick list, (x, y) pairs; null = the map over the owned pixels of the work
    uint32_t n_pick;
    MarchTables tb;                // skipping (MarchTables, svr_kernels.hpp): mm / nbmax for ISO and MAX, empty / deep for OPACITY; all null = every sample is fetched
};

// hit records of the owned pixels of work, or of the pick list
hipError_t launch_hits(const DevScene& scene, const DevWork& work, const DevHits& hp, float stepSize, bool count, int num_cus, hipStream_t stream);

} // namespace svr
