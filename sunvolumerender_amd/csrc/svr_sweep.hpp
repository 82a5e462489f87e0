// svr_sweep.hpp -- the host loop that launches sweeps of a tile kernel until one of them changes nothing, shared by the grow kernel of
// svr_region_grow.hpp (svr_region.hip, svr_morph.hip) and the relaxation of svr_geo_relax.hpp (svr_geodesic.hip, svr_growcut.hip).  The dirty-map protocol of the kernels is
// described at the head of svr_region.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#ifndef SVR_REGION_BATCH
#define SVR_REGION_BATCH 16         // sweeps launched per read of the `added` counters (measured against 1 and 4: DESIGN.md 8h)
#endif

namespace {

// Launches sweeps until one of them adds nothing or `cap` sweeps are launched: batches of SVR_REGION_BATCH launches, one read of the
// `added` counters and one stream synchronisation per batch.  launch(cur, next, added) starts one sweep over `tiles` tiles that reads the
// dirty map `cur`, marks `next` and counts the tiles it changed in *added.  `dirty` holds 2 * tiles words, `added_device`
// SVR_REGION_BATCH.  *sweeps_out = the launches (surplus included), *done_out = the fixpoint was reached.  The stream is idle on return
// unless a HIP call failed.
template <class Launch>
inline hipError_t sweep_to_fixpoint(hipStream_t st, size_t tiles, uint32_t* dirty_maps, uint32_t* added_device, uint32_t cap, uint32_t* sweeps_out,
                                    bool* done_out, Launch launch)
{
    uint32_t* dirty[2] = {dirty_maps, dirty_maps + tiles};
    uint32_t sweeps = 0u;
    bool done = false;
    hipError_t e = hipSuccess;
    while (!done && sweeps < cap) {
        const uint32_t nb = cap - sweeps < (uint32_t)SVR_REGION_BATCH ? cap - sweeps : (uint32_t)SVR_REGION_BATCH;
        if ((e = hipMemsetAsync(added_device, 0, SVR_REGION_BATCH * sizeof(uint32_t), st)) != hipSuccess) break;
        for (uint32_t i = 0; i < nb; ++i) launch(dirty[(sweeps + i) & 1u], dirty[(sweeps + i + 1u) & 1u], added_device + i);
        if ((e = hipGetLastError()) != hipSuccess) break;
        sweeps += nb;
        uint32_t added[SVR_REGION_BATCH];
        if ((e = hipMemcpyAsync(added, added_device, sizeof added, hipMemcpyDeviceToHost, st)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) break;
        for (uint32_t i = 0; i < nb; ++i) if (added[i] == 0u) done = true;
    }
    *sweeps_out = sweeps;
    *done_out = done;
    return e;
}

} // namespace
