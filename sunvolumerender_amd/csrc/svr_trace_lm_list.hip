// svr_trace_lm_list.hip -- the local-majorant kernels (SVR_OPT_LOCAL_MAJORANT: the pools and their straight-line form) for the launches of adaptive sampling
// (svr_render_pathtracer_adaptive): the same source as svr_trace_lm.hip, compiled a second time into namespace svr_list with the task
// order over a list of 16 x 16 tiles (svr_tile_tasks.hpp, SVR_TILE_LIST).  The ordinary builds keep their code and registers.
#define SVR_TILE_LIST 1
#define svr svr_list
#include "svr_trace_lm.hip"
#undef svr

namespace svr_list {
// type-erased entry for svr_api_trace.hip (its DevScene / DevWork / LaunchCfg are the layout-identical types of namespace svr)
hipError_t launch_trace_lm_raw(const void* scene, const void* work, const void* cfg, hipStream_t st)
{
    return launch_trace_lm(*static_cast<const DevScene*>(scene), *static_cast<const DevWork*>(work), *static_cast<const LaunchCfg*>(cfg), st);
}
}
