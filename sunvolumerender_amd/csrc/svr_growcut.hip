// svr_growcut.hip -- grow-from-seeds: every voxel goes to the class whose markers reach it over the path that crosses the least image
// contrast (Fast GrowCut, Zhu et al.: the shortest-path form of GrowCut), and the two calls that turn picks and masks into class markers
// (svr_region_growcut, _growcut_params_default, _seed_classes, _label_paint, _growcut_last_ms; the contract is in include/svr_abi.h, the
// design in DESIGN.md 8q).  The keys, the relaxation under ContrastCost (the move cost, the saturating add and why the result is still
// unique) and its host driver are in svr_geo_relax.hpp; here are the parameter checks, the report of a saturated cost and k_gc_paint
// (one lane per voxel).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>

#include "../../include/svr_abi.h"
#include "svr_internal.hpp"
#include "svr_geo_relax.hpp"        // ContrastCost, geo_run, place_seeds, check_geo_outputs, classes_of; the mask layout and the host scaffolding

using svr::failf;

namespace {

__global__ __launch_bounds__(LANE_THREADS) void k_gc_paint(uint32_t* __restrict__ labels, const uint32_t* __restrict__ mask, RegionDims d, size_t words,
                                                           uint32_t label, int only_unlabelled)
{
    const LaneAt a = lane_at(d, words);
    if (!a.inside || !((mask[a.i] >> a.bit) & 1u)) return;
    if (only_unlabelled && labels[a.v] != 0u) return;
    labels[a.v] = label;
}

// ---------------- host side ----------------
int check_dims3(const char* who, const int32_t* d) { return check_dims(who, d[0], d[1], d[2]); }

int check_params(const char* who, const svr_growcut_params* p, ContrastCost* out)
{
    uint64_t wmax = 0;
    for (int c = 0; c < 7; ++c) {
        out->gw.w[c] = p->step_weights[c];
        wmax = p->step_weights[c] > wmax ? p->step_weights[c] : wmax;
    }
    if (wmax == 0) return failf(-3, "%s: all seven step weights are 0: no move is allowed", who);
    if (p->contrast_gain > 65535u) return failf(-3, "%s: contrast_gain must lie in 0 .. 65535 (got %u)", who, p->contrast_gain);
    if (p->contrast_shift > 15u) return failf(-3, "%s: contrast_shift must lie in 0 .. 15 (got %u)", who, p->contrast_shift);
    if (wmax + (uint64_t)p->contrast_gain * (uint64_t)(65535u >> p->contrast_shift) > 0x7FFFFFFFull)
        return failf(-3, "%s: a move could cost more than 0x7FFFFFFF under the largest step weight %llu, contrast_gain %u and contrast_shift %u", who,
                     (unsigned long long)wmax, p->contrast_gain, p->contrast_shift);
    out->gw.reach = geo_reach(out->gw.w);
    out->gain = p->contrast_gain;
    out->shift = p->contrast_shift;
    return 0;
}

CallEvents g_events;                                     // around the device work of the last call of this file (svr_region_growcut_last_ms)

} // namespace

extern "C" {

int svr_region_growcut_params_default(svr_growcut_params* p, int connectivity)
{
    const char* who = "svr_region_growcut_params_default";
    if (!p) return failf(-4, "%s: null argument", who);
    if (int e = check_connectivity(who, "connectivity", connectivity)) return e;
    memset(p, 0, sizeof *p);
    for (int c = 0; c < classes_of(connectivity); ++c) p->step_weights[c] = 1u;
    p->contrast_gain = 1u;
    return 0;
}

int svr_region_growcut(const uint16_t* voxels, const int32_t dims[3], int src_is_device, const uint32_t* marker_labels_device,
                       const uint32_t* domain_mask_device_or_null, const svr_growcut_params* params, uint32_t* cost_device_or_null,
                       uint32_t* zones_device_or_null, svr_growcut_info* info_or_null)
{
    const char* who = "svr_region_growcut";
    if (!voxels || !dims || !marker_labels_device || !params) return failf(-4, "%s: null argument", who);
    if (!cost_device_or_null && !zones_device_or_null) return failf(-4, "%s: both outputs are null", who);
    if (int e = check_dims3(who, dims)) return e;
    ContrastCost cost;
    if (int e = check_params(who, params, &cost)) return e;
    const RegionDims d = make_dims(dims[0], dims[1], dims[2]);
    const size_t n = (size_t)d.nx * d.ny * d.nz;
    if (int e = check_geo_outputs(who, marker_labels_device, n * sizeof(uint32_t), domain_mask_device_or_null, mask_words(d) * sizeof(uint32_t),
                                  src_is_device ? voxels : nullptr, n * sizeof(uint16_t), cost_device_or_null, zones_device_or_null))
        return e;
    if (svr::ensure_ready()) return svr_last_error_code();
    DeviceVoxels vox;                                    // a host source is uploaded once, outside the time of the call
    SVR_HIP_TRY(vox.get(voxels, n, src_is_device, svr::current_stream()));
    GeoResult res;
    const int e = geo_run(who, g_events, cost, vox.p, marker_labels_device, domain_mask_device_or_null, d, params->max_sweeps, cost_device_or_null,
                          zones_device_or_null, &res);                                    // (synchronises: an upload is freed on return)
    if (e && e != SVR_REGION_ERR_SWEEPS) return e;
    if (info_or_null) {
        info_or_null->sweeps = res.sweeps;
        info_or_null->unreached = res.unreached;
        info_or_null->saturated = res.capped;
    }
    if (e) return e;
    if (res.capped)
        return failf(SVR_REGION_ERR_RANGE, "%s: the cost of %u voxels reached the cap 0x%X: raise contrast_shift or lower contrast_gain (the outputs hold "
                     "the saturated solution)", who, res.capped, SVR_GROWCUT_CAP);
    return 0;
}

int svr_region_seed_classes(const int32_t* seeds_xyz, const uint32_t* classes, uint32_t nseeds, const int32_t dims[3], uint32_t* labels_device)
{
    const char* who = "svr_region_seed_classes";
    if (!seeds_xyz || !classes || !dims || !labels_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, dims)) return e;
    const int nx = dims[0], ny = dims[1], nz = dims[2];
    if (int e = check_seeds(who, seeds_xyz, nseeds, nx, ny, nz)) return e;
    for (uint32_t i = 0; i < nseeds; ++i)
        if (classes[i] == 0u) return failf(-3, "%s: seed %u has class 0 (classes are non-zero)", who, i);
    return place_seeds(who, g_events, seeds_xyz, classes, nseeds, nx, ny, nz, labels_device);
}

int svr_region_label_paint(uint32_t* labels_device, const int32_t dims[3], const uint32_t* mask_device, uint32_t label, int only_unlabelled)
{
    const char* who = "svr_region_label_paint";
    if (!labels_device || !dims || !mask_device) return failf(-4, "%s: null argument", who);
    if (int e = check_dims3(who, dims)) return e;
    if (label == 0u) return failf(-3, "%s: the label must be non-zero", who);
    const RegionDims d = make_dims(dims[0], dims[1], dims[2]);
    const size_t words = mask_words(d);
    if (overlap(labels_device, (size_t)d.nx * d.ny * d.nz * sizeof(uint32_t), mask_device, words * sizeof(uint32_t)))
        return failf(-3, "%s: the labels must not overlap the mask", who);
    if (svr::ensure_ready()) return svr_last_error_code();
    hipStream_t st = svr::current_stream();
    CallTimer timer(g_events, st);
    hipLaunchKernelGGL(k_gc_paint, lane_grid(words), dim3(LANE_THREADS), 0, st, labels_device, mask_device, d, words, label, only_unlabelled);
    SVR_HIP_TRY(hipGetLastError());
    return 0;
}

int svr_region_growcut_last_ms(float* ms)
{
    if (!ms) return failf(-4, "svr_region_growcut_last_ms: null argument");
    *ms = g_events.last_ms();
    return 0;
}

} // extern "C"
