// svr_path.hpp -- the arithmetic of a path's three events (kernel_pathtracer's loop, pathtracer.cu:216-277), once: the light seen by the
// camera ray, the direct light through a shadow walk, the throughput after bsdf_sample.  The bit-exact contract fixes
// the operation ORDER of these expressions.  Used by svr_kernels.hip, svr_wavefront.hip, svr_trace_env.hip and the BSDF stage of
// svr_trace_lm.hip; the tile kernel and its queue machines (svr_trace_tile.hip, svr_primary.hpp, svr_lanes.hpp) and the walk pools of
// svr_trace_lm.hip keep their own copies of the same expressions: every adoption tried there cost registers or stack in some build.
#pragma once
#include "svr_device.hpp"

namespace svr {

SVR_DEV v3 light_radiance(const DevLight& l) { return V3(l.radiance[0], l.radiance[1], l.radiance[2]); }

// a light seen by the camera ray `dir` (pathtracer.cu:220-229): its radiance if it faces the ray, else nothing,
// ... added to the path's radiance: L + (T x radiance) x gate
SVR_DEV v3 light_seen(v3 L, v3 T, const DevLight& l, v3 dir)
{
    const float cosTerm = dot(V3(l.normal[0], l.normal[1], l.normal[2]), -dir);
    return L + (T * light_radiance(l)) * (cosTerm <= 0.f ? 0.f : 1.f);
}

// transmittance.h:15-16 on a shadow walk's result ts (the collision's ray parameter, or -FLT_MAX) and the ray's box interval: binary
SVR_DEV float shadow_transmittance(float ts, float sMin, float sMax) { return ((ts > sMin) && (ts < sMax)) ? 0.f : 1.f; }

// estimate_direct_light's tail (pathtracer.cu:191-198): Ld of the sampled light (Li = its radiance: sample_light returned true, so the
// light faces the event) with the BSDF value B and the light sample's pdf; the path adds T x Ld
SVR_DEV v3 direct_light_tr(float Tr, uint32_t num_lights, v3 Li, v3 B, float pdf)
{
    const float kf = Tr * (float)num_lights;
    return ((B * kf) * Li) / pdf;
}
SVR_DEV v3 direct_light(float ts, float sMin, float sMax, uint32_t num_lights, v3 Li, v3 B, float pdf)
{
    return direct_light_tr(shadow_transmittance(ts, sMin, sMax), num_lights, Li, B, pdf);
}

// the throughput after bsdf_sample returned f, wi, pdf (pathtracer.cu:260-270): phase function (st = 0) or BRDF with its cosine
SVR_DEV v3 bsdf_throughput(v3 T, const Shade& vs, v3 f, v3 wi, float pdf)
{
    const float cosTerm = __builtin_fabsf(dot(normalize(vs.gradient), wi));
    if (fmax_(f.x, fmax_(f.y, f.z)) > 0.f && pdf > 0.f) {
        if (vs.st == 0) T = T * (f / (pdf * (1.f - vs.Pbrdf)));
        else T = T * ((f * cosTerm) / (pdf * vs.Pbrdf));
    }
    return T;
}

} // namespace svr
