// svr_march.hpp -- the march of ONE lane along ONE ray over the ray caster's samples (the pinhole centre ray, the clipped box interval, the
// float chain t_{n+1} = fl(t_n + h), h = stepSize / 2), shared by k_project (svr_project.hip) and k_hits (svr_hits.hip), with the two
// things both do at an isosurface crossing: the bisection and the central-difference gradient.  A hit record is the picture only while
// both kernels walk the same samples and skip by the same rules, so the loop exists here and nowhere else.  (k_raycast, svr_raycast.hip,
// spreads a ray over several lanes and keeps its own form.)
//
// RULES: what a fetched intensity I does to the ray's state M, each the literal expression of include/svr_abi.h, float32 without contraction.
//   MIP        M = max(M, I)                                        (SVR_PROJ_MIP)
//   MEAN       M = M + I, in sample order                           (SVR_PROJ_MEAN)
//   ISO        the first sample with I >= level ends the march      (SVR_PROJ_ISO, SVR_HIT_ISO)
//   FIRST_MAX  I > M, strictly: M = I, and the sample is recorded   (SVR_HIT_MAX: the FIRST sample that attains the MIP value)
//   OPACITY    M = M + (1 - M) * alpha(I); M > level ends the march (SVR_HIT_OPACITY: k_raycast's accumulated opacity)
// MIP and FIRST_MAX are two expressions on purpose: they differ on -0.
//
// SKIPPING (all of it result-neutral).  Every intensity a fetch in macro-cell m can return is I <= Imax(m) = raw_bound(rmax(m)), with rmax(m)
// from the volume's macro-cell table mm and the macro-cell from the sampler's own cell (svr_walk.hpp, macro_of and raw_bound, where the
// argument stands), so the per-sample test needs no margin.
//   MIP, FIRST_MAX: a sample with Imax(m) <= M leaves max(M, I) as it is and cannot pass the strict I > M: not fetched.
//   ISO:       a sample with Imax(m) < level cannot be the first crossing: not fetched.  The bisection's 8 fetches and the gradient's 6
//              are never skipped.
//   MEAN:      rmax(m) == 0: all eight voxels are 0, every lerp is fma(t, 0, 0) = +0, the product with the two non-negative factors is +0
//              (or -0 under densityScale = -0), and S + (+-0) = S bit for bit (S starts at +0 and never becomes -0).  The sample still
//              counts in N.
//   OPACITY:   k_raycast's test.  A sample whose cell lies in an `empty` macro-cell of the (volume, transfer function) mask has alpha = 0
//              exactly, and A + (1 - A) * 0 = A + 0 = A bit for bit (A starts at +0 and never becomes -0).
// Consecutive samples mostly share a macro-cell, so its verdict is kept (the table costs a dependent load).  A kept "fetch" is always
// safe; a kept "skip" stays true because M only grows and the level and the tables are fixed.
//
// LEAPS.  nbmax(m) = the largest rmax over m and its in-grid neighbours (k_nbmax, built once per volume texture); for OPACITY the mask's
// deep-empty bit says the same of `empty`.  If the test above holds for the neighbourhood, every sample whose cell lies in m or one of
// its 26 neighbours is skippable.  From a sample in m the ray may advance until its largest-axis displacement is 0.95 macro-cells: every
// point before that lies in m or a neighbour (the host only allows leaps when the float error of p = orig + dir * t, in macro-cells, is
// below 0.02 and the clipped box lies inside the texture domain, so that every sample maps into the grid).  The samples before that
// parameter are counted with the closed form of the float chain (svr_chain.hpp, chain_count) and passed with chain_advance, which replay
// t += h exactly; wherever the closed form gives up (t < 1, a tie, a binade the form does not cover) the ray takes single steps.  ISO
// needs the chain element BEFORE the one a leap lands on (the bisection's lower end): a leap of k steps advances k - 1 in closed form and
// takes the last step with a real addition, so that t_prev stays exact.
#pragma once
#include "svr_walk.hpp"
#include "svr_chain.hpp"

namespace svr {

enum { MARCH_MIP, MARCH_MEAN, MARCH_ISO, MARCH_FIRST_MAX, MARCH_OPACITY };

struct NoLds {};                   // what a march that is not OPACITY passes for the alpha table

struct March {
    float t_prev;                  // the chain element before the last sample visited (the bisection's lower end)
    float M;                       // MIP, FIRST_MAX: the maximum; MEAN: the sum; OPACITY: the accumulated opacity
    float I_hit, t_hit;            // ISO, OPACITY: value and parameter of the sample that ended the march; FIRST_MAX: t of the recorded sample
    uint32_t steps, fetched;       // samples visited (the ending one included), and those of them that were fetched
    uint32_t sample;               // index of the recorded sample
    bool hit;                      // a sample ended the march (ISO, OPACITY) or was recorded (FIRST_MAX)
};

// can no fetch in macro-cell m -- nb: nor in any of its neighbours -- change the ray's state M?
template <int RULE>
SVR_DEV bool march_skippable(const DevScene& s, const MarchTables& tb, uint32_t m, float M, float level, bool nb)
{
    if (RULE == MARCH_OPACITY) return (((nb ? tb.deep : tb.empty)[m >> 5] >> (m & 31u)) & 1u) != 0u;
    const uint32_t r = nb ? tb.nbmax[m] : tb.mm[2u * m + 1u];
    if (RULE == MARCH_MEAN) return r == 0u;
    const float imax = raw_bound(s, r);
    return RULE == MARCH_ISO ? imax < level : imax <= M;
}

// level: the iso value (ISO) or the opacity to exceed (OPACITY); L: the block's alpha table (OPACITY), else NoLds
template <int LAYOUT, int RULE, bool SKIP, typename LDS>
SVR_DEV March march_ray(const DevScene& s, const LDS& L, const MarchTables& tb, float level, v3 orig, v3 dir, float tNear, float tFar, float h)
{
    // leaps: parameter distance over which the ray moves 0.95 macro-cells along its fastest axis
    float leap_dt = 0.f;
    if (SKIP && tb.leap) {
        const float bmax = fmax_(__builtin_fabsf(dir.x * tb.mc_scale[0]), fmax_(__builtin_fabsf(dir.y * tb.mc_scale[1]), __builtin_fabsf(dir.z * tb.mc_scale[2])));
        if (bmax > 0.f && bmax < u2f(SVR_INF_BITS)) leap_dt = (0.95f * 0.999f) / bmax;
    }
    March r;
    r.t_prev = tNear; r.M = 0.f; r.I_hit = 0.f; r.t_hit = 0.f;
    r.steps = 0u; r.fetched = 0u; r.sample = 0u; r.hit = false;
    float t = tNear;                                      // steps = the index of the sample at t
    uint32_t no_leap_m = 0xffffffffu;                     // the macro-cell whose neighbourhood test failed last
    uint32_t seen_m = 0xffffffffu;                        // the macro-cell of the previous sample and its verdict
    bool seen_skip = false;
    while (t <= tFar) {
        const Cell c = cell_of(s, orig + dir * t);
        bool skip = false;
        uint32_t m = 0u;
        if (SKIP) {
            const bool inb = macro_of(s, c, m);
            if (inb && m == seen_m) skip = seen_skip;
            else {
                skip = inb && march_skippable<RULE>(s, tb, m, r.M, level, false);
                seen_m = inb ? m : 0xffffffffu; seen_skip = skip;
            }
            if (skip && leap_dt > 0.f && m != no_leap_m) {
                if (march_skippable<RULE>(s, tb, m, r.M, level, true)) {
                    const float t_end = t + leap_dt;
                    const bool to_end = t_end > tFar;
                    bool exact, ok = false;
                    const uint32_t cnt = chain_count(t, h, to_end ? tFar : t_end, to_end, exact);
                    if (cnt >= 2u) {
                        const float tp = chain_advance(t, h, cnt - 1u, ok);
                        if (ok) { r.t_prev = tp; t = tp + h; r.steps += cnt; continue; }
                    }
                } else no_leap_m = m;
            }
        }
        if (!skip) {
            r.fetched++;
            const float I = tex_fetch<LAYOUT>(s, c) * s.densityScale;
            bool stop = false;
            if (RULE == MARCH_MIP) r.M = fmax_(r.M, I);
            else if (RULE == MARCH_MEAN) r.M = r.M + I;
            else if (RULE == MARCH_FIRST_MAX) {
                if (I > r.M) { r.M = I; r.hit = true; r.sample = r.steps; r.t_hit = t; }
            } else if constexpr (RULE == MARCH_OPACITY) {
                const float a = alpha_of(L, s, I);
                r.M = r.M + (1.f - r.M) * a;
                stop = r.M > level;
            } else stop = I >= level;
            if (stop) { r.hit = true; r.sample = r.steps; r.t_hit = t; r.I_hit = I; r.steps++; break; }
        }
        r.steps++;
        r.t_prev = t;
        t = t + h;
    }
    return r;
}

// The crossing between a sample below the level (at lo) and the first one at or above it (at hi, value I_hi): 8 bisections, always fetched.
struct Crossing { float t, I; };
template <int LAYOUT>
SVR_DEV Crossing refine_crossing(const DevScene& s, v3 orig, v3 dir, float level, float lo, float hi, float I_hi)
{
#pragma unroll 1
    for (int b = 0; b < 8; ++b) {
        const float mid = 0.5f * (lo + hi);
        const float Im = intensity_at<LAYOUT>(s, orig + dir * mid);
        if (Im >= level) { hi = mid; I_hi = Im; } else lo = mid;
    }
    return {hi, I_hi};
}

// the ray caster's gradient (svr_raycast.hip; cudaVolume::Gradient_CentralDiff, core/cuda_volume.h:54-61): six taps, always fetched
template <int LAYOUT>
SVR_DEV v3 central_gradient(const DevScene& s, v3 p)
{
    float xd = intensity_at<LAYOUT>(s, V3(p.x + s.spacing[0], p.y + 0.f, p.z + 0.f)) -
               intensity_at<LAYOUT>(s, V3(p.x - s.spacing[0], p.y - 0.f, p.z - 0.f));
    float yd = intensity_at<LAYOUT>(s, V3(p.x + 0.f, p.y + s.spacing[1], p.z + 0.f)) -
               intensity_at<LAYOUT>(s, V3(p.x - 0.f, p.y - s.spacing[1], p.z - 0.f));
    float zd = intensity_at<LAYOUT>(s, V3(p.x + 0.f, p.y + 0.f, p.z + s.spacing[2])) -
               intensity_at<LAYOUT>(s, V3(p.x - 0.f, p.y - 0.f, p.z - s.spacing[2]));
    return V3((xd * 0.5f) * s.invSpacing[0], (yd * 0.5f) * s.invSpacing[1], (zd * 0.5f) * s.invSpacing[2]);
}

} // namespace svr
