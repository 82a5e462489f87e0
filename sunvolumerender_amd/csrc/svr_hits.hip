// svr_hits.hip -- hit maps and point picks along the ray caster's rays (svr_render_hits, svr_pick; include/svr_abi.h): where the
// pixel's ray meets what the picture shows -- the sample at which the ray caster's accumulated opacity exceeds a level, the refined
// isosurface crossing that SVR_PROJ_ISO shades, or the first sample that attains the SVR_PROJ_MIP maximum -- as a 40-byte record
// (status, sample index, ray parameter, value, world position, normal).  The ray and its samples are the projection's (the pinhole
// centre ray, the clipped box interval, the float chain t_{n+1} = fl(t_n + h), h = stepSize / 2); the definition of every mode is in
// the header and is implemented here literally, float32 without contraction.
//
// One lane owns one ray, as in k_project (svr_project.hip): the map form gives a wave an 8 x 8 pixel tile, the pick form 64 entries of
// the list; persistent 256-thread blocks pull these tasks from sharded tickets.
//
// SKIPPING (all of it result-neutral).
//   ISO, MAX: the rules of svr_project.hip on Imax(m) = raw_bound(rmax(m)) from the volume's macro-cell table mm.  ISO: a sample
//          with Imax(m) < iso cannot be the first crossing.  MAX: a sample with Imax(m) <= M cannot pass the strict update I > M, so the
//          FIRST sample that attains the maximum stays the one that is recorded.  The bisection's 8 fetches and the gradient's 6 are
//          never skipped.
//   OPACITY: k_raycast's test (svr_raycast.hip).  A sample whose cell lies in an `empty` macro-cell of the (volume, transfer function)
//          mask has a_n = 0 exactly, and A + (1 - A) * 0 = A + 0 = A bit for bit (A starts at +0 and never becomes -0).
// LEAPS, as in svr_project.hip and under the same host-side condition: if the test holds for the whole neighbourhood of m (nbmax(m) for
// ISO and MAX, the mask's deep-empty bit for OPACITY), the ray advances 0.95 macro-cells along its fastest axis through the closed
// form of the float chain (svr_chain.hpp), one step short and the last step with a real addition, so that t_prev stays exact.
#include "svr_walk.hpp"
#include "svr_chain.hpp"
#include "svr_hits.hpp"

namespace svr {

#define SVR_HT_THREADS 256

namespace {

// can no fetch in macro-cell m change the ray's state?  (MAX: st = M; ISO, OPACITY: st unused)
template <int MODE>
SVR_DEV bool cell_skippable(const DevScene& s, const DevHits& hp, uint32_t m, float st)
{
    if (MODE == HIT_OPACITY) return ((hp.empty[m >> 5] >> (m & 31u)) & 1u) != 0u;
    const float imax = raw_bound(s, hp.mm[2u * m + 1u]);
    return MODE == HIT_MAX ? imax <= st : imax < hp.iso;
}
// ... nor in m or any of its neighbours?
template <int MODE>
SVR_DEV bool neighbourhood_skippable(const DevScene& s, const DevHits& hp, uint32_t m, float st)
{
    if (MODE == HIT_OPACITY) return ((hp.deep[m >> 5] >> (m & 31u)) & 1u) != 0u;
    const float imax = raw_bound(s, hp.nbmax[m]);
    return MODE == HIT_MAX ? imax <= st : imax < hp.iso;
}

} // namespace

template <int LAYOUT, int MODE, bool COUNT, bool SKIP>
__global__ __launch_bounds__(SVR_HT_THREADS) void k_hits(const DevScene s, const DevWork w, const DevHits hp, float stepSize)
{
    __shared__ LdsTileNoMask L;                                   // OPACITY: the alpha table of the transfer function
    if (MODE == HIT_OPACITY) lds_tile_load(L, s, false);
    const uint32_t lane = threadIdx.x & 63u;
    const bool pick = hp.pixels != nullptr;
    const uint32_t wv = w.x1 - w.x0;
    const uint32_t tiles_x = (wv + 7u) >> 3, tiles_y = (w.n_rows + 7u) >> 3;
    const uint32_t n_tasks = pick ? (hp.n_pick + 63u) >> 6 : tiles_x * tiles_y;
    const uint32_t per_shard = (n_tasks + TICKET_SHARDS - 1u) / TICKET_SHARDS;
    const uint32_t shard0 = blockIdx.x % TICKET_SHARDS;
    const float h = stepSize * 0.5f;
    uint32_t n_steps = 0, n_taps = 0, n_exec = 0;

    for (uint32_t si = 0; si < TICKET_SHARDS; ++si) {
        const uint32_t shard = (shard0 + si) % TICKET_SHARDS;
        const uint32_t t_begin = shard * per_shard;
        const uint32_t t_count = t_begin >= n_tasks ? 0u : min(per_shard, n_tasks - t_begin);
        uint32_t* ticket = w.ticket + shard * TICKET_STRIDE;
        for (;;) {
            uint32_t u = 0;
            if (lane == 0) u = atomicAdd(ticket, 1u);
            u = __builtin_amdgcn_readfirstlane(u);
            if (u >= t_count) break;
            const uint32_t task = t_begin + u;
            uint32_t x, y;
            size_t rec;                                           // (lane 0 always owns a pixel / an entry of its task)
            if (pick) {
                const uint32_t i = (task << 6) + lane;
                if (i >= hp.n_pick) continue;
                x = hp.pixels[2u * i]; y = hp.pixels[2u * i + 1u];
                rec = i;
            } else {
                const uint32_t ty = task / tiles_x, tx = task - ty * tiles_x;
                const uint32_t px = (tx << 3) + (lane & 7u), r = (ty << 3) + (lane >> 3);
                if (!(px < wv && r < w.n_rows)) continue;
                x = w.x0 + px; y = owned_row_to_y(w, r);
                rec = (size_t)y * s.imageW + x;
            }
            v3 orig, dir;
            camera_ray_pinhole(s, x, y, orig, dir);
            float tNear, tFar;
            uint32_t status = HIT_STATUS_MISS, sample = 0u;
            float t_hit = 0.f, I_hit = 0.f;
            v3 p = V3(0.f, 0.f, 0.f), normal = V3(0.f, 0.f, 0.f);
            if (volume_intersect(s, orig, dir, tNear, tFar)) {
                // leaps: parameter distance over which the ray moves 0.95 macro-cells along its fastest axis
                float leap_dt = 0.f;
                if (SKIP && hp.leap) {
                    const float bmax = fmax_(__builtin_fabsf(dir.x * hp.mc_scale[0]), fmax_(__builtin_fabsf(dir.y * hp.mc_scale[1]), __builtin_fabsf(dir.z * hp.mc_scale[2])));
                    if (bmax > 0.f && bmax < u2f(SVR_INF_BITS)) leap_dt = (0.95f * 0.999f) / bmax;
                }
                float t = tNear, t_prev = tNear;
                uint32_t steps = 0, fetched = 0;                  // steps = the index of the sample at t
                float M = 0.f;                                    // MAX: running maximum; OPACITY: accumulated opacity A
                bool hit = false;
                uint32_t no_leap_m = 0xffffffffu;                 // the macro-cell whose neighbourhood test failed last
                uint32_t seen_m = 0xffffffffu;                    // the macro-cell of the previous sample and its verdict
                bool seen_skip = false;
                while (t <= tFar) {
                    const Cell c = cell_of(s, orig + dir * t);
                    bool skip = false;
                    uint32_t m = 0u;
                    if (SKIP) {
                        // consecutive samples mostly share a macro-cell: its verdict is kept (the table costs a dependent load).  A kept
                        // "fetch" is always safe; a kept "skip" stays true because M only grows and iso and the mask are fixed
                        const bool inb = macro_of(s, c, m);
                        if (inb && m == seen_m) skip = seen_skip;
                        else {
                            skip = inb && cell_skippable<MODE>(s, hp, m, M);
                            seen_m = inb ? m : 0xffffffffu; seen_skip = skip;
                        }
                        if (skip && leap_dt > 0.f && m != no_leap_m) {
                            if (neighbourhood_skippable<MODE>(s, hp, m, M)) {
                                const float t_end = t + leap_dt;
                                const bool to_end = t_end > tFar;
                                bool exact, ok = false;
                                const uint32_t cnt = chain_count(t, h, to_end ? tFar : t_end, to_end, exact);
                                if (cnt >= 2u) {
                                    const float tp = chain_advance(t, h, cnt - 1u, ok);
                                    if (ok) { t_prev = tp; t = tp + h; steps += cnt; continue; }
                                }
                            } else no_leap_m = m;
                        }
                    }
                    if (!skip) {
                        fetched++;
                        const float I = tex_fetch<LAYOUT>(s, c) * s.densityScale;
                        if (MODE == HIT_MAX) {
                            if (I > M) { M = I; hit = true; sample = steps; t_hit = t; }
                        } else if (MODE == HIT_OPACITY) {
                            const float a = alpha_of(L, s, I);
                            M = M + (1.f - M) * a;
                            if (M > hp.alpha) { hit = true; sample = steps; t_hit = t; I_hit = I; steps++; break; }
                        } else if (I >= hp.iso) { hit = true; sample = steps; t_hit = t; I_hit = I; steps++; break; }
                    }
                    steps++;
                    t_prev = t;
                    t = t + h;
                }
                if (COUNT) { n_steps += steps; n_taps += steps; n_exec += fetched; }
                if (MODE == HIT_MAX) I_hit = M;

                if (MODE == HIT_ISO && hit && sample > 0u) {
                    float lo = t_prev, hi = t_hit;
#pragma unroll 1
                    for (int b = 0; b < 8; ++b) {
                        const float mid = 0.5f * (lo + hi);
                        const float Im = intensity_at<LAYOUT>(s, orig + dir * mid);
                        if (Im >= hp.iso) { hi = mid; I_hit = Im; } else lo = mid;
                    }
                    t_hit = hi;
                    if (COUNT) { n_taps += 8u; n_exec += 8u; }
                }
                status = HIT_STATUS_NONE;
                if (!hit) { sample = steps; t_hit = 0.f; I_hit = 0.f; }
                else {
                    status = HIT_STATUS_FOUND;
                    p = orig + dir * t_hit;
                    // the ray caster's gradient (svr_raycast.hip; cudaVolume::Gradient_CentralDiff, core/cuda_volume.h:54-61)
                    float xd = intensity_at<LAYOUT>(s, V3(p.x + s.spacing[0], p.y + 0.f, p.z + 0.f)) -
                               intensity_at<LAYOUT>(s, V3(p.x - s.spacing[0], p.y - 0.f, p.z - 0.f));
                    float yd = intensity_at<LAYOUT>(s, V3(p.x + 0.f, p.y + s.spacing[1], p.z + 0.f)) -
                               intensity_at<LAYOUT>(s, V3(p.x - 0.f, p.y - s.spacing[1], p.z - 0.f));
                    float zd = intensity_at<LAYOUT>(s, V3(p.x + 0.f, p.y + 0.f, p.z + s.spacing[2])) -
                               intensity_at<LAYOUT>(s, V3(p.x - 0.f, p.y - 0.f, p.z - s.spacing[2]));
                    if (COUNT) { n_taps += 6u; n_exec += 6u; }
                    const v3 gradient = V3((xd * 0.5f) * s.invSpacing[0], (yd * 0.5f) * s.invSpacing[1], (zd * 0.5f) * s.invSpacing[2]);
                    const float gm = __builtin_sqrtf(dot(gradient, gradient));
                    if ((double)gm > 1e-3) normal = normalize(gradient);
                }
            }
            uint32_t* o = hp.out + rec * HIT_WORDS;
            o[0] = status; o[1] = sample;
            o[2] = f2u(t_hit); o[3] = f2u(I_hit);
            o[4] = f2u(p.x); o[5] = f2u(p.y); o[6] = f2u(p.z);
            o[7] = f2u(normal.x); o[8] = f2u(normal.y); o[9] = f2u(normal.z);
        }
    }
    if (COUNT) {
        const unsigned long long st = wave_sum((unsigned long long)n_steps), tp = wave_sum((unsigned long long)n_taps), ex = wave_sum((unsigned long long)n_exec);
        if (lane == 0) {
            atomicAdd(&w.counters[CNT_RAYCAST], st);
            atomicAdd(&w.counters[CNT_VOL_TAPS], tp);
            atomicAdd(&w.counters[CNT_TAPS_EXEC], ex);
        }
    }
}

hipError_t launch_hits(const DevScene& s, const DevWork& w, const DevHits& hp, float stepSize, bool count, int num_cus, hipStream_t st)
{
    const bool pick = hp.pixels != nullptr;
    if (pick ? hp.n_pick == 0u : (w.x1 == w.x0 || w.n_rows == 0)) return hipSuccess;
    if (hp.mode != HIT_OPACITY && hp.mode != HIT_ISO && hp.mode != HIT_MAX) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(w.ticket, 0, sizeof(uint32_t) * TICKET_SHARDS * TICKET_STRIDE, st);
    if (e != hipSuccess) return e;
    const uint32_t n_tasks = pick ? (hp.n_pick + 63u) >> 6 : ((w.x1 - w.x0 + 7u) >> 3) * ((w.n_rows + 7u) >> 3);
    const uint32_t need = (n_tasks + SVR_HT_THREADS / 64 - 1u) / (SVR_HT_THREADS / 64);
    const uint32_t max_blocks = (uint32_t)num_cus * 8u;                  // 8 blocks of 4 waves per CU (OPACITY: 4 KB of LDS each)
    const dim3 g(persistent_blocks(need, max_blocks)), b(SVR_HT_THREADS);
    const bool skip = hp.mode == HIT_OPACITY ? hp.empty != nullptr : hp.mm != nullptr;
    with_layout(s.layout, [&](auto lay) {
        auto go = [&](auto mode) {
            with_bool(count, [&](auto cnt) {
                with_bool(skip, [&](auto sk) {
                    hipLaunchKernelGGL((k_hits<decltype(lay)::value, decltype(mode)::value, decltype(cnt)::value, decltype(sk)::value>), g, b, 0, st, s, w, hp, stepSize);
                });
            });
        };
        if (hp.mode == HIT_OPACITY) go(std::integral_constant<int, HIT_OPACITY>{});
        else if (hp.mode == HIT_ISO) go(std::integral_constant<int, HIT_ISO>{});
        else go(std::integral_constant<int, HIT_MAX>{});
    });
    return hipGetLastError();
}

} // namespace svr
