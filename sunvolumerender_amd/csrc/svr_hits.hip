// svr_hits.hip -- hit maps and point picks along the ray caster's rays (svr_render_hits, svr_pick; include/svr_abi.h): where the
// pixel's ray meets what the picture shows -- the sample at which the ray caster's accumulated opacity exceeds a level, the refined
// isosurface crossing that SVR_PROJ_ISO shades, or the first sample that attains the SVR_PROJ_MIP maximum -- as a 40-byte record
// (status, sample index, ray parameter, value, world position, normal).  The ray and its samples are the projection's (the pinhole
// centre ray, the clipped box interval, the float chain t_{n+1} = fl(t_n + h), h = stepSize / 2); the definition of every mode is in
// the header and is implemented here literally, float32 without contraction.
//
// One lane owns one ray, as in k_project (svr_project.hip): the map form gives a wave an 8 x 8 pixel tile, the pick form 64 entries of
// the list; persistent 256-thread blocks pull these tasks from sharded tickets.  The kernel is the ray's set-up, its march
// (svr_march.hpp: the rules OPACITY, ISO and FIRST_MAX, with their SKIPPING and LEAPS -- the very loop, bisection and gradient that
// k_project runs) and the record.
#include "svr_march.hpp"
#include "svr_hits.hpp"

namespace svr {

template <int LAYOUT, int MODE, bool COUNT, bool SKIP>
__global__ __launch_bounds__(SVR_VIEW_THREADS) void k_hits(const DevScene s, const DevWork w, const DevHits hp, float stepSize)
{
    constexpr int RULE = MODE == HIT_OPACITY ? MARCH_OPACITY : MODE == HIT_ISO ? MARCH_ISO : MARCH_FIRST_MAX;
    __shared__ LdsTileNoMask L;                                   // OPACITY: the alpha table of the transfer function
    if (MODE == HIT_OPACITY) lds_tile_load(L, s, false);
    const uint32_t lane = threadIdx.x & 63u;
    const bool pick = hp.pixels != nullptr;
    const uint32_t wv = w.x1 - w.x0, tiles_x = (wv + 7u) >> 3;
    const uint32_t n_tasks = pick ? (hp.n_pick + 63u) >> 6 : view_tiles(w);
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
                const uint32_t px = (tx << 3) + (lane & 7u), row = (ty << 3) + (lane >> 3);
                if (!(px < wv && row < w.n_rows)) continue;
                x = w.x0 + px; y = owned_row_to_y(w, row);
                rec = (size_t)y * s.imageW + x;
            }
            v3 orig, dir;
            camera_ray_pinhole(s, x, y, orig, dir);
            float tNear, tFar;
            uint32_t status = HIT_STATUS_MISS, sample = 0u;
            float t_hit = 0.f, I_hit = 0.f;
            v3 p = V3(0.f, 0.f, 0.f), normal = V3(0.f, 0.f, 0.f);
            if (volume_intersect(s, orig, dir, tNear, tFar)) {
                const March r = march_ray<LAYOUT, RULE, SKIP>(s, L, hp.tb, MODE == HIT_OPACITY ? hp.alpha : hp.iso, orig, dir, tNear, tFar, h);
                if (COUNT) { n_steps += r.steps; n_taps += r.steps; n_exec += r.fetched; }
                status = HIT_STATUS_NONE;
                sample = r.steps;
                if (r.hit) {
                    status = HIT_STATUS_FOUND;
                    sample = r.sample; t_hit = r.t_hit; I_hit = MODE == HIT_MAX ? r.M : r.I_hit;
                    if (MODE == HIT_ISO && r.sample > 0u) {
                        const Crossing surf = refine_crossing<LAYOUT>(s, orig, dir, hp.iso, r.t_prev, r.t_hit, r.I_hit);
                        t_hit = surf.t; I_hit = surf.I;
                        if (COUNT) { n_taps += 8u; n_exec += 8u; }
                    }
                    p = orig + dir * t_hit;
                    const v3 gradient = central_gradient<LAYOUT>(s, p);
                    if (COUNT) { n_taps += 6u; n_exec += 6u; }
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
    if (COUNT) view_counters_flush(w, n_steps, n_taps, n_exec);
}

hipError_t launch_hits(const DevScene& s, const DevWork& w, const DevHits& hp, float stepSize, bool count, int num_cus, hipStream_t st)
{
    const bool pick = hp.pixels != nullptr;
    if (pick ? hp.n_pick == 0u : (w.x1 == w.x0 || w.n_rows == 0)) return hipSuccess;
    if (hp.mode != HIT_OPACITY && hp.mode != HIT_ISO && hp.mode != HIT_MAX) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(w.ticket, 0, sizeof(uint32_t) * TICKET_SHARDS * TICKET_STRIDE, st);
    if (e != hipSuccess) return e;
    const dim3 g(view_blocks(pick ? (hp.n_pick + 63u) >> 6 : view_tiles(w), num_cus)), b(SVR_VIEW_THREADS);      // (OPACITY: 4 KB of LDS per block)
    const bool skip = hp.mode == HIT_OPACITY ? hp.tb.empty != nullptr : hp.tb.mm != nullptr;
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
