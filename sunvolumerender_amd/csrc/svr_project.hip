// svr_project.hip -- projection modes of the ray caster (svr_render_projection, include/svr_abi.h): maximum intensity,
// mean intensity and a head-light shaded isosurface.  One deterministic ray per pixel over the ray caster's samples; the
// definition of every mode is in the header and is implemented literally, float32 without contraction.
//
// One lane owns one ray (MEAN needs its sum in sample order, and nothing here is as heavy as a shaded sample of
// k_raycast); a wave is an 8 x 8 pixel tile, persistent 256-thread blocks pull tiles from sharded tickets.  The kernel is
// the ray's set-up, its march (svr_march.hpp: the rules MIP, MEAN and ISO, with their SKIPPING and LEAPS) and the colour.
#include "svr_march.hpp"
#include "svr_project.hpp"

namespace svr {

template <int LAYOUT, int MODE, bool COUNT, bool SKIP>
__global__ __launch_bounds__(SVR_VIEW_THREADS) void k_project(const DevScene s, const DevWork w, const DevProjection pj, float stepSize)
{
    constexpr int RULE = MODE == PROJ_MIP ? MARCH_MIP : MODE == PROJ_MEAN ? MARCH_MEAN : MARCH_ISO;
    const v3 cam = V3(s.cam_pos[0], s.cam_pos[1], s.cam_pos[2]);
    const float h = stepSize * 0.5f;
    const bool color_tf = (pj.flags & PROJ_COLOR_TF) != 0u;
    uint32_t n_steps = 0, n_taps = 0, n_exec = 0;

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = w.x1 - w.x0, tiles_x = (wv + 7u) >> 3;
    const uint32_t n_tasks = view_tiles(w);
    const uint32_t per_shard = (n_tasks + TICKET_SHARDS - 1u) / TICKET_SHARDS;
    const uint32_t shard0 = blockIdx.x % TICKET_SHARDS;
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
            const uint32_t ty = task / tiles_x, tx = task - ty * tiles_x;
            const uint32_t px = (tx << 3) + (lane & 7u), row = (ty << 3) + (lane >> 3);
            if (!(px < wv && row < w.n_rows)) continue;               // (lane 0 always owns a pixel of its tile)
            const uint32_t x = w.x0 + px, y = owned_row_to_y(w, row);
            v3 orig, dir;
            camera_ray_pinhole(s, x, y, orig, dir);
            float tNear, tFar;
            uint32_t rgba = 0u;                                       // a miss, or no crossing: (0, 0, 0, 0)
            if (volume_intersect(s, orig, dir, tNear, tFar)) {
                const March r = march_ray<LAYOUT, RULE, SKIP>(s, NoLds{}, pj.tb, pj.iso, orig, dir, tNear, tFar, h);
                if (COUNT) { n_steps += r.steps; n_taps += r.steps; n_exec += r.fetched; }
                if (MODE == PROJ_ISO) {
                    if (r.hit) {
                        Crossing surf = {r.t_hit, r.I_hit};
                        if (r.steps > 1u) {                            // (the first sample has nothing before it to bisect)
                            surf = refine_crossing<LAYOUT>(s, orig, dir, pj.iso, r.t_prev, r.t_hit, r.I_hit);
                            if (COUNT) { n_taps += 8u; n_exec += 8u; }
                        }
                        const v3 p = orig + dir * surf.t;
                        float co[4] = {1.f, 1.f, 1.f, 1.f};
                        if (color_tf) { tf_rgba(s, s.tf, surf.I, co); co[3] = 1.f; }
                        // the ray caster's head-light term (svr_raycast.hip)
                        const v3 gradient = central_gradient<LAYOUT>(s, p);
                        if (COUNT) { n_taps += 6u; n_exec += 6u; }
                        float gm = __builtin_sqrtf(dot(gradient, gradient));
                        float cosTerm = 1.f, specularTerm = 0.f;
                        if ((double)gm > 1e-3) {
                            v3 normal = normalize(gradient);
                            v3 lightDir = normalize(cam - p);
                            cosTerm = __builtin_fabsf(dot(normal, lightDir));
                            specularTerm = powf_(cosTerm, 30.f);
                        }
                        co[0] = co[0] * co[3] * cosTerm * 0.8f + co[3] * specularTerm * 0.2f;
                        co[1] = co[1] * co[3] * cosTerm * 0.8f + co[3] * specularTerm * 0.2f;
                        co[2] = co[2] * co[3] * cosTerm * 0.8f + co[3] * specularTerm * 0.2f;
                        const float cr = fmin_(co[0], 1.f), cg = fmin_(co[1], 1.f), cb = fmin_(co[2], 1.f);
                        rgba = to_u8(cr * 255) | (to_u8(cg * 255) << 8) | (to_u8(cb * 255) << 16) | (255u << 24);
                    }
                } else {
                    float M = r.M;
                    if (MODE == PROJ_MEAN) M = M / (float)r.steps;
                    float cr, cg, cb;
                    if (color_tf) {
                        float co[4];
                        tf_rgba(s, s.tf, M, co);
                        cr = fmin_(fmax_(co[0], 0.f), 1.f); cg = fmin_(fmax_(co[1], 0.f), 1.f); cb = fmin_(fmax_(co[2], 0.f), 1.f);
                    } else {
                        const float g = fmin_(fmax_((M - pj.window_lo) / (pj.window_hi - pj.window_lo), 0.f), 1.f);
                        cr = g; cg = g; cb = g;
                    }
                    rgba = to_u8(cr * 255) | (to_u8(cg * 255) << 8) | (to_u8(cb * 255) << 16) | (255u << 24);
                }
            }
            reinterpret_cast<uint32_t*>(w.img)[(size_t)y * s.imageW + x] = rgba;
        }
    }
    if (COUNT) view_counters_flush(w, n_steps, n_taps, n_exec);
}

// nb(m) = the largest rmax over macro-cell m and its in-grid neighbours
__global__ __launch_bounds__(256) void k_nbmax(const uint16_t* __restrict__ mm, uint16_t* __restrict__ nb, int gx, int gy, int gz)
{
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;
    if (m >= (uint32_t)gx * (uint32_t)gy * (uint32_t)gz) return;
    const int mx = (int)(m % (uint32_t)gx), my = (int)((m / (uint32_t)gx) % (uint32_t)gy), mz = (int)(m / ((uint32_t)gx * (uint32_t)gy));
    uint32_t hi = 0u;
    for (int z = max(mz - 1, 0); z <= min(mz + 1, gz - 1); ++z)
        for (int y = max(my - 1, 0); y <= min(my + 1, gy - 1); ++y)
            for (int x = max(mx - 1, 0); x <= min(mx + 1, gx - 1); ++x)
                hi = max(hi, (uint32_t)mm[2u * ((uint32_t)x + (uint32_t)gx * ((uint32_t)y + (uint32_t)gy * (uint32_t)z)) + 1u]);
    nb[m] = (uint16_t)hi;
}

hipError_t launch_nbmax(const uint16_t* mm, uint16_t* nbmax, int gx, int gy, int gz, hipStream_t st)
{
    const uint32_t n = (uint32_t)gx * (uint32_t)gy * (uint32_t)gz;
    hipLaunchKernelGGL(k_nbmax, dim3((n + 255u) / 256u), dim3(256), 0, st, mm, nbmax, gx, gy, gz);
    return hipGetLastError();
}

hipError_t launch_projection(const DevScene& s, const DevWork& w, const DevProjection& pj, float stepSize, bool count, int num_cus, hipStream_t st)
{
    if (w.x1 == w.x0 || w.n_rows == 0) return hipSuccess;
    if (pj.mode != PROJ_MIP && pj.mode != PROJ_MEAN && pj.mode != PROJ_ISO) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(w.ticket, 0, sizeof(uint32_t) * TICKET_SHARDS * TICKET_STRIDE, st);
    if (e != hipSuccess) return e;
    const dim3 g(view_blocks(view_tiles(w), num_cus)), b(SVR_VIEW_THREADS);                  // no LDS
    const bool skip = pj.tb.mm != nullptr;
    with_layout(s.layout, [&](auto lay) {
        auto go = [&](auto mode) {
            with_bool(count, [&](auto cnt) {
                with_bool(skip, [&](auto sk) {
                    hipLaunchKernelGGL((k_project<decltype(lay)::value, decltype(mode)::value, decltype(cnt)::value, decltype(sk)::value>), g, b, 0, st, s, w, pj, stepSize);
                });
            });
        };
        if (pj.mode == PROJ_MIP) go(std::integral_constant<int, PROJ_MIP>{});
        else if (pj.mode == PROJ_MEAN) go(std::integral_constant<int, PROJ_MEAN>{});
        else go(std::integral_constant<int, PROJ_ISO>{});
    });
    return hipGetLastError();
}

} // namespace svr
