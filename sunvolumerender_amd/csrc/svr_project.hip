// svr_project.hip -- projection modes of the ray caster (svr_render_projection, include/svr_abi.h): maximum intensity,
// mean intensity and a head-light shaded isosurface.  One deterministic ray per pixel over the ray caster's samples
// (the pinhole centre ray, the clipped box interval, the float chain t_{n+1} = fl(t_n + h), h = stepSize / 2); the
// definition of every mode is in the header and is implemented here literally, float32 without contraction.
//
// One lane owns one ray (MEAN needs its sum in sample order, and nothing here is as heavy as a shaded sample of
// k_raycast); a wave is an 8 x 8 pixel tile, persistent 256-thread blocks pull tiles from sharded tickets.
//
// SKIPPING (all of it result-neutral).  Every intensity a fetch in macro-cell m can return is I <= Imax(m) = raw_bound(rmax(m)),
// with rmax(m) from the volume's macro-cell table mm and the macro-cell from the sampler's own cell (svr_walk.hpp, macro_of and
// raw_bound, where the argument stands), so the per-sample test needs no margin.
//   MIP:   a sample with Imax(m) <= M leaves M = max(M, I) as it is: not fetched.
//   ISO:   a sample with Imax(m) <  iso cannot be the first crossing I >= iso: not fetched.  The 8 bisection fetches,
//          the gradient's 6 and nothing else of the surface point are ever skipped.
//   MEAN:  rmax(m) == 0: all eight voxels are 0, every lerp is fma(t, 0, 0) = +0, the product with the two
//          non-negative factors is +0 (or -0 under densityScale = -0), and S + (+-0) = S bit for bit (S starts at +0 and
//          never becomes -0).  The sample still counts in N.
// LEAPS.  nb(m) = the largest rmax over m and its in-grid neighbours (k_nbmax, built once per volume texture).  If the
// test above holds for nb(m), every sample whose cell lies in m or one of its 26 neighbours is skippable.  From a
// sample in m the ray may advance until its largest-axis displacement is 0.95 macro-cells: every point before that lies
// in m or a neighbour (the host only allows leaps when the float error of p = orig + dir * t, in macro-cells, is below
// 0.02 and the clipped box lies inside the texture domain, so that every sample maps into the grid).  The samples
// before that parameter are counted with the closed form of the float chain (svr_chain.hpp, chain_count) and passed with
// chain_advance, which replay t += h exactly; wherever the closed form gives up (t < 1, a tie, a binade the form does
// not cover) the ray takes single steps.  ISO needs the chain element BEFORE the one a leap lands on (the bisection's
// lower end): a leap of k steps advances k - 1 in closed form and takes the last step with a real addition.
#include "svr_walk.hpp"
#include "svr_chain.hpp"
#include "svr_project.hpp"

namespace svr {

#define SVR_PJ_THREADS 256

namespace {

// can no fetch whose raw values are <= r change the ray's state?  (MIP: st = M; ISO: st = iso; MEAN: unused)
template <int MODE>
SVR_DEV bool skippable(const DevScene& s, uint32_t r, float st)
{
    if (MODE == PROJ_MEAN) return r == 0u;
    const float imax = raw_bound(s, r);
    return MODE == PROJ_MIP ? imax <= st : imax < st;
}

} // namespace

template <int LAYOUT, int MODE, bool COUNT, bool SKIP>
__global__ __launch_bounds__(SVR_PJ_THREADS) void k_project(const DevScene s, const DevWork w, const DevProjection pj, float stepSize)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = w.x1 - w.x0;
    const uint32_t tiles_x = (wv + 7u) >> 3, tiles_y = (w.n_rows + 7u) >> 3;
    const uint32_t n_tasks = tiles_x * tiles_y;
    const uint32_t per_shard = (n_tasks + TICKET_SHARDS - 1u) / TICKET_SHARDS;
    const uint32_t shard0 = blockIdx.x % TICKET_SHARDS;
    const v3 cam = V3(s.cam_pos[0], s.cam_pos[1], s.cam_pos[2]);
    const float h = stepSize * 0.5f;
    const bool color_tf = (pj.flags & PROJ_COLOR_TF) != 0u;
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
            const uint32_t ty = task / tiles_x, tx = task - ty * tiles_x;
            const uint32_t px = (tx << 3) + (lane & 7u), r = (ty << 3) + (lane >> 3);
            if (!(px < wv && r < w.n_rows)) continue;                 // (lane 0 always owns a pixel of its tile)
            const uint32_t x = w.x0 + px, y = owned_row_to_y(w, r);
            v3 orig, dir;
            camera_ray_pinhole(s, x, y, orig, dir);
            float tNear, tFar;
            uint32_t rgba = 0u;                                   // a miss, or no crossing: (0, 0, 0, 0)
            if (volume_intersect(s, orig, dir, tNear, tFar)) {
                // leaps: parameter distance over which the ray moves 0.95 macro-cells along its fastest axis
                float leap_dt = 0.f;
                if (SKIP && pj.leap) {
                    const float bmax = fmax_(__builtin_fabsf(dir.x * pj.mc_scale[0]), fmax_(__builtin_fabsf(dir.y * pj.mc_scale[1]), __builtin_fabsf(dir.z * pj.mc_scale[2])));
                    if (bmax > 0.f && bmax < u2f(SVR_INF_BITS)) leap_dt = (0.95f * 0.999f) / bmax;
                }
                float t = tNear, t_prev = tNear;
                uint32_t steps = 0, fetched = 0;
                float M = 0.f;                                    // MIP: running maximum; MEAN: running sum
                float I_hit = 0.f;
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
                        // "fetch" is always safe; a kept "skip" stays true because M only grows and iso is fixed
                        const bool inb = macro_of(s, c, m);
                        if (inb && m == seen_m) skip = seen_skip;
                        else {
                            skip = inb && skippable<MODE>(s, pj.mm[2u * m + 1u], MODE == PROJ_ISO ? pj.iso : M);
                            seen_m = inb ? m : 0xffffffffu; seen_skip = skip;
                        }
                        if (skip && leap_dt > 0.f && m != no_leap_m) {
                            if (skippable<MODE>(s, pj.nbmax[m], MODE == PROJ_ISO ? pj.iso : M)) {
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
                        if (MODE == PROJ_MIP) M = fmax_(M, I);
                        else if (MODE == PROJ_MEAN) M = M + I;
                        else if (I >= pj.iso) { hit = true; I_hit = I; steps++; break; }
                    }
                    steps++;
                    t_prev = t;
                    t = t + h;
                }
                if (COUNT) { n_steps += steps; n_taps += steps; n_exec += fetched; }

                if (MODE == PROJ_ISO) {
                    if (hit) {
                        float hi = t, I_hi = I_hit;
                        if (steps > 1u) {
                            float lo = t_prev;
#pragma unroll 1
                            for (int b = 0; b < 8; ++b) {
                                const float mid = 0.5f * (lo + hi);
                                const float Im = intensity_at<LAYOUT>(s, orig + dir * mid);
                                if (Im >= pj.iso) { hi = mid; I_hi = Im; } else lo = mid;
                            }
                            if (COUNT) { n_taps += 8u; n_exec += 8u; }
                        }
                        const v3 p = orig + dir * hi;
                        float co[4] = {1.f, 1.f, 1.f, 1.f};
                        if (color_tf) { tf_rgba(s, s.tf, I_hi, co); co[3] = 1.f; }
                        // the ray caster's head-light term (svr_raycast.hip; cudaVolume::Gradient_CentralDiff, core/cuda_volume.h:54-61)
                        float xd = intensity_at<LAYOUT>(s, V3(p.x + s.spacing[0], p.y + 0.f, p.z + 0.f)) -
                                   intensity_at<LAYOUT>(s, V3(p.x - s.spacing[0], p.y - 0.f, p.z - 0.f));
                        float yd = intensity_at<LAYOUT>(s, V3(p.x + 0.f, p.y + s.spacing[1], p.z + 0.f)) -
                                   intensity_at<LAYOUT>(s, V3(p.x - 0.f, p.y - s.spacing[1], p.z - 0.f));
                        float zd = intensity_at<LAYOUT>(s, V3(p.x + 0.f, p.y + 0.f, p.z + s.spacing[2])) -
                                   intensity_at<LAYOUT>(s, V3(p.x - 0.f, p.y - 0.f, p.z - s.spacing[2]));
                        if (COUNT) { n_taps += 6u; n_exec += 6u; }
                        v3 gradient = V3((xd * 0.5f) * s.invSpacing[0], (yd * 0.5f) * s.invSpacing[1], (zd * 0.5f) * s.invSpacing[2]);
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
                    if (MODE == PROJ_MEAN) M = M / (float)steps;
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
    if (COUNT) {
        const unsigned long long st = wave_sum((unsigned long long)n_steps), tp = wave_sum((unsigned long long)n_taps), ex = wave_sum((unsigned long long)n_exec);
        if (lane == 0) {
            atomicAdd(&w.counters[CNT_RAYCAST], st);
            atomicAdd(&w.counters[CNT_VOL_TAPS], tp);
            atomicAdd(&w.counters[CNT_TAPS_EXEC], ex);
        }
    }
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
    const uint32_t n_tasks = ((w.x1 - w.x0 + 7u) >> 3) * ((w.n_rows + 7u) >> 3);
    const uint32_t need = (n_tasks + SVR_PJ_THREADS / 64 - 1u) / (SVR_PJ_THREADS / 64);
    const uint32_t max_blocks = (uint32_t)num_cus * 8u;                  // 8 blocks of 4 waves per CU, no LDS
    const dim3 g(persistent_blocks(need, max_blocks)), b(SVR_PJ_THREADS);
    const bool skip = pj.mm != nullptr;
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
