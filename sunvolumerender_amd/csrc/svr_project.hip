// svr_project.hip -- projection modes of the ray caster (svr_render_projection, include/svr_abi.h): maximum intensity,
// mean intensity and a head-light shaded isosurface.  One deterministic ray per pixel over the ray caster's samples
// (the pinhole centre ray, the clipped box interval, the float chain t_{n+1} = fl(t_n + h), h = stepSize / 2); the
// definition of every mode is in the header and is implemented here literally, float32 without contraction.
//
// One lane owns one ray (MEAN needs its sum in sample order, and nothing here is as heavy as a shaded sample of
// k_raycast); a wave is an 8 x 8 pixel tile, persistent 256-thread blocks pull tiles from sharded tickets.
//
// SKIPPING (all of it result-neutral).  The volume's macro-cell table mm (svr_accel.hip, k_minmax) holds the smallest
// and largest raw voxel rmin(m), rmax(m) over the footprint of every trilinear cell of macro-cell m.  A fetch is seven
// lerps fma(t, q - p, p), t in [0, 1), each of which rounds monotonically and stays within [min(p, q), max(p, q)], so
// the filtered raw value lies in [rmin, rmax]; the sampler's two multiplies (x 1/65535, x densityScale, the latter
// checked non-negative and finite on the host) are monotone, so every intensity a fetch in m can return is
//     I <= Imax(m) = ((float)rmax(m) * 1/65535) * densityScale                       (k_empty_mask's argument).
// The macro-cell of a sample is taken from the sampler's own trilinear cell (cell_of), as k_raycast's `empty` test
// does, so the per-sample test needs no margin.  Cells outside the grid (clip planes beyond the volume) always fetch.
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
// before that parameter are counted with the closed form of the float chain (chain_count) and passed with
// chain_advance, which replay t += h exactly; wherever the closed form gives up (t < 1, a tie, a binade the form does
// not cover) the ray takes single steps.  ISO needs the chain element BEFORE the one a leap lands on (the bisection's
// lower end): a leap of k steps advances k - 1 in closed form and takes the last step with a real addition.
#include "svr_walk.hpp"
#include "svr_project.hpp"

namespace svr {

#define SVR_PJ_THREADS 256

namespace {

// ------------------------------------------------------------------------------------------------------------------
// The sample parameters are a float accumulation chain t_{n+1} = fl(t_n + h).  Within one binade every t is a multiple
// of u = ulp, and fl(t + h) = t + delta with ONE delta for the whole binade (unless the rounding error is exactly u / 2,
// where ties-to-even alternates).  So k steps inside a binade are t + k * delta on the integer mantissas; the step that
// crosses into the next binade is a real float addition.  (The same closed form as svr_raycast.hip, whose text stays as
// it is; tests/test_more_gpu.py checks that one against a plain loop, tests/test_projection_gpu.py this one through the
// images.)
// ------------------------------------------------------------------------------------------------------------------
struct ChainSeg { uint32_t A, J, kmax; float u; bool ok; };     // t = A u, delta = J u, steps k <= kmax stay in the binade

SVR_DEV ChainSeg chain_segment(float t, float h)
{
    ChainSeg g;
    const uint32_t tb = __float_as_uint(t);
    const uint32_t ex = tb >> 23;                                   // t >= 1: sign 0, exponent >= 127
    g.u = __uint_as_float((ex - 23u) << 23);
    g.A = (tb & 0x7fffffu) | 0x800000u;
    const float t1 = t + h;
    const float delta = t1 - t;                                     // exact
    const float err = h - delta;                                    // exact: the rounding error of t + h
    const bool same = (__float_as_uint(t1) >> 23) == ex;
    g.J = (uint32_t)(delta * __uint_as_float((127u + 127u + 23u - ex) << 23));        // delta / u, an integer < 2^24
    g.ok = same && delta > 0.f && __builtin_fabsf(err) != 0.5f * g.u && t >= 1.f && ex < 127u + 100u;
    g.kmax = g.ok ? (0xffffffu - g.A) / g.J : 0u;
    return g;
}

// number of chain elements t^[0] = t, t^[1], ... that are < bound (inclusive: <= bound).  If the chain leaves the closed
// form first, the count is a lower bound (still safe to skip) and exact is false.
SVR_DEV uint32_t chain_count(float t, float h, float bound, bool inclusive, bool& exact)
{
    uint32_t n = 0;
    exact = true;
    for (int seg = 0; seg < 6; ++seg) {
        if (!(inclusive ? t <= bound : t < bound)) return n;
        const ChainSeg g = chain_segment(t, h);
        if (!g.ok) {
            const float t1 = t + h;                                 // one real step (binade crossing), or give up
            if (!(t1 > t) || !(t >= 1.f)) { exact = false; return n; }
            n += 1u; t = t1;
            continue;
        }
        const float xs = bound * __uint_as_float((254u - (__float_as_uint(g.u) >> 23)) << 23);      // bound / u (exact scaling)
        uint32_t k_in;
        if (xs >= 16777216.f) k_in = g.kmax + 1u;                  // the bound lies beyond this binade
        else {
            const float fl = __builtin_floorf(xs);
            uint32_t X = (uint32_t)fl;                               // t is before the bound, so X >= A >= 2^23
            if (!inclusive && fl == xs) X -= 1u;
            k_in = X >= g.A ? (X - g.A) / g.J + 1u : 0u;
            if (k_in > g.kmax + 1u) k_in = g.kmax + 1u;
        }
        n += k_in;
        if (k_in <= g.kmax) return n;                              // the bound was met inside the binade
        t = (float)(g.A + g.kmax * g.J) * g.u;                     // continue from the first element of the next binade
        t = t + h;
    }
    exact = false;
    return n;
}

// t after n chain steps; ok = false if the closed form gave up (t is then unchanged)
SVR_DEV float chain_advance(float t, float h, uint32_t n, bool& ok)
{
    const float t_in = t;
    ok = true;
    for (int seg = 0; seg < 8 && n != 0u; ++seg) {
        const ChainSeg g = chain_segment(t, h);
        if (!g.ok) {
            const float t1 = t + h;
            if (!(t1 > t) || !(t >= 1.f)) { ok = false; return t_in; }
            t = t1; n -= 1u;
            continue;
        }
        const uint32_t k = n < g.kmax ? n : g.kmax;
        t = (float)(g.A + k * g.J) * g.u;                          // exact: an integer below 2^24 times a power of two
        n -= k;
        if (n != 0u) { t = t + h; n -= 1u; }                       // the crossing step
    }
    if (n != 0u) { ok = false; return t_in; }
    return t;
}

// macro-cell of a trilinear cell (cell_is_empty's index); false outside the grid
SVR_DEV bool macro_of(const DevScene& s, const Cell& c, uint32_t& m)
{
    const uint32_t ux = (uint32_t)(c.cx + 1), uy = (uint32_t)(c.cy + 1), uz = (uint32_t)(c.cz + 1);
    const bool inb = (ux <= (uint32_t)s.nx) & (uy <= (uint32_t)s.ny) & (uz <= (uint32_t)s.nz);
    const uint32_t sh = (uint32_t)s.mc_shift;
    const uint32_t qx = min(ux >> sh, (uint32_t)s.mc_gx - 1u), qy = min(uy >> sh, (uint32_t)s.mc_gy - 1u), qz = min(uz >> sh, (uint32_t)s.mc_gz - 1u);
    m = inb ? qx + qy * (uint32_t)s.mc_gx + qz * (uint32_t)s.mc_gxy : 0u;
    return inb;
}

// can no fetch whose raw values are <= r change the ray's state?  (MIP: st = M; ISO: st = iso; MEAN: unused)
template <int MODE>
SVR_DEV bool skippable(const DevScene& s, uint32_t r, float st)
{
    if (MODE == PROJ_MEAN) return r == 0u;
    const float imax = ((float)r * 1.5259021896696422e-05f) * s.densityScale;       // the two multiplies of tex_fetch / intensity_at
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

template <int LAYOUT, int MODE>
static void launch_cs(const DevScene& s, const DevWork& w, const DevProjection& pj, float stepSize, bool count, bool skip, uint32_t blocks, hipStream_t st)
{
    const dim3 g(blocks), b(SVR_PJ_THREADS);
    if (count) {
        if (skip) hipLaunchKernelGGL((k_project<LAYOUT, MODE, true, true>), g, b, 0, st, s, w, pj, stepSize);
        else hipLaunchKernelGGL((k_project<LAYOUT, MODE, true, false>), g, b, 0, st, s, w, pj, stepSize);
    } else {
        if (skip) hipLaunchKernelGGL((k_project<LAYOUT, MODE, false, true>), g, b, 0, st, s, w, pj, stepSize);
        else hipLaunchKernelGGL((k_project<LAYOUT, MODE, false, false>), g, b, 0, st, s, w, pj, stepSize);
    }
}

template <int LAYOUT>
static void launch_m(const DevScene& s, const DevWork& w, const DevProjection& pj, float stepSize, bool count, bool skip, uint32_t blocks, hipStream_t st)
{
    if (pj.mode == PROJ_MIP) launch_cs<LAYOUT, PROJ_MIP>(s, w, pj, stepSize, count, skip, blocks, st);
    else if (pj.mode == PROJ_MEAN) launch_cs<LAYOUT, PROJ_MEAN>(s, w, pj, stepSize, count, skip, blocks, st);
    else launch_cs<LAYOUT, PROJ_ISO>(s, w, pj, stepSize, count, skip, blocks, st);
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
    const uint32_t blocks = need < max_blocks ? (need ? need : 1u) : max_blocks;
    const bool skip = pj.mm != nullptr;
    if (s.layout == LAYOUT_CELL) launch_m<LAYOUT_CELL>(s, w, pj, stepSize, count, skip, blocks, st);
    else if (s.layout == LAYOUT_PAIR) launch_m<LAYOUT_PAIR>(s, w, pj, stepSize, count, skip, blocks, st);
    else if (s.layout == LAYOUT_LINEAR) launch_m<LAYOUT_LINEAR>(s, w, pj, stepSize, count, skip, blocks, st);
    else launch_m<LAYOUT_BRICK>(s, w, pj, stepSize, count, skip, blocks, st);
    return hipGetLastError();
}

} // namespace svr
