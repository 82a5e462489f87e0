// svr_slice.hip -- slice views (svr_render_slice, svr_render_slice_stack, include/svr_abi.h): an orthographic window onto a
// plane through the volume, axis-aligned or oblique, optionally thickened into a slab of K samples along the plane's normal
// that is reduced by maximum, minimum or mean.  The definition is in the header and is implemented here literally, float32
// without contraction.  With k_project it shares the macro-cell bound (svr_walk.hpp: macro_of, raw_bound), with every kernel the sampler.
//
// One lane owns one pixel (MEAN needs its sum in sample order); a wave is an 8 x 8 pixel tile, persistent 256-thread blocks
// pull tasks from the sharded tickets.  A task is (slice, tile), slice-major, so a stack of any size is one launch.  Mode,
// colour, counting and skipping are wave-uniform run-time branches: the kernel is instantiated per volume layout only.
//
// SAMPLES.  The offset of sample j is the product d_j = fl(fl(j * step) - half_thickness), not a running sum, so a sample
// that is not fetched costs one multiply, one subtraction, the point and the inside test, and nothing has to be replayed.
//
// SKIPPING (result-neutral, SVR_OPT_EMPTY_SKIP).  Every intensity a fetch in macro-cell m can return satisfies
//     Imin(m) = raw_bound(rmin(m))  <=  I  <=  Imax(m) = raw_bound(rmax(m)),
// with rmin, rmax from the volume's macro-cell table mm and the macro-cell from the sampler's own cell (svr_walk.hpp, macro_of and
// raw_bound, where the argument stands), so the test needs no margin.
//   MIP:    a sample with Imax(m) <= M leaves M = max(M, I) as it is: not fetched.
//   MINIP:  a sample with Imin(m) >= M leaves M = min(M, I) as it is: not fetched (M starts at +inf: the first counting
//           sample is always fetched).
//   MEAN and the single plane: rmax(m) == 0: all eight voxels are 0, every lerp is fma(t, 0, 0) = +0 and the product with
//           the two non-negative factors is +0 (-0 under densityScale = -0): S + (+-0) = S bit for bit (S starts at +0 and
//           never becomes -0), and a plane value of +-0 maps to the same colour as +0 (g = (+-0 - lo) / d clamps to 0 or is
//           -lo / d either way; the table coordinate of the transfer function is fma(+-0, n, -0.5) = -0.5).  The sample
//           still counts.
// A verdict is kept while consecutive counting samples stay in one macro-cell (the table costs a dependent load): a kept
// "fetch" is always safe; a kept "skip" stays true because M only grows (MIP), only shrinks (MINIP), or is not looked at.
// Skipped samples count in raycast_steps and vol_taps, not in vol_taps_executed.  The host passes the table for MIP and
// MINIP slabs only: on a single plane the test costs a table load to save one fetch at most, and for MEAN it lost on every
// scene measured; the rule for them stays here because it is the same branch.
#include "svr_walk.hpp"
#include "svr_slice.hpp"

namespace svr {

#define SVR_SL_THREADS 256

template <int LAYOUT>
__global__ __launch_bounds__(SVR_SL_THREADS) void k_slice(const DevScene s, const DevWork w, const DevSlice sl)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = w.x1 - w.x0;
    const uint32_t tiles_x = (wv + 7u) >> 3, tiles_y = (w.n_rows + 7u) >> 3;
    const uint32_t tiles = tiles_x * tiles_y;
    const uint32_t n_tasks = tiles * sl.count;                      // < 2^32, checked on the host
    const uint32_t per_shard = (n_tasks + TICKET_SHARDS - 1u) / TICKET_SHARDS;
    const uint32_t shard0 = blockIdx.x % TICKET_SHARDS;
    const bool color_tf = (sl.flags & SLICE_COLOR_TF) != 0u;
    const bool skip_on = sl.mm != nullptr;
    const int mode = sl.mode;
    const v3 U = V3(sl.u[0], sl.u[1], sl.u[2]), V = V3(sl.v[0], sl.v[1], sl.v[2]), N = V3(sl.n[0], sl.n[1], sl.n[2]);
    const float fw = (float)s.imageW, fh = (float)s.imageH;
    uint32_t n_steps = 0, n_exec = 0;

    for (uint32_t si = 0; si < TICKET_SHARDS; ++si) {
        const uint32_t shard = (shard0 + si) % TICKET_SHARDS;
        const uint32_t t_begin = shard * per_shard;
        const uint32_t t_count = t_begin >= n_tasks ? 0u : min(per_shard, n_tasks - t_begin);
        uint32_t* ticket = w.ticket + shard * TICKET_STRIDE;
        for (;;) {
            uint32_t tk = 0;
            if (lane == 0) tk = atomicAdd(ticket, 1u);
            tk = __builtin_amdgcn_readfirstlane(tk);
            if (tk >= t_count) break;
            const uint32_t task = t_begin + tk;
            const uint32_t slice = task / tiles, tile = task - slice * tiles;
            const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
            const uint32_t px = (tx << 3) + (lane & 7u), r = (ty << 3) + (lane >> 3);
            if (!(px < wv && r < w.n_rows)) continue;                 // (lane 0 always owns a pixel of its tile)
            const uint32_t x = w.x0 + px, y = owned_row_to_y(w, r);

            v3 ck = V3(sl.center[0], sl.center[1], sl.center[2]);
            if (slice != 0u) ck = ck + N * (sl.spacing * (float)slice);
            const float a = ((float)x + 0.5f) - 0.5f * fw;
            const float b = ((float)y + 0.5f) - 0.5f * fh;
            const v3 c = (ck + U * a) + V * b;

            float M = mode == SLAB_MINIP ? u2f(SVR_INF_BITS) : 0.f;    // MIP: running maximum; MINIP: running minimum; MEAN: running sum
            uint32_t counted = 0, fetched = 0;
            uint32_t seen_m = 0xffffffffu;                            // the macro-cell of the previous counting sample and its verdict
            bool seen_skip = false;
            for (uint32_t j = 0; j < sl.K; ++j) {
                const float d = (float)j * sl.step - sl.half_thickness;
                const v3 p = c + N * d;
                const bool inside = (p.x >= sl.box_lo[0]) & (p.x <= sl.box_hi[0]) & (p.y >= sl.box_lo[1]) & (p.y <= sl.box_hi[1]) &
                                    (p.z >= sl.box_lo[2]) & (p.z <= sl.box_hi[2]);
                if (!inside) continue;
                counted++;
                const Cell cl = cell_of(s, p);
                bool skip = false;
                if (skip_on) {
                    uint32_t m;
                    const bool inb = macro_of(s, cl, m);
                    if (inb && m == seen_m) skip = seen_skip;
                    else {
                        if (inb) {
                            if (mode == SLAB_MIP) skip = raw_bound(s, sl.mm[2u * m + 1u]) <= M;
                            else if (mode == SLAB_MINIP) skip = raw_bound(s, sl.mm[2u * m]) >= M;
                            else skip = sl.mm[2u * m + 1u] == 0u;
                        }
                        seen_m = inb ? m : 0xffffffffu; seen_skip = skip;
                    }
                }
                if (!skip) {
                    fetched++;
                    const float I = tex_fetch<LAYOUT>(s, cl) * s.densityScale;
                    if (mode == SLAB_MIP) M = fmax_(M, I);
                    else if (mode == SLAB_MINIP) M = fmin_(M, I);
                    else if (mode == SLAB_MEAN) M = M + I;
                    else M = I;
                }
            }
            n_steps += counted; n_exec += fetched;

            uint32_t rgba = 0u;                                   // no counting sample: (0, 0, 0, 0)
            if (counted != 0u) {
                if (mode == SLAB_MEAN) M = M / (float)counted;
                float cr, cg, cb;
                if (color_tf) {
                    float co[4];
                    tf_rgba(s, s.tf, M, co);
                    cr = fmin_(fmax_(co[0], 0.f), 1.f); cg = fmin_(fmax_(co[1], 0.f), 1.f); cb = fmin_(fmax_(co[2], 0.f), 1.f);
                } else {
                    const float g = fmin_(fmax_((M - sl.window_lo) / (sl.window_hi - sl.window_lo), 0.f), 1.f);
                    cr = g; cg = g; cb = g;
                }
                rgba = to_u8(cr * 255) | (to_u8(cg * 255) << 8) | (to_u8(cb * 255) << 16) | (255u << 24);
            }
            reinterpret_cast<uint32_t*>(w.img)[((size_t)slice * s.imageH + y) * s.imageW + x] = rgba;
        }
    }
    if (sl.counting) {
        const unsigned long long st = wave_sum((unsigned long long)n_steps), ex = wave_sum((unsigned long long)n_exec);
        if (lane == 0) {
            atomicAdd(&w.counters[CNT_RAYCAST], st);
            atomicAdd(&w.counters[CNT_VOL_TAPS], st);
            atomicAdd(&w.counters[CNT_TAPS_EXEC], ex);
        }
    }
}

hipError_t launch_slice(const DevScene& s, const DevWork& w, const DevSlice& sl, int num_cus, hipStream_t st)
{
    if (w.x1 == w.x0 || w.n_rows == 0 || sl.count == 0u) return hipSuccess;
    if (sl.mode != SLICE_PLANE && sl.mode != SLAB_MIP && sl.mode != SLAB_MINIP && sl.mode != SLAB_MEAN) return hipErrorInvalidValue;
    const uint64_t n_tasks = (uint64_t)((w.x1 - w.x0 + 7u) >> 3) * ((w.n_rows + 7u) >> 3) * sl.count;
    if (n_tasks > 0xffffffffull - TICKET_SHARDS) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(w.ticket, 0, sizeof(uint32_t) * TICKET_SHARDS * TICKET_STRIDE, st);
    if (e != hipSuccess) return e;
    const uint64_t need = (n_tasks + SVR_SL_THREADS / 64 - 1u) / (SVR_SL_THREADS / 64);
    const uint32_t max_blocks = (uint32_t)num_cus * 8u;                  // 8 blocks of 4 waves per CU, no LDS
    const dim3 g(persistent_blocks(need, max_blocks)), b(SVR_SL_THREADS);
    with_layout(s.layout, [&](auto lay) { hipLaunchKernelGGL((k_slice<decltype(lay)::value>), g, b, 0, st, s, w, sl); });
    return hipGetLastError();
}

} // namespace svr
