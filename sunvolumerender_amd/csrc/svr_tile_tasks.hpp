// svr_tile_tasks.hpp -- what the persistent tile kernels (svr_trace_tile.hip, svr_trace_lm.hip, svr_trace_env.hip) share: the order in which a
// launch's wave-tasks are handed out (task_take, task_lanes; task_launch_setup on the host), and the running mean of a pixel's frames
// inside the kernel (fold_pending).
#pragma once
#include "svr_kernel_common.hpp"

namespace svr {

// SVR_TILE_LIST = 1: the builds of adaptive launches (svr_render_pathtracer_adaptive; the *_list.hip sources compile the trace kernels a second
// time, into namespace svr_list): the tasks run over DevWork.tile_list.  0 (the ordinary builds): the full grid, DevWork.tile_list is not read --
// the remap costs registers in the persistent kernels, so it is not in their code at all
#ifndef SVR_TILE_LIST
#define SVR_TILE_LIST 0
#endif

// task index of the centre-out order -> tile row, tile column, frame group (see k_trace_tile)
struct TaskShape {
    uint32_t tiles_x, tiles_y, fgroups, row_tasks, c_row, tw2, th2, P2, fl2, wv, n_tasks;
#if SVR_TILE_LIST
    const uint32_t* list;
#endif
};

// tasks of a launch: the wave tiles of the grid x frame groups, or (list builds with DevWork.tile_list set) the (16 >> tw2) x (16 >> th2)
// wave tiles of every listed 16 x 16 tile x frame groups.  Host and device (the launchers size their grids with it)
__host__ __device__ inline uint32_t launch_tasks(const DevWork& w, uint32_t tw2, uint32_t th2, uint32_t fgroups)
{
#if SVR_TILE_LIST
    if (w.tile_list != nullptr) return (w.tile_count << ((4u - tw2) + (4u - th2))) * fgroups;
#endif
    return (((w.x1 - w.x0) + (1u << tw2) - 1u) >> tw2) * ((w.n_rows + (1u << th2) - 1u) >> th2) * fgroups;
}

SVR_DEV TaskShape task_shape(const DevWork& w)
{
    TaskShape ts;
    ts.wv = w.x1 - w.x0;
    ts.fl2 = w.frames_log2;                                   // 0..6
    ts.P2 = 6u - ts.fl2;                                      // log2(pixels per wave)
    ts.tw2 = (ts.P2 + 1u) >> 1; ts.th2 = ts.P2 >> 1;          // pixel block 8x8, 8x4, 4x4, 4x2, 2x2, 2x1, 1x1
    ts.tiles_x = (ts.wv + (1u << ts.tw2) - 1u) >> ts.tw2;
    ts.tiles_y = (w.n_rows + (1u << ts.th2) - 1u) >> ts.th2;
    ts.fgroups = (w.nframes + (1u << ts.fl2) - 1u) >> ts.fl2;
    ts.row_tasks = ts.tiles_x * ts.fgroups;                   // tasks of one tile row
    ts.c_row = ts.tiles_y >> 1;
#if SVR_TILE_LIST
    ts.list = w.tile_list;
#endif
    ts.n_tasks = launch_tasks(w, ts.tw2, ts.th2, ts.fgroups);
    return ts;
}
SVR_DEV void task_decode(const TaskShape& ts, uint32_t k, uint32_t& tx, uint32_t& ty, uint32_t& fg)
{
#if SVR_TILE_LIST
    if (ts.list != nullptr) {
        // adaptive launch (whole frame): task k = (listed 16 x 16 tile a, wave tile j inside it, frame group).  The wave tiles nest exactly in
        // the 16 x 16 tiles, so tx, ty are coordinates of the ordinary grid; those past the image edge have no live lane
        const uint32_t sx2 = 4u - ts.tw2, sy2 = 4u - ts.th2;
        const uint32_t per = ts.fgroups << (sx2 + sy2);
        const uint32_t a = k / per, in_t = k - a * per;
        const uint32_t j = in_t / ts.fgroups;
        fg = in_t - j * ts.fgroups;
        const uint32_t p = ts.list[a];
        tx = ((p & 0xffffu) << sx2) + (j & ((1u << sx2) - 1u));
        ty = ((p >> 16) << sy2) + (j >> sx2);
        return;
    }
#endif
    const uint32_t rr = k / ts.row_tasks, in_row = k - rr * ts.row_tasks;
    const uint32_t off = (rr + 1u) >> 1;
    ty = (rr & 1u) ? ts.c_row - off : ts.c_row + off;
    tx = in_row / ts.fgroups;
    fg = in_row - tx * ts.fgroups;
}

// The next task of ticket counter `shard` for this wave, or TASK_NONE: the counter is drained.  si = how many counters the wave has
// visited before this one: away from its home counter (si != 0) it looks before taking -- when the launch runs out every wave visits
// every counter once, and a plain load of a drained counter is free (the counters only grow: a stale value just means one atomic more).
constexpr uint32_t TASK_NONE = 0xffffffffu;
SVR_DEV uint32_t task_take(const DevWork& w, const TaskShape& ts, uint32_t shard, uint32_t si, uint32_t lane)
{
    uint32_t* ticket = w.ticket + shard * TICKET_STRIDE;
    if (si != 0u && __atomic_load_n(ticket, __ATOMIC_RELAXED) * TICKET_SHARDS + shard >= ts.n_tasks) return TASK_NONE;
    uint32_t u = 0;
    if (lane == 0) u = atomicAdd(ticket, 1u);
    u = __builtin_amdgcn_readfirstlane(u);
    const uint32_t k = u * TICKET_SHARDS + shard;
    return k < ts.n_tasks ? k : TASK_NONE;
}

// What lane `lane` of the wave holds of task k: pixel column px and row r (of the launch's window / owned rows), frame slot, and whether
// all three lie inside the launch.  The low P2 bits of a lane number its pixel in the task's tw x th block, the rest its frame.
struct TaskLanes { uint32_t px, r, slot; bool live; };
SVR_DEV TaskLanes task_lanes(const TaskShape& ts, const DevWork& w, uint32_t k, uint32_t lane)
{
    uint32_t tx, ty, fg;
    task_decode(ts, k, tx, ty, fg);
    const uint32_t pl = lane & ((1u << ts.P2) - 1u);
    TaskLanes t;
    t.slot = (fg << ts.fl2) + (lane >> ts.P2);
    t.px = (tx << ts.tw2) + (pl & ((1u << ts.tw2) - 1u));
    t.r = (ty << ts.th2) + (pl >> ts.tw2);
    t.live = t.px < ts.wv && t.r < w.n_rows && t.slot < w.nframes;
    return t;
}

// Host side of the same, for the launchers of the persistent kernels (launch_tile_t, launch_lm_t, launch_env_t): frames per wave, the
// task count and the grid of a launch, its DevWork (unit = one task per ticket) and the reset of the ticket counters.
//   frames per wave: the largest power of two <= min(nframes, 64), unless frames_log2 >= 0 asks for fewer; a FOLDING launch (fold:
//   in-kernel accumulation) keeps every frame of a pixel in ONE wave -- frame lanes 0 .. nframes - 1 of its group; the caller has
//   checked nframes <= 64, or (the tile kernel's wide-draining builds) a multiple of 64: then a task is one pixel x one group of 64 frames
//   grid: one wave per task up to num_cus x blocks_per_cu x 4 waves
struct TaskGrid { uint32_t n_tasks, blocks; };
inline hipError_t task_launch_setup(const DevWork& w, const LaunchCfg& cfg, uint32_t waves_per_block, bool fold, int frames_log2, hipStream_t st,
                                    DevWork& w2, TaskGrid& g)
{
    uint32_t fl2 = 0;
    while (fl2 < 6u && (2u << fl2) <= w.nframes) ++fl2;
    if (frames_log2 >= 0 && (uint32_t)frames_log2 < fl2) fl2 = (uint32_t)frames_log2;
    if (fold) {
        fl2 = 0;
        while (fl2 < 6u && (1u << fl2) < w.nframes) ++fl2;          // (more than 64 frames: whole groups of 64, the tile kernel's wide-draining builds)
    }
    const uint32_t P2 = 6u - fl2, tw2 = (P2 + 1u) >> 1, th2 = P2 >> 1;
    const uint32_t fgroups = (w.nframes + (1u << fl2) - 1u) >> fl2;
    g.n_tasks = launch_tasks(w, tw2, th2, fgroups);
    const uint32_t max_blocks = (uint32_t)(cfg.num_cus * cfg.blocks_per_cu) * 4u / waves_per_block;
    g.blocks = (g.n_tasks + waves_per_block - 1u) / waves_per_block;
    if (g.blocks > max_blocks) g.blocks = max_blocks;
    if (g.blocks == 0) g.blocks = 1;
    w2 = w;
    w2.unit = 1u;
    w2.frames_log2 = fl2;
    return hipMemsetAsync(w.ticket, 0, sizeof(uint32_t) * TICKET_SHARDS * TICKET_STRIDE, st);
}

// running_estimate (pathtracer.cu:81-84,279) for the pending tasks of this wave: the 1 << fl2 lanes of a task that
// hold one pixel are that pixel's frames frame0 .. frame0 + nframes - 1 IN ORDER, so one lane per (pixel, channel)
// replays the reference's sequence acc += (L - acc) / (n + 1) frame by frame -- the same float operations in the same
// order as nframes calls of the reference -- and the accumulator is read and written once per launch (12 B per
// pixel) instead of once per frame.  clear_hdr_buffer (pathtracer.cu:86-94) is the frame0 == 0 case.
// rows: [task * 3 + channel] rows of `row` floats (this wave's), tasks: their task numbers
// AHEAD (SVR_FOLD_LOAD_AHEAD; rows in GLOBAL memory: the traceDepth-1 QUEUE builds of the tile kernel, the local-majorant pools): the chain of divisions had
// one exposed load round trip in front of every link (global_load, s_waitcnt vmcnt(0), 13 dependent instructions; 2 x 64 links per 32 tasks
// of the headline launch).  The samples of FOLD_CHUNK frames are loaded together, then folded in frame order: c3 + 1.4 % ... + 2.3 % (two boxes)
// (profiles/r06_notes_experiments.txt).  Rows in LDS (the straight-line builds, 4 pending tasks) keep the plain loop: they lost 0.9 % with it.
#ifndef SVR_FOLD_LOAD_AHEAD
#define SVR_FOLD_LOAD_AHEAD 1
#endif
constexpr uint32_t FOLD_CHUNK = 8;
template <bool AHEAD = true>
SVR_DEV void fold_pending(const DevScene& s, const DevWork& w, const float* rows, uint32_t row, const uint32_t* tasks, uint32_t npend)
{
    const TaskShape ts = task_shape(w);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t npx = 1u << ts.P2;
    const uint32_t items = npend * npx * 3u;
    const uint32_t nfr = min(w.nframes, 1u << ts.fl2);
    for (uint32_t i = lane; i < items; i += 64u) {
        const uint32_t pi = (i * 0xAAABu) >> 17;           // i / 3 for i < 2^15
        const uint32_t ch = i - 3u * pi;
        const uint32_t q = pi >> ts.P2, pl = pi & (npx - 1u);
        uint32_t tx, ty, fg;
        task_decode(ts, tasks[q], tx, ty, fg);
        const uint32_t px = (tx << ts.tw2) + (pl & ((1u << ts.tw2) - 1u));
        const uint32_t r = (ty << ts.th2) + (pl >> ts.tw2);
        if (px >= ts.wv || r >= w.n_rows) continue;
        const uint32_t x = w.x0 + px, y = owned_row_to_y(w, r);
        float* h = w.hdr + 3 * ((size_t)y * s.imageW + x) + ch;
        float acc = (w.frame0 == 0u) ? 0.f : *h;
        const float* rp = rows + (size_t)(q * 3u + ch) * row + pl;
        if (w.nan_guard) {
            // SVR_OPT_NAN_GUARD: a non-finite sample (the reference's 0/0, pathtracer.cu:106-131) is replaced by the running mean
            for (uint32_t f = 0; f < nfr; ++f) {
                float Lf = rp[f << ts.P2];
                Lf = (f2u(Lf) & 0x7f800000u) == 0x7f800000u ? acc : Lf;
                const float n1 = (float)(w.frame0 + f) + 1.f;
                acc = acc + (Lf - acc) / n1;
            }
        } else {
            uint32_t f = 0;
            if constexpr (AHEAD && SVR_FOLD_LOAD_AHEAD) {
                for (; f + FOLD_CHUNK <= nfr; f += FOLD_CHUNK) {
                    float Lv[FOLD_CHUNK];
#pragma unroll
                    for (uint32_t j = 0; j < FOLD_CHUNK; ++j) Lv[j] = rp[(f + j) << ts.P2];
#pragma unroll
                    for (uint32_t j = 0; j < FOLD_CHUNK; ++j) {
                        const float n1 = (float)(w.frame0 + f + j) + 1.f;
                        acc = acc + (Lv[j] - acc) / n1;
                    }
                }
            }
            for (; f < nfr; ++f) {
                const float Lf = rp[f << ts.P2];
                const float n1 = (float)(w.frame0 + f) + 1.f;
                acc = acc + (Lf - acc) / n1;
            }
        }
        *h = acc;
    }
}

// fold_pending for a folding launch of SEVERAL groups of 64 frames (fgroups > 1: one pixel x 64 frames per task, nframes a multiple of 64; the
// wide-draining builds of svr_trace_tile.hip only -- every other kernel keeps fold_pending, so its text does not move).  The launcher makes a ticket a
// multiple of fgroups tasks, so the groups 0 .. fgroups - 1 of a pixel are consecutive tasks of ONE wave, in order, and the running mean of a pixel
// is replayed in frame order across them:
//   * the groups of a pixel that are pending together are CHAINED in one accumulator: one read of hdr, fgroups x 64 links, one write.  A chain
//     starts at a pending task that is group 0 or does not follow its predecessor's task number; one lane per (chain, channel);
//   * a pixel whose groups straddle two drains continues from hdr: the first part writes it, the second part reads it back (fg > 0) even when
//     frame0 == 0.  This wave wrote that value itself in its previous flush -- no other wave ever touches the pixel -- and the workgroup fences
//     around flush() order the store before this load;
//   * the clear (acc = 0) is for absolute frame 0 alone: frame0 == 0 and group 0.
// The sample number of frame lane f of group fg is frame0 + 64 fg + f.  rows: [task * 3 + channel] rows of 64 floats.
SVR_DEV void fold_pending_groups(const DevScene& s, const DevWork& w, const float* rows, const uint32_t* tasks, uint32_t npend)
{
    const TaskShape ts = task_shape(w);                    // P2 == 0, fl2 == 6: a task is one pixel, tx / ty are its column / row
    const uint32_t lane = threadIdx.x & 63u;
    // the chain heads among the (at most 64) pending tasks, and the r-th head's index in lane r
    const bool mine = lane < npend;
    const uint32_t k_l = mine ? tasks[lane] : 0u, k_p = (mine && lane != 0u) ? tasks[lane - 1u] : 0u;
    uint32_t tx_l, ty_l, fg_l;
    task_decode(ts, k_l, tx_l, ty_l, fg_l);
    const bool head = mine && (lane == 0u || fg_l == 0u || k_p + 1u != k_l);
    const uint64_t heads = __ballot(head);
    const uint32_t nheads = (uint32_t)__popcll(heads);
    const uint32_t rank = (uint32_t)__popcll(heads & ((1ull << lane) - 1ull));
    const uint32_t dest = head ? rank : nheads + (lane - rank);                  // a permutation of the lanes: heads first, in order
    const uint32_t q_of = (uint32_t)__builtin_amdgcn_ds_permute((int)(dest << 2), (int)lane);
    const uint32_t items = nheads * 3u;
    for (uint32_t i0 = 0u; i0 < items; i0 += 64u) {
        const uint32_t i = i0 + lane;
        const uint32_t j = (i * 0xAAABu) >> 17;            // i / 3 for i < 2^15
        const uint32_t ch = i - 3u * j;
        const uint32_t q = (uint32_t)__shfl((int)q_of, (int)(j & 63u), 64);
        if (i >= items) continue;
        uint32_t tx, ty, fg;
        task_decode(ts, tasks[q], tx, ty, fg);
        if (tx >= ts.wv || ty >= w.n_rows) continue;
        const uint64_t above = q < 63u ? heads >> (q + 1u) : 0ull;
        const uint32_t len = above ? (uint32_t)__builtin_ctzll(above) + 1u : npend - q;     // pending groups of this pixel from q on
        const uint32_t x = w.x0 + tx, y = owned_row_to_y(w, ty);
        float* h = w.hdr + 3 * ((size_t)y * s.imageW + x) + ch;
        float acc = (w.frame0 == 0u && fg == 0u) ? 0.f : *h;
        for (uint32_t gi = 0u; gi < len; ++gi) {
            const float* rp = rows + (size_t)((q + gi) * 3u + ch) * 64u;
            const uint32_t n0 = w.frame0 + ((fg + gi) << 6);
            if (w.nan_guard) {
                // SVR_OPT_NAN_GUARD, as in fold_pending
                for (uint32_t f = 0; f < 64u; ++f) {
                    float Lf = rp[f];
                    Lf = (f2u(Lf) & 0x7f800000u) == 0x7f800000u ? acc : Lf;
                    const float n1 = (float)(n0 + f) + 1.f;
                    acc = acc + (Lf - acc) / n1;
                }
            } else {
                for (uint32_t f = 0; f < 64u; f += FOLD_CHUNK) {
                    float Lv[FOLD_CHUNK];
#pragma unroll
                    for (uint32_t jj = 0; jj < FOLD_CHUNK; ++jj) Lv[jj] = rp[f + jj];
#pragma unroll
                    for (uint32_t jj = 0; jj < FOLD_CHUNK; ++jj) {
                        const float n1 = (float)(n0 + f + jj) + 1.f;
                        acc = acc + (Lv[jj] - acc) / n1;
                    }
                }
            }
        }
        *h = acc;
    }
}

// Launches that do NOT fold (frames traced ahead of the calls that ask for them, svr_api_trace.hip: k_resolve / k_mean_flat fold one scratch slot
// per call): the radiance of the path with id = (pending task << 6 | lane) of this wave goes straight to lbuf[frame slot][pixel].
// tasks: the wave's pending task numbers (LDS).
SVR_DEV void direct_put(const DevScene& s, const DevWork& w, const uint32_t* tasks, uint32_t id, v3 L)
{
    const TaskShape ts = task_shape(w);
    uint32_t tx, ty, fg;
    task_decode(ts, tasks[id >> 6], tx, ty, fg);
    const uint32_t ln = id & 63u, pl = ln & ((1u << ts.P2) - 1u), fs = ln >> ts.P2;
    const uint32_t px = (tx << ts.tw2) + (pl & ((1u << ts.tw2) - 1u));
    const uint32_t r = (ty << ts.th2) + (pl >> ts.tw2);
    const uint32_t x = w.x0 + px, y = owned_row_to_y(w, r), slot = (fg << ts.fl2) + fs;
    float* o = w.lbuf + (size_t)slot * w.slot_stride + 3 * ((size_t)y * s.imageW + x);
    o[0] = L.x; o[1] = L.y; o[2] = L.z;
}

} // namespace svr
