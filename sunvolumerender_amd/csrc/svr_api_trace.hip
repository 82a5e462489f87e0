// svr_api_trace.hip -- the path tracer's side of the C-ABI layer (svr_api.hip): the launch plan of a render call, its folding and
// pipelined launches, the frames traced ahead, and the render_pathtracer entry points.
#include "svr_api_state.hpp"

#include <cstring>

namespace svr_fast { hipError_t launch_trace_tile_raw(const void* scene, const void* work, const void* cfg, hipStream_t st); }   // svr_trace_tile_fast.hip
// the trace kernels of adaptive launches (DevWork.tile_list set): svr_trace_{tile,lm,env}_list.hip
namespace svr_list {
hipError_t launch_trace_tile_raw(const void* scene, const void* work, const void* cfg, hipStream_t st);
hipError_t launch_trace_lm_raw(const void* scene, const void* work, const void* cfg, hipStream_t st);
hipError_t launch_trace_env_raw(const void* scene, const void* work, const void* cfg, hipStream_t st);
}

using namespace svr_host;

namespace {

// scratch radiance slots: sized for the frame and for the largest group requested so far (a host that only
// ever calls render_pathtracer keeps 1 slot per set; svr_render_pathtracer_frames grows it up to GROUP)
int ensure_slots(uint32_t W, uint32_t H, uint32_t nslots)
{
    size_t need = (size_t)3 * W * H;
    if (g.slot_floats == need && g.slots_per_set >= nslots) return 0;
    HIP_TRY(hipDeviceSynchronize());
    invalidate_ahead();
    for (auto& st : g.sets) {
        if (st.lbuf) { HIP_TRY(hipFree(st.lbuf)); st.lbuf = nullptr; }
        st.used = false;
    }
    if (g.slot_floats != need || nslots > g.slots_per_set) g.slots_per_set = nslots;
    for (auto& st : g.sets) HIP_TRY(hipMalloc((void**)&st.lbuf, need * sizeof(float) * g.slots_per_set));
    g.slot_floats = need;
    return 0;
}

// per-wave path-record queues (REC_WORDS x QUEUE_CAP_MAX words) and pending-radiance rows (QUEUE_TASKS_MAX x 3 x 64 floats) of the
// tile kernel's QUEUE builds (svr_trace_tile.hip, svr_lanes.hpp), sized for the largest form (svr_kernels.hpp, DrainShape: 1024 records in
// every build, 64 tasks in the skipping traceDepth-1 builds): 184 KB + 48 KB per wave, 0.95 GB for 256 blocks.  The builds with 32 tasks
// and the local-majorant pools use the front of their slices.
// soft: the caller can do without them (SVR_OPT_QUEUE = 1): running out of device memory is then not an error, the launches
// use the straight-line kernel and the allocation is not tried again until the option is set anew.
using svr::QUEUE_WORDS_PER_BLOCK;
using svr::PEND_FLOATS_PER_BLOCK;
int ensure_record_queues(uint32_t blocks, bool soft, bool& available)
{
    available = true;
    if (g.d_queue && g.d_pend && g.queue_blocks >= blocks) return 0;
    if (soft && g.queue_alloc_failed) { available = false; return 0; }
    HIP_TRY(hipDeviceSynchronize());
    if (g.d_queue) { HIP_TRY(hipFree(g.d_queue)); g.d_queue = nullptr; }
    if (g.d_pend) { HIP_TRY(hipFree(g.d_pend)); g.d_pend = nullptr; }
    g.queue_blocks = 0;
    hipError_t e = hipMalloc((void**)&g.d_queue, QUEUE_WORDS_PER_BLOCK * sizeof(uint32_t) * blocks);
    if (e == hipSuccess) e = hipMalloc((void**)&g.d_pend, PEND_FLOATS_PER_BLOCK * sizeof(float) * blocks);
    if (e != hipSuccess) {
        if (g.d_queue) { (void)hipFree(g.d_queue); g.d_queue = nullptr; }
        g.d_pend = nullptr;
        if (soft && e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            g.queue_alloc_failed = true;
            available = false;
            return 0;
        }
        return fail((int)e, "HIP error allocating the tile kernel's queue memory (%zu MB: %u records and %u task rows per wave): %s",
                    ((QUEUE_WORDS_PER_BLOCK + PEND_FLOATS_PER_BLOCK) * 4 * blocks) >> 20, svr::QUEUE_CAP_MAX, svr::QUEUE_TASKS_MAX, hipGetErrorName(e));
    }
    g.queue_blocks = blocks;
    return 0;
}

int ensure_queues(uint32_t W, uint32_t H)
{
    size_t need = (size_t)W * H * Context::GROUP;
    if (g.queue_capacity == need) return 0;
    HIP_TRY(hipDeviceSynchronize());
    for (auto& st : g.sets) {
        for (auto& p : st.planes) if (p) { HIP_TRY(hipFree(p)); p = nullptr; }
        if (!st.wf_counts) HIP_TRY(hipMalloc((void**)&st.wf_counts, 64 * sizeof(uint32_t)));
    }
    if (need >= ((size_t)1 << 31)) return fail(-3, "frame too large for the wavefront queues");
    for (auto& st : g.sets)
        for (auto& p : st.planes) HIP_TRY(hipMalloc((void**)&p, need * sizeof(float4)));
    g.queue_capacity = need;
    return 0;
}

// What a render call decides once (plan_launch) and every launch of the call reads
struct LaunchPlan {
    svr::DevScene s;
    svr::LaunchCfg cfg;
    void* img = nullptr;
    const svr_render_params* rp = nullptr;
    const TileList* tiles = nullptr;    // the launches trace these tiles only
    bool fold_batch = false;            // the tile kernel folds the frames of its launches into the accumulator
    bool use_queue = false;             // ... in its QUEUE builds
    bool fold_groups = false;           // ... and a folding launch may take several groups of 64 frames (fold_group_frames)
    bool local_majorant = false;        // the local-majorant kernel in place of the tile kernel
    bool frame_ahead = false;           // one frame per call, the next ones traced ahead (render_ahead)
};

// short launches (< FOLD_MIN frames) keep the slots: they end in a tail of a few long tasks that only overlapping launches
// on several streams hide, and a folding launch cannot overlap its predecessor (measured, 1 frame per call: 0.276 vs 0.366 ms)
constexpr uint32_t FOLD_MIN = 8;

// the launch plan of a render call of nframes >= 1 frames: every automatic decision, and the device memory its launches need
int plan_launch(LaunchPlan& p, void* img, const svr_render_params* rp, uint32_t nframes, const TileList* adaptive)
{
    svr::DevScene& s = p.s;
    svr::LaunchCfg& cfg = p.cfg;
    p.img = img;
    p.rp = rp;
    p.tiles = adaptive != nullptr && adaptive->list != nullptr ? adaptive : nullptr;
    if (build_scene(g.vol, g.tf, g.cam, s)) return g.err_code;
    if (add_lights_env(s)) return g.err_code;
    if ((size_t)3 * s.imageW * s.imageH >= ((size_t)1 << 32)) return fail(-3, "image too large");
    // clear_hdr_buffer zeroes the WHOLE accumulator at frame 0 (pathtracer.cu:86-94,297-300); under a row shard or a
    // window the kernels only touch their own pixels, so the rest is cleared here (the strips of the ranks are then
    // summed into one frame: stale values outside the owned rows would corrupt it)
    if (rp->frameNo == 0 && partial_frame(s.imageW, s.imageH))
        HIP_TRY(hipMemsetAsync(rp->hdrBuffer, 0, sizeof(float) * 3 * (size_t)s.imageW * s.imageH, g.stream));
    cfg.kernel = g.opt_kernel == svr::KERNEL_AUTO ? svr::KERNEL_TILE : g.opt_kernel;
    // OPT-IN importance sampling of the environment map (svr_trace_env.hip): where there is a map, the environment term is on and a bounce follows the
    // first scatter event (the env sample of event k pairs with the escape term of bounce k + 1)
    if (g.opt_env_nee && cfg.kernel == svr::KERNEL_TILE && s.env != nullptr && s.env_cdf != nullptr && s.env_on_escape && rp->traceDepth >= 2 && !g.opt_debug_stop)
        cfg.kernel = svr::KERNEL_ENV_NEE;
    if ((cfg.kernel == svr::KERNEL_TILE || cfg.kernel == svr::KERNEL_WAVEFRONT || cfg.kernel == svr::KERNEL_ENV_NEE) && ensure_mask(s, g.vol, g.tf)) return g.err_code;
    if (cfg.kernel == svr::KERNEL_WAVEFRONT) {
        if (rp->traceDepth > 15) return fail(-3, "the wavefront kernels support traceDepth <= 15 (got %u)", rp->traceDepth);
        if (ensure_queues(s.imageW, s.imageH)) return g.err_code;
    }
    cfg.count = g.opt_count != 0;
    cfg.num_cus = g.num_cus;
    cfg.blocks_per_cu = g.opt_blocks_per_cu > 0 ? g.opt_blocks_per_cu : 4;
    cfg.frames_log2 = g.opt_frames_log2;
    cfg.unit_override = g.opt_unit;
    cfg.lm_straight = g.opt_local_majorant == 2;
    cfg.pool_primary = false;            // (decided below, once the acceleration data says what kind of medium this is)
    // The tile kernel folds the frames of a launch into the accumulator itself (running mean in frame order, 12 B per
    // pixel per launch, svr_trace_tile.hip); the scratch slots + k_resolve remain for frames traced AHEAD of the calls
    // that ask for them (their radiance is folded later, one frame per call) and for the other kernels.
    p.fold_batch = cfg.kernel == svr::KERNEL_TILE && g.opt_fold && !g.opt_debug_stop && cfg.frames_log2 < 0;
    // QUEUE builds (the hits of a task are shaded in place, then their paths continue on a per-lane state machine,
    // svr_lanes.hpp) ride on the folding launches.  Auto: with empty-space skipping on (without it every walk is long and the
    // straight-line code wins: c3, 1660 against 1452 Msamples/s), for deep paths and media without exactly transparent space
    // always (c3 depth 2 / 4: +10 % / +30 %, c3n: +34 %), otherwise when the launch gives every wave at least
    // QUEUE_AUTO_TASKS_PER_WAVE = 128 tasks (c3 / c4 / c5: +4 % / +3 % / +12 %; c2, 512^2 pixels: -2 %).  The threshold was set as 4 drains of
    // 32 tasks and stays where it was measured now that the traceDepth-1 builds drain 64 at a time (c3 has 256 tasks per wave)
    p.use_queue = p.fold_batch && g.opt_queue == 2;
    if (p.fold_batch && g.opt_queue == 1 && g.opt_empty_skip) {
        svr::DevWork wq;
        fill_work(wq, s.imageW, s.imageH);
        const uint64_t waves = (uint64_t)(cfg.num_cus * cfg.blocks_per_cu) / 4u * svr::TILE_WAVES;    // blocks of 1024 threads
        p.use_queue = rp->traceDepth >= 2 || s.bound_cull || (uint64_t)wq.n_items >= svr::QUEUE_AUTO_TASKS_PER_WAVE * waves;
    }
    // OPT-IN local majorants (svr_trace_lm.hip): needs the class table and whole-ray validity; its folding launches keep the waves'
    // pending radiance in the rows next to the record queues
    p.local_majorant = g.opt_local_majorant && cfg.kernel == svr::KERNEL_TILE && s.empty_mask != nullptr && s.ray_skip && !g.opt_debug_stop;
    // the slot-per-path pool of deeper paths settles its walks (slot loads and stores) and refills less eagerly: 2 cells per turn, a
    // refill from 32 idle lanes, settling from 48 ended walks (c3 depth 4: 3 390 Msamples/s against 2 630 with the depth-1 setting,
    // c3n depth 4: 1 080 against 810; gpurun_out/r03u_tune.log)
    if (p.local_majorant && !g.opt_lm_tune && rp->traceDepth > 1) s.lm_tune = 2u | (32u << 8) | (48u << 16) | (s.lm_tune & 0xff000000u);
    if (p.local_majorant) p.use_queue = false;
    // POOL (svr_trace_tile.hip): pooled primary walks pay where the walks of a wave are not coherent -- media without exactly transparent
    // space under bound culling (c3n) -- and cost where they are (c3): auto = such media only
    cfg.pool_primary = p.use_queue && (g.opt_pool == 2 || (g.opt_pool == 1 && s.bound_cull && !s.has_empty));
    if (p.use_queue || (p.local_majorant && p.fold_batch)) {          // (a frame-ahead call traces its batches with the same kernels)
        bool available = true;
        if (ensure_record_queues((uint32_t)(cfg.num_cus * cfg.blocks_per_cu) * 4u / 16u, g.opt_queue == 1 && !p.local_majorant, available)) return g.err_code;
        p.use_queue = p.use_queue && available;
    }
    p.frame_ahead = nframes == 1 && g.opt_frame_ahead && g.opt_pipeline && !g.opt_count && !g.opt_debug_stop && cfg.kernel == svr::KERNEL_TILE &&
                    adaptive == nullptr;
    // Folding launches of SEVERAL groups of 64 frames (SVR_OPT_GROUP_FRAMES = 128 / 256) exist in one form of the tile kernel: the skipping traceDepth-1
    // queue builds without pooled walks, one pixel x 64 frames per task, full grid, tickets in units of tasks (launch_tile_t refuses every other launch
    // of more than 64 frames).  Every other plan keeps at most 64 frames per launch
    p.fold_groups = p.fold_batch && p.use_queue && !p.local_majorant && !cfg.pool_primary && p.tiles == nullptr && rp->traceDepth == 1 &&
                    s.empty_mask != nullptr && s.layout != svr::LAYOUT_LINEAR && s.cam_pinhole && s.ray_skip && !g.opt_row_order && !p.frame_ahead;
    // (whole groups of 64 frames go first: what is left of a call is less than the smaller of 64 and the option)
    const uint32_t tail_frames = nframes % (uint32_t)(p.fold_batch ? (g.opt_group_frames < 64 ? g.opt_group_frames : 64) : Context::GROUP);
    if ((!p.fold_batch || p.frame_ahead || (tail_frames != 0 && tail_frames < FOLD_MIN)) &&
        ensure_slots(s.imageW, s.imageH, nframes < (uint32_t)Context::GROUP ? nframes : (uint32_t)Context::GROUP)) return g.err_code;
    return 0;
}

// the fields every trace launch of the plan shares: the owned pixels (fill_work), frames first .. first + n - 1 into rp's accumulator, the
// image if want_img, and the tile list of an adaptive call
svr::DevWork launch_work(const LaunchPlan& p, uint32_t first, uint32_t n, bool want_img)
{
    svr::DevWork w;
    fill_work(w, p.s.imageW, p.s.imageH);
    w.hdr = (float*)p.rp->hdrBuffer;
    w.img = want_img ? (uint8_t*)p.img : nullptr;
    w.traceDepth = p.rp->traceDepth;
    w.frame0 = first;
    w.nframes = n;
    if (p.tiles) {
        // adaptive launch (whole frame, one process): the listed tiles only; the ticket arithmetic of row_order assumes the full grid
        w.tile_list = p.tiles->list;
        w.tile_count = p.tiles->count;
        w.tile_active = p.tiles->active;
        w.row_order = 0;
    }
    return w;
}

// one launch of the plan's trace kernel on stream st (set: the scratch set it traces into, whose wavefront queues KERNEL_WAVEFRONT uses), between
// the events of the timing ring (SVR_OPT_TIMING); a launch that uses the record queues runs behind their previous user
int launch_trace(const LaunchPlan& p, const svr::DevWork& w, hipStream_t st, const Context::SlotSet* set)
{
    const svr::DevScene& s = p.s;
    const svr::LaunchCfg& cfg = p.cfg;
    const bool listed = w.tile_list != nullptr;
    int slot = -1;
    if (g.opt_timing) {
        if (g.ev_count == Context::EV_RING) collect_timing();
        slot = g.ev_head;
        HIP_TRY(hipEventRecord(g.ev0[slot], st));
    }
    if (w.queue != nullptr && g.queue_used) HIP_TRY(hipStreamWaitEvent(st, g.queue_done, 0));
    if (cfg.kernel == svr::KERNEL_WAVEFRONT)
        HIP_TRY(svr::launch_wavefront(s, w, cfg, set->planes, set->wf_counts, (uint32_t)g.queue_capacity, st));
    else if (cfg.kernel == svr::KERNEL_ENV_NEE) HIP_TRY(listed ? svr_list::launch_trace_env_raw(&s, &w, &cfg, st) : svr::launch_trace_env(s, w, cfg, st));
    else if (cfg.kernel != svr::KERNEL_TILE) HIP_TRY(svr::launch_pathtrace(s, w, cfg, st));
    else if (p.local_majorant) HIP_TRY(listed ? svr_list::launch_trace_lm_raw(&s, &w, &cfg, st) : svr::launch_trace_lm(s, w, cfg, st));
    else if (listed) HIP_TRY(svr_list::launch_trace_tile_raw(&s, &w, &cfg, st));
    else HIP_TRY(g.opt_fast_math ? svr_fast::launch_trace_tile_raw(&s, &w, &cfg, st) : svr::launch_trace_tile(s, w, cfg, st));
    if (w.queue != nullptr) { HIP_TRY(hipEventRecord(g.queue_done, st)); g.queue_used = true; }
    if (g.opt_timing) {
        HIP_TRY(hipEventRecord(g.ev1[slot], st));
        g.ev_head = (g.ev_head + 1) % Context::EV_RING;
        g.ev_count++;
    }
    return 0;
}

// one folding launch: trace + accumulate on the caller's stream (the launches of a render update the same accumulator,
// so they run in order anyway), tone map behind the last one
int trace_fold(const LaunchPlan& p, uint32_t first, uint32_t n, bool want_img)
{
    svr::DevWork w = launch_work(p, first, n, want_img);
    w.ticket = g.d_ticket + (size_t)svr::TICKET_SHARDS * svr::TICKET_STRIDE * Context::NSETS;   // (the sets' own counters may be in use by frames traced ahead)
    w.fold = 1u;
    const bool queues = p.use_queue || p.local_majorant;
    w.queue = queues ? g.d_queue : nullptr;
    w.pend = queues ? g.d_pend : nullptr;
    w.queue_blocks = g.queue_blocks;
    if (launch_trace(p, w, g.stream, nullptr)) return g.err_code;
    if (want_img) HIP_TRY(svr::launch_tonemap(p.s, w, g.stream));
    return 0;
}

int next_set()
{
    const int si = g.next_set;
    g.next_set = (g.next_set + 1) % Context::NSETS;
    return si;
}

// one trace launch of n_trace frames starting at frame `first` into scratch set `si`, then the resolve of its
// first n_resolve frames (with_queue: the QUEUE build of the tile kernel)
int trace_group(const LaunchPlan& p, int si, uint32_t first, uint32_t n_trace, uint32_t n_resolve, bool want_img, bool with_queue = false)
{
    Context::SlotSet& set = g.sets[si];
    for (auto& a : g.ahead) if (a.valid && a.set == si) a.valid = false;     // its slots are about to be overwritten
    hipStream_t ts = g.opt_pipeline ? set.stream : g.stream;
    svr::DevWork w = launch_work(p, first, n_trace, want_img);
    w.lbuf = set.lbuf;
    w.slot_stride = (uint32_t)g.slot_floats;
    w.ticket = g.d_ticket + (size_t)svr::TICKET_SHARDS * svr::TICKET_STRIDE * si;
    if (with_queue) { w.queue = g.d_queue; w.pend = g.d_pend; w.queue_blocks = g.queue_blocks; }
    // the scratch slots of this set are free again once their previous resolve has run
    if (g.opt_pipeline && set.used) HIP_TRY(hipStreamWaitEvent(ts, set.resolved, 0));
    // A large trace launch fills the chip by itself; running two of them at once only makes them share L2
    // and stretches both.  They are chained (the resolve of one still overlaps the trace of the next).
    // Smaller launches (one frame per call; a GPU's share of the frame under row sharding) end in a ~0.1 ms
    // tail of a few long tasks and overlap freely to hide it.
    if (g.opt_pipeline && (uint64_t)w.n_items * n_trace >= Context::CHAIN_MIN_PATHS && g.prev_traced)
        HIP_TRY(hipStreamWaitEvent(ts, g.prev_traced, 0));
    if (launch_trace(p, w, ts, &set)) return g.err_code;
    if (g.opt_pipeline) {
        HIP_TRY(hipEventRecord(set.traced, ts));
        g.prev_traced = set.traced;
        // (a batch traced purely AHEAD -- nothing of it is resolved by this call -- must not hold the caller's stream: the calls that
        // consume the batch in stock run beside it and wait for `traced` when they get to this one)
        if (n_resolve) HIP_TRY(hipStreamWaitEvent(g.stream, set.traced, 0));
    }
    if (n_resolve) {
        w.nframes = n_resolve;
        HIP_TRY(svr::launch_resolve(p.s, w, g.stream));
        if (g.opt_pipeline) HIP_TRY(hipEventRecord(set.resolved, g.stream));
    }
    set.used = true;
    if (n_resolve < n_trace) {
        // a free entry, else the older batch
        Context::Ahead& a = !g.ahead[0].valid ? g.ahead[0] : (!g.ahead[1].valid ? g.ahead[1] : (g.ahead[0].first < g.ahead[1].first ? g.ahead[0] : g.ahead[1]));
        a.valid = true; a.scene = p.s; a.shape = w; a.content = g.content_version;
        a.first = first; a.count = n_trace; a.depth = p.rp->traceDepth; a.set = si;
    }
    return 0;
}

// The reference's host calls render_pathtracer once per frame (gui/canvas.cpp:96).  A frame's radiance is a pure
// function of (scene, pixel, frame number), so frames can be traced AHEAD of the calls that ask for them: a
// 32-frame launch costs 0.13 ms per frame on c3, a 1-frame launch 0.23.  The batch doubles with the frame number
// (1, 2, 4 ... GROUP), so a host that restarts the render on every mouse event never traces more than twice what
// it shows.  Anything that could change a frame -- scene PODs, texture contents, window, shard, trace depth --
// invalidates the frames in stock.
int render_ahead(const LaunchPlan& p, bool want_img)
{
    const svr::DevScene& s = p.s;
    const uint32_t n = p.rp->frameNo;
    svr::DevWork shape;
    fill_work(shape, s.imageW, s.imageH);
    // at most 4 GB of scratch frames per set (64 frames up to ~2300^2 pixels; fewer for larger images)
    const uint64_t slot_bytes = (uint64_t)3 * s.imageW * s.imageH * sizeof(float);
    uint32_t batch_max = 1;
    while (batch_max < (uint32_t)Context::AHEAD_MAX && 2ull * batch_max * slot_bytes <= (4ull << 30)) batch_max *= 2u;
    // the queue builds of the tile kernel (first scatter events shaded in place, then the lane machine) for the batches too: they hand
    // their radiance rows to the scratch slots instead of folding them (svr_tile_tasks.hpp, scatter_pending)
    const bool ahead_queue = p.use_queue && !p.local_majorant && !g.opt_fast_math;
    auto in_stock = [&](const Context::Ahead& a, uint32_t frame) {
        return a.valid && a.content == g.content_version && a.depth == p.rp->traceDepth && frame >= a.first && frame - a.first < a.count &&
               memcmp(&a.scene, &s, sizeof s) == 0 && same_shape(a.shape, shape);
    };
    for (Context::Ahead& a : g.ahead) {
        if (!in_stock(a, n)) continue;
        // in stock: fold slot n - first into the accumulator
        Context::SlotSet& set = g.sets[a.set];
        svr::DevWork w = launch_work(p, n, 1, want_img);
        w.slot_stride = (uint32_t)g.slot_floats;
        w.lbuf = set.lbuf + (size_t)(n - a.first) * g.slot_floats;
        HIP_TRY(hipStreamWaitEvent(g.stream, set.traced, 0));
        HIP_TRY(svr::launch_resolve(s, w, g.stream));
        HIP_TRY(hipEventRecord(set.resolved, g.stream));
        // steady state: a full batch takes as long to trace as to consume, so the NEXT one starts when this one is first used (it runs on
        // its set's stream beside the per-call resolves: the queue builds of the tile kernel leave the register room a resolve wave needs)
        // (while the batches still grow -- 1, 2, 4 ... -- the next one, twice as long, is started the same way: the ramp's traces then run back to
        // back instead of each waiting for its predecessor to be consumed; a host that restarts the render has at most two batches traced in vain)
        const uint32_t next_first = a.first + a.count;
        const uint32_t next_count = 2u * a.count < batch_max ? 2u * a.count : batch_max;
        if (next_count > 1u && !in_stock(g.ahead[0], next_first) && !in_stock(g.ahead[1], next_first))
            return trace_group(p, next_set(), next_first, next_count, 0, false, ahead_queue && next_count >= 16u);
        return 0;
    }
    uint32_t batch = 1;
    while (batch < batch_max && 2u * batch <= n + 1u) batch *= 2u;
    if (batch_max > 1 && ensure_slots(s.imageW, s.imageH, batch_max)) return g.err_code;
    if (trace_group(p, next_set(), n, batch, 1, want_img, ahead_queue && batch >= 16u)) return g.err_code;
    if (batch_max > 1) {
        const uint32_t next_count = 2u * batch < batch_max ? 2u * batch : batch_max;
        return trace_group(p, next_set(), n + batch, next_count, 0, false, ahead_queue && next_count >= 16u);
    }
    return 0;
}

// frames of the next launch of a folding call with `left` frames to go: SVR_OPT_GROUP_FRAMES of them.  Above 64 that is whole groups of 64 frames in one
// launch where the plan has the form for it (LaunchPlan.fold_groups) and the ticket unit, if the caller set one, is a multiple of the group count (the
// groups of a pixel must stay in one wave: launch_tile_t); otherwise 64.  What is left below 64 frames is one launch as ever
uint32_t fold_group_frames(const LaunchPlan& p, uint32_t left)
{
    const uint32_t group = (uint32_t)g.opt_group_frames;
    if (group <= 64u || left < 128u || !p.fold_groups) {
        const uint32_t cap = group < 64u ? group : 64u;
        return left < cap ? left : cap;
    }
    const uint32_t n = (left < group ? left : group) & ~63u;
    if (g.opt_unit > 0 && (uint32_t)g.opt_unit % (n >> 6) != 0u) return 64u;
    return n;
}

} // namespace

namespace svr_host {

void collect_timing()
{
    while (g.ev_count > 0) {
        int i = (g.ev_head - g.ev_count + 2 * Context::EV_RING) % Context::EV_RING;
        float ms = 0.f;
        if (hipEventSynchronize(g.ev1[i]) == hipSuccess && hipEventElapsedTime(&ms, g.ev0[i], g.ev1[i]) == hipSuccess) {
            g.kernel_ms += (double)ms;
            g.kernel_launches += 1;
        }
        g.ev_count--;
    }
}

// do two launches (fill_work) cover the same pixels: window, strip rows, rank, world?
bool same_shape(const svr::DevWork& a, const svr::DevWork& b)
{
    return a.x0 == b.x0 && a.x1 == b.x1 && a.y0 == b.y0 && a.y1 == b.y1 && a.strip_rows == b.strip_rows && a.rank == b.rank && a.world == b.world;
}

// nframes frames into rp's accumulator, tone-mapped into img if `tonemap` (adaptive: the launches of an adaptive call, else null)
int render_frames_traced(void* img, const svr_render_params* rp, uint32_t nframes, bool tonemap, const TileList* adaptive)
{
    if (ensure_init()) return g.err_code;
    if (!rp) return fail(-4, "render_pathtracer: renderParams is null");
    if (!g.have_vol || !g.have_tf || !g.have_cam)
        return fail(-4, "render_pathtracer before setup_volume/setup_transferfunction/setup_camera");
    if (!rp->hdrBuffer) return fail(-4, "render_pathtracer: renderParams.hdrBuffer is null (call SetupHDRBuffer)");
    if (nframes == 0) return 0;
    LaunchPlan p;
    if (plan_launch(p, img, rp, nframes, adaptive)) return g.err_code;
    const bool want_img = tonemap && !g.opt_skip_tonemap;
    if (p.frame_ahead) return render_ahead(p, want_img);
    // folding launches may take 64 frames (a wave = ONE pixel x 64 frames): half as many launch boundaries
    for (uint32_t g0 = 0, n = 0; g0 < nframes; g0 += n) {
        n = p.fold_batch ? fold_group_frames(p, nframes - g0) : (nframes - g0 < (uint32_t)Context::GROUP ? nframes - g0 : (uint32_t)Context::GROUP);
        const bool img_now = want_img && g0 + n >= nframes;
        if (p.fold_batch && n >= FOLD_MIN) {
            if (trace_fold(p, rp->frameNo + g0, n, img_now)) return g.err_code;
        } else if (trace_group(p, next_set(), rp->frameNo + g0, n, n, img_now)) return g.err_code;
    }
    return 0;
}

// show the whole accumulator hdr in img: the denoised preview if `denoise` and its memory is available, else the tone map
int show_full_frame(void* img, const void* hdr, bool denoise)
{
    if (denoise) {
        bool ok = true;
        if (denoise_frame(img, nullptr, hdr, g.cam.imageW, g.cam.imageH, g.dn, true, ok)) return g.err_code;
        if (ok) return 0;
    }
    svr::DevScene s;
    if (build_scene(g.vol, g.tf, g.cam, s)) return g.err_code;
    svr::DevWork w;
    fill_work_full(w, s.imageW, s.imageH);
    w.hdr = (float*)const_cast<void*>(hdr);
    w.img = (uint8_t*)img;
    HIP_TRY(svr::launch_tonemap(s, w, g.stream));
    return 0;
}

// render_pathtracer / svr_render_pathtracer_frames.  SVR_OPT_DENOISE_PREVIEW = N > 0: while the frame shown has at most N samples per
// pixel the traced frames are resolved WITHOUT their tone map, and guides (if stale) + filter + tone map follow on the caller's stream --
// behind the resolve or fold that writes the accumulator, so svr_device_synchronize still waits for the shown image.  Inert under a row
// shard, a render window or SVR_OPT_SKIP_TONEMAP.
int render_frames_shown(void* img, const svr_render_params* rp, uint32_t nframes, bool tonemap)
{
    const bool preview = rp && img && nframes > 0 && tonemap && !g.opt_skip_tonemap && g.opt_denoise_preview > 0 && g.have_vol && g.have_tf && g.have_cam &&
                         (uint64_t)rp->frameNo + nframes <= (uint64_t)g.opt_denoise_preview && !partial_frame(g.cam.imageW, g.cam.imageH);
    if (render_frames_traced(img, rp, nframes, tonemap && !preview, nullptr)) return g.err_code;
    if (!preview) return 0;
    return show_full_frame(img, rp->hdrBuffer, true);
}

// ... and, with SVR_OPT_NOISE_ESTIMATE on, the estimate's state rules behind the call (they only read the accumulator)
int render_frames(void* img, const svr_render_params* rp, uint32_t nframes, bool tonemap)
{
    if (ensure_init()) return g.err_code;
    const uint64_t call = ++g.render_calls;
    if (render_frames_shown(img, rp, nframes, tonemap)) return g.err_code;
    if (!g.opt_noise_estimate) return 0;
    return noise_after_render(rp, nframes, call);
}

} // namespace svr_host

extern "C" {

// ---------------- render entry points ----------------
void render_pathtracer(void* img, const svr_render_params* renderParams)
{
    render_frames(img, renderParams, 1, true);
}

int svr_render_pathtracer_frames(void* img, const svr_render_params* renderParams, uint32_t nframes)
{
    return render_frames(img, renderParams, nframes, true);
}

int svr_hdr_to_ldr(void* img, const svr_render_params* rp)
{
    if (ensure_init()) return g.err_code;
    if (!rp || !rp->hdrBuffer || !img) return fail(-4, "svr_hdr_to_ldr: null argument");
    if (!g.have_vol || !g.have_tf || !g.have_cam) return fail(-4, "svr_hdr_to_ldr before setup_*");
    svr::DevScene s;
    if (build_scene(g.vol, g.tf, g.cam, s)) return g.err_code;
    svr::DevWork w;
    fill_work(w, s.imageW, s.imageH);
    w.hdr = (float*)rp->hdrBuffer;
    w.img = (uint8_t*)img;
    HIP_TRY(svr::launch_tonemap(s, w, g.stream));
    return 0;
}

int svr_hdr_to_ldr_frame(void* img, const void* hdr, uint32_t w_, uint32_t h_)
{
    if (ensure_init()) return g.err_code;
    if (!hdr || !img || w_ == 0 || h_ == 0) return fail(-4, "svr_hdr_to_ldr_frame: bad argument");
    if (!g.have_cam) return fail(-4, "svr_hdr_to_ldr_frame before setup_camera (the exposure comes from the camera)");
    svr::DevScene s;
    memset(&s, 0, sizeof s);
    s.imageW = w_; s.imageH = h_;
    s.exposure = g.cam.exposure;
    svr::DevWork w;
    fill_work_full(w, w_, h_);
    w.hdr = (float*)const_cast<void*>(hdr);
    w.img = (uint8_t*)img;
    HIP_TRY(svr::launch_tonemap(s, w, g.stream));
    return 0;
}

} // extern "C"
