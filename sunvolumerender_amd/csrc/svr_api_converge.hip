// svr_api_converge.hip -- how a render converges, in the C-ABI layer (svr_api.hip): the denoised preview, the noise estimate,
// render-until-converged and adaptive sampling.
#include "svr_api_state.hpp"
#include "svr_denoise.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace svr_host;

namespace {

// ---------------- denoised preview (svr_denoise.hip) ----------------

int check_denoise_params(const svr_denoise_params& p)
{
    if (p.passes < 1 || p.passes > 10) return fail(-6, "svr_denoise_params.passes must be 1..10 (got %d)", p.passes);
    const float v[6] = {p.sigma_depth, p.sigma_normal, p.sigma_albedo, p.sigma_opacity, p.sigma_color, p.step};
    for (float x : v)
        if (!std::isfinite(x) || x < 0.f) return fail(-6, "svr_denoise_params: sigmas and step must be finite and >= 0");
    return 0;
}

// march step of the guides: p.step, or half the smallest voxel edge of the volume in world units
float guide_step(const svr::DevScene& s, const svr_denoise_params& p)
{
    if (p.step > 0.f) return p.step;
    double e = 1e30;
    const double n[3] = {s.fnx, s.fny, s.fnz};
    for (int a = 0; a < 3; ++a) {
        const double edge = 1.0 / ((double)s.invSize[a] * n[a]);
        if (edge > 0.0 && edge < e) e = edge;
    }
    return (float)(0.5 * e);
}

// device memory of the preview; soft: an allocation failure is recorded in svr_last_error() without an error code and
// reported as `ok` = false (the caller falls back to the ordinary tone map)
int ensure_denoise_memory(size_t px, bool soft, bool& ok)
{
    ok = true;
    auto grow = [&](float4*& buf, size_t& have, size_t want) -> int {
        if (have >= want && buf) return 0;
        if (buf) HIP_TRY(hipFree(buf));
        buf = nullptr; have = 0;
        const hipError_t e = hipMalloc((void**)&buf, want * sizeof(float4));
        if (e == hipSuccess) { have = want; return 0; }
        buf = nullptr;
        (void)hipGetLastError();
        if (!soft) return fail((int)e, "denoise: hipMalloc of %zu bytes failed: %s", want * sizeof(float4), hipGetErrorName(e));
        g.err_msg = std::string("denoise preview: device memory unavailable (") + hipGetErrorName(e) + "), fell back to the ordinary tone map";
        ok = false;
        return 0;
    };
    if (g.guides_px < px) g.guides_valid = false;
    if (grow(g.d_guides, g.guides_px, 2 * px)) return g.err_code;
    if (!ok) return 0;
    if (grow(g.d_dn_scratch, g.dn_scratch_px, 2 * px)) return g.err_code;
    return 0;
}

// the guides of the current scene in g.d_guides, recomputed on the caller's stream only when something they depend on changed
int ensure_guides(const svr_denoise_params& p, bool soft, bool& ok)
{
    svr::DevScene s;
    if (build_scene(g.vol, g.tf, g.cam, s)) return g.err_code;
    const size_t px = (size_t)s.imageW * s.imageH;
    if (ensure_denoise_memory(px, soft, ok) || !ok) return g.err_code;
    const float h = guide_step(s, p);
    Texture* tt = find_tex(g.tf.tex, TEX_TF);
    const uint64_t tf_version = tt ? tt->version : 0;
    if (g.guides_valid && memcmp(&g.guides_key, &s, sizeof s) == 0 && g.guides_vol == g.vol.tex && g.guides_tf == g.tf.tex &&
        g.guides_tf_version == tf_version && g.guides_h == h && g.guides_skip == g.opt_empty_skip)
        return 0;
    const svr::DevScene key = s;
    if (ensure_mask(s, g.vol, g.tf)) return g.err_code;       // empty-space skipping (same guides without it)
    HIP_TRY(svr::launch_guides(s, g.d_guides, h, g.stream));
    g.guides_valid = true;
    g.guides_key = key;
    g.guides_vol = g.vol.tex; g.guides_tf = g.tf.tex; g.guides_tf_version = tf_version;
    g.guides_h = h;
    g.guides_skip = g.opt_empty_skip;
    g.guide_builds++;
    return 0;
}

// ---------------- noise estimate (svr_noise.hip) ----------------

// per-tile buffers of `tiles` tiles; soft: an allocation failure sets ok = false and a message without an error code
int ensure_noise_buf(Context::NoiseBuf& b, size_t tiles, bool soft, bool& ok)
{
    ok = true;
    if (b.mem && b.tiles >= tiles) return 0;
    if (b.mem) HIP_TRY(hipFree(b.mem));
    b.mem = nullptr; b.tiles = 0;
    const size_t bytes = sizeof(svr::NoiseTotals) + tiles * (sizeof(double) + sizeof(float) + 2 * sizeof(uint32_t));
    const hipError_t e = hipMalloc(&b.mem, bytes);
    if (e == hipSuccess) { b.tiles = tiles; return 0; }
    b.mem = nullptr;
    (void)hipGetLastError();
    if (!soft) return fail((int)e, "noise estimate: hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorName(e));
    g.err_msg = std::string("noise estimate: device memory unavailable (") + hipGetErrorName(e) + "), no estimate for this render";
    ok = false;
    return 0;
}

// launch arguments for the estimate of A(n) against A(m) over the pixels of `own` (a DevWork of fill_work / fill_work_full)
svr::NoiseArgs noise_args(uint32_t W, uint32_t H, const svr::DevWork& own, uint32_t m, uint32_t n, float exposure)
{
    svr::NoiseArgs a;
    a.W = W; a.H = H;
    a.tiles_x = (W + svr::NOISE_TILE - 1u) / svr::NOISE_TILE;
    a.tiles_y = (H + svr::NOISE_TILE - 1u) / svr::NOISE_TILE;
    a.x0 = own.x0; a.x1 = own.x1; a.y0 = own.y0; a.y1 = own.y1;
    a.strip_rows = own.strip_rows ? own.strip_rows : 1u; a.rank = own.rank; a.world = own.world;
    a.exposure = exposure;
    a.ratio = (float)((double)m / (double)(n - m));
    a.scale = (float)((double)m * (double)(n - m) / ((double)n * (double)n));
    return a;
}

void noise_fill(svr_noise_estimate& out, const svr::NoiseTotals& t, uint32_t m, uint32_t n, uint32_t tiles_x, uint32_t tiles_y)
{
    out.frames = n;
    out.frames_ref = m;
    out.tiles_x = tiles_x;
    out.tiles_y = tiles_y;
    out.pixels = t.pixels;
    out.nonfinite = t.nonfinite;
    out.sse = t.sse;
    out.rmse = t.pixels ? (float)std::sqrt(t.sse / (double)t.pixels) : std::nanf("");
    out.tile_max = t.tile_max;
}

// would a render call of rp, made next, continue the render the estimate follows?
bool noise_continues(const svr_render_params* rp, uint64_t call)
{
    const Context::Noise& ns = g.ns;
    if (!ns.tracking || rp->frameNo == 0 || rp->frameNo != ns.last_n || ns.call + 1 != call || ns.hdr != rp->hdrBuffer ||
        ns.W != g.cam.imageW || ns.H != g.cam.imageH || ns.depth != rp->traceDepth)
        return false;
    svr::DevWork w;
    fill_work(w, g.cam.imageW, g.cam.imageH);
    return same_shape(w, ns.shape);
}

// the snapshot A(m) of the tracked render for px pixels; soft: an allocation failure sets ok = false and a message without an error code
int ensure_noise_snap(size_t px, bool soft, bool& ok)
{
    Context::Noise& ns = g.ns;
    ok = true;
    if (ns.d_snap && ns.snap_px >= px) return 0;
    if (ns.d_snap) HIP_TRY(hipFree(ns.d_snap));
    ns.d_snap = nullptr; ns.snap_px = 0;
    const hipError_t e = hipMalloc((void**)&ns.d_snap, px * 3 * sizeof(float));
    if (e == hipSuccess) { ns.snap_px = px; return 0; }
    ns.d_snap = nullptr;
    (void)hipGetLastError();
    if (!soft) return fail((int)e, "noise estimate: hipMalloc of %zu bytes failed: %s", px * 3 * sizeof(float), hipGetErrorName(e));
    g.err_msg = std::string("noise estimate: device memory unavailable (") + hipGetErrorName(e) + "), no estimate for this render";
    ok = false;
    return 0;
}

// HIP_TRY for a loop that must leave through its end: 0, or the error code with the message set
int hip_check(hipError_t e)
{
    if (e == hipSuccess) return 0;
    return fail((int)e, "HIP error in svr_render_pathtracer_adaptive: code=%d(%s)", (int)e, hipGetErrorName(e));
}

// the active tiles, packed tx | ty << 16, in the centre-out tile-row order of the full grid (svr_tile_tasks.hpp task_decode: rows c, c + 1,
// c - 1, c + 2 ...), and their map -> device.  The library's streams are drained first: no launch still reads the previous list.
int adaptive_upload(const std::vector<uint8_t>& active, uint32_t tiles_x, uint32_t tiles_y)
{
    std::vector<uint32_t> list;
    list.reserve(active.size());
    const uint32_t c = tiles_y >> 1;
    for (uint32_t rr = 0; rr < 2u * tiles_y + 1u; ++rr) {
        const uint32_t off = (rr + 1u) >> 1;
        if ((rr & 1u) ? off > c : c + off >= tiles_y) continue;
        const uint32_t ty = (rr & 1u) ? c - off : c + off;
        for (uint32_t tx = 0; tx < tiles_x; ++tx)
            if (active[(size_t)ty * tiles_x + tx]) list.push_back(tx | ty << 16);
    }
    for (auto& st : g.sets) if (st.stream) HIP_TRY(hipStreamSynchronize(st.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    if (!list.empty()) HIP_TRY(hipMemcpyAsync(g.d_ad_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, g.stream));
    HIP_TRY(hipMemcpyAsync(g.d_ad_map, active.data(), active.size(), hipMemcpyHostToDevice, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    g.ad_len = (uint32_t)list.size();
    return 0;
}

} // namespace

namespace svr_host {

// filter a whole W x H accumulator with the current scene's guides: tone-mapped into img, or (img null) into hdr_out
int denoise_frame(void* img, float* hdr_out, const void* hdr, uint32_t W, uint32_t H, const svr_denoise_params& p, bool soft, bool& ok)
{
    ok = true;
    if (W != g.cam.imageW || H != g.cam.imageH)
        return fail(-4, "denoise: the frame (%u x %u) must have the image size of the current camera (%u x %u)", W, H, g.cam.imageW, g.cam.imageH);
    if (ensure_guides(p, soft, ok) || !ok) return g.err_code;
    svr::DenoiseArgs a;
    a.W = W; a.H = H;
    a.passes = p.passes;
    a.sigma_depth = p.sigma_depth; a.sigma_normal = p.sigma_normal; a.sigma_albedo = p.sigma_albedo;
    a.sigma_opacity = p.sigma_opacity; a.sigma_color = p.sigma_color;
    a.pix_scale = H > 1 ? 2.f * g.cam.tanFovxOverTwo / (float)(H - 1) : 2.f * g.cam.tanFovxOverTwo;
    a.exposure = g.cam.exposure;
    HIP_TRY(svr::launch_denoise((const float*)hdr, g.d_guides, g.d_dn_scratch, (uint8_t*)img, hdr_out, a, g.stream));
    return 0;
}

// the state rules of SVR_OPT_NOISE_ESTIMATE, behind a render call of rp that ended at n = frameNo + nframes (render call number `call`):
// a new render (frameNo 0, a gap in the frame numbers or the calls, another accumulator / size / shape / depth) resets; the first call
// that ends at n >= 4 takes the snapshot A(m), m = n; after that every call that ends at n >= 2m runs the fused estimate + snapshot, m = n.
// All on the caller's stream behind the resolve / fold that wrote A(n); nothing waits for the host.
int noise_after_render(const svr_render_params* rp, uint32_t nframes, uint64_t call)
{
    Context::Noise& ns = g.ns;
    const uint64_t n64 = (uint64_t)rp->frameNo + nframes;
    if (!noise_continues(rp, call)) {
        ns.tracking = true;
        ns.unavailable = false;
        ns.m = 0;
        ns.have = false;
        ns.hdr = rp->hdrBuffer;
        ns.W = g.cam.imageW; ns.H = g.cam.imageH;
        ns.depth = rp->traceDepth;
        fill_work(ns.shape, ns.W, ns.H);
    }
    ns.call = call;
    if (n64 > 0xffffffffull) { ns.tracking = false; return 0; }
    const uint32_t n = (uint32_t)n64;
    ns.last_n = n;
    if (ns.unavailable) return 0;
    const size_t px = (size_t)ns.W * ns.H;
    if (ns.m == 0) {
        if (n < 4) return 0;
        bool ok = true;
        if (ensure_noise_snap(px, true, ok)) return g.err_code;
        if (!ok) { ns.unavailable = true; return 0; }
        HIP_TRY(hipMemcpyAsync(ns.d_snap, rp->hdrBuffer, px * 3 * sizeof(float), hipMemcpyDeviceToDevice, g.stream));
        ns.m = n;
        return 0;
    }
    if ((uint64_t)n < 2ull * ns.m) return 0;
    const svr::NoiseArgs a = noise_args(ns.W, ns.H, ns.shape, ns.m, n, g.cam.exposure);
    bool ok = true;
    if (ensure_noise_buf(ns.buf, (size_t)a.tiles_x * a.tiles_y, true, ok)) return g.err_code;
    if (!ok) { ns.unavailable = true; ns.have = false; return 0; }
    HIP_TRY(svr::launch_noise(ns.d_snap, (const float*)rp->hdrBuffer, true, a, ns.buf.rmse(), ns.buf.sse(), ns.buf.cnt(), ns.buf.totals(), g.stream));
    ns.have = true;
    ns.est_m = ns.m; ns.est_n = n;
    ns.tiles_x = a.tiles_x; ns.tiles_y = a.tiles_y;
    ns.m = n;
    return 0;
}

} // namespace svr_host

extern "C" {

// ---------------- noise estimate ----------------
// is [p, p + bytes) inside one device allocation?
static bool device_range_ok(const void* p, size_t bytes)
{
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)const_cast<void*>(p)) != hipSuccess) { (void)hipGetLastError(); return false; }
    return (const char*)p + bytes <= (const char*)base + size;
}

int svr_get_noise_estimate(svr_noise_estimate* out, float* tile_rmse_device)
{
    if (ensure_init()) return g.err_code;
    if (!out) return fail(-4, "svr_get_noise_estimate: out is null");
    memset(out, 0, sizeof *out);
    out->rmse = out->tile_max = std::nanf("");
    const Context::Noise& ns = g.ns;
    if (!ns.have) return 0;
    if (tile_rmse_device) {
        // the estimate is the library's (the render it last followed): its map may be larger than the caller expects
        const size_t bytes = sizeof(float) * ns.tiles_x * ns.tiles_y;
        if (!device_range_ok(tile_rmse_device, bytes))
            return fail(-4, "svr_get_noise_estimate: the tile map must be a device buffer of %u x %u floats (the estimate's tiles_x x tiles_y)",
                        ns.tiles_x, ns.tiles_y);
        HIP_TRY(hipMemcpyAsync(tile_rmse_device, ns.buf.rmse(), bytes, hipMemcpyDeviceToDevice, g.stream));
    }
    svr::NoiseTotals t;
    HIP_TRY(hipMemcpyAsync(&t, ns.buf.totals(), sizeof t, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    noise_fill(*out, t, ns.est_m, ns.est_n, ns.tiles_x, ns.tiles_y);
    return 0;
}

int svr_estimate_noise(const void* hdr_m, uint32_t m, const void* hdr_n, uint32_t n, uint32_t w, uint32_t h, float* tile_rmse_device,
                       svr_noise_estimate* out)
{
    if (ensure_init()) return g.err_code;
    if (!hdr_m || !hdr_n || !out) return fail(-4, "svr_estimate_noise: null argument");
    if (m == 0 || m >= n) return fail(-6, "svr_estimate_noise: the frame counts must satisfy 0 < m < n (got m = %u, n = %u)", m, n);
    if (w == 0 || h == 0 || (size_t)3 * w * h >= ((size_t)1 << 32)) return fail(-4, "svr_estimate_noise: bad frame size %u x %u", w, h);
    if (!g.have_cam) return fail(-4, "svr_estimate_noise before setup_camera (the exposure comes from the camera)");
    const size_t bytes = sizeof(float) * 3 * (size_t)w * h;
    const uint32_t tx = (w + svr::NOISE_TILE - 1u) / svr::NOISE_TILE, ty = (h + svr::NOISE_TILE - 1u) / svr::NOISE_TILE;
    if (!device_range_ok(hdr_m, bytes) || !device_range_ok(hdr_n, bytes))
        return fail(-4, "svr_estimate_noise: the accumulators must be device buffers of %u x %u x 3 floats", w, h);
    if (tile_rmse_device && !device_range_ok(tile_rmse_device, sizeof(float) * tx * ty))
        return fail(-4, "svr_estimate_noise: the tile map must be a device buffer of %u x %u floats", tx, ty);
    bool ok = true;
    if (ensure_noise_buf(g.nb_call, (size_t)tx * ty, false, ok)) return g.err_code;
    svr::DevWork full;
    fill_work_full(full, w, h);
    const svr::NoiseArgs a = noise_args(w, h, full, m, n, g.cam.exposure);
    HIP_TRY(svr::launch_noise((float*)const_cast<void*>(hdr_m), (const float*)hdr_n, false, a, tile_rmse_device ? tile_rmse_device : g.nb_call.rmse(),
                              g.nb_call.sse(), g.nb_call.cnt(), g.nb_call.totals(), g.stream));
    svr::NoiseTotals t;
    HIP_TRY(hipMemcpyAsync(&t, g.nb_call.totals(), sizeof t, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    noise_fill(*out, t, m, n, tx, ty);
    return 0;
}

int svr_render_pathtracer_until(void* img, svr_render_params* rp, float target_rmse, float target_tile_rmse, uint32_t max_frames,
                                uint32_t* frames_done)
{
    if (ensure_init()) return g.err_code;
    if (!img || !rp) return fail(-4, "svr_render_pathtracer_until: null argument");
    if (!(target_rmse >= 0.f) || !(target_tile_rmse >= 0.f))
        return fail(-6, "svr_render_pathtracer_until: the targets must be >= 0 (got %g, %g)", (double)target_rmse, (double)target_tile_rmse);
    if (max_frames == 0) return fail(-6, "svr_render_pathtracer_until: max_frames must be > 0");
    if ((uint64_t)rp->frameNo + max_frames > 0xffffffffull) return fail(-6, "svr_render_pathtracer_until: frameNo + max_frames exceeds 2^32 - 1");
    if (frames_done) *frames_done = 0;
    const uint32_t f0 = rp->frameNo;
    const bool check = target_rmse > 0.f || target_tile_rmse > 0.f;
    const int opt = g.opt_noise_estimate;
    g.opt_noise_estimate = 1;                    // the estimator for the call's own duration
    uint32_t done = 0;
    int rc = 0;
    while (done < max_frames) {
        svr_render_params cur = *rp;
        cur.frameNo = f0 + done;
        // the next checkpoint of the state rules: the snapshot (n >= 4) of a new render, else n = 2m
        const bool cont = noise_continues(&cur, g.render_calls + 1);
        uint64_t next = (uint64_t)f0 + max_frames;
        if (check && !(cont && g.ns.unavailable)) {
            if (cont && g.ns.m > 0) next = 2ull * g.ns.m;
            else next = cur.frameNo + 1u > 4u ? cur.frameNo + 1u : 4u;
        }
        const uint32_t chunk = (uint32_t)std::min<uint64_t>(next - cur.frameNo, max_frames - done);
        if ((rc = render_frames(img, &cur, chunk, true)) != 0) break;
        done += chunk;
        if (!check || !g.ns.have || g.ns.est_n != f0 + done) continue;
        svr_noise_estimate e;
        if ((rc = svr_get_noise_estimate(&e, nullptr)) != 0) break;
        if ((target_rmse == 0.f || e.rmse <= target_rmse) && (target_tile_rmse == 0.f || e.tile_max <= target_tile_rmse)) break;
    }
    g.opt_noise_estimate = opt;
    rp->frameNo = f0 + done;
    if (frames_done) *frames_done = done;
    return rc;
}

// ---------------- adaptive sampling ----------------
int svr_render_pathtracer_adaptive(void* img, svr_render_params* rp, float target_tile_rmse, uint32_t min_frames, uint32_t max_frames,
                                   svr_adaptive_result* out)
{
    if (ensure_init()) return g.err_code;
    if (!img || !rp || !out) return fail(-4, "svr_render_pathtracer_adaptive: null argument");
    if (!(target_tile_rmse > 0.f) || !std::isfinite(target_tile_rmse))
        return fail(-6, "svr_render_pathtracer_adaptive: target_tile_rmse must be > 0 and finite (got %g)", (double)target_tile_rmse);
    if (max_frames == 0) return fail(-6, "svr_render_pathtracer_adaptive: max_frames must be > 0");
    if ((uint64_t)rp->frameNo + max_frames > 0xffffffffull) return fail(-6, "svr_render_pathtracer_adaptive: frameNo + max_frames exceeds 2^32 - 1");
    if (!g.have_vol || !g.have_tf || !g.have_cam) return fail(-4, "svr_render_pathtracer_adaptive before setup_volume/setup_transferfunction/setup_camera");
    if (!rp->hdrBuffer) return fail(-4, "svr_render_pathtracer_adaptive: renderParams.hdrBuffer is null (call SetupHDRBuffer)");
    const uint32_t W = g.cam.imageW, H = g.cam.imageH;
    if (g.world > 1 || partial_frame(W, H))
        return fail(-6, "svr_render_pathtracer_adaptive: the whole frame on one process only (a row shard or a render window is set)");
    if (g.opt_kernel == svr::KERNEL_PIXEL || g.opt_kernel == svr::KERNEL_ULOOP || g.opt_kernel == svr::KERNEL_WAVEFRONT)
        return fail(-6, "svr_render_pathtracer_adaptive: SVR_OPT_KERNEL %d does not trace tile lists (0 / 2 do)", g.opt_kernel);
    if (g.opt_fast_math) return fail(-6, "svr_render_pathtracer_adaptive: the fast-math build (SVR_OPT_FAST_MATH) does not trace tile lists");
    if ((size_t)3 * W * H >= ((size_t)1 << 32)) return fail(-3, "image too large");

    const uint32_t tiles_x = (W + svr::NOISE_TILE - 1u) / svr::NOISE_TILE, tiles_y = (H + svr::NOISE_TILE - 1u) / svr::NOISE_TILE;
    const size_t nt = (size_t)tiles_x * tiles_y, px = (size_t)W * H;
    // memory: the tile list + map, and the estimator's snapshot and tile buffers (the call leaves the estimator without a render anyway)
    if (g.ad_cap < nt) {
        if (g.d_ad_list) HIP_TRY(hipFree(g.d_ad_list));
        g.d_ad_list = nullptr; g.d_ad_map = nullptr; g.ad_cap = 0;
        HIP_TRY(hipMalloc((void**)&g.d_ad_list, nt * (sizeof(uint32_t) + 1u)));
        g.d_ad_map = (uint8_t*)(g.d_ad_list + nt);
        g.ad_cap = nt;
    }
    Context::Noise& ns = g.ns;
    ns.tracking = false; ns.have = false; ns.m = 0;
    ++g.render_calls;                            // (the next render call starts a new render by the estimator's state rules)
    bool ok = true;
    if (ensure_noise_snap(px, false, ok) || ensure_noise_buf(ns.buf, nt, false, ok)) return g.err_code;

    const uint32_t f0 = rp->frameNo;
    const uint64_t end = (uint64_t)f0 + max_frames;
    const uint32_t snap_at = f0 + 1u > 4u ? f0 + 1u : 4u;
    std::vector<uint32_t> frames(nt, f0), est_n(nt, 0u);
    std::vector<uint8_t> active(nt, 1u), below_prev(nt, 0u);
    std::vector<float> trmse(nt, std::nanf(""));
    size_t n_active = nt;
    uint32_t n = f0, m = 0, checkpoints = 0;
    bool list_mode = false;
    int rc = 0;
    for (;;) {
        uint64_t next = m == 0 ? (uint64_t)snap_at : 2ull * m;
        const bool checkpoint = next <= end;
        if (!checkpoint) next = end;
        // frames n .. next - 1 of the active tiles (all of them until the first freeze: the ordinary launches)
        svr_render_params cur = *rp;
        cur.frameNo = n;
        const TileList tiles = {list_mode ? g.d_ad_list : nullptr, g.ad_len, g.d_ad_map};
        if ((rc = render_frames_traced(img, &cur, (uint32_t)(next - n), false, &tiles))) break;
        n = (uint32_t)next;
        for (size_t t = 0; t < nt; ++t) if (active[t]) frames[t] = n;
        if (!checkpoint) break;
        bool changed = false;
        if (m == 0) {
            if ((rc = hip_check(hipMemcpyAsync(ns.d_snap, rp->hdrBuffer, px * 3 * sizeof(float), hipMemcpyDeviceToDevice, g.stream)))) break;
        } else {
            // the masked estimate of A(n) against A(m) + the snapshot, for the active tiles (the frozen ones keep theirs), then the freeze rule
            svr::DevWork full;
            fill_work_full(full, W, H);
            const svr::NoiseArgs a = noise_args(W, H, full, m, n, g.cam.exposure);
            if ((rc = hip_check(svr::launch_noise(ns.d_snap, (const float*)rp->hdrBuffer, true, a, ns.buf.rmse(), ns.buf.sse(), ns.buf.cnt(),
                                                  ns.buf.totals(), g.stream, list_mode ? g.d_ad_map : nullptr)))) break;
            std::vector<float> r(nt);
            if ((rc = hip_check(hipMemcpyAsync(r.data(), ns.buf.rmse(), nt * sizeof(float), hipMemcpyDeviceToHost, g.stream)))) break;
            if ((rc = hip_check(hipStreamSynchronize(g.stream)))) break;
            ++checkpoints;
            for (size_t t = 0; t < nt; ++t) {
                if (!active[t]) continue;
                trmse[t] = r[t];
                est_n[t] = n;
                const bool below = !(r[t] > target_tile_rmse);        // (NaN: a tile without a counted pixel counts as below)
                if (n >= min_frames && below && below_prev[t]) { active[t] = 0u; --n_active; changed = true; }
                below_prev[t] = below ? 1u : 0u;
            }
        }
        m = n;
        if (n_active == 0 || n >= end) break;
        if (changed) {
            if ((rc = adaptive_upload(active, tiles_x, tiles_y))) break;
            list_mode = true;
        }
    }
    if (rc) return rc;

    // the result: frozen tiles keep the estimate they froze with, active ones scale their last one to the final frame count
    svr_adaptive_result res;
    memset(&res, 0, sizeof res);
    res.tiles_x = tiles_x; res.tiles_y = tiles_y;
    res.tiles_active = (uint32_t)n_active;
    res.checkpoints = checkpoints;
    res.frames_min = 0xffffffffu;
    std::vector<double> sse(nt, 0.0);
    std::vector<uint32_t> cnt(2 * nt, 0u);
    if (checkpoints) {
        HIP_TRY(hipMemcpyAsync(sse.data(), ns.buf.sse(), nt * sizeof(double), hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipMemcpyAsync(cnt.data(), ns.buf.cnt(), 2 * nt * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
    }
    HIP_TRY(hipStreamSynchronize(g.stream));
    float tile_max = -1.f;
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) {
            const size_t t = (size_t)ty * tiles_x + tx;
            res.frames_max = std::max(res.frames_max, frames[t]);
            res.frames_min = std::min(res.frames_min, frames[t]);
            const uint64_t tp = (uint64_t)std::min(svr::NOISE_TILE, W - tx * svr::NOISE_TILE) * std::min(svr::NOISE_TILE, H - ty * svr::NOISE_TILE);
            res.pixel_frames += tp * (frames[t] - f0);
            if (est_n[t] == 0) { trmse[t] = std::nanf(""); continue; }
            const double scale = (double)est_n[t] / (double)frames[t];
            res.sse += sse[t] * scale;
            res.pixels += cnt[2 * t];
            res.nonfinite += cnt[2 * t + 1];
            trmse[t] = cnt[2 * t] ? (float)((double)trmse[t] * std::sqrt(scale)) : std::nanf("");
            if (cnt[2 * t]) tile_max = std::max(tile_max, trmse[t]);
        }
    res.rmse = res.pixels ? (float)std::sqrt(res.sse / (double)res.pixels) : std::nanf("");
    res.tile_max = tile_max < 0.f ? std::nanf("") : tile_max;
    g.ad_have = true;
    g.ad_tx = tiles_x; g.ad_ty = tiles_y;
    g.ad_frames = frames;
    g.ad_rmse = trmse;

    // the image: the tone map of the final accumulator (or the denoised preview while the render has at most SVR_OPT_DENOISE_PREVIEW frames)
    if (!g.opt_skip_tonemap && show_full_frame(img, rp->hdrBuffer, g.opt_denoise_preview > 0 && res.frames_max <= (uint32_t)g.opt_denoise_preview))
        return g.err_code;
    rp->frameNo = res.frames_max;
    *out = res;
    return 0;
}

int svr_get_adaptive_tiles(uint32_t* tile_frames_device, float* tile_rmse_device)
{
    if (ensure_init()) return g.err_code;
    if (!g.ad_have) return fail(-4, "svr_get_adaptive_tiles before any svr_render_pathtracer_adaptive call");
    const size_t nt = (size_t)g.ad_tx * g.ad_ty;
    if (tile_frames_device && !device_range_ok(tile_frames_device, nt * sizeof(uint32_t)))
        return fail(-4, "svr_get_adaptive_tiles: the frame map must be a device buffer of %u x %u uint32", g.ad_tx, g.ad_ty);
    if (tile_rmse_device && !device_range_ok(tile_rmse_device, nt * sizeof(float)))
        return fail(-4, "svr_get_adaptive_tiles: the RMSE map must be a device buffer of %u x %u floats", g.ad_tx, g.ad_ty);
    if (tile_frames_device) HIP_TRY(hipMemcpyAsync(tile_frames_device, g.ad_frames.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice, g.stream));
    if (tile_rmse_device) HIP_TRY(hipMemcpyAsync(tile_rmse_device, g.ad_rmse.data(), nt * sizeof(float), hipMemcpyHostToDevice, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return 0;
}

// ---------------- denoised preview ----------------
int svr_denoise_params_default(svr_denoise_params* p)
{
    if (!p) return fail(-4, "svr_denoise_params_default: null argument");
    *p = DN_DEFAULT;
    return 0;
}

int svr_set_denoise_params(const svr_denoise_params* p)
{
    if (!p) return fail(-4, "svr_set_denoise_params: null argument");
    if (check_denoise_params(*p)) return g.err_code;
    g.dn = *p;
    return 0;
}

int svr_get_denoise_params(svr_denoise_params* p)
{
    if (!p) return fail(-4, "svr_get_denoise_params: null argument");
    *p = g.dn;
    return 0;
}

int svr_render_guides(void* guides)
{
    if (ensure_init()) return g.err_code;
    if (!guides) return fail(-4, "svr_render_guides: null argument");
    if (!g.have_vol || !g.have_tf || !g.have_cam) return fail(-4, "svr_render_guides before setup_volume/setup_transferfunction/setup_camera");
    bool ok = true;
    if (ensure_guides(g.dn, false, ok)) return g.err_code;
    HIP_TRY(hipMemcpyAsync(guides, g.d_guides, (size_t)g.cam.imageW * g.cam.imageH * 2 * sizeof(float4), hipMemcpyDeviceToDevice, g.stream));
    return 0;
}

uint64_t svr_guide_builds(void) { return g.guide_builds; }

static int denoise_call(void* img, void* hdr_out, const void* hdr, uint32_t w, uint32_t h, const svr_denoise_params* p, const char* who)
{
    if (ensure_init()) return g.err_code;
    if (!hdr || (!img && !hdr_out) || w == 0 || h == 0) return fail(-4, "%s: bad argument", who);
    if (!g.have_vol || !g.have_tf || !g.have_cam) return fail(-4, "%s before setup_volume/setup_transferfunction/setup_camera", who);
    const svr_denoise_params prm = p ? *p : g.dn;
    if (check_denoise_params(prm)) return g.err_code;
    bool ok = true;
    return denoise_frame(img, (float*)hdr_out, hdr, w, h, prm, false, ok);
}

int svr_denoise_to_ldr(void* img, const void* hdr, uint32_t w, uint32_t h, const svr_denoise_params* p)
{
    if (!img) { ensure_init(); return fail(-4, "svr_denoise_to_ldr: img is null"); }
    return denoise_call(img, nullptr, hdr, w, h, p, "svr_denoise_to_ldr");
}

int svr_denoise_hdr(void* out, const void* hdr, uint32_t w, uint32_t h, const svr_denoise_params* p)
{
    if (!out) { ensure_init(); return fail(-4, "svr_denoise_hdr: out is null"); }
    return denoise_call(nullptr, out, hdr, w, h, p, "svr_denoise_hdr");
}

} // extern "C"
