// svr_api_views.hip -- the image calls of the C-ABI layer (svr_api.hip) that march the camera's rays or a plane through the volume: the
// ray caster, the projection modes, slice views, hit maps and picks.
#include "svr_api_state.hpp"
#include "svr_project.hpp"
#include "svr_slice.hpp"
#include "svr_hits.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace svr_host;

extern "C" {

void render_raycasting(void* img, svr_volume* volume, svr_transfer_function* transferFunction, svr_camera* camera, float stepSize)
{
    if (ensure_init()) return;
    if (!img || !volume || !transferFunction || !camera) { fail(-4, "render_raycasting: null argument"); return; }
    if (check_step("render_raycasting", stepSize)) return;
    svr::DevScene s;
    svr::DevWork w;
    if (image_scene(*volume, *transferFunction, *camera, img, s, w)) return;
    if (ensure_mask(s, *volume, *transferFunction)) return;
    hipError_t e = svr::launch_raycast(s, w, stepSize, g.opt_count != 0, g.num_cus, g.opt_rc_lanes, g.stream);
    if (e != hipSuccess) fail((int)e, "render_raycasting launch failed: %s", hipGetErrorName(e));
}

// ---------------- projection modes of the ray caster (svr_project.hip) ----------------
int svr_projection_params_default(svr_projection_params* p)
{
    if (!p) return fail(-4, "svr_projection_params_default: null argument");
    p->mode = SVR_PROJ_MIP; p->flags = 0u; p->iso = 0.5f; p->window_lo = 0.f; p->window_hi = 1.f;
    return 0;
}

int svr_render_projection(void* img, const svr_volume* volume, const svr_transfer_function* tf, const svr_camera* camera, float stepSize,
                          const svr_projection_params* p)
{
    if (ensure_init()) return g.err_code;
    if (!img || !volume || !tf || !camera || !p) return fail(-4, "svr_render_projection: null argument");
    if (p->mode != SVR_PROJ_MIP && p->mode != SVR_PROJ_MEAN && p->mode != SVR_PROJ_ISO) return fail(-3, "svr_render_projection: unknown mode %d", (int)p->mode);
    if (p->flags & ~SVR_PROJ_COLOR_TF) return fail(-3, "svr_render_projection: unknown flags 0x%x", (unsigned)p->flags);
    if (int e = check_step("svr_render_projection", stepSize)) return e;
    if (!std::isfinite(p->iso)) return fail(-3, "svr_render_projection: iso must be finite");
    if (int e = check_window("svr_render_projection", p->window_lo, p->window_hi)) return e;
    if (int e = check_density_scale("svr_render_projection", volume->densityScale)) return e;
    svr::DevScene s;
    svr::DevWork w;
    if (int e = image_scene(*volume, *tf, *camera, img, s, w)) return e;
    svr::DevProjection pj;
    memset(&pj, 0, sizeof pj);
    pj.mode = p->mode; pj.flags = p->flags; pj.iso = p->iso; pj.window_lo = p->window_lo; pj.window_hi = p->window_hi;
    Texture* tv = find_tex(volume->tex, TEX_VOLUME);
    if (g.opt_empty_skip && tv && tv->mm) {
        if (int e = fill_march_tables("svr_render_projection", s, *volume, tv, pj.tb)) return e;
        // MEAN skips only samples whose eight voxels are 0.  A volume without a macro-cell whose neighbourhood is all zero (noisy air)
        // has next to nothing to skip and nothing to leap over, and the per-sample test then only costs (c3n: 2.5 ms against 1.6 ms,
        // DESIGN.md 8e): such volumes are rendered without the test
        if (pj.mode == SVR_PROJ_MEAN && (!pj.tb.leap || tv->nb_zero == 0u)) pj.tb.mm = nullptr;
    }
    hipError_t e = svr::launch_projection(s, w, pj, stepSize, g.opt_count != 0, g.num_cus, g.stream);
    if (e != hipSuccess) return fail((int)e, "svr_render_projection launch failed: %s", hipGetErrorName(e));
    return 0;
}

// ---------------- slice views (svr_slice.hip) ----------------
int svr_slice_params_default(svr_slice_params* p)
{
    if (!p) return fail(-4, "svr_slice_params_default: null argument");
    memset(p, 0, sizeof *p);
    p->u.x = 1.f; p->v.y = 1.f;
    p->step = 1.f; p->mode = SVR_SLAB_MIP; p->window_lo = 0.f; p->window_hi = 1.f;
    return 0;
}

// the box volume.Intersect clips to (build_scene's clip_vmin / clip_vmax, ordered)
static void slice_box(const svr_volume& vol, float lo[3], float hi[3])
{
    const float e0[3] = {vol.bbox.vmin.x * (-vol.x_clip.x), vol.bbox.vmin.y * (-vol.y_clip.x), vol.bbox.vmin.z * (-vol.z_clip.x)};
    const float e1[3] = {vol.bbox.vmax.x * vol.x_clip.y, vol.bbox.vmax.y * vol.y_clip.y, vol.bbox.vmax.z * vol.z_clip.y};
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(e0[a], e1[a]); hi[a] = std::max(e0[a], e1[a]); }
}

int svr_slice_params_axis(svr_slice_params* p, const svr_volume* volume, int axis, float position, uint32_t w, uint32_t h)
{
    if (!p || !volume) return fail(-4, "svr_slice_params_axis: null argument");
    if (axis < 0 || axis > 2) return fail(-3, "svr_slice_params_axis: axis must be 0, 1 or 2 (got %d)", axis);
    if (!(position >= 0.f && position <= 1.f)) return fail(-3, "svr_slice_params_axis: position must lie in [0, 1] (got %g)", (double)position);
    if (w == 0 || h == 0) return fail(-3, "svr_slice_params_axis: image size is zero");
    float lo[3], hi[3];
    slice_box(*volume, lo, hi);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || !(hi[a] > lo[a])) return fail(-3, "svr_slice_params_axis: the clipped box is not finite or has no extent");
    // image right / down: +y / -z, +x / -z, +x / -y
    const int ar = axis == 0 ? 1 : 0, ad = axis == 2 ? 1 : 2;
    const float px = std::max((hi[ar] - lo[ar]) / (float)w, (hi[ad] - lo[ad]) / (float)h);
    float c[3], u[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f};
    for (int a = 0; a < 3; ++a) c[a] = 0.5f * (lo[a] + hi[a]);
    c[axis] = position == 1.f ? hi[axis] : lo[axis] + position * (hi[axis] - lo[axis]);
    c[axis] = std::min(std::max(c[axis], lo[axis]), hi[axis]);
    u[ar] = px; v[ad] = -px;
    svr_slice_params_default(p);
    p->center.x = c[0]; p->center.y = c[1]; p->center.z = c[2];
    p->u.x = u[0]; p->u.y = u[1]; p->u.z = u[2];
    p->v.x = v[0]; p->v.y = v[1]; p->v.z = v[2];
    p->step = px;
    return 0;
}

int svr_render_slice_stack(void* imgs, const svr_volume* volume, const svr_transfer_function* tf, uint32_t w, uint32_t h,
                           const svr_slice_params* p, uint32_t count, float spacing)
{
    if (ensure_init()) return g.err_code;
    if (!imgs || !volume || !tf || !p) return fail(-4, "svr_render_slice: null argument");
    if (w == 0 || h == 0) return fail(-3, "svr_render_slice: image size is zero");
    if (count == 0) return fail(-3, "svr_render_slice_stack: count is zero");
    if (!finite3(p->center) || !finite3(p->u) || !finite3(p->v) || !std::isfinite(p->thickness) || !std::isfinite(p->step) || !std::isfinite(spacing))
        return fail(-3, "svr_render_slice: center, u, v, thickness, step and spacing must be finite");
    if (p->flags & ~SVR_SLICE_COLOR_TF) return fail(-3, "svr_render_slice: unknown flags 0x%x", (unsigned)p->flags);
    if (int e = check_window("svr_render_slice", p->window_lo, p->window_hi)) return e;
    if (p->thickness < 0.f) return fail(-3, "svr_render_slice: thickness must be >= 0 (got %g)", (double)p->thickness);
    svr::DevSlice sl;
    memset(&sl, 0, sizeof sl);
    sl.K = 1u; sl.mode = svr::SLICE_PLANE;
    if (p->thickness > 0.f) {
        if (!(p->step > 0.f)) return fail(-3, "svr_render_slice: a slab needs step > 0 (got %g)", (double)p->step);
        if (p->mode != SVR_SLAB_MIP && p->mode != SVR_SLAB_MINIP && p->mode != SVR_SLAB_MEAN) return fail(-3, "svr_render_slice: unknown slab mode %d", (int)p->mode);
        const float q = std::floor(p->thickness / p->step);
        if (!(q < (float)SVR_SLICE_MAX_SAMPLES)) return fail(-3, "svr_render_slice: thickness / step gives more than %d samples", SVR_SLICE_MAX_SAMPLES);
        sl.K = (uint32_t)q + 1u;
        sl.mode = p->mode;
        sl.step = p->step;
        sl.half_thickness = 0.5f * p->thickness;
    }
    if (int e = check_density_scale("svr_render_slice", volume->densityScale)) return e;
    // n = normalize(cross(u, v)), the operations the header names (this file is compiled without contraction)
    const float crx = p->u.y * p->v.z - p->u.z * p->v.y, cry = p->u.z * p->v.x - p->u.x * p->v.z, crz = p->u.x * p->v.y - p->u.y * p->v.x;
    const float len2 = (crx * crx + cry * cry) + crz * crz;
    const float inv = 1.f / std::sqrt(len2);
    if (!(len2 > 0.f) || !std::isfinite(inv) || !std::isfinite(crx * inv) || !std::isfinite(cry * inv) || !std::isfinite(crz * inv))
        return fail(-3, "svr_render_slice: cross(u, v) has no length (u and v must span a plane)");
    const uint64_t n_tasks = (uint64_t)((w + 7u) >> 3) * ((h + 7u) >> 3) * count;
    if (n_tasks > 0xffffffffull - svr::TICKET_SHARDS) return fail(-3, "svr_render_slice_stack: %u slices of %u x %u are more than 2^32 - 1 tile tasks", count, w, h);
    svr_camera cam;
    memset(&cam, 0, sizeof cam);
    cam.imageW = w; cam.imageH = h;
    svr::DevScene s;
    svr::DevWork wk;
    if (int e = image_scene(*volume, *tf, cam, imgs, s, wk)) return e;
    sl.center[0] = p->center.x; sl.center[1] = p->center.y; sl.center[2] = p->center.z;
    sl.u[0] = p->u.x; sl.u[1] = p->u.y; sl.u[2] = p->u.z;
    sl.v[0] = p->v.x; sl.v[1] = p->v.y; sl.v[2] = p->v.z;
    sl.n[0] = crx * inv; sl.n[1] = cry * inv; sl.n[2] = crz * inv;
    slice_box(*volume, sl.box_lo, sl.box_hi);
    sl.spacing = spacing; sl.count = count;
    sl.flags = p->flags; sl.window_lo = p->window_lo; sl.window_hi = p->window_hi;
    sl.counting = g.opt_count != 0 ? 1u : 0u;
    Texture* tv = find_tex(volume->tex, TEX_VOLUME);
    // A single plane is rendered without the skipping test: the test is a dependent table load per pixel that can save one fetch at most
    // (measured equal with and without it).  So is slab MEAN: its test only finds exactly empty macro-cells, and it lost on every scene
    // and thickness measured (c3, 256 samples: 0.665 ms against 0.625 ms; c3n: 0.90 against 0.63).  MIP and MINIP keep it
    if (g.opt_empty_skip && sl.K > 1u && sl.mode != svr::SLAB_MEAN && tv && tv->mm) {
        sl.mm = tv->mm;
        use_macro_grid(s, tv);
    }
    hipError_t e = svr::launch_slice(s, wk, sl, g.num_cus, g.stream);
    if (e != hipSuccess) return fail((int)e, "svr_render_slice launch failed: %s", hipGetErrorName(e));
    return 0;
}

int svr_render_slice(void* img, const svr_volume* volume, const svr_transfer_function* tf, uint32_t w, uint32_t h, const svr_slice_params* p)
{
    return svr_render_slice_stack(img, volume, tf, w, h, p, 1u, 0.f);
}

int svr_slice_params_through(svr_slice_params* p, const svr_volume* volume, int axis, const svr_vec3* point, uint32_t w, uint32_t h)
{
    if (!p || !volume || !point) return fail(-4, "svr_slice_params_through: null argument");
    if (axis < 0 || axis > 2) return fail(-3, "svr_slice_params_through: axis must be 0, 1 or 2 (got %d)", axis);
    if (!finite3(*point)) return fail(-3, "svr_slice_params_through: the point is not finite");
    svr_slice_params q;
    if (int e = svr_slice_params_axis(&q, volume, axis, 0.5f, w, h)) return e;
    float lo[3], hi[3];
    slice_box(*volume, lo, hi);
    const float c = axis == 0 ? point->x : axis == 1 ? point->y : point->z;
    if (!(c >= lo[axis] && c <= hi[axis]))
        return fail(-3, "svr_slice_params_through: the point (%g on axis %d) lies outside the clipped box (%g .. %g)", (double)c, axis, (double)lo[axis], (double)hi[axis]);
    (axis == 0 ? q.center.x : axis == 1 ? q.center.y : q.center.z) = c;
    *p = q;
    return 0;
}

// ---------------- hit maps and picks (svr_hits.hip) ----------------
int svr_hit_params_default(svr_hit_params* p)
{
    if (!p) return fail(-4, "svr_hit_params_default: null argument");
    p->mode = SVR_HIT_OPACITY; p->alpha = 0.5f; p->iso = 0.5f;
    return 0;
}

// svr_render_hits (pixels_xy null) and svr_pick
static int hits_call(const char* who, void* hits, const uint32_t* pixels_xy, uint32_t n, const svr_volume* volume, const svr_transfer_function* tf,
                     const svr_camera* camera, float stepSize, const svr_hit_params* p)
{
    if (ensure_init()) return g.err_code;
    if (!hits || !volume || !tf || !camera || !p) return fail(-4, "%s: null argument", who);
    if (p->mode != SVR_HIT_OPACITY && p->mode != SVR_HIT_ISO && p->mode != SVR_HIT_MAX) return fail(-3, "%s: unknown mode %d", who, (int)p->mode);
    if (int e = check_step(who, stepSize)) return e;
    if (!std::isfinite(p->iso)) return fail(-3, "%s: iso must be finite", who);
    if (!(p->alpha >= 0.f && p->alpha <= 0.95f)) return fail(-3, "%s: alpha must lie in [0, 0.95] (got %g)", who, (double)p->alpha);
    if (int e = check_density_scale(who, volume->densityScale)) return e;
    svr::DevScene s;
    svr::DevWork w;
    if (int e = image_scene(*volume, *tf, *camera, nullptr, s, w)) return e;
    svr::DevHits hp;
    memset(&hp, 0, sizeof hp);
    hp.mode = p->mode; hp.alpha = p->alpha; hp.iso = p->iso;
    hp.out = (uint32_t*)hits;
    if (pixels_xy) {
        // a pick is a query: the whole image is in reach, whatever shard or window is set
        for (uint32_t i = 0; i < n; ++i)
            if (pixels_xy[2u * i] >= s.imageW || pixels_xy[2u * i + 1u] >= s.imageH)
                return fail(-3, "%s: pixel %u (%u, %u) lies outside the %u x %u image", who, i, pixels_xy[2u * i], pixels_xy[2u * i + 1u], s.imageW, s.imageH);
        fill_work_full(w, s.imageW, s.imageH);
        if (!g.d_pick) HIP_TRY(hipMalloc((void**)&g.d_pick, sizeof(uint32_t) * 2u * SVR_PICK_MAX));
    }
    Texture* tv = find_tex(volume->tex, TEX_VOLUME);
    if (p->mode == SVR_HIT_OPACITY) {
        // k_raycast's mask of the (volume, transfer function) pair: `empty` bits per sample, deep-empty bits for the leaps
        if (int e = ensure_mask(s, *volume, *tf)) return e;
        if (s.empty_mask && tv) {
            hp.tb.empty = s.empty_mask + svr::DIST_WORDS_MAX + svr::MASK_WORDS_MAX;
            hp.tb.deep = s.empty_mask + svr::DIST_WORDS_MAX;
            hp.tb.leap = leaps_allowed(s, *volume, tv, hp.tb.mc_scale) ? 1u : 0u;
        }
    } else if (g.opt_empty_skip && tv && tv->mm) {
        if (int e = fill_march_tables(who, s, *volume, tv, hp.tb)) return e;
    }
    if (pixels_xy) {
        HIP_TRY(hipMemcpyAsync(g.d_pick, pixels_xy, sizeof(uint32_t) * 2u * n, hipMemcpyHostToDevice, g.stream));
        hp.pixels = g.d_pick; hp.n_pick = n;
    }
    hipError_t e = svr::launch_hits(s, w, hp, stepSize, g.opt_count != 0, g.num_cus, g.stream);
    if (e != hipSuccess) return fail((int)e, "%s launch failed: %s", who, hipGetErrorName(e));
    return 0;
}

int svr_render_hits(void* hits, const svr_volume* volume, const svr_transfer_function* tf, const svr_camera* camera, float stepSize, const svr_hit_params* p)
{
    return hits_call("svr_render_hits", hits, nullptr, 0u, volume, tf, camera, stepSize, p);
}

int svr_pick(void* hits, const uint32_t* pixels_xy, uint32_t n, const svr_volume* volume, const svr_transfer_function* tf, const svr_camera* camera,
             float stepSize, const svr_hit_params* p)
{
    if (!pixels_xy) { ensure_init(); return fail(-4, "svr_pick: null argument"); }
    if (n == 0u || n > SVR_PICK_MAX) { ensure_init(); return fail(-3, "svr_pick: n must lie in 1 .. %d (got %u)", SVR_PICK_MAX, n); }
    return hits_call("svr_pick", hits, pixels_xy, n, volume, tf, camera, stepSize, p);
}

} // extern "C"
