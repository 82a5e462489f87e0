// svr_api_scene.hip -- from the scene PODs of the C-ABI layer (svr_api.hip) to what a launch reads: the device scene, the owned pixels
// as its work, and the skipping tables of the current (volume, transfer function) pair.
#include "svr_api_state.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace svr_host;

namespace {

// Can a camera ray (cudaCamera::GenerateRay, core/cuda_camera.h:66-83) reach the disk?  Conservative: true unless the disk's
// bounding sphere lies behind the lens plane or outside the view frustum widened by the lens.  A ray leaves the lens point a
// (|a| <= aperture) towards the image-plane point n at depth f = focalLength; at depth z > 0 its lateral offset is
// a (1 - z / f) + n z / f, with |n_x| <= (1 + 2 / (W - 1)) aspect tan(fov / 2) f (pixel jitter included).
bool light_reachable_by_camera_rays(const svr::DevScene& s, const svr_area_light& l)
{
    const double f = s.focalLength, A = std::fabs((double)s.apeture);
    if (!(f > 0.0) || !std::isfinite(f) || !std::isfinite(A) || s.imageW < 2 || s.imageH < 2) return true;
    const double u[3] = {s.cam_u[0], s.cam_u[1], s.cam_u[2]}, v[3] = {s.cam_v[0], s.cam_v[1], s.cam_v[2]}, w[3] = {s.cam_w[0], s.cam_w[1], s.cam_w[2]};
    auto dot3 = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    // the argument needs an orthonormal camera frame (cudaCamera::Setup builds one); anything else: no culling
    if (std::fabs(dot3(u, u) - 1.0) > 1e-3 || std::fabs(dot3(v, v) - 1.0) > 1e-3 || std::fabs(dot3(w, w) - 1.0) > 1e-3 ||
        std::fabs(dot3(u, v)) > 1e-3 || std::fabs(dot3(u, w)) > 1e-3 || std::fabs(dot3(v, w)) > 1e-3) return true;
    const double c[3] = {(double)l.disk.center.x - s.cam_pos[0], (double)l.disk.center.y - s.cam_pos[1], (double)l.disk.center.z - s.cam_pos[2]};
    const double r = std::fabs((double)l.disk.radius) * 1.01 + 1e-3;
    const double cx = dot3(c, u), cy = dot3(c, v), cz = -dot3(c, w);
    if (!std::isfinite(cx) || !std::isfinite(cy) || !std::isfinite(cz) || !std::isfinite(r)) return true;
    if (cz + r <= 0.0) return false;                                        // behind the lens plane: rays only go forward (dir . -w = f > 0)
    const double z0 = cz - r > 0.0 ? cz - r : 0.0, z1 = cz + r;
    const double k = std::fmax(std::fabs(1.0 - z0 / f), std::fabs(1.0 - z1 / f));
    const double tanh_ = std::fabs((double)s.tanFovxOverTwo);
    const double nx = (1.0 + 2.0 / ((double)s.imageW - 1.0)) * std::fabs((double)s.aspectRatio) * tanh_ * f;
    const double ny = (1.0 + 2.0 / ((double)s.imageH - 1.0)) * tanh_ * f;
    const double bx = (A * k + nx * z1 / f) * 1.01 + 1e-3, by = (A * k + ny * z1 / f) * 1.01 + 1e-3;
    if (!std::isfinite(bx) || !std::isfinite(by)) return true;
    return std::fabs(cx) - r <= bx && std::fabs(cy) - r <= by;
}

} // namespace

namespace svr_host {

// the macro-cell grid of a volume texture (its min/max table, the masks built from it) as the kernels index it
void use_macro_grid(svr::DevScene& s, const Texture* tv)
{
    s.mc_shift = tv->mc_shift;
    s.mc_gx = tv->mc_gx; s.mc_gy = tv->mc_gy; s.mc_gz = tv->mc_gz; s.mc_gxy = tv->mc_gx * tv->mc_gy;
}

// Build the device scene from the PODs.  All derived values use the same float operations, in
// the same order, as the reference's device code would (they are part of the numeric contract).
int build_scene(const svr_volume& vol, const svr_transfer_function& tf, const svr_camera& cam,
                svr::DevScene& s)
{
    memset(&s, 0, sizeof s);
    Texture* tv = find_tex(vol.tex, TEX_VOLUME);
    if (!tv) return fail(-2, "cudaVolume.tex (0x%llx) is not a live volume texture handle", (unsigned long long)vol.tex);
    Texture* tt = find_tex(tf.tex, TEX_TF);
    if (!tt) return fail(-2, "cudaTransferFunction.tex (0x%llx) is not a live transfer-function handle", (unsigned long long)tf.tex);
    if (!(tf.maxOpacity > 0.f) || !std::isfinite(tf.maxOpacity))
        return fail(-3, "transfer function maxOpacity (Woodcock majorant) must be finite and > 0, got %g", (double)tf.maxOpacity);
    if (!finite3(vol.bbox.vmin) || !finite3(vol.bbox.vmax) || !finite3(vol.bbox.invSize) || !finite3(vol.spacing) ||
        !finite3(vol.invSpacing) || !std::isfinite(vol.densityScale))
        return fail(-3, "cudaVolume has non-finite fields");
    if (cam.imageW == 0 || cam.imageH == 0) return fail(-3, "camera image size is zero");

    s.vmin[0] = vol.bbox.vmin.x; s.vmin[1] = vol.bbox.vmin.y; s.vmin[2] = vol.bbox.vmin.z;
    s.invSize[0] = vol.bbox.invSize.x; s.invSize[1] = vol.bbox.invSize.y; s.invSize[2] = vol.bbox.invSize.z;
    // cuda_bbox.h:38-39
    s.clip_vmin[0] = vol.bbox.vmin.x * (-vol.x_clip.x);
    s.clip_vmin[1] = vol.bbox.vmin.y * (-vol.y_clip.x);
    s.clip_vmin[2] = vol.bbox.vmin.z * (-vol.z_clip.x);
    s.clip_vmax[0] = vol.bbox.vmax.x * vol.x_clip.y;
    s.clip_vmax[1] = vol.bbox.vmax.y * vol.y_clip.y;
    s.clip_vmax[2] = vol.bbox.vmax.z * vol.z_clip.y;
    s.densityScale = vol.densityScale;
    s.invMaxMagnitude = vol.invMaxMagnitude;
    s.gradientFactor = vol.gradientFactor;
    {
        volatile float c = -25.f * vol.gradientFactor;     // pathtracer.cu:251, left to right
        c = c * vol.gradientFactor;
        c = c * vol.gradientFactor;
        s.pbrdf_c = c;
    }
    s.spacing[0] = vol.spacing.x; s.spacing[1] = vol.spacing.y; s.spacing[2] = vol.spacing.z;
    s.invSpacing[0] = vol.invSpacing.x; s.invSpacing[1] = vol.invSpacing.y; s.invSpacing[2] = vol.invSpacing.z;
    s.vox = (const uint16_t*)tv->data;
    s.nx = tv->nx; s.ny = tv->ny; s.nz = tv->nz;
    s.layout = tv->layout;
    s.fnx = (float)tv->nx; s.fny = (float)tv->ny; s.fnz = (float)tv->nz;
    s.sy = tv->sy; s.sz = tv->sz; s.bnx = tv->bnx; s.bny = tv->bny;

    s.tf = (const float*)tt->data;
    s.tf_n = tt->nx;
    s.tf_nf = (float)tt->nx;
    s.sigmaMax = tf.maxOpacity;
    {
        volatile float a = 1.f / tf.maxOpacity;            // woodcock_tracking.h:30
        volatile float b = tf.maxOpacity * 1.f;            // BASE_SAMPLE_STEP_SIZE 1.f, :18
        volatile float c2 = 1.f / b;                       // :31
        s.invSigmaMax = a;
        s.invSigmaMaxSI = c2;
    }

    s.imageW = cam.imageW; s.imageH = cam.imageH;
    s.exposure = cam.exposure; s.apeture = cam.apeture; s.focalLength = cam.focalLength;
    s.aspectRatio = cam.aspectRatio; s.tanFovxOverTwo = cam.tanFovxOverTwo;
    s.wm1 = (float)cam.imageW - 1.f;
    s.hm1 = (float)cam.imageH - 1.f;
    {
        // cudaCamera::GenerateRay with apeture == +0 (the reference's default, gui/canvas.h:218): lens sample = (cos(theta) * 0, sin(theta) * 0)
        // = (+-0, +-0).  orig = pos + u * (+-0) + v * (+-0) is pos bit for bit unless a component of pos is -0 (-0 + +0 = +0); the image-plane
        // coordinates are +0 or non-zero when their scales are positive, so subtracting +-0 changes nothing.  Then the kernels may skip the
        // sqrt and the sincos of the lens sample (the two draws are still consumed).
        uint32_t ap_bits, p_bits[3];
        memcpy(&ap_bits, &cam.apeture, 4);
        memcpy(p_bits, &cam.pos, 12);
        const float scale_x = cam.aspectRatio * cam.tanFovxOverTwo * cam.focalLength, scale_y = cam.tanFovxOverTwo * cam.focalLength;
        s.cam_pinhole = (g.opt_pinhole_fast && ap_bits == 0u && p_bits[0] != 0x80000000u && p_bits[1] != 0x80000000u && p_bits[2] != 0x80000000u &&
                         cam.aspectRatio > 1e-20f && cam.tanFovxOverTwo > 1e-20f && cam.focalLength > 1e-20f && scale_x > 1e-20f && scale_y > 1e-20f &&
                         std::isfinite(scale_x) && std::isfinite(scale_y)) ? 1u : 0u;
    }
    s.cam_pos[0] = cam.pos.x; s.cam_pos[1] = cam.pos.y; s.cam_pos[2] = cam.pos.z;
    s.cam_u[0] = cam.u.x; s.cam_u[1] = cam.u.y; s.cam_u[2] = cam.u.z;
    s.cam_v[0] = cam.v.x; s.cam_v[1] = cam.v.y; s.cam_v[2] = cam.v.z;
    s.cam_w[0] = cam.w.x; s.cam_w[1] = cam.w.y; s.cam_w[2] = cam.w.z;
    return 0;
}

int add_lights_env(svr::DevScene& s)
{
    s.env = nullptr;
    if (g.env.tex != 0) {
        Texture* te = find_tex(g.env.tex, TEX_ENV);
        if (!te) return fail(-2, "cudaEnvironmentLight.tex (0x%llx) is not a live environment texture handle", (unsigned long long)g.env.tex);
        s.env = (const float*)te->data;
        s.env_w = te->nx; s.env_h = te->ny;
        s.env_cdf = te->env_cdf;
    }
    s.env_default[0] = g.env.defaultRadiance.x; s.env_default[1] = g.env.defaultRadiance.y; s.env_default[2] = g.env.defaultRadiance.z;
    s.env_intensity = g.env.intensity;
    s.env_offset[0] = g.env.offset.x; s.env_offset[1] = g.env.offset.y;
    s.env_on_escape = (uint32_t)g.opt_env_on_escape;
    s.num_lights = g.num_lights;
    s.primary_light_mask = 0u;
    for (uint32_t i = 0; i < g.num_lights; ++i) {
        const svr_area_light& l = g.lights[i];
        svr::DevLight& d = s.lights[i];
        if (!g.opt_light_cull || light_reachable_by_camera_rays(s, l)) s.primary_light_mask |= 1u << i;
        d.radius = l.disk.radius;
        d.center[0] = l.disk.center.x; d.center[1] = l.disk.center.y; d.center[2] = l.disk.center.z;
        d.normal[0] = l.disk.normal.x; d.normal[1] = l.disk.normal.y; d.normal[2] = l.disk.normal.z;
        // cuda_disk.h:53-56: M_PI * radius * radius (double) -> float
        volatile float area = (float)(3.14159265358979323846 * (double)l.disk.radius * (double)l.disk.radius);
        d.area = area;
        // cuda_arealight.h:57: 500.f * color * intensity * float(M_1_PI) / area, left to right per component
        const float c3[3] = {l.color.x, l.color.y, l.color.z};
        for (int c = 0; c < 3; ++c) {
            volatile float r = 500.f * c3[c];
            r = r * l.intensity;
            r = r * (float)0.31830988618379067154;
            r = r / area;
            d.radiance[c] = r;
        }
    }
    return 0;
}

int fill_work(svr::DevWork& w, uint32_t W, uint32_t H)
{
    memset(&w, 0, sizeof w);
    w.counters = g.d_counters;
    w.ticket = g.d_ticket;
    w.refill_min_idle = (uint32_t)g.opt_refill;
    w.debug_stop = (uint32_t)g.opt_debug_stop;
    w.row_order = (uint32_t)g.opt_row_order;
    w.nan_guard = (uint32_t)g.opt_nan_guard;
    w.strip_rows = g.strip_rows ? g.strip_rows : 1;
    w.rank = g.rank;
    w.world = g.world;
    if (g.world > 1) {
        // interleaved strips over the full frame
        w.x0 = 0; w.x1 = W; w.y0 = 0; w.y1 = H;
        uint32_t rows = 0;
        uint32_t nstrips = (H + w.strip_rows - 1) / w.strip_rows;
        for (uint32_t sidx = g.rank; sidx < nstrips; sidx += g.world) {
            uint32_t ys = sidx * w.strip_rows;
            uint32_t ye = ys + w.strip_rows < H ? ys + w.strip_rows : H;
            rows += ye - ys;
        }
        // the strip->row formula in the kernels needs whole strips except possibly the last owned one
        w.n_rows = rows;
    } else {
        int x0 = g.wx0 < 0 ? 0 : g.wx0, y0 = g.wy0 < 0 ? 0 : g.wy0;
        int x1 = (g.wx1 < 0 || g.wx1 > (int)W) ? (int)W : g.wx1;
        int y1 = (g.wy1 < 0 || g.wy1 > (int)H) ? (int)H : g.wy1;
        if (x0 > x1) x0 = x1;
        if (y0 > y1) y0 = y1;
        w.x0 = (uint32_t)x0; w.x1 = (uint32_t)x1; w.y0 = (uint32_t)y0; w.y1 = (uint32_t)y1;
        w.n_rows = w.y1 - w.y0;
    }
    w.n_items = w.n_rows * (w.x1 - w.x0);
    return 0;
}

// what an image call (ray caster, projection, slice) does between its argument checks and its launch: the device scene, and the owned
// pixels of the camera's image as the work, drawn into img
int image_scene(const svr_volume& vol, const svr_transfer_function& tf, const svr_camera& cam, void* img, svr::DevScene& s, svr::DevWork& w)
{
    if (build_scene(vol, tf, cam, s)) return g.err_code;
    fill_work(w, s.imageW, s.imageH);
    w.img = (uint8_t*)img;
    return 0;
}

// the whole frame, whatever shard or window is set
void fill_work_full(svr::DevWork& w, uint32_t W, uint32_t H)
{
    memset(&w, 0, sizeof w);
    w.counters = g.d_counters;
    w.ticket = g.d_ticket;
    w.strip_rows = 1; w.rank = 0; w.world = 1;
    w.x0 = 0; w.x1 = W; w.y0 = 0; w.y1 = H;
    w.n_rows = H;
    w.n_items = W * H;
}

bool partial_frame(uint32_t W, uint32_t H)
{
    svr::DevWork w;
    fill_work(w, W, H);
    return w.n_items != W * H;
}

// (Re)build the empty-space bitmask when the volume, the transfer-function table or densityScale
// changed.  Scene edits are rare (UI events), so the rebuild simply drains the device first.
int ensure_mask(svr::DevScene& s, const svr_volume& vol, const svr_transfer_function& tf)
{
    s.empty_mask = nullptr;
    // the lane machine's parking thresholds are not the mask's: a queue build forced on without empty-space skipping (SVR_OPT_QUEUE = 2,
    // SVR_OPT_EMPTY_SKIP = 0) reads them too, and with 0 its walk loop leaves before every iteration and the drain never ends
    s.park_end = (uint32_t)g.opt_park_end;
    s.park_cheap = (uint32_t)g.opt_park_cheap;
    if (!g.opt_empty_skip) return 0;
    Texture* tv = find_tex(vol.tex, TEX_VOLUME);
    Texture* tt = find_tex(tf.tex, TEX_TF);
    if (!tv || !tt || !tv->mm || !tt->zero_prefix) return 0;
    uint32_t ds_bits, sg_bits;
    memcpy(&ds_bits, &vol.densityScale, 4);
    memcpy(&sg_bits, &tf.maxOpacity, 4);
    uint32_t n_cells = (uint32_t)tv->mc_gx * (uint32_t)tv->mc_gy * (uint32_t)tv->mc_gz;
    uint32_t words = (n_cells + 31u) / 32u;
    if (!(g.mask_valid && g.mask_vol == vol.tex && g.mask_tf == tf.tex && g.mask_tf_version == tt->version &&
          g.mask_ds_bits == ds_bits && g.mask_sigma_bits == sg_bits)) {
        {
            // the tables built here, their scratch (d_mask_tmp, d_sub8: one byte per cell) and the walks' LDS copies have these fixed capacities
            // (svr_macro_grid keeps every grid within them, so no volume texture reaches this): never launch beyond
            const size_t hn = (size_t)((tv->mc_gx + 1) / 2) * (size_t)((tv->mc_gy + 1) / 2) * (size_t)((tv->mc_gz + 1) / 2);
            if ((size_t)tv->mc_gx * (size_t)tv->mc_gy * (size_t)tv->mc_gz > (size_t)svr::MASK_WORDS_MAX * 32 || (hn + 7) / 8 > svr::DIST_WORDS_MAX)
                return fail(-6, "macro grid %d x %d x %d exceeds the acceleration tables (%u mask words of %u, %zu distance words of %u)", tv->mc_gx, tv->mc_gy,
                            tv->mc_gz, words, svr::MASK_WORDS_MAX, (hn + 7) / 8, svr::DIST_WORDS_MAX);
        }
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(svr::launch_empty_mask(tv->mm, tv->mc_gx, tv->mc_gy, tv->mc_gz, tt->zero_prefix, tt->nx,
                                       vol.densityScale, g.d_mask, words, g.d_mask_tmp, g.stream));
        if (tv->mm_fine) {
            const size_t fcells = (size_t)tv->fg_x * tv->fg_y * tv->fg_z, fwords = (fcells + 31) / 32;
            if (fwords > g.fine_mask_words) {
                if (g.d_fine_mask) HIP_TRY(hipFree(g.d_fine_mask));
                g.d_fine_mask = nullptr; g.fine_mask_words = 0;
                HIP_TRY(hipMalloc((void**)&g.d_fine_mask, fwords * sizeof(uint32_t)));
                g.fine_mask_words = fwords;
            }
            HIP_TRY(svr::launch_fine_mask(tv->mm_fine, (uint32_t)fcells, tt->zero_prefix, tt->nx, vol.densityScale, g.d_fine_mask, (uint32_t)fwords, g.stream));
            if (!g.d_sub8) HIP_TRY(hipMalloc((void**)&g.d_sub8, (size_t)svr::MASK_WORDS_MAX * 32));
            HIP_TRY(svr::launch_sub8(g.d_fine_mask, tv->fg_x, tv->fg_y, tv->fg_z, tv->mc_gx, tv->mc_gy, tv->mc_gz, g.d_sub8, g.stream));
        }
        g.sub8_valid = tv->mm_fine != nullptr;
        HIP_TRY(svr::launch_bound_class(tv->mm, tv->mc_gx, tv->mc_gy, tv->mc_gz, (const float*)tt->data, tt->nx, vol.densityScale,
                                        s.invSigmaMax, g.d_mask, g.stream));
        g.bnd8_valid = false;
        // (the byte table has fixed rows of BOUND8_DIM entries: a half-resolution grid with more cells on an axis -- an elongated volume -- does without it)
        const int b8 = (int)svr::BOUND8_DIM - 2;
        if (tv->mm_wide && (tv->mc_gx + 1) / 2 <= b8 && (tv->mc_gy + 1) / 2 <= b8 && (tv->mc_gz + 1) / 2 <= b8) {
            if (!g.d_bnd8) HIP_TRY(hipMalloc((void**)&g.d_bnd8, svr::BOUND8_BYTES));
            HIP_TRY(svr::launch_bound8(tv->mm_wide, (tv->mc_gx + 1) / 2, (tv->mc_gy + 1) / 2, (tv->mc_gz + 1) / 2, (const float*)tt->data, tt->nx, vol.densityScale,
                                       s.invSigmaMax, g.d_bnd8, g.stream));
            g.bnd8_valid = true;
        }
        HIP_TRY(hipStreamSynchronize(g.stream));
        // the bound test costs two dependent LDS reads per tested cell (4 % on a scene where it never rejects anything): use
        // it where at least 2 % of the coarse cells that can hold a collision have a bound below 1
        uint32_t census[3] = {0u, 0u, 0u};
        HIP_TRY(hipMemcpy(census, g.d_mask + svr::ACCEL_CENSUS_OFF, sizeof census, hipMemcpyDeviceToHost));
        g.mask_has_empty = census[2] != 0u;
        g.mask_cull_useful = (uint64_t)census[0] * 50u >= (uint64_t)census[0] + census[1] && census[0] != 0u;
        g.mask_valid = true; g.mask_vol = vol.tex; g.mask_tf = tf.tex; g.mask_tf_version = tt->version;
        g.mask_ds_bits = ds_bits; g.mask_sigma_bits = sg_bits; g.mask_words = words;
    }
    s.empty_mask = g.d_mask;
    s.mask_words = g.mask_words;
    {
        const int hgx = (tv->mc_gx + 1) / 2, hgy = (tv->mc_gy + 1) / 2, hgz = (tv->mc_gz + 1) / 2;
        s.mc_hgx = hgx; s.mc_hgxy = hgx * hgy;
        s.dist_words = ((uint32_t)hgx * (uint32_t)hgy * (uint32_t)hgz + 7u) / 8u;
    }
    use_macro_grid(s, tv);
    // macro-grid coordinate of a world point: ((p - vmin) * invSize * N + 0.5) / S  (cell c' = c + 1)
    float invS = 1.f / (float)(1 << tv->mc_shift);
    s.mc_scale[0] = s.invSize[0] * s.fnx * invS;
    s.mc_scale[1] = s.invSize[1] * s.fny * invS;
    s.mc_scale[2] = s.invSize[2] * s.fnz * invS;
    s.mc_off = 0.5f * invS;
    // whole-ray tests need every fetch of a walk inside the texture domain: clipped box within the bbox
    bool inside = true;
    const float lo[3] = {vol.bbox.vmin.x, vol.bbox.vmin.y, vol.bbox.vmin.z};
    const float hi[3] = {vol.bbox.vmax.x, vol.bbox.vmax.y, vol.bbox.vmax.z};
    for (int a = 0; a < 3; ++a) {
        float cl = s.clip_vmin[a] < s.clip_vmax[a] ? s.clip_vmin[a] : s.clip_vmax[a];
        float ch = s.clip_vmin[a] < s.clip_vmax[a] ? s.clip_vmax[a] : s.clip_vmin[a];
        inside = inside && cl >= lo[a] && ch <= hi[a] && lo[a] < hi[a];
    }
    s.ray_skip = (inside && g.opt_ray_skip) ? 1u : 0u;
    // the fine level costs a dependent (cached) global load per tested cell, which is what it saves: c5 fetches 3.9 instead of 5.9
    // taps per path at 5.18 instead of 5.27 Gsamples/s, c3 3.0 instead of 4.0 at 7.89 instead of 8.06 -> off by default (1 = auto
    // would turn it on for cells >= 16 voxels)
    s.fine_mask = (tv->mm_fine && g.d_fine_mask && (g.opt_fine_mask == 2 || (g.opt_fine_mask == 1 && tv->mc_shift >= 4))) ? g.d_fine_mask : nullptr;
    s.fg_x = tv->fg_x; s.fg_y = tv->fg_y; s.fg_z = tv->fg_z; s.fg_xy = tv->fg_x * tv->fg_y;
    // sub-cell occupancy pays where macro-cells are large (c5, 16 voxels: +6 %) and costs where they are small (c3, 8 voxels: -4 %)
    s.sub8 = (g.sub8_valid && g.d_sub8 && (g.opt_lm_sub == 2 || (g.opt_lm_sub == 1 && tv->mc_shift >= 4))) ? g.d_sub8 : nullptr;
    s.has_empty = g.mask_has_empty ? 1u : 0u;
    s.bound_cull = (g.opt_bound_cull == 2 || (g.opt_bound_cull == 1 && g.mask_cull_useful)) ? 1u : 0u;
    // pool tuning (same-box sweeps, gpurun_out/r03p_lm_tune.log): on the full-resolution grid (scenes with empty space) one cell per turn
    // (c3 9 920 / c5 8 430 Msamples/s against 9 480 / 7 630 with three), on the half-resolution grid of fog-like media three cells
    // and later refills (c3n 4 860 against 4 290 with one cell)
    // tasks per batch of the traceDepth-1 pool (bits 24-31; same-box A/B, 10 / 16 / 21 tasks: c3 10 215 / 10 064 / 9 821, c5 8 611 / 8 383 / 8 173, c3n 4 747 / 4 932 / 4 972)
    s.lm_tune = g.opt_lm_tune ? (uint32_t)g.opt_lm_tune : (g.mask_has_empty ? (1u | (16u << 8) | (16u << 16) | (10u << 24)) : (3u | (24u << 8) | (24u << 16) | (21u << 24)));
    if ((s.lm_tune >> 24) == 0u) s.lm_tune |= (g.mask_has_empty ? 10u : 21u) << 24;
    // five-iteration trips of the lane machine: walks of tens of iterations with few fetches -- media without exactly transparent space under
    // bound culling (c3n: +20 %; c3 / c5 at depth 2: -1..2 %)
    s.trips = (g.opt_trips == 2 || (g.opt_trips == 1 && s.bound_cull && !s.has_empty)) ? 1u : 0u;
    // Fast bound look-up of the lane machine's trips (svr_lanes.hpp iterate_rot; svr_accel.hip k_bound8): media without exactly transparent space under
    // bound culling.  The look-up takes the macro-cell from one fma per axis on the ray parameter; the table covers one voxel of error, the float chains
    // differ by ~8 ulp of the largest intermediate -- |origin - volume| * N voxels * 2^-21 -- so the camera may be up to 2^21 / (16 N) volume extents
    // away (128 at N = 1024; scatter points and shadow rays start inside the volume) before the kernel falls back to the exact cell.  The look-up
    // does not clamp: the clipped box must lie inside the texture domain (`inside`), as for the whole-ray tests.
    s.bnd8 = nullptr;
    s.hc_scale[0] = 0.5f * s.mc_scale[0]; s.hc_scale[1] = 0.5f * s.mc_scale[1]; s.hc_scale[2] = 0.5f * s.mc_scale[2];
    s.hc_off = 0.5f * s.mc_off + 1.f;
    if (g.opt_fast_bound && g.bnd8_valid && s.bound_cull && !s.has_empty && s.fine_mask == nullptr && s.trips && inside) {
        bool near_enough = true;
        const int nmax = tv->nx > tv->ny ? (tv->nx > tv->nz ? tv->nx : tv->nz) : (tv->ny > tv->nz ? tv->ny : tv->nz);
        const double reach = 2097152.0 / (16.0 * (double)nmax);
        for (int a = 0; a < 3; ++a) {
            const double c = 0.5 * ((double)lo[a] + (double)hi[a]), ext = (double)hi[a] - (double)lo[a];
            const double d = ((double)s.cam_pos[a] - c) / ext;
            near_enough = near_enough && ext > 0.0 && d == d && (d < 0 ? -d : d) <= reach;
        }
        if (near_enough) s.bnd8 = g.d_bnd8;
    }
    return 0;
}

// Leaps of the projection and hit kernels (svr_march.hpp, LEAPS): every sample must map into the macro grid (the clipped box inside the
// texture domain), and the float error of p = orig + dir * t -- a few ulp of the largest magnitude involved, |orig| + |p| with p in the
// box -- must stay below 0.02 macro-cells.  mc_scale = macro-cells per world unit (s holds the scene and tv's macro grid)
bool leaps_allowed(const svr::DevScene& s, const svr_volume& vol, const Texture* tv, float mc_scale[3])
{
    const float invS = 1.f / (float)(1 << tv->mc_shift);
    mc_scale[0] = s.invSize[0] * s.fnx * invS; mc_scale[1] = s.invSize[1] * s.fny * invS; mc_scale[2] = s.invSize[2] * s.fnz * invS;
    const float lo[3] = {vol.bbox.vmin.x, vol.bbox.vmin.y, vol.bbox.vmin.z}, hi[3] = {vol.bbox.vmax.x, vol.bbox.vmax.y, vol.bbox.vmax.z};
    bool inside = true;
    double mag = 0.0, scale = 0.0;
    for (int a = 0; a < 3; ++a) {
        const float cl = std::min(s.clip_vmin[a], s.clip_vmax[a]), ch = std::max(s.clip_vmin[a], s.clip_vmax[a]);
        inside = inside && cl >= lo[a] && ch <= hi[a] && lo[a] < hi[a];
        mag = std::max(mag, (double)std::fabs(s.cam_pos[a]) + std::max(std::fabs((double)lo[a]), std::fabs((double)hi[a])));
        scale = std::max(scale, (double)std::fabs(mc_scale[a]));
    }
    const double err_cells = 2.0 * mag * 4.0 * 5.9604644775390625e-08 * scale;       // 4 ulp of 2 (|orig| + |p|), in macro-cells
    return inside && std::isfinite(err_cells) && err_cells <= 0.02;
}

// the tables a march over tv's min/max table skips by (svr_march.hpp): the table, and the neighbourhood table where leaps are allowed
int fill_march_tables(const char* who, svr::DevScene& s, const svr_volume& vol, Texture* tv, svr::MarchTables& tb)
{
    tb.mm = tv->mm;
    use_macro_grid(s, tv);
    if (leaps_allowed(s, vol, tv, tb.mc_scale)) {
        if (int e = ensure_nbmax(who, tv)) return e;
        tb.nbmax = tv->nbmax;
        tb.leap = 1u;
    }
    return 0;
}

} // namespace svr_host
