// svr_denoise.hip -- edge-aware denoised preview of the first frames of a render (SVR_OPT_DENOISE_PREVIEW).
//
//  k_guides     one deterministic ray per pixel (the pinhole centre ray, cuda_camera.h:85-95) marched at a fixed step h
//               through the clipped box (woodcock_tracking.h:22-26 interval) with the path tracer's extinction (TF alpha of
//               volume(p), BASE_SAMPLE_STEP_SIZE 1): first-collision weights w_i = T_i (1 - exp(-sigma_i h)), T_{i+1} = T_i exp(-sigma_i h),
//               stop at T < 2^-10.  Four guides per pixel, two float4: (N.xyz, D) and (A.rgb, O) -- opacity O = sum w, expected depth
//               D = sum w t / O, albedo A = sum w rgb / O, normal N = normalize(sum w grad); O == 0: D = -1, N = 0, A = 1.
//               Samples in `empty` macro-cells (svr_accel.hip) contribute exactly nothing and are not fetched; deep-empty stretches
//               are leapt over with the distance field (svr_walk.hpp, first_occupied).  Same result with and without skipping.
//  k_demod      c = hdr / max(A, 1e-3) (demodulated radiance, float4 per pixel)
//  k_atrous     one pass of the edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010): 5 x 5 B3-spline taps at a
//               distance of 2^k pixels, weights normalised per pixel; edge stops on depth, normal, albedo, opacity and
//               (optionally) luminance.  The last pass remodulates by max(A, 1e-3) and tone-maps (tonemapping.h:13-27, the float
//               operations of k_tonemap) or writes the HDR result.  Pixels with O == 0 pass through untouched and contribute to no
//               pixel with O > 0.
// The accumulator is only read.
#include "svr_walk.hpp"
#include "svr_denoise.hpp"

namespace svr {

constexpr uint32_t GUIDE_TILE = 32;      // a 1024-thread block marches a 32 x 32 pixel tile (a wave = 32 x 2 pixels)

template <bool SKIP>
struct LdsGuides : std::conditional<SKIP, LdsTile, LdsTileNoMask>::type {
    float4 rgba[SVR_TF_MAX + SVR_TF_PAD];  // entry e = texel clamp(e-1)
};

template <int LAYOUT, bool SKIP>
__global__ __launch_bounds__(1024) void k_guides(const DevScene s, float4* __restrict__ out, float h)
{
    __shared__ LdsGuides<SKIP> L;
    {
        const int n = s.tf_n;
        const float4* gtf = reinterpret_cast<const float4*>(s.tf);
        for (int e = threadIdx.x; e < n + SVR_TF_PAD; e += blockDim.x) L.rgba[e] = gtf[min(max(e - 1, 0), n - 1)];
    }
    lds_tile_load(L, s, SKIP);                 // alpha table (+ the masks), then a barrier
    const uint32_t x = blockIdx.x * GUIDE_TILE + (threadIdx.x & (GUIDE_TILE - 1u));
    const uint32_t y = blockIdx.y * GUIDE_TILE + (threadIdx.x / GUIDE_TILE);
    if (x >= s.imageW || y >= s.imageH) return;
    v3 o, d;
    camera_ray_pinhole(s, x, y, o, d);
    float O = 0.f, Ds = 0.f, T = 1.f;
    v3 As = V3(0.f, 0.f, 0.f), Ns = V3(0.f, 0.f, 0.f);
    float tNear, tFar;
    if (volume_intersect(s, o, d, tNear, tFar)) {
        const float tMin = tNear < 0.f ? (float)1e-6 : tNear, tMax = tFar;     // woodcock_tracking.h:22-26
        const float INF = u2f(SVR_INF_BITS);
        uint32_t i = 0;
        bool done = false;
        // index of a sample at or before ray parameter t (one sample of margin: a sample that is skipped wrongly would change the result,
        // one that is evaluated needlessly would not)
        auto index_before = [&](float t) -> uint32_t {
            const float k = __builtin_floorf((t - tMin) / h) - 1.f;
            return k > 0.f ? (k < 4194304.f ? (uint32_t)k : 4194304u) : 0u;
        };
        if (SKIP && s.ray_skip) {
            const float t_occ = first_occupied(s, L, o, d, tMin, tMax);
            if (t_occ == INF) done = true;
            else i = index_before(t_occ);
        }
        for (uint32_t guard = 0; !done && guard < 4194304u; ++guard, ++i) {
            const float t = tMin + (float)i * h;
            if (!(t <= tMax)) break;
            const v3 p = o + d * t;
            const Cell c = cell_of(s, p);
            if (SKIP && cell_is_empty<false>(L, s, c)) {
                if (s.ray_skip && cell_is_empty<true>(L, s, c)) {
                    // deep-empty: leap to the next possibly-occupied stretch
                    const float t_occ = first_occupied(s, L, o, d, t, tMax);
                    if (t_occ == INF) break;
                    const uint32_t j = index_before(t_occ);
                    if (j > i + 1u) i = j - 1u;
                }
                continue;
            }
            const float xi = tex_fetch<LAYOUT>(s, c) * s.densityScale;       // = volume(p), cuda_volume.h:87-100
            const float sigma = alpha_of(L, s, xi);
            if (sigma == 0.f) continue;                                         // exactly transparent: w = 0, T unchanged
            const float e = expf_(-sigma * h);
            const float w = T * (1.f - e);
            T = T * e;
            if (w > 0.f) {
                int te; float ta;
                lds_tf_coord(s, xi, te, ta);
                const float4 t0 = L.rgba[te], t1 = L.rgba[te + 1];
                const v3 rgb = V3(lerpf(t0.x, t1.x, ta), lerpf(t0.y, t1.y, ta), lerpf(t0.z, t1.z, ta));
                const v3 gr = volume_gradient<LAYOUT>(s, p);
                O = O + w;
                Ds = Ds + w * t;
                As = As + rgb * w;
                Ns = Ns + gr * w;
            }
            if (T < 0.0009765625f) break;
        }
    }
    float4 g0, g1;
    if (O == 0.f) {
        g0 = make_float4(0.f, 0.f, 0.f, -1.f);
        g1 = make_float4(1.f, 1.f, 1.f, 0.f);
    } else {
        const float n2 = dot(Ns, Ns);
        const v3 N = n2 > 0.f ? normalize(Ns) : V3(0.f, 0.f, 0.f);
        g0 = make_float4(N.x, N.y, N.z, Ds / O);
        g1 = make_float4(As.x / O, As.y / O, As.z / O, O);
    }
    const size_t pix = (size_t)y * s.imageW + x;
    out[2 * pix] = g0;
    out[2 * pix + 1] = g1;
}

// c = hdr / max(A, 1e-3)
__global__ __launch_bounds__(256) void k_demod(const float* __restrict__ hdr, const float4* __restrict__ guides, float4* __restrict__ c, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 a = guides[2 * (size_t)i + 1];
    const float* hp = hdr + 3 * (size_t)i;
    c[i] = make_float4(hp[0] / fmax_(a.x, 1e-3f), hp[1] / fmax_(a.y, 1e-3f), hp[2] / fmax_(a.z, 1e-3f), 0.f);
}

SVR_DEV bool finite4(float4 v)
{
    return ((f2u(v.x) & 0x7f800000u) != 0x7f800000u) & ((f2u(v.y) & 0x7f800000u) != 0x7f800000u) & ((f2u(v.z) & 0x7f800000u) != 0x7f800000u);
}

SVR_DEV float lum(float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// One a-trous pass at step 2^k.  mode 0: write cout; mode 1: remodulate + tone map into img; mode 2: remodulate into hdr_out (float3).
__global__ __launch_bounds__(256) void k_atrous(const float4* __restrict__ cin, float4* __restrict__ cout, const float4* __restrict__ guides,
                                                const float* __restrict__ hdr, uint32_t* __restrict__ img, float* __restrict__ hdr_out,
                                                const DenoiseArgs a, uint32_t k, int mode)
{
    const uint32_t x = blockIdx.x * 16u + (threadIdx.x & 15u), y = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * a.W + x;
    const float4 gp0 = guides[2 * p], gp1 = guides[2 * p + 1];
    if (gp1.w == 0.f) {
        // O == 0: passes through untouched (background, environment, lights seen through air)
        if (mode == 0) { cout[p] = cin[p]; return; }
        const float* hp = hdr + 3 * p;
        if (mode == 1) img[p] = tonemap_pixel(V3(hp[0], hp[1], hp[2]), a.exposure);
        else { hdr_out[3 * p] = hp[0]; hdr_out[3 * p + 1] = hp[1]; hdr_out[3 * p + 2] = hp[2]; }
        return;
    }
    const int step = 1 << k;
    const float4 cp = cin[p];
    const float lp = lum(cp);
    // exponent scales (0 = the term is off)
    const float kd = a.sigma_depth > 0.f ? 1.f / (a.sigma_depth * (float)step * (gp0.w * a.pix_scale)) : 0.f;
    const float ka = a.sigma_albedo > 0.f ? 1.f / (a.sigma_albedo * a.sigma_albedo) : 0.f;
    const float ko = a.sigma_opacity > 0.f ? 1.f / a.sigma_opacity : 0.f;
    const float kc = a.sigma_color > 0.f ? 1.f / (a.sigma_color * a.sigma_color * u2f((uint32_t)(127 - (int)k) << 23)) : 0.f;
    const float hw[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
    for (int j = -2; j <= 2; ++j) {
        const int qy = (int)y + j * step;
        if (qy < 0 || qy >= (int)a.H) continue;
        for (int i = -2; i <= 2; ++i) {
            const int qx = (int)x + i * step;
            if (qx < 0 || qx >= (int)a.W) continue;
            const float hk = hw[j + 2] * hw[i + 2];
            float wgt;
            float4 cq;
            if (i == 0 && j == 0) { wgt = hk; cq = cp; }
            else {
                const size_t q = (size_t)qy * a.W + qx;
                const float4 gq1 = guides[2 * q + 1];
                if (gq1.w == 0.f) continue;                                     // O == 0 never contributes to O > 0
                cq = cin[q];
                if (!finite4(cq)) continue;
                const float4 gq0 = guides[2 * q];
                const float dd = __builtin_fabsf(gp0.w - gq0.w);
                const float dar = gp1.x - gq1.x, dag = gp1.y - gq1.y, dab = gp1.z - gq1.z;
                const float da2 = (dar * dar + dag * dag) + dab * dab;
                const float dop = __builtin_fabsf(gp1.w - gq1.w);
                const float dl = lp - lum(cq);
                const float ex = ((dd * kd + da2 * ka) + dop * ko) + (dl * dl) * kc;
                wgt = hk * expf_(-ex);
                if (a.sigma_normal > 0.f) {
                    const float nd = (gp0.x * gq0.x + gp0.y * gq0.y) + gp0.z * gq0.z;
                    wgt = nd > 0.f ? wgt * powf_(nd, a.sigma_normal) : 0.f;
                }
                if (!(wgt > 0.f)) continue;
            }
            sw = sw + wgt;
            sr = sr + wgt * cq.x;
            sg = sg + wgt * cq.y;
            sb = sb + wgt * cq.z;
        }
    }
    const float4 r = make_float4(sr / sw, sg / sw, sb / sw, 0.f);
    if (mode == 0) { cout[p] = r; return; }
    const v3 L = V3(r.x * fmax_(gp1.x, 1e-3f), r.y * fmax_(gp1.y, 1e-3f), r.z * fmax_(gp1.z, 1e-3f));
    if (mode == 1) img[p] = tonemap_pixel(L, a.exposure);
    else { hdr_out[3 * p] = L.x; hdr_out[3 * p + 1] = L.y; hdr_out[3 * p + 2] = L.z; }
}

hipError_t launch_guides(const DevScene& s, float4* out, float h, hipStream_t st)
{
    const dim3 grid((s.imageW + GUIDE_TILE - 1u) / GUIDE_TILE, (s.imageH + GUIDE_TILE - 1u) / GUIDE_TILE);
    with_layout(s.layout, [&](auto lay) {
        with_bool(s.empty_mask != nullptr, [&](auto sk) { hipLaunchKernelGGL((k_guides<decltype(lay)::value, decltype(sk)::value>), grid, dim3(1024), 0, st, s, out, h); });
    });
    return hipGetLastError();
}

hipError_t launch_denoise(const float* hdr, const float4* guides, float4* scratch, uint8_t* img, float* hdr_out, const DenoiseArgs& a, hipStream_t st)
{
    const uint32_t n = a.W * a.H;
    float4* buf[2] = {scratch, scratch + n};
    hipLaunchKernelGGL(k_demod, dim3((n + 255u) / 256u), dim3(256), 0, st, hdr, guides, buf[0], n);
    const dim3 grid((a.W + 15u) / 16u, (a.H + 15u) / 16u);
    for (int k = 0; k < a.passes; ++k) {
        const bool last = k + 1 == a.passes;
        const int mode = !last ? 0 : (img != nullptr ? 1 : 2);
        hipLaunchKernelGGL(k_atrous, grid, dim3(256), 0, st, buf[k & 1], buf[(k + 1) & 1], guides, hdr, reinterpret_cast<uint32_t*>(img), hdr_out, a,
                           (uint32_t)k, mode);
    }
    return hipGetLastError();
}

} // namespace svr
