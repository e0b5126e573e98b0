// shm/gbuffer.h — the G-buffer pass's per-sample arithmetic: what a camera ray's first hit leaves for a denoiser (position, geometric and shading normal, uv, albedo).
// Single source like every header here: k_gbuffer.hip compiles it for the device, host/host_mirror.cpp for the CPU twin (shm_gbuffer_samples_host), and the two are held
// to each other bit for bit (tests/test_gpu_gbuffer.py).
//
// PBRT-v4's GBufferFilm / VisibleSurface are the model (film.h, interaction.h); the pass is defined in DESIGN.md section 4i:
//   p, n, ns, uv   of si = hit_interaction(sv, hit, -d) after get_bsdf (bump and normal maps moved the shading frame); n and ns flipped to face wo = -d
//   albedo         BSDF::rho_hd(wo, uc[16], u2[16]) on the fixed points below, weighted by the sensor's three response curves — at unit exposure, unclamped: an albedo
//                  must not move with the film's imaging ratio
// The pass draws no sampler dimension beyond the camera ray's.
#pragma once
#include "path.h"

namespace shm {

constexpr int GBUFFER_RHO_SAMPLES = 16;
// one sample's record: p[3], n[3], ns[3], uv[2], albedo[3], then 1 where the ray hit (0: escaped, everything else 0 too) and a zero
constexpr int GBUFFER_SAMPLE_FLOATS = 16;
constexpr int GBUFFER_HIT_FLAG = 14;
constexpr uint32_t GBUFFER_SPACE_RENDER = 0u, GBUFFER_SPACE_CAMERA = 1u;

// What the first hit of a camera ray shows, before the sensor sees it
struct GBufferSurface {
    V3 p, n, ns;
    V2 uv;
    Spec rho;            // BSDF::rho_hd at the ray's four wavelengths
    Wavelengths lambda;  // ... as get_bsdf left them (a dispersive dielectric ends the secondary wavelengths)
};

// `d`: the camera ray's direction; `aux`: its auxiliary rays (read where HAS_TEX: the scene binds textures); `lambda`: the camera sample's wavelengths.
// options.force_diffuse and `regularize` are not looked at.
template <bool HAS_TEX>
SHM_HD GBufferSurface gbuffer_surface(const SceneView& sv, V3 d, const AuxRays& aux, const Hit& hit, const Wavelengths& lambda_in, const ShmRenderParams& params) {
    // rho_hd's points: u2[i] = ((i + 0.5) / 16, (rev4(i) + 0.5) / 16) — the 4-bit van der Corput pair — and uc[i] = (((5 i) mod 16) + 0.5) / 16
    const Float u2x[GBUFFER_RHO_SAMPLES] = {0.03125f, 0.09375f, 0.15625f, 0.21875f, 0.28125f, 0.34375f, 0.40625f, 0.46875f,
                                            0.53125f, 0.59375f, 0.65625f, 0.71875f, 0.78125f, 0.84375f, 0.90625f, 0.96875f};
    const Float u2y[GBUFFER_RHO_SAMPLES] = {0.03125f, 0.53125f, 0.28125f, 0.78125f, 0.15625f, 0.65625f, 0.40625f, 0.90625f,
                                            0.09375f, 0.59375f, 0.34375f, 0.84375f, 0.21875f, 0.71875f, 0.46875f, 0.96875f};
    const Float uc[GBUFFER_RHO_SAMPLES] = {0.03125f, 0.34375f, 0.65625f, 0.96875f, 0.28125f, 0.59375f, 0.90625f, 0.21875f,
                                           0.53125f, 0.84375f, 0.15625f, 0.46875f, 0.78125f, 0.09375f, 0.40625f, 0.71875f};
    V2 u2[GBUFFER_RHO_SAMPLES];
    for (int i = 0; i < GBUFFER_RHO_SAMPLES; ++i) u2[i] = v2(u2x[i], u2y[i]);
    GBufferSurface g;
    g.lambda = lambda_in;
    const V3 wo = -d;
    SurfaceInteraction si = hit_interaction<false>(sv, hit, wo);
    const PrimRec& prim = sv.prim_recs[hit.prim];
    Differentials df = differentials_zero();
    if (HAS_TEX) df = compute_differentials(sv, si, aux, params.samples_per_pixel, params.disable_pixel_jitter != 0, params.disable_texture_filtering != 0);
    const BSDF bsdf = get_bsdf<HAS_TEX>(sv, si, sv.materials[prim.material], g.lambda, &df);
    g.p = si.p();
    g.n = dot(si.n, wo) < 0.0f ? -si.n : si.n;
    g.ns = dot(si.shading.n, wo) < 0.0f ? -si.shading.n : si.shading.n;
    g.uv = si.uv;
    g.rho = bsdf_rho_hd(bsdf, wo, uc, u2, GBUFFER_RHO_SAMPLES);
    return g;
}

// One sample's record (GBUFFER_SAMPLE_FLOATS floats). `space`: GBUFFER_SPACE_RENDER, or GBUFFER_SPACE_CAMERA — p through camera_from_render as a point, n and ns as
// normals (the transpose of render_from_camera, not renormalised: PBRT-v4's Transform applied to a Normal3f).
template <bool HAS_TEX>
SHM_HD void gbuffer_sample(const SceneView& sv, V3 d, const AuxRays& aux, const Hit& hit, const Wavelengths& lambda, const ShmRenderParams& params, uint32_t space, Float* out) {
    for (int i = 0; i < GBUFFER_SAMPLE_FLOATS; ++i) out[i] = 0.0f;
    if (hit.prim < 0) return;
    GBufferSurface g = gbuffer_surface<HAS_TEX>(sv, d, aux, hit, lambda, params);
    if (space == GBUFFER_SPACE_CAMERA) {
        g.p = xf_point(sv.camera.camera_from_render, g.p);
        g.n = xf_normal(sv.camera.render_from_camera, g.n);
        g.ns = xf_normal(sv.camera.render_from_camera, g.ns);
    }
    // PixelSensor::to_sensor_rgb (film_sample_rgb, path.h) without the imaging ratio and without the film's clamp
    const Spec r = safe_div(g.rho, pdf_spec(g.lambda));
    out[0] = g.p.x; out[1] = g.p.y; out[2] = g.p.z;
    out[3] = g.n.x; out[4] = g.n.y; out[5] = g.n.z;
    out[6] = g.ns.x; out[7] = g.ns.y; out[8] = g.ns.z;
    out[9] = g.uv.x; out[10] = g.uv.y;
    out[11] = average(dense_table_sample(sv.sensor_r_bar, g.lambda) * r);
    out[12] = average(dense_table_sample(sv.sensor_g_bar, g.lambda) * r);
    out[13] = average(dense_table_sample(sv.sensor_b_bar, g.lambda) * r);
    out[GBUFFER_HIT_FLAG] = 1.0f;
}

// A pixel's sums take a sample as RgbFilm::add_sample takes a radiance sample (render.hip, film_add_samples): the float product with the filter weight, widened.
// sums: the 16 doubles of a ShmGBufferPixel, in its order — p, n, ns, uv, albedo, weight_hit, weight_sum.
SHM_HD void gbuffer_add_sample(double* sums, const Float* sample, Float weight) {
    if (sample[GBUFFER_HIT_FLAG] != 0.0f) {
        for (int i = 0; i < 14; ++i) sums[i] += (double)(weight * sample[i]);
        sums[14] += (double)weight;
    }
    sums[15] += (double)weight;
}

}  // namespace shm
