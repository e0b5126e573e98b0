// shm/ao.h — the ambient occlusion integrator's per-sample arithmetic: PBRT-v4's AOIntegrator::Li (integrators.cpp) written with the functions this library already has.
// Single source like every header here: k_ao.hip compiles it for the device (k_shade_ao), host/host_mirror.cpp for the CPU twin (shm_ao_samples_host), and the two are
// held to each other bit for bit (tests/test_gpu_ambient_occlusion.py). The reference has no such integrator: there is no quirk to reproduce, and none is.
//
// One sample, behind the camera ray K1 generated and its closest hit:
//   escaped      L = 0, nothing queued
//   hit          si = hit_interaction(sv, hit, -d): only pi (with its error bounds) and the geometric normal are read — no get_bsdf, no material, no texture, no
//                differentials, no emission; n = face_forward(si.n, -d)
//   u            sampler_get_2d at the sampler position directly behind the camera sample; nothing else is drawn
//   wl, pdf      sample_cosine_hemisphere(u), cosine_hemisphere_pdf(|wl.z|) — or, uniform mode, sample_uniform_hemisphere(u) and the literal 1 / (2 pi) (NOT
//                uniform_hemisphere_pdf, whose reference-exact value is 1 / (4 pi)); pdf == 0: L = 0, nothing queued
//   wi           frame_from_z(n).from_local(wl)
//   ray          the interaction's spawn_ray(wi): origin offset by the error bounds on wi's side, direction wi, t_max = the maximum distance (PBRT-v4: IntersectP(r, maxDistance))
//   contribution illum_scale * illuminant(lambda) * dot(wi, n) / (pi * pdf), added to L by the any-hit launch where the ray is unoccluded
#pragma once
#include "path.h"

namespace shm {

// ShmRenderParams::ao_max_distance as a t_max: 0 is PBRT-v4's default, infinity (negative and NaN never get here: the entry points reject them)
SHM_HD Float ao_t_max(Float max_distance) { return max_distance > 0.0f ? max_distance : infinity(); }

// The direction in the local frame of n and its density. False: the density is 0 (a cosine sample on the horizon) and the sample is black.
SHM_HD bool ao_sample_direction(V2 u, bool uniform, V3& wl, Float& pdf) {
    if (uniform) {
        wl = sample_uniform_hemisphere(u);
        pdf = INV_2PI;
    } else {
        wl = sample_cosine_hemisphere(u);
        pdf = cosine_hemisphere_pdf(abs(wl.z));
    }
    return pdf != 0.0f;
}

// What the occlusion ray carries if nothing blocks it. `illuminant`: the colour space's 471-entry table; `illum_scale`: 1 / its CIE Y, the float the scene keeps.
SHM_HD Spec ao_contribution(const Float* illuminant, Float illum_scale, const Wavelengths& lambda, V3 wi, V3 n, Float pdf) {
    return (illum_scale * dense_table_sample(illuminant, lambda)) * (dot(wi, n) / (PI_F * pdf));
}

// One sample at a hit (hit.prim >= 0). `d`: the camera ray's direction; `rng`: the sampler directly behind the camera sample (advanced by the one 2-D draw).
// True: `ray` is the occlusion ray to queue and `contrib` its contribution. False: nothing is queued and the sample is black.
// (`pdf_out`: the direction's density, for the twin's caller)
SHM_HD bool ao_sample(const SceneView& sv, const Hit& hit, V3 d, Rng& rng, const Wavelengths& lambda, bool uniform, Float max_distance, Float illum_scale, ShmRay& ray,
                      Spec& contrib, Float* pdf_out = nullptr) {
    const V3 wo = -d;
    const SurfaceInteraction si = hit_interaction<false>(sv, hit, wo);
    const V3 n = face_forward(si.n, wo);
    const V2 u = sampler_get_2d(rng);
    V3 wl;
    Float pdf;
    if (!ao_sample_direction(u, uniform, wl, pdf)) return false;
    const V3 wi = frame_from_z(n).from_local(wl);
    const V3 o = offset_ray_origin(si.pi, si.n, wi);  // si.spawn_ray(wi)
    ray.o[0] = o.x; ray.o[1] = o.y; ray.o[2] = o.z;
    ray.d[0] = wi.x; ray.d[1] = wi.y; ray.d[2] = wi.z;
    ray.t_max = ao_t_max(max_distance);
    ray.pad = 0.0f;
    contrib = ao_contribution(sv.cs_illuminant, illum_scale, lambda, wi, n, pdf);
    if (pdf_out) *pdf_out = pdf;
    return true;
}

}  // namespace shm
