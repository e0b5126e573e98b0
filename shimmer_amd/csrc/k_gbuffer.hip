// k_gbuffer.hip — the G-buffer pass's two kernels (include/shimmer_hip.h, shm_gbuffer_render_wave) and their launcher, wf_launch_gbuffer.
// They run behind K1 (wf_generate, lean_first = false) and the scene's own closest-hit launch over the batch's slots (32-byte hit records):
//   k_gbuffer<HAS_TEX>     one path slot per lane: shm::gbuffer_sample (shm/gbuffer.h) — the interaction, get_bsdf, the 16-sample rho_hd, the sensor weighting — and the
//                          slot's 16-float record, written where the path's CtxRec lives (64 bytes per path in every workspace; nothing of this pass reads a CtxRec,
//                          and a render's first vertex writes it before anything reads it)
//   k_gbuffer_accumulate   one pixel per lane: the pixel's samples added to its ShmGBufferPixel in sample order, in double, each with the weight K6 would give it
// One build serves every scene class, so the shared headers' extensions are all ON here (delta lights are not touched; the diffuse transmission material and the
// disk / cylinder are): the unit sets the switches itself, and its name matches none of the Makefile's *_zs / *_dl patterns.
#define K_DELTA_LIGHTS true
#define K_QUADRICS true
#include "wavefront.h"
#include "shm/gbuffer.h"

namespace {

static_assert(sizeof(CtxRec) == GBUFFER_SAMPLE_FLOATS * sizeof(float), "a slot's G-buffer record takes the place of its CtxRec");
static_assert(sizeof(ShmGBufferPixel) == 16 * sizeof(double), "ShmGBufferPixel is 16 doubles, in gbuffer_add_sample's order");

// LayeredBxDF::sample_f sixteen times over wants every register there is: one workgroup of 256 lanes per SIMD quartet at whatever the allocator needs
// (tools/kernel_resources.py has the outcome: profiles/gbuffer.md)
template <bool HAS_TEX>
__global__ void __launch_bounds__(SHADE2_BLOCK) k_gbuffer(SceneView sv_global, PathArrays pa, uint32_t total, ShmRenderParams params, uint32_t space, LdsTables lds_tables) {
    __shared__ uint4 s_tables[LDS_TABLE_BUDGET / 16];
    __shared__ uint4 s_view[HAS_TEX ? SCENE_VIEW_UINT4S : 1];
    const SceneView sv = stage_scene_tables_tex<HAS_TEX>(sv_global, lds_tables, s_tables, s_view);
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= total) return;
    Hit hit;
    {
        const float4* hp = reinterpret_cast<const float4*>(pa.hit + slot);
        const float4 h0 = hp[0], h1 = hp[1];
        hit.prim = __float_as_int(h0.x); hit.t = h0.y; hit.b0 = h0.z; hit.b1 = h0.w; hit.b2 = h1.x; hit.phi = h1.y; hit.inst = __float_as_int(h1.z) - 1;
    }
    float out[GBUFFER_SAMPLE_FLOATS];
    if (hit.prim < 0) {
        for (int i = 0; i < GBUFFER_SAMPLE_FLOATS; ++i) out[i] = 0.0f;
    } else {
        const float4* rp = reinterpret_cast<const float4*>(pa.ray + slot);
        const float4 r0 = rp[0], r1 = rp[1];
        const V3 d = v3(r0.w, r1.x, r1.y);
        Wavelengths lambda;
        const float4 a = pa.lambda[slot], b = pa.lambda_pdf[slot];
        lambda.lambda[0] = a.x; lambda.lambda[1] = a.y; lambda.lambda[2] = a.z; lambda.lambda[3] = a.w;
        lambda.pdf[0] = b.x; lambda.pdf[1] = b.y; lambda.pdf[2] = b.z; lambda.pdf[3] = b.w;
        AuxRays aux = aux_none();
        if (HAS_TEX) aux = ld_aux(pa, slot);  // (camera rays always carry auxiliary rays)
        gbuffer_sample<HAS_TEX>(sv, d, aux, hit, lambda, params, space, out);
    }
    float4* o = reinterpret_cast<float4*>(pa.ctx + slot);
    o[0] = make_float4(out[0], out[1], out[2], out[3]);
    o[1] = make_float4(out[4], out[5], out[6], out[7]);
    o[2] = make_float4(out[8], out[9], out[10], out[11]);
    o[3] = make_float4(out[12], out[13], out[14], out[15]);
}

// W: shm_plan::FILM_WEIGHT_* — the rule of film_add_samples (render.hip)
__global__ void __launch_bounds__(SHADE_BLOCK) k_gbuffer_accumulate(SceneView sv, PathArrays pa, const uint32_t* pixels, uint32_t n_pix, int n_samples, ShmGBufferPixel* gbuffer,
                                                                    uint32_t pix_group, int w_kind, const float* filter_weight, float weight_k) {
    const uint32_t p_local = blockIdx.x * blockDim.x + threadIdx.x;
    if (p_local >= n_pix) return;
    const uint32_t pix = pixels[p_local];
    const int px = (int)(pix & 0xffffu), py = (int)(pix >> 16);
    const int width = sv.pixel_bounds[2] - sv.pixel_bounds[0];
    double* gp = reinterpret_cast<double*>(gbuffer + (size_t)(py - sv.pixel_bounds[1]) * (size_t)width + (size_t)(px - sv.pixel_bounds[0]));
    double sums[16];
    for (int i = 0; i < 16; ++i) sums[i] = gp[i];
    for (int s = 0; s < n_samples; ++s) {
        const uint32_t slot = slot_of(p_local, (uint32_t)s, n_pix, (uint32_t)n_samples, pix_group);
        const float4* rec = reinterpret_cast<const float4*>(pa.ctx + slot);
        const float4 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
        const float sample[GBUFFER_SAMPLE_FLOATS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
        const float weight = w_kind == shm_plan::FILM_WEIGHT_ONE ? 1.0f : (w_kind == shm_plan::FILM_WEIGHT_CONSTANT ? weight_k : filter_weight[slot]);
        gbuffer_add_sample(sums, sample, weight);
    }
    for (int i = 0; i < 16; ++i) gp[i] = sums[i];
}

}  // namespace

int wf_launch_gbuffer(ShmScene* s, const GBufferArgs& a) {
    const uint32_t total = a.n_pix * (uint32_t)a.n_samples;
    const dim3 grid((total + SHADE2_BLOCK - 1) / SHADE2_BLOCK), block(SHADE2_BLOCK);
    if (a.tex) hipLaunchKernelGGL(k_gbuffer<true>, grid, block, 0, a.stream, s->dsv, s->pa, total, a.params, a.space, s->lds_tables);
    else hipLaunchKernelGGL(k_gbuffer<false>, grid, block, 0, a.stream, s->dsv, s->pa, total, a.params, a.space, s->lds_tables);
    LAUNCH_TRY("k_gbuffer");
    if (a.film_weight == shm_plan::FILM_WEIGHT_PER_SAMPLE && !s->d_filter_weight) { shm_err() = "internal: the G-buffer pass has no per-sample filter weights"; return SHM_ERR_INTERNAL; }
    hipLaunchKernelGGL(k_gbuffer_accumulate, dim3((a.n_pix + SHADE_BLOCK - 1) / SHADE_BLOCK), dim3(SHADE_BLOCK), 0, a.stream, s->dsv, s->pa, a.pixels, a.n_pix, a.n_samples,
                       s->d_gbuffer, s->pix_group, a.film_weight, s->d_filter_weight, s->flat.dist_data.empty() ? 1.0f : s->flat.dist_data[0]);
    LAUNCH_TRY("k_gbuffer_accumulate");
    return SHM_OK;
}
