// k_ao.hip — the ambient occlusion integrator's shade kernel (include/shimmer_hip.h, SHM_INTEGRATOR_AMBIENT_OCCLUSION) and its launcher,
// wf_launch_shade_ao. It takes the place of a path vertex in render_batch's loop (render.hip, ROUTE_AO), which runs once: K1, the scene's closest-hit launch, this
// kernel, the scene's any-hit launch over the shadow queue, K6.
//   k_shade_ao<ZS>   one path slot per lane: shm::ao_sample (shm/ao.h) on the slot's 32-byte hit record — the occlusion ray into pa.shadow_ray, its contribution into
//                    pa.shadow_contrib, the slot onto the shadow queue, L = 0
// It reads no material, texture or light, so it stages no table in LDS. One build serves every scene class and both samplers: the unit sets the disk / cylinder switch
// itself (a hit on one builds its interaction here), instantiates the kernel per sampler, and its name matches none of the Makefile's *_zs / *_dl patterns — no copy of
// it is built that no scene runs.
#define K_QUADRICS true
#include "wavefront.h"
#include "shm/ao.h"

namespace {

template <bool ZS>
__global__ void __launch_bounds__(SHADE2_BLOCK) k_shade_ao(SceneView sv, PathArrays pa, const uint32_t* __restrict__ q_cur, uint32_t* __restrict__ q_shadow, QueueState* qs,
                                                          int cur, ShmRenderParams params, int shadow_parity, float illum_scale) {
    const uint32_t n = qs->n_active[cur];
    const bool uniform = params.ao_uniform_sample != 0;
    const float max_distance = params.ao_max_distance;
    __shared__ uint32_t s_shadow[SHADE_CHUNK];
    __shared__ uint32_t s_cnt, s_base;
    for (uint32_t chunk0 = blockIdx.x * SHADE_CHUNK; chunk0 < n; chunk0 += gridDim.x * SHADE_CHUNK) {
      if (threadIdx.x == 0) s_cnt = 0;
      __syncthreads();
      for (uint32_t k = 0; k < SHADE_CHUNK / SHADE2_BLOCK; ++k) {
        const uint32_t i = chunk0 + k * SHADE2_BLOCK + threadIdx.x;
        bool push_shadow = false;
        uint32_t path = 0;
        if (i < n) {
            path = q_cur[i];
            const float4* hp = reinterpret_cast<const float4*>(pa.hit + path);
            const float4 h0 = hp[0], h1 = hp[1];
            Hit hit;
            hit.prim = __float_as_int(h0.x); hit.t = h0.y; hit.b0 = h0.z; hit.b1 = h0.w; hit.b2 = h1.x; hit.phi = h1.y; hit.inst = __float_as_int(h1.z) - 1;
            pa.L[path] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // an escaped ray, a zero density, an occluded ray: black, and the sample still reaches the film
            if (hit.prim >= 0) {
                const float4* rp = reinterpret_cast<const float4*>(pa.ray + path);
                const float4 r0 = rp[0], r1 = rp[1];
                const V3 ray_d = v3(r0.w, r1.x, r1.y);
                Wavelengths lambda;
                const float4 a = pa.lambda[path], b = pa.lambda_pdf[path];
                lambda.lambda[0] = a.x; lambda.lambda[1] = a.y; lambda.lambda[2] = a.z; lambda.lambda[3] = a.w;
                lambda.pdf[0] = b.x; lambda.pdf[1] = b.y; lambda.pdf[2] = b.z; lambda.pdf[3] = b.w;
                const uint2 rs = pa.rec[path].rng;  // K1 left the sampler directly behind the camera sample
                const uint32_t pix = pa.rec[path].pixel;
                Rng rng = sampler_resume((uint64_t)rs.x | ((uint64_t)rs.y << 32), pix & 0xffffu, pix >> 16, params.seed, sampler_word<ZS>(sv));
                ShmRay sh;
                Spec contrib;
                if (ao_sample(sv, hit, ray_d, rng, lambda, uniform, max_distance, illum_scale, sh, contrib)) {
                    pa.shadow_ray[path] = sh;
                    pa.shadow_contrib[path] = st_spec(contrib);  // added to L by K3 if unoccluded
                    push_shadow = true;
                }
            }
        }
        const uint32_t s1 = queue_push_slot(&s_cnt, push_shadow);
        if (push_shadow) s_shadow[s1] = path;
      }
      __syncthreads();
      if (threadIdx.x == 0) s_base = s_cnt ? atomicAdd(&qs->n_shadow[shadow_parity], s_cnt) : 0u;
      __syncthreads();
      for (uint32_t j = threadIdx.x; j < s_cnt; j += SHADE2_BLOCK) q_shadow[s_base + j] = s_shadow[j];
      __syncthreads();
    }
}

}  // namespace

int wf_launch_shade_ao(ShmScene* s, const ShadeArgs& a, bool zs) {
    const dim3 grid(a.blocks), block(SHADE2_BLOCK);
    if (zs) hipLaunchKernelGGL(k_shade_ao<true>, grid, block, 0, a.stream, s->dsv, s->pa, s->d_q_active[a.cur], s->d_q_shadow, s->d_qs, a.cur, a.params, a.shadow_parity, s->ao_illum_scale);
    else hipLaunchKernelGGL(k_shade_ao<false>, grid, block, 0, a.stream, s->dsv, s->pa, s->d_q_active[a.cur], s->d_q_shadow, s->d_qs, a.cur, a.params, a.shadow_parity, s->ao_illum_scale);
    LAUNCH_TRY("k_shade_ao");
    return SHM_OK;
}
